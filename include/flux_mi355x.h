/*
 * flux_mi355x.h — C-ABI of the MI355X-native FLUX.1 denoise path (libflux_mi355x.so).
 *
 * This is the drop-in boundary for the hot path of EricLBuehler/diffusion-rs
 * (SURVEY.md §8b).  Everything here is `extern "C"`, plain pointers and sizes, no torch /
 * candle types.  A Rust `extern "C"` block (or cgo / ctypes) binds it 1:1; INTEGRATION.md
 * shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - Every function returning `int` returns FMI_OK (0) or a negative fmi_status; the
 *     message is available from fmi_last_error() (thread-local).  The reference's only
 *     native library (diffusion_rs_backend/kernels/bitsandbytes/dequant.cu:172-232) has
 *     void returns and no error channel; the `dequantize_*` entry points below keep that
 *     exact signature so the reference's ffi.rs binds them unchanged.
 *   - All tensors are row-major, contiguous unless a leading dimension is given.
 *   - Data pointers are DEVICE pointers borrowed for the call unless the parameter name
 *     ends in `_host` or the doc says "host or device" (those go through
 *     hipMemcpyDefault).  The caller owns every output buffer (same ownership rule as
 *     the reference's CustomOp::cuda_fwd call sites, bitsandbytes/op.rs:204-228).
 *   - `stream` is a hipStream_t passed as void*; NULL = the null stream.  All compute is
 *     asynchronous on that stream unless stated.
 *   - Not thread-safe per handle (the reference serialises on a Mutex too,
 *     diffusion_rs_core/src/pipelines/mod.rs:110-113); distinct handles are independent.
 */
#ifndef FLUX_MI355X_H
#define FLUX_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared here are exported. */
#pragma GCC visibility push(default)

/* 4 (round 4): + fmi_build_id, fmi_comm_probe, fmi_flux_set_attention_kernel; fmi_flux_set_modulation_gemm accepts 2; fmi_set_attention_kernel accepts 5.
 * 5 (round 5): + the caller-owned-workspace forms fmi_sdpa_bf16_ws / fmi_sdpa_fp8qk_ws / fmi_linear_fp8_ws / fmi_linear_i8_ws and their size queries;
 *   fmi_sdpa_* / fmi_linear_fp8 / fmi_linear_i8 no longer synchronise the stream or call hipMalloc; + fmi_quantize_rows_i8_asym, fmi_rowsum_i8,
 *   fmi_gemm_i8_asym (the int8 mode's post-GELU operand form); fmi_flux_set_quant_dense_cache accepts -1 (default: by memory) and 3.
 *   + fmi_sdpa_fp8 / fmi_sdpa_fp8_ws (e4m3 P and V as well; op-level only: fmi_flux_set_fp8_attention still accepts 0..2).
 * 6 (round 6): + fmi_release_scratch; + the small f32 seams fmi_timestep_embedding, fmi_rope_table, fmi_rmsnorm_rope; + fmi_flux_calibrate_int8
 *   (per-channel smoothing of the int8 mode from a calibration; fmi_flux_quantize_int8 without one is unchanged).  The op-level entries that use
 *   the library's per-stream scratch (fmi_sdpa_*, fmi_linear_fp8 / _i8, fmi_groupnorm_nhwc) now enqueue their kernels under one lock: host threads
 *   may share a stream.  Later additions under the same number: fmi_flux_get_tensor and the LoRA adapter calls fmi_flux_lora_*.
 *   Then, still 6: image to image and inpainting — fmi_preprocess_u8, fmi_latent_mask, fmi_encode_latents, fmi_scale_noise, fmi_flux_denoise_inpaint.
 *   Then, still 6: reference-image (FLUX.1 Kontext) conditioning — fmi_flux_context, fmi_flux_forward_context, fmi_flux_denoise_context, fmi_latent_ids.
 *   Then, still 6: the GEMM launcher's test seams — fmi_gemm_desc, fmi_gemm_group, fmi_splitk_resid_gate, fmi_set_gemm_kernel.
 *   Then, still 6: the GEMM tile heights — fmi_set_gemm_rows, fmi_gemm_tile_rows.
 *   Then, still 6: the first-block step cache of the denoise loop — fmi_flux_step_cache, fmi_flux_denoise_cached, fmi_flux_step_cache_bytes.
 *   Then, still 6: true classifier-free guidance (negative prompts) in the denoise loop — fmi_flux_true_cfg, fmi_flux_denoise_cfg, fmi_cfg_euler_step.
 *   Then, still 6: channel-concatenated conditioning (FLUX.1 Fill / Canny / Depth) — fmi_flux_create_cond, fmi_flux_cond_channels, fmi_flux_control,
 *   fmi_flux_forward_control, fmi_flux_denoise_control, fmi_cast_cols_bf16, fmi_mask_image, fmi_fill_condition.
 *   Then, still 6: the denoise loop's options in one struct — fmi_flux_denoise_options, fmi_flux_denoise_with; the six fmi_flux_denoise* entries remain.
 *   Then, still 6: GGUF transformers (ggml block formats) — fmi_gguf_block_info, fmi_gguf_dequantize, fmi_flux_set_linear_gguf.
 *   Then, still 6: FLUX IP-Adapters (image prompts) — fmi_ip_adapter_*, fmi_flux_ip, fmi_flux_forward_ip, fmi_flux_denoise_ip, fmi_ip_attention.
 *   Then, still 6: the CLIP vision encoder (an image prompt from a picture) — fmi_resize_bicubic_u8, fmi_clip_preprocess_u8, fmi_clip_vision_*.
 *   Then, still 6: FLUX.1 Redux (image variation: a SigLIP vision tower and the Redux embedder) — fmi_siglip_vision_*, fmi_redux_*.
 *   Then, still 6: single-file fp8 checkpoints (OCP e4m3fn / e5m2 weights resident as codes) — fmi_f8_dequantize, fmi_flux_set_linear_f8.
 *   Then, still 6: second-order solvers in the denoise loop (Heun, DPM-Solver++ 2M) — fmi_flux_solver, fmi_flux_denoise_solver, fmi_flux_solver_bytes,
 *                  fmi_heun_predict, fmi_heun_correct, fmi_dpmpp_2m_step, fmi_dpmpp_2m_coefficients.
 * Additions only: a host bound against version 3 keeps working. */
#define FMI_ABI_VERSION 6

typedef enum fmi_status {
  FMI_OK = 0,
  FMI_ERR_INVALID = -1,     /* bad argument / shape / unknown tensor name */
  FMI_ERR_HIP = -2,         /* a HIP runtime call failed */
  FMI_ERR_STATE = -3,       /* missing weights, wrong call order */
  FMI_ERR_UNSUPPORTED = -4, /* valid request this build does not implement */
  FMI_ERR_NOMEM = -5
} fmi_status;

/* Element types of tensors crossing the boundary (host side of set_tensor, or device
 * activations).  NF4/FP4/INT8 are the bitsandbytes storage types of
 * diffusion_rs_backend/src/bitsandbytes/mod.rs:26-31. */
typedef enum fmi_dtype {
  FMI_F32 = 0,
  FMI_F16 = 1,
  FMI_BF16 = 2,
  FMI_U8 = 3,
  FMI_I8 = 4
} fmi_dtype;

/* Mirrors diffusion_rs_core::ModelDType (util/auto_dtype.rs) — the compute dtype of the
 * DiT/VAE weights and activations.  This build computes in BF16 on MFMA with f32
 * accumulation; Auto resolves to BF16.  F16/F32 are rejected with FMI_ERR_UNSUPPORTED. */
typedef enum fmi_model_dtype { FMI_MODEL_AUTO = 0, FMI_MODEL_BF16 = 1, FMI_MODEL_F16 = 2, FMI_MODEL_F32 = 3 } fmi_model_dtype;

const char* fmi_last_error(void);
int fmi_abi_version(void);
/* Select the HIP device for this thread (hipSetDevice) and warm the runtime. */
int fmi_init(int device_ordinal);
/* Device / build info as a JSON string (static storage, valid until next call); includes "build_id" and the count of fp8-QK^T
 * attention launches that fell back from the one-wave stream to the 8-wave kernel ("fp8_attention_fallbacks"). */
const char* fmi_device_info(void);
/* Source identity of this binary: the first 16 hex digits of sha256 over every file of diffusion-rs_amd/csrc/, include/flux_mi355x.h and the Makefile
 * (sorted by path, concatenated) at build time.  __graft_entry__.build() recomputes it from the tree and rebuilds on a mismatch,
 * so a stale prebuilt .so cannot stand in for the sources next to it. */
const char* fmi_build_id(void);
/* 1 = this is the TEST build (libflux_mi355x_alt.so, `make alt`: compiled with -DFMI_ALT_KERNELS=1), which carries the superseded kernels as well —
 * attention kernels 0, 2, 3, 4 of fmi_set_attention_kernel, the dense 4-wave GEMM (FMI_GEMM_W4=1) — for the bit-identity cross-checks of tests/.
 * The product library returns 0, carries kernels 5 and 1, and answers a request for another with FMI_ERR_UNSUPPORTED. */
int fmi_has_alt_kernels(void);

/* ------------------------------------------------------------------------------------
 * FLUX DiT — replaces diffusion_rs_core::models::flux::Flux (model.rs:709-838)
 * ---------------------------------------------------------------------------------- */

/* Mirrors `Config` (model.rs:21-31) + the model constants (model.rs:16-19).  hidden_size
 * must be num_attention_heads*128 (pe_dim = sum(axes_dim) = 128); mlp_ratio is fixed 4. */
typedef struct fmi_flux_config {
  int in_channels;           /* 64 */
  int pooled_projection_dim; /* 768 */
  int joint_attention_dim;   /* 4096 */
  int num_attention_heads;   /* 24 */
  int num_layers;            /* 19 double-stream blocks */
  int num_single_layers;     /* 38 single-stream blocks */
  int guidance_embeds;       /* 1 = dev, 0 = schnell */
  int axes_dim[3];           /* {16,56,56} */
  int theta;                 /* 10000 */
} fmi_flux_config;

typedef struct fmi_flux fmi_flux; /* opaque */

/* Fill `cfg` with the public FLUX.1 config (dev if guidance_embeds else schnell). */
void fmi_flux_default_config(fmi_flux_config* cfg, int guidance_embeds);

/* Allocate the model: one bf16 weight arena in HBM sized from cfg (23.8 GB for FLUX.1),
 * zero-initialised.  == Flux::new (model.rs:722-787) minus the tensor reads. */
int fmi_flux_create(const fmi_flux_config* cfg, fmi_model_dtype dtype, fmi_flux** out);
/* The same for a channel-conditioned checkpoint (FLUX.1 Canny-dev / Depth-dev: cond_channels 64, Fill-dev: 320): x_embedder is
 * (hidden, in_channels + cond_channels); cfg->in_channels keeps meaning the width of the state, of pred_out and of proj_out's rows (diffusers' out_channels).
 * cond_channels >= 0, a multiple of 64, in_channels + cond_channels <= 512, else FMI_ERR_INVALID.  fmi_flux_create(cfg, ..) is fmi_flux_create_cond(cfg, 0, ..). */
int fmi_flux_create_cond(const fmi_flux_config* cfg, int cond_channels, fmi_model_dtype dtype, fmi_flux** out);
int fmi_flux_cond_channels(const fmi_flux*);
void fmi_flux_destroy(fmi_flux*);

/* Provide one tensor by its diffusers name, exactly the names VarBuilder looks up in
 * Flux::new (model.rs:165-772), e.g.
 *   "x_embedder.weight", "context_embedder.bias",
 *   "time_text_embed.timestep_embedder.linear_1.weight",
 *   "transformer_blocks.3.attn.to_q.weight", "transformer_blocks.3.norm1.linear.bias",
 *   "transformer_blocks.3.attn.norm_added_k.weight", "transformer_blocks.3.ff.net.0.proj.weight",
 *   "single_transformer_blocks.7.proj_mlp.weight", "single_transformer_blocks.7.attn.norm_q.weight",
 *   "norm_out.linear.weight", "proj_out.bias".
 * `data` may be a host or device pointer; `dtype` F32/F16/BF16 is converted to bf16 (RNE)
 * and placed into the fused layouts the kernels read (q|k|v|proj_mlp rows concatenated,
 * all modulation linears in one matrix).  Shape is checked against cfg. Synchronous. */
int fmi_flux_set_tensor(fmi_flux*, const char* name, const void* data, fmi_dtype dtype,
                        const int64_t* shape, int rank);

/* bitsandbytes 4-bit weight for linear `prefix` (e.g. "transformer_blocks.0.attn.to_q"):
 * packed u8 (out*in/2), f32 absmax (out*in/blocksize), quant type 1=fp4 2=nf4
 * (bitsandbytes/mod.rs:137-222; nested absmax must be resolved by the caller with
 * fmi_dequantize_blockwise first, as BnbLinear::dequantize_4bit does, mod.rs:230-239).
 * The layer then runs through the fused dequant-GEMM. host or device pointers. */
int fmi_flux_set_linear_bnb4(fmi_flux*, const char* prefix, const uint8_t* packed,
                             const float* absmax, int blocksize, int quant_type,
                             int out_features, int in_features);

/* Number of tensors still missing (never set); names via fmi_flux_missing_name(i). */
/* LLM.int8 linear (BnbLinear::Int8, bitsandbytes/mod.rs:104-134,293-300): weight int8 (out,in) row
 * major + SCB f32 (out); effective weight = w * SCB[row] / 127 (dequant.cu:205-214), expanded to
 * bf16 inside the layer's GEMM (small launches) or right before it (see fmi_flux_set_quant_dense_cache).
 * Same prefix rules as fmi_flux_set_linear_bnb4. */
int fmi_flux_set_linear_int8(fmi_flux*, const char* prefix, const int8_t* weight, const float* scb, int out_features, int in_features);
/* Quantised block / modulation linears (BnbLinear::forward = dequantize, then matmul: bitsandbytes/mod.rs:293-312) — where the expanded
 * weights live.  Launches of up to 383 rows (nf4 / fp4) or 256 rows (LLM.int8) always multiply straight from the packed codes with the
 * fused dequant-GEMM (the expansion is an LDS stage of the GEMM; the packed read wins there).  For larger launches the dense kernel on
 * expanded weights is measured faster, and `mode` says where those come from:
 *   -1 (default) by memory: 3 if, when the first such launch comes, the device has at least twice the dense block arena free (it does
 *      on a 288 GB part: an nf4 FLUX.1-dev then holds 7 GB of codes + 16 GB of expanded block matrices and runs at bf16 speed), else 0;
 *    0 packed only: the matrix is expanded per call into a reusable scratch (2 x the largest fused matrix); ~7 GB resident for FLUX.1-dev;
 *    1 every quantised matrix, the 6.5 GB modulation matrix included, is expanded ONCE into its slot of the bf16 arenas (+23 GB);
 *    2 every launch on the fused kernels;
 *    3 as 0, but a matrix that 0 would expand per call is expanded once into its dense slot (small launches stay on the codes).
 * All of them produce the same bits. */
int fmi_flux_set_quant_dense_cache(fmi_flux*, int mode);

/* ggml block formats (llama.cpp's .gguf files).  Supported ggml type ids: Q4_0 2, Q4_1 3, Q5_0 6, Q5_1 7, Q8_0 8 (32 weights per block of
 * 18 / 20 / 22 / 24 / 34 bytes) and Q4_K 12, Q5_K 13, Q6_K 14 (256 weights per block of 144 / 176 / 210 bytes).  Every other id — Q2_K, Q3_K,
 * Q8_1, Q8_K, the IQ family — is refused by name with FMI_ERR_UNSUPPORTED; F32 / F16 / BF16 tensors (0 / 1 / 30) are plain and go through
 * fmi_flux_set_tensor.  block_elems / block_bytes may be NULL. */
int fmi_gguf_block_info(int ggml_type, int* block_elems, int* block_bytes);
/* n_elems weights of `blocks` (DEVICE pointer, 2-byte aligned, n_elems / block_elems consecutive blocks) -> out (DEVICE pointer, BF16 or F32).
 * Values are those of ggml's dequantize_row_* evaluated in f32 with every multiply and add rounded on its own, then one RNE rounding to bf16:
 * bit-equal to a scalar float32 restatement.  FMI_ERR_INVALID: n_elems not a multiple of the block's elements, another out_dtype, a null or
 * misaligned pointer.  Indexes in 64 bits. */
int fmi_gguf_dequantize(int ggml_type, const void* blocks, int64_t n_elems, void* out, fmi_dtype out_dtype, void* stream);
/* A Linear given as ggml blocks: row-major, each of the out_features rows is in_features / block_elems blocks (in_features % block_elems != 0:
 * FMI_ERR_INVALID).  Host or device pointer.  Same prefix rules and refusals as fmi_flux_set_linear_bnb4 (unknown prefix, shape mismatch: INVALID; a
 * ControlNet handle: UNSUPPORTED; a model in an 8-bit mode, a weight with LoRA adapters merged: STATE).
 *   - embedders and the final layer are expanded into their bf16 slot at load;
 *   - modulation linears (norm1.linear, norm1_context.linear, norm.linear, norm_out.linear) are expanded at load into the fused modulation matrix,
 *     in every mode: that matrix has 3.2e9 weights in FLUX.1-dev and never goes through the per-call scratch, so a packed-only GGUF FLUX.1-dev
 *     holds the blocks of the block linears PLUS 6.5 GB of dense modulation weights;
 *   - parts of a fused block matrix keep their packed blocks resident, in storage the matrix owns.  If all parts of a matrix have the same ggml
 *     type, only the blocks are resident; a mixture of types, or of GGUF and dense / bitsandbytes parts, is expanded into the dense arena once.
 * There is no fused dequant-GEMM for these formats: at EVERY row count the matrix is expanded, once into its dense slot or per call into the
 * scratch, as fmi_flux_set_quant_dense_cache says: -1 by free memory, 0 per call, 1 and 3 once, 2 per call as 0 (there is no fused kernel for 2
 * to select).  Every mode computes the bits of a bf16 model loaded with the dequantised weights.  fmi_flux_get_tensor and fmi_flux_lora_add on
 * a Linear resident as blocks, fmi_flux_quantize_fp8 / _int8 / fmi_flux_calibrate_int8 and fmi_flux_state_export on such a model return
 * FMI_ERR_UNSUPPORTED, as for nf4.  fmi_flux_size_in_bytes counts the blocks.
 * Not verified: no file written by ggml itself was available — conformance rests on the reference's to_float code and on literal known answers; the
 * FLUX.1-dev-size model was run and timed on generated blocks (profiles/gguf.txt), its values were checked at the small test configuration only; one
 * expansion past 2^31 weights is checked at the op level on a periodic input, none inside the model (the modulation matrix arrives as 77 Linears of at
 * most 5.7e7 weights each). */
int fmi_flux_set_linear_gguf(fmi_flux*, const char* prefix, int ggml_type, const void* data, int out_features, int in_features);

/* 8-bit float weights (single-file .safetensors checkpoints whose tensors carry the dtypes F8_E4M3 / F8_E5M2).  format: 1 = OCP e4m3fn (no
 * infinities; 0x7f / 0xff are NaN; largest finite value 448), 2 = OCP e5m2 (IEEE-like; largest finite value 57344).
 * n_elems codes of `codes` (DEVICE pointer, ANY byte alignment) -> out (DEVICE pointer aligned to its element size, BF16 or F32).  The semantics are
 * this library's own decision:
 *   y = f32(code)            exact: every code of either format is an f32 value
 *   y = y * scale            ONE f32 multiply, rounded to nearest even (__fmul_rn)
 *   BF16 output: then ONE RNE rounding to bf16
 * so scale == 1.0f gives the code's value exactly, and the result is bit-equal to (codes as torch.float8_*).float() * scale [.to(bfloat16)] for every
 * non-NaN code.  A NaN code gives a NaN of unspecified payload; e5m2's infinities stay infinities.  Results that are bf16 / f32 subnormals are outside
 * the contract (keep scale within [2^-40, 2^40]).  FMI_ERR_INVALID: another format, another out_dtype, scale not finite or not > 0, n_elems < 0, a null
 * pointer with n_elems > 0, out not aligned to its element size — all refused before any launch.  n_elems == 0 returns 0.  Indexes in 64 bits. */
int fmi_f8_dequantize(int format, const void* codes, int64_t n_elems, float scale, void* out, fmi_dtype out_dtype, void* stream);
/* A Linear given as 8-bit float codes: row-major (out_features, in_features), one code per weight, and ONE scale for the Linear (1.0f for a plain
 * cast; a "scaled fp8" file's scale_weight): its values are those of fmi_f8_dequantize.  Host or device pointer.  Same prefix rules and refusals as
 * fmi_flux_set_linear_gguf (unknown prefix, shape mismatch, another format, scale not finite or not > 0: INVALID; a ControlNet handle: UNSUPPORTED; a
 * model in an 8-bit mode, a weight with LoRA adapters merged: STATE).
 *   - embedders and the final layer are expanded into their bf16 slot at load;
 *   - modulation linears (norm1.linear, norm1_context.linear, norm.linear, norm_out.linear) are expanded at load into the fused modulation matrix,
 *     in every mode, as for GGUF: an fp8 FLUX.1-dev holds the codes of the block linears (11.9 GB) PLUS 6.5 GB of dense modulation weights;
 *   - parts of a fused block matrix keep their codes resident, in storage the matrix owns, each part with its own scale.  If all parts of a matrix
 *     have the same format, only the codes are resident (the parts' scales may differ: the expansion runs per part); a mixture — e4m3 with e5m2, or
 *     fp8 with dense, GGUF or bitsandbytes parts — is expanded into the dense arena once.
 * There is no fused dequant-GEMM for these codes (feeding them to the e4m3 GEMM mode is another recipe with other values): at EVERY row count the
 * matrix is expanded, once into its dense slot or per call into the scratch, as fmi_flux_set_quant_dense_cache says: -1 by free memory, 0 per call,
 * 1 and 3 once, 2 per call as 0.  Every mode computes the bits of a bf16 model loaded with the dequantised weights.  fmi_flux_get_tensor and
 * fmi_flux_lora_add on a Linear resident as codes, fmi_flux_quantize_fp8 / _int8 / fmi_flux_calibrate_int8 and fmi_flux_state_export on such a model
 * return FMI_ERR_UNSUPPORTED, as for GGUF.  fmi_flux_size_in_bytes counts the codes.
 * Not verified: no fp8 checkpoint written by another program was available — the "scaled fp8" naming (scale_weight, scale_input, scaled_fp8) is
 * ComfyUI's as remembered; the FLUX.1-dev-size model was run and timed on generated codes, its values were checked at the small test configuration
 * only. */
int fmi_flux_set_linear_f8(fmi_flux*, const char* prefix, int format, const void* codes, float scale, int out_features, int in_features);

/* Read back the CURRENT value of any tensor fmi_flux_set_tensor accepts (same names, same shapes; `shape` / `rank` are checked): the row range of
 * the fused matrix it lives in, bf16 converted exactly to `dtype` F32 or BF16.  `out` may be a host or device pointer.  Synchronises the device.
 * FMI_ERR_STATE for a tensor that was never set; FMI_ERR_UNSUPPORTED for a Linear that is resident only as packed nf4 / fp4 / LLM.int8 codes.
 * With LoRA adapters loaded it returns the merged weight. */
int fmi_flux_get_tensor(fmi_flux*, const char* name, void* out, fmi_dtype dtype, const int64_t* shape, int rank);

/* LoRA adapters, MERGED into the resident bf16 weights (no runtime low-rank path: the denoise loop runs the same GEMMs at the same speed).
 * For a Linear with loaded weight W0 (out, in) and adapters a = 1..n, each holding A_a (r_a, in), B_a (out, r_a), scale_a (= alpha / r) and a
 * user weight_a (default 1), the resident weight is
 *     W = bf16_rne( W0 + sum_a weight_a * scale_a * (B_a A_a) )
 * with the sum taken over the adapters in lexicographic order of their names.  The factors are kept as f32, converted exactly from F32 / F16 / BF16,
 * and never rounded to bf16; products and sums run in f64 (products of f32 values are exact there) and there is ONE rounding at the end, so every
 * element of W is the correctly rounded value of the expression — also where W0 and the update cancel, which f32 sums cannot guarantee.  W is always recomputed from a pristine copy of W0 that
 * the library keeps while a Linear has an active adapter (weight != 0) — never patched incrementally — so stacking, reweighting and switching do
 * not depend on the history of calls, and removing the adapters restores the loaded weights bit for bit.  Biases are never touched.
 *   fmi_flux_lora_add        one (A, B) pair of adapter `adapter` for the Linear `prefix` (as in fmi_flux_set_linear_bnb4, e.g.
 *                            "transformer_blocks.0.attn.to_k"); host or device pointers; a pair the adapter already holds for that Linear is replaced.
 *   fmi_flux_lora_set_weight the user weight of an adapter; 0 switches it off (its factors stay loaded).
 *   fmi_flux_lora_remove     drop an adapter (NULL: every adapter).
 *   fmi_flux_lora_count / fmi_flux_lora_name(i): the loaded adapters in lexicographic order (the pointer is valid until that adapter is removed).
 * The three mutating calls are load-time operations: each synchronises the device on entry (which orders it against evaluations on any stream),
 * re-merges the affected Linears and completes before it returns.  They validate first and leave every weight and adapter untouched on error:
 * FMI_ERR_STATE once the model is in an 8-bit mode (adapters go in BEFORE fmi_flux_quantize_fp8 / _int8, which then quantise the merged weights) or
 * while tensors are missing; FMI_ERR_UNSUPPORTED for a Linear resident as nf4 / fp4 / LLM.int8 codes (merging into packed codes is out of scope);
 * FMI_ERR_INVALID for an unknown Linear or adapter, rank < 1, a null pointer, a non-finite scale or weight.  While a weight has adapters,
 * fmi_flux_set_tensor, fmi_flux_set_linear_bnb4 and fmi_flux_set_linear_int8 on it return FMI_ERR_STATE (remove the adapters first).  Quantising to
 * 8 bits freezes the adapters and releases their factors and the pristine copies; the names stay listed.  The pristine copies are private allocations, not part of
 * fmi_flux_state_*: the flat state carries the effective (merged) weights. */
int fmi_flux_lora_add(fmi_flux*, const char* adapter, const char* prefix, const void* A, const void* B, fmi_dtype dtype, int rank, float scale);
int fmi_flux_lora_set_weight(fmi_flux*, const char* adapter, float weight);
int fmi_flux_lora_remove(fmi_flux*, const char* adapter);
int fmi_flux_lora_count(const fmi_flux*);
const char* fmi_flux_lora_name(const fmi_flux*, int i);

/* LyCORIS and DoRA adapters: the other parametrisations FLUX adapters are written in, merged like LoRA.  For a Linear with loaded weight W0 (out, in)
 *     W = bf16_rne( W0 + sum_a weight_a * Delta_a ),   adapters in lexicographic name order, ONE rounding, always from the pristine copy of W0,
 * and Delta depends on the term's kind (which fields of fmi_adapter_term are read is listed per kind; every tensor has the one `dtype`, F32 / F16 / BF16,
 * and is row-major; pointers may be host or device memory for fmi_flux_lora_add_term and are device memory for fmi_adapter_merge):
 *   FMI_ADAPTER_LORA  Delta = scale * B A.                       factor[0] = A (r, in), factor[1] = B (out, r).
 *   FMI_ADAPTER_LOHA  Delta = scale * (w1_a w1_b) (.) (w2_a w2_b), (.) element-wise.
 *                     factor[0] = hada_w1_a (out, r), factor[1] = hada_w1_b (r, in), factor[2] = hada_w2_a (out, r), factor[3] = hada_w2_b (r, in).
 *   FMI_ADAPTER_LOKR  Delta[i, j] = scale * w1[(i + row_offset) / c, j / d] * w2[(i + row_offset) % c, j % d], w1 (a, b), w2 (c, d), b * d == in,
 *                     row_offset + out <= a * c.  factor[0] = lokr_w1 (a, b) with factor[1] NULL, or factor[0] = lokr_w1_a (a, r1) and
 *                     factor[1] = lokr_w1_b (r1, b); factor[2] / factor[3] the same for w2.  row_offset is the first row of this Linear inside a
 *                     fused module the factors describe (0 otherwise).  A full difference (`.diff`) is w1 = [[1]], w2 = the (out, in) tensor.
 *   FMI_ADAPTER_DORA  with V = W0 + scale * B A and n_i = ||V[i, :]||_2:  Delta = m (.) V / n - W0 (row i scaled by m_i / n_i).
 *                     factor[0] = A, factor[1] = B as for LORA, magnitude = m (out values).  The norm uses the pristine W0 and this term alone; it is
 *                     computed once when the term is added.  A row with n_i zero or not finite is FMI_ERR_INVALID.
 * factor_rows / factor_cols give the shape of each non-NULL factor.  `scale` is alpha / r (the file reader's rule; the library multiplies by it as given).
 * Numerics: factors resident as f32 (exact conversions), every product, sum, square root and division in f64 (DoRA's row sum of squares by a fixed
 * reduction tree: the same bits from run to run), W0 plus all terms rounded once (f64 -> f32 to odd -> bf16 to nearest-even).  Only a Linear whose
 * active terms are all plain LoRA keeps the claim "correctly rounded value of the exact expression" (it runs exactly the LoRA path above); the other
 * kinds multiply or divide rounded f64 values, so an element is the one rounding of an f64 evaluation of the formula.
 * The formulas are written down from memory of PEFT, LyCORIS and ComfyUI; no file or output of those libraries was compared.
 *   fmi_flux_lora_add_term   the contract of fmi_flux_lora_add (which is this call with kind LORA): replaces the adapter's term on that Linear, a new
 *                            adapter starts at weight 1, validates first and changes nothing on error.  Further FMI_ERR_INVALID cases: an unknown kind,
 *                            factor shapes that disagree with the Linear or with each other (b * d != in, row_offset + out > a * c, unequal LoHa
 *                            ranks, a missing factor), a DoRA row norm of zero (the message names the Linear).
 *   fmi_adapter_merge        the op-level entry the model's re-merge runs through: w (rows, K) bf16 <- W0 (rows, K) bf16 plus the terms in the ORDER GIVEN,
 *                            term i at weights[i].  Device pointers; K % 8 == 0, 16-byte aligned w0 / w; completes before it returns.
 * fmi_flux_lora_set_weight / _remove / _count / _name cover every kind, and everything said above about adapted weights (set_tensor, the quantised
 * setters, state_adopt, the 8-bit freeze, ControlNets, packed Linears) holds for every kind. */
typedef enum { FMI_ADAPTER_LORA = 0, FMI_ADAPTER_LOHA = 1, FMI_ADAPTER_LOKR = 2, FMI_ADAPTER_DORA = 3 } fmi_adapter_kind;
typedef struct fmi_adapter_term {
  int kind;                /* fmi_adapter_kind */
  int dtype;               /* fmi_dtype of every tensor of the term */
  float scale;
  int row_offset;          /* LOKR */
  const void* factor[4];
  int factor_rows[4];
  int factor_cols[4];
  const void* magnitude;   /* DORA: out values */
} fmi_adapter_term;
int fmi_flux_lora_add_term(fmi_flux*, const char* adapter, const char* prefix, const fmi_adapter_term* term);
int fmi_adapter_merge(const void* w0_bf16, void* w_bf16, int rows, int K, const fmi_adapter_term* terms, const float* weights, int n_terms, void* stream);
/* Single-image sequence parallelism.  The reference runs one image on one device
 * (pipelines/mod.rs:214-217 "This will need to be updated!"); here the tokens of ONE image are sharded over the
 * world_size ranks of a group: rank r passes ONLY its token shard to fmi_flux_forward / fmi_flux_denoise
 * (txt rows [r*T/N, (r+1)*T/N), img rows [r*S/N, (r+1)*S/N), the matching txt_ids / img_ids rows; B = 1) and gets
 * its shard of the prediction / latents back.  Everything per token runs on the local rows; the joint attention
 * (model.rs:540-552) is made head-local by two all-to-alls per block, which the library asks the caller to run:
 *   a2a(user, send, recv, bytes_per_peer, stream): block p (bytes_per_peer bytes) of `send` goes to rank p, block p
 *   of `recv` comes from rank p; device buffers owned by the library; the exchange must be ordered on `stream`
 *   (hipStream_t) like a kernel launch (RCCL: all_to_all on that stream).  Returns 0 on success.
 * Needs heads % world_size == 0 and equal shards (T, S divisible by world_size); bf16 mode.  world_size 1 (or a
 * null callback) switches it off.  Results are bit-identical to the single-device forward. */
/* Latency mode for small launches (default off).  A residual projection (attention output projection, MLP down projection,
 * single-block linear2) launched on so few rows that it has fewer than 128 tiles of 256 x 256 — the shards of sequence
 * parallelism — is split along K into up to 8 parts of one grouped launch and reduced in a fixed order by a second kernel;
 * and the sequence-parallel attention of few heads walks up to 4 key ranges in parallel workgroups whose partial outputs
 * are merged by their log-sum-exp.  Deterministic, but sums are associated differently from the unsplit launches: results
 * agree to rounding, not bit for bit (which is why it is opt-in).  Per-rank effect: profiles/r02_sp_rank_time.txt. */
int fmi_flux_set_split_k(fmi_flux*, int enable);
typedef int (*fmi_all_to_all_fn)(void* user, const void* send, void* recv, size_t bytes_per_peer, void* stream);
int fmi_flux_set_sequence_parallel(fmi_flux*, int rank, int world_size, fmi_all_to_all_fn a2a, void* user);

/* ------------------------------------------------------------------------------------
 * RCCL communicator (rccl_comm.hip): the collectives of the multi-GPU path behind plain C — the counterpart a host
 * without torch.distributed needs (the reference itself is single-device, pipelines/mod.rs:214-217).  librccl.so.1 is
 * opened with dlopen on first use (FMI_ERR_UNSUPPORTED if absent).  One fmi_comm per process / GPU; rank 0 calls
 * fmi_comm_unique_id and ships the FMI_COMM_ID_BYTES bytes to the other ranks by any host channel; fmi_comm_create is
 * collective (ncclCommInitRank) and binds the comm to the CURRENT device.  All operations are enqueued on `stream`
 * (hipStream_t) like a kernel launch; none synchronises the host.
 *   fmi_comm_all_to_all  has the fmi_all_to_all_fn signature: pass (fmi_comm_all_to_all, comm) to
 *                        fmi_flux_set_sequence_parallel and the two exchanges per block are one ncclAllToAll each.
 *   fmi_comm_broadcast   in place, e.g. on every fmi_flux_state_buffer (weights from rank 0).
 *   fmi_comm_gather      rank r's `bytes` land at recv + r*bytes on root (decoded u8 images to rank 0). */
#define FMI_COMM_ID_BYTES 128
typedef struct fmi_comm fmi_comm;
/* Non-collective: FMI_OK iff librccl is usable and the thread has a current device.  Call it on every rank and agree on the
 * results over the host channel BEFORE fmi_comm_create, which blocks in ncclCommInitRank until every rank has arrived. */
int fmi_comm_probe(void);
int fmi_comm_unique_id(void* id_out /* FMI_COMM_ID_BYTES */);
int fmi_comm_create(const void* id, int rank, int world_size, fmi_comm** out);
void fmi_comm_destroy(fmi_comm*);
int fmi_comm_rank(const fmi_comm*);
int fmi_comm_world_size(const fmi_comm*);
int fmi_comm_stats(const fmi_comm*, unsigned long long* calls, unsigned long long* bytes_sent);
int fmi_comm_all_to_all(void* comm, const void* send, void* recv, size_t bytes_per_peer, void* stream);
int fmi_comm_broadcast(fmi_comm*, void* buf, size_t bytes, int root, void* stream);
int fmi_comm_gather(fmi_comm*, const void* send, void* recv, size_t bytes, int root, void* stream);
/* PROCESS-WIDE test / ablation hooks — fmi_set_bnb4_onewave_min_rows, fmi_set_attention_kernel (below; a model handle can override it for itself: fmi_flux_set_attention_kernel) and the environment
 * variables FMI_GEMM_W4 / FMI_ATT_W4 / FMI_ATT_W16 / FMI_ATT_W32 / FMI_ATT_W16L (0 | 1, read once at load and folded into the initial fmi_set_attention_kernel kind by precedence: W16L (default 1) -> 5, else W32 (0) -> 4, else W16 (1) -> 3, else W4 (1) -> 2, else 1), FMI_TWO_STREAMS=1 (read
 * by fmi_flux_create: the text chain of a double block on an internal second stream — an experiment measured at -0.3 %, same bits, default off) FMI_GEMM_W4_QKV_MIN_N=<n> (read at load, with FMI_GEMM_W4=1: dense q|k|v launches at least n wide on the 4-wave GEMM kernel too — measured 5 % slower in round 4, default never) and FMI_GEMM_BAND=<n> (read at the first GEMM launch: pins the band height of the
 * GEMM tile order, a bijection of the tiles whatever its value) — are shared by every handle and thread of the process: they pick between
 * kernels that produce identical bits (the attention kernels: identical within a family, equal to rounding across, see
 * fmi_set_attention_kernel), so they move time, not results.  Set them before starting work on other threads.
 * Everything that changes results (fp8 / int8 mode and their attention operands, split-K latency mode, the quantised-weight policy, sequence parallelism) is per handle.
 * Rows from which 4-bit GEMMs use the one-wave-per-SIMD fused kernel (default 256): */
int fmi_set_bnb4_onewave_min_rows(int rows);
/* Test hook of the attention kernel's deferred-rescale branch, a BOOLEAN: 0 = rescale the accumulator on every key tile,
 * any other value = the default (rescale only when the running maximum grew by more than 6.0 in log2 units; the kernels are
 * instantiated for these two settings only). */
int fmi_flux_set_attention_rescale_threshold(fmi_flux*, int thr_x16);
/* PER HANDLE: the attention kernel this model uses, in fmi_set_attention_kernel's numbering (0 .. 5; see there), or -1 (default) = follow
 * the process-wide switch.  Two handles of one process can run different kernels; the op-level fmi_sdpa_* entry points have no handle and
 * keep following the process-wide switch. */
int fmi_flux_set_attention_kernel(fmi_flux*, int kind);
/* The weights as flat device buffers — the unit of the multi-GPU broadcast (north star: "RCCL broadcast of
 * weights").  Rank 0 loads a checkpoint, fmi_flux_state_export() fills a small host blob saying which
 * arenas exist and how every fused matrix is stored (pass blob_host = NULL to query *len); the other ranks
 * fmi_flux_state_adopt() it (same arenas allocated, every tensor marked present) and receive the bytes of
 * buffers 0 .. fmi_flux_state_buffer_count()-1 (fmi_flux_state_buffer: device pointer + size, NULL / 0 for
 * an arena this checkpoint does not use).  LLM.int8 matrices are not covered (FMI_ERR_UNSUPPORTED).
 * The reference is single-device (pipelines/mod.rs:214-217). */
int fmi_flux_state_buffer_count(void);
int fmi_flux_state_export(fmi_flux*, uint8_t* blob_host, size_t cap, size_t* len);
int fmi_flux_state_adopt(fmi_flux*, const uint8_t* blob_host, size_t len);
int fmi_flux_state_buffer(fmi_flux*, int index, void** ptr, size_t* bytes);
/* fmi_flux_denoise computes every step's modulation vectors (they depend on t, guidance and y only) before
 * the loop: 1 (default) = one MFMA GEMM (n_steps*B, D) x (n_mod, D)^T with silu(vec) rounded to bf16, the
 * 6.5 GB modulation matrix read once per image, taken when n_steps * B > 4; 0 = f32 GEMV passes of 4 rows (one pass per
 * 4 steps); 2 = the GEMM at any row count (test hook: lets a 2-step run at full size go through the one-GEMM path). */
int fmi_flux_set_modulation_gemm(fmi_flux*, int enable);
/* fp8 inference mode (BASELINE.json configs[4]; the reference has no fp8 path, SURVEY.md §8d — the recipe
 * is this library's own, restated in oracle/flux_oracle.cpp:orc_quantize_rows_fp8).  Call once after all
 * tensors are set: every DiT block Linear (q|k|v, attention out, MLP, single-block linear1/linear2) is
 * quantised from its bf16 values to OCP e4m3 with one f32 scale per output channel; from then on their
 * GEMMs run on v_mfma_f32_32x32x64_f8f6f4 with activations quantised per token by the producing kernel
 * (AdaLN-modulate) or by one row pass (attention output, GELU(MLP)).  Attention, the residual stream,
 * modulation, embedders and the final layer stay bf16/f32.  Not combinable with bnb-quantised linears. */
int fmi_flux_quantize_fp8(fmi_flux*, void* stream);
/* int8 inference mode (round 4; this library's own recipe like the fp8 one, restated in oracle/flux_oracle.cpp: orc_quantize_rows_i8 and
 * lin_blk mode 5).  The same per-row scheme on symmetric int8 codes — scale = absmax / 127 per output channel (weights, once) and per
 * token (activations, by the producing AdaLN-modulate kernel or one row pass), codes = clamp(rint(x * 127 / absmax), -127, 127) — and
 * the GEMMs on v_mfma_i32_32x32x32_i8: the sum over k is an exact int32, converted once and multiplied by scale_a[m] * scale_w[n].
 * Why it exists: an e4m3 operand carries 2.65e-2 rms relative noise whatever the scale granularity (3-bit mantissa), an int8 one
 * 8.5e-3 (uniform steps over a Gaussian row), at the same matrix-pipe rate; with the default mask the full model stays within the
 * tolerance stated for 8-bit modes where the e4m3 mode is a factor three outside it.
 * `linear_mask` says WHICH block linears are quantised (the others keep their bf16 GEMM): FMI_INT8_DEFAULT_MASK = all but the double
 * blocks' MLP, the two linears that carry most of the error per millisecond saved (DESIGN.md 4.3c's table).  Attention, residual
 * stream, modulation, embedders and final layer stay bf16 / f32 — except that, as in the fp8 mode and under the same switch
 * (fmi_flux_set_fp8_attention, default on), the blocks whose q|k|v linear is in the mask hand q and k to the attention as e4m3 with the
 * static scales and QK^T runs on the fp8 MFMA (measured cost: 5.9e-3 alone, 2.40e-2 -> 2.50e-2 with the default mask at 6 + 12 blocks; P, V
 * and the accumulation are unchanged).  Call once after all tensors are set; not combinable with bnb-quantised linears or with
 * fmi_flux_quantize_fp8 (FMI_ERR_STATE). */
#define FMI_Q8_DOUBLE_QKV 1u      /* double blocks: q|k|v of both streams */
#define FMI_Q8_DOUBLE_OUT 2u      /* double blocks: attention output projections */
#define FMI_Q8_DOUBLE_MLP_IN 4u   /* double blocks: MLP linear 1 (+ GELU) */
#define FMI_Q8_DOUBLE_MLP_OUT 8u  /* double blocks: MLP linear 2 */
#define FMI_Q8_SINGLE_LINEAR1 16u /* single blocks: q|k|v|proj_mlp */
#define FMI_Q8_SINGLE_LINEAR2 32u /* single blocks: proj_out over cat(attention, gelu(mlp)) */
#define FMI_INT8_DEFAULT_MASK (FMI_Q8_DOUBLE_QKV | FMI_Q8_DOUBLE_OUT | FMI_Q8_SINGLE_LINEAR1 | FMI_Q8_SINGLE_LINEAR2)
int fmi_flux_quantize_int8(fmi_flux*, unsigned linear_mask, void* stream);
/* Calibration of the SMOOTHED int8 recipe (ABI 6, round 6).  The per-token grid above is sized by a row's largest element; real DiT activations have a
 * few hidden channels two orders of magnitude above the rest (their AdaLN (1 + scale) is 30-100 at every step), which would leave the other ~3 000
 * channels of the row a handful of levels.  fmi_flux_calibrate_int8(m, 1) — bf16 mode, all tensors set — zeroes a set of statistics; from then on every
 * fmi_flux_forward / fmi_flux_denoise evaluation ALSO folds max |x[:, k]| of each block linear's input into them (the results are unchanged; a handful of
 * evaluations at timesteps across the schedule is enough: the outlier channels are the same at every step).  The next fmi_flux_quantize_int8 consumes them:
 *   A[k] = amax_x[k] / median(amax_x),  W[k] = amax_W[k] / median(amax_W)      (amax_W[k] = max_n |W[n, k]|)
 *   s[k] = min(sqrt(ra / rw), 2^10),  ra = A - 1 if A > 2 else 1,  rw = W / (1 - W) if W < 1/2 (W floored at 1/64) else 1      (continuous; ~sqrt(A / W) for a genuine outlier)
 *   — SmoothQuant with alpha = 1/2 for the channels that stand out of the median ONLY: every other channel has s = 1 exactly, so a checkpoint without outlier channels
 *   quantises as without calibration, and a short calibration cannot create outliers of its own
 *   weight codes from W[n, k] * s[k], activation rows from x[m, k] * (1 / s[k]) — both in f32 before the per-row recipe; x W^T is unchanged in exact arithmetic
 * (the 1 / s multiply rides in the AdaLN-modulate kernel or the row pass that quantises the activation; the GEMMs are untouched) and ends the recording.
 * fmi_flux_calibrate_int8(m, 0) drops the statistics.  Without a calibration fmi_flux_quantize_int8 is bit for bit the unsmoothed recipe; the e4m3 mode
 * never smooths (a floating-point grid has no use for it).  Oracle: orc_flux_set_calibration (flux_oracle.cpp, lin_blk mode 5). */
int fmi_flux_calibrate_int8(fmi_flux*, int enable);
/* fp8 and int8 modes, attention operands: 1 (default) = q and k leave the fused QKV epilogue as e4m3 with static per-block
 * scales 448 / (sqrt(128) * max|QkNorm weight|) (no element of a normalised, rotated head vector can exceed them) and
 * QK^T runs on the fp8 MFMA; P and V stay bf16.  Applies when both streams of a block take the fused epilogue (token
 * counts and offsets multiples of 16, model width a multiple of 256), else that block uses bf16 operands.  0 = always bf16.
 * 2 = the same in EVERY mode, the bf16 block linears included (opt-in; the static scales are read from the QkNorm weights at the next
 * evaluation; blocks whose q|k|v linear is bnb-quantised keep bf16 operands; not with sequence parallelism).  A reduced-precision
 * attention operand is not the reference's semantics, which is why it is never the default outside the 8-bit modes — measured on
 * FLUX.1-dev in full at the headline size it moves the result less than the bf16 path's own distance to f32. */
int fmi_flux_set_fp8_attention(fmi_flux*, int enable);
int fmi_flux_missing_count(const fmi_flux*);
const char* fmi_flux_missing_name(const fmi_flux*, int i);
/* Bytes of HBM held by the model (weights + current workspace). */
size_t fmi_flux_size_in_bytes(const fmi_flux*);

/* One denoise-model evaluation == Flux::forward (model.rs:790-833).
 *   img      (B,S,in_channels)         img_dtype  F32|BF16
 *   img_ids  (B,S,3)  f32              (row/col positions; reference builds them in
 *                                        State::new, flux/sampling.rs:134-148)
 *   txt      (B,T,joint_attention_dim) txt_dtype  F32|BF16
 *   txt_ids  (B,T,3)  f32
 *   timesteps(B) f32,  y (B,pooled_projection_dim) y_dtype F32|BF16,
 *   guidance (B) f32 or NULL (must be non-NULL iff cfg.guidance_embeds, as model.rs:814-819)
 *   pred_out (B,S,in_channels) f32
 * Only batch element 0's ids are used to build the RoPE table when ids are identical
 * across the batch (they always are in the reference, sampling.rs:147-150); set
 * `ids_per_sample`=1 to build one table per sample. */
typedef struct fmi_flux_inputs {
  const void* img;      fmi_dtype img_dtype;
  const float* img_ids;
  const void* txt;      fmi_dtype txt_dtype;
  const float* txt_ids;
  const float* timesteps;
  const void* y;        fmi_dtype y_dtype;
  const float* guidance;
  int B, S, T;
  int ids_per_sample;
} fmi_flux_inputs;

int fmi_flux_forward(fmi_flux*, const fmi_flux_inputs* in, float* pred_out, void* stream);

/* ---- What an evaluation can be conditioned on.  Each block below gives one option's struct and semantics; the loop that takes them all is
 * fmi_flux_denoise_with, after them. ---- */

/* The inpainting blend (no counterpart in the reference; the flow-matching form of diffusers' FluxInpaintPipeline): x0 / noise / mask.
 * After the model evaluation of step i, with s = f32(timesteps[i+1]):
 *   e = img + pred * dt                     (the plain update, same rounding)
 *   k = (1 - s) * x0 + s * noise            (the source re-noised to the step's target time, fmi_scale_noise's form)
 *   img = mask * e + (1 - mask) * k
 * mask = 1 gives e and mask = 0 gives k bit for bit; the schedule ends at s = 0, where k = x0 bit for bit, so kept
 * elements end as the source's exactly.  x0, noise, mask: (B,S,in_channels) f32 device buffers laid out like img_inout
 * (fmi_encode_latents, the packed noise the image would have started from, fmi_latent_mask); under sequence parallelism
 * this rank's rows, like img_inout.  Nothing before or inside the model evaluation knows about the blend.
 * Plain image-to-image (no mask) needs no blend: it is fmi_scale_noise at the first timestep of the cut schedule followed by the plain loop on that schedule. */

/* Reference-image ("in-context") conditioning as in FLUX.1 Kontext (the reference has no counterpart).  The reference image is encoded and
 * packed like the latents (fmi_vae_encode, fmi_encode_latents) and its R tokens are appended to the image tokens with a 1 in axis 0 of their position ids
 * (fmi_latent_ids with id0 = 1).  A model evaluation is Flux::forward over img' = cat([img, ctx], 1) and img_ids' = cat([img_ids, ctx_ids], 1) — S + R
 * image-stream rows per sample in every block — and the prediction is rows [0, S) of each sample: the final layer runs on those rows only.
 *   fmi_flux_forward_context  one such evaluation; `in` as for fmi_flux_forward, pred_out (B,S,in_channels) f32.  Bit for bit rows [0, S) of fmi_flux_forward on
 *                             the concatenated inputs.
 *   in the loop               the state is img_inout alone, (B,S,in_channels) f32; the update and the blend touch those rows only, with the same expressions and
 *                             roundings.  The context's rows of the model input and of the RoPE table are written once per call; each step casts only the S
 *                             state rows.
 * With R = 0 or a NULL context the launches are those of an evaluation without one.
 * FMI_ERR_INVALID: R < 0; R > 0 with a NULL ctx or ctx_ids; a ctx_dtype other than F32 / BF16.
 * FMI_ERR_UNSUPPORTED: a context (R > 0) under fmi_flux_set_sequence_parallel. */
typedef struct fmi_flux_context {
  const void* ctx;      fmi_dtype ctx_dtype; /* (B,R,in_channels) F32|BF16: packed reference latents, fmi_encode_latents' output */
  const float* ctx_ids;                      /* (B,R,3) f32; in->ids_per_sample applies to them as to img_ids */
  int R;                                     /* context tokens per sample; 0 (or a NULL struct) = no context */
} fmi_flux_context;
int fmi_flux_forward_context(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_context* ctx, float* pred_out, void* stream);

/* First-block step cache for the denoise loop (the method of ParaAttention's FBCache / diffusers' FirstBlockCacheConfig; the reference has no
 * counterpart).  Every step runs the input embedding and double block 0, takes the block's residual r = X1 - X0 of the f32 image stream (S' = S + R rows per
 * sample), and measures per sample
 *   d_b = sum |r - r_ref| / sum |r_ref|         (r_ref: the residual of the last COMPUTED step; divided on the host in double, +inf for a zero denominator)
 * A step is reused when a computed step precedes it and force[i] == 1, or force[i] < 0 (or force NULL), threshold > 0 and EVERY sample's d_b < threshold — the
 * decision is per call, not per sample, so a batched call under a threshold may differ from its single-sample runs (under a forced mask it does not).  A reused
 * step adds the cached output residual of all other blocks (XF = X1 + delta) and goes straight to the final layer: it costs img_in, one double block and the final
 * layer.  A computed step runs every block as always and refreshes delta = XF - X1 and r_ref.  Step 0 is always computed; nothing forces the last step.
 * The distances are compared as the f32 values distances_out reports.  The sums use no atomics and a decomposition fixed by S' * D: the same bits from run to run
 * and for any B.
 * No threshold is recommended here: ParaAttention suggests 0.08 for FLUX.1-dev, which nothing in this project could verify (it has no real weights).
 * With a cache, every step after the first computed one makes ONE small device-to-host copy and ONE hipStreamSynchronize on `stream` (the decision is taken on
 * the host): a cached loop is not legal under stream capture; decisions_out and distances_out are complete when it returns (the last step's launches may still be
 * queued, as without a cache).  The first cached call allocates four (B,S',D) f32 device buffers (regrown when a larger shape comes; fmi_flux_step_cache_bytes
 * reports them); a call without a cache never allocates them.
 * Works in the bf16, int8 and e4m3 modes, with nf4 weights and with LoRA adapters: it touches the f32 residual stream only.
 * FMI_ERR_INVALID: threshold negative or NaN; a force entry outside -1 / 0 / 1; force[0] == 1.  FMI_ERR_UNSUPPORTED: a model without double blocks
 * (num_layers < 1); sequence parallelism set (the distance would need an all-reduce).  FMI_ERR_STATE: while int8 calibration is recording. */
typedef struct fmi_flux_step_cache {
  float threshold;          /* 0: never reuse by distance; > 0: reuse when every sample's distance < threshold */
  const int8_t* force;      /* NULL or n_steps entries: -1 decide by threshold, 0 compute, 1 reuse */
  int32_t* decisions_out;   /* NULL or n_steps: 0 computed, 1 reused (host) */
  float* distances_out;     /* NULL or n_steps * B, step-major: d_b, -1 where not measured (host) */
} fmi_flux_step_cache;
size_t fmi_flux_step_cache_bytes(fmi_flux*);

/* True classifier-free guidance in the denoise loop (diffusers' FluxPipeline with negative_prompt= and true_cfg_scale > 1, `do_true_cfg`; the
 * reference has no counterpart).  Every step evaluates the model ONCE on an internal batch of 2B samples: rows [0,B) the prompt's (in->txt, in->y), rows [B,2B)
 * the negative's (neg_txt, neg_y); the state (B,S,in_channels) f32, the ids, the guidance vector, the context rows and the control are the same in both halves.
 * With dt = f32(ts[i+1] - ts[i]) and s = f32(ts[i+1]) the update is one pass,
 *   g = neg + scale * (pos - neg)             (diffusers' expression, the difference first: pos == neg or scale == 0 gives neg bit for bit;
 *                                              scale == 1 is NOT special-cased and is not pos bit for bit)
 *   e = img + g * dt                          (the plain update)
 *   img = e,  or with x0 / noise / mask       img = mask * e + (1 - mask) * ((1 - s) * x0 + s * noise)       (the blend, unchanged)
 * The once-per-image modulation GEMM, txt_in, the context rows and the RoPE table are hoisted for the 2B rows exactly as for a batch of 2B prompts, and each
 * sample of the call equals its own B = 1 call bit for bit.  The workspace is that of a batch of 2B.
 * Works in the bf16, int8 and e4m3 modes and on models without a guidance vector (in->guidance NULL).
 * FMI_ERR_INVALID: neg_txt or neg_y NULL; a dtype that is not F32 or BF16; scale negative, NaN or infinite.
 * FMI_ERR_UNSUPPORTED: in->B > 4 (2B would exceed the per-device limit of 8); sequence parallelism set (it runs B = 1); n_steps * 2B > 4096 (the
 * loop's limit of n_steps * B rows, counted on the internal batch).
 * FMI_ERR_STATE: while int8 calibration is recording. */
typedef struct fmi_flux_true_cfg {
  const void* neg_txt; fmi_dtype neg_txt_dtype;   /* (B,T,joint_attention_dim) F32|BF16, same T as in->txt */
  const void* neg_y;   fmi_dtype neg_y_dtype;     /* (B,pooled_projection_dim) F32|BF16 */
  float scale;                                    /* finite, >= 0 */
} fmi_flux_true_cfg;

/* Channel-concatenated conditioning (diffusers' FluxControlPipeline and FluxFillPipeline; the reference has no counterpart).  On a model made by
 * fmi_flux_create_cond with cond_channels > 0 one evaluation is Flux::forward on cat([img, cond], 2): the bf16 x_embedder operand (B*S, in_channels + cond_channels)
 * takes the state in its first in_channels columns every step and the conditioning in the others once per call (fmi_cast_cols_bf16).  The prediction, the state,
 * the Euler update, the blend and the CFG combine stay in_channels wide and keep their expressions; under true CFG both halves of the batch see the same cond.
 * The once-per-image modulation GEMM, txt_in and the RoPE table are hoisted as ever.  The forward and the loop work in the bf16, int8 and e4m3 modes (x_embedder
 * is not a block linear) and while int8 calibration records (the forward; the loop without cfg).
 * FMI_ERR_INVALID: ctl or ctl->cond NULL, or a cond_dtype that is not F32 / BF16, on a model with cond_channels > 0 — hence EVERY forward / denoise call without
 * a control on such a model —; a non-NULL ctl on a model with cond_channels == 0.  FMI_ERR_UNSUPPORTED: sequence parallelism. */
typedef struct fmi_flux_control {
  const void* cond; fmi_dtype cond_dtype;   /* (B,S,cond_channels) F32|BF16 */
} fmi_flux_control;
int fmi_flux_forward_control(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_control* ctl, float* pred_out, void* stream);

/* FLUX ControlNets: residual conditioning (diffusers' FluxControlNetModel, FluxTransformer2DModel.forward(controlnet_block_samples=,
 * controlnet_single_block_samples=) and FluxControlNetPipeline; the reference has no counterpart).  A ControlNet is a truncated FLUX transformer of nd >= 1 double
 * and ns >= 0 single blocks at the main model's width D, with the same embedders, no norm_out / proj_out, and
 *   controlnet_x_embedder         Linear(in_channels -> D) on cond, the packed VAE latents of the control image (B,S,in_channels), as fmi_encode_latents makes them
 *   controlnet_blocks.{i}         Linear(D -> D), one per double block            controlnet_single_blocks.{j}   Linear(D -> D), one per single block
 * Its evaluation on the main model's img, ids, txt, t, y, guidance (the guidance only if the net has guidance_embeds) is
 *   x = x_embedder(img) + controlnet_x_embedder(cond);  txt = context_embedder(txt);  vec, pe as ever
 *   for i < nd:  x, txt = transformer_blocks[i](x, txt, vec, pe);  d_i = controlnet_blocks[i](x)
 *   xs = cat([txt, x], 1);  for j < ns:  xs = single_transformer_blocks[j](xs, vec, pe);  s_j = controlnet_single_blocks[j](xs[:, T:])
 * and the main model (ND double, NS single blocks), with kd = ceil(ND / nd), ks = ceil(NS / ns), adds
 *   after double block i:  x_img += c * d[i / kd]            after single block j:  xs[:, T:, :] += c * s[j / ks]      (nothing if ns == 0)
 * Decisions of this library:
 *   - the samples d_i, s_j are stored as bf16: the round-to-nearest-even of the GEMM's f32 accumulator plus bias;
 *   - the scale is applied at the injection, in f32, as one __fmul_rn and one __fadd_rn per element, x = x + c * f32(sample), never contracted;
 *   - a step (or a forward) whose c is 0 launches neither the ControlNet's evaluation nor any injection: it is the plain step, launch for launch;
 *   - controlnet_x_embedder(cond) is computed once per call and kept in f32; each evaluation adds it to x_embedder(img) in f32;
 *   - in the loop the ControlNet's modulation vectors of all steps and its txt_in are hoisted like the main model's; its RoPE table is built once per call;
 *   - under true CFG the ControlNet runs on the same internal batch of 2B: the negative half sees the negative's txt / y, the same state and the same cond.
 * fmi_flux_create_controlnet makes an fmi_flux of this kind: cfg->num_layers / num_single_layers are the net's (num_single_layers == 0 is allowed).  It takes
 * FLUX's tensor names without norm_out.* / proj_out.*, plus controlnet_x_embedder.{weight,bias}, controlnet_blocks.{i}.{weight,bias} and
 * controlnet_single_blocks.{j}.{weight,bias}, through fmi_flux_set_tensor / fmi_flux_get_tensor / fmi_flux_missing_*.  Its sample buffers are sized by its first
 * evaluation and counted by fmi_flux_size_in_bytes; a call without a ControlNet allocates none.
 * The net runs in bf16 only.  On a ControlNet handle FMI_ERR_UNSUPPORTED: fmi_flux_quantize_fp8 / _int8, fmi_flux_calibrate_int8, fmi_flux_set_fp8_attention(2),
 * fmi_flux_lora_*, fmi_flux_set_linear_bnb4 / _int8, fmi_flux_set_sequence_parallel (world_size > 1), and every fmi_flux_forward* / fmi_flux_denoise* entry (and
 * with them the step cache).  The main model may be in any mode: the injection touches only its f32 stream.
 * Out of scope, refused where it would enter: several ControlNets at once, union modes (num_mode), the XLabs pixel-space hint block
 * (conditioning_embedding_channels), controlnet_blocks_repeat, quantised or LoRA-patched ControlNets, a ControlNet with a context, the step cache, channel
 * conditioning or sequence parallelism, resizing the control image, and fusing the injection into the blocks' last GEMM epilogue.
 * With a fmi_flux_controlnet — FMI_ERR_INVALID: net NULL or not a ControlNet; cond NULL; a cond_dtype that is not F32 / BF16; a scale or a step_scales entry that
 * is not finite; a net whose width, head count, joint_attention_dim, pooled_projection_dim, axes_dim, theta or in_channels differ from the main model's, or that
 * lives on another device; a guidance_embeds net without in->guidance.  FMI_ERR_UNSUPPORTED: see the table at fmi_flux_denoise_with.  FMI_ERR_STATE: a net
 * with missing tensors. */
int fmi_flux_create_controlnet(const fmi_flux_config* cfg, fmi_model_dtype dtype, fmi_flux** out);
int fmi_flux_is_controlnet(const fmi_flux*);
typedef struct fmi_flux_controlnet {
  fmi_flux* net;                            /* fmi_flux_create_controlnet's handle, every tensor set */
  const void* cond; fmi_dtype cond_dtype;   /* (B,S,in_channels) F32|BF16 */
  float scale;                              /* finite; the conditioning scale c */
  const float* step_scales;                 /* NULL, or n_steps host floats multiplied onto scale (c_i = scale * step_scales[i], in f32); a single forward ignores it */
} fmi_flux_controlnet;
/* One evaluation of the main model with the ControlNet's samples injected; pred_out (B,S,in_channels) f32.  cn NULL: fmi_flux_forward. */
int fmi_flux_forward_controlnet(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_controlnet* cn, float* pred_out, void* stream);
/* Test seams.  fmi_flux_controlnet_eval runs the ControlNet alone (`in` as for fmi_flux_forward, cond (B,S,in_channels)) and leaves its samples in the handle;
 * fmi_flux_controlnet_sample widens sample `index` of the double (single == 0) or single blocks of the last evaluation into out_f32 (B,S,D), a device buffer
 * (it synchronises the device). */
int fmi_flux_controlnet_eval(fmi_flux* net, const fmi_flux_inputs* in, const void* cond, fmi_dtype cond_dtype, void* stream);
int fmi_flux_controlnet_sample(fmi_flux* net, int single, int index, float* out_f32);
/* The injection kernel on its own (op-level glue; device pointers, no allocation): for b < B, r < rows, d < D
 *   x[b * x_batch_stride + r * D + d] = x[...] + scale * f32(src[(b * rows + r) * D + d])          (__fadd_rn(x, __fmul_rn(scale, src)): numpy reproduces the bits)
 * x_batch_stride >= rows * D, in floats: (B*S, D) contiguous is stride S * D; the image rows [T, T + S) of every (T + S)-row sample of the joint stream are the
 * pointer advanced by T * D with stride (T + S) * D.  Nothing outside those rows is touched.  16-byte accesses when rows * D % 8 == 0, x_batch_stride % 4 == 0
 * and both pointers are 16-byte aligned, else scalar ones: the same bits either way.  FMI_ERR_INVALID: a null pointer, a negative size, a stride below rows * D. */
int fmi_add_scaled_rows_bf16(float* x_f32, int64_t x_batch_stride, const void* src_bf16, int B, int64_t rows, int D, float scale, void* stream);

/* FLUX IP-Adapter: image-prompt attention in the double blocks (XLabs flux-ip-adapter / -v2, diffusers' FluxIPAdapterMixin and
 * FluxIPAdapterAttnProcessor; the reference has no counterpart).  With D = H * 128, J = joint_attention_dim, an adapter of N tokens on embeddings of width E holds
 *   image_proj.image_embeds   Linear(E -> N * J)           image_proj.norm   LayerNorm(J, eps 1e-5, affine)
 *   ip_adapter.{i}.to_k_ip / to_v_ip   Linear(J -> D), one pair per double block i; their biases are optional (zero unless set)
 * Once per call:   tok = LayerNorm(Linear(embeds)).reshape(B, N, J);   K_i = to_k_ip_i(tok), V_i = to_v_ip_i(tok), viewed (B, N, H, 128) — no QkNorm, no RoPE.
 * In double block i of every evaluation, with q = norm_q_i(to_q_i(LayerNorm-modulated image rows)) — after the block's RMSNorm, BEFORE RoPE —
 *   ip = softmax(q K_i^T / sqrt(128)) V_i   per sample and head, over the N tokens, for every image row;   after the block: x_img += c * ip   (f32)
 * ip does not pass the attention's output projection and is not gated; text rows and single blocks are untouched; a ControlNet's residual is added after it.
 * Decisions of this library:
 *   - the raw q is the bf16 the q|k|v GEMM stores; RMSNorm, scores and softmax are f32 (the normed q is not rounded to bf16); tok is f32; K_i / V_i are the f32
 *     accumulator plus bias rounded once to bf16; ip accumulates in f32; the update is one __fmul_rn and one __fadd_rn per element, x = x + c * ip;
 *   - while an adapter with c != 0 is attached, the image stream's q|k|v projection of the double blocks takes the plain epilogue and the stand-alone relayout
 *     kernels (the fused relayout epilogue keeps only the rotated q); a call without an adapter, and a step whose c is 0, keeps the fused path, launch for launch;
 *   - tok and every K_i / V_i are computed once per call into buffers the adapter owns (sized by the first call, regrown when a larger batch comes);
 *   - under true CFG the prompt half attends to embeds, the negative half to neg_embeds or — NULL — to all-zero embeddings through the same projection (the bias
 *     and the LayerNorm make those tokens non-zero), as diffusers does; the ControlNet's own evaluation is not image-prompted.
 * 1 <= N <= 32 (XLabs: 4); another N is FMI_ERR_UNSUPPORTED.  E and J multiples of 8, at most 16384.  A CLIP vision encoder is out of scope: embeddings are supplied.
 * With a fmi_flux_ip — FMI_ERR_INVALID: adapter or embeds NULL; an embeds_dtype that is not F32 / BF16; a scale or step_scales entry that is not finite; an adapter
 * whose width, joint_attention_dim or number of double blocks differ from the model's, or that lives on another device.  FMI_ERR_UNSUPPORTED: a context (R > 0),
 * the step cache, sequence parallelism, the fp8 / int8 modes, fmi_flux_set_fp8_attention(m, 2).  FMI_ERR_STATE: an adapter with missing tensors.  It combines
 * with the negative, x0 / noise / mask, a control (ctl) and a ControlNet. */
typedef struct fmi_ip_adapter fmi_ip_adapter; /* opaque */
/* cfg: the transformer's (num_attention_heads, joint_attention_dim and num_layers are used).  The weights (bf16) are allocated here, zero-initialised. */
int fmi_ip_adapter_create(const fmi_flux_config* cfg, int embed_dim, int num_tokens, fmi_ip_adapter** out);
void fmi_ip_adapter_destroy(fmi_ip_adapter*);
/* One tensor by the names above plus .weight / .bias (host or device pointer, F32 / F16 / BF16, shape checked; synchronous).  FMI_ERR_INVALID: unknown name, wrong shape. */
int fmi_ip_adapter_set_tensor(fmi_ip_adapter*, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank);
int fmi_ip_adapter_missing_count(const fmi_ip_adapter*);
const char* fmi_ip_adapter_missing_name(const fmi_ip_adapter*, int i);
size_t fmi_ip_adapter_size_in_bytes(const fmi_ip_adapter*); /* weights + the per-call projection buffers */
typedef struct fmi_flux_ip {
  fmi_ip_adapter* adapter;                       /* every required tensor set */
  const void* embeds; fmi_dtype embeds_dtype;    /* (B,E) F32|BF16: one image embedding per sample */
  const void* neg_embeds;                        /* (B,E) of embeds_dtype, or NULL (zeros): the negative half's under true CFG; ignored without a negative */
  float scale;                                   /* finite; the adapter scale c */
  const float* step_scales;                      /* NULL, or n_steps host floats multiplied onto scale (c_i = scale * step_scales[i], in f32); a single forward ignores it */
} fmi_flux_ip;
/* One evaluation with the adapter; ctl (a cond_channels > 0 model's control) and cn may be NULL.  ip NULL: fmi_flux_forward_controlnet / _control. */
int fmi_flux_forward_ip(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_control* ctl, const fmi_flux_controlnet* cn, const fmi_flux_ip* ip, float* pred_out, void* stream);
/* The image-prompt attention kernel on its own (op-level; device pointers, no allocation): for b < B, r < S, h < H
 *   x[b * x_batch_stride + r * H * 128 + h * 128 + :] += scale * ip(q[b * q_batch_stride + r * q_row_stride + h * 128 + :], norm_q, k[b, h, :, :], v[b, h, :, :])
 * with q bf16 (the q|k|v GEMM's plain output: row stride 3 * H * 128 there), norm_q (128) bf16, k / v (B, H, N, 128) bf16, x f32, by the recipe above.  Strides in
 * elements; every pointer 16-byte aligned, the q strides multiples of 8, x_batch_stride a multiple of 4 and >= S * H * 128.  max_row_blocks: 0, or a cap on the
 * grid's row dimension (a test seam: the bits do not depend on it).  FMI_ERR_UNSUPPORTED: N outside [1, 32].  FMI_ERR_INVALID: everything else. */
int fmi_ip_attention(const void* q_bf16, int q_row_stride, int64_t q_batch_stride, const void* norm_q_bf16, const void* k_bf16, const void* v_bf16, float* x_f32,
                     int64_t x_batch_stride, int B, int H, int S, int N, float scale, int max_row_blocks, void* stream);

/* The whole denoise loop == Sampler::sample(FlowMatchEulerDiscrete)
 * (pipelines/sampling.rs:25-48) around the step closure (pipelines/flux/mod.rs:305-318):
 *   for (t_curr,t_prev) in windows(timesteps): img += forward(img, t_curr) * (t_prev-t_curr)
 * `img_inout` (B,S,C) f32 is the state, updated in place (in->img and in->timesteps are ignored); `timesteps_host`
 * (n_steps+1 f64, host) drives the loop, exactly the Vec<f64> of SchedulerConfig::get_timesteps.
 * The latent stays f32 between steps.
 * `opts` names what every evaluation and the per-step update are conditioned on; a NULL opts is a struct of NULLs, the reference's loop.  An option that is
 * NULL costs nothing: the call then issues exactly the launches, and makes exactly the allocations, of a call that never heard of it.
 * Which options combine (yes), and the code that refuses the pairs that do not:
 *             ctl                   cfg    cache                 x0/noise/mask
 *   ctx       FMI_ERR_UNSUPPORTED   yes    yes                   yes
 *   ctl                             yes    FMI_ERR_UNSUPPORTED   yes
 *   cfg                                    FMI_ERR_UNSUPPORTED   yes
 *   cache                                                        yes
 *   cn        ctx: FMI_ERR_UNSUPPORTED   ctl (a cond_channels > 0 model): FMI_ERR_UNSUPPORTED   cfg: yes   cache: FMI_ERR_UNSUPPORTED   x0/noise/mask: yes
 * (cn: the ControlNet argument of fmi_flux_denoise_controlnet below, not a field of this struct; under sequence parallelism FMI_ERR_UNSUPPORTED.)
 *   ip        ctx: FMI_ERR_UNSUPPORTED   ctl: yes   cfg: yes   cache: FMI_ERR_UNSUPPORTED   x0/noise/mask: yes   cn: yes
 * (ip: the IP-Adapter argument of fmi_flux_denoise_ip below; FMI_ERR_UNSUPPORTED under sequence parallelism and in the fp8 / int8 modes.)
 * Three or more combine when every pair among them does.  x0 / noise / mask given only in part: FMI_ERR_INVALID.  Each option's own refusals are listed at its
 * struct above; n_steps * B > 4096 is FMI_ERR_UNSUPPORTED.  EVERY refusal — of an argument, an option or a combination — comes before any launch, any
 * allocation and any use of `stream`: a refused call leaves img_inout, the outputs of `cache` and the model as they were. */
typedef struct fmi_flux_denoise_options {
  const fmi_flux_context*    ctx;    /* NULL or R == 0: none */
  const fmi_flux_control*    ctl;    /* required on a cond_channels > 0 model, refused on any other */
  const fmi_flux_true_cfg*   cfg;    /* NULL: no negative prompt */
  const fmi_flux_step_cache* cache;  /* NULL: no step cache */
  const float *x0, *noise, *mask;    /* all three or none */
} fmi_flux_denoise_options;
int fmi_flux_denoise_with(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_denoise_options* opts /* NULL == all NULL */,
                          float* img_inout, const double* timesteps_host, int n_steps, void* stream);
/* The same loop with a ControlNet (see fmi_flux_controlnet above): step i evaluates the ControlNet on the step's state and injects its samples at
 * c_i = cn->scale * step_scales[i] (cn->scale without step_scales); a step whose c_i is 0 is the plain step.  The ControlNet is an argument of its own — the
 * options struct keeps its 7 fields — and fmi_flux_denoise_with IS this call with cn == NULL: the same launches, bits, errors and allocations. */
int fmi_flux_denoise_controlnet(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_denoise_options* opts /* NULL == all NULL */, const fmi_flux_controlnet* cn,
                                float* img_inout, const double* timesteps_host, int n_steps, void* stream);
/* The same loop with an IP-Adapter (see fmi_flux_ip above), and a ControlNet if cn is not NULL: every double block of step i adds the image-prompt attention at
 * c_i = ip->scale * step_scales[i] (ip->scale without step_scales); a step whose c_i is 0 is the plain step, launch for launch.  The projection of the embeddings
 * runs once per call, never per step.  fmi_flux_denoise_controlnet IS this call with ip == NULL: the same launches, bits, errors and allocations. */
int fmi_flux_denoise_ip(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_denoise_options* opts /* NULL == all NULL */, const fmi_flux_controlnet* cn,
                        const fmi_flux_ip* ip, float* img_inout, const double* timesteps_host, int n_steps, void* stream);
/* The same loop with a second-order integrator.  Flow matching: sigma = t, alpha = 1 - t; g is the model's prediction, or under a negative
 * prompt neg + scale * (pos - neg).  The solver is an argument of its own and fmi_flux_denoise_ip IS this call with solver == NULL; FMI_SOLVER_EULER is the
 * same: the launches, bits, errors and allocations of a call that never heard of a solver.
 *   FMI_SOLVER_HEUN, step i with dt = t_{i+1} - t_i:  g1 = g(x, t_i);  xp = x + g1 * dt;  if t_{i+1} == 0: x = xp (the Euler step) — else g2 = g(xp, t_{i+1}) and
 *     x = x + ((g1 + g2) * 0.5) * dt.  2 n_steps - 1 evaluations when the schedule ends at 0, else 2 n_steps.  The per-image hoisted rows cover all n_steps + 1
 *     times; both evaluations of step i run at step i's ControlNet / IP-Adapter scale.  With x0 / noise / mask both xp and the corrected x are states at t_{i+1}
 *     and both are blended there.
 *   FMI_SOLVER_DPMPP_2M (data prediction, two-step, midpoint), with l(t) = ln((1 - t) / t):  D_i = x - t_i * g;  a = t_{i+1} / t_i, c = 1 - a,
 *     w = (l_{i+1} - l_i) / (2 (l_i - l_{i-1})), and w = 0 at i == 0, after t_{i-1} == 1 and into t_{i+1} == 0;  D' = D_i + w * (D_i - D_{i-1});
 *     x = a * x + c * D';  the history becomes D_i;  then the blend at t_{i+1}, if any.  One evaluation per step; a, c, w are computed in double and rounded once
 *     (fmi_dpmpp_2m_coefficients).
 * A solver's schedule is strictly decreasing with 1 >= timesteps_host[0] and timesteps_host[n_steps] >= 0: FMI_ERR_INVALID otherwise, and for an unknown kind.
 * Not in the table above, in the solver's own check: FMI_SOLVER_HEUN with the step cache, and either solver under sequence parallelism, answer
 * FMI_ERR_UNSUPPORTED.  Everything else combines: the blend, a context, a control, a negative prompt, a ControlNet, an IP-Adapter, LoRA, the 8-bit modes, and
 * FMI_SOLVER_DPMPP_2M with the step cache (a reused step's prediction enters the update like any other).  Like every refusal these come before any launch or
 * allocation.  The first solver call allocates state-sized f32 buffers — two for Heun (xp, g1), one for 2M (the history); regrown when a larger state comes,
 * counted by fmi_flux_size_in_bytes and fmi_flux_solver_bytes, released with the model; a loop without a solver never allocates them. */
enum { FMI_SOLVER_EULER = 0, FMI_SOLVER_HEUN = 1, FMI_SOLVER_DPMPP_2M = 2 };
typedef struct fmi_flux_solver {
  int kind; /* FMI_SOLVER_* */
} fmi_flux_solver;
int fmi_flux_denoise_solver(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_denoise_options* opts /* NULL == all NULL */, const fmi_flux_controlnet* cn,
                            const fmi_flux_ip* ip, const fmi_flux_solver* solver /* NULL == FMI_SOLVER_EULER */, float* img_inout, const double* timesteps_host,
                            int n_steps, void* stream);
size_t fmi_flux_solver_bytes(fmi_flux*); /* device bytes the solvers' buffers hold (0 until the first Heun / 2M call) */

/* The entries from before fmi_flux_denoise_with.  Each IS fmi_flux_denoise_with with the fields it names set from its arguments and every other field NULL —
 * the same launches, bits, errors and allocations. */
/* no field */
int fmi_flux_denoise(fmi_flux*, const fmi_flux_inputs* in, float* img_inout,
                     const double* timesteps_host, int n_steps, void* stream);
/* x0, noise, mask — here all three are required (FMI_ERR_INVALID) */
int fmi_flux_denoise_inpaint(fmi_flux*, const fmi_flux_inputs* in, float* img_inout, const double* timesteps_host, int n_steps,
                             const float* x0, const float* noise, const float* mask, void* stream);
/* ctx, x0, noise, mask */
int fmi_flux_denoise_context(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_context* ctx, float* img_inout, const double* timesteps_host, int n_steps,
                             const float* x0, const float* noise, const float* mask, void* stream);
/* ctx, x0, noise, mask, cache */
int fmi_flux_denoise_cached(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_context* ctx, float* img_inout, const double* timesteps_host,
                            int n_steps, const float* x0, const float* noise, const float* mask, const fmi_flux_step_cache* cache, void* stream);
/* ctx, cfg, x0, noise, mask */
int fmi_flux_denoise_cfg(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_context* ctx, const fmi_flux_true_cfg* cfg,
                         float* img_inout, const double* timesteps_host, int n_steps,
                         const float* x0, const float* noise, const float* mask, void* stream);
/* ctl, cfg, x0, noise, mask */
int fmi_flux_denoise_control(fmi_flux*, const fmi_flux_inputs* in, const fmi_flux_control* ctl, const fmi_flux_true_cfg* cfg,
                             float* img_inout, const double* timesteps_host, int n_steps,
                             const float* x0, const float* noise, const float* mask, void* stream);

/* Per-phase device time of the last forward in ms (hipEvents; enabled by
 * fmi_flux_set_profiling(1), which also serialises phases).  Phases: see fmi_flux_phase_name.
 * With FMI_ROCTX=1 in the environment every phase is also a roctx range (roctxRangePushA / Pop from
 * librocprofiler-sdk-roctx, opened at run time), so `rocprofv3 --marker-trace --kernel-trace` groups the trace by phase. */
int fmi_flux_set_profiling(fmi_flux*, int enable);
/* Tuning / verification knob (default 1): QkNorm (model.rs:433-452) + apply_rope (:77-101) + the
 * head-major q,k and transposed v relayout run in the epilogue of the [q|k|v] projection GEMM
 * instead of as stand-alone kernels over the stored projection.  Both forms use the same arithmetic
 * and give bit-identical results; shapes whose token offsets are not multiples of 16 always take the
 * stand-alone kernels. */
int fmi_flux_set_fused_qkv_relayout(fmi_flux*, int enable);
int fmi_flux_phase_count(void);
const char* fmi_flux_phase_name(int i);
int fmi_flux_phase_ms(fmi_flux*, float* ms_out /* [phase_count] */);

/* ------------------------------------------------------------------------------------
 * VAE decoder — replaces AutoEncoderKl::decode (vaes/autoencoder_kl.rs:112-119) and
 * Decoder::forward (vaes/vae.rs:436-456)
 * ---------------------------------------------------------------------------------- */
typedef struct fmi_vae_config {
  int in_channels;           /* 3  (unused by decode) */
  int out_channels;          /* 3 */
  int block_out_channels[4]; /* {128,256,512,512} */
  int n_blocks;              /* 4 */
  int layers_per_block;      /* 2 */
  int latent_channels;       /* 16 */
  int norm_num_groups;       /* 32 */
  int mid_block_add_attention;
  int use_post_quant_conv;   /* 0 for FLUX */
  double scaling_factor;     /* 0.3611 */
  double shift_factor;       /* 0.1159 */
  int use_quant_conv;        /* 0 for FLUX (encoder side 1x1 conv, autoencoder_kl.rs:67-77) */
} fmi_vae_config;

typedef struct fmi_vae fmi_vae;
void fmi_vae_default_config(fmi_vae_config* cfg);
int fmi_vae_create(const fmi_vae_config* cfg, fmi_model_dtype dtype, fmi_vae** out);
void fmi_vae_destroy(fmi_vae*);
/* diffusers names under "decoder." / "post_quant_conv.", e.g.
 * "decoder.conv_in.weight", "decoder.mid_block.resnets.0.norm1.weight",
 * "decoder.mid_block.attentions.0.to_q.weight", "decoder.up_blocks.2.resnets.0.conv_shortcut.weight",
 * "decoder.up_blocks.0.upsamplers.0.conv.bias", "decoder.conv_norm_out.weight" (vae.rs:371-433).
 * Conv weights are (Cout,Cin,kh,kw) as stored; they are re-laid out for the implicit-GEMM
 * kernels.  host or device pointer, F32/F16/BF16. */
int fmi_vae_set_tensor(fmi_vae*, const char* name, const void* data, fmi_dtype dtype,
                       const int64_t* shape, int rank);
int fmi_vae_missing_count(const fmi_vae*);
const char* fmi_vae_missing_name(const fmi_vae*, int i);
double fmi_vae_scale_factor(const fmi_vae*); /* VAEModel::scale_factor, vaes/mod.rs:15-28 */
double fmi_vae_shift_factor(const fmi_vae*);
/* z (B,latent_channels,h,w) f32 NCHW -> image (B,out_channels,8h,8w) f32 NCHW.
 * == VAEModel::decode. */
int fmi_vae_decode(fmi_vae*, const float* z, int B, int h, int w, float* image_out, void* stream);
/* image (B,in_channels,H,W) f32 NCHW, H and W multiples of 8 -> z (B,latent_channels,H/8,W/8) f32 =
 * mean + exp(0.5*logvar) * noise.  == VAEModel::encode = Encoder::forward (vaes/vae.rs:330-349),
 * optional quant_conv, DiagonalGaussian (vae.rs:470-480).  The reference draws `noise` with an
 * unseedable randn_like; here the caller passes it (fmi_randn) or NULL for z = mean.
 * moments_out (B,2*latent_channels,H/8,W/8) f32 optional.  decode needs only the `decoder.*`
 * tensors, encode only `encoder.*` (+ `quant_conv.*`). */
int fmi_vae_encode(fmi_vae*, const float* image, int B, int H, int W, const float* noise, float* z_out, float* moments_out, void* stream);
/* AttnBlock::forward (vaes/vae.rs:95-111) of the decoder's mid block as one op: x and out (B,H,W,C) bf16 NHWC device
 * buffers, C = block_out_channels.last; out = x + to_out(sdpa(q,k,v)(group_norm(x))).  Needs the
 * `decoder.*` tensors.  Used by the parity tests to check the block alone at production size. */
int fmi_vae_mid_attention(fmi_vae*, const void* x_bf16_nhwc, int B, int H, int W, void* out_bf16_nhwc, void* stream);

/* ------------------------------------------------------------------------------------
 * Text encoders — they run once per image in front of the denoise loop and
 * produce its `txt` (B,T,4096) and `y` (B,768) inputs (pipelines/flux/mod.rs:237-262).
 * Token ids are int32, row-major (B,T), in host OR device memory (copied with hipMemcpyDefault).
 * Tokenisation itself (tokenizers crate, flux/mod.rs:203-221) stays on the host side.
 * ---------------------------------------------------------------------------------- */
/* T5Config (diffusion_rs_core/src/models/t5/mod.rs:72-91); feed_forward_proj as an enum */
typedef enum fmi_t5_act { FMI_T5_RELU = 0 /* "relu", ungated */, FMI_T5_GATED_GELU = 1 /* "gated-gelu" (NewGelu) */, FMI_T5_GATED_SILU = 2 } fmi_t5_act;
typedef struct fmi_t5_config {
  int vocab_size, d_model, d_kv, d_ff, num_layers, num_heads;
  int relative_attention_num_buckets, relative_attention_max_distance;
  float layer_norm_epsilon;
  fmi_t5_act feed_forward_act;
} fmi_t5_config;
typedef struct fmi_t5 fmi_t5;
void fmi_t5_default_config(fmi_t5_config*); /* t5-v1_1-xxl encoder (FLUX.1 text_encoder_2) */
/* == T5EncoderModel::new (t5/mod.rs:614-627); d_kv must be 64, d_model/d_ff multiples of 64;
 * quantised (bnb) T5 linears are not supported (FMI_ERR_INVALID on their side tensors). */
int fmi_t5_create(const fmi_t5_config*, fmi_t5** out);
void fmi_t5_destroy(fmi_t5*);
/* tensor names as T5EncoderModel's VarBuilder reads them: shared.weight,
 * encoder.block.N.layer.0.{layer_norm.weight, SelfAttention.{q,k,v,o}.weight},
 * encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight,
 * encoder.block.N.layer.1.{layer_norm.weight, DenseReluDense.{wi_0,wi_1,wo}.weight},
 * encoder.final_layer_norm.weight */
int fmi_t5_set_tensor(fmi_t5*, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank);
/* bitsandbytes-quantised Linears of the encoder blocks (`<prefix>` = "encoder.block.N.layer.0.SelfAttention.q" ...): the
 * reference builds every T5 Linear as a QuantMethod from text_encoder_2's quantization_config (t5/mod.rs:132-173,258-261 ->
 * BnbLinear, bitsandbytes/mod.rs:111-239).  Arguments as fmi_flux_set_linear_bnb4 / _int8 (host or device pointers).  The
 * codes are expanded once at load into the encoder's bf16 weights (BnbLinear::forward = dequantise + matmul, mod.rs:293-312;
 * the encoder runs once per image), bit-exact with dequantize_blockwise_bf16_* / dequantize_8bit_kernel_bf16. */
int fmi_t5_set_linear_bnb4(fmi_t5*, const char* prefix, const uint8_t* packed, const float* absmax, int blocksize, int quant_type,
                           int out_features, int in_features);
int fmi_t5_set_linear_int8(fmi_t5*, const char* prefix, const int8_t* weight, const float* scb, int out_features, int in_features);
int fmi_t5_missing_count(const fmi_t5*);
const char* fmi_t5_missing_name(fmi_t5*, int i);
size_t fmi_t5_size_in_bytes(const fmi_t5*);
/* == T5EncoderModel::forward (t5/mod.rs:629-631): out (B,T,d_model) device, FMI_BF16 or FMI_F32.
 * Synchronises the stream before returning (token-id range check). */
int fmi_t5_forward(fmi_t5*, const int32_t* input_ids, int B, int T, void* out, fmi_dtype out_dtype, void* stream);

/* ClipTextConfig (models/clip/text.rs:24-33): projection_dim is used as the hidden width */
typedef struct fmi_clip_config {
  int vocab_size, projection_dim, intermediate_size, max_position_embeddings, num_hidden_layers, num_attention_heads;
} fmi_clip_config;
typedef struct fmi_clip fmi_clip;
void fmi_clip_default_config(fmi_clip_config*); /* clip-vit-large-patch14 text tower (FLUX.1 text_encoder) */
int fmi_clip_create(const fmi_clip_config*, fmi_clip** out); /* head dim must be 64 */
void fmi_clip_destroy(fmi_clip*);
/* names under the "text_model." prefix (flux/mod.rs:105), e.g.
 * text_model.encoder.layers.N.self_attn.q_proj.{weight,bias} */
int fmi_clip_set_tensor(fmi_clip*, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank);
int fmi_clip_missing_count(const fmi_clip*);
const char* fmi_clip_missing_name(fmi_clip*, int i);
size_t fmi_clip_size_in_bytes(const fmi_clip*);
/* == ClipTextTransformer::forward (clip/text.rs:303-317): pooled (B,projection_dim) = final
 * hidden state at argmax(token id) of each row, FMI_F32 or FMI_BF16; hidden_out (B,T,dim) f32
 * optional (NULL to skip).  Synchronises the stream before returning. */
int fmi_clip_forward(fmi_clip*, const int32_t* input_ids, int B, int T, void* pooled_out, fmi_dtype pooled_dtype, float* hidden_out, void* stream);

/* ------------------------------------------------------------------------------------
 * CLIP vision encoder (not in the reference): the image prompt of the IP-Adapter (fmi_flux_ip.embeds) from
 * a picture.  It runs once per request in front of the denoise loop, like the text encoders.
 * ---------------------------------------------------------------------------------- */
/* u8 (h,w,3) device image -> u8 (nh,nw,3), PIL's Image.resize(BICUBIC) as CLIP's image processor calls it: two separable
 * passes, horizontal first, then vertical (a pass whose size stays is skipped), the value rounded to nearest and clamped to
 * [0,255] after each.  Along an axis, output o reads the inputs [lo, hi): scale = in / out, fs = max(scale, 1), support =
 * 2 fs, centre = (o + 0.5) scale, lo = max(0, int(centre - support + 0.5)), hi = min(in, int(centre + support + 0.5)), with
 * the weights k((j - centre + 0.5) / fs) normalised to sum 1, k = Keys' cubic at a = -0.5.  f32 arithmetic, one thread per
 * output pixel, no atomics: the same bits for any launch grid.  PIL itself works in 22-bit fixed point: a value can differ
 * from PIL's by 1.  FMI_ERR_INVALID for h, w, nh, nw <= 0. */
int fmi_resize_bicubic_u8(const uint8_t* in, int h, int w, uint8_t* out, int nh, int nw, void* stream);
/* u8 (nh,nw,3) device image -> pixel_values (3,S,S) f32: the centre crop at top = (nh - S) / 2, left = (nw - S) / 2 (integer
 * division), then (v / 255 - mean[c]) / std[c] as three f32 operations.  mean, std: 3 host floats.  FMI_ERR_INVALID for
 * nh < S or nw < S (the crop never pads). */
int fmi_clip_preprocess_u8(const uint8_t* in, int nh, int nw, int S, const float* mean, const float* std_, float* out, void* stream);
/* HuggingFace's CLIPVisionConfig; hidden_act is quick_gelu and layer_norm_eps 1e-5, as in every CLIP checkpoint */
typedef struct fmi_clip_vision_config {
  int image_size, patch_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, projection_dim;
} fmi_clip_vision_config;
typedef struct fmi_clip_vision fmi_clip_vision;
void fmi_clip_vision_default_config(fmi_clip_vision_config*); /* openai/clip-vit-large-patch14's vision tower: 224 / 14 / 1024 / 4096 / 24 / 16 / 768 */
/* head dim (hidden_size / num_attention_heads) must be 64, the three widths multiples of 64, image_size a multiple of
 * patch_size, and 1 + (image_size / patch_size)^2 tokens at most 1024 (the encoder attention's limit) */
int fmi_clip_vision_create(const fmi_clip_vision_config*, fmi_clip_vision** out);
void fmi_clip_vision_destroy(fmi_clip_vision*);
/* HuggingFace's names (CLIPVisionModelWithProjection, and the vision half of a CLIPModel checkpoint):
 * vision_model.embeddings.{class_embedding (D), patch_embedding.weight (D,3,P,P), position_embedding.weight (1 + Np, D)},
 * vision_model.pre_layrnorm.{weight,bias} (their spelling), vision_model.encoder.layers.N.* as the text tower's,
 * vision_model.post_layernorm.{weight,bias}, visual_projection.weight (projection_dim, D) */
int fmi_clip_vision_set_tensor(fmi_clip_vision*, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank);
int fmi_clip_vision_missing_count(const fmi_clip_vision*);
const char* fmi_clip_vision_missing_name(fmi_clip_vision*, int i);
size_t fmi_clip_vision_size_in_bytes(const fmi_clip_vision*);
/* == CLIPVisionModelWithProjection.forward: pixel_values (B,3,S,S) f32 device, S = image_size -> image_embeds
 * (B,projection_dim), FMI_F32 or FMI_BF16 = visual_projection(post_layernorm(class row)); hidden_out (B, 1 + Np, D) f32
 * optional (NULL to skip): the encoder's output before post_layernorm, HF's last_hidden_state.  Synchronises the stream
 * before returning. */
int fmi_clip_vision_forward(fmi_clip_vision*, const float* pixel_values, int B, void* image_embeds_out, fmi_dtype dtype, float* hidden_out, void* stream);

/* ------------------------------------------------------------------------------------
 * FLUX.1 Redux (not in the reference; diffusers' FluxPriorReduxPipeline): image variation.  A SigLIP
 * vision tower turns a picture into (Np, D) hidden states, the Redux embedder turns those into (Np, J) image tokens, and
 * the caller appends scale * tokens behind the T5 rows of fmi_flux_inputs.txt (T = T_prompt + Np, txt_ids zeros): the
 * denoise loop itself is unchanged.  The picture is prepared by fmi_resize_bicubic_u8 straight to S x S and
 * fmi_clip_preprocess_u8 with nh = nw = S, which crops nothing.
 * ---------------------------------------------------------------------------------- */
/* HuggingFace's SiglipVisionConfig; hidden_act is gelu_pytorch_tanh */
typedef struct fmi_siglip_vision_config {
  int image_size, patch_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads;
  float layer_norm_eps;
} fmi_siglip_vision_config;
typedef struct fmi_siglip_vision fmi_siglip_vision;
void fmi_siglip_vision_default_config(fmi_siglip_vision_config*); /* google/siglip-so400m-patch14-384: 384 / 14 / 1152 / 4304 / 27 / 16 / 1e-6 */
/* hidden_size a multiple of 64; head dim (hidden_size / num_attention_heads) any multiple of 8 up to 128 — the attention
 * runs at d = 128 on heads that are zero-padded in the weights; intermediate_size any positive size (padded to the next
 * multiple of 64 the same way); image_size >= patch_size: the convolution has no padding, so there are G = image_size /
 * patch_size (rounded down) patches per side, Np = G^2, and the pixels past G * patch_size are not read (384 / 14: 27) */
int fmi_siglip_vision_create(const fmi_siglip_vision_config*, fmi_siglip_vision** out);
void fmi_siglip_vision_destroy(fmi_siglip_vision*);
/* HuggingFace's names (SiglipVisionModel): vision_model.embeddings.{patch_embedding.{weight (D,3,P,P), bias (D)},
 * position_embedding.weight (Np, D)}, vision_model.encoder.layers.N.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2,
 * mlp.fc1, mlp.fc2}.{weight,bias}, vision_model.post_layernorm.{weight,bias}.  The pooling head (vision_model.head.*) is
 * not part of the model: the caller drops it. */
int fmi_siglip_vision_set_tensor(fmi_siglip_vision*, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank);
int fmi_siglip_vision_missing_count(const fmi_siglip_vision*);
const char* fmi_siglip_vision_missing_name(fmi_siglip_vision*, int i);
size_t fmi_siglip_vision_size_in_bytes(const fmi_siglip_vision*);
/* == SiglipVisionModel.forward(...).last_hidden_state: pixel_values (B,3,S,S) f32 device -> hidden_out (B, Np, D), FMI_F32
 * or FMI_BF16, Np = (S / P rounded down)^2: post_layernorm of every row.  Synchronises the stream before returning. */
int fmi_siglip_vision_forward(fmi_siglip_vision*, const float* pixel_values, int B, void* hidden_out, fmi_dtype dtype, void* stream);
/* Test seam: sizes the handle's workspace for a batch of B and fills every byte of it with 0xff (a NaN in bf16 and in f32),
 * so that a following forward shows whether anything reads a lane it did not write.  Synchronises the stream. */
int fmi_siglip_vision_poison_workspace(fmi_siglip_vision*, int B, void* stream);

/* diffusers' ReduxImageEncoder: redux_up Linear(redux_dim -> 3 txt_dim), SiLU, redux_down Linear(3 txt_dim -> txt_dim), both
 * biased; redux_dim and txt_dim multiples of 64 */
typedef struct fmi_redux fmi_redux;
int fmi_redux_create(int redux_dim, int txt_dim, fmi_redux** out);
void fmi_redux_destroy(fmi_redux*);
/* redux_up.{weight (3 J, D), bias (3 J)}, redux_down.{weight (J, 3 J), bias (J)} */
int fmi_redux_set_tensor(fmi_redux*, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank);
int fmi_redux_missing_count(const fmi_redux*);
const char* fmi_redux_missing_name(fmi_redux*, int i);
size_t fmi_redux_size_in_bytes(const fmi_redux*);
/* hidden (rows, redux_dim) f32 device (rounded to bf16 for the first GEMM) -> out (rows, txt_dim), FMI_F32 or FMI_BF16 =
 * scale * redux_down(silu(redux_up(hidden))): the scale multiplies the biased result, in f32, before the one rounding of a
 * bf16 output.  scale finite.  Synchronises the stream before returning. */
int fmi_redux_forward(fmi_redux*, const float* hidden, int rows, float scale, void* out, fmi_dtype dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Pipeline glue on device — the tensor code of FluxPipeline::forward
 * (pipelines/flux/mod.rs:270-332) and flux/sampling.rs
 * ---------------------------------------------------------------------------------- */
/* State::new patchify: latent (B,C,h,w) f32 -> img (B,(h/2)*(w/2),C*4) f32 and
 * img_ids (B,(h/2)(w/2),3) f32  (flux/sampling.rs:131-148). */
int fmi_pack_latents(const float* latent, int B, int C, int h, int w, float* img_out,
                     float* img_ids_out, void* stream);
/* unpack (flux/sampling.rs:162-169) fused with `img/scale_factor + shift_factor`
 * (flux/mod.rs:329): img (B,(h/2)(w/2),C*4) -> z (B,C,h,w). */
int fmi_unpack_latents(const float* img, int B, int C, int h, int w, double scale_factor,
                       double shift_factor, float* z_out, void* stream);
/* ((clamp(x,-1,1)+1)*127.5) as u8, truncating (flux/mod.rs:332, cpu_backend/mod.rs:2571-2574),
 * NCHW f32 -> NCHW u8 (interleave=0) or NHWC u8 (interleave=1, what Pipeline::forward hands
 * to RgbImage::from_raw, pipelines/mod.rs:253-266). */
int fmi_postprocess_u8(const float* image, int B, int C, int H, int W, int interleave,
                       uint8_t* out, void* stream);
/* ---- image-to-image / inpainting glue (the reference has neither) ----
 * u8 image -> f32 NCHW in [-1, 1], the mirror of fmi_postprocess_u8: in (B,C,H,W) u8 (interleaved=0) or (B,H,W,C) u8
 * (interleaved=1, what Pipeline::forward returns), x = (u + 0.5) / 127.5 - 1 in f32 — the centre of the bin that the
 * truncating post-process maps to u, so fmi_postprocess_u8(fmi_preprocess_u8(u)) == u for all 256 values (u / 127.5 - 1
 * comes back one too low on 63 of them). */
int fmi_preprocess_u8(const uint8_t* in, int B, int C, int H, int W, int interleaved, float* out, void* stream);
/* Pixel mask (B,H,W) f32 in [0,1] (1 = repaint, 0 = keep) -> latent mask (B,(H/16)(W/16),C*4) f32: the mean of every
 * 8x8 block, broadcast over the C latent channels and laid out as fmi_pack_latents lays the latents out. */
int fmi_latent_mask(const float* mask, int B, int C, int H, int W, float* out, void* stream);   /* H, W multiples of 16 */
/* The mirror of fmi_unpack_latents: z (B,C,h,w) f32 (fmi_vae_encode's output) -> x0 (B,(h/2)(w/2),C*4) f32 =
 * pack((z - shift_factor) * scale_factor), two roundings with the scalars rounded to f32, and img_ids (B,(h/2)(w/2),3)
 * as fmi_pack_latents writes them (img_ids_out may be NULL). */
int fmi_encode_latents(const float* z, int B, int C, int h, int w, double scale_factor, double shift_factor,
                       float* x0_out, float* img_ids_out, void* stream);
/* Position ids as fmi_pack_latents writes them, with a caller-chosen axis 0 and origin: ids_out (B,h2*w2,3) f32 = (id0, row0 + r, col0 + c) for the token at
 * row r, column c of the (h2, w2) grid (one f32 addition each).  (0, 0, 0) gives fmi_pack_latents' ids; a reference image's tokens take id0 = 1. */
int fmi_latent_ids(int B, int h2, int w2, float id0, float row0, float col0, float* ids_out, void* stream);
/* FlowMatchEulerDiscreteScheduler.scale_noise: out = (1 - t) * x0 + t * noise over n f32 elements, t rounded to f32 and
 * 1 - t computed once: t = 1 gives noise and t = 0 gives x0 bit for bit.  The start state of image-to-image at
 * t = timesteps[num_steps - n_run]. */
int fmi_scale_noise(const float* x0, const float* noise, double t, int64_t n, float* out, void* stream);
/* The update of fmi_flux_denoise_cfg on its own (op-level glue; device pointers, no allocation): over n f32 elements
 *   g = neg + scale * (pos - neg);  e = img + g * dt;  img = e, or with x0 / noise / mask (all three or none) mask * e + (1 - mask) * ((1 - s) * x0 + s * noise).
 * img is read and written in place.  16-byte accesses when n % 4 == 0 and every pointer is 16-byte aligned, else scalar ones: the same bits either way.
 * FMI_ERR_INVALID: a null img / pos / neg, n < 0, a scale that is negative, NaN or infinite, x0 / noise / mask given in part. */
int fmi_cfg_euler_step(float* img, const float* pos, const float* neg, float scale, float dt, int64_t n,
                       const float* x0, const float* noise, const float* mask, float s, void* stream);
/* The updates of fmi_flux_denoise_solver on their own (op-level glue; device pointers, no allocation), over n f32 elements, one pass each.
 * g(pos, neg) = pos when neg is NULL (scale is then ignored), else neg + scale * (pos - neg).  blend(e) = e without x0 / noise / mask (all three or none), else
 * mask * e + (1 - mask) * ((1 - s) * x0 + s * noise).  Every product that feeds a sum is one fused multiply-add.  16-byte accesses when n % 4 == 0 and every
 * pointer is 16-byte aligned, else scalar ones: the same bits either way.
 *   fmi_heun_predict:   g1 = g(pos, neg);  x_pred = blend(img + g1 * dt).  img is only read; img, x_pred and g1 are three buffers.
 *   fmi_heun_correct:   img = blend(img + ((g1 + g(pos, neg)) * 0.5) * dt), in place; pos / neg are the evaluation on x_pred at the target time.
 *   fmi_dpmpp_2m_step:  D = img - t * g(pos, neg);  D' = D + w * (D - history), or D when w == 0 (history is then not read);  img = blend(a * img + c * D');
 *                       history = D.  img and history are updated in place.  a, c, w: fmi_dpmpp_2m_coefficients; t: the step's time, rounded to f32.
 * FMI_ERR_INVALID: a null required pointer, n < 0, buffers that must differ given as one, with neg a scale that is negative, NaN or infinite, x0 / noise / mask
 * given in part. */
int fmi_heun_predict(const float* img, const float* pos, const float* neg, float scale, float dt, int64_t n, float* x_pred, float* g1,
                     const float* x0, const float* noise, const float* mask, float s, void* stream);
int fmi_heun_correct(float* img, const float* g1, const float* pos, const float* neg, float scale, float dt, int64_t n,
                     const float* x0, const float* noise, const float* mask, float s, void* stream);
int fmi_dpmpp_2m_step(float* img, const float* pos, const float* neg, float scale, float t, float a, float c, float w, int64_t n, float* history,
                      const float* x0, const float* noise, const float* mask, float s, void* stream);
/* Step i (0 <= i < n_steps) of the schedule's 2M scalars, computed in double and rounded once to f32: a = t_{i+1} / t_i, c = 1 - a, and
 * w = (l_{i+1} - l_i) / (2 (l_i - l_{i-1})) with l(t) = ln((1 - t) / t) — 0 when i == 0, when t_{i-1} == 1 and when t_{i+1} == 0.  Host only, no device.
 * FMI_ERR_INVALID: a null pointer, i out of range, a schedule that is not strictly decreasing inside [0, 1]. */
int fmi_dpmpp_2m_coefficients(const double* timesteps_host, int n_steps, int i, float* a, float* c, float* w);
/* ---- channel-concatenated conditioning glue (FLUX.1 Fill / Canny / Depth; device pointers, no allocation) ----
 * A column window of a wider bf16 matrix: row r of src, shaped (rows_src, cols) F32 | BF16 contiguous and read at r % rows_src, goes to
 * dst[r * dst_ld + col0 .. + cols) as bf16 (round to nearest even; a bf16 source is copied), for r in [0, rows); columns outside the window are not touched.
 * The per-step kernel of a conditioned model: the f32 state into columns [0, 64) of the (B*S, 64 + Cc) x_embedder operand, both halves of a true-CFG batch in
 * one launch (rows_src = rows / 2); the conditioning into [64, 64 + Cc) once per call.  16-byte accesses when src and dst are 16-byte aligned, else scalar.
 * FMI_ERR_INVALID: cols, dst_ld or col0 not a multiple of 8, a window that leaves the row, rows_src not dividing rows, a dtype that is not F32 / BF16. */
int fmi_cast_cols_bf16(const void* src, fmi_dtype dt, int64_t rows, int64_t rows_src, int cols, void* dst_bf16, int dst_ld, int col0, void* stream);
/* The masked image of a Fill request: out (B,C,H,W) = image * (1 - b), b = mask >= 0.5 ? 1 : 0 with mask (B,H,W) f32, 1 = fill — diffusers' mask processor
 * binarises, then FluxFillPipeline takes image * (1 - mask). */
int fmi_mask_image(const float* image, const float* mask, int B, int C, int H, int W, float* out, void* stream);
/* The 320 conditioning channels of FLUX.1 Fill: cond_out (B,S,320) f32, S = (H/16)(W/16), H and W multiples of 16.  Columns [0, 64) are masked_latents (B,S,64),
 * the packed VAE latents of the masked image; columns [64, 320) the binarised mask (B,H,W), pixel-unshuffled by 8 and packed 2x2 like the latents:
 *   cond[b, i*(W/16) + j, 64 + (py*8 + px)*4 + dy*2 + dx] = (mask[b, 16i + 8dy + py, 16j + 8dx + px] >= 0.5)       py, px in 0..7, dy, dx in 0..1
 * == mask.view(B,h,8,w,8).permute(0,2,4,1,3).reshape(B,64,h,w) followed by fmi_pack_latents. */
int fmi_fill_condition(const float* masked_latents, const float* mask, int B, int H, int W, float* cond_out, void* stream);
/* Deterministic N(0,1) latents from a counter-based Philox4x32-10 generator
 * (the reference's RNG is unseedable; this is the explicit-seed extension).
 * Elements 4q..4q+3 of sample b come from the four words of philox(counter = (q lo, q hi, s lo, s hi),
 * key = (seed lo, seed hi)), s = first_sample + b: words (0,1) and (2,3) each feed one Box-Muller pair,
 * u = f32(f32(word >> 8) + 0.5f) * 2^-24 (f32 roundings included), z = sqrt(-2 ln u1) * (cos, sin)(2 pi u2).  Replaces get_noise
 * (pipelines/flux/sampling.rs:5-14). */
int fmi_randn(float* out, int64_t n_per_sample, int B, uint64_t seed, uint64_t first_sample,
              void* stream);
/* The raw 32-bit words fmi_randn draws from, same indexing (out (B, n_per_sample) u32): integer work,
 * bit-exact against the oracle's Philox, which is pinned by Random123's known-answer vectors. */
int fmi_philox_u32(uint32_t* out, int64_t n_per_sample, int B, uint64_t seed, uint64_t first_sample,
                   void* stream);

/* Host-side schedule helpers (f64, bit-for-bit the reference formulas). */
double fmi_calculate_shift(int image_seq_len, int base_seq_len, int max_seq_len,
                           double base_shift, double max_shift); /* flux/sampling.rs:171-181 */
typedef struct fmi_scheduler_config { /* SchedulerConfig, pipelines/scheduler.rs:4-20 */
  int base_image_seq_len; double base_shift; int max_image_seq_len; double max_shift;
  double shift; int use_dynamic_shifting;
} fmi_scheduler_config;
/* out_host[num_steps+1]; mu is ignored unless use_dynamic_shifting. (scheduler.rs:28-51) */
int fmi_get_timesteps(const fmi_scheduler_config* cfg, int num_steps, double mu, double* out_host);

/* ------------------------------------------------------------------------------------
 * Operator-level entry points (seam S3) — used by the parity tests and
 * usable as CustomOp::cuda_fwd replacements.
 * ---------------------------------------------------------------------------------- */
typedef enum fmi_epilogue {
  FMI_EPI_NONE = 0,      /* y = x W^T (+bias) */
  FMI_EPI_GELU_TANH = 1, /* y = gelu_tanh(x W^T + bias)  (Mlp, model.rs:459-463) */
  FMI_EPI_SILU = 2
} fmi_epilogue;

/* y(M,N) = epi(x(M,K) · W(N,K)^T + bias(N)); x,W,y bf16, bias bf16 or NULL, f32 accumulate.
 * == UnquantLinear::forward (unquantized/mod.rs:34-77). K % 64 == 0 required. */
int fmi_linear_bf16(const void* x, const void* w, const void* bias, void* y, int M, int N,
                    int K, fmi_epilogue epi, void* stream);
/* Same with a bitsandbytes 4-bit weight: W = dequant(packed, absmax, blocksize) fused into
 * the GEMM's weight-tile load (BnbLinear::forward semantics, bitsandbytes/mod.rs:301-312,
 * minus the dense round trip).  quant_type 1=fp4, 2=nf4. K % 64 == 0, blocksize % 64 == 0. */
int fmi_linear_bnb4_bf16(const void* x, const uint8_t* packed, const float* absmax,
                         int blocksize, int quant_type, const void* bias, void* y, int M,
                         int N, int K, fmi_epilogue epi, void* stream);
/* Same with an LLM.int8 weight (BnbLinear::Int8, bitsandbytes/mod.rs:104-134, 293-300): W = weight_i8 * SCB[row] / 127
 * (dequantize_8bit, dequant.cu:205-214) expanded inside the GEMM's weight-tile stage, bit-identical to the stand-alone
 * dequant followed by fmi_linear_bf16.  weight (N,K) int8 row-major, 16-byte aligned; scb (N) f32.  K % 64 == 0. */
int fmi_linear_int8_bf16(const void* x, const int8_t* weight, const float* scb, const void* bias, void* y,
                         int M, int N, int K, fmi_epilogue epi, void* stream);
/* Row-wise dynamic e4m3 quantisation: scale[r] = max(absmax(x[r,:]), 1e-30) / 448,
 * out[r,k] = e4m3_rne(x[r,k] * (448 / max(absmax, 1e-30))).  x (rows,K) bf16, out (rows,K) u8, K % 8 == 0,
 * K <= 16384.  Used for weights (row = output channel) and activations (row = token). */
int fmi_quantize_rows_fp8(const void* x, int rows, int K, uint8_t* out, float* scale, void* stream);
/* y(M,N) = epi((xq · Wq^T) * xs[m] * ws[n] + bias), xq/xs = fmi_quantize_rows_fp8(x) computed internally,
 * Wq (N,K) e4m3 + ws (N) from fmi_quantize_rows_fp8(W); y bf16, f32 accumulate on the fp8 MFMA.
 * N > 128, K % 128 == 0. */
int fmi_linear_fp8(const void* x, const uint8_t* wq, const float* w_scale, const void* bias, void* y, int M, int N,
                   int K, fmi_epilogue epi, void* stream);
/* The int8 forms of the two (fmi_flux_quantize_int8's recipe; oracle: orc_quantize_rows_i8 / orc_linear_i8): scale[r] =
 * max(absmax, 1e-30) / 127, out[r,k] = clamp(rint(x[r,k] * (127 / max(absmax, 1e-30))), -127, 127); y = epi(float(xq · Wq^T as an exact
 * int32) * (xs[m] * ws[n]) + bias) on v_mfma_i32_32x32x32_i8.  Same shape rules. */
int fmi_quantize_rows_i8(const void* x, int rows, int K, int8_t* out, float* scale, void* stream);
int fmi_linear_i8(const void* x, const int8_t* wq, const float* w_scale, const void* bias, void* y, int M, int N,
                  int K, fmi_epilogue epi, void* stream);
/* Caller-owned workspace forms of the two (the reference's convention: the caller allocates, bitsandbytes/op.rs:204-228): `workspace`
 * = at least fmi_linear_q8_workspace_bytes(M, K) bytes of device memory, 256-byte aligned, that must stay untouched until the call's work
 * has run on `stream`.  fmi_linear_fp8 / fmi_linear_i8 above are these with the workspace taken from a grow-only block the
 * library keeps per (device, stream): every form is asynchronous on the stream — a call allocates only if it needs more than any earlier
 * call on that stream did (once, without waiting for the stream), and none synchronises the host. */
size_t fmi_linear_q8_workspace_bytes(int M, int K);
int fmi_linear_fp8_ws(const void* x, const uint8_t* wq, const float* w_scale, const void* bias, void* y, int M, int N, int K,
                      fmi_epilogue epi, void* workspace, size_t workspace_bytes, void* stream);
int fmi_linear_i8_ws(const void* x, const int8_t* wq, const float* w_scale, const void* bias, void* y, int M, int N, int K,
                     fmi_epilogue epi, void* workspace, size_t workspace_bytes, void* stream);
/* The 8-bit GEMM alone on operands the caller already quantised with fmi_quantize_rows_fp8 (kind 1) / fmi_quantize_rows_i8 (kind 2):
 * y(M,N) bf16 = epi(acc(xq · wq^T) * x_scale[m] * w_scale[n] + bias); stream-ordered, no allocation (the form a caller that keeps
 * activations quantised between layers binds; also what tools/hipblaslt_yardstick.py times against the vendor library's fp8 GEMM). */
int fmi_gemm_q8(const void* xq, const float* x_scale, const void* wq, const float* w_scale, const void* bias, void* y,
                int M, int N, int K, int kind, fmi_epilogue epi, void* stream);
/* The int8 recipe's form for POST-GELU operands (round 5; oracle: orc_quantize_rows_i8_asym / orc_linear_i8_asym).  gelu(h) >= -0.17, so a grid
 * symmetric around 0 wastes half of its codes there.  Columns [0, d0) of a row (a signed segment in front — the single blocks' linear2 reads
 * cat(attention, gelu(mlp)), d0 = 3072; d0 = 0 for none) stay symmetric, columns [d0, K) take 256 levels over their [min, max] = [lo, hi], all with
 * ONE step per row so the product stays one exact int32 sum:
 *   scale[r] = s = max(max((hi - lo) / 255, absmax(front) / 127), 1e-30);  offset[r] = lo + 128 s
 *   k <  d0: out = clamp(rint(x / s), -127, 127)            k >= d0: out = clamp(rint((x - lo) / s), 0, 255) - 128
 *   fmi_rowsum_i8:    w_sum[n] = w_scale[n] * float(sum_{k >= d0} wq[n,k])      (once per weight)
 *   fmi_gemm_i8_asym: y = epi(float(xq · wq^T) * (x_scale[m] * w_scale[n]) + x_offset[m] * w_sum[n] + bias[n])
 * x (rows,K) bf16, K % 8 == 0, K <= 16384, d0 % 16 == 0; GEMM shape rules as fmi_gemm_q8.  What fmi_flux_quantize_int8 uses in front of the double
 * blocks' MLP-out and the single blocks' linear2.  Stream-ordered, nothing allocated. */
int fmi_quantize_rows_i8_asym(const void* x, int rows, int K, int d0, int8_t* out, float* scale, float* offset, void* stream);
int fmi_rowsum_i8(const int8_t* wq, const float* w_scale, int N, int K, int d0, float* w_sum, void* stream);
/* The smoothed int8 recipe (fmi_flux_calibrate_int8) at the op level (ABI 6): fmi_quantize_rows_i8_scaled = fmi_quantize_rows_i8 (d0 < 0; `offset` unused)
 * or fmi_quantize_rows_i8_asym (d0 >= 0) on x[r, k] * col_scale[k], the product taken in f32 (col_scale: K floats, 16-byte aligned; 1 / s for an
 * activation, s for a weight).  fmi_col_absmax folds max_r |x[r, k]| of a bf16 matrix (rows, K) with row stride ld into amax_inout[k] (a running maximum:
 * zero it first; K, ld % 8 == 0) — the statistic s[k] = sqrt(amax_x[k] / amax_W[k]) is made of. */
int fmi_quantize_rows_i8_scaled(const void* x, int rows, int K, int d0, const float* col_scale, int8_t* out, float* scale, float* offset, void* stream);
int fmi_col_absmax(const void* x, int rows, int K, int ld, float* amax_inout, void* stream);
int fmi_gemm_i8_asym(const void* xq, const float* x_scale, const float* x_offset, const void* wq, const float* w_scale, const float* w_sum,
                     const void* bias, void* y, int M, int N, int K, fmi_epilogue epi, void* stream);
/* TEST SEAMS into the GEMM launcher (ABI 6; tests/test_gpu_gemm_epilogues.py) — not part of the product surface.  The entries above reach three
 * of the launcher's eight epilogues, one problem per launch, dense leading dimensions; the rest (gated f32 residual update with per-batch gate
 * rows, GELU from a column on, f32 store / scaled store, the int8 offset term, strided operands, grouped launches, the split-K reduce) otherwise
 * runs only inside the models.  fmi_gemm_group hands 1 .. 8 descriptors to the launcher as ONE grouped launch:
 *   pre[m, n] = alpha * sum_k a[m, k] w[n, k]   (q8 != 0: the 8-bit sum * a_scale[m] * w_scale[n] + a_off[m] * w_sum[n], then * alpha)  + bias[n]
 *   FMI_GEMM_STORE_BF16 / _GELU_BF16 / _SILU_BF16: out bf16 = act(pre)           (alpha: STORE_F32 and SCALE_BF16 only, exactly 1 elsewhere)
 *   FMI_GEMM_RESID_GATE_F32: out f32 (read-modify-write) += gate_b[n] * pre,  gate_b = gate + (rows_per_batch > 0 ? m / rows_per_batch : 0) * gate_bstride
 *   FMI_GEMM_GELU_FROM_COL:  out bf16 = n >= gelu_from ? gelu(pre) : pre      (gelu_from % 4 == 0)
 *   FMI_GEMM_STORE_F32 / _SCALE_BF16: out f32 / bf16 = pre                    FMI_GEMM_RESID_ADD_BF16: out bf16 = resid[m * ldo + n] + pre
 * a (M, K) and w (N, K) bf16 (q8 = 1: OCP e4m3 bytes, 2: int8; then N > 128, K % 128 == 0, lda / ldw % 16 == 0, both scale vectors; a_off / w_sum
 * int8 only, both or neither), 16-byte aligned, leading dimensions in elements (>= K, multiples of 8); K % 64 == 0; bias (N) bf16 or NULL;
 * gate f32, 16-byte aligned, gate_bstride % 4 == 0; ldo >= N.  All problems of a group share q8 and the activation kind (none / GELU /
 * GELU from a column / the rest).  Everything is checked on the host before anything is launched: FMI_ERR_INVALID, nothing written.
 * fmi_splitk_resid_gate is the second kernel of the split-K latency mode (fmi_flux_set_split_k): out[m, n] += gate_b[n] * (parts_0 + ... + parts_{S-1}
 * + bias[n]), parts (S, M, N) f32 contiguous added in index order; N, ldo % 4 == 0, out and parts 16-byte aligned.
 * fmi_set_gemm_kernel picks, PROCESS-WIDE, the kernel of the dense bf16 launches wider than 128 columns: pingpong = 1 (default) the ping-pong kernel,
 * 0 its double-buffered predecessor; w4 = 1 sends the residual-update launches to the 4-wave kernel.  The three are bit-identical; the two
 * alternatives live in the test build — in the product library a launch that would need one fails with FMI_ERR_UNSUPPORTED. */
typedef enum fmi_gemm_epi {
  FMI_GEMM_STORE_BF16 = 0,
  FMI_GEMM_GELU_BF16 = 1,
  FMI_GEMM_RESID_GATE_F32 = 2,
  FMI_GEMM_GELU_FROM_COL = 3,
  FMI_GEMM_STORE_F32 = 4,
  FMI_GEMM_SCALE_BF16 = 5,
  FMI_GEMM_RESID_ADD_BF16 = 6,
  FMI_GEMM_SILU_BF16 = 7
} fmi_gemm_epi;
typedef struct fmi_gemm_desc {
  const void* a;
  const void* w;
  const void* bias;
  void* out;
  const float* gate;
  const void* resid;
  int M, N, K;
  int lda, ldw, ldo;
  int epi; /* fmi_gemm_epi */
  int gelu_from;
  float alpha;
  int rows_per_batch;
  int gate_bstride;
  int q8; /* 0 bf16, 1 e4m3, 2 int8 */
  const float* a_scale;
  const float* w_scale;
  const float* a_off;
  const float* w_sum;
} fmi_gemm_desc;
int fmi_gemm_group(const fmi_gemm_desc* probs, int nprob, void* stream);
int fmi_splitk_resid_gate(const float* parts, int S, const void* bias, const float* gate, int rows_per_batch, int gate_bstride, float* out, int ldo,
                          int M, int N, void* stream);
int fmi_set_gemm_kernel(int pingpong, int w4);
/* Tile heights of the dense bf16 ping-pong GEMM kernel, PROCESS-WIDE (a test / ablation hook like fmi_set_gemm_kernel; FMI_GEMM_ROWS=<n> in the
 * environment sets the initial value): 0 (default) = chosen per launch by a scheduling model — 256-row tiles, with the last rows of a problem in
 * 192-row tiles where that saves at least a quarter round of the CUs; 256 = 256-row tiles only; 192 = 192-row tiles only; 448 = 256-row tiles
 * while at least 448 rows remain, 192-row tiles for the rest (a mixed launch at any size).  Rows are split, never K: every setting gives the same
 * bits.  Other kernels have one height and ignore it.  Anything else: FMI_ERR_INVALID.
 * fmi_gemm_tile_rows is the model alone (pure, no device): for a group of nprob <= 8 problems (M[i], N[i]) on `cus` compute units, operands q8
 * (0 = bf16: the kernel above; 1 / 2: an 8-bit kernel, one height) and a setting `mode` as above, the numbers of 256-row and 192-row tiles along
 * M per problem, the first workgroup id of each problem's 256-row and 192-row tiles in the launch order (nprob + 1 entries each, the last = the
 * end of that region; all 256-row tiles come first) and the modelled makespan in quarters of a 256-row tile's time. */
int fmi_set_gemm_rows(int rows);
int fmi_gemm_tile_rows(const int* M, const int* N, int nprob, int cus, int q8, int mode, int* n256, int* n192, int* tall_start, int* short_start,
                       int* quarters);
/* softmax(q k^T * scale) v, q,k,v,o (B,H,L,d) bf16, d == 128, non-causal; o is written
 * token-major (B,L,H*d) when `out_token_major`, else (B,H,L,d).
 * == backend::ops::sdpa fallback (ops.rs:247-262) without materialising the scores. */
int fmi_sdpa_bf16(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq,
                  int Lk, int d, float scale, int out_token_major, void* stream);
/* The attention kernels read V transposed (B,H,128,Lk rounded up to 64) with the kv index permuted inside groups of 16; the op-level
 * entry points build that image first.  fmi_sdpa_bf16 / fmi_sdpa_fp8qk keep it in a grow-only block the library holds per (device, stream)
 * — calls on one stream run in order and share it; a call allocates only when it needs more than any earlier call on that stream (once,
 * without waiting for the stream) and none synchronises the host: a host that binds ops::sdpa to them enqueues 57 calls per denoise step
 * without ever waiting —; the *_ws forms take it from the caller
 * (fmi_sdpa_workspace_bytes(B, H, Lk) bytes, 16-byte aligned, untouched until the call's work has run on `stream`). */
size_t fmi_sdpa_workspace_bytes(int B, int H, int Lk);
/* Threads (ABI 6): an entry that uses the library-held block takes one lock from the moment it picks the block until its last kernel is enqueued, so
 * host threads that share a stream cannot interleave their launches around it; the block is keyed by (device, stream), NULL and hipStreamLegacy being
 * one stream and hipStreamPerThread one stream PER calling thread.  fmi_release_scratch returns every such block to the driver: it drains the
 * devices that hold one first (the only op-level entry that waits; for teardown or memory pressure) and reports the bytes freed
 * (`freed_bytes` may be NULL).  The next op-level call allocates again. */
int fmi_release_scratch(size_t* freed_bytes);
int fmi_sdpa_bf16_ws(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk, int d, float scale,
                     int out_token_major, void* workspace, size_t workspace_bytes, void* stream);
/* Process-wide choice of the bf16 attention kernel (test / benchmark hook):
 *   5 (default) round 4's lock-step schedule of kernel 3 (attention_w16l.h: the wave's four 16-query blocks walk a KV tile together, one
 *     K / V^T fragment read feeds four MFMAs) — the arithmetic of 3 / 4; bit-identical to them when every tile rescales, equal to
 *     rounding otherwise (the deferred-rescale decision is taken over 64 queries instead of 32);
 *   3 one wave per SIMD on v_mfma_f32_16x16x32_bf16, the whole KV stream generated assembly (attention_w16.h);
 *   4 the same design on v_mfma_f32_32x32x16_bf16 (attention_w32.h) — 3 and 4 are bit-identical to each other;
 *   2 round 2's one-wave kernel (attention_w4.h), 1 the 8-wave ping-pong kernel, 0 the 8-wave single-barrier kernel — these
 *   three are bit-identical to each other, and equal to 3 / 4 to rounding (3 / 4 round q * scale * log2(e) to bf16 once and
 *   normalise by the sum of the bf16-rounded probabilities: rel-L2 ~3e-3 between the families, both within the oracle tolerance). */
int fmi_set_attention_kernel(int kind);
/* Same with q and k as OCP e4m3 bytes (B,H,L,128): QK^T on the fp8 MFMA, softmax / P / V in f32 / bf16 as above.
 * `scale` must include 1 / (q scale * k scale).  The fp8-mode attention of fmi_flux_* (fmi_flux_set_fp8_attention). */
int fmi_sdpa_fp8qk(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq,
                  int Lk, int d, float scale, int out_token_major, void* stream);
/* The one-wave fp8 streams carry the score factor scale * log2(e) in the MFMA's E8M0 block scale, so they serve factors 2^n,
 * n = -126 .. 0; anything else runs the 8-wave kernel (slower; counted in fmi_device_info's "fp8_attention_fallbacks").  A caller that
 * KNOWS its factor is 2^n says so as an integer: score_exp2 = n (then `scale` is not read); FMI_SDPA_NO_EXP2 = derive it from `scale`
 * (accepted when f32(scale * log2 e) is a power of two or one ulp beside one, which is where scale = 2^n / log2(e) built in f32 lands). */
#define FMI_SDPA_NO_EXP2 (1 << 30)
int fmi_sdpa_fp8qk_ws(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk, int d, float scale,
                      int score_exp2, int out_token_major, void* workspace, size_t workspace_bytes, void* stream);
/* Round 5: every operand of both products as OCP e4m3 — q, k bytes as fmi_sdpa_fp8qk; v is handed over as bf16 (B,H,Lk,128) and enters the
 * second product as e4m3(clamp(v * v_scale, +-448)); the probabilities exp2(s - m) are rounded to e4m3 as they are (the deferred rescale keeps them
 * <= 64), the row sums are taken over the rounded values, and 1 / v_scale leaves with the final normalisation.  Both products run on the
 * K = 128 / K = 64 fp8 MFMA at twice the bf16 rate (attention_w16l_kernel<.., true, true>).  Needs score_exp2 (or a `scale` that is a power of
 * two as above) and Lk > 64 — FMI_ERR_UNSUPPORTED otherwise: no other kernel reads this V^T.  An OP-LEVEL entry only: the model's 8-bit modes keep
 * bf16 P and V (the stream is issue-bound, the e4m3 second product buys no time: DESIGN 4.4), and fmi_flux_set_fp8_attention rejects 3.
 * Workspace: fmi_sdpa_workspace_bytes (half of it is used). */
int fmi_sdpa_fp8(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk, int d, float scale, int score_exp2,
                 float v_scale, int out_token_major, void* stream);
int fmi_sdpa_fp8_ws(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk, int d, float scale, int score_exp2,
                    float v_scale, int out_token_major, void* workspace, size_t workspace_bytes, void* stream);
/* LayerNorm(eps, no affine) then x*(1+scale)+shift: x (rows,D) f32 -> out bf16;
 * scale/shift f32 (D) (layer_norm helper model.rs:33-38 + ModulationOut::scale_shift :218-221).
 * scale/shift may be NULL (plain LN). */
int fmi_layernorm_mod(const float* x, const float* scale, const float* shift, void* out_bf16,
                      int rows, int D, float eps, void* stream);
/* The small f32 pieces of Flux::forward, one at a time (ABI 6; the kernels the model itself launches):
 * timestep_embedding (model.rs:104-122): t (B) f32 -> out (B, dim) f32 = [cos(1000 t f_i), sin(1000 t f_i)], f_i = exp(-ln(1e4) i / (dim/2)) in f32. */
int fmi_timestep_embedding(const float* t, int B, int dim, float* out, void* stream);
/* EmbedNd / rope (model.rs:65-102, 124-163): ids (B,T,3) and (B,S,3) f32 (either count may be 0) -> pe (B, T+S, sum(axes_dim)/2, 2) f32 = {cos, sin} of
 * pos * inv_freq, text rows first; inv_freq = 1f32 / f32(theta^(2j/dim) evaluated in f64) as model.rs:71-74.  (The reference materialises the 2x2
 * rotation [cos, -sin, sin, cos]; this table keeps its two distinct entries.) */
int fmi_rope_table(const float* txt_ids, const float* img_ids, int B, int T, int S, const int* axes_dim /*[3]*/, int theta, float* pe, void* stream);
/* QkNorm (RmsNorm over the head dim, eps 1e-6, model.rs:186-209) + apply_rope (model.rs:52-63) in front of the attention: q, k (B, L, ld >= H*128)
 * bf16 token-major (head h at columns h*128..), weights (128) bf16, pe (B, L, 64, 2) f32 from fmi_rope_table -> q_out, k_out (B, H, L, 128)
 * head-major, bf16 (out_dtype FMI_BF16: the operands the attention reads; the q|k|v GEMM's fused epilogue produces the same bits) or f32
 * (FMI_F32: the same arithmetic without the final rounding).  d must be 128; every pointer 16-byte aligned. */
int fmi_rmsnorm_rope(const void* q, const void* k, int ld, const void* q_weight, const void* k_weight, const float* pe, void* q_out, void* k_out,
                     int B, int H, int L, int d, fmi_dtype out_dtype, void* stream);
/* GroupNorm (+optional SiLU) on NHWC bf16 activations, f32 two-pass statistics
 * (nn/group_norm.rs:39-74): x (B,HW,C). */
int fmi_groupnorm_nhwc(const void* x_bf16, const float* weight, const float* bias, void* out_bf16,
                       int B, int HW, int C, int groups, float eps, int fuse_silu, void* stream);
/* 3x3/1x1 stride-1 conv, zero pad k/2, NHWC bf16, weights (Cout,kh,kw,Cin) bf16, bias bf16 (Cout)
 * or NULL; Cin % 64 == 0 (zero-pad the channels);
 * optional nearest-2x upsample folded into the input gather (Upsample::forward vae.rs:223-229)
 * and optional residual add (ResnetBlock::forward vae.rs:157-172). (in_h,in_w) is the stored
 * input size; output is (in_h*(up?2:1), in_w*(up?2:1)). */
int fmi_conv2d_nhwc(const void* x_bf16, const void* w_bf16, const void* bias_bf16,
                    const void* residual_bf16, void* out_bf16, int B, int in_h, int in_w, int Cin,
                    int Cout, int ksize, int upsample2x, void* stream);

/* The reference's own extern "C" convention, kept verbatim so ffi.rs:5-114 binds without
 * edits (CUstream -> hipStream_t).  n = number of OUTPUT elements; blocksize as stored in
 * quant_state; `code` is the 256-entry map for int8 and ignored for fp4/nf4 (the kernels
 * use the constant tree/LUT of dequant.cu:12-92). */
void dequantize_blockwise_f32_int8(const float* code, const uint8_t* A, const float* absmax, float* out, int blocksize, int n, void* stream);
void dequantize_blockwise_f32_fp4(const float* code, const uint8_t* A, const float* absmax, float* out, int blocksize, int n, void* stream);
void dequantize_blockwise_f32_nf4(const float* code, const uint8_t* A, const float* absmax, float* out, int blocksize, int n, void* stream);
void dequantize_blockwise_f16_int8(const float* code, const uint8_t* A, const float* absmax, void* out, int blocksize, int n, void* stream);
void dequantize_blockwise_f16_fp4(const float* code, const uint8_t* A, const float* absmax, void* out, int blocksize, int n, void* stream);
void dequantize_blockwise_f16_nf4(const float* code, const uint8_t* A, const float* absmax, void* out, int blocksize, int n, void* stream);
void dequantize_blockwise_bf16_int8(const float* code, const uint8_t* A, const float* absmax, void* out, int blocksize, int n, void* stream);
void dequantize_blockwise_bf16_fp4(const float* code, const uint8_t* A, const float* absmax, void* out, int blocksize, int n, void* stream);
void dequantize_blockwise_bf16_nf4(const float* code, const uint8_t* A, const float* absmax, void* out, int blocksize, int n, void* stream);
/* LLM.int8 weight: out[i] = w[i]*SCB[i/col]/127 (dequant.cu:205-232). The reference
 * launches these on the legacy default stream; so do we (stream argument absent, as in ffi.rs). */
void dequantize_8bit_kernel_f32(const int8_t* weight, const float* scb, float* out, int row, int col, int n);
void dequantize_8bit_kernel_f16(const int8_t* weight, const float* scb, void* out, int row, int col, int n);
void dequantize_8bit_kernel_bf16(const int8_t* weight, const float* scb, void* out, int row, int col, int n);

/* ------------------------------------------------------------------------------------
 * Small device-memory helpers so a non-HIP host (Rust, ctypes) needs nothing else.
 * ---------------------------------------------------------------------------------- */
int fmi_malloc(void** dptr, size_t bytes);
int fmi_free(void* dptr);
int fmi_memcpy(void* dst, const void* src, size_t bytes, void* stream); /* hipMemcpyDefault, async */
int fmi_memset(void* dst, int value, size_t bytes, void* stream);
int fmi_stream_synchronize(void* stream);
/* Event timing on an arbitrary stream (bench.py uses these so the timed region is measured
 * on the stream the kernels are launched on). */
int fmi_event_create(void** ev);
int fmi_event_record(void* ev, void* stream);
int fmi_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
int fmi_event_destroy(void* ev);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* FLUX_MI355X_H */
