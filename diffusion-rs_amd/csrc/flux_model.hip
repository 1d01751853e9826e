// flux_model.hip — host side of the FLUX DiT: weight arenas, diffusers-name resolution, and the
// kernel schedule of Flux::forward (diffusion_rs_core/src/models/flux/model.rs:790-833) and
// Sampler::sample (pipelines/sampling.rs:25-48).
//
// Memory plan (MI355X, 288 GB HBM3E): weights live in four arenas holding FUSED matrices — [q|k|v] per stream of a
// double block, [q|k|v|proj_mlp] per single block, and ONE (344*D, D) matrix with every modulation linear of the
// model so all AdaLN vectors of an image come from a single weight-streaming GEMM:
//   BASE    embedders, final projection, QkNorm weights, every bias            (always allocated, ~0.3 GB)
//   MOD     the modulation matrix in bf16 (6.5 GB)                             (allocated when a dense part arrives)
//   BLOCKS  the block linears in bf16 (17.0 GB)                                (allocated when a dense part arrives)
//   Q4      the same matrices as bitsandbytes nf4 / fp4 codes + f32 absmax     (allocated when a 4-bit part arrives)
// LLM.int8 matrices, ggml blocks (4.5 to 8.5 bits per weight) and 8-bit float codes do not fit Q4's slots: the matrix owns them (struct Dense),
// so a bf16 checkpoint occupies 23.8 GB and an nf4 one 6.7 GB — no bf16 duplicate of a quantised layer is resident
// unless the caller asks for the expanded cache (fmi_flux_set_quant_dense_cache).  The arenas are also the unit of
// the multi-GPU weight broadcast (fmi_flux_state_*).  Activations live in a per-(B,S,T) workspace that is allocated
// once and reused by every step; nothing is allocated inside a step.
#include <algorithm>
#include <cstring>
#include <map>
#include <set>
#include <cmath>
#include <cstring>
#include <vector>

#include <dlfcn.h>

#include "common.h"
#include "ip_adapter.h"
#include "quant_kinds.h"

using namespace fmi;

namespace {

enum ArenaId { AR_BASE = 0, AR_MOD, AR_BLOCKS, AR_Q4, AR_COUNT };
struct Arena {
  DeviceBuffer base;
  size_t bytes = 0;  // layout size (known before the arena is allocated)
};
struct Dense {  // one (possibly fused) Linear: W (N,K) bf16 row-major, bias (N) bf16
  bf16_t* w = nullptr;  // null until the arena `ar` is allocated
  bf16_t* b = nullptr;  // BASE arena
  int N = 0, K = 0;
  int ar = AR_BASE;
  size_t w_off = 0, q_off = 0, am_off = 0;  // byte offsets in `ar` / in Q4 (packed codes, absmax sized for blocksize 64)
  // Quantised form, used instead of w when q_type != 0: the PartState (quant_kinds.h) that every part holds, set by finalize().  Where each kind lives:
  //   fp4, nf4     wq / absmax = the matrix's slot of the Q4 arena: packed codes (N, K / 2) + f32 absmax per blocksize weights
  //   LLM.int8     wq / absmax = own_wq / own_absmax: int8 (N, K) + SCB (N), allocated with the matrix's first int8 part and kept from then on
  //   gguf, f8     gq[part]: the part's ggml blocks or 8-bit float codes, one allocation per part (the parts of one matrix may differ in type and in
  //                scale until finalize() decides; empty on a matrix that never saw such a part), gscale[part]: the f8 scale (1 for ggml blocks)
  uint8_t* wq = nullptr;  // what the kernels read
  float* absmax = nullptr;
  DeviceBuffer own_wq, own_absmax;
  int q_type = 0, q_blocksize = 0;
  std::vector<DeviceBuffer> gq;
  std::vector<float> gscale;
  // optional fp8 form (fmi_flux_quantize_fp8): e4m3 (N,K) + per-output-channel f32 scale, used instead of w
  uint8_t* w8 = nullptr;
  float* w8_scale = nullptr;
  // int8 mode, linears whose input is a post-GELU operand (the double blocks' MLP-out: d0 = 0; the single blocks' linear2 over
  // cat(attention, gelu(mlp)): d0 = D): the input rows carry an offset segment from column w8_d0 on (fp8.hip's header) and
  // w8_sum[n] = w8_scale[n] * sum_{k >= w8_d0} w8[n,k] is the column factor of the offset term.  w8_d0 < 0: symmetric rows.
  float* w8_sum = nullptr;
  int w8_d0 = -1;
  // smoothed int8 recipe (round 6; fp8.hip's header): sm_amax[k] = max |input[:, k]| seen by the calibration evaluations (fmi_flux_calibrate_int8);
  // at quantise time s[k] = sqrt(amax[k] / max_n |W[n, k]|), the codes are taken from W * s and the rows of the input from x / s (sm_inv; null = unsmoothed)
  float* sm_amax = nullptr;
  float* sm_s = nullptr;
  float* sm_inv = nullptr;        // == sm_inv_store once the linear has been quantised with smoothing
  float* sm_inv_store = nullptr;
  // the named Linears this matrix is made of (rows r0 .. r0+rows) and what each was loaded as
  struct Part {
    int r0, rows;
    uint8_t state;
    int blocksize;
  };
  std::vector<Part> parts;
};

struct Dest {  // where a named tensor lands
  Dense* d;    // weight / bias of part `part` of a Dense, or null: `ptr` directly (QkNorm weights)
  int part;
  bool bias;
  void* ptr;
  int64_t numel;
  int rows, cols;  // expected shape (cols == 0 -> 1-D of `rows`)
};

enum Phase { PH_EMBED = 0, PH_MOD, PH_LN, PH_GEMM_QKV, PH_RELAYOUT, PH_ATTN, PH_GEMM_PROJ, PH_GEMM_MLP, PH_FINAL, PH_COUNT };
const char* kPhaseNames[PH_COUNT] = {"embed", "modulation", "layernorm_mod", "gemm_qkv", "qk_norm_rope_vT", "attention",
                                     "gemm_proj", "gemm_mlp", "final_layer"};

}  // namespace

struct fmi_flux {
  fmi_flux_config cfg;
  int cond = 0;  // fmi_flux_create_cond: conditioning channels concatenated to the state's for x_embedder; cfg.in_channels stays the state's width
  int D, M, H;
  int device = 0;
  Arena arena[AR_COUNT];
  size_t cursor[AR_COUNT] = {0, 0, 0, 0};  // layout cursors
  std::vector<Dense*> fused;  // every Dense whose parts can arrive quantised (block linears + the modulation matrix), fixed order
  bool finalized = false;
  // weights
  Dense img_in, txt_in, time1, time2, guid1, guid2, vecin1, vecin2, final_proj;
  Dense mod_all;  // (n_mod, D)
  struct DoubleW {
    Dense qkv[2], proj[2], mlp1[2], mlp2[2];  // [0]=img, [1]=txt
    bf16_t* nq[2];
    bf16_t* nk[2];
    int64_t mod_off[2];
  };
  struct SingleW {
    Dense w1, w2;
    bf16_t* nq;
    bf16_t* nk;
    int64_t mod_off;
  };
  std::vector<DoubleW> dbl;
  std::vector<SingleW> sgl;
  int64_t mod_final_off = 0, n_mod = 0;
  std::map<std::string, Dest> names;
  MissingSet missing;
  // workspace
  struct WS {
    int B = 0, S = 0, T = 0;
    DeviceBuffer base;
    float *x_img, *x_txt, *x_txt0, *x, *vec, *mod, *temb, *h1, *yf, *pe, *img_f32, *pred_tmp, *tv;  // x_txt0: txt_in(txt), the same at every step of an image
    bf16_t *img_bf, *txt_bf, *xm, *qkv_img, *qkv_txt, *big, *Qh, *Kh, *Vt, *attn_img, *attn_txt, *hid, *vec_bf;
    uint8_t* a8 = nullptr;  // fp8 mode: the current GEMM input, rows [txt | img], (B*L, <= D+M) e4m3
    float* a8s = nullptr;   //           its per-token scales (B*L)
    float* a8o = nullptr;   // int8 mode: the per-token offsets of a post-GELU input (B*L; Dense::w8_d0)
    int Lpad = 0;
  } ws;
  // profiling
  bool profiling = false;
  // Experiment (FMI_TWO_STREAMS=1, read at create): the image and text chains of a double block between two attentions
  // (proj -> LayerNorm -> MLP) run on two streams so that the text chain's small launches fill the partial rounds of the image chain
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool two_streams = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float phase_ms[PH_COUNT] = {0};
  int attn_thr = 96;
  int attn_kind = -1;  // fmi_flux_set_attention_kernel: 0..5 = this handle's attention kernel, -1 = follow the process-wide switch
  // 4-bit weights, large-M regime: per-layer streaming dequant into a reusable bf16 scratch
  // all denoise steps' modulation vectors (n_steps*B, n_mod) and vec (n_steps*B, D), see fmi_flux_denoise
  DeviceBuffer mod_steps, vec_steps, temb_steps, h1_steps;  // f32
  DeviceBuffer vec_steps_bf;                                // silu(vec_steps) in bf16: A operand of the modulation GEMM
  size_t mod_steps_rows = 0;
  int mod_gemm = 1;  // fmi_flux_denoise: 1 = all steps' modulation vectors in one MFMA GEMM when there are more than 4 rows (else GEMV passes of 4 rows), 0 = always GEMV, 2 = always the GEMM
  // first-block step cache (fmi_flux_denoise_cached): four (B, S', D) f32 buffers — X0, overwritten by the copy of X1 once the residual is
  // taken; the residual r and the reference residual r_ref, swapped by index on computed steps; the output delta — plus the reduction's partials and sums.
  // Allocated by the first cached call, regrown like mod_steps, never touched by the plain entries.
  DeviceBuffer sc_x0, sc_r[2], sc_delta, sc_part, sc_sums;
  DeviceBuffer cfg_gd;  // true CFG: the guidance vector once for each half of the 2B batch, 8 floats, allocated by the first fmi_flux_denoise_cfg call
  size_t sc_elems = 0, sc_part_floats = 0;
  // the second-order solvers (fmi_flux_denoise_solver): state-sized f32 buffers — Heun's predicted state and first slope, or 2M's history in [0].
  // Allocated by the first solver call, regrown when a larger state comes, never touched by a loop without a solver.
  DeviceBuffer solver_buf[2];
  double* sc_host = nullptr;  // pinned: (num, den) per sample, read by the host after the per-step synchronisation
  bool fuse_qkv_relayout = true;  // QkNorm + RoPE + head/transposed relayout in the QKV GEMM's epilogue
  // Quantised block linears (nf4 / fp4 / LLM.int8): only the packed codes are resident; small launches multiply from them
  // (fused dequant-GEMM), large ones expand per call into a scratch and run the dense kernel (densify()).
  // Opt-in cache (fmi_flux_set_quant_dense_cache(1)): expand ONCE into the layer's slot of the BLOCKS arena — allocated
  // on first use, 17 GB more — and run the dense kernels.
  bool dense_cache = false;
  // fmi_flux_set_quant_dense_cache.  -1 (default): 3 if the device has the room when the first large quantised launch comes, else 0.
  // 0: packed only — fused below the row thresholds of densify(), per-call expansion into a scratch above; 1: dense cache (every matrix
  // expanded once); 2: always fused; 3: by size like 0, but a matrix that 0 would expand per call is expanded ONCE into its dense slot
  // (the small launches keep multiplying from the packed codes: the 50-row modulation GEMM reads 1.8 GB instead of 6.5)
  int quant_mode = -1;
  bool quant_auto = true;  // quant_mode was (or will be) chosen from the free memory: an arena that then cannot be had demotes it to 0 instead of failing every forward
  std::set<const void*> dense_ready;
  DeviceBuffer wscratch[2];  // per-call expansion of quantised matrices at large M (densify): bf16, both of one size
  // single-image sequence parallelism (fmi_flux_set_sequence_parallel; seq_parallel.hip)
  int sp_rank = 0, sp_world = 1;
  fmi_all_to_all_fn sp_a2a = nullptr;
  void* sp_user = nullptr;
  DeviceBuffer sp_base;  // [send | recv | Qf | Kf | Vtf | O (+ SP_SPLITS partial outputs) | lse]
  int sp_Tl = 0, sp_Sl = 0, sp_Nw = 0;  // the (txt, img, world) shard shape the exchange buffers were laid out for
  void *sp_send = nullptr, *sp_recv = nullptr;
  bf16_t *sp_Qf = nullptr, *sp_Kf = nullptr, *sp_Vtf = nullptr, *sp_O = nullptr;
  float* sp_lse = nullptr;
  static constexpr int SP_SPLITS = 4;  // key ranges of the latency mode's attention (attention_sp)
  // latency mode for small launches (fmi_flux_set_split_k): see gemm_split_k
  bool split_k = false;
  DeviceBuffer splitk_scratch;  // f32 partial products (grow-only)
  // 8-bit modes (fmi_flux_quantize_fp8 / fmi_flux_quantize_int8): fp8 = some block linears hold an 8-bit form (Dense::w8) and the workspace
  // has the code buffers; q8_kind says which (1 OCP e4m3, 2 int8 — GemmProblem::fp8), q8_mask which linears (FMI_Q8_* bits of the header)
  bool fp8 = false;
  int q8_kind = 0;
  unsigned q8_mask = 0;
  DeviceBuffer fp8_arena;
  // calibration of the smoothed int8 recipe: while `calib` is set every bf16 evaluation folds the column absmax of each block linear's input into
  // Dense::sm_amax (one arena: amax | s | 1/s per block linear + a scratch row for the weights' column absmax)
  bool calib = false;
  int calib_evals = 0;
  DeviceBuffer calib_arena;
  float* calib_wmax = nullptr;
  // fp8 attention operands (QK^T on the fp8 MFMA): static scales per block, 448 / (sqrt(128) * max|norm weight|) — a
  // QkNorm'ed, rotated head vector has norm sqrt(128) * |w|, so no element can exceed the e4m3 range
  int fp8_attn = 1;  // 0 off, 1 on in the 8-bit modes, 2 on in bf16 mode too (fmi_flux_set_fp8_attention)
  std::vector<float> q8_dbl, k8_dbl, q8_sgl, k8_sgl;
  bool attn_scales_valid = false;  // set by compute_attention_scales on success only; cleared whenever a weight can have changed (set_tensor, state_adopt)
  std::vector<int> n8_dbl, n8_sgl;  // fp8 attention: softmax_scale * log2(e) / (q8 * k8) == 2^-n8 EXACTLY (q_scale_pow2); handed to the attention as an integer
  // LoRA adapters (fmi_flux_lora_*; lora.hip): merged into the resident bf16 rows.  A Linear with at least one active adapter (weight != 0) has a pristine
  // copy of its rows in lora_backup, and its effective rows are ALWAYS recomputed from that copy and every active adapter in name order (lora_remerge) —
  // never patched incrementally — so the result does not depend on the order of the calls and removing the adapters restores the loaded bits.
  // One term per (adapter, Linear): a plain pair (kind LORA: f[0] = A (r, in), f[1] = B (out, r), scale = alpha / r) or a LoHa / LoKr / DoRA term (adapter.hip).
  struct LoraAdapter {
    float weight = 1.f;
    std::map<std::string, AdapterTerm> pairs;  // by weight name ("<prefix>.weight")
  };
  std::map<std::string, LoraAdapter> loras;       // by adapter name: iteration order == lexicographic order == summation order
  std::map<std::string, DeviceBuffer> lora_backup;  // by weight name: private allocations, not part of the flat state (fmi_flux_state_*)
  DeviceBuffer lora_scratch;                        // the concatenated factors of the merge in flight (grow-only; released with the last adapter)
  DeviceBuffer lora_descs;                          // the term descriptors of a LoHa / LoKr / DoRA merge in flight (adapter.hip; grow-only, released with the scratch)
  std::vector<DeviceBuffer> lora_dead;              // blocks a LoRA call has retired (MOVED here, not freed): freed behind its one final synchronisation (lora_leave)
  // ControlNet (fmi_flux_create_controlnet): a truncated FLUX without a final layer, whose every block's image rows go through a zero-initialised
  // Linear(D, D) into a bf16 sample the main model's evaluation adds to its own f32 stream.  bf16 only: the 8-bit modes, LoRA and the quantised setters refuse it.
  bool is_cn = false;
  Dense cn_x;                         // controlnet_x_embedder (D, in_channels)
  std::vector<Dense> cn_dbl, cn_sgl;  // controlnet_blocks.{i}, controlnet_single_blocks.{j}
  // sized by the first evaluation, regrown when a larger shape comes (fmi_flux_size_in_bytes counts them); a handle that is no ControlNet never allocates them
  DeviceBuffer cn_samples;  // bf16: sample k (k < nd: double block k; nd + j: single block j) at k * cn_elems, each (B, S, D)
  DeviceBuffer cn_cx;       // f32 (B*S, D): controlnet_x_embedder(cond), once per call
  DeviceBuffer cn_cond_bf;  // bf16 (B*S, in_channels): its operand
  size_t cn_elems = 0;      // B * S * D of the evaluation the samples belong to
  int cn_B = 0, cn_S = 0;
};

static int compute_attention_scales(fmi_flux* m);  // (defined with the 8-bit modes below)
static void lora_release_storage(fmi_flux* m);      // (defined with the LoRA calls at the end)

namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

size_t arena_take(fmi_flux* m, int ar, size_t bytes) {
  const size_t off = align_up(m->cursor[ar], 256);
  m->cursor[ar] = off + bytes;
  return off;
}
// Allocate arena `ar` (zero-filled) on first need and resolve the pointers of every matrix laid out in it.
int ensure_arena(fmi_flux* m, int ar) {
  Arena& a = m->arena[ar];
  if (a.base || a.bytes == 0) return FMI_OK;
  hipError_t e = a.base.alloc(a.bytes);
  if (e != hipSuccess) return fail(FMI_ERR_NOMEM, "flux: hipMalloc of " + std::to_string(a.bytes) + " bytes (weight arena " + std::to_string(ar) + ") failed: " + hipGetErrorString(e));
  FMI_HIP_TRY(hipMemset(a.base.ptr, 0, a.bytes));
  FMI_HIP_TRY(hipDeviceSynchronize());  // (an arena can appear in the middle of a forward — the expand-once policy — on a stream the null stream does not order)
  for (Dense* d : m->fused) {
    if (ar == d->ar) d->w = reinterpret_cast<bf16_t*>(a.base.as<char>() + d->w_off);
    if (ar == AR_Q4 && !d->own_wq) {
      d->wq = reinterpret_cast<uint8_t*>(a.base.as<char>() + d->q_off);
      d->absmax = reinterpret_cast<float*>(a.base.as<char>() + d->am_off);
    }
  }
  return FMI_OK;
}

// Layout pass (offsets only; BASE pointers are resolved by the caller once that arena exists).
void layout_dense(fmi_flux* m, Dense& d, int N, int K, int ar, bool bias = true) {
  d.N = N;
  d.K = K;
  d.ar = ar;
  d.w_off = arena_take(m, ar, (size_t)N * K * 2);
  d.b = bias ? reinterpret_cast<bf16_t*>(arena_take(m, AR_BASE, (size_t)N * 2) + 1) : nullptr;  // offset + 1, rebased below
  if (ar != AR_BASE) {
    d.q_off = arena_take(m, AR_Q4, (size_t)N * K / 2);
    d.am_off = arena_take(m, AR_Q4, (size_t)N * K / 64 * 4);
    m->fused.push_back(&d);
  }
}

void reg(fmi_flux* m, const std::string& name, void* ptr, int rows, int cols) {
  Dest d{nullptr, 0, false, ptr, (int64_t)rows * (cols ? cols : 1), rows, cols};
  m->names[name] = d;
  m->missing.insert(name);
}
// register W/bias of a Linear that occupies rows [r0, r0+rows) of a fused Dense
void reg_lin(fmi_flux* m, const std::string& prefix, Dense& d, int r0, int rows) {
  const int part = (int)d.parts.size();
  d.parts.push_back({r0, rows, PS_UNSET, 0});
  m->names[prefix + ".weight"] = Dest{&d, part, false, nullptr, (int64_t)rows * d.K, rows, d.K};
  m->missing.insert(prefix + ".weight");
  if (d.b) {
    m->names[prefix + ".bias"] = Dest{&d, part, true, d.b + r0, rows, rows, 0};
    m->missing.insert(prefix + ".bias");
  }
}

void build_layout(fmi_flux* m) {
  const fmi_flux_config& c = m->cfg;
  const int D = m->D, M = m->M;
  layout_dense(m, m->img_in, D, c.in_channels + m->cond, AR_BASE);  // (the one matrix that sees the conditioning channels)
  layout_dense(m, m->txt_in, D, c.joint_attention_dim, AR_BASE);
  layout_dense(m, m->time1, D, 256, AR_BASE);
  layout_dense(m, m->time2, D, D, AR_BASE);
  if (c.guidance_embeds) {
    layout_dense(m, m->guid1, D, 256, AR_BASE);
    layout_dense(m, m->guid2, D, D, AR_BASE);
  }
  layout_dense(m, m->vecin1, D, c.pooled_projection_dim, AR_BASE);
  layout_dense(m, m->vecin2, D, D, AR_BASE);
  if (m->is_cn) layout_dense(m, m->cn_x, D, c.in_channels, AR_BASE);  // (a ControlNet has no norm_out / proj_out)
  else layout_dense(m, m->final_proj, c.in_channels, D, AR_BASE);
  m->n_mod = (int64_t)c.num_layers * 12 * D + (int64_t)c.num_single_layers * 3 * D + (m->is_cn ? 0 : 2 * D);
  layout_dense(m, m->mod_all, (int)m->n_mod, D, AR_MOD);
  m->dbl.resize(c.num_layers);
  m->sgl.resize(c.num_single_layers);
  int64_t moff = 0;
  std::vector<bf16_t**> norm_ptrs;  // QkNorm weights: BASE offsets (+1) stored in the pointer until the arena exists
  auto take_norm = [&](bf16_t*& p) {
    p = reinterpret_cast<bf16_t*>(arena_take(m, AR_BASE, 128 * 2) + 1);
    norm_ptrs.push_back(&p);
  };
  for (int i = 0; i < c.num_layers; ++i) {
    auto& b = m->dbl[i];
    for (int s = 0; s < 2; ++s) {
      layout_dense(m, b.qkv[s], 3 * D, D, AR_BLOCKS);
      layout_dense(m, b.proj[s], D, D, AR_BLOCKS);
      layout_dense(m, b.mlp1[s], M, D, AR_BLOCKS);
      layout_dense(m, b.mlp2[s], D, M, AR_BLOCKS);
      take_norm(b.nq[s]);
      take_norm(b.nk[s]);
      b.mod_off[s] = moff;
      moff += 6 * D;
    }
  }
  for (int i = 0; i < c.num_single_layers; ++i) {
    auto& b = m->sgl[i];
    layout_dense(m, b.w1, 3 * D + M, D, AR_BLOCKS);
    layout_dense(m, b.w2, D, D + M, AR_BLOCKS);
    take_norm(b.nq);
    take_norm(b.nk);
    b.mod_off = moff;
    moff += 3 * D;
  }
  m->mod_final_off = moff;
  if (m->is_cn) {  // the zero-linears, one per block (sized before the first layout: `fused` keeps pointers into the vectors)
    m->cn_dbl.resize(c.num_layers);
    m->cn_sgl.resize(c.num_single_layers);
    for (auto& d : m->cn_dbl) layout_dense(m, d, D, D, AR_BLOCKS);
    for (auto& d : m->cn_sgl) layout_dense(m, d, D, D, AR_BLOCKS);
  }
  for (int a = 0; a < AR_COUNT; ++a) m->arena[a].bytes = align_up(m->cursor[a], 256) + 256;
}

// BASE exists: turn the stored offsets into pointers and register the diffusers names looked up by Flux::new (model.rs:165-772)
void resolve_base_and_names(fmi_flux* m) {
  const fmi_flux_config& c = m->cfg;
  const int D = m->D, M = m->M;
  char* base = m->arena[AR_BASE].base.as<char>();
  auto fix = [&](bf16_t*& p) {
    if (p) p = reinterpret_cast<bf16_t*>(base + (reinterpret_cast<uintptr_t>(p) - 1));
  };
  std::vector<Dense*> small = {&m->img_in, &m->txt_in, &m->time1, &m->time2, &m->vecin1, &m->vecin2, m->is_cn ? &m->cn_x : &m->final_proj};
  if (c.guidance_embeds) small.push_back(&m->guid1), small.push_back(&m->guid2);
  for (Dense* d : small) {
    d->w = reinterpret_cast<bf16_t*>(base + d->w_off);
    fix(d->b);
  }
  for (Dense* d : m->fused) fix(d->b);
  for (auto& b : m->dbl)
    for (int s = 0; s < 2; ++s) fix(b.nq[s]), fix(b.nk[s]);
  for (auto& b : m->sgl) fix(b.nq), fix(b.nk);

  reg_lin(m, "x_embedder", m->img_in, 0, D);
  reg_lin(m, "context_embedder", m->txt_in, 0, D);
  reg_lin(m, "time_text_embed.timestep_embedder.linear_1", m->time1, 0, D);
  reg_lin(m, "time_text_embed.timestep_embedder.linear_2", m->time2, 0, D);
  if (c.guidance_embeds) {
    reg_lin(m, "time_text_embed.guidance_embedder.linear_1", m->guid1, 0, D);
    reg_lin(m, "time_text_embed.guidance_embedder.linear_2", m->guid2, 0, D);
  }
  reg_lin(m, "time_text_embed.text_embedder.linear_1", m->vecin1, 0, D);
  reg_lin(m, "time_text_embed.text_embedder.linear_2", m->vecin2, 0, D);
  if (m->is_cn) {
    reg_lin(m, "controlnet_x_embedder", m->cn_x, 0, D);
    for (int i = 0; i < c.num_layers; ++i) reg_lin(m, "controlnet_blocks." + std::to_string(i), m->cn_dbl[i], 0, D);
    for (int i = 0; i < c.num_single_layers; ++i) reg_lin(m, "controlnet_single_blocks." + std::to_string(i), m->cn_sgl[i], 0, D);
  } else {
    reg_lin(m, "proj_out", m->final_proj, 0, c.in_channels);
    reg_lin(m, "norm_out.linear", m->mod_all, (int)m->mod_final_off, 2 * D);
  }
  for (int i = 0; i < c.num_layers; ++i) {
    auto& b = m->dbl[i];
    const std::string p = "transformer_blocks." + std::to_string(i) + ".";
    reg_lin(m, p + "norm1.linear", m->mod_all, (int)b.mod_off[0], 6 * D);
    reg_lin(m, p + "norm1_context.linear", m->mod_all, (int)b.mod_off[1], 6 * D);
    const char* qn[2][3] = {{"attn.to_q", "attn.to_k", "attn.to_v"}, {"attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj"}};
    const char* on[2] = {"attn.to_out.0", "attn.to_add_out"};
    const char* nqn[2] = {"attn.norm_q.weight", "attn.norm_added_q.weight"};
    const char* nkn[2] = {"attn.norm_k.weight", "attn.norm_added_k.weight"};
    const char* f1[2] = {"ff.net.0.proj", "ff_context.net.0.proj"};
    const char* f2[2] = {"ff.net.2", "ff_context.net.2"};
    for (int s = 0; s < 2; ++s) {
      for (int j = 0; j < 3; ++j) reg_lin(m, p + qn[s][j], b.qkv[s], j * D, D);
      reg_lin(m, p + on[s], b.proj[s], 0, D);
      reg(m, p + nqn[s], b.nq[s], 128, 0);
      reg(m, p + nkn[s], b.nk[s], 128, 0);
      reg_lin(m, p + f1[s], b.mlp1[s], 0, M);
      reg_lin(m, p + f2[s], b.mlp2[s], 0, D);
    }
  }
  for (int i = 0; i < c.num_single_layers; ++i) {
    auto& b = m->sgl[i];
    const std::string p = "single_transformer_blocks." + std::to_string(i) + ".";
    reg_lin(m, p + "norm.linear", m->mod_all, (int)b.mod_off, 3 * D);
    reg_lin(m, p + "attn.to_q", b.w1, 0, D);
    reg_lin(m, p + "attn.to_k", b.w1, D, D);
    reg_lin(m, p + "attn.to_v", b.w1, 2 * D, D);
    reg_lin(m, p + "proj_mlp", b.w1, 3 * D, M);
    reg(m, p + "attn.norm_q.weight", b.nq, 128, 0);
    reg(m, p + "attn.norm_k.weight", b.nk, 128, 0);
    reg_lin(m, p + "proj_out", b.w2, 0, D);
  }
}

// Rows [r0, r0 + rows) of a matrix whose codes are in wq / absmax (fp4, nf4, int8) -> the same rows of `image`, an (N, K) bf16 image of the matrix (d.w or
// the scratch): one launch per chunk of at most 2^28 elements (the dequant kernels index in 32 bits; chunk starts stay multiples of the quantisation
// block: K % 64 == 0).  Every FLUX block matrix is a single chunk.
int expand_wq_rows(Dense& d, int r0, int rows, int kind, int blocksize, bf16_t* image, hipStream_t s) {
  const int chunk = std::max(64, (int)std::min<int64_t>(rows, ((1ll << 28) / d.K) / 64 * 64));
  for (const int end = r0 + rows; r0 < end; r0 += chunk) {
    const size_t e0 = (size_t)r0 * d.K;
    const void* src = kind == PS_INT8 ? d.wq + e0 : d.wq + e0 / 2;
    const float* scales = kind == PS_INT8 ? d.absmax + r0 : d.absmax + e0 / blocksize;
    FMI_TRY(dequant_to_bf16(kind, blocksize, src, scales, 0.f, d.K, (int64_t)std::min(chunk, end - r0) * d.K, image + e0, s));
  }
  return FMI_OK;
}
// Part `part` of `d`, resident as any quantised kind, -> its bf16 rows of `image`
int expand_part(Dense& d, int part, bf16_t* image, hipStream_t s) {
  const Dense::Part& pt = d.parts[part];
  if (!is_codes(pt.state)) return expand_wq_rows(d, pt.r0, pt.rows, pt.state, pt.blocksize, image, s);
  return dequant_to_bf16(pt.state, 0, d.gq[part].ptr, nullptr, d.gscale[part], d.K, (int64_t)pt.rows * d.K, image + (size_t)pt.r0 * d.K, s);
}
// A matrix of one kind (q_type != 0) -> `image`.  fp4 / nf4 / int8 in one pass over the whole matrix; ggml blocks and 8-bit float codes part by part (their
// types and scales are per part).
int expand_matrix(Dense& d, bf16_t* image, hipStream_t s) {
  if (!is_codes(d.q_type)) return expand_wq_rows(d, 0, d.N, d.q_type, d.q_blocksize, image, s);
  for (int i = 0; i < (int)d.parts.size(); ++i) FMI_TRY(expand_part(d, i, image, s));
  return FMI_OK;
}

// The tail of every setter that has put the weight of part `part` of `d` in place as `state`: a part that stops being ggml blocks / 8-bit float codes gives
// up its buffer, and whatever was derived from the matrix's earlier contents (its cached expansion, finalize()'s decision) goes.
void part_loaded(fmi_flux* m, Dense& d, int part, int state, int blocksize, const std::string& wname) {
  d.parts[part].state = (uint8_t)state, d.parts[part].blocksize = blocksize;
  if (!is_codes(state) && part < (int)d.gq.size()) d.gq[part].reset();
  m->dense_ready.erase(&d);
  m->finalized = false;
  m->missing.erase(wname);
}

// part `part` of `d` is resident as plain bf16 rows of d.w (what a LoRA merge patches and fmi_flux_get_tensor reads): a Linear outside the fused matrices,
// or a dense part of a matrix that finalize() left dense (such a part's arena exists: every path that marks a part dense has allocated it)
bool part_is_plain(const Dense& d, int part) { return d.ar == AR_BASE || (d.q_type == 0 && d.parts[part].state == PS_DENSE && d.w); }
// the device bytes a matrix owns outside the arenas: its LLM.int8 weight and SCB, its parts' ggml blocks / 8-bit float codes
size_t resident_code_bytes(const Dense& d) {
  size_t b = d.own_wq ? (size_t)d.N * d.K + (size_t)d.N * 4 : 0;
  for (const DeviceBuffer& g : d.gq) b += g.bytes();
  return b;
}

// Decide how every fused matrix is multiplied: all parts the same quantised kind -> that kind (packed form only);
// all dense -> dense; a mixture (e.g. a checkpoint that quantises to_q but not to_v) -> the quantised parts are
// expanded into the dense arena once and the matrix is dense.
int finalize(fmi_flux* m) {
  if (m->finalized) return FMI_OK;
  for (Dense* d : m->fused) {
    bool any_dense = false, uniform = true;
    const uint8_t k0 = d->parts.empty() ? (uint8_t)PS_DENSE : d->parts[0].state;
    const int bs0 = d->parts.empty() ? 0 : d->parts[0].blocksize;
    for (auto& pt : d->parts) {
      if (pt.state == PS_DENSE) any_dense = true;
      if (pt.state != k0 || pt.blocksize != bs0) uniform = false;
    }
    if (uniform && !any_dense) {
      d->q_type = k0, d->q_blocksize = bs0;
      continue;
    }
    if (!uniform) {
      FMI_TRY(ensure_arena(m, d->ar));
      for (int i = 0; i < (int)d->parts.size(); ++i) {
        auto& pt = d->parts[i];
        if (pt.state == PS_DENSE) continue;
        FMI_TRY(expand_part(*d, i, d->w, nullptr));
        pt.state = PS_DENSE, pt.blocksize = 0;
      }
      FMI_HIP_TRY(hipDeviceSynchronize());
      d->gq.clear(), d->gscale.clear();  // (after the synchronisation: the expansions have read the blocks)
    }
    d->q_type = 0, d->q_blocksize = 0;
  }
  m->dense_ready.clear();
  m->finalized = true;
  return FMI_OK;
}

constexpr int PE_ROW_FLOATS = 128;  // one position of the RoPE table: 64 (cos, sin) pairs — the head dim fmi_flux_create checks axes_dim against
int ensure_workspace(fmi_flux* m, int B, int S, int T) {
  auto& w = m->ws;
  if (w.base && w.B == B && w.S == S && w.T == T) return FMI_OK;
  const int D = m->D, M = m->M, H = m->H, L = S + T;
  const int Lpad = (L + 63) / 64 * 64;
  const int C = m->cfg.in_channels, J = m->cfg.joint_attention_dim, P = m->cfg.pooled_projection_dim;
  const int ldbig = 3 * D + M;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    off = align_up(off, 256);
    size_t o = off;
    off += bytes;
    return o;
  };
  struct Item {
    void** p;
    size_t bytes;
    size_t o;
  };
  std::vector<Item> items;
  auto add = [&](void** p, size_t bytes) { items.push_back({p, bytes, take(bytes)}); };
  add((void**)&w.x_img, (size_t)B * S * D * 4);
  add((void**)&w.x_txt, (size_t)B * T * D * 4);
  add((void**)&w.x_txt0, (size_t)B * T * D * 4);
  add((void**)&w.x, (size_t)B * L * D * 4);
  add((void**)&w.vec, (size_t)B * D * 4);
  add((void**)&w.mod, (size_t)B * m->n_mod * 4);
  add((void**)&w.temb, (size_t)B * 256 * 4);
  add((void**)&w.h1, (size_t)B * D * 4);
  add((void**)&w.yf, (size_t)B * P * 4);
  add((void**)&w.pe, (size_t)B * L * PE_ROW_FLOATS * 4);
  add((void**)&w.img_f32, (size_t)B * S * C * 4);
  add((void**)&w.pred_tmp, (size_t)B * S * C * 4);
  add((void**)&w.tv, 4096 * 4);
  add((void**)&w.img_bf, (size_t)B * S * (C + m->cond) * 2);  // the x_embedder operand: [state | conditioning] columns
  add((void**)&w.txt_bf, (size_t)B * T * J * 2);
  add((void**)&w.xm, (size_t)B * L * D * 2);
  add((void**)&w.qkv_img, (size_t)B * S * 3 * D * 2);
  add((void**)&w.qkv_txt, (size_t)B * T * 3 * D * 2);
  add((void**)&w.big, (size_t)B * L * ldbig * 2);
  add((void**)&w.Qh, (size_t)B * H * L * 128 * 2);
  add((void**)&w.Kh, (size_t)B * H * L * 128 * 2);
  add((void**)&w.Vt, (size_t)B * H * 128 * Lpad * 2);
  add((void**)&w.attn_img, (size_t)B * S * D * 2);
  add((void**)&w.attn_txt, (size_t)B * T * D * 2);
  add((void**)&w.hid, (size_t)B * L * M * 2);
  add((void**)&w.vec_bf, (size_t)B * D * 2);
  if (m->fp8) {
    add((void**)&w.a8, (size_t)B * L * (D + M));
    add((void**)&w.a8s, (size_t)B * L * 4);
    add((void**)&w.a8o, (size_t)B * L * 4);
  }
  const size_t total = align_up(off, 256);
  if (w.base) FMI_HIP_TRY(hipDeviceSynchronize());
  FMI_HIP_TRY(w.base.alloc(total));
  FMI_HIP_TRY(hipMemset(w.base.ptr, 0, total));  // also zeroes the Vt pad columns once
  for (auto& it : items) *it.p = w.base.as<char>() + it.o;
  if (B == 1) {
    // one sample: the two streams of the double blocks ARE the halves of the joint stream the single blocks read — cat([txt, img], 1) (model.rs:827)
    // is then no copy at all (with B > 1 the streams are (B*T, D) / (B*S, D) row blocks for the grouped GEMMs and the concat interleaves them per sample)
    w.x_txt = w.x;
    w.x_img = w.x + (size_t)T * D;
  }
  w.B = B, w.S = S, w.T = T, w.Lpad = Lpad;
  return FMI_OK;
}

// fp8 mode: the block linear `d` on a quantised input (rows of a8 / a8s starting at `row0`, row length d.K)
GemmProblem make_problem_fp8(const fmi_flux* m, const Dense& d, int row0, int Mrows, void* out, int ldo, int epi) {
  GemmProblem p{};
  p.A = reinterpret_cast<const bf16_t*>(m->ws.a8 + (size_t)row0 * d.K);
  p.W = reinterpret_cast<const bf16_t*>(d.w8);
  p.bias = d.b;
  p.out = out;
  p.M = Mrows, p.N = d.N, p.K = d.K;
  p.lda = d.K, p.ldw = d.K, p.ldo = ldo;
  p.epi = epi;
  p.alpha = 1.0f;
  p.fp8 = m->q8_kind;
  p.a_scale = m->ws.a8s + row0;
  p.w_scale = d.w8_scale;
  if (d.w8_d0 >= 0) p.a_off = m->ws.a8o + row0, p.w_sum = d.w8_sum;  // the input was quantised by quantize_act (post-GELU form)
  return p;
}
// 8-bit modes: the row pass in front of a block linear whose input no producer quantises (attention output, gelu(mlp), their concat) —
// the int8 mode's post-GELU form when the consuming linear asks for it (Dense::w8_d0), else the symmetric per-row recipe
int quantize_act(fmi_flux* m, const Dense& d, const bf16_t* x, int ld, int rows, int row0, hipStream_t s) {
  uint8_t* out = m->ws.a8 + (size_t)row0 * d.K;
  if (d.w8_d0 >= 0) return launch_quantize_rows_i8_asym(x, ld, rows, d.K, d.w8_d0, out, m->ws.a8s + row0, m->ws.a8o + row0, s, d.sm_inv);
  return launch_quantize_rows_fp8(x, ld, rows, d.K, out, m->ws.a8s + row0, s, m->q8_kind, d.sm_inv);
}
// calibration (fmi_flux_calibrate_int8): the column absmax of a block linear's bf16 input, folded into its statistics
int calib_rec(fmi_flux* m, const Dense& d, const bf16_t* x, int ld, int rows, hipStream_t s) {
  if (!m->calib || !d.sm_amax) return FMI_OK;
  return launch_col_absmax(x, ld, rows, d.K, d.sm_amax, s);
}
GemmProblem make_problem(const Dense& d, const bf16_t* A, int lda, int Mrows, void* out, int ldo, int epi) {
  GemmProblem p{};
  p.A = A;
  p.W = d.w;
  p.bias = d.b;
  p.out = out;
  p.M = Mrows;
  p.N = d.N;
  p.K = d.K;
  p.lda = lda;
  p.ldw = d.K;
  p.ldo = ldo;
  p.epi = epi;
  p.alpha = 1.0f;
  if (d.q_type) {
    p.Wq = d.wq;
    p.absmax = d.absmax;
    p.q_type = d.q_type;
    p.q_blocksize = d.q_blocksize;
  }
  return p;
}
// Fused relayout epilogue of a [q|k|v](|mlp) projection (GemmProblem::qk_*); returns false if this
// shape must take the stand-alone kernels (positions not 16-aligned, model width not 256-aligned).
bool can_fuse_relayout(const fmi_flux* m, int Mrows, int rows, int row_off) {
  return m->fuse_qkv_relayout && m->D % 256 == 0 && rows % 16 == 0 && row_off % 16 == 0 && Mrows % 16 == 0;
}
bool with_qkv_relayout(fmi_flux* m, GemmProblem& p, const bf16_t* nq, const bf16_t* nk, int64_t pe_bs, int rows, int row_off, int Ltot, float q8 = 0.f,
                       float k8 = 0.f) {
  auto& w = m->ws;
  if (!can_fuse_relayout(m, p.M, rows, row_off) || p.N < 256) return false;
  p.qk_q8 = q8, p.qk_k8 = k8;
  p.qk_qh = w.Qh, p.qk_kh = w.Kh, p.qk_vt = w.Vt;
  p.qk_wq = nq, p.qk_wk = nk;
  p.qk_pe = w.pe, p.qk_pe_bstride = pe_bs;
  p.qk_H = m->H, p.qk_D = m->D, p.qk_rows = rows, p.qk_row_off = row_off, p.qk_Ltot = Ltot, p.qk_Lpad = w.Lpad;
  return true;
}
void with_gate(GemmProblem& p, const float* gate, int rows_per_batch, int bstride) {
  p.gate = gate;
  p.rows_per_batch = rows_per_batch;
  p.gate_bstride = bstride;
}
// Quantised linears (BnbLinear::forward, bitsandbytes/mod.rs:293-312: "dequantize_w then matmul"):
//   nf4 / fp4  -> the fused dequant-GEMM reads the packed codes (launch_gemm picks the kernel by M), nothing is expanded;
//                 with the dense cache on, the matrix is expanded once into its slot of the BLOCKS / MOD arena instead;
//   LLM.int8   -> up to INT8_FUSED_MAX_ROWS rows: expanded (w * SCB / 127) by the GEMM's weight-tile stage (gemm_bf16_kernel<1>: VALU
//                 expansion into the swizzled LDS image, bit-identical to the stand-alone dequant); above: stand-alone expansion
//                 into a reusable scratch + the dense kernel (faster, see densify); with the dense cache on, expanded once.
// Above these row counts a quantised matrix is expanded per call into a reusable scratch (2 x the largest fused matrix,
// 264 MB) and the dense kernel runs — measured faster than the fused kernels, because ONE stand-alone expansion is amortised
// over all M rows while the fused expansion is repeated by every row tile:
//   LLM.int8  fused stage 0.44-0.59x dense; 4608 x 21504 x 3072: 432 + 38 us against 728 us fused   -> from 257 rows
//   nf4 / fp4 fused kernel 0.61-0.76x dense; same shape: 436 + 35 us against 626 us fused; 512 x 9216 x 3072: 53 + 15 us
//             against 87 us                                                                          -> from 384 rows
// (profiles/r02_gemm_bench_quantised.txt, dense = the 16x16x32 kernel; below these sizes the GEMM is short or bound by weight
// bytes and the packed read wins).  Either way only the packed codes are resident.
constexpr int INT8_FUSED_MAX_ROWS = 256;
constexpr int Q4_FUSED_MAX_ROWS = 383;
// The default policy follows the memory: BnbLinear::forward is "dequantise, then matmul" for every call
// (bitsandbytes/mod.rs:301-312) because the reference targets 24 GB cards; on a 288 GB part the per-call expansion of a large launch
// (228 per denoise step, 4.4 ms) buys nothing.  When the first launch that would take the scratch comes and the device has at least
// twice the dense arenas' bytes free, those matrices are expanded once (mode 3); otherwise only the packed codes stay resident (mode 0).
static int resolve_quant_mode(fmi_flux* m) {
  if (m->quant_mode >= 0) return m->quant_mode;
  size_t need = 0, fr = 0, tot = 0;
  if (!m->arena[AR_BLOCKS].base) need += m->arena[AR_BLOCKS].bytes;
  if (!m->arena[AR_MOD].base && (size_t)m->mod_all.N * m->mod_all.K < (1ull << 31)) need += m->arena[AR_MOD].bytes;  // (FLUX.1's stays packed: densify)
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = 0;
  m->quant_mode = fr >= 2 * need ? 3 : 0;
  return m->quant_mode;
}
int densify(fmi_flux* m, GemmProblem* p, Dense* const* dn, int n, hipStream_t s) {
  // one decision per launch group (the img + txt problems of a double block stay one grouped launch)
  bool scratch = false;
  for (int i = 0; i < n && i < 2; ++i)
    if (dn[i] && p[i].q_type && !is_codes(p[i].q_type) && m->quant_mode != 1 && m->quant_mode != 2)
      scratch = scratch || p[i].M > (p[i].q_type == PS_INT8 ? INT8_FUSED_MAX_ROWS : Q4_FUSED_MAX_ROWS);
  // A matrix of 2^31 or more weights (the fused modulation matrix of FLUX.1: 344 D x D = 3.2e9) never goes through the scratch —
  // the stand-alone dequant launchers count elements in 32 bits and the scratch is sized for the block matrices — it stays on
  // the fused dequant-GEMM kernels at any row count (8 prompts x 50 steps = 400 rows of the modulation precompute).
  for (int i = 0; i < n && i < 2; ++i)
    if (dn[i] && p[i].q_type && (size_t)p[i].N * p[i].K >= (1ull << 31)) scratch = false;
  for (int i = 0; i < n && i < 2; ++i) {
    Dense* d = dn[i];
    if (!d || !p[i].q_type) continue;
    // ggml blocks (fmi_flux_set_linear_gguf) and 8-bit float codes (fmi_flux_set_linear_f8) have no fused dequant-GEMM: at every row count the matrix is
    // expanded, once (modes 1 and 3) or per call (0 and 2)
    const bool gguf = is_codes(p[i].q_type);
    if (!m->dense_cache && !scratch && !gguf) continue;  // fused paths (launch_gemm picks the kernel)
    const size_t elems = (size_t)p[i].N * p[i].K;
    bool once = m->dense_cache || ((scratch || gguf) && resolve_quant_mode(m) == 3);
    if (once && !m->dense_cache && m->quant_auto && !m->arena[d->ar].base) {
      // the "by memory" policy decided on ONE hipMemGetInfo snapshot: if the arena cannot be had after all — memory taken since, or a
      // later arena of the same model — fall back to the packed-only policy for good instead of answering every forward with FMI_ERR_NOMEM
      if (ensure_arena(m, d->ar) == FMI_ERR_NOMEM) {
        (void)hipGetLastError();
        m->quant_mode = 0;
        once = false;
      }
    }
    if (once) {
      FMI_TRY(ensure_arena(m, d->ar));
      if (!m->dense_ready.count(d)) {
        FMI_TRY(expand_matrix(*d, d->w, s));
        m->dense_ready.insert(d);
      }
      p[i].W = d->w;
    } else {
      if (elems * sizeof(bf16_t) > m->wscratch[1].bytes()) {  // ([1] is allocated last: it has the size only when both have it)
        const size_t want = std::max(elems, (size_t)(3 * m->D + m->M) * (size_t)m->D);  // largest fused weight of the model
        FMI_HIP_TRY(hipDeviceSynchronize());
        for (int k = 0; k < 2; ++k) FMI_HIP_TRY(m->wscratch[k].alloc(want * sizeof(bf16_t)));
      }
      bf16_t* ws_i = m->wscratch[i].as<bf16_t>();
      FMI_TRY(expand_matrix(*d, ws_i, s));
      p[i].W = ws_i;
    }
    p[i].ldw = p[i].K;
    p[i].Wq = nullptr, p[i].absmax = nullptr, p[i].q_type = 0, p[i].q_blocksize = 0;
  }
  return FMI_OK;
}
// Latency mode (opt-in, fmi_flux_set_split_k): a residual projection whose launch is less than half a wave of 256 x 256 tiles —
// a sequence-parallel shard of 576 rows x 3072 columns is 36 tiles on 256 CUs, and a tile's K loop (K up to 15 360) takes as long
// as in the full-size launch — is cut along K into S problems of the SAME grouped launch (A and W advanced by s * K / S columns,
// partial products stored as f32), and a second kernel adds the S parts in index order, the bias, and applies the gated residual
// update.  Deterministic (fixed order), but NOT the bits of the unsplit launch: the f32 sum is associated differently.  That is
// why it is opt-in: by default a sequence-parallel forward reproduces the single-device one bit for bit.
int gemm_split_k(fmi_flux* m, const GemmProblem* p, int n, hipStream_t s, bool* done) {
  *done = false;
  if (!m->split_k || n < 1 || n > 2) return FMI_OK;
  int tiles = 0;
  size_t floats = 0;
  for (int i = 0; i < n; ++i) {
    const GemmProblem& q = p[i];
    if (q.epi != EPI_RESID_GATE_F32 || q.q_type || q.fp8 || q.cv_ks || q.qk_qh || q.alpha != 1.0f || q.N % 4 || q.ldo % 4) return FMI_OK;
    tiles += ((q.M + 255) / 256) * ((q.N + 255) / 256);
    floats += (size_t)q.M * q.N;
  }
  if (tiles >= 128) return FMI_OK;
  int S = 8;
  auto fits = [&](int S_) {
    if (tiles * S_ > 256 || n * S_ > 8) return false;
    for (int i = 0; i < n; ++i)
      if (p[i].K % (64 * S_) || p[i].K / S_ < 256) return false;
    return true;
  };
  while (S > 1 && !fits(S)) S >>= 1;
  if (S == 1) return FMI_OK;
  if (floats * S * sizeof(float) > m->splitk_scratch.bytes()) {
    FMI_HIP_TRY(hipStreamSynchronize(s));
    FMI_HIP_TRY(m->splitk_scratch.alloc(floats * S * sizeof(float)));
  }
  GemmProblem parts[8];
  const float* base[2];
  float* cur = m->splitk_scratch.as<float>();
  int np = 0;
  for (int i = 0; i < n; ++i) {
    base[i] = cur;
    const int Kc = p[i].K / S;
    for (int k = 0; k < S; ++k) {
      GemmProblem q = p[i];
      q.A = p[i].A + (size_t)k * Kc, q.W = p[i].W + (size_t)k * Kc, q.K = Kc;
      q.bias = nullptr, q.gate = nullptr, q.rows_per_batch = 0, q.gate_bstride = 0;
      q.epi = EPI_STORE_F32, q.out = cur, q.ldo = p[i].N;
      parts[np++] = q;
      cur += (size_t)p[i].M * p[i].N;
    }
  }
  FMI_TRY(launch_gemm(parts, np, s));
  for (int i = 0; i < n; ++i)
    FMI_TRY(launch_splitk_resid_gate(base[i], S, p[i].bias, p[i].gate, p[i].rows_per_batch, p[i].gate_bstride, reinterpret_cast<float*>(p[i].out), p[i].ldo, p[i].M,
                                     p[i].N, s));
  *done = true;
  return FMI_OK;
}
// launch 1 or 2 problems (dn[i] = the weight matrix of problem i); quantised and dense problems cannot share a grid
int gemm2(fmi_flux* m, GemmProblem* p, Dense* const* dn, int n, hipStream_t s) {
  FMI_TRY(densify(m, p, dn, n, s));
  bool split = false;
  FMI_TRY(gemm_split_k(m, p, n, s, &split));
  if (split) return FMI_OK;
  if (n == 2 && (p[0].q_type != 0) != (p[1].q_type != 0)) {
    FMI_TRY(launch_gemm(p, 1, s));
    return launch_gemm(p + 1, 1, s);
  }
  return launch_gemm(p, n, s);
}
int gemm1(fmi_flux* m, GemmProblem& p, Dense& d, hipStream_t s) {
  Dense* dn[1] = {&d};
  return gemm2(m, &p, dn, 1, s);
}

// Sequence-parallel joint attention: the local (H, Ll) q|k|v go out, (H/N heads, all L tokens) come in, attention runs on
// this rank's heads, and the output rows travel back to their owners.  `out` = where the local rows of the result go.
int ensure_sp_buffers(fmi_flux* m, int Tl, int Sl) {
  if (m->sp_base && m->sp_Tl == Tl && m->sp_Sl == Sl && m->sp_Nw == m->sp_world) return FMI_OK;  // sizes and offsets depend on all three
  const int N = m->sp_world, Hr = m->H / N, Ll = Tl + Sl, L = N * Ll, Lp = (L + 63) / 64 * 64;
  const size_t xb = align_up((size_t)N * std::max(sp_qkv_bytes_per_peer(Hr, Ll), sp_o_bytes_per_peer(Hr, Ll)), 256);
  const size_t qb = align_up((size_t)Hr * L * 128 * 2, 256), vb = align_up((size_t)Hr * 128 * Lp * 2, 256);
  const size_t lb = align_up((size_t)fmi_flux::SP_SPLITS * Hr * L * sizeof(float), 256);
  const size_t total = 2 * xb + 2 * qb + vb + (1 + fmi_flux::SP_SPLITS) * qb + lb;
  FMI_HIP_TRY(hipDeviceSynchronize());
  FMI_HIP_TRY(m->sp_base.alloc(total));
  char* c = m->sp_base.as<char>();
  m->sp_send = c, c += xb;
  m->sp_recv = c, c += xb;
  m->sp_Qf = reinterpret_cast<bf16_t*>(c), c += qb;
  m->sp_Kf = reinterpret_cast<bf16_t*>(c), c += qb;
  m->sp_Vtf = reinterpret_cast<bf16_t*>(c), c += vb;
  m->sp_O = reinterpret_cast<bf16_t*>(c), c += (1 + fmi_flux::SP_SPLITS) * qb;
  m->sp_lse = reinterpret_cast<float*>(c);
  m->sp_Tl = Tl, m->sp_Sl = Sl, m->sp_Nw = m->sp_world;
  return FMI_OK;
}
int attention_sp(fmi_flux* m, const AttnOut& out, int Tl, int Sl, float scale, hipStream_t s) {
  auto& w = m->ws;
  const int N = m->sp_world, H = m->H, Hr = H / N, Ll = Tl + Sl, L = N * Ll, Lp = (L + 63) / 64 * 64;
  FMI_TRY(ensure_sp_buffers(m, Tl, Sl));
  FMI_TRY(launch_sp_pack_qkv(w.Qh, w.Kh, w.Vt, m->sp_send, H, Tl, Sl, N, s));
  if (m->sp_a2a(m->sp_user, m->sp_send, m->sp_recv, sp_qkv_bytes_per_peer(Hr, Ll), s) != 0)
    return fail(FMI_ERR_STATE, "flux: the sequence-parallel all-to-all callback failed (q|k|v exchange)");
  FMI_TRY(launch_sp_unpack_qkv(m->sp_recv, m->sp_Qf, m->sp_Kf, m->sp_Vtf, H, Tl, Sl, N, s));
  AttnOut o{};
  o.p0 = nullptr, o.rows0 = 0;
  o.p1 = m->sp_O, o.ld1 = Hr * 128, o.bstride1 = (int64_t)L * Hr * 128;
  const int ntiles = (L + 63) / 64, wgs = Hr * ((L + 255) / 256);
  int S = fmi_flux::SP_SPLITS;
  while (S > 1 && (wgs * S > 256 || ntiles < 4 * S)) S >>= 1;
  if (m->split_k && S > 1) {
    // Latency mode: H/N heads are too few workgroups for 256 CUs (3 heads x 18 query blocks = 54, each walking all 72 KV tiles).
    // The keys are cut into S <= SP_SPLITS ranges of whole tiles (as many as keep the grid within one wave of workgroups): ONE launch of the one-wave kernel with SP_SPLITS x the workgroups,
    // each walking its range and also writing the rows' log-sum-exp, and sp_merge_splits combines the normalised partial outputs
    // with the weights 2^(lse_s - max) in a fixed order.  Equal to the unsplit attention to bf16 rounding of the partial
    // outputs, not bit for bit (the mode is opt-in: fmi_flux_set_split_k).
    const size_t part = (size_t)L * Hr * 128;
    AttnOut parts = o;
    parts.p1 = m->sp_O + part;  // slices 1 .. S of the buffer; slice 0 receives the merged result
    FMI_TRY(launch_attention_ex(m->sp_Qf, m->sp_Kf, m->sp_Vtf, parts, 1, Hr, L, L, Lp, scale, m->attn_thr, s, 0, m->sp_lse, S, ATT_NO_EXP2, m->attn_kind));
    FMI_TRY(launch_sp_merge_splits(m->sp_O + part, m->sp_lse, S, m->sp_O, Hr, L, s));
  } else {
    FMI_TRY(launch_attention_ex(m->sp_Qf, m->sp_Kf, m->sp_Vtf, o, 1, Hr, L, L, Lp, scale, m->attn_thr, s, 0, nullptr, 0, ATT_NO_EXP2, m->attn_kind));
  }
  FMI_TRY(launch_sp_pack_o(m->sp_O, m->sp_send, H, Tl, Sl, N, s));
  if (m->sp_a2a(m->sp_user, m->sp_send, m->sp_recv, sp_o_bytes_per_peer(Hr, Ll), s) != 0)
    return fail(FMI_ERR_STATE, "flux: the sequence-parallel all-to-all callback failed (attention output exchange)");
  return launch_sp_unpack_o(m->sp_recv, out, H, Ll, N, s);
}

// roctx ranges around the phases (rocprofv3 --marker-trace groups the kernel trace by them): FMI_ROCTX=1 in the environment.
// The marker library is opened at run time (librocprofiler-sdk-roctx.so.1, else libroctx64.so.4): no link-time dependency, and
// nothing happens — not even the dlopen — unless the variable is set.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* e = getenv("FMI_ROCTX");
    if (!e || !atoi(e)) return;
    for (const char* lib : {"librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "libroctx64.so"}) {
      if (void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL)) {
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push && pop) return;
        push = nullptr, pop = nullptr;
      }
    }
  }
};
const Roctx& roctx() {
  static const Roctx r;
  return r;
}

struct PhaseTimer {
  fmi_flux* m;
  hipStream_t s;
  int ph;
  PhaseTimer(fmi_flux* m_, hipStream_t s_, int ph_) : m(m_), s(s_), ph(ph_) {
    if (roctx().push) roctx().push(kPhaseNames[ph]);
    if (m->profiling) hipEventRecord(m->ev0, s);
  }
  ~PhaseTimer() {
    if (m->profiling) {
      hipEventRecord(m->ev1, s);
      hipEventSynchronize(m->ev1);
      float ms = 0;
      hipEventElapsedTime(&ms, m->ev0, m->ev1);
      m->phase_ms[ph] += ms;
    }
    if (roctx().pop) roctx().pop();
  }
};

int check_ready(fmi_flux* m) {
  FMI_TRY(m->missing.ready("flux"));
  return finalize(m);
}
// the handle's device becomes the calling thread's current device (hipSetDevice is per thread)
int use_device(const fmi_flux* m) { return use_device_ordinal(m->device); }

// What the evaluations of one call are conditioned on: the caller's options as validate() accepted them, with what it resolved from them.  Built once per call.
struct EvalPlan {
  fmi_flux_denoise_options o;  // every field null where the call has none
  int R;                       // context rows per sample (0: none, the text-to-image launches)
  int Bs;                      // the state's samples: in->B — under true CFG `in` is the loop's internal batch of 2 * Bs
  const fmi_flux_controlnet* cn = nullptr;  // the call's ControlNet, else null
};
// The injection hook of forward_core: the ControlNet whose samples the evaluation adds to its f32 stream, and this step's scale (never 0: such a step has no hook).
struct CnInject {
  const fmi_flux* net;
  float c;
};
// The IP-Adapter hook of forward_core: the adapter whose K / V (projected once per call, ip_prepare) the image queries of every double block attend to, and this
// step's scale (never 0: such a step has no hook and keeps the fused q|k|v relayout).
struct IpInject {
  const fmi_ip_adapter* a;
  float c;
};

// The ControlNet's per-shape buffers, sized by the first evaluation and regrown when a larger shape comes.
int cn_ensure(fmi_flux* net, int B, int S, hipStream_t s) {
  const size_t elems = (size_t)B * S * net->D, n = net->cn_dbl.size() + net->cn_sgl.size();
  if (net->cn_samples.bytes() < n * elems * 2 || net->cn_cx.bytes() < elems * 4) {
    FMI_HIP_TRY(hipStreamSynchronize(s));
    if (net->cn_samples.alloc(n * elems * 2) != hipSuccess || net->cn_cx.alloc(elems * 4) != hipSuccess ||
        net->cn_cond_bf.alloc((size_t)B * S * net->cfg.in_channels * 2) != hipSuccess) {
      net->cn_samples.reset(), net->cn_cx.reset(), net->cn_cond_bf.reset();
      return fail(FMI_ERR_NOMEM, "flux controlnet: hipMalloc of the sample buffers failed");
    }
  }
  net->cn_elems = elems, net->cn_B = B, net->cn_S = S;
  return FMI_OK;
}
// controlnet_x_embedder(cond) for the B samples of the evaluations to come (cond holds Bs of them: both halves of a true-CFG batch see the same), once per call:
// it does not depend on the state or on t.  Kept in f32 — the sum x_embedder(img) + controlnet_x_embedder(cond) is taken in f32 at every step.
int cn_embed_cond(fmi_flux* net, const void* cond, fmi_dtype dt, int B, int Bs, int S, hipStream_t s) {
  const int C = net->cfg.in_channels;
  PhaseTimer pt(net, s, PH_EMBED);
  FMI_TRY(launch_cast_cols_bf16(cond, dt, (int64_t)B * S, (int64_t)Bs * S, C, net->cn_cond_bf.as<bf16_t>(), C, 0, s));
  GemmProblem p = make_problem(net->cn_x, net->cn_cond_bf.as<bf16_t>(), C, B * S, net->cn_cx.ptr, net->D, EPI_STORE_F32);
  return gemm1(net, p, net->cn_x, s);
}

// Everything of Flux::forward that does not depend on the timestep: input casts + RoPE table.
// p.R > 0 (a context evaluation): the context's rows of the table, and its rows [S, S + R) of every sample of the bf16 img_in operand
// p.o.cfg (true CFG): `in` is the loop's internal batch of 2 * Bs samples whose txt / y / ids / context pointers are the caller's Bs samples'; the
// negative's txt and y fill the second halves, and samples Bs .. 2 Bs - 1 take the table and the context rows of samples 0 .. Bs - 1.  Null: nothing changes.
// p.o.ctl (a channel-conditioned model): the conditioning (Bs, S, cond) goes into columns [C, C + cond) of every row of the img_in operand, once.
int prepare_static(fmi_flux* m, const fmi_flux_inputs* in, const EvalPlan& p, hipStream_t s) {
  auto& w = m->ws;
  const fmi_flux_denoise_options& o = p.o;
  const int B = in->B, Bs = p.Bs, R = p.R, S = in->S, T = in->T, C = m->cfg.in_channels;
  const int64_t n_txt = (int64_t)Bs * T * m->cfg.joint_attention_dim, n_y = (int64_t)Bs * m->cfg.pooled_projection_dim;
  PhaseTimer pt(m, s, PH_EMBED);
  FMI_TRY(launch_cast_to_bf16(in->txt, in->txt_dtype, w.txt_bf, n_txt, s));
  FMI_TRY(launch_cast_to_f32(in->y, in->y_dtype, w.yf, n_y, s));
  if (o.cfg) {
    FMI_TRY(launch_cast_to_bf16(o.cfg->neg_txt, o.cfg->neg_txt_dtype, w.txt_bf + n_txt, n_txt, s));
    FMI_TRY(launch_cast_to_f32(o.cfg->neg_y, o.cfg->neg_y_dtype, w.yf + n_y, n_y, s));
  }
  // pe = EmbedNd(cat([txt_ids, img_ids], 1)) (model.rs:807-810); one table per batch element
  const int tables = in->ids_per_sample ? Bs : 1;
  FMI_TRY(launch_rope_table(in->txt_ids, in->img_ids, tables, T, S, m->cfg.axes_dim, m->cfg.theta, w.pe, s, R ? o.ctx->ctx_ids : nullptr, R));
  if (o.cfg && in->ids_per_sample) {
    const size_t half = (size_t)Bs * (T + S + R) * PE_ROW_FLOATS;
    FMI_HIP_TRY(hipMemcpyAsync(w.pe + half, w.pe, half * 4, hipMemcpyDeviceToDevice, s));
  }
  if (o.ctl) return launch_cast_cols_bf16(o.ctl->cond, o.ctl->cond_dtype, (int64_t)B * S, (int64_t)Bs * S, m->cond, w.img_bf, C + m->cond, C, s);
  if (!R) return FMI_OK;
  return launch_cast_rows_bf16(o.ctx->ctx, o.ctx->ctx_dtype, (int64_t)R * C, w.img_bf + (size_t)S * C, (int64_t)(S + R) * C, B, (int64_t)R * C, s, Bs);
}
// vec_ = time_in(temb(t)) [+ guidance_in(temb(g))] + vector_in(y)   (model.rs:813-820) -> vec_out (B, D) f32
int compute_vec(fmi_flux* m, const fmi_flux_inputs* in, const float* timesteps_dev, float* vec_out, hipStream_t s) {
  auto& w = m->ws;
  const fmi_flux_config& c = m->cfg;
  const int B = in->B, D = m->D;
  FMI_TRY(launch_timestep_embedding(timesteps_dev, B, 256, w.temb, s));
  FMI_TRY(launch_gemv(w.temb, m->time1.w, m->time1.b, w.h1, B, D, 256, 0, 0, s));
  FMI_TRY(launch_gemv(w.h1, m->time2.w, m->time2.b, vec_out, B, D, D, 1, 0, s));
  if (c.guidance_embeds) {
    if (!in->guidance) return fail(FMI_ERR_INVALID, "flux: guidance_embeds model needs a guidance vector");
    FMI_TRY(launch_timestep_embedding(in->guidance, B, 256, w.temb, s));
    FMI_TRY(launch_gemv(w.temb, m->guid1.w, m->guid1.b, w.h1, B, D, 256, 0, 0, s));
    FMI_TRY(launch_gemv(w.h1, m->guid2.w, m->guid2.b, vec_out, B, D, D, 1, 1, s));
  }
  FMI_TRY(launch_gemv(w.yf, m->vecin1.w, m->vecin1.b, w.h1, B, D, c.pooled_projection_dim, 0, 0, s));
  FMI_TRY(launch_gemv(w.h1, m->vecin2.w, m->vecin2.b, vec_out, B, D, D, 1, 1, s));
  return FMI_OK;
}

// The same for all R = n_steps * B rows of an image at once (fmi_flux_denoise; row i*B + b = step i, sample b): the guidance and pooled-text terms do not
// depend on the step — computed once —, the timestep term runs as row passes over its two matrices (each output row depends on its own input row only),
// and the three are added in compute_vec's order ((time + guidance) + pooled): the same f32 operations, hence the same bits, in 32 launches instead of 350.
int compute_vec_steps(fmi_flux* m, const fmi_flux_inputs* in, const float* tv_dev, int n_steps, float* vec_steps, float* temb_steps, float* h1_steps, hipStream_t s) {
  auto& w = m->ws;
  const fmi_flux_config& c = m->cfg;
  const int B = in->B, D = m->D, R = n_steps * B;
  FMI_TRY(launch_timestep_embedding(tv_dev, R, 256, temb_steps, s));
  FMI_TRY(launch_gemv(temb_steps, m->time1.w, m->time1.b, h1_steps, R, D, 256, 0, 0, s));
  FMI_TRY(launch_gemv(h1_steps, m->time2.w, m->time2.b, vec_steps, R, D, D, 1, 0, s));
  float* gterm = nullptr;
  if (c.guidance_embeds) {
    if (!in->guidance) return fail(FMI_ERR_INVALID, "flux: guidance_embeds model needs a guidance vector");
    gterm = h1_steps;  // (free again: rows 0 .. B-1 hold the guidance term, rows B .. 2B-1 the pooled-text term)
    FMI_TRY(launch_timestep_embedding(in->guidance, B, 256, w.temb, s));
    FMI_TRY(launch_gemv(w.temb, m->guid1.w, m->guid1.b, w.h1, B, D, 256, 0, 0, s));
    FMI_TRY(launch_gemv(w.h1, m->guid2.w, m->guid2.b, gterm, B, D, D, 1, 0, s));
  }
  float* vterm = h1_steps + (size_t)B * D;
  FMI_TRY(launch_gemv(w.yf, m->vecin1.w, m->vecin1.b, w.h1, B, D, c.pooled_projection_dim, 0, 0, s));
  FMI_TRY(launch_gemv(w.h1, m->vecin2.w, m->vecin2.b, vterm, B, D, D, 1, 0, s));
  return launch_add2_rows(vec_steps, gterm, vterm, R, B, D, s);
}

// The first-block step cache of one cached loop: the caller's settings and the state the steps hand on.
struct StepCacheRun {
  const fmi_flux_step_cache* o;  // the caller's settings and outputs
  int step = 0;        // index of the evaluation under way
  bool valid = false;  // a computed step has left r_ref and the delta behind
  int ref = 0;         // m->sc_r[ref] is r_ref, m->sc_r[ref ^ 1] receives this step's residual
};

// After double block 0 of a cached evaluation: r = X1 - X0 (X0's buffer takes the copy of X1), the per-sample distances to r_ref through one small device-to-host
// copy and ONE hipStreamSynchronize, the decision on the host, and on reuse XF = X1 + delta written where the final layer reads the image rows.
int step_cache_decide(fmi_flux* m, StepCacheRun* sc, int B, int S, int T, hipStream_t s, bool* reuse) {
  auto& w = m->ws;
  const int64_t n = (int64_t)S * m->D, L = S + T;
  PhaseTimer pt(m, s, PH_EMBED);
  const int i = sc->step;
  float* const r_ref = m->sc_r[sc->ref].as<float>();
  FMI_TRY(launch_step_cache_residual(w.x_img, n, m->sc_x0.as<float>(), sc->valid ? r_ref : nullptr, m->sc_r[sc->ref ^ 1].as<float>(), m->sc_part.as<float>(),
                                     m->sc_sums.as<double>(), B, n, s));
  bool below = true;  // every sample's distance is under the threshold (a NaN distance is not)
  if (sc->valid) {
    FMI_HIP_TRY(hipMemcpyAsync(m->sc_host, m->sc_sums.ptr, (size_t)2 * B * sizeof(double), hipMemcpyDeviceToHost, s));
    FMI_HIP_TRY(hipStreamSynchronize(s));
  }
  for (int b = 0; b < B; ++b) {
    // d_b = num_b / den_b in double, +inf for den_b == 0, -1 while nothing has been computed yet; reported — and compared — as f32
    float d = -1.f;
    if (sc->valid) d = m->sc_host[2 * b + 1] == 0.0 ? INFINITY : (float)(m->sc_host[2 * b] / m->sc_host[2 * b + 1]);
    if (sc->o->distances_out) sc->o->distances_out[(size_t)i * B + b] = d;
    below = below && d < sc->o->threshold;
  }
  const int f = sc->o->force ? sc->o->force[i] : -1;
  *reuse = sc->valid && (f == 1 || (f < 0 && sc->o->threshold > 0.f && below));
  if (sc->o->decisions_out) sc->o->decisions_out[i] = *reuse ? 1 : 0;
  if (*reuse) FMI_TRY(launch_step_cache_apply(w.x_img, n, m->sc_delta.as<float>(), w.x + (size_t)T * m->D, L * m->D, B, n, s));
  return FMI_OK;
}

// One model evaluation given prepared static inputs; img_f32 (Bs,S,C) -> pred (B,S,C) f32.
// p.R: context rows per sample.  The image stream then has in->S + R rows per sample — rows [in->S, in->S + R) of w.img_bf and of the RoPE table were
// written by prepare_static — and everything between the input assembly and the final layer sees only that longer stream; img_f32 and pred stay (., in->S, C).
// p.Bs: samples of img_f32; fewer than in->B under true CFG (sample b of the operand is the state's sample b % Bs) — the input assembly is all
// that knows.
// mod_pre: this step's (B, n_mod) modulation vectors where the loop precomputed them, else null.
// txt_pre: txt_in(txt) where the loop computed it once for all steps (it does not depend on the latent or on t), else null.
// sc: the step cache of a cached loop, else null — and with null every launch below is the one it always was.
// inj: the ControlNet samples this evaluation adds to its f32 stream, else null — likewise.  On a ControlNet handle (m->is_cn) the evaluation
// instead captures those samples after every block into m->cn_samples and ends after the last block: it has no final layer, and pred is not written.
// ipj: the IP-Adapter of this evaluation, else null — likewise.  With it the image stream's q|k|v projection of every double block takes the plain
// bf16 epilogue (the fused relayout keeps only the rotated q) and the block ends with x_img += c * ip(raw q), before the ControlNet's injection.
int forward_core(fmi_flux* m, const fmi_flux_inputs* in, const EvalPlan& p, const float* img_f32, const float* timesteps_dev, float* pred, const float* mod_pre,
                 const float* txt_pre, StepCacheRun* sc, const CnInject* inj, const IpInject* ipj, hipStream_t s) {
  auto& w = m->ws;
  const fmi_flux_config& c = m->cfg;
  const int B = in->B, Bs = p.Bs, R = p.R, Ss = in->S, S = Ss + R, T = in->T, L = S + T;  // Ss: the state's rows, S: the image stream's
  const int D = m->D, Mh = m->M, H = m->H, C = c.in_channels;
  const int nmod = (int)m->n_mod;
  const int64_t pe_bs = in->ids_per_sample ? (int64_t)L * PE_ROW_FLOATS : 0;
  const float att_scale = 1.0f / sqrtf(128.0f);
  const bool fp8 = m->fp8;
  const int qk = m->q8_kind;  // 1 e4m3, 2 int8
  // sequence parallel: S, T (and the ids) are this rank's shard; only the attention sees the other ranks (attention_sp)
  const bool sp = m->sp_world > 1 && m->sp_a2a;
  if (sp && (B != 1 || fp8)) return fail(FMI_ERR_UNSUPPORTED, "flux: sequence parallelism runs one image (B = 1) in bf16 mode");
  if (m->calib) {
    if (sp || fp8) return fail(FMI_ERR_STATE, "flux: int8 calibration runs on one device in bf16 mode");
    ++m->calib_evals;
  }
  // (normally computed by fmi_flux_set_fp8_attention(m, 2) / quantize_8bit, outside any evaluation; this is the path of a weight reloaded
  // afterwards: 4 n_double + 2 n_single small synchronous device-to-host copies, once — not legal under stream capture, like set_tensor itself)
  if (m->fp8_attn == 2 && !sp && !m->attn_scales_valid) FMI_TRY(compute_attention_scales(m));
  const bool qk8_any = m->fp8_attn == 2 && !sp;  // opt-in: e4m3 q, k in front of QK^T whatever the block linears run on
  const int BT = B * T;  // a8 / a8s rows: [txt (B*T) | img (B*S)]
  // The two ControlNet hooks, after double block i (single = false) or single block i: `rows` = where the block left the image rows, sample b at rows + b * bs.
  //   capture (a ControlNet handle)   sample = bf16(zero_linear(bf16(rows))): the rows cast into the free LayerNorm output buffer, then the existing GEMM launcher
  //   inject (the main model)         rows += c * f32(sample[i // ceil(n_main / n_net)]), one launch (controlnet.hip)
  const auto cn_hook = [&](bool single, int i, float* rows, int64_t bs) -> int {
    if (m->is_cn) {
      PhaseTimer pt(m, s, PH_EMBED);
      FMI_TRY(launch_cast_rows_bf16(rows, FMI_F32, bs, w.xm, (int64_t)S * D, B, (int64_t)S * D, s));
      Dense& zl = single ? m->cn_sgl[i] : m->cn_dbl[i];
      GemmProblem q = make_problem(zl, w.xm, D, B * S, m->cn_samples.as<bf16_t>() + ((single ? m->cn_dbl.size() : 0) + i) * m->cn_elems, D, EPI_STORE_BF16);
      return gemm1(m, q, zl, s);
    }
    if (!inj) return FMI_OK;
    const int n_net = (int)(single ? inj->net->cn_sgl.size() : inj->net->cn_dbl.size()), n_main = single ? c.num_single_layers : c.num_layers;
    if (!n_net) return FMI_OK;  // (a ControlNet without single blocks leaves the single blocks alone)
    const int k = i / ((n_main + n_net - 1) / n_net);
    PhaseTimer pt(m, s, PH_EMBED);
    return launch_add_scaled_rows_bf16(rows, bs, inj->net->cn_samples.as<bf16_t>() + ((single ? inj->net->cn_dbl.size() : 0) + k) * inj->net->cn_elems, B, S, D, inj->c, s);
  };
  // The IP-Adapter hook, at the end of double block i and before the ControlNet's: the image-prompt attention of the block's own raw queries — the q third of
  // qkv_img, which nothing has overwritten since the block's q|k|v GEMM — added to the image stream, one launch (ip_adapter.hip).
  const auto ip_hook = [&](int i) -> int {
    if (!ipj) return FMI_OK;
    PhaseTimer pt(m, s, PH_ATTN);
    return launch_ip_attention(w.qkv_img, 3 * D, (int64_t)S * 3 * D, m->dbl[i].nq[0], ipj->a->k_of(i), ipj->a->v_of(i), w.x_img, (int64_t)S * D, B, H, S, ipj->a->N, ipj->c,
                               0, s);
  };
  {
    PhaseTimer pt(m, s, PH_EMBED);
    if (m->cond)  // the state into columns [0, C) of the [state | conditioning] operand, both halves of a true-CFG batch in the one launch (no context: R == 0)
      FMI_TRY(launch_cast_cols_bf16(img_f32, FMI_F32, (int64_t)B * S, (int64_t)Bs * S, C, w.img_bf, m->img_in.K, 0, s));
    else if (R || Bs != B) FMI_TRY(launch_cast_rows_bf16(img_f32, FMI_F32, (int64_t)Ss * C, w.img_bf, (int64_t)S * C, B, (int64_t)Ss * C, s, Bs));  // the state rows into their places
    else FMI_TRY(launch_cast_to_bf16(img_f32, FMI_F32, w.img_bf, (int64_t)B * S * C, s));
    if (!mod_pre) FMI_TRY(compute_vec(m, in, timesteps_dev, w.vec, s));
    // img = img_in(img), txt = txt_in(txt)   (model.rs:811-812) -> f32 residual streams
    GemmProblem p[2];
    p[0] = make_problem(m->img_in, w.img_bf, m->img_in.K, B * S, w.x_img, D, EPI_STORE_F32);  // K = C + the conditioning channels
    p[1] = make_problem(m->txt_in, w.txt_bf, c.joint_attention_dim, B * T, w.x_txt, D, EPI_STORE_F32);
    Dense* dn[2] = {&m->img_in, &m->txt_in};
    if (txt_pre) {  // the text stream starts every step from the same values: a 6 MB copy instead of a 13-GFLOP GEMM per step (same bits)
      FMI_HIP_TRY(hipMemcpyAsync(w.x_txt, txt_pre, (size_t)B * T * D * 4, hipMemcpyDeviceToDevice, s));
      FMI_TRY(gemm1(m, p[0], m->img_in, s));
    } else {
      FMI_TRY(gemm2(m, p, dn, 2, s));
    }
    if (m->is_cn)  // x = x_embedder(img) + controlnet_x_embedder(cond), the second term computed once per call (cn_embed_cond); c = 1: one exact f32 addition
      FMI_TRY(launch_add_scaled_rows_f32(w.x_img, (int64_t)S * D, m->cn_cx.as<float>(), B, S, D, 1.0f, s));
    // step cache: X0 leaves before block 0's epilogues update the stream in place
    if (sc) FMI_HIP_TRY(hipMemcpyAsync(m->sc_x0.ptr, w.x_img, (size_t)B * S * D * 4, hipMemcpyDeviceToDevice, s));
  }
  if (!mod_pre) {
    // every Modulation1/2 + LastLayer.ada_ln of the model in one GEMV: lin(silu(vec)) (model.rs:244-299,695-698)
    PhaseTimer pt(m, s, PH_MOD);
    if (m->mod_all.q_type) {  // quantised modulation matrix: bf16(silu(vec)) through the fused dequant-GEMM
      FMI_TRY(launch_silu_to_bf16(w.vec, w.vec_bf, (int64_t)B * D, s));
      GemmProblem p = make_problem(m->mod_all, w.vec_bf, D, B, w.mod, nmod, EPI_STORE_F32);
      FMI_TRY(gemm1(m, p, m->mod_all, s));
    } else {
      FMI_TRY(launch_gemv(w.vec, m->mod_all.w, m->mod_all.b, w.mod, B, nmod, D, 1, 0, s));
    }
  }
  const float* const mod = mod_pre ? mod_pre : w.mod;

  // ---------------- double-stream blocks (model.rs:523-565)
  bool reuse = false;  // step cache: this evaluation takes the cached output residual of every block after double block 0
  for (int i = 0; i < c.num_layers; ++i) {
    if (sc && i == 1) {  // (both chains of block 0 have joined the caller's stream)
      FMI_TRY(step_cache_decide(m, sc, B, S, T, s, &reuse));
      if (reuse) break;
    }
    auto& bw = m->dbl[i];
    const float* mi = mod + bw.mod_off[0];  // shift1, scale1, gate1, shift2, scale2, gate2
    const float* mt = mod + bw.mod_off[1];
    bf16_t* xm_txt = w.xm;
    bf16_t* xm_img = w.xm + (size_t)B * T * D;
    bool fused_img = false, fused_txt = false, qk8 = false;
    // which of the block's linears run on 8-bit operands (all of them in fp8 mode; the int8 mode's mask leaves some in bf16)
    const bool q_qkv = fp8 && bw.qkv[0].w8, q_out = fp8 && bw.proj[0].w8, q_m1 = fp8 && bw.mlp1[0].w8, q_m2 = fp8 && bw.mlp2[0].w8;
    {
      PhaseTimer pt(m, s, PH_LN);
      if (q_qkv) {
        FMI_TRY(launch_layernorm_mod_fp8_2(w.x_img, mi + D, mi, nmod, S, w.a8 + (size_t)BT * D, w.a8s + BT, B * S, w.x_txt, mt + D, mt, T, w.a8, w.a8s,
                                           B * T, D, 1e-6f, s, qk, bw.qkv[0].sm_inv, bw.qkv[1].sm_inv));
      } else {
        FMI_TRY(launch_layernorm_mod2(w.x_img, mi + D, mi, nmod, S, xm_img, B * S, w.x_txt, mt + D, mt, T, xm_txt, B * T, D, 1e-6f, s));
        FMI_TRY(calib_rec(m, bw.qkv[0], xm_img, D, B * S, s));
        FMI_TRY(calib_rec(m, bw.qkv[1], xm_txt, D, B * T, s));
      }
    }
    {
      PhaseTimer pt(m, s, PH_GEMM_QKV);
      GemmProblem p[2];
      p[0] = q_qkv ? make_problem_fp8(m, bw.qkv[0], BT, B * S, w.qkv_img, 3 * D, EPI_STORE_BF16)
                   : make_problem(bw.qkv[0], xm_img, D, B * S, w.qkv_img, 3 * D, EPI_STORE_BF16);
      p[1] = q_qkv ? make_problem_fp8(m, bw.qkv[1], 0, B * T, w.qkv_txt, 3 * D, EPI_STORE_BF16)
                   : make_problem(bw.qkv[1], xm_txt, D, B * T, w.qkv_txt, 3 * D, EPI_STORE_BF16);
      // joint order [txt, img] (model.rs:540-542): txt tokens at positions [0,T), img at [T,T+S)
      // fp8 attention operands only when BOTH streams take the fused epilogue (the stand-alone kernels write bf16)
      qk8 = ((q_qkv && m->fp8_attn) || (qk8_any && !bw.qkv[0].q_type && !bw.qkv[1].q_type)) && can_fuse_relayout(m, B * S, S, T) && can_fuse_relayout(m, B * T, T, 0);  // (either 8-bit mode; opt-in: any)
      const float q8 = qk8 ? m->q8_dbl[i] : 0.f, k8 = qk8 ? m->k8_dbl[i] : 0.f;
      fused_img = !ipj && with_qkv_relayout(m, p[0], bw.nq[0], bw.nk[0], pe_bs, S, T, L, q8, k8);  // (an adapter reads the raw q from qkv_img at the block's end)
      fused_txt = with_qkv_relayout(m, p[1], bw.nq[1], bw.nk[1], pe_bs, T, 0, L, q8, k8);
      Dense* dn[2] = {&bw.qkv[0], &bw.qkv[1]};
      FMI_TRY(gemm2(m, p, dn, 2, s));
    }
    if (!(fused_img && fused_txt)) {
      PhaseTimer pt(m, s, PH_RELAYOUT);
      // q,k: QkNorm + rope + head-major, joint order [txt, img] (model.rs:540-542)
      if (!fused_txt) {
        FMI_TRY(launch_qk_norm_rope(w.qkv_txt, w.qkv_txt + D, 3 * D, (int64_t)T * 3 * D, bw.nq[1], bw.nk[1], w.pe, pe_bs, w.Qh, w.Kh, B, H, T, 0, L, s));
        FMI_TRY(launch_v_transpose(w.qkv_txt + 2 * D, 3 * D, (int64_t)T * 3 * D, w.Vt, B, H, T, 0, w.Lpad, s));
      }
      if (!fused_img) {
        FMI_TRY(launch_qk_norm_rope(w.qkv_img, w.qkv_img + D, 3 * D, (int64_t)S * 3 * D, bw.nq[0], bw.nk[0], w.pe, pe_bs, w.Qh, w.Kh, B, H, S, T, L, s));
        FMI_TRY(launch_v_transpose(w.qkv_img + 2 * D, 3 * D, (int64_t)S * 3 * D, w.Vt, B, H, S, T, w.Lpad, s));
      }
    }
    {
      PhaseTimer pt(m, s, PH_ATTN);
      AttnOut o{};
      o.p0 = w.attn_txt, o.rows0 = T, o.ld0 = D, o.bstride0 = (int64_t)T * D;
      o.p1 = w.attn_img, o.ld1 = D, o.bstride1 = (int64_t)S * D;
      const float sc = qk8 ? att_scale / (m->q8_dbl[i] * m->k8_dbl[i]) : att_scale;
      if (sp) FMI_TRY(attention_sp(m, o, T, S, sc, s));
      else FMI_TRY(launch_attention_ex(w.Qh, w.Kh, w.Vt, o, B, H, L, L, w.Lpad, sc, m->attn_thr, s, qk8 ? 1 : 0, nullptr, 0, qk8 ? -m->n8_dbl[i] : ATT_NO_EXP2, m->attn_kind));
    }
    if (m->two_streams && !fp8 && !sp && !m->profiling && !m->calib && !bw.proj[0].q_type && !bw.proj[1].q_type && !bw.mlp1[0].q_type && !bw.mlp1[1].q_type &&
        !bw.mlp2[0].q_type && !bw.mlp2[1].q_type && !m->split_k) {
      // the two chains are independent from here to the next block's joint attention: text on the side stream, image on the caller's
      bf16_t* hid_txt = w.hid;
      bf16_t* hid_img = w.hid + (size_t)B * T * Mh;
      FMI_HIP_TRY(hipEventRecord(m->ev_fork, s));
      FMI_HIP_TRY(hipStreamWaitEvent(m->side, m->ev_fork, 0));
      for (int st = 0; st < 2; ++st) {  // st 0 = image chain on s, 1 = text chain on the side stream
        hipStream_t q = st ? m->side : s;
        const int rows = st ? B * T : B * S, rpb = st ? T : S;
        const float* mo = st ? mt : mi;
        float* x = st ? w.x_txt : w.x_img;
        bf16_t* xm_ = st ? xm_txt : xm_img;
        bf16_t* hid_ = st ? hid_txt : hid_img;
        GemmProblem p = make_problem(bw.proj[st], st ? w.attn_txt : w.attn_img, D, rows, x, D, EPI_RESID_GATE_F32);
        with_gate(p, mo + 2 * D, rpb, nmod);
        FMI_TRY(gemm1(m, p, bw.proj[st], q));
        FMI_TRY(launch_layernorm_mod(x, mo + 4 * D, mo + 3 * D, nmod, rpb, xm_, rows, D, 1e-6f, q));
        p = make_problem(bw.mlp1[st], xm_, D, rows, hid_, Mh, EPI_GELU_BF16);
        FMI_TRY(gemm1(m, p, bw.mlp1[st], q));
        p = make_problem(bw.mlp2[st], hid_, Mh, rows, x, D, EPI_RESID_GATE_F32);
        with_gate(p, mo + 5 * D, rpb, nmod);
        FMI_TRY(gemm1(m, p, bw.mlp2[st], q));
      }
      FMI_HIP_TRY(hipEventRecord(m->ev_join, m->side));
      FMI_HIP_TRY(hipStreamWaitEvent(s, m->ev_join, 0));
      FMI_TRY(ip_hook(i));
      FMI_TRY(cn_hook(false, i, w.x_img, (int64_t)S * D));  // (behind the join: the image chain ran on s, and the hook's launches are ordered after both chains)
      continue;
    }
    {
      PhaseTimer pt(m, s, PH_GEMM_PROJ);
      GemmProblem p[2];
      if (q_out) {
        FMI_TRY(quantize_act(m, bw.proj[0], w.attn_img, D, B * S, BT, s));
        FMI_TRY(quantize_act(m, bw.proj[1], w.attn_txt, D, B * T, 0, s));
      } else {
        FMI_TRY(calib_rec(m, bw.proj[0], w.attn_img, D, B * S, s));
        FMI_TRY(calib_rec(m, bw.proj[1], w.attn_txt, D, B * T, s));
      }
      p[0] = q_out ? make_problem_fp8(m, bw.proj[0], BT, B * S, w.x_img, D, EPI_RESID_GATE_F32)
                   : make_problem(bw.proj[0], w.attn_img, D, B * S, w.x_img, D, EPI_RESID_GATE_F32);
      with_gate(p[0], mi + 2 * D, S, nmod);
      p[1] = q_out ? make_problem_fp8(m, bw.proj[1], 0, B * T, w.x_txt, D, EPI_RESID_GATE_F32)
                   : make_problem(bw.proj[1], w.attn_txt, D, B * T, w.x_txt, D, EPI_RESID_GATE_F32);
      with_gate(p[1], mt + 2 * D, T, nmod);
      Dense* dn[2] = {&bw.proj[0], &bw.proj[1]};
      FMI_TRY(gemm2(m, p, dn, 2, s));
    }
    {
      PhaseTimer pt(m, s, PH_LN);
      if (q_m1) {
        FMI_TRY(launch_layernorm_mod_fp8_2(w.x_img, mi + 4 * D, mi + 3 * D, nmod, S, w.a8 + (size_t)BT * D, w.a8s + BT, B * S, w.x_txt, mt + 4 * D,
                                           mt + 3 * D, T, w.a8, w.a8s, B * T, D, 1e-6f, s, qk, bw.mlp1[0].sm_inv, bw.mlp1[1].sm_inv));
      } else {
        FMI_TRY(launch_layernorm_mod2(w.x_img, mi + 4 * D, mi + 3 * D, nmod, S, xm_img, B * S, w.x_txt, mt + 4 * D, mt + 3 * D, T, xm_txt, B * T, D,
                                      1e-6f, s));
        FMI_TRY(calib_rec(m, bw.mlp1[0], xm_img, D, B * S, s));
        FMI_TRY(calib_rec(m, bw.mlp1[1], xm_txt, D, B * T, s));
      }
    }
    {
      PhaseTimer pt(m, s, PH_GEMM_MLP);
      bf16_t* hid_txt = w.hid;
      bf16_t* hid_img = w.hid + (size_t)B * T * Mh;
      GemmProblem p[2];
      p[0] = q_m1 ? make_problem_fp8(m, bw.mlp1[0], BT, B * S, hid_img, Mh, EPI_GELU_BF16) : make_problem(bw.mlp1[0], xm_img, D, B * S, hid_img, Mh, EPI_GELU_BF16);
      p[1] = q_m1 ? make_problem_fp8(m, bw.mlp1[1], 0, B * T, hid_txt, Mh, EPI_GELU_BF16) : make_problem(bw.mlp1[1], xm_txt, D, B * T, hid_txt, Mh, EPI_GELU_BF16);
      Dense* dn1[2] = {&bw.mlp1[0], &bw.mlp1[1]};
      FMI_TRY(gemm2(m, p, dn1, 2, s));
      if (q_m2) {  // hid is (B*L, M) with the txt rows first, like a8
        if (bw.mlp2[0].sm_inv || bw.mlp2[1].sm_inv) {  // (smoothed: each stream's MLP-out has its own per-channel factors)
          FMI_TRY(quantize_act(m, bw.mlp2[1], hid_txt, Mh, B * T, 0, s));
          FMI_TRY(quantize_act(m, bw.mlp2[0], hid_img, Mh, B * S, BT, s));
        } else {
          FMI_TRY(quantize_act(m, bw.mlp2[0], w.hid, Mh, B * L, 0, s));  // (both streams' MLP-out read it: same form, one pass)
        }
      } else {
        FMI_TRY(calib_rec(m, bw.mlp2[0], hid_img, Mh, B * S, s));
        FMI_TRY(calib_rec(m, bw.mlp2[1], hid_txt, Mh, B * T, s));
      }
      p[0] = q_m2 ? make_problem_fp8(m, bw.mlp2[0], BT, B * S, w.x_img, D, EPI_RESID_GATE_F32)
                  : make_problem(bw.mlp2[0], hid_img, Mh, B * S, w.x_img, D, EPI_RESID_GATE_F32);
      with_gate(p[0], mi + 5 * D, S, nmod);
      p[1] = q_m2 ? make_problem_fp8(m, bw.mlp2[1], 0, B * T, w.x_txt, D, EPI_RESID_GATE_F32)
                  : make_problem(bw.mlp2[1], hid_txt, Mh, B * T, w.x_txt, D, EPI_RESID_GATE_F32);
      with_gate(p[1], mt + 5 * D, T, nmod);
      Dense* dn2[2] = {&bw.mlp2[0], &bw.mlp2[1]};
      FMI_TRY(gemm2(m, p, dn2, 2, s));
    }
    FMI_TRY(ip_hook(i));
    FMI_TRY(cn_hook(false, i, w.x_img, (int64_t)S * D));
  }

  // ---------------- cat([txt, img], 1) (model.rs:827) then single-stream blocks (model.rs:638-662)
  if (sc && c.num_layers == 1) FMI_TRY(step_cache_decide(m, sc, B, S, T, s, &reuse));
  // (a reused step has its image rows of the joint stream already and runs neither the concat nor a single block)
  for (int b = 0; b < B && w.x_txt != w.x && !reuse; ++b) {  // (B == 1: the streams alias the joint buffer, ensure_workspace)
    FMI_HIP_TRY(hipMemcpyAsync(w.x + (size_t)b * L * D, w.x_txt + (size_t)b * T * D, (size_t)T * D * 4, hipMemcpyDeviceToDevice, s));
    FMI_HIP_TRY(hipMemcpyAsync(w.x + ((size_t)b * L + T) * D, w.x_img + (size_t)b * S * D, (size_t)S * D * 4, hipMemcpyDeviceToDevice, s));
  }
  const int ldbig = 3 * D + Mh;
  for (int i = 0; i < (reuse ? 0 : c.num_single_layers); ++i) {
    auto& bw = m->sgl[i];
    const float* mo = mod + bw.mod_off;  // shift, scale, gate
    bool fused = false;
    const bool q_w1 = fp8 && bw.w1.w8, q_w2 = fp8 && bw.w2.w8;
    const bool qk8 = ((q_w1 && m->fp8_attn) || (qk8_any && !bw.w1.q_type)) && can_fuse_relayout(m, B * L, L, 0);
    {
      PhaseTimer pt(m, s, PH_LN);
      if (q_w1) {
        FMI_TRY(launch_layernorm_mod_fp8(w.x, mo + D, mo, nmod, L, w.a8, w.a8s, B * L, D, 1e-6f, s, qk, bw.w1.sm_inv));
      } else {
        FMI_TRY(launch_layernorm_mod(w.x, mo + D, mo, nmod, L, w.xm, B * L, D, 1e-6f, s));
        FMI_TRY(calib_rec(m, bw.w1, w.xm, D, B * L, s));
      }
    }
    {
      PhaseTimer pt(m, s, PH_GEMM_QKV);
      // [q|k|v|gelu(proj_mlp)] in one GEMM; the concat of model.rs:660 is never materialised
      GemmProblem p = q_w1 ? make_problem_fp8(m, bw.w1, 0, B * L, w.big, ldbig, EPI_GELU_FROM_COL)
                           : make_problem(bw.w1, w.xm, D, B * L, w.big, ldbig, EPI_GELU_FROM_COL);
      p.gelu_from = 3 * D;
      fused = with_qkv_relayout(m, p, bw.nq, bw.nk, pe_bs, L, 0, L, qk8 ? m->q8_sgl[i] : 0.f, qk8 ? m->k8_sgl[i] : 0.f);
      FMI_TRY(gemm1(m, p, bw.w1, s));
    }
    if (!fused) {
      PhaseTimer pt(m, s, PH_RELAYOUT);
      FMI_TRY(launch_qk_norm_rope(w.big, w.big + D, ldbig, (int64_t)L * ldbig, bw.nq, bw.nk, w.pe, pe_bs, w.Qh, w.Kh, B, H, L, 0, L, s));
      FMI_TRY(launch_v_transpose(w.big + 2 * D, ldbig, (int64_t)L * ldbig, w.Vt, B, H, L, 0, w.Lpad, s));
    }
    {
      PhaseTimer pt(m, s, PH_ATTN);
      // attention output overwrites the (now consumed) v slot, right in front of gelu(mlp):
      // big[:, 2D : 3D+M] is exactly cat([attn, gelu(mlp)], -1)
      AttnOut o{};
      o.p0 = nullptr, o.rows0 = 0;
      o.p1 = w.big + 2 * D, o.ld1 = ldbig, o.bstride1 = (int64_t)L * ldbig;
      const float sc = qk8 ? att_scale / (m->q8_sgl[i] * m->k8_sgl[i]) : att_scale;
      if (sp) FMI_TRY(attention_sp(m, o, T, S, sc, s));
      else FMI_TRY(launch_attention_ex(w.Qh, w.Kh, w.Vt, o, B, H, L, L, w.Lpad, sc, m->attn_thr, s, qk8 ? 1 : 0, nullptr, 0, qk8 ? -m->n8_sgl[i] : ATT_NO_EXP2, m->attn_kind));
    }
    {
      PhaseTimer pt(m, s, PH_GEMM_PROJ);
      if (q_w2) FMI_TRY(quantize_act(m, bw.w2, w.big + 2 * D, ldbig, B * L, 0, s));
      else FMI_TRY(calib_rec(m, bw.w2, w.big + 2 * D, ldbig, B * L, s));
      GemmProblem p = q_w2 ? make_problem_fp8(m, bw.w2, 0, B * L, w.x, D, EPI_RESID_GATE_F32)
                           : make_problem(bw.w2, w.big + 2 * D, ldbig, B * L, w.x, D, EPI_RESID_GATE_F32);
      with_gate(p, mo + 2 * D, L, nmod);
      FMI_TRY(gemm1(m, p, bw.w2, s));
    }
    FMI_TRY(cn_hook(true, i, w.x + (size_t)T * D, (int64_t)L * D));
  }
  if (m->is_cn) return FMI_OK;
  if (sc) {
    if (!reuse) {  // a computed step: delta = XF - X1 (the copy taken with the residual), this step's residual becomes the reference
      PhaseTimer pt(m, s, PH_EMBED);
      FMI_TRY(launch_step_cache_delta(w.x + (size_t)T * D, (int64_t)L * D, m->sc_x0.as<float>(), m->sc_delta.as<float>(), B, (int64_t)S * D, s));
      sc->ref ^= 1, sc->valid = true;
    }
    ++sc->step;
  }

  // ---------------- img = img[:, T:] ; LastLayer (model.rs:694-705): chunks = (scale, shift) — on the state's rows only: a context's rows end here
  {
    PhaseTimer pt(m, s, PH_FINAL);
    const float* mf = mod + m->mod_final_off;
    for (int b = 0; b < B; ++b)
      FMI_TRY(launch_layernorm_mod(w.x + ((size_t)b * L + T) * D, mf + (size_t)b * nmod, mf + (size_t)b * nmod + D, 0, 0,
                                   w.xm + (size_t)b * Ss * D, Ss, D, 1e-6f, s));
    GemmProblem p = make_problem(m->final_proj, w.xm, D, B * Ss, pred, C, EPI_STORE_F32);
    FMI_TRY(gemm1(m, p, m->final_proj, s));
  }
  return FMI_OK;
}

int check_inputs(fmi_flux* m, const fmi_flux_inputs* in) {
  if (!m || !in) return fail(FMI_ERR_INVALID, "flux: null handle or inputs");
  if (in->B <= 0 || in->S <= 0 || in->T <= 0) return fail(FMI_ERR_INVALID, "flux: B, S, T must be positive");
  if (in->B > 8) return fail(FMI_ERR_UNSUPPORTED, "flux: batch > 8 per device not supported (shard across GPUs)");
  if (!in->img_ids || !in->txt || !in->txt_ids || !in->y) return fail(FMI_ERR_INVALID, "flux: null input tensor");
  FMI_TRY(use_device(m));
  return check_ready(m);
}

// Every refusal of a forward or denoise call — of its arguments, each option and each combination (the table at fmi_flux_denoise_with) — in the one place, before the call's
// stream is used or anything is launched or allocated for it (check_inputs makes the handle's device current and completes a freshly loaded model: the model's state, not the
// call's).  *p: the accepted call's plan.  A forward is n_steps == 1 with ctx / ctl only.  bad_io: the entry's message when a pointer outside `in` and `o` is unusable, else null.
int validate(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_denoise_options& o, const fmi_flux_controlnet* cn, const fmi_flux_ip* ip, int n_steps, const char* bad_io,
             EvalPlan* p) {
  if (m && m->is_cn) return fail(FMI_ERR_UNSUPPORTED, "flux: a ControlNet handle is evaluated through the main model (fmi_flux_forward_controlnet / fmi_flux_denoise_controlnet) or fmi_flux_controlnet_eval");
  if ((o.x0 || o.noise || o.mask) && !(o.x0 && o.noise && o.mask)) return fail(FMI_ERR_INVALID, "flux_denoise: x0, noise and mask go together (all three or none)");
  FMI_TRY(check_inputs(m, in));
  if (bad_io) return fail(FMI_ERR_INVALID, bad_io);
  const bool sp = m->sp_world > 1 && m->sp_a2a;
  const auto f32_or_bf16 = [](fmi_dtype t) { return t == FMI_F32 || t == FMI_BF16; };
  *p = EvalPlan{o, 0, in->B};
  if (const fmi_flux_context* ctx = o.ctx; ctx && ctx->R != 0) {  // R == 0 is no context
    if (ctx->R < 0) return fail(FMI_ERR_INVALID, "flux: context R must not be negative");
    if (!ctx->ctx || !ctx->ctx_ids) return fail(FMI_ERR_INVALID, "flux: a context of R > 0 rows needs ctx and ctx_ids");
    if (!f32_or_bf16(ctx->ctx_dtype)) return fail(FMI_ERR_INVALID, "flux: ctx_dtype must be F32 or BF16");
    if (sp) return fail(FMI_ERR_UNSUPPORTED, "flux: a context is not supported under sequence parallelism");
    p->R = ctx->R;
  }
  if (!m->cond && o.ctl) return fail(FMI_ERR_INVALID, "flux: a control was given to a model without conditioning channels (fmi_flux_create_cond)");
  if (m->cond) {  // a channel-conditioned model needs a control at every evaluation
    if (!o.ctl || !o.ctl->cond)
      return fail(FMI_ERR_INVALID, "flux: this model has " + std::to_string(m->cond) + " conditioning channels: every evaluation needs a control (fmi_flux_forward_control, fmi_flux_denoise_with)");
    if (!f32_or_bf16(o.ctl->cond_dtype)) return fail(FMI_ERR_INVALID, "flux: cond_dtype must be F32 or BF16");
    if (sp) return fail(FMI_ERR_UNSUPPORTED, "flux: a control is not supported under sequence parallelism");
    if (p->R) return fail(FMI_ERR_UNSUPPORTED, "flux: a context and a control are not combined");
  }
  if (const fmi_flux_true_cfg* cfg = o.cfg) {
    if (o.cache) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: true CFG is not combined with the step cache");
    if (!cfg->neg_txt || !cfg->neg_y) return fail(FMI_ERR_INVALID, "flux_denoise: true CFG needs neg_txt and neg_y");
    if (!f32_or_bf16(cfg->neg_txt_dtype) || !f32_or_bf16(cfg->neg_y_dtype)) return fail(FMI_ERR_INVALID, "flux_denoise: neg_txt_dtype and neg_y_dtype must be F32 or BF16");
    if (!(cfg->scale >= 0.f) || std::isinf(cfg->scale)) return fail(FMI_ERR_INVALID, "flux_denoise: the true-CFG scale must be finite and >= 0");
    if (p->Bs > 4) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: B > 4 not supported under true CFG (the loop evaluates 2 B samples; the per-device limit is 8)");
    if (sp) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: true CFG is not supported under sequence parallelism (it runs B = 1)");
    if (m->calib) return fail(FMI_ERR_STATE, "flux_denoise: no true CFG while int8 calibration is recording");
    if (m->cfg.guidance_embeds && !in->guidance) return fail(FMI_ERR_INVALID, "flux: guidance_embeds model needs a guidance vector");
  }
  if ((int64_t)n_steps * (o.cfg ? 2 : 1) * p->Bs > 4096) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: n_steps * B > 4096 (ws.tv holds 4096 rows; true CFG counts 2 B)");
  if (const fmi_flux_step_cache* cache = o.cache) {
    if (o.ctl) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: the step cache is not combined with a control");
    if (!(cache->threshold >= 0.f)) return fail(FMI_ERR_INVALID, "flux_denoise: the step-cache threshold must be >= 0 (and not NaN)");
    for (int i = 0; cache->force && i < n_steps; ++i)
      if (cache->force[i] < -1 || cache->force[i] > 1 || (i == 0 && cache->force[i] == 1))
        return fail(FMI_ERR_INVALID, "flux_denoise: step-cache force entries are -1, 0 or 1, and step 0 cannot be reused (force[0] != 1)");
    if (m->cfg.num_layers < 1) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: the step cache needs at least one double block");
    if (sp) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: the step cache is not supported under sequence parallelism");
    if (m->calib) return fail(FMI_ERR_STATE, "flux_denoise: no step cache while int8 calibration is recording");
  }
  if (cn) {  // one ControlNet; several at once, union modes and the pixel-space hint block are out of scope
    fmi_flux* net = cn->net;
    if (!net || !net->is_cn) return fail(FMI_ERR_INVALID, "flux: controlnet->net is not a ControlNet handle (fmi_flux_create_controlnet)");
    if (!cn->cond) return fail(FMI_ERR_INVALID, "flux: a ControlNet needs cond, the packed latents of the control image (B,S,in_channels)");
    if (!f32_or_bf16(cn->cond_dtype)) return fail(FMI_ERR_INVALID, "flux: controlnet cond_dtype must be F32 or BF16");
    if (!std::isfinite(cn->scale)) return fail(FMI_ERR_INVALID, "flux: the ControlNet scale must be finite");
    for (int i = 0; cn->step_scales && i < n_steps; ++i)
      if (!std::isfinite(cn->step_scales[i])) return fail(FMI_ERR_INVALID, "flux_denoise: every entry of the ControlNet's step_scales must be finite");
    const fmi_flux_config &a = m->cfg, &b = net->cfg;
    if (net->D != m->D || a.num_attention_heads != b.num_attention_heads || a.joint_attention_dim != b.joint_attention_dim ||
        a.pooled_projection_dim != b.pooled_projection_dim || a.in_channels != b.in_channels || a.theta != b.theta || a.axes_dim[0] != b.axes_dim[0] ||
        a.axes_dim[1] != b.axes_dim[1] || a.axes_dim[2] != b.axes_dim[2])
      return fail(FMI_ERR_INVALID, "flux: the ControlNet's width, heads, joint_attention_dim, pooled_projection_dim, axes_dim, theta and in_channels must be the main model's");
    if (net->device != m->device) return fail(FMI_ERR_INVALID, "flux: the ControlNet lives on another device than the main model");
    if (b.guidance_embeds && !in->guidance) return fail(FMI_ERR_INVALID, "flux: a guidance_embeds ControlNet needs a guidance vector");
    if (p->R) return fail(FMI_ERR_UNSUPPORTED, "flux: a ControlNet is not combined with a context");
    if (m->cond) return fail(FMI_ERR_UNSUPPORTED, "flux: a ControlNet is not combined with a channel-conditioned model (cond_channels > 0)");
    if (o.cache) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: a ControlNet is not combined with the step cache");
    if (sp) return fail(FMI_ERR_UNSUPPORTED, "flux: a ControlNet is not supported under sequence parallelism");
    FMI_TRY(net->missing.ready("flux controlnet"));
    FMI_TRY(finalize(net));
    p->cn = cn;
  }
  if (ip) {  // one IP-Adapter; a CLIP vision encoder, several adapters at once and image prompts in the single blocks are out of scope
    const fmi_ip_adapter* a = ip->adapter;
    if (!a) return fail(FMI_ERR_INVALID, "flux: ip->adapter is NULL (fmi_ip_adapter_create)");
    if (!ip->embeds) return fail(FMI_ERR_INVALID, "flux: an IP-Adapter needs embeds, the image embeddings (B,embed_dim)");
    if (!f32_or_bf16(ip->embeds_dtype)) return fail(FMI_ERR_INVALID, "flux: the IP-Adapter's embeds_dtype must be F32 or BF16");
    if (!std::isfinite(ip->scale)) return fail(FMI_ERR_INVALID, "flux: the IP-Adapter scale must be finite");
    for (int i = 0; ip->step_scales && i < n_steps; ++i)
      if (!std::isfinite(ip->step_scales[i])) return fail(FMI_ERR_INVALID, "flux_denoise: every entry of the IP-Adapter's step_scales must be finite");
    if (a->D != m->D || a->J != m->cfg.joint_attention_dim || a->nd != m->cfg.num_layers)
      return fail(FMI_ERR_INVALID, "flux: the IP-Adapter's width, joint_attention_dim and number of double blocks must be the main model's");
    if (a->device != m->device) return fail(FMI_ERR_INVALID, "flux: the IP-Adapter lives on another device than the main model");
    if (p->R) return fail(FMI_ERR_UNSUPPORTED, "flux: an IP-Adapter is not combined with a context (reference rows)");
    if (o.cache) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: an IP-Adapter is not combined with the step cache");
    if (sp) return fail(FMI_ERR_UNSUPPORTED, "flux: an IP-Adapter is not supported under sequence parallelism");
    if (m->fp8) return fail(FMI_ERR_UNSUPPORTED, std::string("flux: an IP-Adapter is not supported in the ") + (m->q8_kind == 2 ? "int8" : "fp8") + " mode (it reads the bf16 q of the q|k|v projection)");
    if (m->fp8_attn == 2) return fail(FMI_ERR_UNSUPPORTED, "flux: an IP-Adapter is not supported with fp8 attention operands in every mode (fmi_flux_set_fp8_attention(m, 2))");
    FMI_TRY(a->missing.ready("flux ip_adapter"));
  }
  return FMI_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------- C-ABI
extern "C" void fmi_flux_default_config(fmi_flux_config* cfg, int guidance_embeds) {
  cfg->in_channels = 64;
  cfg->pooled_projection_dim = 768;
  cfg->joint_attention_dim = 4096;
  cfg->num_attention_heads = 24;
  cfg->num_layers = 19;
  cfg->num_single_layers = 38;
  cfg->guidance_embeds = guidance_embeds ? 1 : 0;
  cfg->axes_dim[0] = 16, cfg->axes_dim[1] = 56, cfg->axes_dim[2] = 56;
  cfg->theta = 10000;
}

static int flux_create(const fmi_flux_config* cfg, int cond_channels, bool controlnet, fmi_model_dtype dtype, fmi_flux** out);
extern "C" int fmi_flux_create(const fmi_flux_config* cfg, fmi_model_dtype dtype, fmi_flux** out) { return flux_create(cfg, 0, false, dtype, out); }
extern "C" int fmi_flux_cond_channels(const fmi_flux* m) { return m ? m->cond : 0; }
// A ControlNet (diffusers' FluxControlNetModel): cfg->num_layers / num_single_layers are the net's own (at least one double block; no single
// blocks is allowed), everything else must be the main model's when the two meet.  No norm_out / proj_out; controlnet_x_embedder and one zero-linear per block more.
extern "C" int fmi_flux_create_controlnet(const fmi_flux_config* cfg, fmi_model_dtype dtype, fmi_flux** out) {
  if (cfg && cfg->num_layers < 1) return fail(FMI_ERR_INVALID, "flux_create_controlnet: a ControlNet has at least one double block");
  return flux_create(cfg, 0, true, dtype, out);
}
extern "C" int fmi_flux_is_controlnet(const fmi_flux* m) { return m && m->is_cn ? 1 : 0; }

// x_embedder of a channel-conditioned checkpoint (FLUX.1 Fill / Canny / Depth) is (D, in_channels + cond_channels); everything else keeps in_channels.
extern "C" int fmi_flux_create_cond(const fmi_flux_config* cfg, int cond_channels, fmi_model_dtype dtype, fmi_flux** out) {
  return flux_create(cfg, cond_channels, false, dtype, out);
}
static int flux_create(const fmi_flux_config* cfg, int cond_channels, bool controlnet, fmi_model_dtype dtype, fmi_flux** out) {
  if (!cfg || !out) return fail(FMI_ERR_INVALID, "flux_create: null argument");
  if (cond_channels < 0 || cond_channels % 64 || (int64_t)cfg->in_channels + cond_channels > 512)
    return fail(FMI_ERR_INVALID, "flux_create_cond: cond_channels must be >= 0, a multiple of 64, and in_channels + cond_channels at most 512");
  if (dtype == FMI_MODEL_F16 || dtype == FMI_MODEL_F32)
    return fail(FMI_ERR_UNSUPPORTED, "flux_create: this build computes in bf16 on MFMA; F16/F32 model dtypes are not implemented");
  if (cfg->axes_dim[0] + cfg->axes_dim[1] + cfg->axes_dim[2] != 128 || (cfg->axes_dim[0] | cfg->axes_dim[1] | cfg->axes_dim[2]) & 1)
    return fail(FMI_ERR_INVALID, "flux_create: axes_dim must be even and sum to 128 (head dim)");
  if (cfg->num_attention_heads <= 0 || cfg->num_layers < 0 || cfg->num_single_layers < 0) return fail(FMI_ERR_INVALID, "flux_create: bad layer counts");
  if (cfg->in_channels % 64 || cfg->joint_attention_dim % 64 || cfg->pooled_projection_dim % 8)
    return fail(FMI_ERR_INVALID, "flux_create: in_channels and joint_attention_dim must be multiples of 64, pooled dim of 8");
  fmi_flux* m = new fmi_flux();
  m->cfg = *cfg;
  m->cond = cond_channels;
  m->is_cn = controlnet;
  hipGetDevice(&m->device);
  m->H = cfg->num_attention_heads;
  m->D = m->H * 128;  // HIDDEN_SIZE (model.rs:17) generalised as heads * pe_dim
  m->M = 4 * m->D;    // MLP_RATIO (model.rs:16)
  build_layout(m);
  if (ensure_arena(m, AR_BASE) != FMI_OK) {
    delete m;
    return FMI_ERR_NOMEM;
  }
  resolve_base_and_names(m);
  hipEventCreate(&m->ev0);
  hipEventCreate(&m->ev1);
  if (const char* e = getenv("FMI_TWO_STREAMS"); e && atoi(e) != 0) {
    m->two_streams = hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking) == hipSuccess &&
                     hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming) == hipSuccess;
  }
  *out = m;
  return FMI_OK;
}

extern "C" void fmi_flux_destroy(fmi_flux* m) {
  if (!m) return;
  use_device(m);
  hipDeviceSynchronize();
  if (m->ev0) hipEventDestroy(m->ev0);
  if (m->ev1) hipEventDestroy(m->ev1);
  if (m->ev_fork) hipEventDestroy(m->ev_fork);
  if (m->ev_join) hipEventDestroy(m->ev_join);
  if (m->side) hipStreamDestroy(m->side);
  if (m->sc_host) (void)hipHostFree(m->sc_host);
  delete m;  // (every device block is a DeviceBuffer member)
}

extern "C" int fmi_flux_set_tensor(fmi_flux* m, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  if (!m || !name || !data) return fail(FMI_ERR_INVALID, "flux_set_tensor: null argument");
  if (m->fp8) return fail(FMI_ERR_STATE, "flux_set_tensor: the model was quantised to 8 bits (fmi_flux_quantize_fp8 / _int8); create a new one to load other weights");
  for (const auto& ad : m->loras)
    if (ad.second.pairs.count(name)) return fail(FMI_ERR_STATE, std::string("flux_set_tensor: ") + name + " has LoRA adapters merged into it; remove the adapters first");
  m->attn_scales_valid = false;  // (fmi_flux_set_fp8_attention(m, 2) in bf16 mode: the static attention scales follow the QkNorm weights — recomputed once at the next evaluation)
  auto it = m->names.find(name);
  if (it == m->names.end()) return fail(FMI_ERR_INVALID, std::string("flux_set_tensor: unknown tensor name '") + name + "'");
  const Dest& d = it->second;
  int64_t numel = 1;
  for (int i = 0; i < rank; ++i) numel *= shape[i];
  bool ok = numel == d.numel;
  if (ok && d.cols) ok = rank == 2 && shape[0] == d.rows && shape[1] == d.cols;
  if (ok && !d.cols) ok = rank == 1 && shape[0] == d.rows;
  if (!ok) {
    std::string got = "(";
    for (int i = 0; i < rank; ++i) got += std::to_string(shape[i]) + (i + 1 < rank ? "," : "");
    got += ")";
    return fail(FMI_ERR_INVALID, std::string("flux_set_tensor: shape mismatch for ") + name + ": got " + got + ", expected (" +
                                     std::to_string(d.rows) + (d.cols ? "," + std::to_string(d.cols) : "") + ")");
  }
  if (dtype != FMI_F32 && dtype != FMI_F16 && dtype != FMI_BF16) return fail(FMI_ERR_INVALID, "flux_set_tensor: dtype must be F32/F16/BF16");
  FMI_TRY(use_device(m));
  void* dst = d.ptr;
  if (d.d && !d.bias) {  // a weight part of a (fused) matrix: its arena is allocated on first need
    FMI_TRY(ensure_arena(m, d.d->ar));
    dst = d.d->w + (size_t)d.d->parts[d.part].r0 * d.d->K;
  }
  FMI_TRY(upload_as_bf16(data, dtype, numel, (bf16_t*)dst));
  if (d.d && !d.bias) part_loaded(m, *d.d, d.part, PS_DENSE, 0, name);
  else m->missing.erase(name);
  return FMI_OK;
}

// ---- The quantised setters: one head (the shared refusals and the lookup), the setter's own storage, one tail (part_loaded).
namespace {
struct LinearSlot {  // the Linear `prefix` names: its weight's name, where it lands, and its part of the (fused) matrix
  std::string wname;
  const Dest* dst = nullptr;
  Dense* d = nullptr;
  Dense::Part* pt = nullptr;
};
// The refusals the setters share, in their order: of the handle (null_arg: one of the setter's pointers is null; q8: how it words the 8-bit modes), then own()
// — the setter's checks of its own arguments — then the lookup: a Linear of this model, no LoRA adapter merged into it, of the stated shape.
template <class Own>
int setter_head(fmi_flux* m, const std::string& fn, bool null_arg, const char* q8, const char* prefix, int out_features, int in_features, Own&& own, LinearSlot* t) {
  if (null_arg) return fail(FMI_ERR_INVALID, fn + ": null argument");
  if (m->is_cn) return fail(FMI_ERR_UNSUPPORTED, fn + ": a ControlNet runs in bf16 only (quantised ControlNets are out of scope)");
  if (m->fp8) return fail(FMI_ERR_STATE, fn + ": the model was quantised to " + q8);
  FMI_TRY(own());
  FMI_TRY(use_device(m));
  t->wname = std::string(prefix) + ".weight";
  auto it = m->names.find(t->wname);
  if (it == m->names.end() || !it->second.d) return fail(FMI_ERR_INVALID, fn + ": unknown linear '" + prefix + "'");
  for (const auto& ad : m->loras)
    if (ad.second.pairs.count(t->wname)) return fail(FMI_ERR_STATE, fn + ": " + t->wname + " has LoRA adapters merged into it; remove the adapters first");
  t->dst = &it->second, t->d = it->second.d, t->pt = &t->d->parts[it->second.part];
  if (t->dst->rows != out_features || t->dst->cols != in_features) return fail(FMI_ERR_INVALID, fn + ": shape mismatch for " + t->wname);
  return FMI_OK;
}
// a quantised Linear that is not a fused GEMM matrix (embedders, final projection): staged on the device and expanded, once, into its rows of the BASE arena
int expand_small(fmi_flux* m, const LinearSlot& t, int kind, int blocksize, const void* q, size_t qbytes, const float* sc, size_t scbytes) {
  const Dense& d = *t.d;
  FMI_TRY(with_staged_pair(q, qbytes, sc, scbytes, [&](void* dq, void* ds) {
    return dequant_to_bf16(kind, blocksize, dq, (const float*)ds, 0.f, d.K, (int64_t)t.pt->rows * d.K, d.w + (size_t)t.pt->r0 * d.K, nullptr);
  }));
  m->missing.erase(t.wname);
  return FMI_OK;
}
}  // namespace

// bitsandbytes 4-bit Linear (BnbLinear::Nf4Fp4, bitsandbytes/mod.rs:137-239): packed codes (out*in/2 bytes, high nibble
// first) + f32 absmax per `blocksize` weights.  Block linears and modulation linears keep this form (Q4 arena).
extern "C" int fmi_flux_set_linear_bnb4(fmi_flux* m, const char* prefix, const uint8_t* packed, const float* absmax, int blocksize,
                                        int quant_type, int out_features, int in_features) {
  LinearSlot t;
  FMI_TRY(setter_head(m, "set_linear_bnb4", !m || !prefix || !packed || !absmax, "fp8", prefix, out_features, in_features, [&] {
    if (quant_type != 1 && quant_type != 2) return fail(FMI_ERR_INVALID, "set_linear_bnb4: quant_type must be 1 (fp4) or 2 (nf4)");
    if (blocksize % 64 || blocksize <= 0 || in_features % blocksize)
      return fail(FMI_ERR_UNSUPPORTED, "set_linear_bnb4: blocksize must be a multiple of 64 dividing in_features");
    return (int)FMI_OK;
  }, &t));
  Dense* d = t.d;
  const size_t n = (size_t)out_features * in_features;
  if (d->ar == AR_BASE) {
    if (n >= (1ull << 31)) return fail(FMI_ERR_UNSUPPORTED, "set_linear_bnb4: linear too large");
    return expand_small(m, t, quant_type, blocksize, packed, n / 2, absmax, n / blocksize * 4);
  }
  if (d->own_wq) return fail(FMI_ERR_UNSUPPORTED, "set_linear_bnb4: this fused projection already holds int8 parts");
  FMI_TRY(ensure_arena(m, AR_Q4));
  FMI_HIP_TRY(hipMemcpy(d->wq + (size_t)t.pt->r0 * d->K / 2, packed, n / 2, hipMemcpyDefault));
  FMI_HIP_TRY(hipMemcpy(d->absmax + (size_t)t.pt->r0 * d->K / blocksize, absmax, n / blocksize * 4, hipMemcpyDefault));
  part_loaded(m, *d, t.dst->part, quant_type, blocksize, t.wname);
  return FMI_OK;
}

// LLM.int8 linears (BnbLinear::Int8, bitsandbytes/mod.rs:104-134): weight i8 (out,in) + SCB f32 (out).
// forward = dequantize_8bit (w * SCB[row] / 127, dequant.cu:205-214) then matmul (mod.rs:293-300):
// fused matrices keep the int8 weight and are expanded right before their GEMM (or once, with the dense cache).
extern "C" int fmi_flux_set_linear_int8(fmi_flux* m, const char* prefix, const int8_t* weight, const float* scb, int out_features, int in_features) {
  LinearSlot t;
  FMI_TRY(setter_head(m, "set_linear_int8", !m || !prefix || !weight || !scb, "fp8", prefix, out_features, in_features, [] { return (int)FMI_OK; }, &t));
  Dense* d = t.d;
  const size_t n = (size_t)out_features * in_features;
  if (d->ar == AR_BASE) return expand_small(m, t, PS_INT8, 0, weight, n, scb, (size_t)out_features * 4);
  for (auto& pt : d->parts)
    if (pt.state == PS_FP4 || pt.state == PS_NF4) return fail(FMI_ERR_UNSUPPORTED, "set_linear_int8: this fused projection already holds 4-bit parts");
  if (!d->own_wq) {  // the matrix changes only once both blocks exist and are zeroed
    DeviceBuffer wq, sc;
    FMI_HIP_TRY(wq.alloc((size_t)d->N * d->K));
    FMI_HIP_TRY(sc.alloc((size_t)d->N * 4));
    FMI_HIP_TRY(hipMemset(wq.ptr, 0, wq.bytes()));
    FMI_HIP_TRY(hipMemset(sc.ptr, 0, sc.bytes()));
    d->own_wq = std::move(wq), d->own_absmax = std::move(sc);
    d->wq = d->own_wq.as<uint8_t>(), d->absmax = d->own_absmax.as<float>();
  }
  FMI_HIP_TRY(hipMemcpy(d->wq + (size_t)t.pt->r0 * d->K, weight, n, hipMemcpyDefault));
  FMI_HIP_TRY(hipMemcpy(d->absmax + t.pt->r0, scb, (size_t)out_features * 4, hipMemcpyDefault));
  part_loaded(m, *d, t.dst->part, PS_INT8, 0, t.wname);
  return FMI_OK;
}

namespace {
// The two kinds that have no fused dequant-GEMM — ggml blocks, 8-bit float codes with one scale — behind the head: `bytes` of `data` go to the device.
// Embedders, the final layer and the modulation linears are expanded into their bf16 rows here (the fused modulation matrix never goes through densify()'s
// scratch, and as dense rows it keeps the bf16 model's GEMV); the parts of a fused block matrix keep their blocks / codes (Dense::gq) and their scale
// (Dense::gscale), and finalize() / densify() decide.
int set_linear_codes(fmi_flux* m, const LinearSlot& t, int kind, const void* data, size_t bytes, float scale) {
  Dense* d = t.d;
  DeviceBuffer buf;
  FMI_HIP_TRY(buf.alloc(bytes));
  FMI_HIP_TRY(hipMemcpy(buf.ptr, data, bytes, hipMemcpyDefault));
  if (d->ar == AR_BASE || d->ar == AR_MOD) {
    FMI_TRY(ensure_arena(m, d->ar));
    FMI_TRY(dequant_to_bf16(kind, 0, buf.ptr, nullptr, scale, d->K, (int64_t)t.pt->rows * d->K, d->w + (size_t)t.pt->r0 * d->K, nullptr));
    FMI_HIP_TRY(hipDeviceSynchronize());
    m->attn_scales_valid = false;
    if (d->ar == AR_MOD) part_loaded(m, *d, t.dst->part, PS_DENSE, 0, t.wname);
    else m->missing.erase(t.wname);
    return FMI_OK;
  }
  if (d->gq.size() < d->parts.size()) d->gq.resize(d->parts.size());
  if (d->gscale.size() < d->parts.size()) d->gscale.resize(d->parts.size(), 1.0f);
  FMI_HIP_TRY(hipDeviceSynchronize());  // (a replaced part's blocks / codes may still be read by an expansion in flight)
  d->gq[t.dst->part] = std::move(buf);
  d->gscale[t.dst->part] = scale;
  part_loaded(m, *d, t.dst->part, kind, 0, t.wname);
  return FMI_OK;
}
}  // namespace

// A Linear as ggml blocks (llama.cpp's .gguf files; gguf_dequant.hip): row-major, in_features / block_elems blocks per row.
extern "C" int fmi_flux_set_linear_gguf(fmi_flux* m, const char* prefix, int ggml_type, const void* data, int out_features, int in_features) {
  LinearSlot t;
  int be = 0, bb = 0;
  FMI_TRY(setter_head(m, "set_linear_gguf", !m || !prefix || !data, "8 bits", prefix, out_features, in_features, [&] {
    FMI_TRY(fmi_gguf_block_info(ggml_type, &be, &bb));
    if (in_features <= 0 || out_features <= 0 || in_features % be)
      return fail(FMI_ERR_INVALID, "set_linear_gguf: in_features must be a positive multiple of the block's " + std::to_string(be) + " elements");
    return (int)FMI_OK;
  }, &t));
  return set_linear_codes(m, t, PS_GGUF0 + ggml_type, data, (size_t)((int64_t)out_features * in_features / be) * bb, 1.0f);
}

// A Linear as OCP e4m3fn / e5m2 codes with one scale (single-file fp8 checkpoints; f8_dequant.hip): row-major, one code per weight.
extern "C" int fmi_flux_set_linear_f8(fmi_flux* m, const char* prefix, int format, const void* codes, float scale, int out_features, int in_features) {
  LinearSlot t;
  FMI_TRY(setter_head(m, "set_linear_f8", !m || !prefix || !codes, "8 bits", prefix, out_features, in_features, [&] {
    if (format != 1 && format != 2) return fail(FMI_ERR_INVALID, "set_linear_f8: format must be 1 (OCP e4m3fn) or 2 (OCP e5m2), got " + std::to_string(format));
    if (!std::isfinite(scale) || !(scale > 0.f)) return fail(FMI_ERR_INVALID, "set_linear_f8: scale must be finite and > 0");
    if (in_features <= 0 || out_features <= 0) return fail(FMI_ERR_INVALID, "set_linear_f8: in_features and out_features must be positive");
    return (int)FMI_OK;
  }, &t));
  return set_linear_codes(m, t, format == 1 ? PS_F8_E4M3 : PS_F8_E5M2, codes, (size_t)out_features * in_features, scale);
}

extern "C" int fmi_flux_missing_count(const fmi_flux* m) { return m ? m->missing.count() : 0; }
extern "C" const char* fmi_flux_missing_name(const fmi_flux* m, int i) { return m ? m->missing.name(i) : nullptr; }
extern "C" size_t fmi_flux_size_in_bytes(const fmi_flux* m) {
  if (!m) return 0;
  size_t b = m->ws.base.bytes() + m->fp8_arena.bytes() + m->wscratch[0].bytes() + m->wscratch[1].bytes() + m->mod_steps_rows * ((size_t)m->n_mod * 4 + (size_t)m->D * 6);
  b += m->cn_samples.bytes() + m->cn_cx.bytes() + m->cn_cond_bf.bytes();  // (a ControlNet's per-shape buffers; 0 on any other handle)
  b += m->solver_buf[0].bytes() + m->solver_buf[1].bytes();               // (0 until the first Heun / 2M loop)
  for (int a = 0; a < AR_COUNT; ++a)
    if (m->arena[a].base) b += m->arena[a].bytes;
  for (const Dense* d : m->fused) b += resident_code_bytes(*d);
  for (const auto& ad : m->loras)
    for (const auto& pr : ad.second.pairs) {
      b += pr.second.bytes();  // (f32 factors, expanded LoKr factors and DoRA's per-row vectors; 0 once the 8-bit modes have frozen the adapters)
    }
  for (const auto& bk : m->lora_backup) b += (size_t)m->names.at(bk.first).numel * 2;
  return b + m->lora_scratch.bytes() + m->lora_descs.bytes();
}

// ---- weight state as a handful of flat device buffers: the unit of the multi-GPU weight broadcast.
// Rank 0 loads a checkpoint as usual; fmi_flux_state_export describes which arenas exist and how every fused matrix is
// stored; the other ranks fmi_flux_state_adopt that description (allocating the same arenas, marking every tensor as
// present) and then receive the bytes of buffers 0 .. fmi_flux_state_buffer_count()-1 — four RCCL broadcasts instead
// of one per tensor.  LLM.int8 matrices own separate allocations and are not covered (FMI_ERR_UNSUPPORTED: load per rank).
extern "C" int fmi_flux_state_buffer_count(void) { return AR_COUNT; }
extern "C" int fmi_flux_state_export(fmi_flux* m, uint8_t* blob_host, size_t cap, size_t* len) {
  if (!m || !len) return fail(FMI_ERR_INVALID, "state_export: null argument");
  FMI_TRY(use_device(m));
  FMI_TRY(check_ready(m));
  if (m->fp8) return fail(FMI_ERR_UNSUPPORTED, "state_export: export before fmi_flux_quantize_fp8 (every rank quantises its own copy)");
  const size_t need = 8 + AR_COUNT + 5 * m->fused.size();
  *len = need;
  if (!blob_host) return FMI_OK;
  if (cap < need) return fail(FMI_ERR_INVALID, "state_export: buffer too small");
  uint8_t* o = blob_host;
  memcpy(o, "FMIS", 4);
  const uint32_t nf = (uint32_t)m->fused.size();
  memcpy(o + 4, &nf, 4);
  o += 8;
  for (int a = 0; a < AR_COUNT; ++a) *o++ = m->arena[a].base ? 1 : 0;
  for (const Dense* d : m->fused) {
    if (d->own_wq) return fail(FMI_ERR_UNSUPPORTED, "state_export: LLM.int8 matrices are not part of the flat weight state");
    if (is_gguf(d->q_type)) return fail(FMI_ERR_UNSUPPORTED, "state_export: matrices resident as ggml blocks are not part of the flat weight state");
    if (is_f8(d->q_type)) return fail(FMI_ERR_UNSUPPORTED, "state_export: matrices resident as 8-bit float codes are not part of the flat weight state");
    *o++ = (uint8_t)d->q_type;
    const uint32_t bs = (uint32_t)d->q_blocksize;
    memcpy(o, &bs, 4);
    o += 4;
  }
  return FMI_OK;
}
extern "C" int fmi_flux_state_adopt(fmi_flux* m, const uint8_t* blob_host, size_t len) {
  if (!m || !blob_host) return fail(FMI_ERR_INVALID, "state_adopt: null argument");
  FMI_TRY(use_device(m));
  uint32_t nf = 0;
  if (!m->loras.empty()) return fail(FMI_ERR_STATE, "state_adopt: the model holds LoRA adapters; remove the adapters first");
  if (len < 8 || memcmp(blob_host, "FMIS", 4)) return fail(FMI_ERR_INVALID, "state_adopt: bad blob");
  memcpy(&nf, blob_host + 4, 4);
  if (nf != m->fused.size() || len != 8 + AR_COUNT + 5 * (size_t)nf) return fail(FMI_ERR_INVALID, "state_adopt: the blob describes a different model configuration");
  const uint8_t* o = blob_host + 8;
  for (int a = 0; a < AR_COUNT; ++a)
    if (*o++) FMI_TRY(ensure_arena(m, a));
  for (Dense* d : m->fused) {
    const int qt = *o++;
    uint32_t bs = 0;
    memcpy(&bs, o, 4);
    o += 4;
    if (qt == PS_INT8 || d->own_wq) return fail(FMI_ERR_UNSUPPORTED, "state_adopt: LLM.int8 matrices are not part of the flat weight state");
    if (is_codes(qt)) return fail(FMI_ERR_UNSUPPORTED, "state_adopt: matrices resident as ggml blocks or 8-bit float codes are not part of the flat weight state");
    d->gq.clear(), d->gscale.clear();
    d->q_type = qt, d->q_blocksize = (int)bs;
    for (auto& pt : d->parts) pt.state = qt ? (uint8_t)qt : (uint8_t)PS_DENSE, pt.blocksize = (int)bs;
    if (qt ? !m->arena[AR_Q4].base : !m->arena[d->ar].base) return fail(FMI_ERR_INVALID, "state_adopt: blob is inconsistent (matrix stored in an arena that is not present)");
  }
  m->missing.names.clear();
  m->dense_ready.clear();
  m->attn_scales_valid = false;  // the weights arrive after this call (broadcast into the arenas)
  m->finalized = true;
  return FMI_OK;
}
extern "C" int fmi_flux_state_buffer(fmi_flux* m, int index, void** ptr, size_t* bytes) {
  if (!m || !ptr || !bytes || index < 0 || index >= AR_COUNT) return fail(FMI_ERR_INVALID, "state_buffer: bad argument");
  *ptr = m->arena[index].base.ptr;
  *bytes = m->arena[index].base ? m->arena[index].bytes : 0;
  return FMI_OK;
}

// One evaluation of every forward entry: over cat([img, ctx], 1) with a context, over cat([img, cond], 2) with a control.
// The plan of the ControlNet's own evaluations: the main call's negative prompt and batch, nothing else of its options.
static EvalPlan cn_plan(const EvalPlan& p) { return EvalPlan{fmi_flux_denoise_options{nullptr, nullptr, p.o.cfg}, 0, p.Bs}; }
// Once per call, on the ControlNet: its workspace and sample buffers for the call's batch, its input casts and RoPE table (prepare_static, as on the main model —
// the table is built once per call), and controlnet_x_embedder(cond).
static int cn_prepare(fmi_flux* net, const fmi_flux_inputs* in, const EvalPlan& p, hipStream_t s) {
  FMI_TRY(ensure_workspace(net, in->B, in->S, in->T));
  FMI_TRY(cn_ensure(net, in->B, in->S, s));
  FMI_TRY(prepare_static(net, in, cn_plan(p), s));
  return cn_embed_cond(net, p.cn->cond, p.cn->cond_dtype, in->B, p.Bs, in->S, s);
}

static int forward_eval(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_context* ctx, const fmi_flux_control* ctl, const fmi_flux_controlnet* cn, const fmi_flux_ip* ip,
                        float* pred_out, void* stream) {
  const fmi_flux_denoise_options o{ctx, ctl};  // (every other field null)
  EvalPlan p;
  fmi_flux_controlnet one;  // a single evaluation ignores step_scales
  if (cn) one = *cn, one.step_scales = nullptr, cn = &one;
  fmi_flux_ip one_ip;
  if (ip) one_ip = *ip, one_ip.step_scales = nullptr, ip = &one_ip;
  FMI_TRY(validate(m, in, o, cn, ip, 1, in && in->img && in->timesteps && pred_out ? nullptr : "flux_forward: null img/timesteps/pred_out", &p));
  hipStream_t s = (hipStream_t)stream;
  FMI_TRY(ensure_workspace(m, in->B, in->S + p.R, in->T));
  FMI_TRY(prepare_static(m, in, p, s));
  FMI_TRY(launch_cast_to_f32(in->img, in->img_dtype, m->ws.img_f32, (int64_t)in->B * in->S * m->cfg.in_channels, s));
  IpInject ipj{ip ? ip->adapter : nullptr, ip ? ip->scale : 0.f};
  const IpInject* ipp = ip && ip->scale != 0.f ? &ipj : nullptr;  // (scale 0: the plain evaluation, launch for launch)
  if (ipp) FMI_TRY(ip_prepare(ip->adapter, ip->embeds, nullptr, ip->embeds_dtype, in->B, false, s));
  if (cn && cn->scale != 0.f) {  // (scale 0: the plain evaluation, launch for launch)
    fmi_flux* net = cn->net;
    FMI_TRY(cn_prepare(net, in, p, s));
    FMI_TRY(forward_core(net, in, cn_plan(p), m->ws.img_f32, in->timesteps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s));
    const CnInject inj{net, cn->scale};
    return forward_core(m, in, p, m->ws.img_f32, in->timesteps, pred_out, /*mod_pre*/ nullptr, /*txt_pre*/ nullptr, /*sc*/ nullptr, &inj, ipp, s);
  }
  return forward_core(m, in, p, m->ws.img_f32, in->timesteps, pred_out, /*mod_pre*/ nullptr, /*txt_pre*/ nullptr, /*sc*/ nullptr, /*inj*/ nullptr, ipp, s);
}
// One evaluation over cat([img, ctx], 1); pred_out is the img rows' (DESIGN.md 4.9).  No context: fmi_flux_forward.
extern "C" int fmi_flux_forward_context(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_context* ctx, float* pred_out, void* stream) {
  return forward_eval(m, in, ctx, nullptr, nullptr, nullptr, pred_out, stream);
}
// One evaluation over cat([img, cond], 2) of a channel-conditioned model; pred_out is (B,S,in_channels).  A plain model with ctl NULL: fmi_flux_forward.
extern "C" int fmi_flux_forward_control(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_control* ctl, float* pred_out, void* stream) {
  return forward_eval(m, in, nullptr, ctl, nullptr, nullptr, pred_out, stream);
}
// One evaluation with a ControlNet's residuals injected after every block.  cn NULL: fmi_flux_forward.
extern "C" int fmi_flux_forward_controlnet(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_controlnet* cn, float* pred_out, void* stream) {
  return forward_eval(m, in, nullptr, nullptr, cn, nullptr, pred_out, stream);
}
// One evaluation with an IP-Adapter's image-prompt attention in every double block, and a ControlNet's residuals if cn is given.  ip NULL:
// fmi_flux_forward_controlnet.  A model with conditioning channels takes its control through ctl (NULL on any other model).
extern "C" int fmi_flux_forward_ip(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_control* ctl, const fmi_flux_controlnet* cn, const fmi_flux_ip* ip, float* pred_out,
                                   void* stream) {
  return forward_eval(m, in, nullptr, ctl, cn, ip, pred_out, stream);
}
extern "C" int fmi_flux_forward(fmi_flux* m, const fmi_flux_inputs* in, float* pred_out, void* stream) {
  return fmi_flux_forward_context(m, in, nullptr, pred_out, stream);
}

// (b) of the loop: the step cache's buffers for B streams of `rows` image rows, regrown when a larger shape comes.
static int step_cache_ensure(fmi_flux* m, int B, int rows, hipStream_t s) {
  const size_t per = (size_t)rows * m->D, elems = (size_t)B * per, part = (size_t)B * step_cache_groups((int64_t)per) * 2;
  if (m->sc_elems < elems || m->sc_part_floats < part) {
    FMI_HIP_TRY(hipStreamSynchronize(s));
    m->sc_x0.reset(), m->sc_r[0].reset(), m->sc_r[1].reset(), m->sc_delta.reset(), m->sc_part.reset(), m->sc_elems = 0, m->sc_part_floats = 0;
    for (DeviceBuffer* b : {&m->sc_x0, &m->sc_r[0], &m->sc_r[1], &m->sc_delta})
      if (b->alloc(elems * 4) != hipSuccess) return fail(FMI_ERR_NOMEM, "flux_denoise: hipMalloc of a step-cache buffer (" + std::to_string(elems * 4) + " bytes) failed");
    if (m->sc_part.alloc(part * 4) != hipSuccess) return fail(FMI_ERR_NOMEM, "flux_denoise: hipMalloc of the step cache's partial sums failed");
    m->sc_elems = elems, m->sc_part_floats = part;
  }
  if (!m->sc_sums) FMI_HIP_TRY(m->sc_sums.alloc(2 * 8 * sizeof(double)));  // (B <= 8, check_inputs)
  if (!m->sc_host) FMI_HIP_TRY(hipHostMalloc((void**)&m->sc_host, 2 * 8 * sizeof(double), hipHostMallocDefault));
  return FMI_OK;
}

// The solver's own refusals, after validate()'s and like them before anything is launched or allocated.  Euler refuses nothing: the loop as it was.
static int check_solver(const fmi_flux* m, const fmi_flux_denoise_options& o, const EvalPlan& p, int solver, const double* timesteps_host, int n_steps) {
  if (solver == FMI_SOLVER_EULER) return FMI_OK;
  if (solver != FMI_SOLVER_HEUN && solver != FMI_SOLVER_DPMPP_2M) return fail(FMI_ERR_INVALID, "flux_denoise: solver kind must be FMI_SOLVER_EULER, _HEUN or _DPMPP_2M");
  FMI_TRY(check_solver_schedule(timesteps_host, n_steps, "flux_denoise"));
  if (m->sp_world > 1 && m->sp_a2a) return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: the heun and dpmpp_2m solvers are not supported under sequence parallelism");
  if (solver == FMI_SOLVER_HEUN && o.cache)
    return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: the heun solver is not combined with the step cache (its two evaluations per step are at different times)");
  if (solver == FMI_SOLVER_HEUN && ((int64_t)n_steps + 1) * (o.cfg ? 2 : 1) * p.Bs > 4096)
    return fail(FMI_ERR_UNSUPPORTED, "flux_denoise: (n_steps + 1) * B > 4096 under the heun solver (ws.tv holds 4096 rows; true CFG counts 2 B)");
  return FMI_OK;
}
// The solver's buffers for a state of `elems` floats: two for Heun, one for 2M, regrown when a larger state comes.
static int solver_ensure(fmi_flux* m, int solver, size_t elems, hipStream_t s) {
  for (int k = 0; k < (solver == FMI_SOLVER_HEUN ? 2 : 1); ++k) {
    DeviceBuffer& b = m->solver_buf[k];
    if (b.bytes() >= elems * 4 && b) continue;
    if (b) FMI_HIP_TRY(hipStreamSynchronize(s));
    if (b.alloc(std::max<size_t>(elems, 1) * 4) != hipSuccess)
      return fail(FMI_ERR_NOMEM, "flux_denoise: hipMalloc of a solver buffer (" + std::to_string(elems * 4) + " bytes) failed");
  }
  return FMI_OK;
}

// (c) of the loop, what the steps share, once per call: every step's timestep vector in ws.tv, every step's modulation vectors (*mod_steps; null where each step
// computes its own) and txt_in(txt) (*txt_pre; likewise).  n_steps counts the times that get a row: the loop's steps, and under Heun one more,
// the last step's target time, so that the second evaluation of step i reads row i + 1.
static int hoist_steps(fmi_flux* m, const fmi_flux_inputs* in, const double* timesteps_host, int n_steps, hipStream_t s, const float** mod_steps, const float** txt_pre) {
  const int B = in->B;
  // t_vec = full(1f32, B) * t_curr  (sampling.rs:35,42): all steps' vectors uploaded once
  std::vector<float> tv((size_t)(n_steps > 0 ? n_steps : 1) * B);
  for (int i = 0; i < n_steps; ++i)
    for (int b = 0; b < B; ++b) tv[(size_t)i * B + b] = 1.0f * (float)timesteps_host[i];
  FMI_HIP_TRY(hipMemcpyAsync(m->ws.tv, tv.data(), tv.size() * 4, hipMemcpyHostToDevice, s));
  FMI_HIP_TRY(hipStreamSynchronize(s));  // tv is pageable host memory: finish the copy before it dies
  // The modulation vectors depend on (t, guidance, y) only, never on the latent: all steps' vectors are
  // computed up front, GEMV_MAXROWS rows per pass over the 6.5 GB modulation matrix (13 passes for 50
  // steps instead of 50: the per-step GEMV was 1.2 ms of pure HBM streaming per denoise step).
  *mod_steps = nullptr;
  const size_t R = (size_t)n_steps * B, nmod = (size_t)m->n_mod;
  if (n_steps > 1 && R * nmod * 4 <= (2ull << 30)) {
    if (m->mod_steps_rows < R) {
      FMI_HIP_TRY(hipStreamSynchronize(s));
      m->mod_steps.reset(), m->vec_steps.reset(), m->vec_steps_bf.reset(), m->temb_steps.reset(), m->h1_steps.reset(), m->mod_steps_rows = 0;
      FMI_HIP_TRY(m->mod_steps.alloc(R * nmod * 4));
      FMI_HIP_TRY(m->vec_steps.alloc(R * (size_t)m->D * 4));
      FMI_HIP_TRY(m->vec_steps_bf.alloc(R * (size_t)m->D * 2));
      FMI_HIP_TRY(m->temb_steps.alloc(R * (size_t)256 * 4));
      FMI_HIP_TRY(m->h1_steps.alloc(std::max<size_t>(R, 2 * (size_t)B) * (size_t)m->D * 4));
      m->mod_steps_rows = R;
    }
    {
      PhaseTimer pt(m, s, PH_EMBED);
      FMI_TRY(compute_vec_steps(m, in, m->ws.tv, n_steps, m->vec_steps.as<float>(), m->temb_steps.as<float>(), m->h1_steps.as<float>(), s));
    }
    {
      PhaseTimer pt(m, s, PH_MOD);
      constexpr int GEMV_MAXROWS = 4;  // rows * D * 4 B of x staged in LDS per block (<= 64 KiB)
      if (m->mod_all.q_type || (m->mod_gemm && (R > GEMV_MAXROWS || m->mod_gemm == 2) && m->D % 64 == 0 && nmod % 8 == 0 && R * nmod < (1ull << 31))) {
        // all rows in ONE pass over the matrix on the MFMA GEMM (silu(vec) rounded to bf16 like every other
        // GEMM input): the matrix is read once per image instead of once per 4 steps
        FMI_TRY(launch_silu_to_bf16(m->vec_steps.as<float>(), m->vec_steps_bf.as<bf16_t>(), (int64_t)R * m->D, s));
        GemmProblem p = make_problem(m->mod_all, m->vec_steps_bf.as<bf16_t>(), m->D, (int)R, m->mod_steps.as<float>(), (int)nmod, EPI_STORE_F32);
        FMI_TRY(gemm1(m, p, m->mod_all, s));
      } else {
        for (size_t r0 = 0; r0 < R; r0 += GEMV_MAXROWS)
          FMI_TRY(launch_gemv(m->vec_steps.as<float>() + r0 * m->D, m->mod_all.w, m->mod_all.b, m->mod_steps.as<float>() + r0 * nmod, (int)std::min<size_t>(GEMV_MAXROWS, R - r0),
                              (int)nmod, m->D, 1, 0, s));
      }
    }
    *mod_steps = m->mod_steps.as<float>();
  }
  *txt_pre = nullptr;
  if (n_steps > 1) {  // txt = txt_in(txt) (model.rs:812) depends on the prompt only: once per image
    PhaseTimer pt(m, s, PH_EMBED);
    GemmProblem p = make_problem(m->txt_in, m->ws.txt_bf, m->cfg.joint_attention_dim, B * in->T, m->ws.x_txt0, m->D, EPI_STORE_F32);
    FMI_TRY(gemm1(m, p, m->txt_in, s));
    *txt_pre = m->ws.x_txt0;
  }
  return FMI_OK;
}

// (d) of the loop: the steps.  One evaluation each, then the update of the state — one of three, and all that knows about the negative prompt's scale or the blend.
// The ControlNet of one loop: what its steps share (hoisted like the main model's, null where each step computes its own) and each step's scale.
struct CnRun {
  fmi_flux* net;
  const float *mod_steps, *txt_pre;
  std::vector<float> c;  // scale * step_scales[i]; a step whose c is 0 launches neither the ControlNet nor an injection: it is the plain step
};
// The IP-Adapter of one loop: the adapter (its K / V projected once, before the first step) and each step's scale; a step whose c is 0 is the plain step.
struct IpRun {
  const fmi_ip_adapter* a;
  std::vector<float> c;
};
// solver: FMI_SOLVER_* (DESIGN.md 4.21).  Euler is the loop as it always was; Heun evaluates twice per step — the second time on its predicted state, at the
// hoisted row of the step's target time — and 2M once, each followed by its own one-pass update, which knows the scale and the blend exactly as Euler's does.
static int run_steps(fmi_flux* m, const fmi_flux_inputs* in, const EvalPlan& p, float* img_inout, const double* timesteps_host, int n_steps, const float* mod_steps,
                     const float* txt_pre, StepCacheRun* sc, const CnRun* cn, const IpRun* ip, int solver, hipStream_t s) {
  const fmi_flux_denoise_options& o = p.o;
  const size_t B = in->B, nmod = m->n_mod;
  const int64_t n = (int64_t)p.Bs * in->S * m->cfg.in_channels;
  // One evaluation into ws.pred_tmp: of the state x at the time of hoisted row `row`, at step i's ControlNet and adapter scales.
  const auto eval = [&](const float* x, int row, int i) -> int {
    CnInject inj{};
    const IpInject ipj{ip && ip->c[i] != 0.f ? ip->a : nullptr, ip ? ip->c[i] : 0.f};
    if (cn && cn->c[i] != 0.f) {  // the ControlNet on the step's state, then the main model with its samples
      fmi_flux* net = cn->net;
      FMI_TRY(forward_core(net, in, cn_plan(p), x, net->ws.tv + row * B, nullptr, cn->mod_steps ? cn->mod_steps + row * B * (size_t)net->n_mod : nullptr, cn->txt_pre,
                           nullptr, nullptr, nullptr, s));
      inj = CnInject{net, cn->c[i]};
    }
    return forward_core(m, in, p, x, m->ws.tv + row * B, m->ws.pred_tmp, mod_steps ? mod_steps + row * B * nmod : nullptr, txt_pre, sc, inj.net ? &inj : nullptr,
                        ipj.a ? &ipj : nullptr, s);
  };
  // pred_tmp is (2 Bs, S, C) under true CFG: the prompt's predictions, then the negative's; the blend's arguments are null without a mask
  const float *pos = m->ws.pred_tmp, *neg = o.cfg ? m->ws.pred_tmp + n : nullptr;
  const float scale = o.cfg ? o.cfg->scale : 0.f;
  for (int i = 0; i < n_steps; ++i) {
    FMI_TRY(eval(img_inout, i, i));
    // img = img + pred * (t_prev - t_curr)  (sampling.rs:43), scalar rounded to f32 like candle's affine
    const float dt = (float)(timesteps_host[i + 1] - timesteps_host[i]), t_next = (float)timesteps_host[i + 1];
    if (solver == FMI_SOLVER_DPMPP_2M) {  // the history is buffer 0: written by every step, read from the first step whose w is not 0
      float a, c, w;
      dpmpp_2m_coefficients(timesteps_host, i, &a, &c, &w);
      FMI_TRY(launch_dpmpp_2m(img_inout, pos, neg, scale, (float)timesteps_host[i], a, c, w, n, m->solver_buf[0].as<float>(), s, o.x0, o.noise, o.mask, t_next));
    } else if (solver == FMI_SOLVER_HEUN && timesteps_host[i + 1] != 0.0) {  // (into t = 0 the step is Euler's, below: the model is not evaluated at 0)
      float *xt = m->solver_buf[0].as<float>(), *g1 = m->solver_buf[1].as<float>();
      FMI_TRY(launch_heun_predict(img_inout, pos, neg, scale, dt, n, xt, g1, s, o.x0, o.noise, o.mask, t_next));
      FMI_TRY(eval(xt, i + 1, i));
      FMI_TRY(launch_heun_correct(img_inout, g1, pos, neg, scale, dt, n, s, o.x0, o.noise, o.mask, t_next));
    } else {
      FMI_TRY(launch_euler_step(img_inout, pos, neg, scale, dt, n, s, o.x0, o.noise, o.mask, t_next));
    }
  }
  return FMI_OK;
}

// The denoise loop of every entry (include/flux_mi355x.h: fmi_flux_denoise_with).  An option that is null changes no launch and no allocation, and each is
// known to few places: the blend to the update alone; the context and the control to the input assembly (prepare_static writes the context's rows and the conditioning's columns
// of the img_in operand once, forward_core the state's every step); the negative prompt to the input assembly and the update — `in` below is then the loop's own batch of
// 2 * Bs samples, the prompt's rows, then the negative's —; the step cache to forward_core after double block 0.
static int denoise_loop(fmi_flux* m, const fmi_flux_inputs* in_caller, const fmi_flux_denoise_options& o, const fmi_flux_controlnet* cn, const fmi_flux_ip* ip,
                        float* img_inout, const double* timesteps_host, int n_steps, void* stream, const fmi_flux_solver* solver_arg = nullptr) {
  EvalPlan p;
  FMI_TRY(validate(m, in_caller, o, cn, ip, n_steps, img_inout && timesteps_host && n_steps >= 0 ? nullptr : "flux_denoise: null img/timesteps or negative n_steps", &p));
  const int solver = solver_arg ? solver_arg->kind : FMI_SOLVER_EULER;
  FMI_TRY(check_solver(m, o, p, solver, timesteps_host, n_steps));
  hipStream_t s = (hipStream_t)stream;
  fmi_flux_inputs in = *in_caller;
  if (o.cfg) in.B = 2 * p.Bs;
  StepCacheRun sc{o.cache};
  if (o.cache) FMI_TRY(step_cache_ensure(m, in.B, in.S + p.R, s));
  FMI_TRY(ensure_workspace(m, in.B, in.S + p.R, in.T));
  if (solver != FMI_SOLVER_EULER) FMI_TRY(solver_ensure(m, solver, (size_t)p.Bs * in.S * m->cfg.in_channels, s));
  const int n_rows = solver == FMI_SOLVER_HEUN ? n_steps + 1 : n_steps;  // the times that get a hoisted row: Heun's last second evaluation runs at ts[n_steps]
  if (o.cfg && in.guidance) {  // the same guidance in both halves
    if (!m->cfg_gd) FMI_HIP_TRY(m->cfg_gd.alloc(8 * sizeof(float)));  // (2 Bs <= 8; a call without a negative never allocates it)
    FMI_HIP_TRY(hipMemcpyAsync(m->cfg_gd.as<float>(), in_caller->guidance, (size_t)p.Bs * 4, hipMemcpyDeviceToDevice, s));
    FMI_HIP_TRY(hipMemcpyAsync(m->cfg_gd.as<float>() + p.Bs, in_caller->guidance, (size_t)p.Bs * 4, hipMemcpyDeviceToDevice, s));
    in.guidance = m->cfg_gd.as<float>();
  }
  FMI_TRY(prepare_static(m, &in, p, s));  // txt cast, y cast, the RoPE table and the context's rows of the img_in operand are loop invariant
  const float *mod_steps, *txt_pre;
  FMI_TRY(hoist_steps(m, &in, timesteps_host, n_rows, s, &mod_steps, &txt_pre));
  CnRun cr{cn ? cn->net : nullptr, nullptr, nullptr, {}};
  bool cn_active = false;  // a ControlNet whose every step has scale 0 prepares nothing: the call is the plain loop, launch for launch
  for (int i = 0; cn && i < n_steps; ++i) {
    cr.c.push_back(cn->step_scales ? cn->scale * cn->step_scales[i] : cn->scale);
    cn_active = cn_active || cr.c.back() != 0.f;
  }
  if (cn_active) {  // the ControlNet's once-per-image work, hoisted like the main model's: controlnet_x_embedder(cond), every step's modulation vectors, txt_in
    FMI_TRY(cn_prepare(cr.net, &in, p, s));
    FMI_TRY(hoist_steps(cr.net, &in, timesteps_host, n_rows, s, &cr.mod_steps, &cr.txt_pre));
  }
  IpRun ir{ip ? ip->adapter : nullptr, {}};
  bool ip_active = false;  // likewise: an adapter whose every step has scale 0 projects nothing, and every step keeps the fused q|k|v relayout
  for (int i = 0; ip && i < n_steps; ++i) {
    ir.c.push_back(ip->step_scales ? ip->scale * ip->step_scales[i] : ip->scale);
    ip_active = ip_active || ir.c.back() != 0.f;
  }
  // the adapter's once-per-call work: tok and every block's K / V, for the prompt's embeds and — under true CFG — the negative's (zeros without neg_embeds)
  if (ip_active) FMI_TRY(ip_prepare(ip->adapter, ip->embeds, ip->neg_embeds, ip->embeds_dtype, p.Bs, o.cfg != nullptr, s));
  return run_steps(m, &in, p, img_inout, timesteps_host, n_steps, mod_steps, txt_pre, o.cache ? &sc : nullptr, cn_active ? &cr : nullptr, ip_active ? &ir : nullptr, solver,
                   s);
}

extern "C" int fmi_flux_denoise_with(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_denoise_options* opts, float* img_inout, const double* timesteps_host, int n_steps, void* stream) {
  return denoise_loop(m, in, opts ? *opts : fmi_flux_denoise_options{}, nullptr, nullptr, img_inout, timesteps_host, n_steps, stream);
}
// The same loop with a ControlNet; cn NULL IS fmi_flux_denoise_with.
extern "C" int fmi_flux_denoise_controlnet(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_denoise_options* opts, const fmi_flux_controlnet* cn, float* img_inout,
                                           const double* timesteps_host, int n_steps, void* stream) {
  return denoise_loop(m, in, opts ? *opts : fmi_flux_denoise_options{}, cn, nullptr, img_inout, timesteps_host, n_steps, stream);
}
// The same loop with an IP-Adapter, and a ControlNet if cn is given; ip NULL IS fmi_flux_denoise_controlnet.
extern "C" int fmi_flux_denoise_ip(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_denoise_options* opts, const fmi_flux_controlnet* cn, const fmi_flux_ip* ip,
                                   float* img_inout, const double* timesteps_host, int n_steps, void* stream) {
  return denoise_loop(m, in, opts ? *opts : fmi_flux_denoise_options{}, cn, ip, img_inout, timesteps_host, n_steps, stream);
}
// The same loop with a second-order solver; solver NULL (or FMI_SOLVER_EULER) IS fmi_flux_denoise_ip.
extern "C" int fmi_flux_denoise_solver(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_denoise_options* opts, const fmi_flux_controlnet* cn, const fmi_flux_ip* ip,
                                       const fmi_flux_solver* solver, float* img_inout, const double* timesteps_host, int n_steps, void* stream) {
  return denoise_loop(m, in, opts ? *opts : fmi_flux_denoise_options{}, cn, ip, img_inout, timesteps_host, n_steps, stream, solver);
}
// device bytes the solvers' buffers hold (0 until the first Heun / 2M call)
extern "C" size_t fmi_flux_solver_bytes(fmi_flux* m) { return m ? m->solver_buf[0].bytes() + m->solver_buf[1].bytes() : 0; }

// The entries from before fmi_flux_denoise_with: each fills the options its arguments name — {ctx, ctl, cfg, cache, x0, noise, mask} — and takes the same path.
extern "C" int fmi_flux_denoise(fmi_flux* m, const fmi_flux_inputs* in, float* img_inout, const double* timesteps_host, int n_steps, void* stream) {
  return denoise_loop(m, in, fmi_flux_denoise_options{}, nullptr, nullptr, img_inout, timesteps_host, n_steps, stream);
}
extern "C" int fmi_flux_denoise_inpaint(fmi_flux* m, const fmi_flux_inputs* in, float* img_inout, const double* timesteps_host, int n_steps, const float* x0,
                                        const float* noise, const float* mask, void* stream) {
  if (!x0 || !noise || !mask) return fail(FMI_ERR_INVALID, "flux_denoise_inpaint: x0, noise and mask are all required");
  return denoise_loop(m, in, {/*ctx*/ nullptr, /*ctl*/ nullptr, /*cfg*/ nullptr, /*cache*/ nullptr, x0, noise, mask}, nullptr, nullptr, img_inout, timesteps_host, n_steps, stream);
}
extern "C" int fmi_flux_denoise_context(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_context* ctx, float* img_inout, const double* timesteps_host,
                                        int n_steps, const float* x0, const float* noise, const float* mask, void* stream) {
  return denoise_loop(m, in, {ctx, /*ctl*/ nullptr, /*cfg*/ nullptr, /*cache*/ nullptr, x0, noise, mask}, nullptr, nullptr, img_inout, timesteps_host, n_steps, stream);
}
extern "C" int fmi_flux_denoise_cached(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_context* ctx, float* img_inout, const double* timesteps_host,
                                       int n_steps, const float* x0, const float* noise, const float* mask, const fmi_flux_step_cache* cache, void* stream) {
  return denoise_loop(m, in, {ctx, /*ctl*/ nullptr, /*cfg*/ nullptr, cache, x0, noise, mask}, nullptr, nullptr, img_inout, timesteps_host, n_steps, stream);
}
extern "C" int fmi_flux_denoise_cfg(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_context* ctx, const fmi_flux_true_cfg* cfg, float* img_inout,
                                    const double* timesteps_host, int n_steps, const float* x0, const float* noise, const float* mask, void* stream) {
  return denoise_loop(m, in, {ctx, /*ctl*/ nullptr, cfg, /*cache*/ nullptr, x0, noise, mask}, nullptr, nullptr, img_inout, timesteps_host, n_steps, stream);
}
extern "C" int fmi_flux_denoise_control(fmi_flux* m, const fmi_flux_inputs* in, const fmi_flux_control* ctl, const fmi_flux_true_cfg* cfg, float* img_inout,
                                        const double* timesteps_host, int n_steps, const float* x0, const float* noise, const float* mask, void* stream) {
  return denoise_loop(m, in, {/*ctx*/ nullptr, ctl, cfg, /*cache*/ nullptr, x0, noise, mask}, nullptr, nullptr, img_inout, timesteps_host, n_steps, stream);
}
// device bytes the step cache holds (0 until the first fmi_flux_denoise_cached call with a cache)
extern "C" size_t fmi_flux_step_cache_bytes(fmi_flux* m) {
  if (!m) return 0;
  return m->sc_x0.bytes() + m->sc_r[0].bytes() + m->sc_r[1].bytes() + m->sc_delta.bytes() + m->sc_part.bytes() + m->sc_sums.bytes();
}

extern "C" int fmi_flux_set_profiling(fmi_flux* m, int enable) {
  if (!m) return fail(FMI_ERR_INVALID, "null handle");
  m->profiling = enable != 0;
  for (int i = 0; i < PH_COUNT; ++i) m->phase_ms[i] = 0;
  return FMI_OK;
}
extern "C" int fmi_flux_phase_count(void) { return PH_COUNT; }
extern "C" const char* fmi_flux_phase_name(int i) { return (i >= 0 && i < PH_COUNT) ? kPhaseNames[i] : nullptr; }
extern "C" int fmi_flux_phase_ms(fmi_flux* m, float* ms_out) {
  if (!m || !ms_out) return fail(FMI_ERR_INVALID, "null argument");
  for (int i = 0; i < PH_COUNT; ++i) ms_out[i] = m->phase_ms[i];
  return FMI_OK;
}
// QkNorm + RoPE + head-major / transposed relayout fused into the QKV GEMM's epilogue (default) or as stand-alone kernels
extern "C" int fmi_flux_set_fused_qkv_relayout(fmi_flux* m, int enable) {
  if (!m) return fail(FMI_ERR_INVALID, "null handle");
  m->fuse_qkv_relayout = enable != 0;
  return FMI_OK;
}
// This handle's attention kernel (fmi_set_attention_kernel's numbering), -1 = follow the process-wide switch (the default)
extern "C" int fmi_flux_set_attention_kernel(fmi_flux* m, int kind) {
  if (!m) return fail(FMI_ERR_INVALID, "null handle");
  if (kind < -1 || kind > 5) return fail(FMI_ERR_INVALID, "flux_set_attention_kernel: kind must be -1 .. 5");
  if (!alt_kernels_built() && kind != -1 && kind != 5 && kind != 1)
    return fail(FMI_ERR_UNSUPPORTED, "flux_set_attention_kernel: this build carries kernels 5 and 1; 0, 2, 3, 4 live in the test build (libflux_mi355x_alt.so: make alt)");
  m->attn_kind = kind;
  return FMI_OK;
}
// fmi_flux_denoise's modulation precompute: 1 (default) one MFMA GEMM over all steps (when they are more than 4 rows), 0 f32 GEMV passes of 4 rows,
// 2 the GEMM at any row count (how a 2-step full-size run is compared with the oracle THROUGH the 6.5 GB one-GEMM path)
extern "C" int fmi_flux_set_modulation_gemm(fmi_flux* m, int enable) {
  if (!m) return fail(FMI_ERR_INVALID, "null handle");
  m->mod_gemm = enable == 2 ? 2 : (enable != 0);
  return FMI_OK;
}
// how quantised block linears are multiplied: 0 (default) by size, 1 expanded once into bf16 copies (dense cache), 2 always fused
extern "C" int fmi_flux_set_sequence_parallel(fmi_flux* m, int rank, int world_size, fmi_all_to_all_fn a2a, void* user) {
  if (!m) return fail(FMI_ERR_INVALID, "set_sequence_parallel: null handle");
  if (m->is_cn && world_size > 1) return fail(FMI_ERR_UNSUPPORTED, "set_sequence_parallel: a ControlNet is not supported under sequence parallelism");
  if (world_size < 1 || rank < 0 || rank >= world_size) return fail(FMI_ERR_INVALID, "set_sequence_parallel: rank outside [0, world_size)");
  if (world_size > 1 && !a2a) return fail(FMI_ERR_INVALID, "set_sequence_parallel: world_size > 1 needs the all-to-all callback");
  if (m->H % world_size) return fail(FMI_ERR_INVALID, "set_sequence_parallel: " + std::to_string(m->H) + " heads do not split over " + std::to_string(world_size) + " ranks");
  m->sp_rank = rank, m->sp_world = world_size;
  m->sp_a2a = world_size > 1 ? a2a : nullptr, m->sp_user = user;
  return FMI_OK;
}
extern "C" int fmi_flux_set_split_k(fmi_flux* m, int enable) {
  if (!m) return fail(FMI_ERR_INVALID, "set_split_k: null handle");
  m->split_k = enable != 0;
  return FMI_OK;
}
extern "C" int fmi_flux_set_quant_dense_cache(fmi_flux* m, int mode) {
  if (!m) return fail(FMI_ERR_INVALID, "null handle");
  if (mode < -1 || mode > 3)
    return fail(FMI_ERR_INVALID, "set_quant_dense_cache: mode must be -1 (by memory), 0 (packed only, by size), 1 (dense cache), 2 (always fused) or 3 (by size, large launches expanded once)");
  m->dense_cache = mode == 1;
  m->quant_mode = mode;
  m->quant_auto = mode < 0;
  m->dense_ready.clear();
  return FMI_OK;
}
// static e4m3 scales of the attention operands from the QkNorm weights (see fmi_flux::fp8_attn); needs the weights in place
static int compute_attention_scales(fmi_flux* m) {
    m->attn_scales_valid = false;  // a failure half way must not leave vectors that the next call takes for valid
    auto wmax = [&](const bf16_t* dev, float* out) -> int {
      uint16_t h[128];
      FMI_HIP_TRY(hipMemcpy(h, dev, sizeof(h), hipMemcpyDeviceToHost));
      float mx = 0.f;
      for (int i = 0; i < 128; ++i) {
        uint32_t u = (uint32_t)h[i] << 16;
        float f;
        memcpy(&f, &u, 4);
        mx = std::max(mx, std::fabs(f));
      }
      *out = mx;
      return FMI_OK;
    };
    // (the same expressions, constant for constant, as flux_oracle.cpp: fp8_attn_scale / fp8_q_scale_pow2 — the oracle is a separate
    // program by rule, so the definition is shared as text, and tests/test_gpu_fp8.py compares the resulting codes bit for bit)
    auto scale_of = [](float mx) { return 448.0f / (sqrtf(128.0f) * std::max(mx, 1e-20f)); };
    // The q scale is then lowered (by less than a factor 2: e4m3 keeps its relative precision) to the value that makes the
    // attention's score factor softmax_scale * log2(e) / (sq * sk) an exact power of two 2^-n: the one-wave fp8 attention
    // (attention_w16.h, QK8) folds it into the E8M0 block scale of its score MFMA.  The oracle applies the same rule
    // (flux_oracle.cpp: fp8_q_scale_pow2).
    // n is kept: the attention gets the score factor 2^-n as an INTEGER exponent, not as a float to be recognised again
    auto q_scale_pow2 = [](float q8, float k8, int* n_out) {
      const float c0 = (1.0f / sqrtf(128.0f)) * 1.4426950408889634f;
      const int n = (int)floorf(log2f(q8 * k8 / c0));
      *n_out = n;
      return c0 * ldexpf(1.0f, n) / k8;
    };
    m->q8_dbl.assign(m->dbl.size(), 0.f), m->k8_dbl.assign(m->dbl.size(), 0.f);
    m->q8_sgl.assign(m->sgl.size(), 0.f), m->k8_sgl.assign(m->sgl.size(), 0.f);
    m->n8_dbl.assign(m->dbl.size(), 0), m->n8_sgl.assign(m->sgl.size(), 0);
    for (size_t i = 0; i < m->dbl.size(); ++i) {
      float a, b, c, d;
      FMI_TRY(wmax(m->dbl[i].nq[0], &a));
      FMI_TRY(wmax(m->dbl[i].nq[1], &b));
      FMI_TRY(wmax(m->dbl[i].nk[0], &c));
      FMI_TRY(wmax(m->dbl[i].nk[1], &d));
      m->k8_dbl[i] = scale_of(std::max(c, d));  // both streams feed one attention call: one scale
      m->q8_dbl[i] = q_scale_pow2(scale_of(std::max(a, b)), m->k8_dbl[i], &m->n8_dbl[i]);
    }
    for (size_t i = 0; i < m->sgl.size(); ++i) {
      float a, c;
      FMI_TRY(wmax(m->sgl[i].nq, &a));
      FMI_TRY(wmax(m->sgl[i].nk, &c));
      m->k8_sgl[i] = scale_of(c);
      m->q8_sgl[i] = q_scale_pow2(scale_of(a), m->k8_sgl[i], &m->n8_sgl[i]);
    }
    m->attn_scales_valid = true;
    return FMI_OK;
}
// 8-bit modes: quantise the block Linears of `mask` once (bf16 arena -> e4m3 / int8 codes + per-output-channel scale); see the header.
static int quantize_8bit(fmi_flux* m, int kind, unsigned mask, void* stream) {
  if (!m) return fail(FMI_ERR_INVALID, "null handle");
  if (m->is_cn) return fail(FMI_ERR_UNSUPPORTED, "quantize: a ControlNet runs in bf16 only (the main model may be in any mode: the injection touches its f32 stream)");
  FMI_TRY(use_device(m));
  FMI_TRY(check_ready(m));
  if (m->fp8) {
    if (m->q8_kind == kind && m->q8_mask == mask) return FMI_OK;
    return fail(FMI_ERR_STATE, "quantize: the model already holds another 8-bit form (create a new one)");
  }
  if (!(mask & 0x3f) || (mask & ~0x3fu)) return fail(FMI_ERR_INVALID, "quantize: the linear mask must name at least one of the six block linears (bits 0..5)");
  std::vector<Dense*> lin;
  for (auto& b : m->dbl)
    for (int s = 0; s < 2; ++s) {
      Dense* ds[4] = {&b.qkv[s], &b.proj[s], &b.mlp1[s], &b.mlp2[s]};
      for (int k = 0; k < 4; ++k)
        if (mask >> k & 1) lin.push_back(ds[k]);
    }
  for (auto& b : m->sgl) {
    if (mask >> 4 & 1) lin.push_back(&b.w1);
    if (mask >> 5 & 1) lin.push_back(&b.w2);
  }
  // int8 mode: the linears fed by a post-GELU operand take it on the offset grid (fp8.hip's header) unless FMI_INT8_SYMMETRIC=1 asks for
  // round 4's all-symmetric recipe (a study switch: the oracle's orc_flux_set_q8_symmetric)
  const char* sym_env = getenv("FMI_INT8_SYMMETRIC");
  const bool asym = kind == 2 && !(sym_env && atoi(sym_env) != 0);
  for (auto& b : m->dbl)
    for (int s = 0; s < 2; ++s) b.mlp2[s].w8_d0 = (asym && (mask >> 3 & 1)) ? 0 : -1;
  for (auto& b : m->sgl) b.w2.w8_d0 = (asym && (mask >> 5 & 1)) ? m->D : -1;
  size_t bytes = 0;
  for (Dense* d : lin) {
    if (d->q_type || !d->w) return fail(FMI_ERR_UNSUPPORTED, "quantize_fp8 / quantize_int8: model holds bitsandbytes-quantised linears; load a bf16 checkpoint");
    if (d->K % 128 || d->N <= 128 || d->K > 16384) return fail(FMI_ERR_UNSUPPORTED, "quantize_fp8 / quantize_int8: needs in_features % 128 == 0 (<= 16384) and out_features > 128");
    bytes += align_up((size_t)d->N * d->K, 256) + align_up((size_t)d->N * 4, 256) + (d->w8_d0 >= 0 ? align_up((size_t)d->N * 4, 256) : 0);
  }
  if (lin.empty()) return FMI_OK;
  // int8 mode after a calibration (fmi_flux_calibrate_int8 + at least one evaluation): the smoothed recipe.  e4m3 is a floating-point grid: no smoothing.
  const bool smooth = kind == 2 && m->calib && m->calib_evals > 0;
  if (kind == 2 && m->calib && !smooth) return fail(FMI_ERR_STATE, "quantize_int8: calibration is on but no evaluation has run (fmi_flux_forward / fmi_flux_denoise first, or fmi_flux_calibrate_int8(m, 0))");
  m->calib = false;
  FMI_HIP_TRY(m->fp8_arena.alloc(bytes));  // (a retry after a failed launch below starts from a fresh block: the earlier one is released here)
  char* const arena8 = m->fp8_arena.as<char>();
  hipStream_t s = (hipStream_t)stream;
  size_t off = 0;
  for (Dense* d : lin) {
    d->w8 = reinterpret_cast<uint8_t*>(arena8 + off);
    off += align_up((size_t)d->N * d->K, 256);
    d->w8_scale = reinterpret_cast<float*>(arena8 + off);
    off += align_up((size_t)d->N * 4, 256);
    const float* wvec = nullptr;
    if (smooth && d->sm_amax) {
      // s[k] = sqrt(max |x[:, k]| / max |W[:, k]|): the weights' column absmax into the scratch row, then the factors; the codes come from W * s
      FMI_HIP_TRY(hipMemsetAsync(m->calib_wmax, 0, (size_t)d->K * sizeof(float), s));
      FMI_TRY(launch_col_absmax(d->w, d->K, d->N, d->K, m->calib_wmax, s));
      // the factors are made on the host (medians; once per linear, K <= 16384): two small copies down, two up, ordered on `s`
      std::vector<float> ha(d->K), hw(d->K), hs(d->K), hi(d->K);
      FMI_HIP_TRY(hipMemcpyAsync(ha.data(), d->sm_amax, (size_t)d->K * sizeof(float), hipMemcpyDeviceToHost, s));
      FMI_HIP_TRY(hipMemcpyAsync(hw.data(), m->calib_wmax, (size_t)d->K * sizeof(float), hipMemcpyDeviceToHost, s));
      FMI_HIP_TRY(hipStreamSynchronize(s));
      smooth_factors_host(ha.data(), hw.data(), d->K, hs.data(), hi.data());
      // a linear without a single outlier channel (every factor exactly 1) keeps the plain kernels: multiplying by 1 changes no bit, skipping it saves the
      // per-channel loads in the row kernels (measured on the Gaussian bench checkpoint: 51.1 -> 50.5 ms per step when no linear smooths)
      if (std::any_of(hs.begin(), hs.end(), [](float v) { return v != 1.0f; })) {
        FMI_HIP_TRY(hipMemcpyAsync(d->sm_s, hs.data(), (size_t)d->K * sizeof(float), hipMemcpyHostToDevice, s));
        FMI_HIP_TRY(hipMemcpyAsync(d->sm_inv_store, hi.data(), (size_t)d->K * sizeof(float), hipMemcpyHostToDevice, s));
        FMI_HIP_TRY(hipStreamSynchronize(s));  // (the host vectors go out of scope)
        d->sm_inv = d->sm_inv_store;
        wvec = d->sm_s;
      }
    }
    FMI_TRY(launch_quantize_rows_fp8(d->w, d->K, d->N, d->K, d->w8, d->w8_scale, s, kind, wvec));
    if (d->w8_d0 >= 0) {
      d->w8_sum = reinterpret_cast<float*>(arena8 + off);
      off += align_up((size_t)d->N * 4, 256);
      FMI_TRY(launch_rowsum_i8(reinterpret_cast<const int8_t*>(d->w8), d->w8_scale, d->N, d->K, d->w8_d0, d->w8_sum, s));
    }
  }
  FMI_HIP_TRY(hipStreamSynchronize(s));
  FMI_TRY(compute_attention_scales(m));
  m->ws.base.reset();  // the fp8 workspace has two more buffers: rebuild on the next call
  m->fp8 = true;
  m->q8_kind = kind;
  m->q8_mask = mask;
  lora_release_storage(m);  // the adapters can no longer change (the codes were taken from the merged weights): only their names stay
  return FMI_OK;
}
// Calibration of the smoothed int8 recipe (round 6; VERDICT r5 "next" 3).  Real DiT activations have a few channels two orders of magnitude above the rest
// (the AdaLN (1 + scale) of those channels is 30-100): a per-token int8 grid then spends its 127 steps on them and rounds the other 3 000 channels to
// nothing.  enable = 1 (bf16 mode, complete weights): allocate and zero the statistics; from now on every fmi_flux_forward / fmi_flux_denoise evaluation
// also folds max |x[:, k]| of each block linear's input into them (a handful of evaluations at timesteps across the schedule is enough: the outlier channels
// are the same at every step).  The next fmi_flux_quantize_int8 then uses them — per input channel s[k] = sqrt(max|x[:, k]| / max|W[:, k]|) (SmoothQuant,
// alpha = 1/2), weight codes from W * s, activation rows from x / s, everything else as before — and switches the recording off.  enable = 0: drop the
// statistics (the next quantise is the unsmoothed recipe).  Without a calibration fmi_flux_quantize_int8 is bit for bit what it was.
extern "C" int fmi_flux_calibrate_int8(fmi_flux* m, int enable) {
  if (!m) return fail(FMI_ERR_INVALID, "null handle");
  if (m->is_cn) return fail(FMI_ERR_UNSUPPORTED, "calibrate_int8: a ControlNet runs in bf16 only");
  FMI_TRY(use_device(m));
  if (m->fp8) return fail(FMI_ERR_STATE, "calibrate_int8: the model already holds an 8-bit form (calibrate before quantising)");
  std::vector<Dense*> lin;
  for (auto& b : m->dbl)
    for (int st = 0; st < 2; ++st) {
      Dense* ds[4] = {&b.qkv[st], &b.proj[st], &b.mlp1[st], &b.mlp2[st]};
      for (int k = 0; k < 4; ++k) lin.push_back(ds[k]);
    }
  for (auto& b : m->sgl) lin.push_back(&b.w1), lin.push_back(&b.w2);
  if (!enable) {
    FMI_HIP_TRY(hipDeviceSynchronize());
    m->calib_arena.reset();
    m->calib_wmax = nullptr, m->calib = false, m->calib_evals = 0;
    for (Dense* d : lin) d->sm_amax = d->sm_s = d->sm_inv = d->sm_inv_store = nullptr;
    return FMI_OK;
  }
  FMI_TRY(check_ready(m));
  size_t floats = 0;
  int kmax = 0;
  for (Dense* d : lin) {
    if (d->q_type || !d->w) return fail(FMI_ERR_UNSUPPORTED, "calibrate_int8: model holds bitsandbytes-quantised linears; load a bf16 checkpoint");
    if (d->K % 8) return fail(FMI_ERR_UNSUPPORTED, "calibrate_int8: in_features must be a multiple of 8");
    floats += 3 * (size_t)d->K;
    kmax = std::max(kmax, d->K);
  }
  if (!m->calib_arena) FMI_HIP_TRY(m->calib_arena.alloc((floats + (size_t)kmax) * sizeof(float)));
  FMI_HIP_TRY(hipMemset(m->calib_arena.ptr, 0, (floats + (size_t)kmax) * sizeof(float)));
  float* p = m->calib_arena.as<float>();
  for (Dense* d : lin) {
    d->sm_amax = p, d->sm_s = p + d->K, d->sm_inv_store = p + 2 * (size_t)d->K, d->sm_inv = nullptr;
    p += 3 * (size_t)d->K;
  }
  m->calib_wmax = p;
  m->calib = true, m->calib_evals = 0;
  return FMI_OK;
}
extern "C" int fmi_flux_quantize_fp8(fmi_flux* m, void* stream) { return quantize_8bit(m, 1, 0x3f, stream); }
// int8 mode (round 4): the same per-row recipe on int8 codes (fp8.hip's header) for the linears of `linear_mask`; the others stay bf16.
extern "C" int fmi_flux_quantize_int8(fmi_flux* m, unsigned linear_mask, void* stream) { return quantize_8bit(m, 2, linear_mask, stream); }
// fp8 mode only: 1 (default) = q and k leave the fused relayout epilogue as e4m3 and QK^T runs on the fp8 MFMA whenever
// both streams of a block take that epilogue (token counts multiples of 16); 0 = bf16 attention operands
extern "C" int fmi_flux_set_fp8_attention(fmi_flux* m, int enable) {
  if (!m) return fail(FMI_ERR_INVALID, "null handle");
  if (enable < 0 || enable > 2) return fail(FMI_ERR_INVALID, "set_fp8_attention: 0 (off), 1 (on in the 8-bit modes) or 2 (on in every mode)");
  if (m->is_cn && enable == 2) return fail(FMI_ERR_UNSUPPORTED, "set_fp8_attention: a ControlNet runs in bf16 only");
  m->fp8_attn = enable;
  // 2 in bf16 mode: the static scales come from the QkNorm weights — taken here when the weights are complete (not inside the next evaluation: they
  // are small synchronous copies), else at the first evaluation after the last tensor arrived
  if (enable == 2 && !m->attn_scales_valid && m->missing.names.empty()) {
    FMI_TRY(use_device(m));
    FMI_TRY(compute_attention_scales(m));
  }
  return FMI_OK;
}
// 4-bit weights, process-wide: number of rows from which the one-wave-per-SIMD fused dequant-GEMM (gemm_w4q.h) runs
// instead of the two-workgroups-per-CU one (default 256)
extern "C" int fmi_set_bnb4_onewave_min_rows(int rows) {
  if (rows < 1) return fail(FMI_ERR_INVALID, "set_bnb4_onewave_min_rows: rows must be positive");
  set_gemm_w4q_min_rows(rows);
  return FMI_OK;
}
// test hook: 0 = rescale every tile, else deferred-rescale threshold (default)
extern "C" int fmi_flux_set_attention_rescale_threshold(fmi_flux* m, int thr_x16) {
  if (!m) return fail(FMI_ERR_INVALID, "null handle");
  m->attn_thr = thr_x16;
  return FMI_OK;
}

// ---------------------------------------------------------------------------------------- LoRA adapters (merged; the kernel is lora.hip)
namespace {

// Everything a later re-merge of the Linear `wname` can need, taken BEFORE any adapter state changes (so that a failed allocation leaves the model as it
// was): the factor scratch for the total rank of every plain pair on it plus the term `extra` about to arrive, the descriptor block if a term of another kind is among them, and the pristine copy of its rows (while there is none, the rows ARE
// the loaded weights).  A copy made for a Linear that then has no active adapter is released again by lora_remerge.
int lora_reserve(fmi_flux* m, const std::string& wname, const AdapterTerm* extra = nullptr) {
  const Dest& dst = m->names.at(wname);
  const int rows = dst.rows, K = dst.cols;
  // R: the plain pairs' total rank (the all-LoRA path); T: every term, `mixed`: one of them is no plain pair (the descriptors of adapter_merge_kernel)
  int R = extra && extra->kind == FMI_ADAPTER_LORA ? extra->r : 0, T = extra ? 1 : 0;
  bool mixed = extra && extra->kind != FMI_ADAPTER_LORA;
  for (const auto& ad : m->loras) {
    auto it = ad.second.pairs.find(wname);
    if (it == ad.second.pairs.end()) continue;
    if (it->second.kind == FMI_ADAPTER_LORA) R += it->second.r;
    else mixed = true;
    ++T;
  }
  if (T == 0) return FMI_OK;
  if (mixed && m->lora_descs.bytes() < (size_t)T * sizeof(AdapterDesc)) {  // grow-only; a model of plain pairs never holds the block
    DeviceBuffer grown;
    hipError_t e = grown.alloc((size_t)T * sizeof(AdapterDesc));
    if (e != hipSuccess) return fail(FMI_ERR_NOMEM, std::string("lora: hipMalloc of the term descriptors failed: ") + hipGetErrorString(e));
    if (m->lora_descs) m->lora_dead.push_back(std::move(m->lora_descs));
    m->lora_descs = std::move(grown);
  }
  const int Rpad = (R + LORA_RANK_CHUNK - 1) / LORA_RANK_CHUNK * LORA_RANK_CHUNK;
  const int rows_pad = (rows + LORA_TILE_ROWS - 1) / LORA_TILE_ROWS * LORA_TILE_ROWS;
  const size_t need = align_up((size_t)Rpad * K * 4, 256) + (size_t)Rpad * rows_pad * 8;
  if (R > 0 && m->lora_scratch.bytes() < need) {  // grow-only
    DeviceBuffer grown;
    hipError_t e = grown.alloc(need);
    if (e != hipSuccess) return fail(FMI_ERR_NOMEM, std::string("lora: hipMalloc of the factor scratch failed: ") + hipGetErrorString(e));
    if (m->lora_scratch) m->lora_dead.push_back(std::move(m->lora_scratch));  // (an earlier merge of this call may still read it: freed after the call's synchronisation)
    m->lora_scratch = std::move(grown);
  }
  if (!m->lora_backup.count(wname)) {
    const size_t bytes = (size_t)rows * K * 2;
    DeviceBuffer fresh;
    hipError_t e = fresh.alloc(bytes);
    if (e != hipSuccess) return fail(FMI_ERR_NOMEM, std::string("lora: hipMalloc of the pristine copy failed: ") + hipGetErrorString(e));
    e = hipMemcpyAsync(fresh.ptr, dst.d->w + (size_t)dst.d->parts[dst.part].r0 * K, bytes, hipMemcpyDeviceToDevice, nullptr);
    if (e != hipSuccess) return fail(FMI_ERR_HIP, std::string("lora: ") + hipGetErrorString(e));
    m->lora_backup.emplace(wname, std::move(fresh));
  }
  return FMI_OK;
}

// The rows of the Linear `wname` <- bf16_rne(W0 + sum over the active adapters, in name order, of weight * scale * (B A)), always from the pristine copy.
// No active adapter: the rows are W0 again (copied back) and the copy is released.  Allocates nothing (lora_reserve did): per adapter one launch that
// packs its factors into the scratch, then the merge kernel — all on the null stream, in order, so one scratch block serves Linear after Linear; the C
// entry that called synchronises the device before it returns (lora_leave).
int lora_remerge(fmi_flux* m, const std::string& wname) {
  const Dest& dst = m->names.at(wname);
  Dense* d = dst.d;
  const int rows = dst.rows, K = dst.cols;
  bf16_t* w = d->w + (size_t)d->parts[dst.part].r0 * K;
  const size_t bytes = (size_t)rows * K * 2;
  struct Term {
    const AdapterTerm* p;
    double weight;
    double coef;  // weight * scale, exact in f64
  };
  std::vector<Term> terms;
  int R = 0;
  bool plain = true;  // every active term is a plain pair: today's path, lora_pack_kernel + lora_merge_kernel with the same arguments
  for (const auto& ad : m->loras) {
    if (ad.second.weight == 0.f) continue;
    auto it = ad.second.pairs.find(wname);
    if (it == ad.second.pairs.end()) continue;
    terms.push_back({&it->second, (double)ad.second.weight, (double)ad.second.weight * (double)it->second.scale});
    R += it->second.r;
    plain = plain && it->second.kind == FMI_ADAPTER_LORA;
  }
  auto bk = m->lora_backup.find(wname);
  if (terms.empty()) {
    if (bk != m->lora_backup.end()) {
      FMI_HIP_TRY(hipMemcpyAsync(w, bk->second.ptr, bytes, hipMemcpyDeviceToDevice, nullptr));
      m->lora_dead.push_back(std::move(bk->second));  // freed after the call's one synchronisation
      m->lora_backup.erase(bk);
    }
    return FMI_OK;
  }
  if (!plain) {  // a LoHa / LoKr / DoRA term among them: one launch of adapter_merge_kernel over the terms in name order (plain pairs included, each as its own term)
    if (bk == m->lora_backup.end() || m->lora_descs.bytes() < terms.size() * sizeof(AdapterDesc)) return fail(FMI_ERR_STATE, "lora: re-merge without its reserved storage");
    std::vector<AdapterDesc> descs;
    for (const Term& t : terms) descs.push_back(adapter_term_desc(*t.p, t.weight));
    // (a blocking copy on the null stream: ordered behind the merge of the previous Linear, which read the same block)
    FMI_HIP_TRY(hipMemcpy(m->lora_descs.ptr, descs.data(), descs.size() * sizeof(AdapterDesc), hipMemcpyHostToDevice));
    return launch_adapter_merge(bk->second.as<bf16_t>(), w, rows, K, m->lora_descs.as<AdapterDesc>(), (int)descs.size(), nullptr);
  }
  const int Rpad = (R + LORA_RANK_CHUNK - 1) / LORA_RANK_CHUNK * LORA_RANK_CHUNK;
  const int rows_pad = (rows + LORA_TILE_ROWS - 1) / LORA_TILE_ROWS * LORA_TILE_ROWS;
  const size_t a_bytes = align_up((size_t)Rpad * K * 4, 256), b_bytes = (size_t)Rpad * rows_pad * 8;
  if (bk == m->lora_backup.end() || m->lora_scratch.bytes() < a_bytes + b_bytes) return fail(FMI_ERR_STATE, "lora: re-merge without its reserved storage");
  float* Acat = m->lora_scratch.as<float>();
  double* Bt = reinterpret_cast<double*>(m->lora_scratch.as<char>() + a_bytes);
  if (Rpad > R) {  // the rank rows that pad the last chunk (the pack launches write every other byte the kernel reads)
    FMI_HIP_TRY(hipMemsetAsync(Acat + (size_t)R * K, 0, (size_t)(Rpad - R) * K * 4, nullptr));
    FMI_HIP_TRY(hipMemsetAsync(Bt + (size_t)R * rows_pad, 0, (size_t)(Rpad - R) * rows_pad * 8, nullptr));
  }
  int off = 0;
  for (const Term& t : terms) {
    FMI_TRY(launch_lora_pack(t.p->f[0].as<float>(), t.p->f[1].as<float>(), rows, K, t.p->r, t.coef, Acat, Bt, rows_pad, off, nullptr));
    off += t.p->r;
  }
  return launch_lora_merge(bk->second.as<bf16_t>(), w, rows, K, Acat, Bt, rows_pad, Rpad, nullptr);
}

// the end of every mutating LoRA call: nothing is in flight when it returns; what the call retired is freed behind that one synchronisation
int lora_leave(fmi_flux* m, int rc) {
  hipError_t e = hipDeviceSynchronize();
  if (rc == FMI_OK && e != hipSuccess) rc = fail(FMI_ERR_HIP, std::string("lora: ") + hipGetErrorString(e));
  m->lora_dead.clear();
  if (m->loras.empty()) m->lora_scratch.reset(), m->lora_descs.reset();
  return rc;
}

// what every mutating LoRA call checks first: a complete bf16-mode model; then the device is drained (load-time calls: this orders them against evaluations on any stream)
int lora_enter(fmi_flux* m, const char* what) {
  if (m->fp8) return fail(FMI_ERR_STATE, std::string(what) + ": the model was quantised to 8 bits; adapters go in before fmi_flux_quantize_fp8 / fmi_flux_quantize_int8");
  FMI_TRY(m->missing.ready(what));
  FMI_TRY(use_device(m));
  FMI_HIP_TRY(hipDeviceSynchronize());
  return finalize(m);
}

}  // namespace

extern "C" int fmi_flux_lora_add_term(fmi_flux* m, const char* adapter, const char* prefix, const fmi_adapter_term* term) {
  if (!m || !adapter || !prefix || !term) return fail(FMI_ERR_INVALID, "lora_add: null argument");
  if (m->is_cn) return fail(FMI_ERR_UNSUPPORTED, "lora_add: LoRA-patched ControlNets are out of scope");
  if (m->fp8) return fail(FMI_ERR_STATE, "lora_add: the model was quantised to 8 bits; adapters go in before fmi_flux_quantize_fp8 / fmi_flux_quantize_int8");
  if (!*adapter) return fail(FMI_ERR_INVALID, "lora_add: empty adapter name");
  const std::string wname = std::string(prefix) + ".weight";
  auto it = m->names.find(wname);
  if (it == m->names.end() || !it->second.d || it->second.bias || !it->second.cols)
    return fail(FMI_ERR_INVALID, std::string("lora_add: '") + prefix + "' is not a Linear of this model");
  FMI_TRY(lora_enter(m, "lora_add"));
  const Dest& dst = it->second;
  const Dense* d = dst.d;
  if (!part_is_plain(*d, dst.part))
    return fail(FMI_ERR_UNSUPPORTED, std::string("lora_add: ") + prefix + " is resident as nf4 / fp4 / LLM.int8 codes; merging into packed codes is not implemented");
  if (dst.cols % 8) return fail(FMI_ERR_UNSUPPORTED, "lora_add: in_features must be a multiple of 8");
  // the pristine rows (DoRA's norm reads them): the copy while the Linear has one, else the resident rows, which then ARE the loaded weights
  auto bk = m->lora_backup.find(wname);
  const bf16_t* w0 = bk != m->lora_backup.end() ? bk->second.as<bf16_t>() : d->w + (size_t)d->parts[dst.part].r0 * dst.cols;
  AdapterTerm nt;
  FMI_TRY(adapter_term_build(term, w0, dst.rows, dst.cols, std::string("lora_add: ") + prefix, &nt));
  // storage first, state second: until here nothing of the model has changed, and a re-merge allocates nothing
  if (int rc = lora_reserve(m, wname, &nt)) return lora_leave(m, rc);
  // re-adding a term replaces it: the move-assignment frees the slot's earlier factors HERE (the device is idle: lora_enter), after lora_reserve
  m->loras[adapter].pairs[wname] = std::move(nt);  // (a new adapter starts at weight 1)
  return lora_leave(m, lora_remerge(m, wname));
}

extern "C" int fmi_flux_lora_add(fmi_flux* m, const char* adapter, const char* prefix, const void* A, const void* B, fmi_dtype dtype, int rank, float scale) {
  if (!m || !adapter || !prefix || !A || !B) return fail(FMI_ERR_INVALID, "lora_add: null argument");
  if (rank < 1) return fail(FMI_ERR_INVALID, "lora_add: rank must be at least 1");
  fmi_adapter_term t{};
  t.kind = FMI_ADAPTER_LORA, t.dtype = dtype, t.scale = scale;
  t.factor[0] = A, t.factor[1] = B;
  auto it = m->names.find(std::string(prefix) + ".weight");  // (the factors' shapes follow from the rank and the Linear, as this entry always took them)
  const int rows = it != m->names.end() ? it->second.rows : 1, K = it != m->names.end() && it->second.cols ? it->second.cols : 1;
  t.factor_rows[0] = rank, t.factor_cols[0] = K, t.factor_rows[1] = rows, t.factor_cols[1] = rank;
  return fmi_flux_lora_add_term(m, adapter, prefix, &t);
}

extern "C" int fmi_flux_lora_set_weight(fmi_flux* m, const char* adapter, float weight) {
  if (!m || !adapter) return fail(FMI_ERR_INVALID, "lora_set_weight: null argument");
  if (m->is_cn) return fail(FMI_ERR_UNSUPPORTED, "lora_set_weight: LoRA-patched ControlNets are out of scope");
  if (m->fp8) return fail(FMI_ERR_STATE, "lora_set_weight: the model was quantised to 8 bits (the codes were taken from the merged weights)");
  if (!std::isfinite(weight)) return fail(FMI_ERR_INVALID, "lora_set_weight: weight must be finite");
  auto it = m->loras.find(adapter);
  if (it == m->loras.end()) return fail(FMI_ERR_INVALID, std::string("lora_set_weight: unknown adapter '") + adapter + "'");
  FMI_TRY(lora_enter(m, "lora_set_weight"));
  int rc = FMI_OK;
  for (const auto& pr : it->second.pairs)
    if ((rc = lora_reserve(m, pr.first)) != FMI_OK) return lora_leave(m, rc);  // (nothing has changed yet)
  it->second.weight = weight;
  for (const auto& pr : it->second.pairs)
    if ((rc = lora_remerge(m, pr.first)) != FMI_OK) break;
  return lora_leave(m, rc);
}

extern "C" int fmi_flux_lora_remove(fmi_flux* m, const char* adapter) {
  if (!m) return fail(FMI_ERR_INVALID, "lora_remove: null handle");
  if (m->is_cn) return fail(FMI_ERR_UNSUPPORTED, "lora_remove: LoRA-patched ControlNets are out of scope");
  if (m->fp8) return fail(FMI_ERR_STATE, "lora_remove: the model was quantised to 8 bits (the codes were taken from the merged weights)");
  if (adapter && !m->loras.count(adapter)) return fail(FMI_ERR_INVALID, std::string("lora_remove: unknown adapter '") + adapter + "'");
  if (m->loras.empty()) return FMI_OK;
  FMI_TRY(lora_enter(m, "lora_remove"));
  std::set<std::string> touched;
  for (const auto& ad : m->loras)
    if (!adapter || ad.first == adapter)
      for (const auto& pr : ad.second.pairs) touched.insert(pr.first);
  int rc = FMI_OK;
  for (const std::string& wname : touched)
    if ((rc = lora_reserve(m, wname)) != FMI_OK) return lora_leave(m, rc);  // (nothing has changed yet)
  for (auto ad = m->loras.begin(); ad != m->loras.end();) {
    if (adapter && ad->first != adapter) {
      ++ad;
      continue;
    }
    ad = m->loras.erase(ad);  // (frees its factors: the device is idle, lora_enter)
  }
  for (const std::string& wname : touched)
    if ((rc = lora_remerge(m, wname)) != FMI_OK) break;
  return lora_leave(m, rc);
}

// the 8-bit modes freeze the adapters: their factors, the pristine copies and the scratch are of no further use (up to 17 GB for a full-model adapter)
static void lora_release_storage(fmi_flux* m) {
  hipDeviceSynchronize();
  for (auto& ad : m->loras)
    for (auto& pr : ad.second.pairs) {
      for (DeviceBuffer& f : pr.second.f) f.reset();
      pr.second.x.reset();
    }
  m->lora_backup.clear();
  m->lora_scratch.reset();
  m->lora_descs.reset();
}

extern "C" int fmi_flux_lora_count(const fmi_flux* m) { return m ? (int)m->loras.size() : 0; }
extern "C" const char* fmi_flux_lora_name(const fmi_flux* m, int i) {
  if (!m || i < 0 || i >= (int)m->loras.size()) return nullptr;
  auto it = m->loras.begin();
  std::advance(it, i);
  return it->first.c_str();  // (map nodes are stable: valid until that adapter is removed)
}

extern "C" int fmi_flux_get_tensor(fmi_flux* m, const char* name, void* out, fmi_dtype dtype, const int64_t* shape, int rank) {
  if (!m || !name || !out || !shape) return fail(FMI_ERR_INVALID, "flux_get_tensor: null argument");
  auto it = m->names.find(name);
  if (it == m->names.end()) return fail(FMI_ERR_INVALID, std::string("flux_get_tensor: unknown tensor name '") + name + "'");
  const Dest& d = it->second;
  const bool ok = d.cols ? (rank == 2 && shape[0] == d.rows && shape[1] == d.cols) : (rank == 1 && shape[0] == d.rows);
  if (!ok) return fail(FMI_ERR_INVALID, std::string("flux_get_tensor: shape mismatch for ") + name + ": expected (" + std::to_string(d.rows) + (d.cols ? "," + std::to_string(d.cols) : "") + ")");
  if (dtype != FMI_F32 && dtype != FMI_BF16) return fail(FMI_ERR_INVALID, "flux_get_tensor: dtype must be F32 or BF16 (the exact read-backs of a bf16 value)");
  if (m->missing.names.count(name)) return fail(FMI_ERR_STATE, std::string("flux_get_tensor: ") + name + " was never set");
  FMI_TRY(use_device(m));
  FMI_HIP_TRY(hipDeviceSynchronize());
  if (m->missing.names.empty()) FMI_TRY(finalize(m));  // (a quantised part of a mixed fused matrix becomes dense rows here, as at the first evaluation)
  const void* src = d.ptr;
  if (d.d && !d.bias) {
    if (!part_is_plain(*d.d, d.part))
      return fail(FMI_ERR_UNSUPPORTED, std::string("flux_get_tensor: ") + name + " is resident only as packed nf4 / fp4 / LLM.int8 codes");
    src = d.d->w + (size_t)d.d->parts[d.part].r0 * d.d->K;  // the row range of the fused matrix
  }
  if (dtype == FMI_BF16) {
    FMI_HIP_TRY(hipMemcpy(out, src, (size_t)d.numel * 2, hipMemcpyDefault));
    return FMI_OK;
  }
  DeviceBuffer tmp;  // (the cast runs on the device, the copy out follows: the staging of upload_as_f32 the other way round)
  FMI_HIP_TRY(tmp.alloc((size_t)d.numel * 4));
  int rc = launch_cast_to_f32(src, FMI_BF16, tmp.as<float>(), d.numel, nullptr);
  hipError_t e = hipDeviceSynchronize();
  if (rc == FMI_OK && e == hipSuccess) e = hipMemcpy(out, tmp.ptr, (size_t)d.numel * 4, hipMemcpyDefault);
  if (rc == FMI_OK && e != hipSuccess) rc = fail(FMI_ERR_HIP, std::string("flux_get_tensor: ") + hipGetErrorString(e));
  return rc;
}

// ---- ControlNet test seams
// The ControlNet alone: one evaluation on `in` (img, timesteps and every other field as for fmi_flux_forward) and cond (B,S,in_channels); the samples stay in the
// handle, for fmi_flux_controlnet_sample to widen.
extern "C" int fmi_flux_controlnet_eval(fmi_flux* net, const fmi_flux_inputs* in, const void* cond, fmi_dtype cond_dtype, void* stream) {
  if (!net || !net->is_cn) return fail(FMI_ERR_INVALID, "flux_controlnet_eval: not a ControlNet handle");
  FMI_TRY(check_inputs(net, in));
  if (!in->img || !in->timesteps || !cond) return fail(FMI_ERR_INVALID, "flux_controlnet_eval: null img/timesteps/cond");
  if (cond_dtype != FMI_F32 && cond_dtype != FMI_BF16) return fail(FMI_ERR_INVALID, "flux_controlnet_eval: cond_dtype must be F32 or BF16");
  if (net->cfg.guidance_embeds && !in->guidance) return fail(FMI_ERR_INVALID, "flux: a guidance_embeds ControlNet needs a guidance vector");
  hipStream_t s = (hipStream_t)stream;
  const fmi_flux_controlnet cn{net, cond, cond_dtype, 1.0f, nullptr};
  EvalPlan p{fmi_flux_denoise_options{}, 0, in->B, &cn};
  FMI_TRY(cn_prepare(net, in, p, s));
  FMI_TRY(launch_cast_to_f32(in->img, in->img_dtype, net->ws.img_f32, (int64_t)in->B * in->S * net->cfg.in_channels, s));
  return forward_core(net, in, cn_plan(p), net->ws.img_f32, in->timesteps, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s);
}
// Sample `index` of the double (single == 0) or single blocks of the last evaluation, widened exactly: out_f32 (B,S,D) device.  Synchronises the device.
extern "C" int fmi_flux_controlnet_sample(fmi_flux* net, int single, int index, float* out_f32) {
  if (!net || !net->is_cn || !out_f32) return fail(FMI_ERR_INVALID, "flux_controlnet_sample: not a ControlNet handle, or a null output");
  const int n = (int)(single ? net->cn_sgl.size() : net->cn_dbl.size());
  if (index < 0 || index >= n) return fail(FMI_ERR_INVALID, "flux_controlnet_sample: index outside the net's blocks");
  if (!net->cn_samples || !net->cn_elems) return fail(FMI_ERR_STATE, "flux_controlnet_sample: the ControlNet has not been evaluated yet");
  FMI_TRY(use_device(net));
  FMI_HIP_TRY(hipDeviceSynchronize());
  FMI_TRY(launch_cast_to_f32(net->cn_samples.as<bf16_t>() + ((single ? net->cn_dbl.size() : 0) + index) * net->cn_elems, FMI_BF16, out_f32, (int64_t)net->cn_elems, nullptr));
  FMI_HIP_TRY(hipDeviceSynchronize());
  return FMI_OK;
}
