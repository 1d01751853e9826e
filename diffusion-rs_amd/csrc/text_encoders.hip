// text_encoders.hip — the two text encoders in front of the FLUX denoise loop:
//   fmi_t5_*   == T5EncoderModel::forward          (diffusion_rs_core/src/models/t5/mod.rs:609-632)
//   fmi_clip_* == ClipTextTransformer::forward     (diffusion_rs_core/src/models/clip/text.rs:303-317)
// They run once per image (~0.1 % of a 50-step generation), so the design goal is exact
// semantics on the existing MFMA GEMM, not a new roofline: every Linear goes through
// launch_gemm (fused [q|k|v] and [wi_0|wi_1] weights, f32 residual stream updated in the GEMM
// epilogue), norms / activations / embedding gathers are single-pass HBM kernels, and the d=64
// attention (T5: additive relative-position bias, no 1/sqrt(d); CLIP: causal) is a small
// lane-per-key kernel — L <= 512 keys, 64 heads: 0.1 TFLOP per prompt, not worth an MFMA pipeline.
// What the vision towers (vision_encoders.hip) run as well — the layer kernels, the handle frame, the encoder layer — is in encoder_common.h.
#include "encoder_common.h"
#include "quant_kinds.h"

namespace fmi {
namespace {

// ------------------------------------------------------------------------------------ kernels
// x(r,:) = table[ids[r]] (+ pos[r % T]) as f32.  Embedding::forward (+ ClipTextEmbeddings :63-71)
__global__ void embed_gather_kernel(const int32_t* ids, const bf16_t* table, const bf16_t* pos, int T, int D, int vocab, float* x, int* err) {
  const int r = blockIdx.x;
  const int id = ids[r];
  if (id < 0 || id >= vocab) {
    if (threadIdx.x == 0) atomicExch(err, 1);
    return;
  }
  const bf16_t* src = table + (int64_t)id * D;
  const bf16_t* ps = pos ? pos + (int64_t)(r % T) * D : nullptr;
  for (int i = threadIdx.x; i < D; i += blockDim.x) x[(int64_t)r * D + i] = bf16_to_f32(src[i]) + (ps ? bf16_to_f32(ps[i]) : 0.f);
}

// T5LayerNorm (t5/mod.rs:110-121): x * rsqrt(mean(x^2) + eps) * w ; one wave per row
__global__ void t5_rmsnorm_kernel(const float* x, const bf16_t* w, float eps, int rows, int D, bf16_t* out_bf, float* out_f32) {
  const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* xr = x + (int64_t)r * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s += xr[i] * xr[i];
  s = wave_sum(s);
  const float inv = 1.0f / sqrtf(s / (float)D + eps);
  for (int i = lane; i < D; i += 64) {
    const float v = xr[i] * inv * bf16_to_f32(w[i]);
    if (out_bf) out_bf[(int64_t)r * D + i] = f32_to_bf16(v);
    if (out_f32) out_f32[(int64_t)r * D + i] = v;
  }
}

// position_bias[h][i][j] = rel[bucket(j - i)][h]; the bucket of every distance is computed on the
// host with the reference's own float formula (t5/mod.rs:340-376) so that no device logf rounding
// can move a boundary.  One block per (i, h).
__global__ void t5_bias_kernel(const bf16_t* rel, const int* bucket_of_dist, int H, int T, float* bias) {
  const int i = blockIdx.x, h = blockIdx.y;
  for (int j = threadIdx.x; j < T; j += blockDim.x) bias[((int64_t)h * T + i) * T + j] = bf16_to_f32(rel[(int64_t)bucket_of_dist[j - i + T - 1] * H + h]);
}

// pooled[b] = hidden[b, argmax_t ids[b, t]] (first maximum); clip/text.rs:305-316
__global__ void clip_pool_kernel(const float* hidden, const int32_t* ids, int T, int D, float* pooled) {
  const int b = blockIdx.x;
  __shared__ int best;
  if (threadIdx.x == 0) {
    int bi = 0;
    for (int t = 1; t < T; ++t)
      if (ids[b * T + t] > ids[b * T + bi]) bi = t;
    best = bi;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += blockDim.x) pooled[(int64_t)b * D + i] = hidden[((int64_t)b * T + best) * D + i];
}

// the reference's bucket of a relative position (t5/mod.rs:340-376), rel = j - i
int t5_bucket_of(int rel, int num_buckets_total, int max_distance) {
  const unsigned num_buckets = (unsigned)num_buckets_total / 2, max_exact = num_buckets / 2;
  auto large = [&](unsigned dist) -> unsigned {
    const float b = (logf((float)dist / (float)max_exact) / logf((float)max_distance / (float)max_exact)) * (float)(num_buckets - max_exact);
    return (unsigned)b;
  };
  if (rel > 0) {
    const unsigned d = (unsigned)rel;
    if (d < max_exact) return (int)(d + num_buckets);
    const unsigned v = max_exact + num_buckets + large(d);
    return (int)(v < (unsigned)num_buckets_total - 1 ? v : (unsigned)num_buckets_total - 1);
  }
  const unsigned d = (unsigned)(-rel);
  if (d < max_exact) return (int)d;
  const unsigned v = max_exact + large(d);
  return (int)(v < num_buckets - 1 ? v : num_buckets - 1);
}

}  // namespace
}  // namespace fmi

using namespace fmi;

// =============================================================================================== T5
struct fmi_t5 : EncoderHandle {
  fmi_t5_config cfg;
  bf16_t *shared = nullptr, *rel = nullptr, *final_ln = nullptr;
  struct Layer {
    bf16_t *ln0, *qkv, *o, *ln1, *wi, *wo;
  };
  std::vector<Layer> layers;
  std::vector<int> bucket_host;
};

static void t5_layout(fmi_t5* m) {
  const fmi_t5_config& c = m->cfg;
  const int D = c.d_model, I = c.num_heads * c.d_kv, F = c.d_ff;
  const bool gated = c.feed_forward_act != FMI_T5_RELU;
  Registry& r = m->r;
  m->shared = r.take((size_t)c.vocab_size * D);
  r.reg("shared.weight", m->shared, c.vocab_size, D);
  m->rel = r.take((size_t)c.relative_attention_num_buckets * c.num_heads);
  r.reg("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", m->rel, c.relative_attention_num_buckets, c.num_heads);
  m->layers.resize(c.num_layers);
  for (int l = 0; l < c.num_layers; ++l) {
    fmi_t5::Layer& L = m->layers[l];
    const std::string p = "encoder.block." + std::to_string(l) + ".layer.";
    L.ln0 = r.take(D);
    r.reg(p + "0.layer_norm.weight", L.ln0, D, 0);
    L.qkv = r.take((size_t)3 * I * D);  // fused [q|k|v]
    const char* nm[3] = {"q", "k", "v"};
    for (int i = 0; i < 3; ++i) r.reg(p + "0.SelfAttention." + nm[i] + ".weight", L.qkv ? L.qkv + (size_t)i * I * D : nullptr, I, D);
    L.o = r.take((size_t)D * I);
    r.reg(p + "0.SelfAttention.o.weight", L.o, D, I);
    L.ln1 = r.take(D);
    r.reg(p + "1.layer_norm.weight", L.ln1, D, 0);
    if (gated) {
      L.wi = r.take((size_t)2 * F * D);  // fused [wi_0 | wi_1]
      r.reg(p + "1.DenseReluDense.wi_0.weight", L.wi, F, D);
      r.reg(p + "1.DenseReluDense.wi_1.weight", L.wi ? L.wi + (size_t)F * D : nullptr, F, D);
    } else {
      L.wi = r.take((size_t)F * D);
      r.reg(p + "1.DenseReluDense.wi.weight", L.wi, F, D);
    }
    L.wo = r.take((size_t)D * F);
    r.reg(p + "1.DenseReluDense.wo.weight", L.wo, D, F);
  }
  m->final_ln = r.take(D);
  r.reg("encoder.final_layer_norm.weight", m->final_ln, D, 0);
}

extern "C" void fmi_t5_default_config(fmi_t5_config* c) {
  if (!c) return;
  // google/t5-v1_1-xxl encoder as shipped in FLUX.1's text_encoder_2/config.json
  c->vocab_size = 32128, c->d_model = 4096, c->d_kv = 64, c->d_ff = 10240, c->num_layers = 24, c->num_heads = 64;
  c->relative_attention_num_buckets = 32, c->relative_attention_max_distance = 128, c->layer_norm_epsilon = 1e-6f;
  c->feed_forward_act = FMI_T5_GATED_GELU;
}

extern "C" int fmi_t5_create(const fmi_t5_config* cfg, fmi_t5** out) {
  if (!cfg || !out) return fail(FMI_ERR_INVALID, "t5_create: null argument");
  if (cfg->d_kv != 64) return fail(FMI_ERR_UNSUPPORTED, "t5_create: d_kv must be 64 (got " + std::to_string(cfg->d_kv) + ")");
  if (cfg->d_model % 64 || cfg->d_ff % 64 || cfg->d_model <= 0 || cfg->num_layers <= 0 || cfg->num_heads <= 0 || cfg->vocab_size <= 0)
    return fail(FMI_ERR_INVALID, "t5_create: d_model and d_ff must be positive multiples of 64");
  if (cfg->feed_forward_act < FMI_T5_RELU || cfg->feed_forward_act > FMI_T5_GATED_SILU) return fail(FMI_ERR_INVALID, "t5_create: bad feed_forward_act");
  if (cfg->relative_attention_num_buckets < 4 || cfg->relative_attention_max_distance < 2) return fail(FMI_ERR_INVALID, "t5_create: bad relative attention config");
  std::unique_ptr<fmi_t5> m(new fmi_t5());
  m->cfg = *cfg;
  FMI_TRY(create_arena("t5_create", m.get(), t5_layout, /*zero=*/false));
  *out = m.release();
  return FMI_OK;
}
extern "C" void fmi_t5_destroy(fmi_t5* m) { delete m; }  // (the weight arena and the workspace are DeviceBuffers)
extern "C" int fmi_t5_set_tensor(fmi_t5* m, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  return enc_set_tensor(m, "t5_set_tensor", name, data, dtype, shape, rank);
}
// Quantised T5 Linears.  The reference builds every T5 Linear through `linear_no_bias(.., &cfg.quantization_config, ..)`
// (t5/mod.rs:132-133,164-173,258-261) -> BnbLinear (bitsandbytes/mod.rs:111-239), whose forward is "dequantise W, then matmul"
// (:293-312).  The encoder runs ONCE per image (25 ms of 3.2 s), so the codes are expanded once, here, into the linear's slot of
// the bf16 arena with the library's own dequant kernels (kDequantizeBlockwise / dequantize_8bit semantics: bit-exact with the
// stand-alone entry points) and the forward is the dense one: the same numbers BnbLinear::forward produces, no per-call expansion.
namespace {
int t5_linear_dest(fmi_t5* m, const char* who, const char* prefix, int out_features, int in_features, Dest* out, std::string* wname) {
  *wname = std::string(prefix) + ".weight";
  auto it = m->r.names.find(*wname);
  if (it == m->r.names.end() || !it->second.cols) return fail(FMI_ERR_INVALID, std::string(who) + ": unknown linear '" + prefix + "'");
  if (wname->find("SelfAttention.") == std::string::npos && wname->find("DenseReluDense.") == std::string::npos)
    return fail(FMI_ERR_INVALID, std::string(who) + ": '" + prefix + "' is not a Linear of the encoder blocks");
  if (it->second.rows != out_features || it->second.cols != in_features) return fail(FMI_ERR_INVALID, std::string(who) + ": shape mismatch for " + *wname);
  *out = it->second;
  return FMI_OK;
}
}  // namespace
extern "C" int fmi_t5_set_linear_bnb4(fmi_t5* m, const char* prefix, const uint8_t* packed, const float* absmax, int blocksize, int quant_type,
                                      int out_features, int in_features) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m || !prefix || !packed || !absmax) return fail(FMI_ERR_INVALID, "t5_set_linear_bnb4: null argument");
  if (quant_type != 1 && quant_type != 2) return fail(FMI_ERR_INVALID, "t5_set_linear_bnb4: quant_type must be 1 (fp4) or 2 (nf4)");
  const int64_t n = (int64_t)out_features * in_features;
  if (blocksize <= 0 || (blocksize & (blocksize - 1)) || n % blocksize || n % 2) return fail(FMI_ERR_UNSUPPORTED, "t5_set_linear_bnb4: blocksize must be a power of two dividing the weight");
  if (n >= (1ll << 31)) return fail(FMI_ERR_UNSUPPORTED, "t5_set_linear_bnb4: linear too large");
  Dest d;
  std::string wname;
  FMI_TRY(t5_linear_dest(m, "t5_set_linear_bnb4", prefix, out_features, in_features, &d, &wname));
  const int rc = with_staged_pair(packed, (size_t)n / 2, absmax, (size_t)(n / blocksize) * sizeof(float), [&](void* dq, void* da) {
    return dequant_to_bf16(quant_type, blocksize, dq, (const float*)da, 0.f, in_features, n, d.ptr, nullptr);
  });
  if (rc == FMI_ERR_HIP) return fail(FMI_ERR_HIP, std::string("t5_set_linear_bnb4: ") + fmi_last_error());
  if (rc) return rc;
  m->r.missing.erase(wname);
  return FMI_OK;
}
extern "C" int fmi_t5_set_linear_int8(fmi_t5* m, const char* prefix, const int8_t* weight, const float* scb, int out_features, int in_features) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m || !prefix || !weight || !scb) return fail(FMI_ERR_INVALID, "t5_set_linear_int8: null argument");
  const int64_t n = (int64_t)out_features * in_features;
  Dest d;
  std::string wname;
  FMI_TRY(t5_linear_dest(m, "t5_set_linear_int8", prefix, out_features, in_features, &d, &wname));
  const int rc = with_staged_pair(weight, (size_t)n, scb, (size_t)out_features * sizeof(float), [&](void* dw, void* ds) {
    return dequant_to_bf16(PS_INT8, 0, dw, (const float*)ds, 0.f, in_features, n, d.ptr, nullptr);
  });
  if (rc == FMI_ERR_HIP) return fail(FMI_ERR_HIP, std::string("t5_set_linear_int8: ") + fmi_last_error());
  if (rc) return rc;
  m->r.missing.erase(wname);
  return FMI_OK;
}
extern "C" int fmi_t5_missing_count(const fmi_t5* m) { return enc_missing_count(m); }
extern "C" const char* fmi_t5_missing_name(fmi_t5* m, int i) { return enc_missing_name(m, i); }
extern "C" size_t fmi_t5_size_in_bytes(const fmi_t5* m) { return enc_size_in_bytes(m); }

extern "C" int fmi_t5_forward(fmi_t5* m, const int32_t* input_ids, int B, int T, void* out, fmi_dtype out_dtype, void* stream) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m || !input_ids || !out) return fail(FMI_ERR_INVALID, "t5_forward: null argument");
  if (B <= 0 || T <= 0) return fail(FMI_ERR_INVALID, "t5_forward: empty batch");
  FMI_TRY(m->r.missing.ready("t5_forward"));
  hipStream_t s = (hipStream_t)stream;
  const fmi_t5_config& c = m->cfg;
  const int D = c.d_model, H = c.num_heads, I = H * 64, F = c.d_ff, rows = B * T;
  const bool gated = c.feed_forward_act != FMI_T5_RELU;
  const int FW = gated ? 2 * F : F;
  Carve carve;
  const size_t o_x = carve((size_t)rows * D * 4), o_n = carve((size_t)rows * D * 2), o_qkv = carve((size_t)rows * 3 * I * 2), o_a = carve((size_t)rows * I * 2);
  const size_t o_h = carve((size_t)rows * FW * 2), o_g = carve((size_t)rows * F * 2), o_bias = carve((size_t)H * T * T * 4), o_ones = carve((size_t)D * 4);
  const size_t o_ids = carve((size_t)rows * 4), o_bkt = carve((size_t)(2 * T - 1) * 4), o_err = carve(4), o_of = carve((size_t)rows * D * 4);
  FMI_TRY(m->ws.reserve(carve.total));
  const Workspace& ws = m->ws;
  float *x = ws.at<float>(o_x), *bias = ws.at<float>(o_bias), *ones = ws.at<float>(o_ones), *of = ws.at<float>(o_of);
  bf16_t *n = ws.at<bf16_t>(o_n), *qkv = ws.at<bf16_t>(o_qkv), *a = ws.at<bf16_t>(o_a), *h = ws.at<bf16_t>(o_h), *g = ws.at<bf16_t>(o_g);
  int32_t* ids = ws.at<int32_t>(o_ids);
  int *bkt = ws.at<int>(o_bkt), *err = ws.at<int>(o_err);

  FMI_HIP_TRY(hipMemcpyAsync(ids, input_ids, (size_t)rows * 4, hipMemcpyDefault, s));
  FMI_HIP_TRY(hipMemsetAsync(err, 0, 4, s));
  m->bucket_host.resize(2 * T - 1);
  for (int rel = -(T - 1); rel <= T - 1; ++rel) m->bucket_host[rel + T - 1] = t5_bucket_of(rel, c.relative_attention_num_buckets, c.relative_attention_max_distance);
  FMI_HIP_TRY(hipMemcpyAsync(bkt, m->bucket_host.data(), (size_t)(2 * T - 1) * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(fill_f32_kernel, dim3(16), dim3(256), 0, s, ones, D, 1.0f);
  hipLaunchKernelGGL(t5_bias_kernel, dim3(T, H), dim3(256), 0, s, m->rel, bkt, H, T, bias);
  hipLaunchKernelGGL(embed_gather_kernel, dim3(rows), dim3(256), 0, s, ids, m->shared, (const bf16_t*)nullptr, T, D, c.vocab_size, x, err);
  FMI_LAUNCH_CHECK();
  const int nb = (rows + 3) / 4;
  for (int l = 0; l < c.num_layers; ++l) {
    const fmi_t5::Layer& L = m->layers[l];
    // T5LayerSelfAttention (t5/mod.rs:412-424)
    hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3(nb), dim3(256), 0, s, x, L.ln0, c.layer_norm_epsilon, rows, D, n, (float*)nullptr);
    GemmProblem p = lin(n, D, L.qkv, nullptr, qkv, 3 * I, rows, 3 * I, D, EPI_STORE_BF16);
    FMI_TRY(launch_gemm(&p, 1, s));
    FMI_TRY(enc_attention(qkv, bias, B, T, H, 1.0f, 0, a, s));  // no 1/sqrt(d) in T5 (:317)
    p = lin(a, I, L.o, nullptr, x, D, rows, D, I, EPI_RESID_GATE_F32);
    p.gate = ones;
    FMI_TRY(launch_gemm(&p, 1, s));
    // T5LayerFF (:222-231)
    hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3(nb), dim3(256), 0, s, x, L.ln1, c.layer_norm_epsilon, rows, D, n, (float*)nullptr);
    p = lin(n, D, L.wi, nullptr, h, FW, rows, FW, D, EPI_STORE_BF16);
    FMI_TRY(launch_gemm(&p, 1, s));
    const int act = c.feed_forward_act == FMI_T5_RELU ? 0 : (c.feed_forward_act == FMI_T5_GATED_GELU ? 1 : 2);
    hipLaunchKernelGGL(enc_act_kernel, dim3(1024), dim3(256), 0, s, h, rows, F, act, gated ? 1 : 0, g);
    p = lin(g, F, L.wo, nullptr, x, D, rows, D, F, EPI_RESID_GATE_F32);
    p.gate = ones;
    FMI_TRY(launch_gemm(&p, 1, s));
  }
  hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3(nb), dim3(256), 0, s, x, m->final_ln, c.layer_norm_epsilon, rows, D, n, of);
  FMI_LAUNCH_CHECK();
  FMI_TRY(write_out(of, n, out, out_dtype, (int64_t)rows * D, s));
  int herr = 0;
  FMI_HIP_TRY(hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, s));
  FMI_HIP_TRY(hipStreamSynchronize(s));
  if (herr) return fail(FMI_ERR_INVALID, "t5_forward: token id out of range [0, vocab_size)");
  return FMI_OK;
}

// ============================================================================================= CLIP
struct fmi_clip : EncoderHandle {
  fmi_clip_config cfg;
  bf16_t *tok = nullptr, *pos = nullptr, *fw = nullptr, *fb = nullptr;
  std::vector<EncLayer> layers;
};

static void clip_layout(fmi_clip* m) {
  const fmi_clip_config& c = m->cfg;
  const int D = c.projection_dim, F = c.intermediate_size;
  Registry& r = m->r;
  const std::string tm = "text_model.";
  m->tok = r.take((size_t)c.vocab_size * D);
  r.reg(tm + "embeddings.token_embedding.weight", m->tok, c.vocab_size, D);
  m->pos = r.take((size_t)c.max_position_embeddings * D);
  r.reg(tm + "embeddings.position_embedding.weight", m->pos, c.max_position_embeddings, D);
  m->layers.resize(c.num_hidden_layers);
  for (int l = 0; l < c.num_hidden_layers; ++l) m->layers[l] = enc_layer_layout(r, tm + "encoder.layers." + std::to_string(l) + ".", D, c.num_attention_heads, F, 64);
  m->fw = r.take(D), m->fb = r.take(D);
  r.reg(tm + "final_layer_norm.weight", m->fw, D, 0), r.reg(tm + "final_layer_norm.bias", m->fb, D, 0);
}

extern "C" void fmi_clip_default_config(fmi_clip_config* c) {
  if (!c) return;
  // openai/clip-vit-large-patch14 text tower as shipped in FLUX.1's text_encoder/config.json
  c->vocab_size = 49408, c->projection_dim = 768, c->intermediate_size = 3072, c->max_position_embeddings = 77, c->num_hidden_layers = 12, c->num_attention_heads = 12;
}
extern "C" int fmi_clip_create(const fmi_clip_config* cfg, fmi_clip** out) {
  if (!cfg || !out) return fail(FMI_ERR_INVALID, "clip_create: null argument");
  if (cfg->num_attention_heads <= 0 || cfg->projection_dim != cfg->num_attention_heads * 64)
    return fail(FMI_ERR_UNSUPPORTED, "clip_create: head dim (projection_dim / num_attention_heads) must be 64");
  if (cfg->projection_dim % 64 || cfg->intermediate_size % 64 || cfg->intermediate_size <= 0 || cfg->num_hidden_layers <= 0 || cfg->vocab_size <= 0 || cfg->max_position_embeddings <= 0)
    return fail(FMI_ERR_INVALID, "clip_create: widths must be positive multiples of 64");
  std::unique_ptr<fmi_clip> m(new fmi_clip());
  m->cfg = *cfg;
  FMI_TRY(create_arena("clip_create", m.get(), clip_layout, /*zero=*/false));
  *out = m.release();
  return FMI_OK;
}
extern "C" void fmi_clip_destroy(fmi_clip* m) { delete m; }  // (the weight arena and the workspace are DeviceBuffers)
extern "C" int fmi_clip_set_tensor(fmi_clip* m, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  return enc_set_tensor(m, "clip_set_tensor", name, data, dtype, shape, rank);
}
extern "C" int fmi_clip_missing_count(const fmi_clip* m) { return enc_missing_count(m); }
extern "C" const char* fmi_clip_missing_name(fmi_clip* m, int i) { return enc_missing_name(m, i); }
extern "C" size_t fmi_clip_size_in_bytes(const fmi_clip* m) { return enc_size_in_bytes(m); }

extern "C" int fmi_clip_forward(fmi_clip* m, const int32_t* input_ids, int B, int T, void* pooled_out, fmi_dtype pooled_dtype, float* hidden_out, void* stream) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m || !input_ids || !pooled_out) return fail(FMI_ERR_INVALID, "clip_forward: null argument");
  if (B <= 0 || T <= 0) return fail(FMI_ERR_INVALID, "clip_forward: empty batch");
  const fmi_clip_config& c = m->cfg;
  if (T > c.max_position_embeddings) return fail(FMI_ERR_INVALID, "clip_forward: sequence longer than max_position_embeddings");
  FMI_TRY(m->r.missing.ready("clip_forward"));
  hipStream_t s = (hipStream_t)stream;
  const int D = c.projection_dim, H = c.num_attention_heads, F = c.intermediate_size, rows = B * T;
  Carve carve;
  const size_t o_x = carve((size_t)rows * D * 4), o_n = carve((size_t)rows * D * 2), o_qkv = carve((size_t)rows * 3 * D * 2), o_a = carve((size_t)rows * D * 2);
  const size_t o_h = carve((size_t)rows * F * 2), o_g = carve((size_t)rows * F * 2), o_ones = carve((size_t)D * 4), o_ids = carve((size_t)rows * 4), o_err = carve(4);
  const size_t o_hf = carve((size_t)rows * D * 4), o_pf = carve((size_t)B * D * 4), o_pb = carve((size_t)B * D * 2);
  FMI_TRY(m->ws.reserve(carve.total));
  const Workspace& ws = m->ws;
  float *x = ws.at<float>(o_x), *ones = ws.at<float>(o_ones), *hf = ws.at<float>(o_hf), *pf = ws.at<float>(o_pf);
  bf16_t* pb = ws.at<bf16_t>(o_pb);
  int32_t* ids = ws.at<int32_t>(o_ids);
  int* err = ws.at<int>(o_err);
  const EncLayerBuffers lw{x, ws.at<bf16_t>(o_n), ws.at<bf16_t>(o_qkv), ws.at<bf16_t>(o_a), ws.at<bf16_t>(o_h), ws.at<bf16_t>(o_g), ones};

  FMI_HIP_TRY(hipMemcpyAsync(ids, input_ids, (size_t)rows * 4, hipMemcpyDefault, s));
  FMI_HIP_TRY(hipMemsetAsync(err, 0, 4, s));
  hipLaunchKernelGGL(fill_f32_kernel, dim3(16), dim3(256), 0, s, ones, D, 1.0f);
  hipLaunchKernelGGL(embed_gather_kernel, dim3(rows), dim3(256), 0, s, ids, m->tok, m->pos, T, D, c.vocab_size, x, err);
  FMI_LAUNCH_CHECK();
  const int nb = (rows + 3) / 4;
  FMI_TRY(enc_layers(m->layers, lw, rows, D, D, F, CLIP_LN_EPS, ACT_QUICK_GELU, s, clip_attention(B, T, H, /*causal=*/1, s)));  // ClipEncoder::forward (clip/text.rs:273-291)
  hipLaunchKernelGGL(layernorm_affine_kernel, dim3(nb), dim3(256), 0, s, x, m->fw, m->fb, CLIP_LN_EPS, rows, D, (bf16_t*)nullptr, hf);
  hipLaunchKernelGGL(clip_pool_kernel, dim3(B), dim3(256), 0, s, hf, ids, T, D, pf);
  FMI_LAUNCH_CHECK();
  if (pooled_dtype == FMI_BF16) FMI_TRY(launch_cast_to_bf16(pf, FMI_F32, pb, (int64_t)B * D, s));
  FMI_TRY(write_out(pf, pb, pooled_out, pooled_dtype, (int64_t)B * D, s));
  if (hidden_out) FMI_HIP_TRY(hipMemcpyAsync(hidden_out, hf, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, s));
  int herr = 0;
  FMI_HIP_TRY(hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, s));
  FMI_HIP_TRY(hipStreamSynchronize(s));
  if (herr) return fail(FMI_ERR_INVALID, "clip_forward: token id out of range [0, vocab_size)");
  return FMI_OK;
}
