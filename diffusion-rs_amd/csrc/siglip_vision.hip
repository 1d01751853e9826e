// siglip_vision.hip — FLUX.1 Redux: image variation from a picture.
//   fmi_siglip_vision_*  == HuggingFace's SiglipVisionModel.last_hidden_state (modeling_siglip.py): biased patch embedding + positions (no class token, no
//                           pre-LayerNorm), the SigLIP encoder layers (tanh-GELU, eps from the config), post_layernorm of every row; the pooling head is not run
//   fmi_redux_*          == diffusers' ReduxImageEncoder: redux_down(silu(redux_up(h))), times the request's scale
// The picture is prepared by clip_vision.hip's fmi_resize_bicubic_u8 + fmi_clip_preprocess_u8 (a direct S x S resize crops nothing).  Every Linear goes through
// launch_gemm, and the attention — 729 keys at head dim 72 for the so400m tower — through the transformer's MFMA attention at d = 128: the heads are zero-padded
// in the weights (encoder_common.h: siglip_layers), so no activation is padded per call.
#include <algorithm>
#include <cmath>

#include "encoder_common.h"

namespace fmi {
namespace {

// pixel_values (B, 3, S, S) f32 -> the patch GEMM's operand (B * G * G, Kpad) bf16, G = S / P rounded down (the pixels past G P are not read): row (b, gy, gx) holds its patch in (c, py, px) order — the order
// of patch_embedding.weight (D, 3, P, P) flattened — and zeros in the columns [3 P^2, Kpad)
__global__ __launch_bounds__(256) void siglip_patchify_kernel(const float* __restrict__ pix, int S, int P, int Kpad, bf16_t* __restrict__ out, int64_t n) {
  const int G = S / P, K = 3 * P * P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int col = (int)(i % Kpad);
    const int64_t row = i / Kpad;
    float v = 0.f;
    if (col < K) {
      const int px = col % P, py = (col / P) % P, c = col / (P * P);
      const int gx = (int)(row % G), gy = (int)((row / G) % G);
      const int64_t b = row / ((int64_t)G * G);
      v = pix[((b * 3 + c) * S + gy * P + py) * S + gx * P + px];
    }
    out[i] = f32_to_bf16(v);
  }
}

// SiglipVisionEmbeddings: x[b, t] += position_embedding[t], in place on the f32 stream (the patch GEMM has written patch + conv bias there).  x: (B, Np, D)
__global__ __launch_bounds__(256) void siglip_embed_kernel(float* __restrict__ x, const bf16_t* __restrict__ pos, int64_t per_image, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] += bf16_to_f32(pos[i % per_image]);
}

// out = scale * in: the embedder's result leaves as f32 or bf16 (one multiply in f32, then one rounding)
__global__ __launch_bounds__(256) void redux_scale_kernel(const float* __restrict__ in, float scale, float* __restrict__ out_f32, bf16_t* __restrict__ out_bf, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = __fmul_rn(scale, in[i]);
    if (out_f32) out_f32[i] = v;
    else out_bf[i] = f32_to_bf16(v);
  }
}

dim3 flat_grid(int64_t n) { return dim3((unsigned)std::min<int64_t>(cdiv64(n, 256), 4096)); }

}  // namespace
}  // namespace fmi

using namespace fmi;

// ====================================================================================== SigLIP vision tower
struct fmi_siglip_vision {
  fmi_siglip_vision_config cfg;
  int device = current_device();
  Registry r;
  Workspace ws;
  int Np = 0, K = 0, Kpad = 0;  // patches per image, 3 P^2, and the patch GEMM's K
  bf16_t *patch = nullptr, *patchb = nullptr, *pos = nullptr, *postw = nullptr, *postb = nullptr;
  std::vector<SiglipLayer> layers;
};

static void siglip_vision_layout(fmi_siglip_vision* m) {
  const fmi_siglip_vision_config& c = m->cfg;
  const int D = c.hidden_size, P = c.patch_size;
  Registry& r = m->r;
  r.used = 0;
  r.names.clear();
  r.missing.names.clear();
  const std::string vm = "vision_model.";
  m->patch = r.take((size_t)D * m->Kpad);  // rows of Kpad, zero behind the 3 P^2 columns of the tensor
  r.reg_padded4(vm + "embeddings.patch_embedding.weight", m->patch, D, 3, P, P, m->Kpad);
  m->patchb = r.take(D);
  r.reg(vm + "embeddings.patch_embedding.bias", m->patchb, D, 0);
  m->pos = r.take((size_t)m->Np * D);
  r.reg(vm + "embeddings.position_embedding.weight", m->pos, m->Np, D);
  m->layers.resize(c.num_hidden_layers);
  for (int l = 0; l < c.num_hidden_layers; ++l)
    siglip_layer_layout(r, vm + "encoder.layers." + std::to_string(l) + ".", D, c.num_attention_heads, c.intermediate_size, m->layers[l]);
  m->postw = r.take(D), m->postb = r.take(D);
  r.reg(vm + "post_layernorm.weight", m->postw, D, 0), r.reg(vm + "post_layernorm.bias", m->postb, D, 0);
}

// the workspace of a batch of B pictures: offsets into one block
struct SiglipCarve {
  size_t x, n, qkv, qh, kh, vt, a, h, g, ones, pa, total;
};
static SiglipCarve siglip_carve(const fmi_siglip_vision* m, int B) {
  const fmi_siglip_vision_config& c = m->cfg;
  const size_t rows = (size_t)B * m->Np, D = c.hidden_size, HP = (size_t)c.num_attention_heads * 128, Fp = align_up(c.intermediate_size, 64);
  const size_t Lp = align_up(m->Np, 64);
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off = align_up(off + bytes, 256);
    return o;
  };
  SiglipCarve k;
  k.x = carve(rows * D * 4), k.n = carve(rows * D * 2), k.qkv = carve(rows * 3 * HP * 2), k.qh = carve(rows * HP * 2), k.kh = carve(rows * HP * 2);
  k.vt = carve((size_t)B * HP * Lp * 2), k.a = carve(rows * HP * 2), k.h = carve(rows * Fp * 2), k.g = carve(rows * Fp * 2), k.ones = carve(D * 4);
  k.pa = carve(rows * m->Kpad * 2);
  k.total = off;
  return k;
}

extern "C" void fmi_siglip_vision_default_config(fmi_siglip_vision_config* c) {
  if (!c) return;
  // google/siglip-so400m-patch14-384's vision tower (the image encoder of FLUX.1 Redux)
  c->image_size = 384, c->patch_size = 14, c->hidden_size = 1152, c->intermediate_size = 4304, c->num_hidden_layers = 27, c->num_attention_heads = 16;
  c->layer_norm_eps = 1e-6f;
}
extern "C" int fmi_siglip_vision_create(const fmi_siglip_vision_config* cfg, fmi_siglip_vision** out) {
  if (!cfg || !out) return fail(FMI_ERR_INVALID, "siglip_vision_create: null argument");
  if (cfg->hidden_size <= 0 || cfg->hidden_size % 64 || cfg->hidden_size > 16384)
    return fail(FMI_ERR_INVALID, "siglip_vision_create: hidden_size must be a positive multiple of 64");
  if (cfg->num_attention_heads <= 0 || cfg->num_attention_heads > 1024 || cfg->hidden_size % cfg->num_attention_heads)
    return fail(FMI_ERR_INVALID, "siglip_vision_create: hidden_size must be a multiple of num_attention_heads");
  const int hd = cfg->hidden_size / cfg->num_attention_heads;
  if (hd % 8 || hd > 128)
    return fail(FMI_ERR_UNSUPPORTED, "siglip_vision_create: head dim (hidden_size / num_attention_heads) must be a multiple of 8 up to 128, got " + std::to_string(hd));
  if (cfg->intermediate_size <= 0 || cfg->intermediate_size > (1 << 20))  // (any size: the MLP runs at the next multiple of 64, zero-padded in the weights)
    return fail(FMI_ERR_INVALID, "siglip_vision_create: intermediate_size must be positive (at most 2^20)");
  if (cfg->num_hidden_layers <= 0 || cfg->num_hidden_layers > 4096) return fail(FMI_ERR_INVALID, "siglip_vision_create: num_hidden_layers must be positive");
  // (the convolution has no padding: G = image_size / patch_size patches per side, rounded down — so400m-patch14-384 has 27 and never reads its last 6 rows and columns)
  if (cfg->patch_size <= 0 || cfg->patch_size > 256 || cfg->image_size < cfg->patch_size || cfg->image_size > 16384)
    return fail(FMI_ERR_INVALID, "siglip_vision_create: patch_size must be in 1 .. 256 and image_size in patch_size .. 16384");
  if (!(cfg->layer_norm_eps > 0.f) || !std::isfinite(cfg->layer_norm_eps)) return fail(FMI_ERR_INVALID, "siglip_vision_create: layer_norm_eps must be positive and finite");
  const int64_t G = cfg->image_size / cfg->patch_size;
  if (G * G > (1 << 16)) return fail(FMI_ERR_UNSUPPORTED, "siglip_vision_create: more than 65536 patches per image");
  fmi_siglip_vision* m = new fmi_siglip_vision();
  m->cfg = *cfg;
  m->Np = (int)(G * G), m->K = 3 * cfg->patch_size * cfg->patch_size, m->Kpad = (int)align_up(m->K, 64);
  siglip_vision_layout(m);  // pass 0: size
  m->r.bytes = align_up(m->r.used, 256);
  hipError_t e = m->r.arena.alloc(m->r.bytes);
  if (e == hipSuccess) e = hipMemset(m->r.arena.ptr, 0, m->r.bytes);  // the pads that no tensor writes (fc1's rows [F, Fp) and its bias) are zero from here on
  if (e != hipSuccess) {
    delete m;
    return fail(FMI_ERR_HIP, std::string("siglip_vision_create: hipMalloc of the weight arena: ") + hipGetErrorString(e));
  }
  siglip_vision_layout(m);  // pass 1: pointers
  *out = m;
  return FMI_OK;
}
extern "C" void fmi_siglip_vision_destroy(fmi_siglip_vision* m) {
  delete m;  // (the weight arena and the workspace are DeviceBuffers)
}
extern "C" int fmi_siglip_vision_set_tensor(fmi_siglip_vision* m, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m) return fail(FMI_ERR_INVALID, "siglip_vision_set_tensor: null model");
  return m->r.set("siglip_vision_set_tensor", name, data, dtype, shape, rank);
}
extern "C" int fmi_siglip_vision_missing_count(const fmi_siglip_vision* m) { return m ? m->r.missing.count() : 0; }
extern "C" const char* fmi_siglip_vision_missing_name(fmi_siglip_vision* m, int i) { return m ? m->r.missing.name(i) : nullptr; }
extern "C" size_t fmi_siglip_vision_size_in_bytes(const fmi_siglip_vision* m) { return m ? m->r.bytes + m->ws.base.bytes() : 0; }

static int siglip_check_batch(const fmi_siglip_vision* m, const char* who, int B) {
  if (B <= 0) return fail(FMI_ERR_INVALID, std::string(who) + ": empty batch");
  if ((int64_t)B * m->Np > (1 << 20)) return fail(FMI_ERR_INVALID, std::string(who) + ": batch too large");
  return FMI_OK;
}

extern "C" int fmi_siglip_vision_poison_workspace(fmi_siglip_vision* m, int B, void* stream) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m) return fail(FMI_ERR_INVALID, "siglip_vision_poison_workspace: null model");
  FMI_TRY(siglip_check_batch(m, "siglip_vision_poison_workspace", B));
  FMI_TRY(m->ws.reserve(siglip_carve(m, B).total));
  FMI_HIP_TRY(hipMemsetAsync(m->ws.base.ptr, 0xff, m->ws.base.bytes(), (hipStream_t)stream));  // 0xffff / 0xffffffff: a NaN in bf16 and in f32
  FMI_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return FMI_OK;
}

extern "C" int fmi_siglip_vision_forward(fmi_siglip_vision* m, const float* pixel_values, int B, void* hidden_out, fmi_dtype dtype, void* stream) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m || !pixel_values || !hidden_out) return fail(FMI_ERR_INVALID, "siglip_vision_forward: null argument");
  if (dtype != FMI_F32 && dtype != FMI_BF16) return fail(FMI_ERR_INVALID, "siglip_vision_forward: hidden dtype must be F32 or BF16");
  FMI_TRY(siglip_check_batch(m, "siglip_vision_forward", B));
  FMI_TRY(m->r.missing.ready("siglip_vision_forward"));
  hipStream_t s = (hipStream_t)stream;
  const fmi_siglip_vision_config& c = m->cfg;
  const int D = c.hidden_size, H = c.num_attention_heads, Np = m->Np, Kpad = m->Kpad, rows = B * Np, Lp = (int)align_up(Np, 64);
  const SiglipCarve k = siglip_carve(m, B);
  FMI_TRY(m->ws.reserve(k.total));
  char* w = m->ws.base.as<char>();
  float* x = (float*)(w + k.x);
  float* ones = (float*)(w + k.ones);
  bf16_t* pa = (bf16_t*)(w + k.pa);
  bf16_t* vt = (bf16_t*)(w + k.vt);

  hipLaunchKernelGGL(fill_f32_kernel, dim3(16), dim3(256), 0, s, ones, D, 1.0f);
  // SiglipVisionEmbeddings: the stride-P convolution as one GEMM over patch rows, its bias in the epilogue, straight into the f32 stream; then the positions
  const int64_t npa = (int64_t)rows * Kpad;
  hipLaunchKernelGGL(siglip_patchify_kernel, flat_grid(npa), dim3(256), 0, s, pixel_values, c.image_size, c.patch_size, Kpad, pa, npa);
  FMI_LAUNCH_CHECK();
  GemmProblem p = lin(pa, Kpad, m->patch, m->patchb, x, D, rows, D, Kpad, EPI_STORE_F32);
  FMI_TRY(launch_gemm(&p, 1, s));
  const int64_t nx = (int64_t)rows * D;
  hipLaunchKernelGGL(siglip_embed_kernel, flat_grid(nx), dim3(256), 0, s, x, m->pos, (int64_t)Np * D, nx);
  FMI_LAUNCH_CHECK();
  // V^T's key tail [Np, Lp): zero once — the layers' transposes write the keys below Np only, and the attention multiplies the tail's P = 0 with it
  FMI_TRY(launch_vt_zero_pad(vt, B * H, Np, Lp, s));
  FMI_TRY(siglip_layers(m->layers,
                        SiglipLayerBuffers{x, (bf16_t*)(w + k.n), (bf16_t*)(w + k.qkv), (bf16_t*)(w + k.qh), (bf16_t*)(w + k.kh), vt, (bf16_t*)(w + k.a), (bf16_t*)(w + k.h),
                                           (bf16_t*)(w + k.g), ones},
                        B, Np, D, H, c.intermediate_size, c.layer_norm_eps, s));
  // post_layernorm of every row: last_hidden_state
  hipLaunchKernelGGL(layernorm_affine_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, m->postw, m->postb, c.layer_norm_eps, rows, D,
                     dtype == FMI_BF16 ? (bf16_t*)hidden_out : (bf16_t*)nullptr, dtype == FMI_F32 ? (float*)hidden_out : (float*)nullptr);
  FMI_LAUNCH_CHECK();
  FMI_HIP_TRY(hipStreamSynchronize(s));  // (the workspace is the handle's: the next call may regrow it)
  return FMI_OK;
}

// ====================================================================================== Redux embedder
struct fmi_redux {
  int D = 0, J = 0;  // redux_dim (the tower's hidden_size), txt_in_features (the transformer's joint_attention_dim)
  int device = current_device();
  Registry r;
  Workspace ws;
  bf16_t *up = nullptr, *upb = nullptr, *down = nullptr, *downb = nullptr;
};

static void redux_layout(fmi_redux* m) {
  Registry& r = m->r;
  r.used = 0;
  r.names.clear();
  r.missing.names.clear();
  const int D = m->D, J = m->J;
  m->up = r.take((size_t)3 * J * D), m->upb = r.take((size_t)3 * J);
  r.reg("redux_up.weight", m->up, 3 * J, D), r.reg("redux_up.bias", m->upb, 3 * J, 0);
  m->down = r.take((size_t)J * 3 * J), m->downb = r.take(J);
  r.reg("redux_down.weight", m->down, J, 3 * J), r.reg("redux_down.bias", m->downb, J, 0);
}

extern "C" int fmi_redux_create(int redux_dim, int txt_dim, fmi_redux** out) {
  if (!out) return fail(FMI_ERR_INVALID, "redux_create: null argument");
  if (redux_dim <= 0 || redux_dim % 64 || txt_dim <= 0 || txt_dim % 64 || redux_dim > 16384 || txt_dim > 16384)
    return fail(FMI_ERR_INVALID, "redux_create: redux_dim and txt_dim must be positive multiples of 64, got " + std::to_string(redux_dim) + ", " + std::to_string(txt_dim));
  fmi_redux* m = new fmi_redux();
  m->D = redux_dim, m->J = txt_dim;
  redux_layout(m);
  m->r.bytes = align_up(m->r.used, 256);
  const hipError_t e = m->r.arena.alloc(m->r.bytes);
  if (e != hipSuccess) {
    delete m;
    return fail(FMI_ERR_HIP, std::string("redux_create: hipMalloc of the weight arena: ") + hipGetErrorString(e));
  }
  redux_layout(m);
  *out = m;
  return FMI_OK;
}
extern "C" void fmi_redux_destroy(fmi_redux* m) { delete m; }
extern "C" int fmi_redux_set_tensor(fmi_redux* m, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m) return fail(FMI_ERR_INVALID, "redux_set_tensor: null model");
  return m->r.set("redux_set_tensor", name, data, dtype, shape, rank);
}
extern "C" int fmi_redux_missing_count(const fmi_redux* m) { return m ? m->r.missing.count() : 0; }
extern "C" const char* fmi_redux_missing_name(fmi_redux* m, int i) { return m ? m->r.missing.name(i) : nullptr; }
extern "C" size_t fmi_redux_size_in_bytes(const fmi_redux* m) { return m ? m->r.bytes + m->ws.base.bytes() : 0; }

extern "C" int fmi_redux_forward(fmi_redux* m, const float* hidden, int rows, float scale, void* out, fmi_dtype dtype, void* stream) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m || !hidden || !out) return fail(FMI_ERR_INVALID, "redux_forward: null argument");
  if (rows <= 0 || rows > (1 << 20)) return fail(FMI_ERR_INVALID, "redux_forward: rows must be in 1 .. 2^20");
  if (dtype != FMI_F32 && dtype != FMI_BF16) return fail(FMI_ERR_INVALID, "redux_forward: out dtype must be F32 or BF16");
  if (!std::isfinite(scale)) return fail(FMI_ERR_INVALID, "redux_forward: scale must be finite");
  FMI_TRY(m->r.missing.ready("redux_forward"));
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D, J = m->J;
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off = align_up(off + bytes, 256);
    return o;
  };
  const size_t o_in = carve((size_t)rows * D * 2), o_u = carve((size_t)rows * 3 * J * 2), o_a = carve((size_t)rows * 3 * J * 2), o_f = carve((size_t)rows * J * 4);
  FMI_TRY(m->ws.reserve(off));
  char* w = m->ws.base.as<char>();
  bf16_t *in = (bf16_t*)(w + o_in), *u = (bf16_t*)(w + o_u), *a = (bf16_t*)(w + o_a);
  float* f = (float*)(w + o_f);
  FMI_TRY(launch_cast_to_bf16(hidden, FMI_F32, in, (int64_t)rows * D, s));
  GemmProblem p = lin(in, D, m->up, m->upb, u, 3 * J, rows, 3 * J, D, EPI_STORE_BF16);
  FMI_TRY(launch_gemm(&p, 1, s));
  hipLaunchKernelGGL(enc_act_kernel, dim3(256), dim3(256), 0, s, u, rows, 3 * J, 2, 0, a);  // SiLU
  p = lin(a, 3 * J, m->down, m->downb, f, J, rows, J, 3 * J, EPI_STORE_F32);
  FMI_TRY(launch_gemm(&p, 1, s));
  // scale * (W x + b): the GEMM's alpha would scale the product alone, so the scale is one more pass, which also writes the result in its dtype
  const int64_t n = (int64_t)rows * J;
  hipLaunchKernelGGL(redux_scale_kernel, flat_grid(n), dim3(256), 0, s, f, scale, dtype == FMI_F32 ? (float*)out : (float*)nullptr,
                     dtype == FMI_BF16 ? (bf16_t*)out : (bf16_t*)nullptr, n);
  FMI_LAUNCH_CHECK();
  FMI_HIP_TRY(hipStreamSynchronize(s));  // (the workspace is the handle's: the next call may regrow it)
  return FMI_OK;
}
