// clip_vision.hip — the CLIP vision encoder in front of the IP-Adapter: a picture goes in as a picture.
//   fmi_resize_bicubic_u8    == PIL's Image.resize(BICUBIC) on u8 (what CLIP's image processor resizes with)
//   fmi_clip_preprocess_u8   == centre crop + (v / 255 - mean) / std
//   fmi_clip_vision_*        == HuggingFace's CLIPVisionModelWithProjection (modeling_clip.py): patch embedding, class token + positions, pre-LayerNorm,
//                               the CLIP encoder layers of the text tower without the causal mask, post-LayerNorm of the class row, visual_projection
// It runs once per request next to a 3 s image: the new kernels are single-pass and bandwidth-bound, every Linear goes through launch_gemm (the patch
// embedding as a GEMM over patch rows, K = 3 P^2 zero-padded to the GEMM's multiple of 64), and the layers are encoder_common.h's, shared with fmi_clip_forward.
#include <algorithm>
#include <cmath>

#include "encoder_common.h"

namespace fmi {
namespace {

// Keys' cubic, a = -0.5 (PIL's bicubic_filter)
__device__ __forceinline__ float cubic_keys(float x) {
  const float a = -0.5f;
  x = fabsf(x);
  if (x < 1.0f) return ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
  if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * a;
  return 0.0f;
}

// One pass of PIL's separable resize along one axis of a u8 (rows, cols, 3) image: axis 1 (horizontal) in (h, n_in, 3) -> out (h, n_out, 3), axis 0
// (vertical) in (n_in, w, 3) -> out (n_out, w, 3).  `lines` is the size of the axis that stays.  One thread per output pixel computes its own window and
// weights (precompute_coeffs of PIL's Resample.c, in f32): scale = n_in / n_out, fs = max(scale, 1), support = 2 fs, centre = (o + 0.5) scale, the taps
// [lo, hi) = [max(0, int(centre - support + 0.5)), min(n_in, int(centre + support + 0.5))), w_j = k((j + lo - centre + 0.5) / fs) normalised to sum 1;
// the three channel sums run over the taps in ascending order, are rounded to nearest and clamped to [0, 255].  No atomics, nothing shared between threads: the
// result does not depend on the launch grid.
__global__ __launch_bounds__(256) void resize_axis_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int lines, int n_in, int n_out, int vertical) {
  const int64_t total = (int64_t)lines * n_out;
  const float scale = (float)n_in / (float)n_out;
  const float fs = scale < 1.0f ? 1.0f : scale;
  const float support = 2.0f * fs;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    // horizontal: t = line * n_out + o (the output's own order); vertical: t = o * lines + line (a wave reads and writes along a row)
    const int o = vertical ? (int)(t / lines) : (int)(t % n_out);
    const int line = vertical ? (int)(t % lines) : (int)(t / n_out);
    const float center = ((float)o + 0.5f) * scale;
    int lo = (int)(center - support + 0.5f);
    int hi = (int)(center + support + 0.5f);
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_in ? n_in : hi;
    float ws = 0.f;
    for (int j = lo; j < hi; ++j) ws += cubic_keys(((float)j - center + 0.5f) / fs);
    const int64_t stride = vertical ? (int64_t)lines * 3 : 3;
    const uint8_t* src = in + (vertical ? (int64_t)line * 3 : (int64_t)line * n_in * 3);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = lo; j < hi; ++j) {
      const float wj = cubic_keys(((float)j - center + 0.5f) / fs) / ws;
      const uint8_t* px = src + (int64_t)j * stride;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += wj * (float)px[c];
    }
    uint8_t* dst = out + (vertical ? ((int64_t)o * lines + line) * 3 : ((int64_t)line * n_out + o) * 3);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)fminf(fmaxf(rintf(acc[c]), 0.f), 255.f);
  }
}

// centre crop of a u8 (nh, nw, 3) image to S x S and CLIP's normalisation into f32 (3, S, S): three f32 operations per value, none contracted
__global__ __launch_bounds__(256) void clip_preprocess_u8_kernel(const uint8_t* __restrict__ in, int nw, int top, int left, int S, float m0, float m1, float m2, float s0,
                                                                 float s1, float s2, float* __restrict__ out) {
  const int n = 3 * S * S;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int x = i % S, y = (i / S) % S, c = i / (S * S);
    const float v = (float)in[((int64_t)(top + y) * nw + left + x) * 3 + c];
    out[i] = __fdiv_rn(__fsub_rn(__fdiv_rn(v, 255.0f), c == 0 ? m0 : c == 1 ? m1 : m2), c == 0 ? s0 : c == 1 ? s1 : s2);
  }
}

// pixel_values (B, 3, S, S) f32 -> the patch GEMM's operand (B * G * G, Kpad) bf16, G = S / P: row (b, gy, gx) holds its patch in (c, py, px) order —
// the order of patch_embedding.weight (D, 3, P, P) flattened — and zeros in the columns [3 P^2, Kpad)
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ pix, int S, int P, int Kpad, bf16_t* __restrict__ out, int64_t n) {
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

// CLIPVisionEmbeddings: x[b, 0] = class_embedding + pos[0], x[b, 1 + i] = patch[b, i] + pos[1 + i], in f32.  patch: (B * Np, D) f32, x: (B, 1 + Np, D)
__global__ __launch_bounds__(256) void vision_embed_kernel(const float* __restrict__ patch, const bf16_t* __restrict__ cls, const bf16_t* __restrict__ pos, int Np, int D,
                                                           float* __restrict__ x, int64_t n) {
  const int T = Np + 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D), t = (int)((i / D) % T);
    const int64_t b = i / ((int64_t)D * T);
    const float e = t == 0 ? bf16_to_f32(cls[d]) : patch[(b * Np + t - 1) * D + d];
    x[i] = e + bf16_to_f32(pos[(int64_t)t * D + d]);
  }
}

dim3 flat_grid(int64_t n) { return dim3((unsigned)std::min<int64_t>(cdiv64(n, 256), 4096)); }

}  // namespace
}  // namespace fmi

using namespace fmi;

extern "C" int fmi_resize_bicubic_u8(const uint8_t* in, int h, int w, uint8_t* out, int nh, int nw, void* stream) {
  if (!in || !out) return fail(FMI_ERR_INVALID, "resize_bicubic_u8: null argument");
  if (h <= 0 || w <= 0 || nh <= 0 || nw <= 0)
    return fail(FMI_ERR_INVALID, "resize_bicubic_u8: h, w, nh, nw must be positive, got " + std::to_string(h) + ", " + std::to_string(w) + ", " + std::to_string(nh) + ", " +
                                     std::to_string(nw));
  hipStream_t s = (hipStream_t)stream;
  if (nh == h && nw == w) {  // (PIL returns a copy)
    FMI_HIP_TRY(hipMemcpyAsync(out, in, (size_t)h * w * 3, hipMemcpyDeviceToDevice, s));
    return FMI_OK;
  }
  // horizontal first, then vertical (PIL's order); a pass whose size stays is skipped; the value between the passes is u8, rounded and clamped
  const uint8_t* src = in;
  OpScratch scratch(s);  // (the (h, nw, 3) image between the passes: the library's per-stream op scratch, held until both kernels are enqueued)
  if (nw != w) {
    uint8_t* dst = out;
    if (nh != h) {
      FMI_TRY(scratch.get((size_t)h * nw * 3));
      dst = static_cast<uint8_t*>(scratch.p);
    }
    hipLaunchKernelGGL(resize_axis_u8_kernel, flat_grid((int64_t)h * nw), dim3(256), 0, s, src, dst, h, w, nw, 0);
    FMI_LAUNCH_CHECK();
    src = dst;
  }
  if (nh != h) {
    hipLaunchKernelGGL(resize_axis_u8_kernel, flat_grid((int64_t)nh * nw), dim3(256), 0, s, src, out, nw, h, nh, 1);
    FMI_LAUNCH_CHECK();
  }
  return FMI_OK;
}

extern "C" int fmi_clip_preprocess_u8(const uint8_t* in, int nh, int nw, int S, const float* mean, const float* std_, float* out, void* stream) {
  if (!in || !out || !mean || !std_) return fail(FMI_ERR_INVALID, "clip_preprocess_u8: null argument");
  if (S <= 0) return fail(FMI_ERR_INVALID, "clip_preprocess_u8: S must be positive");
  if (nh < S || nw < S)
    return fail(FMI_ERR_INVALID, "clip_preprocess_u8: nh and nw must be at least S = " + std::to_string(S) + " (the centre crop never pads), got " + std::to_string(nh) + " x " +
                                     std::to_string(nw));
  for (int c = 0; c < 3; ++c)
    if (!(std_[c] > 0.f) || !std::isfinite(mean[c]) || !std::isfinite(std_[c])) return fail(FMI_ERR_INVALID, "clip_preprocess_u8: mean must be finite and std finite and positive");
  hipLaunchKernelGGL(clip_preprocess_u8_kernel, flat_grid((int64_t)3 * S * S), dim3(256), 0, (hipStream_t)stream, in, nw, (nh - S) / 2, (nw - S) / 2, S, mean[0], mean[1],
                     mean[2], std_[0], std_[1], std_[2], out);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

// ====================================================================================== CLIP vision tower
struct fmi_clip_vision {
  fmi_clip_vision_config cfg;
  int device = current_device();
  Registry r;
  Workspace ws;
  int Np = 0, K = 0, Kpad = 0;  // patches per image, 3 P^2, and the GEMM's K
  bf16_t *cls = nullptr, *patch = nullptr, *pos = nullptr, *prew = nullptr, *preb = nullptr, *postw = nullptr, *postb = nullptr, *proj = nullptr;
  std::vector<ClipLayer> layers;
};

static void clip_vision_layout(fmi_clip_vision* m) {
  const fmi_clip_vision_config& c = m->cfg;
  const int D = c.hidden_size, F = c.intermediate_size, P = c.patch_size;
  Registry& r = m->r;
  r.used = 0;
  r.names.clear();
  r.missing.names.clear();
  const std::string vm = "vision_model.";
  m->cls = r.take(D);
  r.reg(vm + "embeddings.class_embedding", m->cls, D, 0);
  m->patch = r.take((size_t)D * m->Kpad);  // rows of Kpad, zero behind the 3 P^2 columns of the tensor
  r.reg_padded4(vm + "embeddings.patch_embedding.weight", m->patch, D, 3, P, P, m->Kpad);
  m->pos = r.take((size_t)(m->Np + 1) * D);
  r.reg(vm + "embeddings.position_embedding.weight", m->pos, m->Np + 1, D);
  m->prew = r.take(D), m->preb = r.take(D);
  r.reg(vm + "pre_layrnorm.weight", m->prew, D, 0), r.reg(vm + "pre_layrnorm.bias", m->preb, D, 0);  // (HuggingFace's spelling)
  m->layers.resize(c.num_hidden_layers);
  for (int l = 0; l < c.num_hidden_layers; ++l) clip_layer_layout(r, vm + "encoder.layers." + std::to_string(l) + ".", D, F, m->layers[l]);
  m->postw = r.take(D), m->postb = r.take(D);
  r.reg(vm + "post_layernorm.weight", m->postw, D, 0), r.reg(vm + "post_layernorm.bias", m->postb, D, 0);
  m->proj = r.take((size_t)c.projection_dim * D);
  r.reg("visual_projection.weight", m->proj, c.projection_dim, D);
}

extern "C" void fmi_clip_vision_default_config(fmi_clip_vision_config* c) {
  if (!c) return;
  // openai/clip-vit-large-patch14's vision tower (the image encoder of the FLUX IP-Adapters)
  c->image_size = 224, c->patch_size = 14, c->hidden_size = 1024, c->intermediate_size = 4096, c->num_hidden_layers = 24, c->num_attention_heads = 16, c->projection_dim = 768;
}
extern "C" int fmi_clip_vision_create(const fmi_clip_vision_config* cfg, fmi_clip_vision** out) {
  if (!cfg || !out) return fail(FMI_ERR_INVALID, "clip_vision_create: null argument");
  if (cfg->num_attention_heads <= 0 || cfg->hidden_size != cfg->num_attention_heads * 64)
    return fail(FMI_ERR_UNSUPPORTED, "clip_vision_create: head dim (hidden_size / num_attention_heads) must be 64");
  if (cfg->hidden_size % 64 || cfg->intermediate_size % 64 || cfg->projection_dim % 64 || cfg->intermediate_size <= 0 || cfg->projection_dim <= 0 || cfg->num_hidden_layers <= 0)
    return fail(FMI_ERR_INVALID, "clip_vision_create: hidden_size, intermediate_size and projection_dim must be positive multiples of 64");
  if (cfg->patch_size <= 0 || cfg->image_size <= 0 || cfg->image_size % cfg->patch_size || cfg->image_size > 16384)
    return fail(FMI_ERR_INVALID, "clip_vision_create: image_size must be a positive multiple of patch_size");
  const int64_t G = cfg->image_size / cfg->patch_size, T = 1 + G * G;
  if (T > 64 * ENC_MAXKB)
    return fail(FMI_ERR_UNSUPPORTED, "clip_vision_create: " + std::to_string(T) + " tokens (1 + (image_size / patch_size)^2) are more than the encoder attention's " +
                                         std::to_string(64 * ENC_MAXKB));
  if (cfg->patch_size > 256) return fail(FMI_ERR_INVALID, "clip_vision_create: patch_size must be at most 256");
  fmi_clip_vision* m = new fmi_clip_vision();
  m->cfg = *cfg;
  m->Np = (int)(G * G), m->K = 3 * cfg->patch_size * cfg->patch_size, m->Kpad = (int)align_up(m->K, 64);
  clip_vision_layout(m);  // pass 0: size
  m->r.bytes = align_up(m->r.used, 256);
  hipError_t e = m->r.arena.alloc(m->r.bytes);
  if (e != hipSuccess) {
    delete m;
    return fail(FMI_ERR_HIP, std::string("clip_vision_create: hipMalloc of the weight arena: ") + hipGetErrorString(e));
  }
  clip_vision_layout(m);  // pass 1: pointers
  *out = m;
  return FMI_OK;
}
extern "C" void fmi_clip_vision_destroy(fmi_clip_vision* m) {
  delete m;  // (the weight arena and the workspace are DeviceBuffers)
}
extern "C" int fmi_clip_vision_set_tensor(fmi_clip_vision* m, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m) return fail(FMI_ERR_INVALID, "clip_vision_set_tensor: null model");
  return m->r.set("clip_vision_set_tensor", name, data, dtype, shape, rank);
}
extern "C" int fmi_clip_vision_missing_count(const fmi_clip_vision* m) { return m ? m->r.missing.count() : 0; }
extern "C" const char* fmi_clip_vision_missing_name(fmi_clip_vision* m, int i) { return m ? m->r.missing.name(i) : nullptr; }
extern "C" size_t fmi_clip_vision_size_in_bytes(const fmi_clip_vision* m) { return m ? m->r.bytes + m->ws.base.bytes() : 0; }

extern "C" int fmi_clip_vision_forward(fmi_clip_vision* m, const float* pixel_values, int B, void* image_embeds_out, fmi_dtype dtype, float* hidden_out, void* stream) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m || !pixel_values || !image_embeds_out) return fail(FMI_ERR_INVALID, "clip_vision_forward: null argument");
  if (B <= 0) return fail(FMI_ERR_INVALID, "clip_vision_forward: empty batch");
  if (dtype != FMI_F32 && dtype != FMI_BF16) return fail(FMI_ERR_INVALID, "clip_vision_forward: image_embeds dtype must be F32 or BF16");
  FMI_TRY(m->r.missing.ready("clip_vision_forward"));
  hipStream_t s = (hipStream_t)stream;
  const fmi_clip_vision_config& c = m->cfg;
  const int D = c.hidden_size, H = c.num_attention_heads, F = c.intermediate_size, E = c.projection_dim, Np = m->Np, T = Np + 1, Kpad = m->Kpad;
  if ((int64_t)B * T > (1 << 24)) return fail(FMI_ERR_INVALID, "clip_vision_forward: batch too large");
  const int rows = B * T, prows = B * Np;
  size_t off = 0;
  auto carve = [&](size_t bytes) {
    const size_t o = off;
    off = align_up(off + bytes, 256);
    return o;
  };
  const size_t o_x = carve((size_t)rows * D * 4), o_n = carve((size_t)rows * D * 2), o_qkv = carve((size_t)rows * 3 * D * 2), o_a = carve((size_t)rows * D * 2);
  const size_t o_h = carve((size_t)rows * F * 2), o_g = carve((size_t)rows * F * 2), o_ones = carve((size_t)D * 4);
  const size_t o_pa = carve((size_t)prows * Kpad * 2), o_pe = carve((size_t)prows * D * 4), o_e = carve((size_t)rows * D * 4);
  const size_t o_cf = carve((size_t)B * D * 4), o_cb = carve((size_t)B * D * 2), o_of = carve((size_t)B * E * 4), o_ob = carve((size_t)B * E * 2);
  FMI_TRY(m->ws.reserve(off));
  char* w = m->ws.base.as<char>();
  float* x = (float*)(w + o_x);
  bf16_t* n = (bf16_t*)(w + o_n);
  float* ones = (float*)(w + o_ones);
  bf16_t* pa = (bf16_t*)(w + o_pa);
  float* pe = (float*)(w + o_pe);
  float* e = (float*)(w + o_e);
  float* cf = (float*)(w + o_cf);
  bf16_t* cb = (bf16_t*)(w + o_cb);
  float* of = (float*)(w + o_of);
  bf16_t* ob = (bf16_t*)(w + o_ob);

  hipLaunchKernelGGL(fill_f32_kernel, dim3(16), dim3(256), 0, s, ones, D, 1.0f);
  // CLIPVisionEmbeddings: the stride-P convolution as one GEMM over patch rows, then class token + positions, then pre_layrnorm into the f32 stream
  const int64_t npa = (int64_t)prows * Kpad;
  hipLaunchKernelGGL(patchify_kernel, flat_grid(npa), dim3(256), 0, s, pixel_values, c.image_size, c.patch_size, Kpad, pa, npa);
  FMI_LAUNCH_CHECK();
  GemmProblem p = lin(pa, Kpad, m->patch, nullptr, pe, D, prows, D, Kpad, EPI_STORE_F32);
  FMI_TRY(launch_gemm(&p, 1, s));
  const int64_t ne = (int64_t)rows * D;
  hipLaunchKernelGGL(vision_embed_kernel, flat_grid(ne), dim3(256), 0, s, pe, m->cls, m->pos, Np, D, e, ne);
  hipLaunchKernelGGL(layernorm_affine_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, e, m->prew, m->preb, 1e-5f, rows, D, (bf16_t*)nullptr, x);
  FMI_LAUNCH_CHECK();
  FMI_TRY(clip_layers(m->layers, ClipLayerBuffers{x, n, (bf16_t*)(w + o_qkv), (bf16_t*)(w + o_a), (bf16_t*)(w + o_h), (bf16_t*)(w + o_g), ones}, B, T, D, H, F,
                      /*causal=*/0, s));
  if (hidden_out) FMI_HIP_TRY(hipMemcpyAsync(hidden_out, x, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, s));  // last_hidden_state: before post_layernorm
  // the tail: post_layernorm of the B class rows only (row 0 of each sample), then visual_projection (no bias)
  FMI_HIP_TRY(hipMemcpy2DAsync(cf, (size_t)D * 4, x, (size_t)T * D * 4, (size_t)D * 4, B, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(layernorm_affine_kernel, dim3((B + 3) / 4), dim3(256), 0, s, cf, m->postw, m->postb, 1e-5f, B, D, cb, (float*)nullptr);
  FMI_LAUNCH_CHECK();
  p = lin(cb, D, m->proj, nullptr, of, E, B, E, D, EPI_STORE_F32);
  FMI_TRY(launch_gemm(&p, 1, s));
  if (dtype == FMI_BF16) FMI_TRY(launch_cast_to_bf16(of, FMI_F32, ob, (int64_t)B * E, s));
  FMI_TRY(write_out(of, ob, image_embeds_out, dtype, (int64_t)B * E, s));
  FMI_HIP_TRY(hipStreamSynchronize(s));  // (the workspace is the handle's: the next call may regrow it)
  return FMI_OK;
}
