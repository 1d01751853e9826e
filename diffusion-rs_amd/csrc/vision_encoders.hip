// vision_encoders.hip — the encoders that take a picture as a picture, in front of the denoise loop:
//   fmi_resize_bicubic_u8    == PIL's Image.resize(BICUBIC) on u8 (what CLIP's and SigLIP's image processors resize with)
//   fmi_clip_preprocess_u8   == centre crop + (v / 255 - mean) / std (SigLIP resizes straight to S x S: its crop takes everything)
//   fmi_clip_vision_*        == HuggingFace's CLIPVisionModelWithProjection (modeling_clip.py): patch embedding, class token + positions, pre-LayerNorm,
//                               the CLIP encoder layers of the text tower without the causal mask, post-LayerNorm of the class row, visual_projection
//   fmi_siglip_vision_*      == HuggingFace's SiglipVisionModel.last_hidden_state (modeling_siglip.py): biased patch embedding + positions (no class token, no
//                               pre-LayerNorm), the encoder layers (tanh-GELU, eps from the config), post_layernorm of every row; the pooling head is not run
//   fmi_redux_*              == diffusers' ReduxImageEncoder: redux_down(silu(redux_up(h))), times the request's scale
// They run once per request next to a 3 s image: the kernels here are single-pass and bandwidth-bound, every Linear goes through launch_gemm (the patch
// embedding as a GEMM over patch rows, K = 3 P^2 zero-padded to the GEMM's multiple of 64).  Handle frame and encoder layer are encoder_common.h's, shared
// with the text towers; the two towers here also share their front end (vision_front_end).  They differ in the attention: CLIP's 64-wide heads run the
// encoders' lane-per-key kernel, SigLIP's — 729 keys at head dim 72 for the so400m tower — the transformer's MFMA attention at d = 128, the heads zero-padded
// in the weights (encoder_common.h: enc_layer_layout), so no activation is padded per call.
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

// pixel_values (B, 3, S, S) f32 -> the patch GEMM's operand (B * G * G, Kpad) bf16, G = S / P rounded down (the pixels past G P are not read): row
// (b, gy, gx) holds its patch in (c, py, px) order — the order of patch_embedding.weight (D, 3, P, P) flattened — and zeros in the columns [3 P^2, Kpad)
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

// SiglipVisionEmbeddings: x[b, t] += position_embedding[t], in place on the f32 stream (the patch GEMM has written patch + conv bias there).  x: (B, Np, D)
__global__ __launch_bounds__(256) void siglip_embed_kernel(float* __restrict__ x, const bf16_t* __restrict__ pos, int64_t per_image, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] += bf16_to_f32(pos[i % per_image]);
}

// q and k of token-major q|k|v rows (rows = B * T, 3 HP columns, head h at columns h * 128 of each third) -> head-major (B, H, T, 128): what the attention
// reads.  One 16-byte load and store per 8 elements, each read once; v stays where it is (launch_v_transpose reads it in place).
__global__ __launch_bounds__(256) void qk_head_major_kernel(const bf16_t* __restrict__ qkv, int T, int H, bf16_t* __restrict__ qh, bf16_t* __restrict__ kh, int64_t n16) {
  const int hp8 = H * 16;  // 16-byte pieces per row of one third
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n16; i += (int64_t)gridDim.x * blockDim.x) {
    const int part = i >= n16;
    const int64_t j = i - part * n16, row = j / hp8;
    const int c8 = (int)(j - row * hp8), h = c8 >> 4, c = c8 & 15;
    const int64_t b = row / T, t = row - b * T;
    const uint4 v = *reinterpret_cast<const uint4*>(qkv + (row * 3 + part) * (int64_t)(hp8 * 8) + c8 * 8);
    *reinterpret_cast<uint4*>((part ? kh : qh) + (((b * H + h) * T + t) * 128 + c * 8)) = v;
  }
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

// ------------------------------------------------------------------------------------ what the two towers share
// a vision tower's handle: the patch grid of its configuration and its pointers into the arena (patchb: SigLIP's convolution has a bias; cls: CLIP's has a
// class token in front of the patches)
struct VisionTower : EncoderHandle {
  int Np = 0, Kpad = 0;  // patches per image, and the patch GEMM's K: 3 P^2 rounded up to 64
  bf16_t *patch = nullptr, *patchb = nullptr, *cls = nullptr, *pos = nullptr, *postw = nullptr, *postb = nullptr;
  std::vector<EncLayer> layers;
  void set_grid(int image_size, int patch_size) {  // (the convolution has no padding: image_size / patch_size patches per side, rounded down)
    const int G = image_size / patch_size;
    Np = G * G, Kpad = (int)align_up(3 * patch_size * patch_size, 64);
  }
};

// The front end: the stride-P convolution as one GEMM over patch rows (pa: its operand (B Np, Kpad) bf16; its bias, where the tower has one, in the
// epilogue) into pe (B Np, D) f32, then the tower's embedding into x.  With a class token x is (B, 1 + Np, D) = class token and patches, + positions; without
// one the positions are added in place, and pe must be x itself.
int vision_front_end(const VisionTower& m, const float* pixel_values, int B, int S, int P, int D, bf16_t* pa, float* pe, float* x, hipStream_t s) {
  const int prows = B * m.Np;
  const int64_t npa = (int64_t)prows * m.Kpad;
  hipLaunchKernelGGL(patchify_kernel, flat_grid(npa), dim3(256), 0, s, pixel_values, S, P, m.Kpad, pa, npa);
  FMI_LAUNCH_CHECK();
  GemmProblem p = lin(pa, m.Kpad, m.patch, m.patchb, pe, D, prows, D, m.Kpad, EPI_STORE_F32);
  FMI_TRY(launch_gemm(&p, 1, s));
  if (m.cls) {
    const int64_t nx = (int64_t)(prows + B) * D;
    hipLaunchKernelGGL(vision_embed_kernel, flat_grid(nx), dim3(256), 0, s, pe, m.cls, m.pos, m.Np, D, x, nx);
  } else {
    const int64_t nx = (int64_t)prows * D;
    hipLaunchKernelGGL(siglip_embed_kernel, flat_grid(nx), dim3(256), 0, s, x, m.pos, (int64_t)m.Np * D, nx);
  }
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

// the SigLIP tower's attention step, T tokens of H heads of head dim hd in 128-wide slots: q and k head-major into qh and kh (B, H, T, 128), v transposed into
// vt (B, H, 128, Lp), Lp = T rounded up to 64, whose tail [T, Lp) is ZERO (launch_vt_zero_pad, once per forward: the transposes never write there), then the
// transformer's attention at d = 128 with the scale of the real head, not of the padded one
auto siglip_attention(int B, int T, int H, int hd, bf16_t* qh, bf16_t* kh, bf16_t* vt, hipStream_t s) {
  return [=](const bf16_t* qkv, bf16_t* out) -> int {
    const int HP = H * 128, Lp = (int)align_up(T, 64);
    const int64_t n16 = (int64_t)B * T * H * 16;
    hipLaunchKernelGGL(qk_head_major_kernel, flat_grid(2 * n16), dim3(256), 0, s, qkv, T, H, qh, kh, n16);
    FMI_LAUNCH_CHECK();
    FMI_TRY(launch_v_transpose(qkv + 2 * HP, 3 * HP, (int64_t)T * 3 * HP, vt, B, H, T, 0, Lp, s));
    return launch_attention(qh, kh, vt, out, B, H, T, T, Lp, 1.0f / sqrtf((float)hd), /*out_token_major=*/1, s);
  };
}

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
struct fmi_clip_vision : VisionTower {
  fmi_clip_vision_config cfg;
  bf16_t *prew = nullptr, *preb = nullptr, *proj = nullptr;
};

static void clip_vision_layout(fmi_clip_vision* m) {
  const fmi_clip_vision_config& c = m->cfg;
  const int D = c.hidden_size, F = c.intermediate_size, P = c.patch_size;
  Registry& r = m->r;
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
  for (int l = 0; l < c.num_hidden_layers; ++l) m->layers[l] = enc_layer_layout(r, vm + "encoder.layers." + std::to_string(l) + ".", D, c.num_attention_heads, F, 64);
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
  std::unique_ptr<fmi_clip_vision> m(new fmi_clip_vision());
  m->cfg = *cfg;
  m->set_grid(cfg->image_size, cfg->patch_size);
  FMI_TRY(create_arena("clip_vision_create", m.get(), clip_vision_layout, /*zero=*/false));
  *out = m.release();
  return FMI_OK;
}
extern "C" void fmi_clip_vision_destroy(fmi_clip_vision* m) { delete m; }  // (the weight arena and the workspace are DeviceBuffers)
extern "C" int fmi_clip_vision_set_tensor(fmi_clip_vision* m, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  return enc_set_tensor(m, "clip_vision_set_tensor", name, data, dtype, shape, rank);
}
extern "C" int fmi_clip_vision_missing_count(const fmi_clip_vision* m) { return enc_missing_count(m); }
extern "C" const char* fmi_clip_vision_missing_name(fmi_clip_vision* m, int i) { return enc_missing_name(m, i); }
extern "C" size_t fmi_clip_vision_size_in_bytes(const fmi_clip_vision* m) { return enc_size_in_bytes(m); }

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
  Carve carve;
  const size_t o_x = carve((size_t)rows * D * 4), o_n = carve((size_t)rows * D * 2), o_qkv = carve((size_t)rows * 3 * D * 2), o_a = carve((size_t)rows * D * 2);
  const size_t o_h = carve((size_t)rows * F * 2), o_g = carve((size_t)rows * F * 2), o_ones = carve((size_t)D * 4);
  const size_t o_pa = carve((size_t)prows * Kpad * 2), o_pe = carve((size_t)prows * D * 4), o_e = carve((size_t)rows * D * 4);
  const size_t o_cf = carve((size_t)B * D * 4), o_cb = carve((size_t)B * D * 2), o_of = carve((size_t)B * E * 4), o_ob = carve((size_t)B * E * 2);
  FMI_TRY(m->ws.reserve(carve.total));
  const Workspace& ws = m->ws;
  float *x = ws.at<float>(o_x), *ones = ws.at<float>(o_ones), *e = ws.at<float>(o_e), *cf = ws.at<float>(o_cf), *of = ws.at<float>(o_of);
  bf16_t *cb = ws.at<bf16_t>(o_cb), *ob = ws.at<bf16_t>(o_ob);
  const EncLayerBuffers lw{x, ws.at<bf16_t>(o_n), ws.at<bf16_t>(o_qkv), ws.at<bf16_t>(o_a), ws.at<bf16_t>(o_h), ws.at<bf16_t>(o_g), ones};

  hipLaunchKernelGGL(fill_f32_kernel, dim3(16), dim3(256), 0, s, ones, D, 1.0f);
  // CLIPVisionEmbeddings (patches, class token + positions), then pre_layrnorm into the f32 stream
  FMI_TRY(vision_front_end(*m, pixel_values, B, c.image_size, c.patch_size, D, ws.at<bf16_t>(o_pa), ws.at<float>(o_pe), e, s));
  hipLaunchKernelGGL(layernorm_affine_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, e, m->prew, m->preb, CLIP_LN_EPS, rows, D, (bf16_t*)nullptr, x);
  FMI_LAUNCH_CHECK();
  FMI_TRY(enc_layers(m->layers, lw, rows, D, D, F, CLIP_LN_EPS, ACT_QUICK_GELU, s, clip_attention(B, T, H, /*causal=*/0, s)));
  if (hidden_out) FMI_HIP_TRY(hipMemcpyAsync(hidden_out, x, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, s));  // last_hidden_state: before post_layernorm
  // the tail: post_layernorm of the B class rows only (row 0 of each sample), then visual_projection (no bias)
  FMI_HIP_TRY(hipMemcpy2DAsync(cf, (size_t)D * 4, x, (size_t)T * D * 4, (size_t)D * 4, B, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(layernorm_affine_kernel, dim3((B + 3) / 4), dim3(256), 0, s, cf, m->postw, m->postb, CLIP_LN_EPS, B, D, cb, (float*)nullptr);
  FMI_LAUNCH_CHECK();
  GemmProblem p = lin(cb, D, m->proj, nullptr, of, E, B, E, D, EPI_STORE_F32);
  FMI_TRY(launch_gemm(&p, 1, s));
  if (dtype == FMI_BF16) FMI_TRY(launch_cast_to_bf16(of, FMI_F32, ob, (int64_t)B * E, s));
  FMI_TRY(write_out(of, ob, image_embeds_out, dtype, (int64_t)B * E, s));
  FMI_HIP_TRY(hipStreamSynchronize(s));  // (the workspace is the handle's: the next call may regrow it)
  return FMI_OK;
}

// ====================================================================================== SigLIP vision tower
struct fmi_siglip_vision : VisionTower {
  fmi_siglip_vision_config cfg;
};

static void siglip_vision_layout(fmi_siglip_vision* m) {
  const fmi_siglip_vision_config& c = m->cfg;
  const int D = c.hidden_size, P = c.patch_size;
  Registry& r = m->r;
  const std::string vm = "vision_model.";
  m->patch = r.take((size_t)D * m->Kpad);  // rows of Kpad, zero behind the 3 P^2 columns of the tensor
  r.reg_padded4(vm + "embeddings.patch_embedding.weight", m->patch, D, 3, P, P, m->Kpad);
  m->patchb = r.take(D);
  r.reg(vm + "embeddings.patch_embedding.bias", m->patchb, D, 0);
  m->pos = r.take((size_t)m->Np * D);
  r.reg(vm + "embeddings.position_embedding.weight", m->pos, m->Np, D);
  m->layers.resize(c.num_hidden_layers);
  for (int l = 0; l < c.num_hidden_layers; ++l)
    m->layers[l] = enc_layer_layout(r, vm + "encoder.layers." + std::to_string(l) + ".", D, c.num_attention_heads, c.intermediate_size, 128);
  m->postw = r.take(D), m->postb = r.take(D);
  r.reg(vm + "post_layernorm.weight", m->postw, D, 0), r.reg(vm + "post_layernorm.bias", m->postb, D, 0);
}

// the workspace of a batch of B pictures: offsets into one block (rows = B Np, HP = H * 128, Fp = F rounded up to 64, Lp = Np rounded up to 64: x (rows, D)
// f32, n (rows, D), qkv (rows, 3 HP), qh and kh (B, H, Np, 128), vt (B, H, 128, Lp), a (rows, HP), h and g (rows, Fp) bf16, ones (D) f32, pa (rows, Kpad) bf16)
struct SiglipCarve {
  size_t x, n, qkv, qh, kh, vt, a, h, g, ones, pa, total;
};
static SiglipCarve siglip_carve(const fmi_siglip_vision* m, int B) {
  const fmi_siglip_vision_config& c = m->cfg;
  const size_t rows = (size_t)B * m->Np, D = c.hidden_size, HP = (size_t)c.num_attention_heads * 128, Fp = align_up(c.intermediate_size, 64);
  const size_t Lp = align_up(m->Np, 64);
  Carve carve;
  SiglipCarve k;
  k.x = carve(rows * D * 4), k.n = carve(rows * D * 2), k.qkv = carve(rows * 3 * HP * 2), k.qh = carve(rows * HP * 2), k.kh = carve(rows * HP * 2);
  k.vt = carve((size_t)B * HP * Lp * 2), k.a = carve(rows * HP * 2), k.h = carve(rows * Fp * 2), k.g = carve(rows * Fp * 2), k.ones = carve(D * 4);
  k.pa = carve(rows * m->Kpad * 2);
  k.total = carve.total;
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
  std::unique_ptr<fmi_siglip_vision> m(new fmi_siglip_vision());
  m->cfg = *cfg;
  m->set_grid(cfg->image_size, cfg->patch_size);
  // zero: the pads that no tensor writes (fc1's rows [F, Fp) and its bias) are zero from here on
  FMI_TRY(create_arena("siglip_vision_create", m.get(), siglip_vision_layout, /*zero=*/true));
  *out = m.release();
  return FMI_OK;
}
extern "C" void fmi_siglip_vision_destroy(fmi_siglip_vision* m) { delete m; }  // (the weight arena and the workspace are DeviceBuffers)
extern "C" int fmi_siglip_vision_set_tensor(fmi_siglip_vision* m, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  return enc_set_tensor(m, "siglip_vision_set_tensor", name, data, dtype, shape, rank);
}
extern "C" int fmi_siglip_vision_missing_count(const fmi_siglip_vision* m) { return enc_missing_count(m); }
extern "C" const char* fmi_siglip_vision_missing_name(fmi_siglip_vision* m, int i) { return enc_missing_name(m, i); }
extern "C" size_t fmi_siglip_vision_size_in_bytes(const fmi_siglip_vision* m) { return enc_size_in_bytes(m); }

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
  const int D = c.hidden_size, H = c.num_attention_heads, Np = m->Np, rows = B * Np, HP = H * 128, Fp = (int)align_up(c.intermediate_size, 64);
  const SiglipCarve k = siglip_carve(m, B);
  FMI_TRY(m->ws.reserve(k.total));
  const Workspace& ws = m->ws;
  float *x = ws.at<float>(k.x), *ones = ws.at<float>(k.ones);
  bf16_t *qh = ws.at<bf16_t>(k.qh), *kh = ws.at<bf16_t>(k.kh), *vt = ws.at<bf16_t>(k.vt);
  const EncLayerBuffers lw{x, ws.at<bf16_t>(k.n), ws.at<bf16_t>(k.qkv), ws.at<bf16_t>(k.a), ws.at<bf16_t>(k.h), ws.at<bf16_t>(k.g), ones};

  hipLaunchKernelGGL(fill_f32_kernel, dim3(16), dim3(256), 0, s, ones, D, 1.0f);
  // SiglipVisionEmbeddings: the patch GEMM, its bias in the epilogue, straight into the f32 stream; then the positions
  FMI_TRY(vision_front_end(*m, pixel_values, B, c.image_size, c.patch_size, D, ws.at<bf16_t>(k.pa), x, x, s));
  // V^T's key tail [Np, Lp): zero once — the layers' transposes write the keys below Np only, and the attention multiplies the tail's P = 0 with it
  FMI_TRY(launch_vt_zero_pad(vt, B * H, Np, (int)align_up(Np, 64), s));
  FMI_TRY(enc_layers(m->layers, lw, rows, D, HP, Fp, c.layer_norm_eps, ACT_GELU_TANH, s, siglip_attention(B, Np, H, D / H, qh, kh, vt, s)));
  // post_layernorm of every row: last_hidden_state
  hipLaunchKernelGGL(layernorm_affine_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, m->postw, m->postb, c.layer_norm_eps, rows, D,
                     dtype == FMI_BF16 ? (bf16_t*)hidden_out : (bf16_t*)nullptr, dtype == FMI_F32 ? (float*)hidden_out : (float*)nullptr);
  FMI_LAUNCH_CHECK();
  FMI_HIP_TRY(hipStreamSynchronize(s));  // (the workspace is the handle's: the next call may regrow it)
  return FMI_OK;
}

// ====================================================================================== Redux embedder
struct fmi_redux : EncoderHandle {
  int D = 0, J = 0;  // redux_dim (the tower's hidden_size), txt_in_features (the transformer's joint_attention_dim)
  bf16_t *up = nullptr, *upb = nullptr, *down = nullptr, *downb = nullptr;
};

static void redux_layout(fmi_redux* m) {
  Registry& r = m->r;
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
  std::unique_ptr<fmi_redux> m(new fmi_redux());
  m->D = redux_dim, m->J = txt_dim;
  FMI_TRY(create_arena("redux_create", m.get(), redux_layout, /*zero=*/false));
  *out = m.release();
  return FMI_OK;
}
extern "C" void fmi_redux_destroy(fmi_redux* m) { delete m; }
extern "C" int fmi_redux_set_tensor(fmi_redux* m, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  return enc_set_tensor(m, "redux_set_tensor", name, data, dtype, shape, rank);
}
extern "C" int fmi_redux_missing_count(const fmi_redux* m) { return enc_missing_count(m); }
extern "C" const char* fmi_redux_missing_name(fmi_redux* m, int i) { return enc_missing_name(m, i); }
extern "C" size_t fmi_redux_size_in_bytes(const fmi_redux* m) { return enc_size_in_bytes(m); }

extern "C" int fmi_redux_forward(fmi_redux* m, const float* hidden, int rows, float scale, void* out, fmi_dtype dtype, void* stream) {
  if (m) FMI_TRY(use_device_ordinal(m->device));
  if (!m || !hidden || !out) return fail(FMI_ERR_INVALID, "redux_forward: null argument");
  if (rows <= 0 || rows > (1 << 20)) return fail(FMI_ERR_INVALID, "redux_forward: rows must be in 1 .. 2^20");
  if (dtype != FMI_F32 && dtype != FMI_BF16) return fail(FMI_ERR_INVALID, "redux_forward: out dtype must be F32 or BF16");
  if (!std::isfinite(scale)) return fail(FMI_ERR_INVALID, "redux_forward: scale must be finite");
  FMI_TRY(m->r.missing.ready("redux_forward"));
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D, J = m->J;
  Carve carve;
  const size_t o_in = carve((size_t)rows * D * 2), o_u = carve((size_t)rows * 3 * J * 2), o_a = carve((size_t)rows * 3 * J * 2), o_f = carve((size_t)rows * J * 4);
  FMI_TRY(m->ws.reserve(carve.total));
  bf16_t *in = m->ws.at<bf16_t>(o_in), *u = m->ws.at<bf16_t>(o_u), *a = m->ws.at<bf16_t>(o_a);
  float* f = m->ws.at<float>(o_f);
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
