// encoder_common.h — what the encoders in front of the denoise loop share (text_encoders.hip: T5 and the CLIP text tower; clip_vision.hip: the CLIP
// vision tower): the single-pass kernels of a pre-norm transformer layer on an f32 residual stream, the d = 64 lane-per-key attention, the named-tensor
// registry over one bf16 weight arena, the grow-only workspace, and the CLIP encoder layer both CLIP towers run.  Everything is file-local to the
// translation unit that includes it (anonymous namespace): the encoders run once per request, their kernels are small.
#pragma once
#include <math.h>

#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "common.h"

namespace fmi {
namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------------------------ kernels
// LayerNorm with affine (nn/layer_norm.rs:131-153, eps 1e-5 for CLIP); one wave per row
__global__ void layernorm_affine_kernel(const float* x, const bf16_t* w, const bf16_t* b, float eps, int rows, int D, bf16_t* out_bf, float* out_f32) {
  const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* xr = x + (int64_t)r * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s += xr[i];
  const float mean = wave_sum(s) / (float)D;
  float v2 = 0.f;
  for (int i = lane; i < D; i += 64) {
    const float d = xr[i] - mean;
    v2 += d * d;
  }
  const float inv = 1.0f / sqrtf(wave_sum(v2) / (float)D + eps);
  for (int i = lane; i < D; i += 64) {
    const float v = (xr[i] - mean) * inv * bf16_to_f32(w[i]) + bf16_to_f32(b[i]);
    if (out_bf) out_bf[(int64_t)r * D + i] = f32_to_bf16(v);
    if (out_f32) out_f32[(int64_t)r * D + i] = v;
  }
}

// softmax(q k^T * scale + bias [causal]) v, head dim 64.  qkv: (B*T, 3*I) bf16 token-major rows
// [q | k | v], head h at columns h*64 of each part.  One wave per query row, lane = key index
// (scores) then lane = output channel (P V).  T <= 64 * MAXKB.
constexpr int ENC_MAXKB = 16;
__global__ __launch_bounds__(256) void enc_attention_kernel(const bf16_t* qkv, const float* bias, int B, int T, int H, float scale, int causal, bf16_t* out) {
  extern __shared__ float enc_sm[];  // per wave: 64 floats of q, then T floats of p
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
  if (i >= T) return;
  const int I = H * 64, ld = 3 * I;
  float* qs = enc_sm + wave * (64 + T);
  float* ps = qs + 64;
  const bf16_t* base = qkv + (int64_t)b * T * ld + h * 64;
  qs[lane] = bf16_to_f32(base[(int64_t)i * ld + lane]) * scale;
  __builtin_amdgcn_wave_barrier();
  const int nkb = (T + 63) >> 6;
  float sc[ENC_MAXKB];
  float mx = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < ENC_MAXKB; ++kb) {
    sc[kb] = -INFINITY;
    if (kb < nkb) {
      const int j = kb * 64 + lane;
      if (j < T && (!causal || j <= i)) {
        const uint4* kr = reinterpret_cast<const uint4*>(base + (int64_t)j * ld + I);
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const uint4 u = kr[c];
          const uint32_t w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc += qs[c * 8 + e * 2] * __uint_as_float(w4[e] << 16);
            acc += qs[c * 8 + e * 2 + 1] * __uint_as_float(w4[e] & 0xffff0000u);
          }
        }
        if (bias) acc += bias[((int64_t)h * T + i) * T + j];
        sc[kb] = acc;
        mx = fmaxf(mx, acc);
      }
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int kb = 0; kb < ENC_MAXKB; ++kb)
    if (kb < nkb) {
      const int j = kb * 64 + lane;
      const float p = sc[kb] == -INFINITY ? 0.f : __expf(sc[kb] - mx);
      if (j < T) ps[j] = p;
      sum += p;
    }
  sum = wave_sum(sum);
  __builtin_amdgcn_wave_barrier();
  const int jend = causal ? i + 1 : T;
  const bf16_t* vcol = base + 2 * I + lane;
  float acc = 0.f;
  for (int j = 0; j < jend; ++j) acc += ps[j] * bf16_to_f32(vcol[(int64_t)j * ld]);
  out[((int64_t)b * T + i) * I + h * 64 + lane] = f32_to_bf16(acc / sum);
}

// act: 0 relu, 1 gelu-tanh (NewGelu), 2 silu, 3 quick-gelu x*sigmoid(1.702x).
// gated: in (rows, 2F) = [gate-input | linear]  -> out (rows, F) = act(in[:, :F]) * in[:, F:]
// else : in (rows, F) -> out = act(in)
__global__ void enc_act_kernel(const bf16_t* in, int rows, int F, int act, int gated, bf16_t* out) {
  const int64_t n = (int64_t)rows * F;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / F, c = e - r * F;
    const float a = bf16_to_f32(in[gated ? r * 2 * F + c : e]);
    float v;
    if (act == 0)
      v = a > 0.f ? a : 0.f;
    else if (act == 1)
      v = gelu_tanh(a);
    else if (act == 2)
      v = silu(a);
    else
      v = a / (1.0f + __expf(-1.702f * a));
    if (gated) v *= bf16_to_f32(in[r * 2 * F + F + c]);
    out[e] = f32_to_bf16(v);
  }
}

__global__ void fill_f32_kernel(float* p, int n, float v) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v;
}

// ------------------------------------------------------------------------------ model plumbing
struct Dest {
  bf16_t* ptr;
  int rows, cols;  // cols == 0 -> 1-D
  int ld = 0;      // row stride in the arena when it is wider than cols (the columns [cols, ld) are zero); 0 -> cols
  int inner[3] = {0, 0, 0};  // inner[0] != 0: the tensor arrives as rank 4, (rows, inner[0], inner[1], inner[2]) with cols = their product
  int own[2] = {0, 0};       // own[0] != 0: the tensor arrives as (own[0], own[1]) (own[1] == 0: 1-D) and is stored as `rows` chunks of `cols` elements (reg_chunks)
};
struct Registry {
  DeviceBuffer arena;
  size_t bytes = 0, used = 0;  // bytes: the layout size (known before the arena exists)
  std::map<std::string, Dest> names;
  MissingSet missing;
  bf16_t* take(size_t count) {
    const size_t off = align_up(used, 256);
    used = off + count * sizeof(bf16_t);
    return arena ? reinterpret_cast<bf16_t*>(arena.as<char>() + off) : nullptr;
  }
  void reg(const std::string& name, bf16_t* p, int rows, int cols) {
    names[name] = Dest{p, rows, cols};
    missing.insert(name);
  }
  // a rank-4 tensor (rows, i0, i1, i2) stored as rows of ld >= i0 * i1 * i2 elements, zero behind the tensor's own columns: a GEMM operand whose K is padded
  void reg_padded4(const std::string& name, bf16_t* p, int rows, int i0, int i1, int i2, int ld) {
    Dest d{p, rows, i0 * i1 * i2};
    d.ld = ld, d.inner[0] = i0, d.inner[1] = i1, d.inner[2] = i2;
    names[name] = d;
    missing.insert(name);
  }
  // a tensor (s0, s1) (s1 == 0: 1-D) cut into `chunks` contiguous pieces of `chunk` elements, piece i stored at element i * ld of the slot, zero in
  // [chunk, ld): rows that scatter into padded head slots (a q / k / v projection (H hd, D): H pieces of hd D elements at a stride of 128 D; its bias: H
  // pieces of hd at 128) and columns that do (an out_proj (D, H hd): D H pieces of hd at 128)
  void reg_chunks(const std::string& name, bf16_t* p, int s0, int s1, int chunks, int chunk, int ld) {
    Dest d{p, chunks, chunk};
    d.ld = ld, d.own[0] = s0, d.own[1] = s1;
    names[name] = d;
    missing.insert(name);
  }
  int set(const char* who, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
    if (!name || !data) return fail(FMI_ERR_INVALID, std::string(who) + ": null argument");
    auto it = names.find(name);
    if (it == names.end()) return fail(FMI_ERR_INVALID, std::string(who) + ": unknown tensor name '" + name + "'");
    const Dest& d = it->second;
    bool ok = d.cols ? (rank == 2 && shape[0] == d.rows && shape[1] == d.cols) : (rank == 1 && shape[0] == d.rows);
    std::string want = std::to_string(d.rows) + (d.cols ? "," + std::to_string(d.cols) : "");
    if (d.inner[0]) {
      ok = rank == 4 && shape[0] == d.rows && shape[1] == d.inner[0] && shape[2] == d.inner[1] && shape[3] == d.inner[2];
      want = std::to_string(d.rows) + "," + std::to_string(d.inner[0]) + "," + std::to_string(d.inner[1]) + "," + std::to_string(d.inner[2]);
    }
    if (d.own[0]) {
      ok = d.own[1] ? (rank == 2 && shape[0] == d.own[0] && shape[1] == d.own[1]) : (rank == 1 && shape[0] == d.own[0]);
      want = std::to_string(d.own[0]) + (d.own[1] ? "," + std::to_string(d.own[1]) : "");
    }
    if (!ok) return fail(FMI_ERR_INVALID, std::string(who) + ": shape mismatch for " + name + " (expected (" + want + "))");
    if (dtype != FMI_F32 && dtype != FMI_F16 && dtype != FMI_BF16) return fail(FMI_ERR_INVALID, std::string(who) + ": dtype must be F32/F16/BF16");
    const int64_t numel = (int64_t)d.rows * (d.cols ? d.cols : 1);
    if (d.ld > d.cols) {  // dense bf16 in a staging block, then a row-strided copy into the zeroed slot
      DeviceBuffer dense;
      FMI_HIP_TRY(dense.alloc((size_t)numel * sizeof(bf16_t)));
      FMI_TRY(upload_as_bf16(data, dtype, numel, dense.as<bf16_t>()));
      FMI_HIP_TRY(hipMemset(d.ptr, 0, (size_t)d.rows * d.ld * sizeof(bf16_t)));
      FMI_HIP_TRY(hipMemcpy2D(d.ptr, (size_t)d.ld * sizeof(bf16_t), dense.ptr, (size_t)d.cols * sizeof(bf16_t), (size_t)d.cols * sizeof(bf16_t), d.rows,
                              hipMemcpyDeviceToDevice));
      FMI_HIP_TRY(hipDeviceSynchronize());  // before the staging block goes
    } else {
      FMI_TRY(upload_as_bf16(data, dtype, numel, d.ptr));
    }
    missing.erase(name);
    return FMI_OK;
  }
};

struct Workspace {
  DeviceBuffer base;
  int B = 0, T = 0;
  int reserve(size_t need) {  // grow-only
    if (need <= base.bytes()) return FMI_OK;
    FMI_HIP_TRY(base.alloc(need));
    return FMI_OK;
  }
};

GemmProblem lin(const bf16_t* A, int lda, const bf16_t* W, const bf16_t* bias, void* out, int ldo, int M, int N, int K, int epi) {
  GemmProblem p{};
  p.A = A, p.W = W, p.bias = bias, p.out = out, p.M = M, p.N = N, p.K = K, p.lda = lda, p.ldw = K, p.ldo = ldo, p.epi = epi, p.alpha = 1.f;
  return p;
}

int enc_attention(const bf16_t* qkv, const float* bias, int B, int T, int H, float scale, int causal, bf16_t* out, hipStream_t s) {
  if (T > 64 * ENC_MAXKB) return fail(FMI_ERR_UNSUPPORTED, "text encoder attention: sequence longer than " + std::to_string(64 * ENC_MAXKB));
  const size_t sm = 4 * (64 + (size_t)T) * sizeof(float);
  hipLaunchKernelGGL(enc_attention_kernel, dim3((T + 3) / 4, H, B), dim3(256), sm, s, qkv, bias, B, T, H, scale, causal, out);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

int write_out(const float* src_f32, const bf16_t* src_bf, void* out, fmi_dtype dt, int64_t n, hipStream_t s) {
  if (dt == FMI_F32) {
    FMI_HIP_TRY(hipMemcpyAsync(out, src_f32, n * 4, hipMemcpyDeviceToDevice, s));
    return FMI_OK;
  }
  if (dt == FMI_BF16) {
    FMI_HIP_TRY(hipMemcpyAsync(out, src_bf, n * 2, hipMemcpyDeviceToDevice, s));
    return FMI_OK;
  }
  return fail(FMI_ERR_INVALID, "text encoder output dtype must be F32 or BF16");
}

// ------------------------------------------------------------------- the CLIP encoder layer (both towers)
// ClipEncoderLayer (clip/text.rs:228-238; HF's CLIPEncoderLayer is the same for the vision tower): LayerNorm -> fused q|k|v -> attention at head dim 64 ->
// out_proj into the f32 stream -> LayerNorm -> fc1 -> quick-GELU -> fc2 into the stream.
struct ClipLayer {
  bf16_t *l1w, *l1b, *qkv, *qkvb, *o, *ob, *l2w, *l2b, *f1, *f1b, *f2, *f2b;
};
// the layer's slots in the arena and its names under prefix p ("text_model.encoder.layers.3."), width D, MLP width F
void clip_layer_layout(Registry& r, const std::string& p, int D, int F, ClipLayer& L) {
  L.l1w = r.take(D), L.l1b = r.take(D);
  r.reg(p + "layer_norm1.weight", L.l1w, D, 0), r.reg(p + "layer_norm1.bias", L.l1b, D, 0);
  L.qkv = r.take((size_t)3 * D * D), L.qkvb = r.take((size_t)3 * D);
  const char* nm[3] = {"q_proj", "k_proj", "v_proj"};
  for (int i = 0; i < 3; ++i) {
    r.reg(p + "self_attn." + nm[i] + ".weight", L.qkv ? L.qkv + (size_t)i * D * D : nullptr, D, D);
    r.reg(p + "self_attn." + nm[i] + ".bias", L.qkvb ? L.qkvb + (size_t)i * D : nullptr, D, 0);
  }
  L.o = r.take((size_t)D * D), L.ob = r.take(D);
  r.reg(p + "self_attn.out_proj.weight", L.o, D, D), r.reg(p + "self_attn.out_proj.bias", L.ob, D, 0);
  L.l2w = r.take(D), L.l2b = r.take(D);
  r.reg(p + "layer_norm2.weight", L.l2w, D, 0), r.reg(p + "layer_norm2.bias", L.l2b, D, 0);
  L.f1 = r.take((size_t)F * D), L.f1b = r.take(F);
  r.reg(p + "mlp.fc1.weight", L.f1, F, D), r.reg(p + "mlp.fc1.bias", L.f1b, F, 0);
  L.f2 = r.take((size_t)D * F), L.f2b = r.take(D);
  r.reg(p + "mlp.fc2.weight", L.f2, D, F), r.reg(p + "mlp.fc2.bias", L.f2b, D, 0);
}
// the buffers a run of layers works in, rows = B * T: x (rows, D) f32 the stream (in / out), n (rows, D), qkv (rows, 3 D), a (rows, D), h and g (rows, F) bf16,
// ones (D) f32 of 1.0 (the residual epilogue's gate)
struct ClipLayerBuffers {
  float* x;
  bf16_t *n, *qkv, *a, *h, *g;
  const float* ones;
};
int clip_layers(const std::vector<ClipLayer>& layers, const ClipLayerBuffers& w, int B, int T, int D, int H, int F, int causal, hipStream_t s) {
  const int rows = B * T, nb = (rows + 3) / 4;
  const float scale = 1.0f / sqrtf(64.0f);  // (head_dim)^-0.5, clip/text.rs:101
  for (const ClipLayer& L : layers) {
    hipLaunchKernelGGL(layernorm_affine_kernel, dim3(nb), dim3(256), 0, s, w.x, L.l1w, L.l1b, 1e-5f, rows, D, w.n, (float*)nullptr);
    GemmProblem p = lin(w.n, D, L.qkv, L.qkvb, w.qkv, 3 * D, rows, 3 * D, D, EPI_STORE_BF16);
    FMI_TRY(launch_gemm(&p, 1, s));
    FMI_TRY(enc_attention(w.qkv, nullptr, B, T, H, scale, causal, w.a, s));  // text: causal mask (:273-291); q * scale (:130)
    p = lin(w.a, D, L.o, L.ob, w.x, D, rows, D, D, EPI_RESID_GATE_F32);
    p.gate = w.ones;
    FMI_TRY(launch_gemm(&p, 1, s));
    hipLaunchKernelGGL(layernorm_affine_kernel, dim3(nb), dim3(256), 0, s, w.x, L.l2w, L.l2b, 1e-5f, rows, D, w.n, (float*)nullptr);
    p = lin(w.n, D, L.f1, L.f1b, w.h, F, rows, F, D, EPI_STORE_BF16);
    FMI_TRY(launch_gemm(&p, 1, s));
    hipLaunchKernelGGL(enc_act_kernel, dim3(256), dim3(256), 0, s, w.h, rows, F, 3, 0, w.g);  // QuickGelu (:13-19)
    p = lin(w.g, F, L.f2, L.f2b, w.x, D, rows, D, F, EPI_RESID_GATE_F32);
    p.gate = w.ones;
    FMI_TRY(launch_gemm(&p, 1, s));
  }
  return FMI_OK;
}

// ------------------------------------------------------------------- the SigLIP encoder layer (siglip_vision.hip)
// HF's SiglipEncoderLayer: LayerNorm(eps) -> fused q|k|v -> attention at head dim hd = D / H on the transformer's MFMA attention (d = 128) -> out_proj into
// the f32 stream -> LayerNorm -> fc1 -> tanh-GELU -> fc2 into the stream.  The heads are zero-padded to 128 IN THE WEIGHTS: head h's q / k / v rows sit at rows
// h * 128 .. h * 128 + hd of a (3 H 128, D) operand, out_proj's K is (D, H 128) with zero pad columns, so the q|k|v GEMM writes 128-wide heads whose lanes
// [hd, 128) are exactly 0 (zero weight rows, zero bias) and contribute 0 to every score and meet zero out_proj columns.  F is padded to Fp = a multiple of 64 the
// same way: zero fc1 rows and bias, gelu(0) = 0, zero fc2 columns.
struct SiglipLayer {
  bf16_t *l1w, *l1b, *qkv, *qkvb, *o, *ob, *l2w, *l2b, *f1, *f1b, *f2, *f2b;
};
// the layer's slots and names under prefix p; the arena must be zero before the tensors arrive (the fc1 pad rows and every bias pad are never written)
void siglip_layer_layout(Registry& r, const std::string& p, int D, int H, int F, SiglipLayer& L) {
  const int hd = D / H, HP = H * 128, Fp = (int)align_up(F, 64);
  L.l1w = r.take(D), L.l1b = r.take(D);
  r.reg(p + "layer_norm1.weight", L.l1w, D, 0), r.reg(p + "layer_norm1.bias", L.l1b, D, 0);
  L.qkv = r.take((size_t)3 * HP * D), L.qkvb = r.take((size_t)3 * HP);
  const char* nm[3] = {"q_proj", "k_proj", "v_proj"};
  for (int i = 0; i < 3; ++i) {
    r.reg_chunks(p + "self_attn." + nm[i] + ".weight", L.qkv ? L.qkv + (size_t)i * HP * D : nullptr, D, D, H, hd * D, 128 * D);
    r.reg_chunks(p + "self_attn." + nm[i] + ".bias", L.qkvb ? L.qkvb + (size_t)i * HP : nullptr, D, 0, H, hd, 128);
  }
  L.o = r.take((size_t)D * HP), L.ob = r.take(D);
  r.reg_chunks(p + "self_attn.out_proj.weight", L.o, D, D, D * H, hd, 128), r.reg(p + "self_attn.out_proj.bias", L.ob, D, 0);
  L.l2w = r.take(D), L.l2b = r.take(D);
  r.reg(p + "layer_norm2.weight", L.l2w, D, 0), r.reg(p + "layer_norm2.bias", L.l2b, D, 0);
  L.f1 = r.take((size_t)Fp * D), L.f1b = r.take(Fp);  // (the rows [F, Fp) stay zero)
  r.reg(p + "mlp.fc1.weight", L.f1, F, D), r.reg(p + "mlp.fc1.bias", L.f1b, F, 0);
  L.f2 = r.take((size_t)D * Fp), L.f2b = r.take(D);
  r.reg_chunks(p + "mlp.fc2.weight", L.f2, D, F, D, F, Fp), r.reg(p + "mlp.fc2.bias", L.f2b, D, 0);
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

// the buffers a run of SigLIP layers works in, rows = B * T, HP = H * 128, Fp = F rounded up to 64, Lp = T rounded up to 64: x (rows, D) f32 the stream (in /
// out), n (rows, D), qkv (rows, 3 HP), qh and kh (B, H, T, 128), vt (B, H, 128, Lp) with its tail [T, Lp) ZERO (launch_vt_zero_pad, once: the transposes never
// write there), a (rows, HP), h and g (rows, Fp) bf16, ones (D) f32 of 1.0
struct SiglipLayerBuffers {
  float* x;
  bf16_t *n, *qkv, *qh, *kh, *vt, *a, *h, *g;
  const float* ones;
};
int siglip_layers(const std::vector<SiglipLayer>& layers, const SiglipLayerBuffers& w, int B, int T, int D, int H, int F, float eps, hipStream_t s) {
  const int rows = B * T, nb = (rows + 3) / 4, HP = H * 128, Fp = (int)align_up(F, 64), Lp = (int)align_up(T, 64);
  const float scale = 1.0f / sqrtf((float)(D / H));  // head_dim^-0.5 of the real head, not of the padded one
  const int64_t n16 = (int64_t)rows * H * 16;
  const dim3 flat((unsigned)std::min<int64_t>(cdiv64(2 * n16, 256), 4096));
  for (const SiglipLayer& L : layers) {
    hipLaunchKernelGGL(layernorm_affine_kernel, dim3(nb), dim3(256), 0, s, w.x, L.l1w, L.l1b, eps, rows, D, w.n, (float*)nullptr);
    GemmProblem p = lin(w.n, D, L.qkv, L.qkvb, w.qkv, 3 * HP, rows, 3 * HP, D, EPI_STORE_BF16);
    FMI_TRY(launch_gemm(&p, 1, s));
    hipLaunchKernelGGL(qk_head_major_kernel, flat, dim3(256), 0, s, w.qkv, T, H, w.qh, w.kh, n16);
    FMI_LAUNCH_CHECK();
    FMI_TRY(launch_v_transpose(w.qkv + 2 * HP, 3 * HP, (int64_t)T * 3 * HP, w.vt, B, H, T, 0, Lp, s));
    FMI_TRY(launch_attention(w.qh, w.kh, w.vt, w.a, B, H, T, T, Lp, scale, /*out_token_major=*/1, s));
    p = lin(w.a, HP, L.o, L.ob, w.x, D, rows, D, HP, EPI_RESID_GATE_F32);
    p.gate = w.ones;
    FMI_TRY(launch_gemm(&p, 1, s));
    hipLaunchKernelGGL(layernorm_affine_kernel, dim3(nb), dim3(256), 0, s, w.x, L.l2w, L.l2b, eps, rows, D, w.n, (float*)nullptr);
    p = lin(w.n, D, L.f1, L.f1b, w.h, Fp, rows, Fp, D, EPI_STORE_BF16);
    FMI_TRY(launch_gemm(&p, 1, s));
    hipLaunchKernelGGL(enc_act_kernel, dim3(256), dim3(256), 0, s, w.h, rows, Fp, 1, 0, w.g);  // gelu_pytorch_tanh
    p = lin(w.g, Fp, L.f2, L.f2b, w.x, D, rows, D, Fp, EPI_RESID_GATE_F32);
    p.gate = w.ones;
    FMI_TRY(launch_gemm(&p, 1, s));
  }
  return FMI_OK;
}

}  // namespace
}  // namespace fmi
