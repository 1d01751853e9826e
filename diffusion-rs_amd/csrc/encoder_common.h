// encoder_common.h — what the encoders in front of the denoise loop share (text_encoders.hip: T5 and the CLIP text tower; vision_encoders.hip: the CLIP and
// SigLIP vision towers and the Redux embedder): the single-pass kernels of a pre-norm transformer layer on an f32 residual stream, the d = 64 lane-per-key
// attention, the handle frame (the named-tensor registry over one bf16 weight arena, the grow-only workspace and its carving, the arena's creation and the
// entry points every handle has), and the encoder layer that the CLIP towers and the SigLIP tower run.  Everything is file-local to the translation unit that
// includes it (anonymous namespace): the encoders run once per request, their kernels are small.
#pragma once
#include <math.h>

#include <algorithm>
#include <map>
#include <memory>
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
  void begin_layout() {  // a layout pass starts from nothing: no bytes taken, no names
    used = 0;
    names.clear();
    missing.names.clear();
  }
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
  int reserve(size_t need) {  // grow-only
    if (need <= base.bytes()) return FMI_OK;
    FMI_HIP_TRY(base.alloc(need));
    return FMI_OK;
  }
  template <class T>
  T* at(size_t off) const {  // the region a Carve put at byte `off`
    return reinterpret_cast<T*>(base.as<char>() + off);
  }
};
// Lays regions out in a workspace, in call order: k(bytes) is the region's offset, every region starts on a multiple of 256, k.total is what to reserve
struct Carve {
  size_t total = 0;
  size_t operator()(size_t bytes) {
    const size_t o = total;
    total = align_up(total + bytes, 256);
    return o;
  }
};

// ------------------------------------------------------------------------------ the handle frame
// What every encoder handle (fmi_t5, fmi_clip, fmi_clip_vision, fmi_siglip_vision, fmi_redux) is: a device, named weights in one arena, a workspace.  The
// handle's own struct adds its configuration and its pointers into the arena; its C entry points forward here with their own name as `who`.
struct EncoderHandle {
  int device = current_device();
  Registry r;
  Workspace ws;
};
// The arena of a new handle.  layout(m) takes and registers every tensor: pass 0 runs it without an arena and only sizes, pass 1 hands out the pointers.
// zero: the arena starts as zeros (a layout with pads that no tensor writes).
template <class M>
int create_arena(const char* who, M* m, void (*layout)(M*), bool zero) {
  Registry& r = m->r;
  r.begin_layout(), layout(m);
  r.bytes = align_up(r.used, 256);
  hipError_t e = r.arena.alloc(r.bytes);
  if (e == hipSuccess && zero) e = hipMemset(r.arena.ptr, 0, r.bytes);
  if (e != hipSuccess) return fail(FMI_ERR_HIP, std::string(who) + ": hipMalloc of the weight arena: " + hipGetErrorString(e));
  r.begin_layout(), layout(m);
  return FMI_OK;
}
int enc_set_tensor(EncoderHandle* m, const char* who, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  if (!m) return fail(FMI_ERR_INVALID, std::string(who) + ": null model");
  FMI_TRY(use_device_ordinal(m->device));
  return m->r.set(who, name, data, dtype, shape, rank);
}
int enc_missing_count(const EncoderHandle* m) { return m ? m->r.missing.count() : 0; }
const char* enc_missing_name(const EncoderHandle* m, int i) { return m ? m->r.missing.name(i) : nullptr; }
size_t enc_size_in_bytes(const EncoderHandle* m) { return m ? m->r.bytes + m->ws.base.bytes() : 0; }

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

// ------------------------------------------------------------------- the encoder layer of the CLIP towers and the SigLIP tower
// ClipEncoderLayer (clip/text.rs:228-238; HF's CLIPEncoderLayer and SiglipEncoderLayer are the same layer): LayerNorm(eps) -> fused q|k|v -> attention ->
// out_proj into the f32 stream -> LayerNorm -> fc1 -> activation -> fc2 into the stream.  What differs between the towers is data: eps, the activation
// (quick-GELU for CLIP, tanh-GELU for SigLIP), the attention step, and the widths the GEMMs run at.  Head h's q / k / v rows sit at rows h * head_slot ..
// h * head_slot + hd of a (3 H head_slot, D) operand and out_proj's K is (D, H head_slot).  The CLIP towers run encoder_common's d = 64 attention: head_slot
// = hd = 64, nothing is padded.  The SigLIP tower runs the transformer's MFMA attention (d = 128) at hd = D / H <= 128: head_slot = 128, the heads are
// zero-padded IN THE WEIGHTS, so the q|k|v GEMM writes 128-wide heads whose lanes [hd, 128) are exactly 0 (zero weight rows, zero bias), contribute 0 to every
// score and meet zero out_proj columns.  F is padded to Fp = a multiple of 64 the same way: zero fc1 rows and bias, act(0) = 0, zero fc2 columns.
struct EncLayer {
  bf16_t *l1w, *l1b, *qkv, *qkvb, *o, *ob, *l2w, *l2b, *f1, *f1b, *f2, *f2b;
};
// the layer's slots in the arena and its names under prefix p ("text_model.encoder.layers.3."), width D, H heads in slots of head_slot, MLP width F.  Where
// there are pads (head_slot > D / H, or F no multiple of 64) the arena must be zero before the tensors arrive: the fc1 pad rows and every bias pad are never
// written.  (A tensor whose pieces fill their slots — every one of CLIP's — is stored as it arrives.)
EncLayer enc_layer_layout(Registry& r, const std::string& p, int D, int H, int F, int head_slot) {
  const int hd = D / H, HP = H * head_slot, Fp = (int)align_up(F, 64);
  EncLayer L;
  L.l1w = r.take(D), L.l1b = r.take(D);
  r.reg(p + "layer_norm1.weight", L.l1w, D, 0), r.reg(p + "layer_norm1.bias", L.l1b, D, 0);
  L.qkv = r.take((size_t)3 * HP * D), L.qkvb = r.take((size_t)3 * HP);
  const char* nm[3] = {"q_proj", "k_proj", "v_proj"};
  for (int i = 0; i < 3; ++i) {
    r.reg_chunks(p + "self_attn." + nm[i] + ".weight", L.qkv ? L.qkv + (size_t)i * HP * D : nullptr, D, D, H, hd * D, head_slot * D);
    r.reg_chunks(p + "self_attn." + nm[i] + ".bias", L.qkvb ? L.qkvb + (size_t)i * HP : nullptr, D, 0, H, hd, head_slot);
  }
  L.o = r.take((size_t)D * HP), L.ob = r.take(D);
  r.reg_chunks(p + "self_attn.out_proj.weight", L.o, D, D, D * H, hd, head_slot), r.reg(p + "self_attn.out_proj.bias", L.ob, D, 0);
  L.l2w = r.take(D), L.l2b = r.take(D);
  r.reg(p + "layer_norm2.weight", L.l2w, D, 0), r.reg(p + "layer_norm2.bias", L.l2b, D, 0);
  L.f1 = r.take((size_t)Fp * D), L.f1b = r.take(Fp);  // (the rows [F, Fp) stay zero)
  r.reg(p + "mlp.fc1.weight", L.f1, F, D), r.reg(p + "mlp.fc1.bias", L.f1b, F, 0);
  L.f2 = r.take((size_t)D * Fp), L.f2b = r.take(D);
  r.reg_chunks(p + "mlp.fc2.weight", L.f2, D, F, D, F, Fp), r.reg(p + "mlp.fc2.bias", L.f2b, D, 0);
  return L;
}
// the buffers a run of layers works in, HP = H * head_slot, Fp = F rounded up to 64: x (rows, D) f32 the stream (in / out), n (rows, D), qkv (rows, 3 HP),
// a (rows, HP), h and g (rows, Fp) bf16, ones (D) f32 of 1.0 (the residual epilogue's gate)
struct EncLayerBuffers {
  float* x;
  bf16_t *n, *qkv, *a, *h, *g;
  const float* ones;
};
// act: enc_act_kernel's code.  attention(qkv, out): the tower's attention step, token-major q|k|v rows (rows, 3 HP) -> (rows, HP)
template <class Attention>
int enc_layers(const std::vector<EncLayer>& layers, const EncLayerBuffers& w, int rows, int D, int HP, int Fp, float eps, int act, hipStream_t s, Attention attention) {
  const int nb = (rows + 3) / 4;
  for (const EncLayer& L : layers) {
    hipLaunchKernelGGL(layernorm_affine_kernel, dim3(nb), dim3(256), 0, s, w.x, L.l1w, L.l1b, eps, rows, D, w.n, (float*)nullptr);
    GemmProblem p = lin(w.n, D, L.qkv, L.qkvb, w.qkv, 3 * HP, rows, 3 * HP, D, EPI_STORE_BF16);
    FMI_TRY(launch_gemm(&p, 1, s));
    FMI_TRY(attention(w.qkv, w.a));
    p = lin(w.a, HP, L.o, L.ob, w.x, D, rows, D, HP, EPI_RESID_GATE_F32);
    p.gate = w.ones;
    FMI_TRY(launch_gemm(&p, 1, s));
    hipLaunchKernelGGL(layernorm_affine_kernel, dim3(nb), dim3(256), 0, s, w.x, L.l2w, L.l2b, eps, rows, D, w.n, (float*)nullptr);
    p = lin(w.n, D, L.f1, L.f1b, w.h, Fp, rows, Fp, D, EPI_STORE_BF16);
    FMI_TRY(launch_gemm(&p, 1, s));
    hipLaunchKernelGGL(enc_act_kernel, dim3(256), dim3(256), 0, s, w.h, rows, Fp, act, 0, w.g);
    p = lin(w.g, Fp, L.f2, L.f2b, w.x, D, rows, D, Fp, EPI_RESID_GATE_F32);
    p.gate = w.ones;
    FMI_TRY(launch_gemm(&p, 1, s));
  }
  return FMI_OK;
}
// the CLIP towers' attention step (head dim 64, q * (head_dim)^-0.5, clip/text.rs:101,130; the text tower's causal mask, :273-291) and their other constants
constexpr float CLIP_LN_EPS = 1e-5f;
constexpr int ACT_QUICK_GELU = 3, ACT_GELU_TANH = 1;  // QuickGelu (clip/text.rs:13-19); gelu_pytorch_tanh
auto clip_attention(int B, int T, int H, int causal, hipStream_t s) {
  return [=](const bf16_t* qkv, bf16_t* out) { return enc_attention(qkv, nullptr, B, T, H, 1.0f / sqrtf(64.0f), causal, out, s); };
}

}  // namespace
}  // namespace fmi
