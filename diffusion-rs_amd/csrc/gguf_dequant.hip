// gguf_dequant.hip — ggml block dequantisation (the formats of llama.cpp's .gguf files) into the bf16 / f32 operands the GEMMs read.
//
// Semantics: the reference's GgmlType::to_float (diffusion_rs_common/src/core/quantized/k_quants.rs — Q4_0 :175, Q4_1 :341, Q5_0 :440,
// Q5_1 :547, Q8_0 :580, Q4_K :1568, Q5_K :1872, Q6_K :2147; block structs :56-158; get_scale_min_k4 utils.rs:49), evaluated in f32 with
// EVERY multiply and every add / subtract rounded on its own (Rust never contracts: `d1 * q - m1` is two roundings, `d * sc * q` is
// `(d * sc) * q`), then ONE RNE rounding to bf16.  hipcc contracts a * b + c into an fma by default, so the whole file is compiled with
// contraction off (the pragma below).  f16 -> f32 and int -> f32 are exact, so the result is bit-equal to a NumPy float32 restatement.
//
// Shape: memory-bound (0.53 .. 1.06 B in, 2 B out per weight).  A block is 18 .. 210 bytes and in general only 2-byte aligned, so a lane
// never reads packed bytes from HBM on its own: a workgroup brings the contiguous byte range of its GROUP elements into LDS with
// 16-byte aligned loads (the 16-byte pieces that straddle the tensor's first / last byte are read as 2-byte words, in bounds), then
// every lane decodes 8 consecutive weights from LDS and stores 16 bytes (bf16) — 1 KiB contiguous per wave-instruction.  All element
// and byte counts are 64-bit: FLUX.1-dev's fused modulation matrix has 3.2e9 weights.
#include <algorithm>

#include "common.h"

#pragma clang fp contract(off)

namespace fmi {
namespace {

enum GgmlType { GQ4_0 = 2, GQ4_1 = 3, GQ5_0 = 6, GQ5_1 = 7, GQ8_0 = 8, GQ4_K = 12, GQ5_K = 13, GQ6_K = 14 };

template <int T>
struct BlockOf;
template <> struct BlockOf<GQ4_0> { static constexpr int elems = 32, bytes = 18; };
template <> struct BlockOf<GQ4_1> { static constexpr int elems = 32, bytes = 20; };
template <> struct BlockOf<GQ5_0> { static constexpr int elems = 32, bytes = 22; };
template <> struct BlockOf<GQ5_1> { static constexpr int elems = 32, bytes = 24; };
template <> struct BlockOf<GQ8_0> { static constexpr int elems = 32, bytes = 34; };
template <> struct BlockOf<GQ4_K> { static constexpr int elems = 256, bytes = 144; };
template <> struct BlockOf<GQ5_K> { static constexpr int elems = 256, bytes = 176; };
template <> struct BlockOf<GQ6_K> { static constexpr int elems = 256, bytes = 210; };

__device__ __forceinline__ float ld_f16(const uint8_t* p) { return f16_to_f32((uint16_t)(p[0] | (p[1] << 8))); }
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// utils.rs:49
__device__ __forceinline__ void scale_min_k4(int j, const uint8_t* q, float& sc, float& mn) {
  uint32_t d, m;
  if (j < 4) {
    d = q[j] & 63u;
    m = q[j + 4] & 63u;
  } else {
    d = (q[j + 4] & 0xFu) | ((uint32_t)(q[j - 4] >> 6) << 4);
    m = (uint32_t)(q[j + 4] >> 4) | ((uint32_t)(q[j] >> 6) << 4);
  }
  sc = (float)d, mn = (float)m;
}

// The 8 weights e .. e+7 (e % 8 == 0) of the block at `b` (an LDS byte address).  A run of 8 never crosses one of a format's internal
// boundaries (nibble half: 16; sub-block: 32; Q6_K scale: 16).
template <int T>
__device__ __forceinline__ void decode8(const uint8_t* b, int e, float (&v)[8]) {
  if constexpr (T == GQ4_0) {  // :175  y[j] = ((qs[j] & 0xF) - 8) * d, y[j + 16] = ((qs[j] >> 4) - 8) * d
    const float d = ld_f16(b);
    const uint8_t* qs = b + 2 + (e & 15);
    const int sh = e >= 16 ? 4 : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)((int)((qs[i] >> sh) & 0xF) - 8) * d;
  } else if constexpr (T == GQ4_1) {  // :341  y = x * d + m
    const float d = ld_f16(b), m = ld_f16(b + 2);
    const uint8_t* qs = b + 4 + (e & 15);
    const int sh = e >= 16 ? 4 : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float t = (float)((qs[i] >> sh) & 0xF) * d;
      v[i] = t + m;
    }
  } else if constexpr (T == GQ5_0 || T == GQ5_1) {  // :440 / :547  bit j of qh is the 5th bit of y[j], bit j + 16 of y[j + 16]
    const float d = ld_f16(b);
    const float m = T == GQ5_1 ? ld_f16(b + 2) : 0.f;
    const uint8_t* qhp = b + (T == GQ5_1 ? 4 : 2);
    const uint32_t qh = ld_u32(qhp) >> e;  // (element e + i of the block: bit e + i in both halves)
    const uint8_t* qs = qhp + 4 + (e & 15);
    const int sh = e >= 16 ? 4 : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int x = (int)(((qs[i] >> sh) & 0xF) | (((qh >> i) & 1u) << 4));
      if constexpr (T == GQ5_0) {
        v[i] = (float)(x - 16) * d;
      } else {
        const float t = (float)x * d;
        v[i] = t + m;
      }
    }
  } else if constexpr (T == GQ8_0) {  // :580
    const float d = ld_f16(b);
    const int8_t* qs = reinterpret_cast<const int8_t*>(b + 2 + e);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)qs[i] * d;
  } else if constexpr (T == GQ4_K || T == GQ5_K) {  // :1568 / :1872  64 weights per 32 bytes of qs: low nibbles, then high nibbles
    const float d = ld_f16(b), mn = ld_f16(b + 2);
    const int g = e >> 6, hi = (e >> 5) & 1, l0 = e & 31;
    float sc, m;
    scale_min_k4(2 * g + hi, b + 4, sc, m);
    const float d1 = d * sc;
    const float m1 = mn * m;
    const uint8_t* qs = b + (T == GQ5_K ? 48 : 16) + g * 32 + l0;
    const uint8_t* qh = b + 16 + l0;  // (Q5_K only)
    const int sh = hi ? 4 : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float q = (float)((qs[i] >> sh) & 0xF);
      if constexpr (T == GQ5_K) q = q + (((qh[i] >> (2 * g + hi)) & 1) ? 16.f : 0.f);
      const float t = d1 * q;
      v[i] = t - m1;
    }
  } else {  // Q6_K :2147  per 128 weights: 64 bytes of ql (low | high nibbles), 32 of qh (2 bits each), 8 scales
    const float d = ld_f16(b + 208);
    const int idx = e >> 7, quarter = (e >> 5) & 3, l0 = e & 31;
    const uint8_t* ql = b + 64 * idx + (quarter & 1) * 32 + l0;
    const uint8_t* qh = b + 128 + 32 * idx + l0;
    const float sc = (float)reinterpret_cast<const int8_t*>(b + 192)[8 * idx + (l0 >> 4) + 2 * quarter];
    const float ds = d * sc;
    const int shl = (quarter >> 1) * 4, shh = 2 * quarter;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = (int)(((ql[i] >> shl) & 0xF) | (((qh[i] >> shh) & 3) << 4)) - 32;
      v[i] = ds * (float)q;
    }
  }
}

constexpr int GROUP = 8192;  // weights per workgroup: 256 lanes x 8 weights x 4 passes
constexpr int THREADS = 256;

// `src`: the tensor's first block (2-byte aligned), nblocks blocks.  Workgroup w decodes blocks [w * GROUP / elems, ...).
template <int T, bool BF16>
__global__ __launch_bounds__(THREADS) void gguf_dequant_kernel(const uint8_t* __restrict src, int64_t nblocks, void* __restrict out, int out_aligned) {
  constexpr int BE = BlockOf<T>::elems, BB = BlockOf<T>::bytes, BPG = GROUP / BE;
  constexpr int LDS_VEC = (BPG * BB + 15) / 16 + 2;  // the group's bytes plus a ragged head and tail
  __shared__ uint4 lds[LDS_VEC];
  const int64_t blk0 = (int64_t)blockIdx.x * BPG;
  const int nb = (int)std::min<int64_t>(BPG, nblocks - blk0);
  if (nb <= 0) return;
  const uintptr_t t0 = reinterpret_cast<uintptr_t>(src), t1 = t0 + (uint64_t)nblocks * BB;  // the tensor's bytes [t0, t1)
  const uintptr_t g0 = t0 + (uint64_t)blk0 * BB, g1 = g0 + (uint64_t)nb * BB;               // this group's bytes
  const uintptr_t a0 = g0 & ~(uintptr_t)15;
  const int nvec = (int)((g1 - a0 + 15) >> 4);  // <= LDS_VEC: (BPG * BB + 15 + 15) / 16
  for (int c = threadIdx.x; c < nvec; c += THREADS) {
    const uintptr_t a = a0 + ((uintptr_t)c << 4);
    uint4 q;
    if (a >= t0 && a + 16 <= t1) {
      q = *reinterpret_cast<const uint4*>(a);
    } else {  // straddles the tensor's first or last byte: its 2-byte words that lie inside (t0 and the block sizes are even)
      uint16_t h[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uintptr_t p = a + 2 * k;
        h[k] = (p >= t0 && p + 2 <= t1) ? *reinterpret_cast<const uint16_t*>(p) : (uint16_t)0;
      }
      __builtin_memcpy(&q, h, 16);
    }
    lds[c] = q;
  }
  __syncthreads();
  const uint8_t* base = reinterpret_cast<const uint8_t*>(lds) + (int)(g0 - a0);
  const int nel = nb * BE;
  const int64_t o0 = blk0 * BE;
  for (int e = threadIdx.x * 8; e < nel; e += THREADS * 8) {
    float v[8];
    decode8<T>(base + (e / BE) * BB, e % BE, v);
    if constexpr (BF16) {
      bf16_t* o = reinterpret_cast<bf16_t*>(out) + o0 + e;
      if (out_aligned) {
        *reinterpret_cast<uint4*>(o) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = f32_to_bf16(v[i]);
      }
    } else {
      float* o = reinterpret_cast<float*>(out) + o0 + e;
      if (out_aligned) {
        reinterpret_cast<float4*>(o)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(o)[1] = make_float4(v[4], v[5], v[6], v[7]);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = v[i];
      }
    }
  }
}

template <int T>
int launch_t(const void* blocks, int64_t n_elems, void* out, bool bf16, hipStream_t s) {
  constexpr int BE = BlockOf<T>::elems;
  const int64_t nblocks = n_elems / BE;
  const int64_t grid = cdiv64(n_elems, GROUP);
  if (grid >= (1ll << 31)) return fail(FMI_ERR_UNSUPPORTED, "gguf_dequantize: tensor too large");
  const int aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  if (bf16) hipLaunchKernelGGL((gguf_dequant_kernel<T, true>), dim3((unsigned)grid), dim3(THREADS), 0, s, (const uint8_t*)blocks, nblocks, out, aligned);
  else hipLaunchKernelGGL((gguf_dequant_kernel<T, false>), dim3((unsigned)grid), dim3(THREADS), 0, s, (const uint8_t*)blocks, nblocks, out, aligned);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

}  // namespace
}  // namespace fmi

using namespace fmi;

static const char* gguf_type_name(int t) {
  static const char* const kNames[] = {"F32",  "F16",  "Q4_0", "Q4_1", "Q4_2",    "Q4_3",    "Q5_0",   "Q5_1",  "Q8_0",   "Q8_1",    "Q2_K",    "Q3_K",
                                       "Q4_K", "Q5_K", "Q6_K", "Q8_K", "IQ2_XXS", "IQ2_XS",  "IQ3_XXS", "IQ1_S", "IQ4_NL", "IQ3_S",   "IQ2_S",   "IQ4_XS",
                                       "I8",   "I16",  "I32",  "I64",  "F64",     "IQ1_M",   "BF16"};
  return t >= 0 && t < (int)(sizeof(kNames) / sizeof(kNames[0])) ? kNames[t] : "unknown";
}

extern "C" int fmi_gguf_block_info(int ggml_type, int* block_elems, int* block_bytes) {
  int e = 0, b = 0;
  switch (ggml_type) {
    case GQ4_0: e = 32, b = 18; break;
    case GQ4_1: e = 32, b = 20; break;
    case GQ5_0: e = 32, b = 22; break;
    case GQ5_1: e = 32, b = 24; break;
    case GQ8_0: e = 32, b = 34; break;
    case GQ4_K: e = 256, b = 144; break;
    case GQ5_K: e = 256, b = 176; break;
    case GQ6_K: e = 256, b = 210; break;
    default:
      return fail(FMI_ERR_UNSUPPORTED, std::string("gguf: ggml type ") + std::to_string(ggml_type) + " (" + gguf_type_name(ggml_type) +
                                           ") is not a supported block format (Q4_0 Q4_1 Q5_0 Q5_1 Q8_0 Q4_K Q5_K Q6_K)");
  }
  if (block_elems) *block_elems = e;
  if (block_bytes) *block_bytes = b;
  return FMI_OK;
}

extern "C" int fmi_gguf_dequantize(int ggml_type, const void* blocks, int64_t n_elems, void* out, fmi_dtype out_dtype, void* stream_) {
  const hipStream_t stream = (hipStream_t)stream_;
  int be = 0, bb = 0;
  FMI_TRY(fmi_gguf_block_info(ggml_type, &be, &bb));
  if (out_dtype != FMI_BF16 && out_dtype != FMI_F32) return fail(FMI_ERR_INVALID, "gguf_dequantize: out_dtype must be BF16 or F32");
  if (n_elems < 0 || n_elems % be) return fail(FMI_ERR_INVALID, "gguf_dequantize: n_elems must be a multiple of the block's " + std::to_string(be) + " elements");
  if (n_elems == 0) return FMI_OK;
  if (!blocks || !out) return fail(FMI_ERR_INVALID, "gguf_dequantize: null argument");
  if (reinterpret_cast<uintptr_t>(blocks) & 1) return fail(FMI_ERR_INVALID, "gguf_dequantize: blocks must be 2-byte aligned");
  if (reinterpret_cast<uintptr_t>(out) & (out_dtype == FMI_BF16 ? 1 : 3)) return fail(FMI_ERR_INVALID, "gguf_dequantize: out is not aligned to its element type");
  const bool bf = out_dtype == FMI_BF16;
  switch (ggml_type) {
    case GQ4_0: return launch_t<GQ4_0>(blocks, n_elems, out, bf, stream);
    case GQ4_1: return launch_t<GQ4_1>(blocks, n_elems, out, bf, stream);
    case GQ5_0: return launch_t<GQ5_0>(blocks, n_elems, out, bf, stream);
    case GQ5_1: return launch_t<GQ5_1>(blocks, n_elems, out, bf, stream);
    case GQ8_0: return launch_t<GQ8_0>(blocks, n_elems, out, bf, stream);
    case GQ4_K: return launch_t<GQ4_K>(blocks, n_elems, out, bf, stream);
    case GQ5_K: return launch_t<GQ5_K>(blocks, n_elems, out, bf, stream);
    default: return launch_t<GQ6_K>(blocks, n_elems, out, bf, stream);
  }
}
