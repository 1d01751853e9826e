// f8_dequant.hip — 8-bit float codes (OCP e4m3fn / e5m2: the safetensors dtypes F8_E4M3 / F8_E5M2 of single-file FLUX checkpoints) into the
// bf16 / f32 operands the GEMMs read.
//
// Semantics (this library's own, include/flux_mi355x.h): y = f32(code), exact — every code of either format is an f32 value —, then
// y = y * scale as ONE rounded f32 multiply, then for bf16 output ONE RNE rounding.  The file is compiled with contraction off like
// gguf_dequant.hip, so the multiply and the rounding stay two steps; scale == 1 gives the code's value exactly.  NaN codes (e4m3 0x7f /
// 0xff, e5m2 0x7d .. 0x7f / 0xfd .. 0xff) give a NaN of unspecified payload, e5m2's infinities stay infinities.  The conversion is the
// hardware's (v_cvt_pk_f32_fp8 / v_cvt_pk_f32_bf8: gfx950's formats are the OCP ones, as fp8.hip relies on).
//
// Shape: memory-bound, 1 B in and 2 B (bf16) or 4 B (f32) out per weight.  `codes` may start at any byte: the at most 15 codes before the
// first 16-byte boundary and the at most 15 after the last whole 16-byte piece are converted one by one by the first workgroup; in
// between each lane reads 16 aligned bytes and writes 32 (bf16) in a grid-stride loop under the glue kernels' grid cap.  The bits are
// the same on either path.  Indexes are 64-bit.
#include <algorithm>
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

namespace fmi {
namespace {

enum F8Format { F8_E4M3 = 1, F8_E5M2 = 2 };
typedef float f8_f32x2 __attribute__((ext_vector_type(2)));

constexpr int THREADS = 256;

// the four codes of `w` (byte 0 first)
template <int FMT>
__device__ __forceinline__ void decode4(uint32_t w, float scale, float (&v)[4]) {
  f8_f32x2 lo, hi;
  if constexpr (FMT == F8_E4M3) {
    lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  } else {
    lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true);
  }
  v[0] = lo.x * scale, v[1] = lo.y * scale, v[2] = hi.x * scale, v[3] = hi.y * scale;
}

template <bool BF16>
__device__ __forceinline__ void store1(void* out, int64_t e, float y) {
  if constexpr (BF16) reinterpret_cast<bf16_t*>(out)[e] = f32_to_bf16(y);
  else reinterpret_cast<float*>(out)[e] = y;
}

// codes [0, head) and [head + 16 * nvec, n) one by one (workgroup 0), codes [head, head + 16 * nvec) 16 per lane: src + head is 16-byte aligned.
// out_aligned: out + head elements is 16-byte aligned (vector stores), else element stores.
template <int FMT, bool BF16>
__global__ __launch_bounds__(THREADS) void f8_dequant_kernel(const uint8_t* __restrict src, int64_t n, float scale, void* __restrict out, int head, int64_t nvec,
                                                            int out_aligned) {
  if (blockIdx.x == 0 && threadIdx.x < 32) {
    const int t = threadIdx.x;
    const int64_t e = t < 16 ? (int64_t)t : (int64_t)head + 16 * nvec + (t - 16);
    if (t < 16 ? t < head : e < n) {
      float v[4];
      decode4<FMT>((uint32_t)src[e], scale, v);
      store1<BF16>(out, e, v[0]);
    }
  }
  const uint4* __restrict body = reinterpret_cast<const uint4*>(src + head);
  for (int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x; c < nvec; c += (int64_t)gridDim.x * THREADS) {
    const uint4 q = body[c];
    float v[4][4];
    decode4<FMT>(q.x, scale, v[0]);
    decode4<FMT>(q.y, scale, v[1]);
    decode4<FMT>(q.z, scale, v[2]);
    decode4<FMT>(q.w, scale, v[3]);
    const int64_t e = (int64_t)head + 16 * c;
    if constexpr (BF16) {
      bf16_t* o = reinterpret_cast<bf16_t*>(out) + e;
      if (out_aligned) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
          reinterpret_cast<uint4*>(o)[i] = make_uint4(pack_bf16x2(v[2 * i][0], v[2 * i][1]), pack_bf16x2(v[2 * i][2], v[2 * i][3]), pack_bf16x2(v[2 * i + 1][0], v[2 * i + 1][1]),
                                                      pack_bf16x2(v[2 * i + 1][2], v[2 * i + 1][3]));
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = f32_to_bf16(v[i / 4][i % 4]);
      }
    } else {
      float* o = reinterpret_cast<float*>(out) + e;
      if (out_aligned) {
#pragma unroll
        for (int i = 0; i < 4; ++i) reinterpret_cast<float4*>(o)[i] = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = v[i / 4][i % 4];
      }
    }
  }
}

template <int FMT, bool BF16>
int launch_t(const void* codes, int64_t n, float scale, void* out, hipStream_t s) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(codes);
  const int head = (int)std::min<int64_t>(n, (int64_t)((16 - (a & 15)) & 15));
  const int64_t nvec = (n - head) / 16;
  const unsigned grid = std::max(1u, map_grid(nvec).x);  // (workgroup 0 also takes the head and the tail)
  const int out_aligned = ((reinterpret_cast<uintptr_t>(out) + (uintptr_t)head * (BF16 ? 2 : 4)) & 15) == 0;
  hipLaunchKernelGGL((f8_dequant_kernel<FMT, BF16>), dim3(grid), dim3(THREADS), 0, s, (const uint8_t*)codes, n, scale, out, head, nvec, out_aligned);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

}  // namespace
}  // namespace fmi

using namespace fmi;

extern "C" int fmi_f8_dequantize(int format, const void* codes, int64_t n_elems, float scale, void* out, fmi_dtype out_dtype, void* stream_) {
  const hipStream_t stream = (hipStream_t)stream_;
  if (format != F8_E4M3 && format != F8_E5M2) return fail(FMI_ERR_INVALID, "f8_dequantize: format must be 1 (OCP e4m3fn) or 2 (OCP e5m2), got " + std::to_string(format));
  if (out_dtype != FMI_BF16 && out_dtype != FMI_F32) return fail(FMI_ERR_INVALID, "f8_dequantize: out_dtype must be BF16 or F32");
  if (!std::isfinite(scale) || !(scale > 0.f)) return fail(FMI_ERR_INVALID, "f8_dequantize: scale must be finite and > 0");
  if (n_elems < 0) return fail(FMI_ERR_INVALID, "f8_dequantize: n_elems is negative");
  if (n_elems == 0) return FMI_OK;
  if (!codes || !out) return fail(FMI_ERR_INVALID, "f8_dequantize: null argument");
  if (reinterpret_cast<uintptr_t>(out) & (out_dtype == FMI_BF16 ? 1 : 3)) return fail(FMI_ERR_INVALID, "f8_dequantize: out is not aligned to its element type");
  if (format == F8_E4M3) return out_dtype == FMI_BF16 ? launch_t<F8_E4M3, true>(codes, n_elems, scale, out, stream) : launch_t<F8_E4M3, false>(codes, n_elems, scale, out, stream);
  return out_dtype == FMI_BF16 ? launch_t<F8_E5M2, true>(codes, n_elems, scale, out, stream) : launch_t<F8_E5M2, false>(codes, n_elems, scale, out, stream);
}
