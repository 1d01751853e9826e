// quant_kinds.h — the storage kinds of a quantised Linear, and the one table from kind to the launcher that expands it into bf16.  The kernels are in
// bnb_dequant.hip, gguf_dequant.hip and f8_dequant.hip; nothing else in the library names their launchers.
#pragma once

#include "common.h"

namespace fmi {

// What a Linear (a part of a fused matrix) was loaded as, and — when every part of a matrix holds the same kind — the q_type its GEMM runs on.
//   PS_FP4 / PS_NF4            bitsandbytes 4-bit codes + f32 absmax per blocksize weights (fmi_*_set_linear_bnb4)
//   PS_INT8                    LLM.int8: int8 (N, K) + f32 SCB per row (fmi_*_set_linear_int8)
//   PS_GGUF0 + ggml type id    ggml blocks, types 2 .. 14 (fmi_flux_set_linear_gguf)
//   PS_F8_E4M3 / PS_F8_E5M2    OCP e4m3fn / e5m2 codes with one f32 scale (fmi_flux_set_linear_f8)
enum PartState : uint8_t { PS_UNSET = 0, PS_FP4 = 1, PS_NF4 = 2, PS_INT8 = 3, PS_GGUF0 = 16, PS_GGUF_END = 48, PS_F8_E4M3 = 48, PS_F8_E5M2 = 49, PS_DENSE = 100 };
inline bool is_gguf(int kind) { return kind >= PS_GGUF0 && kind < PS_GGUF_END; }
inline bool is_f8(int kind) { return kind == PS_F8_E4M3 || kind == PS_F8_E5M2; }
// kinds that have no fused dequant-GEMM: always expanded, once or per call
inline bool is_codes(int kind) { return is_gguf(kind) || is_f8(kind); }

// bf16 out = w_i8 * SCB[row] / 127 (dequant.cu:205-214) on `stream` (bnb_dequant.hip)
int launch_dequant_int8_scb_bf16(const int8_t* w, const float* scb, bf16_t* out, int col, int64_t n, hipStream_t stream);

// n weights of `kind`, device resident at `src`, -> bf16 at `dst` on `stream`.  scales: the f32 absmax per `blocksize` weights (fp4, nf4) or the SCB per
// row of K weights (int8); scale: the one factor of 8-bit float codes; the other kinds ignore them.  fp4 / nf4 count in 32 bits: n < 2^31 is the caller's.
inline int dequant_to_bf16(int kind, int blocksize, const void* src, const float* scales, float scale, int K, int64_t n, bf16_t* dst, hipStream_t stream) {
  if (kind == PS_INT8) return launch_dequant_int8_scb_bf16(static_cast<const int8_t*>(src), scales, dst, K, n, stream);
  if (is_f8(kind)) return fmi_f8_dequantize(kind == PS_F8_E4M3 ? 1 : 2, src, n, scale, dst, FMI_BF16, stream);
  if (is_gguf(kind)) return fmi_gguf_dequantize(kind - PS_GGUF0, src, n, dst, FMI_BF16, stream);
  if (kind == PS_NF4) dequantize_blockwise_bf16_nf4(nullptr, static_cast<const uint8_t*>(src), scales, dst, blocksize, (int)n, stream);
  else dequantize_blockwise_bf16_fp4(nullptr, static_cast<const uint8_t*>(src), scales, dst, blocksize, (int)n, stream);
  return FMI_OK;
}

}  // namespace fmi
