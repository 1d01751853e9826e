// controlnet.hip — the residual injection of a FLUX ControlNet (diffusers' FluxTransformer2DModel.forward(controlnet_block_samples=,
// controlnet_single_block_samples=)): after a block of the main model, `rows` rows of every sample of its f32 stream take a scaled sample of the ControlNet,
//   x[b, r, :] = x[b, r, :] + c * f32(src[b, r, :])          one __fmul_rn and one __fadd_rn per element, never contracted into an fma
// x is addressed with a batch stride, so the image stream of the double blocks ((B*S, D) contiguous) and the image rows [T, T + S) of every L-row sample of the
// single blocks' joint stream are the same kernel.  The ControlNet's own input sum x_embedder(img) + controlnet_x_embedder(cond) is the f32-source form at c = 1.
#include "common.h"

using namespace fmi;

namespace {
__device__ __forceinline__ float src_f32(float v) { return v; }
__device__ __forceinline__ float src_f32(bf16_t v) { return bf16_to_f32(v); }
__device__ __forceinline__ float add_scaled(float x, float c, float v) { return __fadd_rn(x, __fmul_rn(c, v)); }

// per: elements per sample (rows * D); sample b of x at x + b * x_bs, of src at src + b * per.  V8: one item = 8 elements — two 16-B words of x, and one (bf16) or
// two (f32) of src — which needs per % 8 == 0, x_bs % 4 == 0 and both bases on 16 bytes; else one element per item, any alignment.  Grid-stride over the items.
template <typename T, bool V8>
__global__ __launch_bounds__(256) void add_scaled_rows_kernel(float* __restrict__ x, int64_t x_bs, const T* __restrict__ src, int64_t per, int64_t items, float c) {
  const int64_t per_items = V8 ? per / 8 : per;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / per_items, e = (i % per_items) * (V8 ? 8 : 1);
    float* xp = x + b * x_bs + e;
    const T* sp = src + b * per + e;
    if constexpr (!V8) {
      xp[0] = add_scaled(xp[0], c, src_f32(sp[0]));
    } else {
      float4 lo = *reinterpret_cast<const float4*>(xp), hi = *reinterpret_cast<const float4*>(xp + 4);
      float v[8];
      if constexpr (sizeof(T) == 2) {
        const uint4 s = *reinterpret_cast<const uint4*>(sp);
        const uint32_t w[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) v[2 * k] = __uint_as_float(w[k] << 16), v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
      } else {
        const float4 a = *reinterpret_cast<const float4*>(sp), d = *reinterpret_cast<const float4*>(sp + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = d.x, v[5] = d.y, v[6] = d.z, v[7] = d.w;
      }
      lo.x = add_scaled(lo.x, c, v[0]), lo.y = add_scaled(lo.y, c, v[1]), lo.z = add_scaled(lo.z, c, v[2]), lo.w = add_scaled(lo.w, c, v[3]);
      hi.x = add_scaled(hi.x, c, v[4]), hi.y = add_scaled(hi.y, c, v[5]), hi.z = add_scaled(hi.z, c, v[6]), hi.w = add_scaled(hi.w, c, v[7]);
      *reinterpret_cast<float4*>(xp) = lo;
      *reinterpret_cast<float4*>(xp + 4) = hi;
    }
  }
}
template <typename T>
int launch_add_scaled_rows_t(float* x, int64_t x_bs, const T* src, int B, int64_t rows, int D, float c, hipStream_t stream) {
  if (!x || !src || B < 0 || rows < 0 || D <= 0) return fail(FMI_ERR_INVALID, "add_scaled_rows: null pointer or negative size");
  const int64_t per = rows * D;
  if (x_bs < per) return fail(FMI_ERR_INVALID, "add_scaled_rows: the batch stride of x must be at least rows * D (the samples' rows must not overlap)");
  if (B == 0 || per == 0) return FMI_OK;
  if (per % 8 == 0 && x_bs % 4 == 0 && aligned16(x) && aligned16(src)) {
    const int64_t items = (int64_t)B * (per / 8);
    hipLaunchKernelGGL((add_scaled_rows_kernel<T, true>), map_grid(items), dim3(256), 0, stream, x, x_bs, src, per, items, c);
  } else {
    const int64_t items = (int64_t)B * per;
    hipLaunchKernelGGL((add_scaled_rows_kernel<T, false>), map_grid(items), dim3(256), 0, stream, x, x_bs, src, per, items, c);
  }
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
}  // namespace

namespace fmi {
int launch_add_scaled_rows_bf16(float* x, int64_t x_bs, const bf16_t* src, int B, int64_t rows, int D, float c, hipStream_t stream) {
  return launch_add_scaled_rows_t(x, x_bs, src, B, rows, D, c, stream);
}
int launch_add_scaled_rows_f32(float* x, int64_t x_bs, const float* src, int B, int64_t rows, int D, float c, hipStream_t stream) {
  return launch_add_scaled_rows_t(x, x_bs, src, B, rows, D, c, stream);
}
}  // namespace fmi

extern "C" int fmi_add_scaled_rows_bf16(float* x_f32, int64_t x_batch_stride, const void* src_bf16, int B, int64_t rows, int D, float scale, void* stream) {
  return launch_add_scaled_rows_bf16(x_f32, x_batch_stride, (const bf16_t*)src_bf16, B, rows, D, scale, (hipStream_t)stream);
}
