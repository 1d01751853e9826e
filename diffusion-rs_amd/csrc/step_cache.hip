// step_cache.hip — the element-wise passes of the first-block step cache (fmi_flux_denoise_cached) over the f32 image stream:
//   residual + distance : r = X1 - X0, X0 <- X1 (the copy a computed step needs for its delta), per-workgroup partials of sum|r - r_ref| and sum|r_ref|
//   distance_final      : the partials of one sample -> (num, den) in double, fixed order
//   delta / apply       : D = XF - X1copy  /  XF = X1 + D, per-sample row strides (XF lives in the joint stream, X1 in the image stream)
// Determinism: no floating-point atomics.  Element e of a sample always belongs to quad e / 4 of workgroup e / SC_CHUNK and to the same thread of it, whatever
// the batch size, the pointer alignment or the access width (the scalar kernel walks the very quads of the 16-byte one); a thread adds its quads in ascending
// order, a wave reduces by the xor butterfly, the four waves are added in index order, and the final pass adds the partials in a fixed strided order in double.
// The sums of one sample therefore depend on its values and on S' * D alone: the same bits from run to run and for any B.
#include "common.h"

namespace fmi {

namespace {
constexpr int SC_THREADS = 256, SC_ITERS = 8;
constexpr int64_t SC_CHUNK = (int64_t)SC_THREADS * 4 * SC_ITERS;  // elements of one sample per workgroup

template <bool V4>
__device__ __forceinline__ void load4(const float* p, int64_t left, float (&v)[4]) {
  if constexpr (V4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < left ? p[k] : 0.f;
  }
}
template <bool V4>
__device__ __forceinline__ void store4(float* p, int64_t left, const float (&v)[4]) {
  if constexpr (V4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < left) p[k] = v[k];
  }
}

// grid (groups, B).  x1: the image stream after double block 0 (sample stride x1_bs); x0: in X0, out the copy of X1; r_ref null: no distance (partials are zero).
// x0 is read and written at the same elements by the same thread only.
template <bool V4>
__global__ __launch_bounds__(SC_THREADS) void sc_residual_kernel(const float* __restrict__ x1, int64_t x1_bs, float* x0, const float* __restrict__ r_ref,
                                                                 float* __restrict__ r, float* __restrict__ part, int64_t n) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const float* x1b = x1 + (int64_t)b * x1_bs;
  float* x0b = x0 + (int64_t)b * n;
  float* rb = r + (int64_t)b * n;
  const float* refb = r_ref ? r_ref + (int64_t)b * n : nullptr;
  const int64_t base = (int64_t)blockIdx.x * SC_CHUNK;
  float num = 0.f, den = 0.f;
#pragma unroll 2
  for (int it = 0; it < SC_ITERS; ++it) {
    const int64_t e = base + ((int64_t)it * SC_THREADS + tid) * 4;
    if (e >= n) break;
    const int64_t left = n - e;
    float a[4], z[4], d[4];
    load4<V4>(x1b + e, left, a);
    load4<V4>(x0b + e, left, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = a[k] - z[k];
    store4<V4>(rb + e, left, d);
    store4<V4>(x0b + e, left, a);
    if (refb) {
      float f[4];
      load4<V4>(refb + e, left, f);  // (beyond n: d = f = 0, which adds +0 to both sums)
      num += (fabsf(d[0] - f[0]) + fabsf(d[1] - f[1])) + (fabsf(d[2] - f[2]) + fabsf(d[3] - f[3]));
      den += (fabsf(f[0]) + fabsf(f[1])) + (fabsf(f[2]) + fabsf(f[3]));
    }
  }
  __shared__ float red[2][SC_THREADS / 64];
  num = wave_sum(num), den = wave_sum(den);
  if ((tid & 63) == 0) red[0][tid >> 6] = num, red[1][tid >> 6] = den;
  __syncthreads();
  if (tid < 2) part[((int64_t)b * gridDim.x + blockIdx.x) * 2 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// grid (B): the `groups` partial pairs of sample b -> sums[2 b] = num, sums[2 b + 1] = den (double)
__global__ __launch_bounds__(SC_THREADS) void sc_final_kernel(const float* __restrict__ part, int groups, double* __restrict__ sums) {
  const int b = blockIdx.x, tid = threadIdx.x;
  double num = 0, den = 0;
  for (int g = tid; g < groups; g += SC_THREADS) {
    num += (double)part[((int64_t)b * groups + g) * 2];
    den += (double)part[((int64_t)b * groups + g) * 2 + 1];
  }
  __shared__ double red[2][SC_THREADS];
  red[0][tid] = num, red[1][tid] = den;
  __syncthreads();
  for (int o = SC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[0][tid] += red[0][tid + o], red[1][tid] += red[1][tid + o];
    __syncthreads();
  }
  if (tid < 2) sums[2 * b + tid] = red[tid][0];
}

// out = a + sign * c over n elements per sample, every operand with its own sample stride; grid (x, B), grid-stride over quads.  out may be a or c (same index).
template <bool V4, bool SUB>
__global__ __launch_bounds__(SC_THREADS) void sc_combine_kernel(const float* a, int64_t a_bs, const float* c, int64_t c_bs, float* out, int64_t out_bs, int64_t n) {
  const int b = blockIdx.y;
  const float* ab = a + (int64_t)b * a_bs;
  const float* cb = c + (int64_t)b * c_bs;
  float* ob = out + (int64_t)b * out_bs;
  const int64_t quads = (n + 3) / 4;
  for (int64_t q = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * SC_THREADS) {
    const int64_t e = q * 4, left = n - e;
    float x[4], y[4], o[4];
    load4<V4>(ab + e, left, x);
    load4<V4>(cb + e, left, y);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = SUB ? x[k] - y[k] : x[k] + y[k];
    store4<V4>(ob + e, left, o);
  }
}

template <bool SUB>
int launch_combine(const float* a, int64_t a_bs, const float* c, int64_t c_bs, float* out, int64_t out_bs, int B, int64_t n, hipStream_t stream) {
  if (B <= 0 || n <= 0) return FMI_OK;
  const bool v4 = n % 4 == 0 && a_bs % 4 == 0 && c_bs % 4 == 0 && out_bs % 4 == 0 && aligned16(a) && aligned16(c) && aligned16(out);
  const dim3 grid((unsigned)std::min<int64_t>(cdiv64(cdiv64(n, 4), SC_THREADS), 2048), (unsigned)B);
  if (v4) hipLaunchKernelGGL((sc_combine_kernel<true, SUB>), grid, dim3(SC_THREADS), 0, stream, a, a_bs, c, c_bs, out, out_bs, n);
  else hipLaunchKernelGGL((sc_combine_kernel<false, SUB>), grid, dim3(SC_THREADS), 0, stream, a, a_bs, c, c_bs, out, out_bs, n);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
}  // namespace

int step_cache_groups(int64_t n) { return (int)cdiv64(n, SC_CHUNK); }

int launch_step_cache_residual(const float* x1, int64_t x1_bs, float* x0, const float* r_ref, float* r, float* part, double* sums, int B, int64_t n,
                               hipStream_t stream) {
  if (B <= 0 || n <= 0) return fail(FMI_ERR_INVALID, "step cache: empty image stream");
  if (cdiv64(n, SC_CHUNK) > (1 << 24)) return fail(FMI_ERR_UNSUPPORTED, "step cache: image stream too long");
  const int groups = step_cache_groups(n);
  const bool v4 = n % 4 == 0 && x1_bs % 4 == 0 && aligned16(x1) && aligned16(x0) && aligned16(r) && (!r_ref || aligned16(r_ref));
  const dim3 grid((unsigned)groups, (unsigned)B);
  if (v4) hipLaunchKernelGGL(sc_residual_kernel<true>, grid, dim3(SC_THREADS), 0, stream, x1, x1_bs, x0, r_ref, r, part, n);
  else hipLaunchKernelGGL(sc_residual_kernel<false>, grid, dim3(SC_THREADS), 0, stream, x1, x1_bs, x0, r_ref, r, part, n);
  FMI_LAUNCH_CHECK();
  if (r_ref) {
    hipLaunchKernelGGL(sc_final_kernel, dim3(B), dim3(SC_THREADS), 0, stream, part, groups, sums);
    FMI_LAUNCH_CHECK();
  }
  return FMI_OK;
}

int launch_step_cache_delta(const float* xf, int64_t xf_bs, const float* x1copy, float* delta, int B, int64_t n, hipStream_t stream) {
  return launch_combine<true>(xf, xf_bs, x1copy, n, delta, n, B, n, stream);
}
int launch_step_cache_apply(const float* x1, int64_t x1_bs, const float* delta, float* xf, int64_t xf_bs, int B, int64_t n, hipStream_t stream) {
  return launch_combine<false>(x1, x1_bs, delta, n, xf, xf_bs, B, n, stream);
}

}  // namespace fmi
