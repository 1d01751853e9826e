// small_ops.hip — the non-GEMM odds and ends of Flux::forward / FluxPipeline::forward:
//   gemv            : M<=8 row Linear (MlpEmbedder, Modulation1/2, LastLayer.ada_ln) — pure weight
//                     streaming, one wave per output row, 16-B loads  (model.rs:178-183,244-299,695-698)
//   timestep_embedding (model.rs:104-122),
//   pack/unpack latents (pipelines/flux/sampling.rs:26-48,61-68), u8 post-process (flux/mod.rs:332),
//   Philox N(0,1) latents (seedable replacement of get_noise, flux/sampling.rs:5-14), dtype casts,
//   image-to-image / inpainting glue (no counterpart in the reference; the flow-matching forms of diffusers' FluxImg2ImgPipeline /
//   FluxInpaintPipeline): scale_noise, u8 -> f32, latent mask, encode_latents.
#include "common.h"

namespace fmi {

constexpr int GEMV_MAXM = 8;
constexpr int GEMV_ROWS_PER_WAVE = 4;

// y[m][n] (+)= sum_k act(x[m][k]) * W[n][k] + bias[n].  x staged in LDS as f32.
__global__ __launch_bounds__(256) void gemv_kernel(const float* __restrict x, const bf16_t* __restrict W, const bf16_t* __restrict bias,
                                                   float* __restrict y, int M, int N, int K, int silu_in, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // M*K
  for (int i = threadIdx.x; i < M * K; i += 256) {
    float v = x[i];
    xs[i] = silu_in ? silu(v) : v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nbase = (blockIdx.x * 4 + wave) * GEMV_ROWS_PER_WAVE;
#pragma unroll 1
  for (int rr = 0; rr < GEMV_ROWS_PER_WAVE; ++rr) {
    const int n = nbase + rr;
    if (n >= N) break;
    const bf16_t* wr = W + (int64_t)n * K;
    float acc[GEMV_MAXM];
#pragma unroll
    for (int m = 0; m < GEMV_MAXM; ++m) acc[m] = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
      const uint4 raw = *reinterpret_cast<const uint4*>(wr + k);
      const bf16_t* e = reinterpret_cast<const bf16_t*>(&raw);
      float wv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) wv[i] = bf16_to_f32(e[i]);
#pragma unroll
      for (int m = 0; m < GEMV_MAXM; ++m) {
        if (m < M) {
          const float4 a = *reinterpret_cast<const float4*>(xs + m * K + k);
          const float4 c = *reinterpret_cast<const float4*>(xs + m * K + k + 4);
          acc[m] += (a.x * wv[0] + a.y * wv[1]) + (a.z * wv[2] + a.w * wv[3]) + (c.x * wv[4] + c.y * wv[5]) + (c.z * wv[6] + c.w * wv[7]);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < GEMV_MAXM; ++m) {
      if (m < M) {
        float s = wave_sum(acc[m]);
        if (lane == 0) {
          if (bias) s += bf16_to_f32(bias[n]);
          float* o = y + (int64_t)m * N + n;
          *o = accumulate ? *o + s : s;
        }
      }
    }
  }
}

int launch_gemv(const float* x, const bf16_t* W, const bf16_t* bias, float* y, int M, int N, int K, int silu_in, int accumulate,
                hipStream_t stream) {
  if (M <= 0 || N <= 0) return FMI_OK;
  if (K % 8) return fail(FMI_ERR_INVALID, "gemv: K must be a multiple of 8");
  if ((size_t)K * sizeof(float) > 64 * 1024) return fail(FMI_ERR_UNSUPPORTED, "gemv: K too large for LDS staging");
  // The x rows of a pass are staged in LDS as f32 (<= 64 KiB) and a wave keeps GEMV_MAXM accumulators: more rows (8 samples at
  // D = 3072 are 96 KiB) run as several passes over W — each output row depends on its own x row only, so the split changes nothing.
  const int rows_per_pass = std::max(1, std::min<int>(GEMV_MAXM, (int)((64 * 1024) / ((size_t)K * sizeof(float)))));
  const int rows_per_block = 4 * GEMV_ROWS_PER_WAVE;
  for (int m0 = 0; m0 < M; m0 += rows_per_pass) {
    const int mm = std::min(rows_per_pass, M - m0);
    hipLaunchKernelGGL(gemv_kernel, dim3(cdiv(N, rows_per_block)), dim3(256), (size_t)mm * K * sizeof(float), stream, x + (size_t)m0 * K, W, bias,
                       y + (size_t)m0 * N, mm, N, K, silu_in, accumulate);
    FMI_LAUNCH_CHECK();
  }
  return FMI_OK;
}

// timestep_embedding (model.rs:104-122): t*1000; freqs = exp(-ln(1e4) * i/half) in f32; [cos, sin]
__global__ void timestep_embedding_kernel(const float* __restrict t, int dim, float* __restrict out) {
  const int b = blockIdx.x, half = dim / 2;
  const float ts = t[b] * 1000.0f;
  const float c = (float)(-9.210340371976184 / (double)half);  // -ln(10000)/half rounded to f32 (affine scalar)
  for (int i = threadIdx.x; i < half; i += blockDim.x) {
    const float fr = expf((float)i * c);
    const float a = ts * fr;
    float sn, cs;
    sincosf(a, &sn, &cs);
    out[(int64_t)b * dim + i] = cs;
    out[(int64_t)b * dim + half + i] = sn;
  }
}
int launch_timestep_embedding(const float* t, int B, int dim, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(B), dim3(128), 0, stream, t, dim, out);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

template <typename F>
__global__ void map_kernel(int64_t n, F f) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) f(i);
}

int launch_cast_to_bf16(const void* src, fmi_dtype dt, bf16_t* dst, int64_t n, hipStream_t stream) {
  if (n <= 0) return FMI_OK;
  if (dt == FMI_BF16) {
    FMI_HIP_TRY(hipMemcpyAsync(dst, src, n * 2, hipMemcpyDefault, stream));
  } else if (dt == FMI_F32) {
    const float* s = (const float*)src;
    hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, stream, n, [=] __device__(int64_t i) { dst[i] = f32_to_bf16(s[i]); });
  } else if (dt == FMI_F16) {
    const uint16_t* s = (const uint16_t*)src;
    hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, stream, n, [=] __device__(int64_t i) { dst[i] = f32_to_bf16(f16_to_f32(s[i])); });
  } else {
    return fail(FMI_ERR_INVALID, "cast_to_bf16: unsupported source dtype");
  }
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
// dst bf16 = silu(src f32): the MFMA form of the modulation projection lin(silu(vec)) (model.rs:244-259)
int launch_silu_to_bf16(const float* src, bf16_t* dst, int64_t n, hipStream_t stream) {
  if (n <= 0) return FMI_OK;
  hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, stream, n, [=] __device__(int64_t i) { dst[i] = f32_to_bf16(silu(src[i])); });
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
int launch_cast_to_f32(const void* src, fmi_dtype dt, float* dst, int64_t n, hipStream_t stream) {
  if (n <= 0) return FMI_OK;
  if (dt == FMI_F32) {
    FMI_HIP_TRY(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDefault, stream));
  } else if (dt == FMI_BF16) {
    const bf16_t* s = (const bf16_t*)src;
    hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, stream, n, [=] __device__(int64_t i) { dst[i] = bf16_to_f32(s[i]); });
  } else if (dt == FMI_F16) {
    const uint16_t* s = (const uint16_t*)src;
    hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, stream, n, [=] __device__(int64_t i) { dst[i] = f16_to_f32(s[i]); });
  } else {
    return fail(FMI_ERR_INVALID, "cast_to_f32: unsupported source dtype");
  }
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
// The weight upload of every set_tensor (common.h): host or device array -> resident bf16 / f32 (exact or RNE, the cast kernels above)
template <class T, class Cast>
static int upload_as(const void* src, fmi_dtype dtype, fmi_dtype same, int64_t n, T* dst, Cast cast) {
  if (dtype == same) {
    FMI_HIP_TRY(hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDefault));
    return FMI_OK;
  }
  const size_t esz = dtype == FMI_F32 ? 4 : 2;
  DeviceBuffer tmp;
  FMI_HIP_TRY(tmp.alloc(n * esz));
  const hipError_t e = hipMemcpy(tmp.ptr, src, n * esz, hipMemcpyDefault);
  const int rc = e == hipSuccess ? cast(tmp.ptr, dtype, dst, n, nullptr) : fail(FMI_ERR_HIP, hipGetErrorString(e));
  (void)hipDeviceSynchronize();  // the cast reads the staging block, which goes out of scope here
  return rc;
}
int upload_as_bf16(const void* src, fmi_dtype dtype, int64_t n, bf16_t* dst) { return upload_as(src, dtype, FMI_BF16, n, dst, launch_cast_to_bf16); }
int upload_as_f32(const void* src, fmi_dtype dtype, int64_t n, float* dst) { return upload_as(src, dtype, FMI_F32, n, dst, launch_cast_to_f32); }

namespace {
// a * x + t * y with a = 1 - t computed ONCE by the caller: t = 1 gives y and t = 0 gives x bit for bit (finite inputs), contracted or not
__device__ __forceinline__ float lerp_at(float a, float x, float t, float y) { return a * x + t * y; }
__device__ __forceinline__ float4 lerp_at(float a, float4 x, float t, float4 y) {
  return make_float4(lerp_at(a, x.x, t, y.x), lerp_at(a, x.y, t, y.y), lerp_at(a, x.z, t, y.z), lerp_at(a, x.w, t, y.w));
}
// V = float4 (16-B accesses) or float (any alignment, any n); grid-stride like map_kernel
template <typename V>
__global__ __launch_bounds__(256) void scale_noise_kernel(const V* __restrict__ x0, const V* __restrict__ noise, float a, float t, V* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = lerp_at(a, x0[i], t, noise[i]);
}
template <bool V4>
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d) {
  if constexpr (V4)
    *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
  else
    p[0] = a, p[1] = b, p[2] = c, p[3] = d;
}
}  // namespace

// out = (1 - t) * x0 + t * noise  (FlowMatchEulerDiscreteScheduler.scale_noise)
int launch_scale_noise(const float* x0, const float* noise, float t, int64_t n, float* out, hipStream_t stream) {
  if (n <= 0) return FMI_OK;
  const float a = 1.0f - t;
  if (n % 4 == 0 && aligned16(x0) && aligned16(noise) && aligned16(out))
    hipLaunchKernelGGL(scale_noise_kernel<float4>, map_grid(n / 4), dim3(256), 0, stream, reinterpret_cast<const float4*>(x0), reinterpret_cast<const float4*>(noise), a, t,
                       reinterpret_cast<float4*>(out), n / 4);
  else
    hipLaunchKernelGGL(scale_noise_kernel<float>, map_grid(n), dim3(256), 0, stream, x0, noise, a, t, out, n);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

namespace {
__device__ __forceinline__ float row_elem_f32(float v) { return v; }
__device__ __forceinline__ float row_elem_f32(bf16_t v) { return bf16_to_f32(v); }
// n contiguous elements of each of B samples, sample b at src + b * src_bs -> bf16 at dst + b * dst_bs (f32_to_bf16, launch_cast_to_bf16's rounding; a bf16
// source comes through unchanged).  V8: one item = 8 elements, read as 16-B words and written as one; else one element per item, any alignment, any n.
// WRAP: destination sample b reads source sample b % B_src (the state of a true-CFG evaluation, once for each half of its batch).
template <typename T, bool V8, bool WRAP>
__global__ __launch_bounds__(256) void cast_rows_bf16_kernel(const T* __restrict__ src, int64_t src_bs, bf16_t* __restrict__ dst, int64_t dst_bs, int64_t n, int64_t items,
                                                             int B_src) {
  const int64_t per = V8 ? n / 8 : n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / per, e = (i % per) * (V8 ? 8 : 1);
    const T* s = src + (WRAP ? b % B_src : b) * src_bs + e;
    bf16_t* d = dst + b * dst_bs + e;
    if constexpr (!V8) {
      d[0] = f32_to_bf16(row_elem_f32(s[0]));
    } else if constexpr (sizeof(T) == 4) {
      const float4 lo = *reinterpret_cast<const float4*>(s), hi = *reinterpret_cast<const float4*>(s + 4);
      uint4 o;
      o.x = (uint32_t)f32_to_bf16(lo.x) | ((uint32_t)f32_to_bf16(lo.y) << 16), o.y = (uint32_t)f32_to_bf16(lo.z) | ((uint32_t)f32_to_bf16(lo.w) << 16);
      o.z = (uint32_t)f32_to_bf16(hi.x) | ((uint32_t)f32_to_bf16(hi.y) << 16), o.w = (uint32_t)f32_to_bf16(hi.z) | ((uint32_t)f32_to_bf16(hi.w) << 16);
      *reinterpret_cast<uint4*>(d) = o;
    } else {
      *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
    }
  }
}
template <typename T, bool WRAP>
int launch_cast_rows_bf16_t(const T* src, int64_t src_bs, bf16_t* dst, int64_t dst_bs, int B, int64_t n, hipStream_t stream, int B_src) {
  const int64_t src_v = 16 / (int64_t)sizeof(T);  // elements of a 16-B word of the source
  if (n % 8 == 0 && src_bs % src_v == 0 && dst_bs % 8 == 0 && aligned16(src) && aligned16(dst)) {
    const int64_t items = (int64_t)B * (n / 8);
    hipLaunchKernelGGL((cast_rows_bf16_kernel<T, true, WRAP>), map_grid(items), dim3(256), 0, stream, src, src_bs, dst, dst_bs, n, items, B_src);
  } else {
    const int64_t items = (int64_t)B * n;
    hipLaunchKernelGGL((cast_rows_bf16_kernel<T, false, WRAP>), map_grid(items), dim3(256), 0, stream, src, src_bs, dst, dst_bs, n, items, B_src);
  }
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
}  // namespace
// The image-stream operand of a context evaluation is (B, S + R, C) bf16: the S state rows of every sample are cast into their places each
// step and the R context rows once per call — both are this per-sample strided copy, one launch for all B samples.  src F32 or BF16.
// B_src (0: B, every sample its own source): the source holds B_src < B samples and destination sample b takes source sample b % B_src, still in one launch.
int launch_cast_rows_bf16(const void* src, fmi_dtype dt, int64_t src_bs, bf16_t* dst, int64_t dst_bs, int B, int64_t n, hipStream_t stream, int B_src) {
  if (B <= 0 || n <= 0) return FMI_OK;
  if (B_src < 0 || B_src > B) return fail(FMI_ERR_INVALID, "cast_rows_bf16: B_src must be 0 (= B) .. B");
  if (B_src && B_src != B) {
    if (dt == FMI_F32) return launch_cast_rows_bf16_t<float, true>((const float*)src, src_bs, dst, dst_bs, B, n, stream, B_src);
    if (dt == FMI_BF16) return launch_cast_rows_bf16_t<bf16_t, true>((const bf16_t*)src, src_bs, dst, dst_bs, B, n, stream, B_src);
  }
  if (dt == FMI_F32) return launch_cast_rows_bf16_t<float, false>((const float*)src, src_bs, dst, dst_bs, B, n, stream, B);
  if (dt == FMI_BF16) return launch_cast_rows_bf16_t<bf16_t, false>((const bf16_t*)src, src_bs, dst, dst_bs, B, n, stream, B);
  return fail(FMI_ERR_INVALID, "cast_rows_bf16: the source must be F32 or BF16");
}

namespace {
// A column window of a wider bf16 matrix: row r of src (rows_src, cols), read at r % rows_src, -> dst[r * dst_ld + col0 .. + cols) (f32_to_bf16, a bf16 source
// comes through unchanged); the columns outside the window are never written.  V8: one item = 8 elements, read as 16-B words and written as one (cols, dst_ld,
// col0 multiples of 8 make every row's window 16-B aligned when the bases are); else one element per item, any alignment.
template <typename T, bool V8>
__global__ __launch_bounds__(256) void cast_cols_bf16_kernel(const T* __restrict__ src, int64_t rows_src, int cols, bf16_t* __restrict__ dst, int64_t dst_ld, int col0,
                                                             int64_t items) {
  const int per = V8 ? cols / 8 : cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / per;
    const int c = (int)(i % per) * (V8 ? 8 : 1);
    const T* s = src + (r % rows_src) * cols + c;
    bf16_t* d = dst + r * dst_ld + col0 + c;
    if constexpr (!V8) {
      d[0] = f32_to_bf16(row_elem_f32(s[0]));
    } else if constexpr (sizeof(T) == 4) {
      const float4 lo = *reinterpret_cast<const float4*>(s), hi = *reinterpret_cast<const float4*>(s + 4);
      uint4 o;
      o.x = (uint32_t)f32_to_bf16(lo.x) | ((uint32_t)f32_to_bf16(lo.y) << 16), o.y = (uint32_t)f32_to_bf16(lo.z) | ((uint32_t)f32_to_bf16(lo.w) << 16);
      o.z = (uint32_t)f32_to_bf16(hi.x) | ((uint32_t)f32_to_bf16(hi.y) << 16), o.w = (uint32_t)f32_to_bf16(hi.z) | ((uint32_t)f32_to_bf16(hi.w) << 16);
      *reinterpret_cast<uint4*>(d) = o;
    } else {
      *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
    }
  }
}
template <typename T>
int launch_cast_cols_bf16_t(const T* src, int64_t rows, int64_t rows_src, int cols, bf16_t* dst, int dst_ld, int col0, hipStream_t stream) {
  if (aligned16(src) && aligned16(dst)) {
    const int64_t items = rows * (cols / 8);
    hipLaunchKernelGGL((cast_cols_bf16_kernel<T, true>), map_grid(items), dim3(256), 0, stream, src, rows_src, cols, dst, (int64_t)dst_ld, col0, items);
  } else {
    const int64_t items = rows * cols;
    hipLaunchKernelGGL((cast_cols_bf16_kernel<T, false>), map_grid(items), dim3(256), 0, stream, src, rows_src, cols, dst, (int64_t)dst_ld, col0, items);
  }
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
}  // namespace
// The x_embedder operand of a channel-conditioned model is (B*S, 64 + Cc) bf16: the f32 state goes into columns [0, 64) every step — under true
// CFG into both halves of the batch, rows_src = Bs * S — and the conditioning into [64, 64 + Cc) once per call, each in one launch of this cast.
int launch_cast_cols_bf16(const void* src, fmi_dtype dt, int64_t rows, int64_t rows_src, int cols, bf16_t* dst, int dst_ld, int col0, hipStream_t stream) {
  if (!src || !dst || rows < 0 || rows_src <= 0 || cols <= 0 || dst_ld <= 0 || col0 < 0) return fail(FMI_ERR_INVALID, "cast_cols_bf16: bad arguments");
  if (cols % 8 || dst_ld % 8 || col0 % 8) return fail(FMI_ERR_INVALID, "cast_cols_bf16: cols, dst_ld and col0 must be multiples of 8");
  if ((int64_t)col0 + cols > dst_ld) return fail(FMI_ERR_INVALID, "cast_cols_bf16: the window [col0, col0 + cols) must lie inside a row of dst_ld");
  if (rows % rows_src) return fail(FMI_ERR_INVALID, "cast_cols_bf16: rows_src must divide rows");
  if (rows == 0) return FMI_OK;
  if (dt == FMI_F32) return launch_cast_cols_bf16_t((const float*)src, rows, rows_src, cols, dst, dst_ld, col0, stream);
  if (dt == FMI_BF16) return launch_cast_cols_bf16_t((const bf16_t*)src, rows, rows_src, cols, dst, dst_ld, col0, stream);
  return fail(FMI_ERR_INVALID, "cast_cols_bf16: the source must be F32 or BF16");
}

// y[r][n] = (y[r][n] + g[r % B][n]) + v[r % B][n]: the step-invariant terms of `vec` added in the order the accumulating GEMVs added them
int launch_add2_rows(float* y, const float* g, const float* v, int R, int B, int N, hipStream_t stream) {
  const int64_t n = (int64_t)R * N;
  if (n <= 0) return FMI_OK;
  if (g && v)
    hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, stream, n, [=] __device__(int64_t i) {
      const int64_t o = ((i / N) % B) * N + i % N;
      y[i] = (y[i] + g[o]) + v[o];
    });
  else
    hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, stream, n, [=] __device__(int64_t i) { y[i] = y[i] + v[((i / N) % B) * N + i % N]; });
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

// dst (B, rows, D) <- src (B, rows_src_per_b, D)[:, row_off:row_off+rows, :]  (or the reverse by swapping roles)
int launch_split_rows_f32(const float* src, float* dst, int B, int rows_src_per_b, int row_off, int rows, int D, hipStream_t stream) {
  for (int b = 0; b < B; ++b)
    FMI_HIP_TRY(hipMemcpyAsync(dst + (int64_t)b * rows * D, src + ((int64_t)b * rows_src_per_b + row_off) * D, (size_t)rows * D * 4,
                               hipMemcpyDeviceToDevice, stream));
  return FMI_OK;
}

namespace {
__global__ void splitk_resid_gate_kernel(const float4* __restrict__ parts, int S, const bf16_t* __restrict__ bias, const float* __restrict__ gate,
                                         int rows_per_batch, int gate_bstride, float* __restrict__ out, int ldo, int M, int N4) {
  const int64_t total = (int64_t)M * N4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / N4), n = (int)(i % N4) * 4;
    float4 v = parts[i];
    for (int s = 1; s < S; ++s) {  // fixed order: the result does not depend on the launch
      const float4 w = parts[(int64_t)s * total + i];
      v.x += w.x, v.y += w.y, v.z += w.z, v.w += w.w;
    }
    if (bias) v.x += bf16_to_f32(bias[n]), v.y += bf16_to_f32(bias[n + 1]), v.z += bf16_to_f32(bias[n + 2]), v.w += bf16_to_f32(bias[n + 3]);
    const float* g = gate + (rows_per_batch > 0 ? (int64_t)(m / rows_per_batch) * gate_bstride : 0) + n;
    float4* o = reinterpret_cast<float4*>(out + (int64_t)m * ldo + n);
    float4 x = *o;
    x.x += g[0] * v.x, x.y += g[1] * v.y, x.z += g[2] * v.z, x.w += g[3] * v.w;
    *o = x;
  }
}
}  // namespace
int launch_splitk_resid_gate(const float* parts, int S, const bf16_t* bias, const float* gate, int rows_per_batch, int gate_bstride, float* out, int ldo,
                             int M, int N, hipStream_t stream) {
  if (N % 4 || ldo % 4) return fail(FMI_ERR_INVALID, "splitk reduce: N and ldo must be multiples of 4");
  if (!gate) return fail(FMI_ERR_INVALID, "splitk reduce: needs a gate vector");
  const int64_t total = (int64_t)M * (N / 4);
  splitk_resid_gate_kernel<<<map_grid(total), 256, 0, stream>>>(reinterpret_cast<const float4*>(parts), S, bias, gate, rows_per_batch,
                                                                                                 gate_bstride, out, ldo, M, N / 4);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

}  // namespace fmi

using namespace fmi;

// ------------------------------------------------------------------ C-ABI: pipeline glue
extern "C" int fmi_pack_latents(const float* latent, int B, int C, int h, int w, float* img_out, float* img_ids_out, void* stream) {
  if (h % 2 || w % 2) return fail(FMI_ERR_INVALID, "pack_latents: h and w must be even");
  const int h2 = h / 2, w2 = w / 2, C4 = C * 4;
  const int64_t n = (int64_t)B * h2 * w2 * C4;
  hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, (hipStream_t)stream, n, [=] __device__(int64_t i) {
    const int e = (int)(i % C4);
    const int64_t tok = i / C4;
    const int j = (int)(tok % w2), ii = (int)((tok / w2) % h2), b = (int)(tok / ((int64_t)w2 * h2));
    const int c = e >> 2, ph = (e >> 1) & 1, pw = e & 1;
    img_out[i] = latent[(((int64_t)b * C + c) * h + (2 * ii + ph)) * w + (2 * j + pw)];
    if (img_ids_out && e < 3) img_ids_out[tok * 3 + e] = e == 0 ? 0.f : (e == 1 ? (float)ii : (float)j);
  });
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

extern "C" int fmi_unpack_latents(const float* img, int B, int C, int h, int w, double scale_factor, double shift_factor, float* z_out,
                                  void* stream) {
  if (h % 2 || w % 2) return fail(FMI_ERR_INVALID, "unpack_latents: h and w must be even");
  const int h2 = h / 2, w2 = w / 2, C4 = C * 4;
  const int64_t n = (int64_t)B * C * h * w;
  // (img / scale_factor) + shift_factor : two affine ops with the scalars rounded to f32 (flux/mod.rs:329)
  const float inv = (float)(1.0 / scale_factor), sh = (float)shift_factor;
  hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, (hipStream_t)stream, n, [=] __device__(int64_t i) {
    const int x = (int)(i % w), y = (int)((i / w) % h), c = (int)((i / ((int64_t)w * h)) % C), b = (int)(i / ((int64_t)w * h * C));
    const int64_t tok = ((int64_t)b * h2 + (y >> 1)) * w2 + (x >> 1);
    const float v = img[tok * C4 + (c * 2 + (y & 1)) * 2 + (x & 1)];
    z_out[i] = __fadd_rn(__fmul_rn(v, inv), sh);  // two roundings, like the two affine ops
  });
  (void)w2;
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

extern "C" int fmi_postprocess_u8(const float* image, int B, int C, int H, int W, int interleave, uint8_t* out, void* stream) {
  const int64_t n = (int64_t)B * C * H * W;
  hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, (hipStream_t)stream, n, [=] __device__(int64_t i) {
    float v = image[i];
    v = fminf(fmaxf(v, -1.f), 1.f);
    v = (v + 1.0f) * 127.5f;
    // Rust `as u8`: truncate toward zero, saturate, NaN -> 0 (cpu_backend/mod.rs:2571-2574)
    uint8_t u = !(v == v) ? 0 : (v <= 0.f ? 0 : (v >= 255.f ? 255 : (uint8_t)v));
    if (interleave) {
      const int x = (int)(i % W), y = (int)((i / W) % H), c = (int)((i / ((int64_t)W * H)) % C), b = (int)(i / ((int64_t)W * H * C));
      out[(((int64_t)b * H + y) * W + x) * C + c] = u;
    } else {
      out[i] = u;
    }
  });
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

// ---- image-to-image / inpainting glue
namespace {
// one item = four pixels of a row, all C channels: u8 NCHW (uchar4 per channel) or NHWC (4 * C consecutive bytes) -> C stores of four f32
template <bool V4>
__global__ __launch_bounds__(256) void preprocess_u8_kernel(const uint8_t* __restrict__ in, int C, int64_t HW, int interleaved, float* __restrict__ out, int64_t items) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = (i % (HW / 4)) * 4, b = i / (HW / 4);  // pixel index inside the image (a row is a multiple of 4 wide)
    for (int c = 0; c < C; ++c) {
      float f[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t u = interleaved ? in[(b * HW + p + j) * C + c] : in[(b * C + c) * HW + p + j];
        // the centre of the bin that postprocess_u8 truncates into u: three f32 roundings, as the numpy expression
        f[j] = __fsub_rn(__fdiv_rn(__fadd_rn((float)u, 0.5f), 127.5f), 1.0f);
      }
      store4<V4>(out + (b * C + c) * HW + p, f[0], f[1], f[2], f[3]);
    }
  }
}
// one thread per token: the four 8x8 block means of its 16x16 pixels, then the C copies of them in pack_latents' order (c, ph, pw)
template <bool V4>
__global__ __launch_bounds__(64) void latent_mask_kernel(const float* __restrict__ mask, int C, int H, int W, float* __restrict__ out, int64_t tokens) {
  const int h2 = H / 16, w2 = W / 16;
  for (int64_t tok = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tok < tokens; tok += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(tok % w2), ii = (int)((tok / w2) % h2);
    const int64_t b = tok / ((int64_t)w2 * h2);
    const float* src = mask + (b * H + 16 * ii) * W + 16 * j;
    float m[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    for (int y = 0; y < 16; ++y) {
      float l = 0.f, r = 0.f;
      if constexpr (V4) {
        const float4* row = reinterpret_cast<const float4*>(src + (int64_t)y * W);
        const float4 q0 = row[0], q1 = row[1], q2 = row[2], q3 = row[3];
        l = ((q0.x + q0.y) + (q0.z + q0.w)) + ((q1.x + q1.y) + (q1.z + q1.w));
        r = ((q2.x + q2.y) + (q2.z + q2.w)) + ((q3.x + q3.y) + (q3.z + q3.w));
      } else {
        for (int x = 0; x < 8; ++x) l += src[(int64_t)y * W + x], r += src[(int64_t)y * W + 8 + x];
      }
      m[y >> 3][0] += l, m[y >> 3][1] += r;
    }
    const float s = 1.0f / 64.0f;
    for (int c = 0; c < C; ++c) store4<V4>(out + (tok * C + c) * 4, m[0][0] * s, m[0][1] * s, m[1][0] * s, m[1][1] * s);
  }
}
// one thread per (token, channel): the 2x2 patch of z as one 16-B store; (z - shift) * scale in two roundings, the inverse of fmi_unpack_latents' two
template <bool V4>
__global__ __launch_bounds__(256) void encode_latents_kernel(const float* __restrict__ z, int C, int h, int w, float sc, float sh, float* __restrict__ x0,
                                                             float* __restrict__ ids, int64_t n) {
  const int h2 = h / 2, w2 = w / 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int64_t tok = i / C;
    const int j = (int)(tok % w2), ii = (int)((tok / w2) % h2);
    const int64_t b = tok / ((int64_t)w2 * h2);
    const float* p = z + ((b * C + c) * h + 2 * ii) * w + 2 * j;
    store4<V4>(x0 + i * 4, __fmul_rn(__fsub_rn(p[0], sh), sc), __fmul_rn(__fsub_rn(p[1], sh), sc), __fmul_rn(__fsub_rn(p[w], sh), sc),
               __fmul_rn(__fsub_rn(p[w + 1], sh), sc));
    if (ids && c == 0) ids[tok * 3] = 0.f, ids[tok * 3 + 1] = (float)ii, ids[tok * 3 + 2] = (float)j;
  }
}
}  // namespace

extern "C" int fmi_preprocess_u8(const uint8_t* in, int B, int C, int H, int W, int interleaved, float* out, void* stream) {
  if (!in || !out || B < 0 || C <= 0 || H <= 0 || W <= 0) return fail(FMI_ERR_INVALID, "preprocess_u8: bad arguments");
  const int64_t HW = (int64_t)H * W;
  if (B == 0) return FMI_OK;
  if (HW % 4 == 0) {
    const int64_t items = (int64_t)B * (HW / 4);
    if (aligned16(out))
      hipLaunchKernelGGL(preprocess_u8_kernel<true>, map_grid(items), dim3(256), 0, (hipStream_t)stream, in, C, HW, interleaved, out, items);
    else
      hipLaunchKernelGGL(preprocess_u8_kernel<false>, map_grid(items), dim3(256), 0, (hipStream_t)stream, in, C, HW, interleaved, out, items);
  } else {  // an image whose pixel count is no multiple of 4: one element per thread
    const int64_t n = (int64_t)B * C * HW;
    hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, (hipStream_t)stream, n, [=] __device__(int64_t i) {
      const int64_t p = i % HW, c = (i / HW) % C, b = i / (HW * C);
      const uint8_t u = interleaved ? in[(b * HW + p) * C + c] : in[i];
      out[i] = __fsub_rn(__fdiv_rn(__fadd_rn((float)u, 0.5f), 127.5f), 1.0f);
    });
  }
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

extern "C" int fmi_latent_mask(const float* mask, int B, int C, int H, int W, float* out, void* stream) {
  if (!mask || !out || B < 0 || C <= 0) return fail(FMI_ERR_INVALID, "latent_mask: bad arguments");
  if (H <= 0 || W <= 0 || H % 16 || W % 16) return fail(FMI_ERR_INVALID, "latent_mask: H and W must be positive multiples of 16");
  const int64_t tokens = (int64_t)B * (H / 16) * (W / 16);
  if (tokens == 0) return FMI_OK;
  const dim3 grid((unsigned)std::min<int64_t>(cdiv64(tokens, 64), 256 * 8));
  if (aligned16(mask) && aligned16(out))  // W % 16 == 0: every 16-pixel row segment is then 16-B aligned too
    hipLaunchKernelGGL(latent_mask_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, mask, C, H, W, out, tokens);
  else
    hipLaunchKernelGGL(latent_mask_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, mask, C, H, W, out, tokens);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

extern "C" int fmi_encode_latents(const float* z, int B, int C, int h, int w, double scale_factor, double shift_factor, float* x0_out, float* img_ids_out,
                                  void* stream) {
  if (!z || !x0_out || B < 0 || C <= 0 || h <= 0 || w <= 0) return fail(FMI_ERR_INVALID, "encode_latents: bad arguments");
  if (h % 2 || w % 2) return fail(FMI_ERR_INVALID, "encode_latents: h and w must be even");
  const int64_t n = (int64_t)B * (h / 2) * (w / 2) * C;
  if (n == 0) return FMI_OK;
  const float sc = (float)scale_factor, sh = (float)shift_factor;  // the scalars rounded to f32 like candle's affine
  if (aligned16(x0_out))
    hipLaunchKernelGGL(encode_latents_kernel<true>, map_grid(n), dim3(256), 0, (hipStream_t)stream, z, C, h, w, sc, sh, x0_out, img_ids_out, n);
  else
    hipLaunchKernelGGL(encode_latents_kernel<false>, map_grid(n), dim3(256), 0, (hipStream_t)stream, z, C, h, w, sc, sh, x0_out, img_ids_out, n);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

// the position ids of an (h2, w2) token grid: (id0, row0 + r, col0 + c) per token, one f32 addition each — fmi_pack_latents' ids at the defaults (0, 0, 0);
// a reference image's tokens carry id0 = 1
extern "C" int fmi_latent_ids(int B, int h2, int w2, float id0, float row0, float col0, float* ids_out, void* stream) {
  if (!ids_out || B < 0 || h2 < 0 || w2 < 0) return fail(FMI_ERR_INVALID, "latent_ids: bad arguments");
  const int64_t n = (int64_t)B * h2 * w2;
  if (n == 0) return FMI_OK;
  hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, (hipStream_t)stream, n, [=] __device__(int64_t tok) {
    const int c = (int)(tok % w2), r = (int)((tok / w2) % h2);
    float* o = ids_out + tok * 3;
    o[0] = id0, o[1] = __fadd_rn(row0, (float)r), o[2] = __fadd_rn(col0, (float)c);
  });
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

// ---- channel-concatenated conditioning glue (FLUX.1 Fill / Canny / Depth)
namespace {
__device__ __forceinline__ float mask_bit(float m) { return m >= 0.5f ? 1.0f : 0.0f; }  // diffusers' mask processor binarises at 0.5 (a NaN counts as 0)
// out = image * (1 - b): V = float4 (W % 4 == 0: a word never straddles two rows or images) or float
template <typename V>
__global__ __launch_bounds__(256) void mask_image_kernel(const V* __restrict__ image, const V* __restrict__ mask, int64_t HWv, int C, V* __restrict__ out, int64_t items) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i % HWv, b = i / (HWv * C);
    const V x = image[i], m = mask[b * HWv + p];
    if constexpr (sizeof(V) == 16)
      out[i] = make_float4(x.x * (1.0f - mask_bit(m.x)), x.y * (1.0f - mask_bit(m.y)), x.z * (1.0f - mask_bit(m.z)), x.w * (1.0f - mask_bit(m.w)));
    else
      out[i] = x * (1.0f - mask_bit(m));
  }
}
// Twelve items per token.  Items 0..3: 16 of the token's 64 latent values, copied.  Items 4..11: py = item - 4 — the 16 mask pixels of rows 16i + py and
// 16i + 8 + py (dy = 0, 1) of the token's 16x16 square, binarised, become the 32 columns 64 + (py * 8 + px) * 4 + dy * 2 + dx with px = 0..7, dx = 0, 1 the
// pixel 8 dx + px of those rows: four 16-B loads per row, eight 16-B stores.
template <bool V4>
__global__ __launch_bounds__(256) void fill_condition_kernel(const float* __restrict__ lat, const float* __restrict__ mask, int H, int W, float* __restrict__ out,
                                                             int64_t items) {
  const int h2 = H / 16, w2 = W / 16;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(it % 12);
    const int64_t tok = it / 12;
    float* o = out + tok * 320;
    if (q < 4) {
      const float* s = lat + tok * 64 + q * 16;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (V4)
          *reinterpret_cast<float4*>(o + q * 16 + 4 * k) = *reinterpret_cast<const float4*>(s + 4 * k);
        else
          store4<false>(o + q * 16 + 4 * k, s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
      }
      continue;
    }
    const int py = q - 4;
    const int j = (int)(tok % w2), ii = (int)((tok / w2) % h2);
    const int64_t b = tok / ((int64_t)w2 * h2);
    const float* r0 = mask + (b * H + 16 * ii + py) * W + 16 * j;  // dy = 0
    const float* r1 = r0 + (int64_t)8 * W;                          // dy = 1
    __attribute__((aligned(16))) float a[16], c[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (V4) {
        *reinterpret_cast<float4*>(a + 4 * k) = *reinterpret_cast<const float4*>(r0 + 4 * k);
        *reinterpret_cast<float4*>(c + 4 * k) = *reinterpret_cast<const float4*>(r1 + 4 * k);
      } else {
        for (int e = 0; e < 4; ++e) a[4 * k + e] = r0[4 * k + e], c[4 * k + e] = r1[4 * k + e];
      }
    }
#pragma unroll
    for (int px = 0; px < 8; ++px) store4<V4>(o + 64 + (py * 8 + px) * 4, mask_bit(a[px]), mask_bit(a[8 + px]), mask_bit(c[px]), mask_bit(c[8 + px]));
  }
}
}  // namespace

extern "C" int fmi_cast_cols_bf16(const void* src, fmi_dtype dt, int64_t rows, int64_t rows_src, int cols, void* dst_bf16, int dst_ld, int col0, void* stream) {
  return launch_cast_cols_bf16(src, dt, rows, rows_src, cols, (bf16_t*)dst_bf16, dst_ld, col0, (hipStream_t)stream);
}

extern "C" int fmi_mask_image(const float* image, const float* mask, int B, int C, int H, int W, float* out, void* stream) {
  if (!image || !mask || !out || B < 0 || C <= 0 || H <= 0 || W <= 0) return fail(FMI_ERR_INVALID, "mask_image: bad arguments");
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * C * HW;
  if (n == 0) return FMI_OK;
  if (HW % 4 == 0 && aligned16(image) && aligned16(mask) && aligned16(out))
    hipLaunchKernelGGL(mask_image_kernel<float4>, map_grid(n / 4), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(image),
                       reinterpret_cast<const float4*>(mask), HW / 4, C, reinterpret_cast<float4*>(out), n / 4);
  else
    hipLaunchKernelGGL(mask_image_kernel<float>, map_grid(n), dim3(256), 0, (hipStream_t)stream, image, mask, HW, C, out, n);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

extern "C" int fmi_fill_condition(const float* masked_latents, const float* mask, int B, int H, int W, float* cond_out, void* stream) {
  if (!masked_latents || !mask || !cond_out || B < 0) return fail(FMI_ERR_INVALID, "fill_condition: bad arguments");
  if (H <= 0 || W <= 0 || H % 16 || W % 16) return fail(FMI_ERR_INVALID, "fill_condition: H and W must be positive multiples of 16");
  const int64_t items = (int64_t)B * (H / 16) * (W / 16) * 12;
  if (items == 0) return FMI_OK;
  if (aligned16(masked_latents) && aligned16(mask) && aligned16(cond_out))  // W % 16 == 0: every 16-pixel row segment is then 16-B aligned too
    hipLaunchKernelGGL(fill_condition_kernel<true>, map_grid(items), dim3(256), 0, (hipStream_t)stream, masked_latents, mask, H, W, cond_out, items);
  else
    hipLaunchKernelGGL(fill_condition_kernel<false>, map_grid(items), dim3(256), 0, (hipStream_t)stream, masked_latents, mask, H, W, cond_out, items);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

extern "C" int fmi_scale_noise(const float* x0, const float* noise, double t, int64_t n, float* out, void* stream) {
  if (!x0 || !noise || !out || n < 0) return fail(FMI_ERR_INVALID, "scale_noise: bad arguments");
  return launch_scale_noise(x0, noise, (float)t, n, out, (hipStream_t)stream);
}

// Philox4x32-10 + Box-Muller.  counter = (i/4, sample, 0, 0), key = seed; 4 normals per counter.
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t (&k)[2]) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
  const uint32_t n0 = hi1 ^ c[1] ^ k[0], n1 = lo1, n2 = hi0 ^ c[3] ^ k[1], n3 = lo0;
  c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
  k[0] += 0x9E3779B9u;
  k[1] += 0xBB67AE85u;
}
// counter = (quad lo, quad hi, sample lo, sample hi), key = (seed lo, seed hi): 4 words per counter
__device__ __forceinline__ void philox_quad(int64_t qd, uint64_t sample, uint64_t seed, uint32_t (&c)[4]) {
  c[0] = (uint32_t)qd, c[1] = (uint32_t)((uint64_t)qd >> 32), c[2] = (uint32_t)sample, c[3] = (uint32_t)(sample >> 32);
  uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
  for (int r = 0; r < 10; ++r) philox_round(c, k);
}
// the raw stream fmi_randn draws from (checked bit for bit against the oracle / Random123 known answers)
extern "C" int fmi_philox_u32(uint32_t* out, int64_t n_per_sample, int B, uint64_t seed, uint64_t first_sample, void* stream) {
  if (!out || n_per_sample < 0 || B < 0) return fail(FMI_ERR_INVALID, "philox_u32: bad arguments");
  const int64_t quads = (n_per_sample + 3) / 4;
  const int64_t n = quads * B;
  if (n == 0) return FMI_OK;
  auto body = [=] __device__(int64_t i) {
    const int64_t qd = i % quads;
    const int b = (int)(i / quads);
    uint32_t c[4];
    philox_quad(qd, first_sample + (uint64_t)b, seed, c);
    for (int e = 0; e < 4; ++e) {
      const int64_t idx = qd * 4 + e;
      if (idx < n_per_sample) out[(int64_t)b * n_per_sample + idx] = c[e];
    }
  };
  hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, (hipStream_t)stream, n, body);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
extern "C" int fmi_randn(float* out, int64_t n_per_sample, int B, uint64_t seed, uint64_t first_sample, void* stream) {
  if (!out || n_per_sample < 0 || B < 0) return fail(FMI_ERR_INVALID, "randn: bad arguments");
  const int64_t quads = (n_per_sample + 3) / 4;
  const int64_t n = quads * B;
  if (n == 0) return FMI_OK;
  auto body = [=] __device__(int64_t i) {
    const int64_t qd = i % quads;
    const int b = (int)(i / quads);
    uint32_t c[4];
    philox_quad(qd, first_sample + (uint64_t)b, seed, c);
    float z[4];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const float u1 = ((float)(c[2 * p] >> 8) + 0.5f) * (1.0f / 16777216.0f);
      const float u2 = ((float)(c[2 * p + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
      const float rad = sqrtf(-2.0f * logf(u1));
      float sn, cs;
      sincosf(6.283185307179586f * u2, &sn, &cs);
      z[2 * p] = rad * cs;
      z[2 * p + 1] = rad * sn;
    }
    for (int e = 0; e < 4; ++e) {
      const int64_t idx = qd * 4 + e;
      if (idx < n_per_sample) out[(int64_t)b * n_per_sample + idx] = z[e];
    }
  };
  hipLaunchKernelGGL(map_kernel, map_grid(n), dim3(256), 0, (hipStream_t)stream, n, body);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}
