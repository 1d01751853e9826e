// lora.hip — LoRA merge for gfx950: rows of a resident bf16 weight matrix are REWRITTEN as
//   W[n, k] = bf16_rne( W0[n, k] + sum_j Bt[j, n] * A[j, k] )          (f64 FMAs in ascending j, ONE rounding at the end)
// from a pristine copy W0 of those rows and the concatenated low-rank factors of every active adapter on that Linear (flux_model.hip:
// lora_remerge builds them — adapter after adapter in lexicographic name order, weight * scale folded into Bt).  The denoise loop is
// untouched: it keeps running the same GEMMs on the same layouts; this kernel only changes bytes they read.
//
// Why f64 accumulators.  The operands are the adapters' f32 values, never rounded to bf16.  With f32 accumulators the sum carries an
// absolute error of ~1e-9 at these magnitudes (|W0| ~ 0.02): harmless for almost every element, but where W0 and the update cancel
// (|W| < ~1e-6: a handful of elements per matrix) the result is then NOT one of the two bf16 neighbours of the true value — an f32 holding
// the update has an ulp of 2e-9 there, so no order of f32 additions can do better.  An f64 FMA is full rate on this part (by its data sheet the rate
// of an unpacked f32 FMA; the measured cost is in profiles/lora_merge.txt), a product of two f32 values is exact in f64, and the sum of <= a few hundred of them is good to ~1e-18:
// the merged weight is the correctly rounded value of the exact expression, element for element.  The last step rounds f64 -> f32 to ODD
// and f32 -> bf16 to nearest-even, which together are one correct rounding (24 bits >= 8 + 2).
//
// Shape of the work: one pass over the matrix (2 B read + 2 B written per element) with R FMAs per element, R = total rank.  The factors
// are tiny and reused by every element of a tile, so they are staged in LDS in chunks of LORA_RANK_CHUNK rank rows (A as f32, widened at
// the read; Bt as f64); the accumulators (4 rows x 8 columns per lane) stay in registers; the weights move as 16-byte accesses along K.
//
// Tile = LORA_TILE_ROWS (64) rows x 128 columns per workgroup of 256 lanes: lane (ty, tx) = (tid / 16, tid % 16) owns rows 4 ty .. 4 ty + 3 and
// columns 8 tx .. 8 tx + 7.  LDS reads per rank row: its 8 A values and its 4 Bt values as two ds_read_b128 each.  The A tile is stored
// with its 16-byte slots permuted — slot q of a row lands at (q & 1) * 16 + (q >> 1) — so that the 16 lanes of a row read 16 consecutive
// slots (256 B, one bank row) per instruction instead of every other slot (a 2-way conflict).
//
// Preconditions (checked by the launcher): K % 8 == 0 and 16-byte aligned row starts; A has Rpad rows, Bt is (Rpad, rows_pad) with
// Rpad % LORA_RANK_CHUNK == 0 and rows_pad % LORA_TILE_ROWS == 0, zero beyond the real rank / rows (a zero product adds nothing), so
// any rank >= 1 and any row count run through the same loop; loads and stores of W are guarded by n < rows and k < K.
#include "common.h"

namespace fmi {

namespace {

constexpr int LT_N = LORA_TILE_ROWS, LT_K = 128, LT_R = LORA_RANK_CHUNK;

// f64 -> f32 rounded to ODD: the exact value if it is one, else of the two neighbouring f32 values the one whose last bit is set.  A later round to
// nearest-even to fewer bits (bf16) then gives what a single rounding of the f64 value would (no double rounding).  Finite, normal-range values.
__device__ __forceinline__ float f64_to_f32_odd(double d) {
  const float f = (float)d;
  const double back = (double)f;
  if (back == d) return f;
  uint32_t u = __float_as_uint(f);
  if (fabs(back) > fabs(d)) u -= 1;  // the neighbour towards zero (sign-magnitude bits: one step down)
  return __uint_as_float(u | 1u);
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const bf16_t* __restrict__ w0, bf16_t* __restrict__ w, int rows, int K,
                                                         const float* __restrict__ A, const double* __restrict__ Bt, int rows_pad, int Rpad) {
  __shared__ __attribute__((aligned(16))) float sA[LT_R][LT_K];
  __shared__ __attribute__((aligned(16))) double sB[LT_R][LT_N];
  const int ktiles = (K + LT_K - 1) / LT_K;
  const int kt = blockIdx.x % ktiles, nt = blockIdx.x / ktiles;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int k = kt * LT_K + tx * 8, n = nt * LT_N + ty * 4;
  const bool kin = k < K;  // K % 8 == 0: a lane's 8 columns are inside or outside together

  uint4 wv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    wv[i] = make_uint4(0, 0, 0, 0);
    if (kin && n + i < rows) wv[i] = *reinterpret_cast<const uint4*>(w0 + (size_t)(n + i) * K + k);
  }
  double acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[i][c] = 0.0;

  for (int rc = 0; rc < Rpad; rc += LT_R) {
    __syncthreads();  // (the previous chunk has been read)
#pragma unroll
    for (int t = tid; t < LT_R * (LT_K / 4); t += 256) {
      const int j = t / (LT_K / 4), q = t % (LT_K / 4);
      const int kk = kt * LT_K + q * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kk < K) v = *reinterpret_cast<const float4*>(A + (size_t)(rc + j) * K + kk);
      *reinterpret_cast<float4*>(&sA[j][((q & 1) * 16 + (q >> 1)) * 4]) = v;
    }
#pragma unroll
    for (int t = tid; t < LT_R * (LT_N / 2); t += 256) {
      const int j = t / (LT_N / 2), q = t % (LT_N / 2);
      *reinterpret_cast<double2*>(&sB[j][q * 2]) = *reinterpret_cast<const double2*>(Bt + (size_t)(rc + j) * rows_pad + nt * LT_N + q * 2);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LT_R; ++j) {
      const float4 a0 = *reinterpret_cast<const float4*>(&sA[j][tx * 4]);
      const float4 a1 = *reinterpret_cast<const float4*>(&sA[j][64 + tx * 4]);
      const double2 b01 = *reinterpret_cast<const double2*>(&sB[j][ty * 4]);
      const double2 b23 = *reinterpret_cast<const double2*>(&sB[j][ty * 4 + 2]);
      const double a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const double b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[i][c] = fma(b[i], a[c], acc[i][c]);
    }
  }

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!(kin && n + i < rows)) continue;
    const uint32_t in[4] = {wv[i].x, wv[i].y, wv[i].z, wv[i].w};
    uint32_t o[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const double lo = (double)__uint_as_float(in[p] << 16) + acc[i][2 * p];
      const double hi = (double)__uint_as_float(in[p] & 0xffff0000u) + acc[i][2 * p + 1];
      o[p] = pack_bf16x2(f64_to_f32_odd(lo), f64_to_f32_odd(hi));
    }
    *reinterpret_cast<uint4*>(w + (size_t)(n + i) * K + k) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// One adapter's factors into its rank rows [off, off + r) of the concatenated operands, in one launch: Acat[off + j, k] = A[j, k] (a copy) and
// Bt[off + j, n] = coef * B[n, j] for n < rows, 0 for rows <= n < rows_pad (the (rows, r) up-projection transposed, weight * scale folded in, exact in f64).
__global__ void lora_pack_kernel(const float* __restrict__ A, const float* __restrict__ B, int rows, int K, int r, double coef, float* __restrict__ Acat,
                                 double* __restrict__ Bt, int rows_pad, int off) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t na = (int64_t)r * K;
  if (i < na) {
    Acat[(size_t)off * K + i] = A[i];
    return;
  }
  const int64_t t = i - na;
  if (t >= (int64_t)r * rows_pad) return;
  const int j = (int)(t / rows_pad), n = (int)(t % rows_pad);  // consecutive lanes write consecutive n
  Bt[(size_t)(off + j) * rows_pad + n] = n < rows ? coef * (double)B[(size_t)n * r + j] : 0.0;
}

}  // namespace

int launch_lora_pack(const float* A, const float* B, int rows, int K, int r, double coef, float* Acat, double* Bt, int rows_pad, int off, hipStream_t stream) {
  if (rows <= 0 || K <= 0 || r <= 0 || rows > rows_pad || off < 0) return fail(FMI_ERR_INVALID, "lora_pack: bad shape");
  const int64_t n = (int64_t)r * K + (int64_t)r * rows_pad;
  hipLaunchKernelGGL(lora_pack_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, stream, A, B, rows, K, r, coef, Acat, Bt, rows_pad, off);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

int launch_lora_merge(const bf16_t* w0, bf16_t* w, int rows, int K, const float* A, const double* Bt, int rows_pad, int Rpad, hipStream_t stream) {
  if (rows <= 0 || K <= 0 || Rpad <= 0) return fail(FMI_ERR_INVALID, "lora_merge: bad shape");
  if (K % 8) return fail(FMI_ERR_UNSUPPORTED, "lora_merge: in_features must be a multiple of 8 (16-byte accesses along K)");
  if (Rpad % LT_R || rows_pad % LT_N || rows_pad < rows) return fail(FMI_ERR_INVALID, "lora_merge: the factors are not padded to the tile");
  if ((reinterpret_cast<uintptr_t>(w0) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bt)) & 15)
    return fail(FMI_ERR_INVALID, "lora_merge: pointers must be 16-byte aligned");
  const int64_t tiles = (int64_t)cdiv(rows, LT_N) * cdiv(K, LT_K);
  if (tiles >= (1ll << 31)) return fail(FMI_ERR_UNSUPPORTED, "lora_merge: matrix too large");
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, w0, w, rows, K, A, Bt, rows_pad, Rpad);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

}  // namespace fmi
