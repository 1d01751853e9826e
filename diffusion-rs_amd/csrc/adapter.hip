// adapter.hip — LyCORIS / DoRA merge for gfx950: rows of a resident bf16 weight matrix are REWRITTEN as
//   W[n, k] = bf16_rne( W0[n, k] + sum_t weight_t * Delta_t[n, k] )          (every Delta in f64, terms in the order given, ONE rounding at the end)
// for terms that are not low-rank in weight space and so cannot go through lora.hip's concatenated-factor form:
//   LORA   Delta = scale * (B A)                                   (a plain pair that shares its Linear with another kind)
//   LOHA   Delta = scale * (w1_a w1_b) (.) (w2_a w2_b)             (two rank sums per element and their product)
//   LOKR   Delta[n, k] = scale * w1[(n + i0) / c, k / d] * w2[(n + i0) % c, k % d]       (index arithmetic on two small matrices)
//   DORA   Delta = g (.) (W0 + scale * (B A)) - W0, g_n = m_n / ||W0[n, :] + scale * (B A)[n, :]||_2     (g from dora_norm_kernel, once per term)
// A Linear whose active terms are all plain LoRA never comes here (flux_model.hip: lora_remerge keeps lora_pack_kernel + lora_merge_kernel for it).
//
// Shape of the work: lora.hip's — one workgroup of 256 lanes per 64-row x 128-column tile, lane (ty, tx) = (tid / 16, tid % 16) owns rows 4 ty .. 4 ty + 3
// and columns 8 tx .. 8 tx + 7, the weights move as 16-byte accesses along K — and the tile walks a device array of term descriptors.  A rank sum
// (rank_sum below: LORA, DORA, and twice for LOHA) stages its factors through LDS in chunks of 16 rank rows exactly as lora_merge_kernel does (the
// (r, K) factor as f32 with the same slot permutation, the (rows, r) factor transposed and widened to f64), straight from the term's own f32 factors:
// ragged ranks, rows and columns are zero-filled at the staging, so there is no packing pass and no padded copy.  Registers per lane: the running total
// (32 f64) and up to two rank sums (2 x 32 f64) — 192 of the 512 VGPRs a 256-lane workgroup may use per lane; the build's figures are in DESIGN.md 4.7.
//
// Numerics: an f32 x f32 product is exact in f64; everything after it (the rank sums, LoHa's product, LoKr's product, DoRA's sum of squares, sqrt and
// division, the weighting) is an f64 operation rounded once each, so an element is the one rounding of an f64 evaluation of its formula, not the
// correctly rounded value of the exact expression (only the all-LoRA path claims that).  The last step is lora.hip's: f64 -> f32 to odd, f32 -> bf16 RNE.
//
// Preconditions (checked by the launchers): K % 8 == 0, 16-byte aligned w0 / w; loads and stores of W are guarded by n < rows and k < K, so the
// neighbouring parts of a fused matrix are never written.
#include "common.h"

#include <cmath>

namespace fmi {

namespace {

constexpr int AT_N = 64, AT_K = 128, AT_R = 16;
constexpr int AT_BS = AT_N + 2;  // leading dimension of the staged (rows, r) factor: 528 B, a multiple of 16, and off the power of two for the transposing write

__device__ __forceinline__ float f64_to_f32_odd(double d) {  // as in lora.hip
  const float f = (float)d;
  const double back = (double)f;
  if (back == d) return f;
  uint32_t u = __float_as_uint(f);
  if (fabs(back) > fabs(d)) u -= 1;
  return __uint_as_float(u | 1u);
}

struct Lane {
  int tid, tx, ty, kt, nt, k, n;
  bool kin;
};

// acc[i][c] = sum_j Bf[n + i, j] * Af[j, k + c], f64 FMAs in ascending j.  Af (r, K), Bf (rows, r), both f32 row-major.  Every lane of the workgroup calls it.
__device__ __forceinline__ void rank_sum(double (&acc)[4][8], const float* __restrict__ Af, const float* __restrict__ Bf, int r, int rows, int K, const Lane& l,
                                         float (*sA)[AT_K], double (*sB)[AT_BS]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[i][c] = 0.0;
  for (int rc = 0; rc < r; rc += AT_R) {
    __syncthreads();  // (the previous chunk has been read)
#pragma unroll
    for (int t = l.tid; t < AT_R * (AT_K / 4); t += 256) {
      const int j = t / (AT_K / 4), q = t % (AT_K / 4);
      const int kk = l.kt * AT_K + q * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kk < K && rc + j < r) v = *reinterpret_cast<const float4*>(Af + (size_t)(rc + j) * K + kk);  // K % 8 == 0: the 4 columns are inside together
      *reinterpret_cast<float4*>(&sA[j][((q & 1) * 16 + (q >> 1)) * 4]) = v;
    }
#pragma unroll
    for (int t = l.tid; t < AT_R * AT_N; t += 256) {
      const int j = t % AT_R, n = t / AT_R;  // consecutive lanes read consecutive j of one row of Bf
      const int gn = l.nt * AT_N + n;
      sB[j][n] = (gn < rows && rc + j < r) ? (double)Bf[(size_t)gn * r + rc + j] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < AT_R; ++j) {
      const float4 a0 = *reinterpret_cast<const float4*>(&sA[j][l.tx * 4]);
      const float4 a1 = *reinterpret_cast<const float4*>(&sA[j][64 + l.tx * 4]);
      const double2 b01 = *reinterpret_cast<const double2*>(&sB[j][l.ty * 4]);
      const double2 b23 = *reinterpret_cast<const double2*>(&sB[j][l.ty * 4 + 2]);
      const double a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const double b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[i][c] = fma(b[i], a[c], acc[i][c]);
    }
  }
}

__device__ __forceinline__ Lane make_lane(int tile, int ktiles) {
  Lane l;
  l.tid = threadIdx.x, l.tx = l.tid & 15, l.ty = l.tid >> 4;
  l.kt = tile % ktiles, l.nt = tile / ktiles;
  l.k = l.kt * AT_K + l.tx * 8, l.n = l.nt * AT_N + l.ty * 4;
  return l;
}

// the lane's 4 x 8 values of W0 as f64 (0 outside the matrix)
__device__ __forceinline__ void load_w0(double (&w0v)[4][8], const bf16_t* __restrict__ w0, int rows, int K, const Lane& l) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (l.kin && l.n + i < rows) v = *reinterpret_cast<const uint4*>(w0 + (size_t)(l.n + i) * K + l.k);
    const uint32_t in[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      w0v[i][2 * p] = (double)__uint_as_float(in[p] << 16);
      w0v[i][2 * p + 1] = (double)__uint_as_float(in[p] & 0xffff0000u);
    }
  }
}

__device__ __forceinline__ double lokr_at(const void* p, bool f64, size_t i) { return f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i]; }

__global__ __launch_bounds__(256) void adapter_merge_kernel(const bf16_t* __restrict__ w0, bf16_t* __restrict__ w, int rows, int K,
                                                            const AdapterDesc* __restrict__ descs, int n_terms) {
  __shared__ __attribute__((aligned(16))) float sA[AT_R][AT_K];
  __shared__ __attribute__((aligned(16))) double sB[AT_R][AT_BS];
  Lane l = make_lane(blockIdx.x, (K + AT_K - 1) / AT_K);
  l.kin = l.k < K;  // K % 8 == 0: a lane's 8 columns are inside or outside together

  double tot[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 8; ++c) tot[i][c] = 0.0;

  for (int t = 0; t < n_terms; ++t) {
    const AdapterDesc& d = descs[t];  // (uniform over the workgroup)
    const int kind = d.kind;
    if (kind == FMI_ADAPTER_LOKR) {
      const bool f1 = d.w_f64 & 1, f2 = d.w_f64 & 2;
      const int b = d.b, c = d.c, dd = d.d;
      const double coef = d.coef;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!(l.kin && l.n + i < rows)) continue;
        const int gr = l.n + i + d.row_offset;
        const int r1 = gr / c, r2 = gr % c;
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
          const int col = l.k + cc;
          const double v1 = lokr_at(d.w1, f1, (size_t)r1 * b + col / dd);
          const double v2 = lokr_at(d.w2, f2, (size_t)r2 * dd + col % dd);
          tot[i][cc] = fma(coef, v1 * v2, tot[i][cc]);
        }
      }
      continue;
    }
    double acc[4][8];
    rank_sum(acc, d.fa[0], d.fb[0], d.r, rows, K, l, sA, sB);
    if (kind == FMI_ADAPTER_LORA) {
      const double coef = d.coef;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) tot[i][c] = fma(coef, acc[i][c], tot[i][c]);
    } else if (kind == FMI_ADAPTER_LOHA) {
      double acc2[4][8];
      rank_sum(acc2, d.fa[1], d.fb[1], d.r, rows, K, l, sA, sB);
      const double coef = d.coef;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) tot[i][c] = fma(coef, acc[i][c] * acc2[i][c], tot[i][c]);
    } else {  // DORA
      double w0v[4][8];
      load_w0(w0v, w0, rows, K, l);
      const double coef = d.coef, scale = d.scale;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double g = l.n + i < rows ? d.g[l.n + i] : 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const double v = fma(scale, acc[i][c], w0v[i][c]);
          tot[i][c] = fma(coef, g * v - w0v[i][c], tot[i][c]);
        }
      }
    }
  }

  double w0v[4][8];
  load_w0(w0v, w0, rows, K, l);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!(l.kin && l.n + i < rows)) continue;
    uint32_t o[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) o[p] = pack_bf16x2(f64_to_f32_odd(w0v[i][2 * p] + tot[i][2 * p]), f64_to_f32_odd(w0v[i][2 * p + 1] + tot[i][2 * p + 1]));
    *reinterpret_cast<uint4*>(w + (size_t)(l.n + i) * K + l.k) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// DoRA's row norms: one workgroup per 64-row tile walks the K tiles in ascending order; each lane keeps the sum of squares of its 8 columns per row in
// f64, the 16 lanes of a row are then added by a fixed tree in LDS (no atomics: the same bits from run to run).  gn[row] = m[row] / n, gn[rows + row] = n.
__global__ __launch_bounds__(256) void dora_norm_kernel(const bf16_t* __restrict__ w0, int rows, int K, const float* __restrict__ Af, const float* __restrict__ Bf,
                                                        int r, double scale, const float* __restrict__ mag, double* __restrict__ gn) {
  __shared__ __attribute__((aligned(16))) float sA[AT_R][AT_K];
  __shared__ __attribute__((aligned(16))) double sB[AT_R][AT_BS];
  __shared__ double red[AT_N][17];
  const int ktiles = (K + AT_K - 1) / AT_K;
  double sq[4] = {0.0, 0.0, 0.0, 0.0};
  Lane l = make_lane(blockIdx.x * ktiles, ktiles);
  for (int kt = 0; kt < ktiles; ++kt) {
    l = make_lane(blockIdx.x * ktiles + kt, ktiles);
    l.kin = l.k < K;
    double acc[4][8], w0v[4][8];
    rank_sum(acc, Af, Bf, r, rows, K, l, sA, sB);
    load_w0(w0v, w0, rows, K, l);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const double v = fma(scale, acc[i][c], w0v[i][c]);  // (0 outside the matrix: both operands are)
        sq[i] = fma(v, v, sq[i]);
      }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[l.ty * 4 + i][l.tx] = sq[i];
  __syncthreads();
  if (l.tid < AT_N) {
    double s[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) s[j] = red[l.tid][j];
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
      for (int j = 0; j < w; ++j) s[j] = s[j] + s[j + w];
    const int row = blockIdx.x * AT_N + l.tid;
    if (row < rows) {
      const double nrm = sqrt(s[0]);
      gn[row] = (double)mag[row] / nrm;
      gn[rows + row] = nrm;
    }
  }
}

// out (m, n) f64 = fa (m, r) fb (r, n), f32 operands, f64 FMAs in ascending rank: a decomposed LoKr factor, expanded once
__global__ void lokr_expand_kernel(const float* __restrict__ fa, const float* __restrict__ fb, int m, int r, int n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)m * n) return;
  const int row = (int)(i / n), col = (int)(i % n);
  double s = 0.0;
  for (int j = 0; j < r; ++j) s = fma((double)fa[(size_t)row * r + j], (double)fb[(size_t)j * n + col], s);
  out[i] = s;
}

int upload_f32(const void* src, int dtype, int64_t n, DeviceBuffer& out) {
  FMI_HIP_TRY(out.alloc((size_t)n * 4));
  return upload_as_f32(src, (fmi_dtype)dtype, n, out.as<float>());
}

}  // namespace

int launch_adapter_merge(const bf16_t* w0, bf16_t* w, int rows, int K, const AdapterDesc* descs, int n_terms, hipStream_t stream) {
  if (rows <= 0 || K <= 0 || n_terms < 0 || (n_terms && !descs)) return fail(FMI_ERR_INVALID, "adapter_merge: bad shape");
  if (K % 8) return fail(FMI_ERR_UNSUPPORTED, "adapter_merge: in_features must be a multiple of 8 (16-byte accesses along K)");
  if ((reinterpret_cast<uintptr_t>(w0) | reinterpret_cast<uintptr_t>(w)) & 15) return fail(FMI_ERR_INVALID, "adapter_merge: pointers must be 16-byte aligned");
  const int64_t tiles = (int64_t)cdiv(rows, AT_N) * cdiv(K, AT_K);
  if (tiles >= (1ll << 31)) return fail(FMI_ERR_UNSUPPORTED, "adapter_merge: matrix too large");
  hipLaunchKernelGGL(adapter_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, w0, w, rows, K, descs, n_terms);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

AdapterDesc adapter_term_desc(const AdapterTerm& t, double weight) {
  AdapterDesc d{};
  d.kind = t.kind, d.r = t.r;
  d.coef = t.kind == FMI_ADAPTER_DORA ? weight : weight * (double)t.scale;
  d.scale = (double)t.scale;
  if (t.kind == FMI_ADAPTER_LOKR) {
    const double* x = t.x.as<double>();
    d.w1 = t.w1_f64 ? (const void*)x : t.f[0].ptr;
    d.w2 = t.w2_f64 ? (const void*)(x + (t.w1_f64 ? (size_t)t.a * t.b : 0)) : t.f[2].ptr;
    d.w_f64 = (t.w1_f64 ? 1 : 0) | (t.w2_f64 ? 2 : 0);
    d.b = t.b, d.c = t.c, d.d = t.d, d.row_offset = t.row_offset;
    return d;
  }
  d.fa[0] = t.f[0].as<float>(), d.fb[0] = t.f[1].as<float>();
  d.fa[1] = t.f[2].as<float>(), d.fb[1] = t.f[3].as<float>();
  d.g = t.x.as<double>();
  return d;
}

int adapter_term_build(const fmi_adapter_term* t, const bf16_t* w0, int rows, int K, const std::string& what, AdapterTerm* out) {
  if (!t) return fail(FMI_ERR_INVALID, what + ": null term");
  if (t->kind < FMI_ADAPTER_LORA || t->kind > FMI_ADAPTER_DORA) return fail(FMI_ERR_INVALID, what + ": unknown adapter kind " + std::to_string(t->kind));
  if (t->dtype != FMI_F32 && t->dtype != FMI_F16 && t->dtype != FMI_BF16) return fail(FMI_ERR_INVALID, what + ": dtype must be F32/F16/BF16");
  if (!std::isfinite(t->scale)) return fail(FMI_ERR_INVALID, what + ": scale must be finite");
  if (K % 8) return fail(FMI_ERR_UNSUPPORTED, what + ": in_features must be a multiple of 8");
  for (int i = 0; i < 4; ++i)
    if (t->factor[i] && (t->factor_rows[i] < 1 || t->factor_cols[i] < 1)) return fail(FMI_ERR_INVALID, what + ": a factor with an empty shape (rank must be at least 1)");
  auto shape = [&](int i) { return "(" + std::to_string(t->factor_rows[i]) + ", " + std::to_string(t->factor_cols[i]) + ")"; };
  auto numel = [&](int i) { return (int64_t)t->factor_rows[i] * t->factor_cols[i]; };
  AdapterTerm n;
  n.kind = t->kind, n.scale = t->scale;
  const std::string lin = "the Linear is (" + std::to_string(rows) + ", " + std::to_string(K) + ")";
  if (t->kind == FMI_ADAPTER_LOKR) {
    if (!t->factor[0] || !t->factor[2]) return fail(FMI_ERR_INVALID, what + ": LoKr needs w1 (or w1_a) in factor[0] and w2 (or w2_a) in factor[2]");
    for (int h = 0; h < 2; ++h)
      if (t->factor[2 * h + 1] && t->factor_cols[2 * h] != t->factor_rows[2 * h + 1])
        return fail(FMI_ERR_INVALID, what + ": LoKr w" + std::to_string(h + 1) + "_a " + shape(2 * h) + " and w" + std::to_string(h + 1) + "_b " + shape(2 * h + 1) + " do not multiply");
    n.a = t->factor_rows[0], n.b = t->factor[1] ? t->factor_cols[1] : t->factor_cols[0];
    n.c = t->factor_rows[2], n.d = t->factor[3] ? t->factor_cols[3] : t->factor_cols[2];
    n.row_offset = t->row_offset;
    if ((int64_t)n.b * n.d != K)
      return fail(FMI_ERR_INVALID, what + ": LoKr w1 has " + std::to_string(n.b) + " and w2 " + std::to_string(n.d) + " columns: b * d != in, " + lin);
    if (t->row_offset < 0 || (int64_t)t->row_offset + rows > (int64_t)n.a * n.c)
      return fail(FMI_ERR_INVALID, what + ": LoKr row_offset " + std::to_string(t->row_offset) + " + out > a * c = " + std::to_string((int64_t)n.a * n.c) + ", " + lin);
    n.w1_f64 = t->factor[1] != nullptr, n.w2_f64 = t->factor[3] != nullptr;
    const size_t n1 = n.w1_f64 ? (size_t)n.a * n.b : 0, n2 = n.w2_f64 ? (size_t)n.c * n.d : 0;
    if (n1 + n2) FMI_HIP_TRY(n.x.alloc((n1 + n2) * 8));
    for (int h = 0; h < 2; ++h) {
      FMI_TRY(upload_f32(t->factor[2 * h], t->dtype, numel(2 * h), n.f[2 * h]));
      if (!t->factor[2 * h + 1]) continue;
      FMI_TRY(upload_f32(t->factor[2 * h + 1], t->dtype, numel(2 * h + 1), n.f[2 * h + 1]));
      const int m_ = t->factor_rows[2 * h], r_ = t->factor_cols[2 * h], n_ = t->factor_cols[2 * h + 1];
      hipLaunchKernelGGL(lokr_expand_kernel, dim3((unsigned)cdiv64((int64_t)m_ * n_, 256)), dim3(256), 0, nullptr, n.f[2 * h].as<float>(), n.f[2 * h + 1].as<float>(), m_,
                         r_, n_, n.x.as<double>() + (h ? n1 : 0));
      FMI_LAUNCH_CHECK();
    }
    FMI_HIP_TRY(hipDeviceSynchronize());  // the decomposed factors go: only their product stays resident
    for (int h = 0; h < 2; ++h)
      if (t->factor[2 * h + 1]) n.f[2 * h].reset(), n.f[2 * h + 1].reset();
    *out = std::move(n);
    return FMI_OK;
  }
  // the kinds built on rank sums: (rows, r) x (r, K) pairs.  LORA / DORA give (A, B); LOHA gives (w1_a, w1_b, w2_a, w2_b)
  const bool loha = t->kind == FMI_ADAPTER_LOHA;
  const int pairs = loha ? 2 : 1;
  for (int i = 0; i < 2 * pairs; ++i)
    if (!t->factor[i]) return fail(FMI_ERR_INVALID, what + ": null factor");
  for (int p = 0; p < pairs; ++p) {
    const int down = loha ? 2 * p + 1 : 0, up = loha ? 2 * p : 1;  // the (r, K) and the (rows, r) factor
    if (t->factor_cols[up] != t->factor_rows[down] || t->factor_rows[up] != rows || t->factor_cols[down] != K)
      return fail(FMI_ERR_INVALID, what + ": factors " + shape(up) + " x " + shape(down) + " do not give this Linear's shape, " + lin);
    if (p == 0) n.r = t->factor_rows[down];
    else if (t->factor_rows[down] != n.r)
      return fail(FMI_ERR_INVALID, what + ": LoHa ranks differ: w1 has " + std::to_string(n.r) + ", w2 has " + std::to_string(t->factor_rows[down]));
  }
  if (t->kind == FMI_ADAPTER_DORA && !t->magnitude) return fail(FMI_ERR_INVALID, what + ": DoRA needs the magnitude vector");
  for (int p = 0; p < pairs; ++p) {
    const int down = loha ? 2 * p + 1 : 0, up = loha ? 2 * p : 1;
    FMI_TRY(upload_f32(t->factor[down], t->dtype, numel(down), n.f[2 * p]));
    FMI_TRY(upload_f32(t->factor[up], t->dtype, numel(up), n.f[2 * p + 1]));
  }
  if (t->kind == FMI_ADAPTER_DORA) {
    if (!w0 || (reinterpret_cast<uintptr_t>(w0) & 15)) return fail(FMI_ERR_INVALID, what + ": DoRA needs the 16-byte aligned pristine rows");
    DeviceBuffer mag;
    FMI_TRY(upload_f32(t->magnitude, t->dtype, rows, mag));
    FMI_HIP_TRY(n.x.alloc((size_t)rows * 16));
    hipLaunchKernelGGL(dora_norm_kernel, dim3((unsigned)cdiv(rows, AT_N)), dim3(256), 0, nullptr, w0, rows, K, n.f[0].as<float>(), n.f[1].as<float>(), n.r, (double)t->scale,
                       mag.as<float>(), n.x.as<double>());
    FMI_LAUNCH_CHECK();
    std::vector<double> h((size_t)rows * 2);
    FMI_HIP_TRY(hipMemcpy(h.data(), n.x.ptr, h.size() * 8, hipMemcpyDeviceToHost));  // (waits for the null stream: `mag` may go after it)
    for (int i = 0; i < rows; ++i) {
      if (!(h[rows + i] > 0.0) || !std::isfinite(h[rows + i]))
        return fail(FMI_ERR_INVALID, what + ": DoRA row " + std::to_string(i) + " of W0 + scale * B A has norm " + std::to_string(h[rows + i]) + " (zero or not finite): m / n is undefined");
      if (!std::isfinite(h[i])) return fail(FMI_ERR_INVALID, what + ": DoRA magnitude of row " + std::to_string(i) + " is not finite");
    }
  }
  *out = std::move(n);
  return FMI_OK;
}

}  // namespace fmi

using namespace fmi;

extern "C" int fmi_adapter_merge(const void* w0, void* w, int rows, int K, const fmi_adapter_term* terms, const float* weights, int n_terms, void* stream) {
  if (!w0 || !w || n_terms < 0 || (n_terms && (!terms || !weights))) return fail(FMI_ERR_INVALID, "adapter_merge: null argument");
  if (rows <= 0 || K <= 0) return fail(FMI_ERR_INVALID, "adapter_merge: bad shape");
  if (K % 8) return fail(FMI_ERR_UNSUPPORTED, "adapter_merge: in_features must be a multiple of 8 (16-byte accesses along K)");
  if ((reinterpret_cast<uintptr_t>(w0) | reinterpret_cast<uintptr_t>(w)) & 15) return fail(FMI_ERR_INVALID, "adapter_merge: pointers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int i = 0; i < n_terms; ++i)
    if (!std::isfinite(weights[i])) return fail(FMI_ERR_INVALID, "adapter_merge: weights must be finite");
  FMI_HIP_TRY(hipStreamSynchronize(st));  // w0 may have been written on the caller's stream: the pre-passes run on the null stream
  std::vector<AdapterTerm> built((size_t)n_terms);
  std::vector<AdapterDesc> descs;
  for (int i = 0; i < n_terms; ++i) {
    FMI_TRY(adapter_term_build(&terms[i], static_cast<const bf16_t*>(w0), rows, K, "adapter_merge: term " + std::to_string(i), &built[(size_t)i]));
    if (weights[i] != 0.f) descs.push_back(adapter_term_desc(built[(size_t)i], (double)weights[i]));
  }
  DeviceBuffer dd;
  if (!descs.empty()) {
    FMI_HIP_TRY(dd.alloc(descs.size() * sizeof(AdapterDesc)));
    FMI_HIP_TRY(hipMemcpy(dd.ptr, descs.data(), descs.size() * sizeof(AdapterDesc), hipMemcpyHostToDevice));
  }
  FMI_HIP_TRY(hipDeviceSynchronize());  // (the pre-passes and uploads of the null stream, before the caller's stream reads them)
  int rc = launch_adapter_merge(static_cast<const bf16_t*>(w0), static_cast<bf16_t*>(w), rows, K, dd.as<AdapterDesc>(), (int)descs.size(), st);
  hipError_t e = hipStreamSynchronize(st);  // the terms' device copies are freed behind it
  if (rc == FMI_OK && e != hipSuccess) rc = fail(FMI_ERR_HIP, std::string("adapter_merge: ") + hipGetErrorString(e));
  return rc;
}
