// ip_adapter.hip — the FLUX IP-Adapter (XLabs flux-ip-adapter, diffusers' FluxIPAdapterAttnProcessor): image-prompt attention in the double blocks.
//
//   ip_attention   per sample b, image row r and head h, over the adapter's N <= 32 image-prompt tokens:
//                    v   = f32(q_raw[b, r, h, :])                          the q|k|v GEMM's plain bf16 output, before QkNorm and RoPE
//                    qn  = v * rsqrt(mean(v^2) + 1e-6) * f32(norm_q)       the block's RMSNorm, f32, not rounded to bf16
//                    s_n = (qn . f32(K[b, h, n, :])) * (1 / sqrt(128))     K, V stored as bf16 (B, H, N, 128): no QkNorm, no RoPE
//                    e_n = exp(s_n - max_n s),  den = sum_n e_n
//                    ip  = (sum_n e_n * f32(V[b, h, n, :])) * (1 / den)    f32 accumulation
//                    x[b, r, h * 128 + :] = fadd(x, fmul(c, ip))           one rounded product, one rounded sum, never contracted into an fma
//                  Bandwidth-bound: q is read once, x read and written once, in 16-byte accesses; K / V of the block's heads sit in LDS.  A 16-lane DPP row owns
//                  one (row, head): 8 elements per lane, the 128-wide sums by row16_sum (no LDS, no atomics).  Every (row, head) is computed on its own, so the
//                  result does not depend on the grid or on what else runs.
//   the projection once per call: tok = LayerNorm(eps 1e-5, affine)(Linear(E -> N * J)(embeds)) in f32 (bf16 weights, the streaming GEMV of small_ops.hip), K_i / V_i
//                  = Linear(J -> D)(tok) for all blocks in one GEMV over the stacked weights, f32 accumulation, rounded once to bf16 into the (B, H, N, 128) layout.
//   the handle     fmi_ip_adapter_create / _set_tensor / _missing_* / _destroy.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "ip_adapter.h"

using namespace fmi;

namespace {

__device__ __forceinline__ void unpack8(const uint4 r, float (&v)[8]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) v[2 * k] = __uint_as_float(w[k] << 16), v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
}

// One workgroup: sample blockIdx.z, the HT (1, 2 or 4) heads from blockIdx.y * HT, rows blockIdx.x * (16 / HT) + k * gridDim.x * (16 / HT).  Its 16 DPP rows are
// (row, head) pairs: head = group % HT, row = group / HT — with HT == 4 a wave reads 1 KiB of one q row and 2 KiB of one x row.  LDS: K then V of the HT heads,
// [HT][N][128] bf16 each (the (B, H, N, 128) layout makes that one contiguous piece per array).  NMAX: the unrolled token count, N <= NMAX.
template <int NMAX>
__global__ __launch_bounds__(256) void ip_attention_kernel(const bf16_t* __restrict__ q, int ldq, int64_t q_bs, const bf16_t* __restrict__ wq, const bf16_t* __restrict__ K,
                                                           const bf16_t* __restrict__ V, float* __restrict__ x, int64_t x_bs, int H, int S, int N, int HT, float c) {
  extern __shared__ __attribute__((aligned(16))) uint4 kv[];
  const int b = blockIdx.z, h0 = blockIdx.y * HT;
  const int per = HT * N * 16;  // uint4 per array
  {
    const uint4* Kg = reinterpret_cast<const uint4*>(K + ((int64_t)b * H + h0) * N * 128);
    const uint4* Vg = reinterpret_cast<const uint4*>(V + ((int64_t)b * H + h0) * N * 128);
    for (int i = threadIdx.x; i < per; i += 256) kv[i] = Kg[i], kv[per + i] = Vg[i];
  }
  __syncthreads();
  const int g = threadIdx.x >> 4, sub = threadIdx.x & 15;
  const int hl = g % HT, rpp = 16 / HT, h = h0 + hl;
  const uint4* Kl = kv + hl * N * 16 + sub;
  const uint4* Vl = kv + per + hl * N * 16 + sub;
  float w[8];
  unpack8(*reinterpret_cast<const uint4*>(wq + sub * 8), w);
  const bf16_t* qp = q + (int64_t)b * q_bs + h * 128 + sub * 8;
  float* xp = x + (int64_t)b * x_bs + h * 128 + sub * 8;
  const int64_t ldx = (int64_t)H * 128;
  const int stride = gridDim.x * rpp;
  int r = blockIdx.x * rpp + g / HT;
  // the next row's q and x are requested before this row is computed (two rows in flight per lane)
  uint4 qr = make_uint4(0, 0, 0, 0);
  float4 lo = make_float4(0, 0, 0, 0), hi = lo;
  if (r < S) {
    qr = *reinterpret_cast<const uint4*>(qp + (int64_t)r * ldq);
    lo = *reinterpret_cast<const float4*>(xp + r * ldx), hi = *reinterpret_cast<const float4*>(xp + r * ldx + 4);
  }
  while (r < S) {
    const int rn = r + stride;
    uint4 qn_raw = qr;
    float4 nlo = lo, nhi = hi;
    if (rn < S) {
      qn_raw = *reinterpret_cast<const uint4*>(qp + (int64_t)rn * ldq);
      nlo = *reinterpret_cast<const float4*>(xp + rn * ldx), nhi = *reinterpret_cast<const float4*>(xp + rn * ldx + 4);
    }
    float v[8];
    unpack8(qr, v);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ss += v[i] * v[i];
    const float inv = rms_inv128(row16_sum(ss));
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = v[i] * inv * w[i];
    float sc[NMAX];
    float mx = -INFINITY;
#pragma unroll
    for (int n = 0; n < NMAX; ++n) {
      if (n < N) {
        float k[8];
        unpack8(Kl[n * 16], k);
        float p = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) p = fmaf(v[i], k[i], p);
        sc[n] = row16_sum(p) * 0.08838834764831845f;
        mx = fmaxf(mx, sc[n]);
      }
    }
    float den = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < NMAX; ++n) {
      if (n < N) {
        const float e = __builtin_amdgcn_exp2f((sc[n] - mx) * 1.44269504088896340736f);
        den += e;
        float vv[8];
        unpack8(Vl[n * 16], vv);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(e, vv[i], acc[i]);
      }
    }
    const float rd = 1.0f / den;
    lo.x = __fadd_rn(lo.x, __fmul_rn(c, acc[0] * rd)), lo.y = __fadd_rn(lo.y, __fmul_rn(c, acc[1] * rd));
    lo.z = __fadd_rn(lo.z, __fmul_rn(c, acc[2] * rd)), lo.w = __fadd_rn(lo.w, __fmul_rn(c, acc[3] * rd));
    hi.x = __fadd_rn(hi.x, __fmul_rn(c, acc[4] * rd)), hi.y = __fadd_rn(hi.y, __fmul_rn(c, acc[5] * rd));
    hi.z = __fadd_rn(hi.z, __fmul_rn(c, acc[6] * rd)), hi.w = __fadd_rn(hi.w, __fmul_rn(c, acc[7] * rd));
    *reinterpret_cast<float4*>(xp + r * ldx) = lo;
    *reinterpret_cast<float4*>(xp + r * ldx + 4) = hi;
    qr = qn_raw, lo = nlo, hi = nhi, r = rn;
  }
}

// LayerNorm(eps, affine) of `rows` rows of J f32, one workgroup per row; the statistics as layernorm_mod_kernel takes them (E[x^2] - mean^2).
__global__ __launch_bounds__(256) void ip_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y,
                                                           int J, float eps) {
  __shared__ float red[2][4];
  const float* xr = x + (int64_t)blockIdx.x * J;
  float s = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < J; i += 256) {
    const float v = xr[i];
    s += v, s2 += v * v;
  }
  s = wave_sum(s), s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = s, red[1][threadIdx.x >> 6] = s2;
  __syncthreads();
  s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  s2 = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  const float mean = s / (float)J, var = s2 / (float)J - mean * mean;
  const float inv_std = 1.0f / sqrtf(var + eps);
  float* yr = y + (int64_t)blockIdx.x * J;
  for (int i = threadIdx.x; i < J; i += 256) yr[i] = (xr[i] - mean) * inv_std * gamma[i] + beta[i];
}

// (Bt * N, nd * 2 * D) f32 -> (nd * 2, Bt, H, N, 128) bf16, rounded once (RNE)
__global__ __launch_bounds__(256) void ip_kv_pack_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int Bt, int N, int D, int n2, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int e = (int)(i % 128);
    int64_t t = i / 128;
    const int n = (int)(t % N);
    t /= N;
    const int H = D / 128, h = (int)(t % H);
    t /= H;
    const int b = (int)(t % Bt), iw = (int)(t / Bt);
    dst[i] = f32_to_bf16(src[((int64_t)b * N + n) * ((int64_t)n2 * D) + (int64_t)iw * D + h * 128 + e]);
  }
}

int ip_ensure(fmi_ip_adapter* a, int Bt, hipStream_t s) {
  const size_t rows = (size_t)Bt * a->N, n2 = (size_t)a->nd * 2;
  if (a->kv.bytes() < n2 * rows * a->D * 2) {
    FMI_HIP_TRY(hipStreamSynchronize(s));
    if (a->emb.alloc((size_t)Bt * a->E * 4) != hipSuccess || a->tok.alloc(2 * rows * a->J * 4) != hipSuccess || a->kv_f32.alloc(rows * n2 * a->D * 4) != hipSuccess ||
        a->kv.alloc(n2 * rows * a->D * 2) != hipSuccess) {
      a->emb.reset(), a->tok.reset(), a->kv_f32.reset(), a->kv.reset();
      return fail(FMI_ERR_NOMEM, "ip_adapter: hipMalloc of the projection buffers failed");
    }
  }
  a->kv_B = Bt;
  return FMI_OK;
}

}  // namespace

namespace fmi {

int launch_ip_attention(const bf16_t* q, int ldq, int64_t q_bs, const bf16_t* wq, const bf16_t* K, const bf16_t* V, float* x, int64_t x_bs, int B, int H, int S, int N,
                        float c, int max_row_blocks, hipStream_t stream) {
  if (!q || !wq || !K || !V || !x || B < 0 || H <= 0 || S < 0 || max_row_blocks < 0) return fail(FMI_ERR_INVALID, "ip_attention: null pointer or negative size");
  if (N < 1 || N > IP_MAX_TOKENS)
    return fail(FMI_ERR_UNSUPPORTED, "ip_attention: num_tokens N = " + std::to_string(N) + " is outside the supported 1 <= N <= " + std::to_string(IP_MAX_TOKENS));
  const int64_t D = (int64_t)H * 128;
  if (ldq < D || ldq % 8 || q_bs % 8 || q_bs < (int64_t)S * ldq) return fail(FMI_ERR_INVALID, "ip_attention: q needs a row stride >= H * 128 and a batch stride >= S * ldq, both multiples of 8");
  if (x_bs < (int64_t)S * D || x_bs % 4) return fail(FMI_ERR_INVALID, "ip_attention: the batch stride of x must be at least S * H * 128 and a multiple of 4");
  if (!all_aligned16({q, wq, K, V, x})) return fail(FMI_ERR_INVALID, "ip_attention: every pointer must be 16-byte aligned");
  if (B > 65535) return fail(FMI_ERR_UNSUPPORTED, "ip_attention: B > 65535");
  if (B == 0 || S == 0) return FMI_OK;
  int HT = H % 4 == 0 ? 4 : H % 2 == 0 ? 2 : 1;
  while (HT > 1 && (size_t)HT * N * 512 > 32 * 1024) HT /= 2;  // K + V of HT heads: HT * N * 512 bytes of LDS, at most 32 KiB
  const int rpp = 16 / HT;
  const int row_blocks = std::min(cdiv(S, rpp), max_row_blocks ? max_row_blocks : 256);
  const dim3 grid((unsigned)row_blocks, (unsigned)(H / HT), (unsigned)B);
  const size_t lds = (size_t)HT * N * 512;
#define FMI_IP_LAUNCH(NMAX) hipLaunchKernelGGL((ip_attention_kernel<NMAX>), grid, dim3(256), lds, stream, q, ldq, q_bs, wq, K, V, x, x_bs, H, S, N, HT, c)
  if (N <= 4) FMI_IP_LAUNCH(4);
  else if (N <= 8) FMI_IP_LAUNCH(8);
  else if (N <= 16) FMI_IP_LAUNCH(16);
  else FMI_IP_LAUNCH(32);
#undef FMI_IP_LAUNCH
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

int ip_prepare(fmi_ip_adapter* a, const void* embeds, const void* neg_embeds, fmi_dtype dt, int Bs, bool with_negative, hipStream_t s) {
  const int Bt = with_negative ? 2 * Bs : Bs, rows = Bt * a->N, n2 = a->nd * 2;
  FMI_TRY(ip_ensure(a, Bt, s));
  float* emb = a->emb.as<float>();
  FMI_TRY(launch_cast_to_f32(embeds, dt, emb, (int64_t)Bs * a->E, s));
  if (with_negative) {
    if (neg_embeds) FMI_TRY(launch_cast_to_f32(neg_embeds, dt, emb + (size_t)Bs * a->E, (int64_t)Bs * a->E, s));
    else FMI_HIP_TRY(hipMemsetAsync(emb + (size_t)Bs * a->E, 0, (size_t)Bs * a->E * 4, s));  // diffusers: zero embeddings through the same projection
  }
  float *raw = a->tok.as<float>(), *tok = raw + (size_t)rows * a->J;
  FMI_TRY(launch_gemv(emb, a->proj_w, a->proj_b, raw, Bt, a->N * a->J, a->E, 0, 0, s));  // (Bt, N * J) == (Bt * N, J)
  hipLaunchKernelGGL(ip_layernorm_kernel, dim3(rows), dim3(256), 0, s, raw, a->ln_w, a->ln_b, tok, a->J, 1e-5f);
  FMI_LAUNCH_CHECK();
  FMI_TRY(launch_gemv(tok, a->kv_w, a->kv_b, a->kv_f32.as<float>(), rows, n2 * a->D, a->J, 0, 0, s));
  const int64_t total = (int64_t)n2 * rows * a->D;
  hipLaunchKernelGGL(ip_kv_pack_kernel, map_grid(total), dim3(256), 0, s, a->kv_f32.as<float>(), a->kv.as<bf16_t>(), Bt, a->N,
                     a->D, n2, total);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

}  // namespace fmi

// ---------------------------------------------------------------------------------------- C-ABI
extern "C" int fmi_ip_adapter_create(const fmi_flux_config* cfg, int embed_dim, int num_tokens, fmi_ip_adapter** out) {
  if (!cfg || !out) return fail(FMI_ERR_INVALID, "ip_adapter_create: null argument");
  if (cfg->num_attention_heads < 1 || cfg->num_layers < 1) return fail(FMI_ERR_INVALID, "ip_adapter_create: the transformer needs at least one head and one double block");
  if (embed_dim < 8 || embed_dim % 8 || embed_dim > 16384) return fail(FMI_ERR_INVALID, "ip_adapter_create: embed_dim must be a multiple of 8 in [8, 16384]");
  if (cfg->joint_attention_dim < 8 || cfg->joint_attention_dim % 8 || cfg->joint_attention_dim > 16384)
    return fail(FMI_ERR_INVALID, "ip_adapter_create: joint_attention_dim must be a multiple of 8 in [8, 16384]");
  if (num_tokens < 1 || num_tokens > IP_MAX_TOKENS)
    return fail(FMI_ERR_UNSUPPORTED, "ip_adapter_create: num_tokens N = " + std::to_string(num_tokens) + " is outside the supported 1 <= N <= " + std::to_string(IP_MAX_TOKENS));
  auto* a = new fmi_ip_adapter();
  hipGetDevice(&a->device);
  a->H = cfg->num_attention_heads, a->D = a->H * 128, a->J = cfg->joint_attention_dim, a->nd = cfg->num_layers, a->E = embed_dim, a->N = num_tokens;
  const size_t NJ = (size_t)a->N * a->J, n2D = (size_t)a->nd * 2 * a->D;
  size_t off = 0;
  const auto take = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) / 256 * 256;
    return o;
  };
  const size_t o_pw = take(NJ * a->E * 2), o_pb = take(NJ * 2), o_lw = take((size_t)a->J * 4), o_lb = take((size_t)a->J * 4), o_kw = take(n2D * a->J * 2), o_kb = take(n2D * 2);
  if (a->weights.alloc(off) != hipSuccess || hipMemset(a->weights.ptr, 0, off) != hipSuccess) {
    delete a;
    return fail(FMI_ERR_NOMEM, "ip_adapter_create: hipMalloc of " + std::to_string(off) + " bytes of weights failed");
  }
  char* base = a->weights.as<char>();
  a->proj_w = (bf16_t*)(base + o_pw), a->proj_b = (bf16_t*)(base + o_pb), a->ln_w = (float*)(base + o_lw), a->ln_b = (float*)(base + o_lb);
  a->kv_w = (bf16_t*)(base + o_kw), a->kv_b = (bf16_t*)(base + o_kb);
  for (const char* n : {"image_proj.image_embeds.weight", "image_proj.image_embeds.bias", "image_proj.norm.weight", "image_proj.norm.bias"}) a->missing.insert(n);
  for (int i = 0; i < a->nd; ++i)  // (the biases of to_k_ip / to_v_ip are optional: zero unless the file has them)
    for (const char* kv : {"to_k_ip", "to_v_ip"}) a->missing.insert("ip_adapter." + std::to_string(i) + "." + kv + ".weight");
  *out = a;
  return FMI_OK;
}

extern "C" void fmi_ip_adapter_destroy(fmi_ip_adapter* a) {
  if (!a) return;
  (void)use_device_ordinal(a->device);
  (void)hipDeviceSynchronize();
  delete a;
}

extern "C" int fmi_ip_adapter_set_tensor(fmi_ip_adapter* a, const char* name, const void* data, fmi_dtype dtype, const int64_t* shape, int rank) {
  if (!a || !name || !data || !shape) return fail(FMI_ERR_INVALID, "ip_adapter_set_tensor: null argument");
  if (dtype != FMI_F32 && dtype != FMI_F16 && dtype != FMI_BF16) return fail(FMI_ERR_INVALID, "ip_adapter_set_tensor: dtype must be F32, F16 or BF16");
  FMI_TRY(use_device_ordinal(a->device));
  const std::string n = name;
  const int64_t NJ = (int64_t)a->N * a->J;
  int64_t want[2] = {0, 0};
  int want_rank = 1;
  bf16_t* dst16 = nullptr;
  float* dst32 = nullptr;
  if (n == "image_proj.image_embeds.weight") dst16 = a->proj_w, want[0] = NJ, want[1] = a->E, want_rank = 2;
  else if (n == "image_proj.image_embeds.bias") dst16 = a->proj_b, want[0] = NJ;
  else if (n == "image_proj.norm.weight") dst32 = a->ln_w, want[0] = a->J;
  else if (n == "image_proj.norm.bias") dst32 = a->ln_b, want[0] = a->J;
  else {
    int i = -1, used = 0;
    char which = 0, kind[8] = {0};
    if (sscanf(name, "ip_adapter.%d.to_%c_ip.%6[a-z]%n", &i, &which, kind, &used) != 3 || name[used] || i < 0 || i >= a->nd || (which != 'k' && which != 'v') ||
        (strcmp(kind, "weight") && strcmp(kind, "bias")))
      return fail(FMI_ERR_INVALID, "ip_adapter_set_tensor: unknown tensor name '" + n + "'");
    const size_t row0 = ((size_t)i * 2 + (which == 'v')) * a->D;
    if (!strcmp(kind, "weight")) dst16 = a->kv_w + row0 * a->J, want[0] = a->D, want[1] = a->J, want_rank = 2;
    else dst16 = a->kv_b + row0, want[0] = a->D;
  }
  if (rank != want_rank || shape[0] != want[0] || (want_rank == 2 && shape[1] != want[1]))
    return fail(FMI_ERR_INVALID, "ip_adapter_set_tensor: " + n + " must be (" + std::to_string(want[0]) + (want_rank == 2 ? ", " + std::to_string(want[1]) : "") + ")");
  const int64_t count = want[0] * (want_rank == 2 ? want[1] : 1);
  if (dst16) FMI_TRY(upload_as_bf16(data, dtype, count, dst16));
  else FMI_TRY(upload_as_f32(data, dtype, count, dst32));
  a->missing.erase(n);
  return FMI_OK;
}

extern "C" int fmi_ip_adapter_missing_count(const fmi_ip_adapter* a) { return a ? a->missing.count() : 0; }
extern "C" const char* fmi_ip_adapter_missing_name(const fmi_ip_adapter* a, int i) { return a ? a->missing.name(i) : nullptr; }
extern "C" size_t fmi_ip_adapter_size_in_bytes(const fmi_ip_adapter* a) {
  return a ? a->weights.bytes() + a->emb.bytes() + a->tok.bytes() + a->kv_f32.bytes() + a->kv.bytes() : 0;
}

extern "C" int fmi_ip_attention(const void* q_bf16, int q_row_stride, int64_t q_batch_stride, const void* norm_q_bf16, const void* k_bf16, const void* v_bf16, float* x_f32,
                                int64_t x_batch_stride, int B, int H, int S, int N, float scale, int max_row_blocks, void* stream) {
  return launch_ip_attention((const bf16_t*)q_bf16, q_row_stride, q_batch_stride, (const bf16_t*)norm_q_bf16, (const bf16_t*)k_bf16, (const bf16_t*)v_bf16, x_f32,
                             x_batch_stride, B, H, S, N, scale, max_row_blocks, (hipStream_t)stream);
}
