// attention_d512.hip — flash attention for ONE head of width 512 on v_mfma_f32_16x16x32_bf16: the VAE mid block's AttnBlock (L = h w latent positions) without
// its (L, L) score matrix, and the op-level seam fmi_sdpa_d512_bf16.  DESIGN.md 4.25.
//
//   O = softmax(Q K^T * scale) V      q (B, Lq, 512), k, v (B, Lk, 512), o (B, Lq, 512) bf16 token-major, each with its own row and batch stride
//
// Work split.  A workgroup of 4 waves (one per SIMD) owns 64 NQ consecutive queries of one sample, wave w the 16 NQ queries from 16 NQ w on, as NQ blocks of 16.
// A block's Q is 16 MFMA B operands (64 VGPRs) and its O 32 accumulators of 4 (128 VGPRs), both resident for the whole key stream.  The launcher runs NQ = 1:
// 64 queries a workgroup.  NQ = 2 (128 queries: every K and V^T fragment read from LDS would feed two MFMAs, and K / V would be re-streamed half as often)
// needs 384 registers for Q and O alone; with the scores, P, the V staging and the addresses the compiler's allocation does not fit the 512 a wave has at one
// wave per SIMD — it spills 264 VGPRs (about 1 KB of scratch a lane) into the key loop — so that form waits for a hand-assigned instruction stream like the
// d = 128 kernels'.  NQ = 1 compiles to 256 VGPRs + 160 AGPRs without scratch, and makes twice as many workgroups, which is what L = 4096 (1024^2) needs: 64
// workgroups for 256 CUs.
//
// LDS: one 64-key K tile and one 64-key V^T tile, single-buffered, 66 560 + 73 728 = 140 288 of the 163 840 bytes.  The two are filled at different times,
// which is what a second buffer would buy: V(t) arrives under the score MFMAs of tile t, K(t + 1) under the P V MFMAs of tile t.  Two barriers a tile.
//   K tile: row = key, 1024 B of channels + 16 B pad (1040).  One LDS-DMA instruction (global_load_lds, 16 B a lane) moves one row; a wave moves 16 rows.
//     An A operand read is 16 B at (row 16 kb + n, channel 32 s + 8 g): the 16 lanes that share g read 16 rows at one column, 1040 n mod 256 = 16 n — sixteen
//     different 16-byte bank groups, no conflict.
//   V^T tile: row = channel, 64 keys (128 B) + 16 B pad (144).  V is consumed token-major and transposed ON THE WAY IN: a lane loads 8 channels of two
//     neighbouring keys (2 x 16 B) and writes eight 4-byte (channel, key pair) words (a plain transposing write; no ds_read_tr).  Key k of a tile sits at
//     position 32 (k >> 5) + 8 ((k >> 2) & 3) + 4 ((k >> 4) & 1) + (k & 3) of its row, so the 8 keys a lane needs for one 32-key step — 4 g .. 4 g + 3 of two
//     neighbouring 16-key blocks, which is how the score MFMA left P in its registers — are ONE 16-byte read.  Reads: 16 lanes, 16 rows, one column:
//     144 n mod 256 = 16 n + 128 (n & 1), sixteen different bank groups.  Writes: the 64 lanes of a store are 32 key pairs x 2 neighbouring channel octets, word
//     36 c + p with p a permutation of 0 .. 31 and c differing by 8 (288 = 32 mod 64): 64 different banks.
//
// Products (as attention_d64.hip).  S^T = K Q^T: the lane (n, g) of a 16 x 16 result holds query n, keys 4 g .. 4 g + 3 of the 16-key block; 16 k-steps of 32
// channels.  Softmax in f32 in the log2 domain (scale * log2 e folded into the score), keys >= Lk set to -inf BEFORE the maximum, p = 2^(s - m) rounded to bf16
// once — the rounded values feed the row sum and P V alike.  O^T = V^T P^T: A = V^T rows (channels), B = the lane's P values as they stand; the lane ends with
// query n, channels 16 dt + 4 g .. + 3.  O is rescaled only when some row's maximum moved (a wave-uniform branch; the factor is exactly 1 otherwise), divided by
// the f32 row sum at the end and rounded once.  K / V rows >= Lk re-read row Lk - 1 (valid memory; their P is exactly 0), query rows >= Lq re-read row Lq - 1 and
// are never stored.  Every tile holds a visible key, so the running maximum (-1e30 at the start, finite) is finite from the first tile on.
#include <cmath>

#include "common.h"

namespace fmi {
namespace {

constexpr int D512_KROW = 1040;                   // bytes of a K row in LDS
constexpr int D512_KTILE = 64 * D512_KROW;        // 66 560
constexpr int D512_VROW = 144;                    // bytes of a V^T row in LDS
constexpr int D512_VTILE = 512 * D512_VROW;       // 73 728
constexpr int D512_LDS = D512_KTILE + D512_VTILE;  // 140 288 <= 163 840
constexpr float D512_LOG2E = 1.44269504088896340736f;

struct D512Args {
  const bf16_t *q, *k, *v;
  bf16_t* o;
  int64_t rq, rk, rv, ro;  // row strides (elements)
  int64_t bq, bk, bv, bo;  // batch strides
  int Lq, Lk;
  float sl;  // scale * log2(e)
};

template <int NQ>
__global__ __launch_bounds__(256) void attention_d512_kernel(const D512Args a) {
  __shared__ __attribute__((aligned(16))) char smem[D512_LDS];  // K tile at 0, V^T tile behind it
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int b = blockIdx.y, qw = blockIdx.x * (64 * NQ) + wave * (16 * NQ);
  const int Lq = a.Lq, Lk = a.Lk;
  const bf16_t* Qb = a.q + (int64_t)b * a.bq;
  const bf16_t* Kb = a.k + (int64_t)b * a.bk;
  const bf16_t* Vb = a.v + (int64_t)b * a.bv;
  const int nt = (Lk + 63) >> 6;
  const bool live = qw < Lq;  // a wave without a query still stages its share of every tile

  // ---- staging.  K: the wave's rows 16 wave .. + 15, one DMA instruction a row (lane -> channels 8 lane .. + 7)
  auto k_request = [&](int t) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 16 * wave + i;
      const bf16_t* src = Kb + (int64_t)min(t * 64 + row, Lk - 1) * a.rk + lane * 8;
      __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(smem + row * D512_KROW), 16, 0, 0);
    }
  };
  // V: item j (0 .. 7) of a wave is the channel octets 16 wave + 2 j + {0, 1} of all 32 key pairs: lane -> octet (lane & 1), keys 2 (lane >> 1) + {0, 1}
  const int vkey = 2 * (lane >> 1);
  const int vpos = 32 * (vkey >> 5) + 8 * ((vkey >> 2) & 3) + 4 * ((vkey >> 4) & 1) + (vkey & 3);  // even: the pair is one 4-byte word
  auto v_load = [&](int t, int j, uint4 (&r)[2]) {
    const int oc = 16 * wave + 2 * j + (lane & 1);
#pragma unroll
    for (int e = 0; e < 2; ++e) r[e] = *reinterpret_cast<const uint4*>(Vb + (int64_t)min(t * 64 + vkey + e, Lk - 1) * a.rv + 8 * oc);
  };
  auto v_deposit = [&](int j, const uint4 (&r)[2]) {
    const int oc = 16 * wave + 2 * j + (lane & 1);
    char* vt = smem + D512_KTILE + (8 * oc) * D512_VROW + vpos * 2;
    const uint32_t w0[4] = {r[0].x, r[0].y, r[0].z, r[0].w}, w1[4] = {r[1].x, r[1].y, r[1].z, r[1].w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<uint32_t*>(vt + (2 * i) * D512_VROW) = (w0[i] & 0xffffu) | (w1[i] << 16);
      *reinterpret_cast<uint32_t*>(vt + (2 * i + 1) * D512_VROW) = (w0[i] >> 16) | (w1[i] & 0xffff0000u);
    }
  };

  // ---- Q fragments (B operand): block j, query qw + 16 j + n, channels 32 s + 8 g .. + 7
  bf16x8_t qf[NQ][16];
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    const bf16_t* qp = Qb + (int64_t)min(qw + 16 * j + n, Lq - 1) * a.rq + 8 * g;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const uint4 u = *reinterpret_cast<const uint4*>(qp + 32 * s);
      __builtin_memcpy(&qf[j][s], &u, 16);
    }
  }

  f32x4 o[NQ][32];  // O^T: query n, channels 16 dt + 4 g + {0..3}
  float m_run[NQ], l_part[NQ];
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    m_run[j] = -1e30f, l_part[j] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 32; ++dt) o[j][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  k_request(0);
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * 64;
    dma_barrier();  // K(t) has landed for every wave, and every wave is done with V^T(t - 1)
    // S^T = K Q^T, one 16-key block at a time, a quarter of V(t) loaded before it and written behind it
    f32x4 sc[NQ][4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      uint4 vr[2][2];
      v_load(t, 2 * kb, vr[0]);
      v_load(t, 2 * kb + 1, vr[1]);
#pragma unroll
      for (int j = 0; j < NQ; ++j) sc[j][kb] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (live) {
        const char* kr = smem + (16 * kb + n) * D512_KROW + 16 * g;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(kr + 64 * s);
#pragma unroll
          for (int j = 0; j < NQ; ++j) sc[j][kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[j][s], sc[j][kb], 0, 0, 0);
        }
      }
      v_deposit(2 * kb, vr[0]);
      v_deposit(2 * kb + 1, vr[1]);
    }
    // softmax step: scores in the log2 domain, keys past Lk masked by index in the ragged last tile only
    uint32_t pw[NQ][4][2];
    if (live) {
      const bool mask = k0 + 64 > Lk;
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float s = sc[j][kb][r] * a.sl;
            if (mask && k0 + 16 * kb + 4 * g + r >= Lk) s = -INFINITY;
            sc[j][kb][r] = s;
            mx = fmaxf(mx, s);
          }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run[j], mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run[j] - m_new);
        m_run[j] = m_new;
        float psum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const uint32_t u = pack_bf16x2(__builtin_amdgcn_exp2f(sc[j][kb][2 * r] - m_new), __builtin_amdgcn_exp2f(sc[j][kb][2 * r + 1] - m_new));
            pw[j][kb][r] = u;
            psum += __uint_as_float(u << 16) + __uint_as_float(u & 0xffff0000u);
          }
        l_part[j] = fmaf(l_part[j], alpha, psum);
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {  // some row's maximum moved
#pragma unroll
          for (int dt = 0; dt < 32; ++dt) o[j][dt] *= alpha;
        }
      }
    }
    __syncthreads();  // V^T(t) is complete, and every wave is done with K(t)
    if (t + 1 < nt) k_request(t + 1);
    // O^T += V^T P^T: step ks holds key blocks 2 ks, 2 ks + 1
    if (live) {
      const char* vb = smem + D512_KTILE + n * D512_VROW + 16 * g;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_t pf[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          const uint32_t pk[4] = {pw[j][2 * ks][0], pw[j][2 * ks][1], pw[j][2 * ks + 1][0], pw[j][2 * ks + 1][1]};
          __builtin_memcpy(&pf[j], pk, 16);
        }
#pragma unroll
        for (int dt = 0; dt < 32; ++dt) {
          const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(vb + (16 * dt) * D512_VROW + 64 * ks);
#pragma unroll
          for (int j = 0; j < NQ; ++j) o[j][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[j], o[j][dt], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: the row sum joined over the four g lanes, O / l as bf16, 4 channels a store
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    float l = l_part[j];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const int qi = qw + 16 * j + n;
    if (qi < Lq) {
      const float inv = 1.0f / l;
      bf16_t* op = a.o + (int64_t)b * a.bo + (int64_t)qi * a.ro + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 32; ++dt)
        *reinterpret_cast<uint2*>(op + 16 * dt) = uint2{pack_bf16x2(o[j][dt][0] * inv, o[j][dt][1] * inv), pack_bf16x2(o[j][dt][2] * inv, o[j][dt][3] * inv)};
    }
  }
}

}  // namespace

int launch_attention_d512(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, int B, int Lq, int Lk, const int64_t* st, float scale,
                          hipStream_t stream) {
  if (!q || !k || !v || !out) return fail(FMI_ERR_INVALID, "sdpa_d512: null pointer");
  if (B < 0 || Lq < 0 || Lk < 0) return fail(FMI_ERR_INVALID, "sdpa_d512: negative size");
  if (B > 65535) return fail(FMI_ERR_INVALID, "sdpa_d512: B must be at most 65535");
  if (!std::isfinite(scale)) return fail(FMI_ERR_INVALID, "sdpa_d512: scale must be finite");
  if (!all_aligned16({q, k, v, out})) return fail(FMI_ERR_INVALID, "sdpa_d512: operands must be 16-byte aligned");
  for (int i = 0; i < 4; ++i) {
    if (st[2 * i] < 512 || (st[2 * i] & 7)) return fail(FMI_ERR_INVALID, "sdpa_d512: row strides must be multiples of 8 and at least 512");
    if (st[2 * i + 1] < 0 || (st[2 * i + 1] & 7)) return fail(FMI_ERR_INVALID, "sdpa_d512: batch strides must be non-negative multiples of 8");
  }
  if (B > 1 && st[7] < (int64_t)(Lq - 1) * st[6] + 512) return fail(FMI_ERR_INVALID, "sdpa_d512: the output's batch stride is smaller than one sample");
  if (B == 0 || Lq == 0) return FMI_OK;
  if (Lk == 0) return fail(FMI_ERR_INVALID, "sdpa_d512: no keys");
  D512Args a{};
  a.q = q, a.k = k, a.v = v, a.o = out;
  a.rq = st[0], a.bq = st[1], a.rk = st[2], a.bk = st[3], a.rv = st[4], a.bv = st[5], a.ro = st[6], a.bo = st[7];
  a.Lq = Lq, a.Lk = Lk, a.sl = scale * D512_LOG2E;
  hipLaunchKernelGGL(attention_d512_kernel<1>, dim3(cdiv(Lq, 64), B), dim3(256), 0, stream, a);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

}  // namespace fmi
