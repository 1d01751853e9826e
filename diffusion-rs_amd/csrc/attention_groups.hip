// attention_groups.hip — joint attention at head dim 128 with TOKEN GROUP MASKS on v_mfma_f32_16x16x32_bf16: regional prompts, key padding, any "token i may
// not see token j" that is a property of the two tokens.  DESIGN.md 4.23.
//
//   O = softmax(Q K^T * scale + M) V,   M[i][j] = 0 where (qg[i] & kg[j]) != 0, else -inf
//
// Every token carries one 32-bit group word, per sample and shared by all heads: the mask is O(L) metadata, never an L^2 operand.  The caller guarantees a
// visible key for every query (the entries check qg[i] & kg[i] where Lq == Lk), so there is no empty-row branch: the running maximum starts at -1e30, finite.
// q, k head-major (B H, L, 128) bf16 and V as launch_v_transpose's image (B H, 128, Lpad) — what the model's q|k|v epilogue already writes — so the kernel
// stands in for launch_attention_ex at the two call sites of forward_core without a relayout.  Output through AttnOut.
//
// Work split.  A workgroup of 4 waves owns 128 consecutive queries of one (batch, head); a wave owns 32 of them as TWO 16-query fragments, so that every K and
// V^T operand read from LDS feeds two MFMAs.  Q stays in registers as B operands (2 x 4 k-steps), S^T = K Q^T and O^T = V^T P^T: a result lane (n = lane & 15,
// g = lane >> 4) holds ONE query of each fragment, row reductions are the lane's own values and two shuffles.  O^T is 2 x 8 accumulators (64 registers).
//
// Key identity through the V^T permutation.  Position p of the image holds key vt_perm(p) (bits 2 and 3 swapped inside a group of 16: attention.hip).  The PV
// k-step ks reads V^T as it lies: lane g's A operand is the 16 bytes at positions 32 ks + 8 g .. + 7.  Its B operand must hold P of the SAME keys, so the score
// MFMAs choose their K rows accordingly — the A row a lane feeds is free: score group (ks, j), lane n reads key row 32 ks + (n & 7) + 8 j + 16 (n >> 3), and
// result register r of lane g is then the key at position 32 ks + 8 g + 4 j + r.  The two groups of a k-step are the lane's P operand as they stand; no
// shuffle, no second read width.  The key WORDS are staged per tile in position order by the same map (keys past Lk: word 0, which masks the ragged tail).
//
// Data movement.  Key tiles are 64 wide: K 64 rows x 256 B, V^T 128 rows x 128 B, both by LDS-DMA (16 B a lane, 1-KiB pieces, 8 per wave and tile) and both
// double-buffered (64 KiB + 512 B of key words); one barrier per tile.  Swizzles, applied through the global address a lane fetches: K chunk c of row r at
// c ^ ((r & 7) | ((r >> 4 & 1) << 3)) — the 16 rows of a score read differ in exactly those bits, so they cover all 16 chunk positions; V^T chunk c of row r
// at c ^ ((r >> 1) & 7), attention.hip's.
//
// Tile summaries.  key_tile_summary_kernel writes the OR and the AND of the key words of every 64-key tile (once per group set in the model, per call at the op
// level).  The workgroup reduces the OR of its queries' words, each wave its own OR and AND.  A tile whose OR misses the workgroup's OR is never fetched (the
// next tile to visit is found by scanning the summaries); a visited tile whose OR misses a WAVE's OR is skipped by that wave; a full tile with
// (wave AND & tile AND) != 0 has every pair visible and takes the unmasked path; only the rest apply the per-element -inf.  A row without a visible key in a
// visited tile gets p = 2^(-inf - m) = 0 for all of it and alpha = 1: the tile contributes exactly nothing.
// Known cost: next_tile and the per-tile summary reads are dependent scalar global loads in front of every fetch — latency the generated unmasked stream does
// not have, and part of what the all-visible case pays.
//
// Rounding: p is rounded to bf16 once, the rounded values feed both the row sum and P V.  Vector loads and stores only; no workspace beyond the V^T image and
// the summaries; asynchronous.
//
// Key weights (the W instantiation).  O_i = sum_j w_j e^(s_ij) v_j / sum_j w_j e^(s_ij) over the keys query i sees: one positive f32 weight per
// key, per sample and shared by heads and queries, which is softmax(s + ln w).  key_weight_log2_kernel turns w into lw = log2 w once per set; the kernel stages
// 768 + lw per tile in LDS next to the key words, in the same position order, so result register r of a lane finds its key's term in the float4 it reads for its
// score group.  The term enters as t = fma(s, scale log2e, 768 + lw) - 768: in front of the -inf of a hidden pair, the running maximum and exp2.  The bias 768
// puts the sum in [512, 1024), so t lies on the 2^-14 grid (for |t| < 256; a relative step of 4e-5 in p, under bf16's 2e-3) and lw lies on it by construction
// (exponent + log2 of the mantissa rounded to the grid): doubling every weight moves every t and the maximum by exactly 1 and no output bit.  The summaries'
// third word is 1 where every key of a tile has lw == 0: such a tile takes the unweighted path to the letter (s * scale log2e, the unmasked fast path where the
// AND words allow it), only the others pay the fma and the subtraction.  Keys past Lk stage the term 0 and the word 0.
#include <cmath>

#include "common.h"

namespace fmi {
namespace {

constexpr int AG_QBLK = 128;           // queries per workgroup
constexpr int AG_TILE = 16384;         // bytes of a K tile and of a V^T tile
constexpr int AG_VT = 2 * AG_TILE;     // V^T tiles [2] behind the K tiles [2]
constexpr int AG_KW = 4 * AG_TILE;     // key words [2][64] behind them
constexpr int AG_RED = AG_KW + 2 * 256;  // the workgroup's OR reduction, one word a wave
constexpr int AG_LW = AG_RED + 16;       // W only: the keys' biased log2 weights [2][64] f32, behind everything the unweighted kernel uses
constexpr float AG_BIAS = 768.f;         // 1.5 * 2^9: sums in [512, 1024) round to multiples of 2^-14
constexpr float AG_GRID = 16384.f;
constexpr float LOG2E = 1.44269504088896340736f;

struct GroupArgs {
  const bf16_t *q, *k, *vt;
  AttnOut out;
  const uint32_t *qg, *kg, *ksum;  // words (gb, Lq), (gb, Lk); summaries (gb, nt, {OR, AND, every lw == 0, -})
  const float* lw;                 // W only: log2 of the key weights (gb, Lk)
  int64_t qg_bs, kg_bs, ksum_bs;   // their sample strides (0: one set for the whole batch); kg_bs is lw's too
  int H, Lq, Lk, Lkpad, nt;
  float sl;  // scale * log2(e)
};

__device__ __forceinline__ int vt_perm16(int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); }

template <bool W>  // W: per-key weights (the header comment); the other instantiation has no trace of them
__global__ __launch_bounds__(256, 2) void attention_groups_kernel(const GroupArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[W ? AG_LW + 2 * 256 : AG_RED + 16];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nqb = (a.Lq + AG_QBLK - 1) / AG_QBLK, id = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = id / nqb, q0 = (id % nqb) * AG_QBLK, b = bh / a.H, h = bh % a.H, qw = q0 + wave * 32;
  const int Lq = a.Lq, Lk = a.Lk, nt = a.nt;
  const bf16_t* Kb = a.k + (int64_t)bh * Lk * 128;
  const bf16_t* Vb = a.vt + (int64_t)bh * 128 * a.Lkpad;
  const uint32_t* kgb = a.kg + b * a.kg_bs;
  const uint32_t* ksb = a.ksum + b * a.ksum_bs;
  const float* lwb = W ? a.lw + b * a.kg_bs : nullptr;
  const bool live = qw < Lq;  // a wave without a query still stages its share of every tile

  // ---- Q fragments (B operands) and the lane's two query words.  Rows past Lq read row Lq - 1 (its word too: the reductions are unchanged) and are not stored.
  bf16x8_t qf[2][4];
  uint32_t qword[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int row = min(qw + 16 * f + n, Lq - 1);
    const bf16_t* qp = a.q + ((int64_t)bh * Lq + row) * 128 + 8 * g;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[f][s] = *reinterpret_cast<const bf16x8_t*>(qp + 32 * s);
    qword[f] = a.qg[b * a.qg_bs + row];
  }
  uint32_t w_or = qword[0] | qword[1], w_and = qword[0] & qword[1];
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) w_or |= __shfl_xor(w_or, o, 64), w_and &= __shfl_xor(w_and, o, 64);
  w_or = __builtin_amdgcn_readfirstlane(w_or), w_and = __builtin_amdgcn_readfirstlane(w_and);
  uint32_t* red = reinterpret_cast<uint32_t*>(smem + AG_RED);
  if (lane == 0) red[wave] = w_or;
  __syncthreads();
  const uint32_t wg_or = __builtin_amdgcn_readfirstlane(red[0] | red[1] | red[2] | red[3]);
  auto next_tile = [&](int t) {  // the first tile from t on that holds a key some query of the workgroup sees
    while (t < nt && !(ksb[4 * t] & wg_or)) ++t;
    return t;
  };

  // ---- staging.  K piece p = 4 wave + i is rows 4 p .. 4 p + 3 (lane >> 4), LDS chunk lane & 15; V^T piece p is rows 8 p .. 8 p + 7 (lane >> 3), chunk lane & 7
  uint32_t kwreg = 0;
  float lwreg = 0.f;
  auto request = [&](int t, int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = wave * 4 + i, kr = p * 4 + (lane >> 4), vr = p * 8 + (lane >> 3);
      const bf16_t* ks = Kb + (int64_t)min(t * 64 + kr, Lk - 1) * 128 + (((lane & 15) ^ ((kr & 7) | (((kr >> 4) & 1) << 3))) << 3);
      __builtin_amdgcn_global_load_lds((glb_void*)ks, (lds_void*)(smem + buf * AG_TILE + p * 1024), 16, 0, 0);
      const bf16_t* vs = Vb + (int64_t)vr * a.Lkpad + t * 64 + (((lane & 7) ^ ((vr >> 1) & 7)) << 3);
      __builtin_amdgcn_global_load_lds((glb_void*)vs, (lds_void*)(smem + AG_VT + buf * AG_TILE + p * 1024), 16, 0, 0);
    }
    if (tid < 64) {  // the word of the key at position tid of the tile
      const int key = t * 64 + vt_perm16(tid);
      kwreg = key < Lk ? kgb[key] : 0u;
      if (W) lwreg = key < Lk ? lwb[key] : 0.f;
    }
  };
  auto deposit = [&](int buf) {
    if (tid < 64) {
      reinterpret_cast<uint32_t*>(smem + AG_KW + buf * 256)[tid] = kwreg;
      if (W) reinterpret_cast<float*>(smem + AG_LW + buf * 256)[tid] = AG_BIAS + lwreg;  // exact: lw is a multiple of 2^-14 and small against 256
    }
  };

  f32x4 o[2][8];  // O^T: fragment f, query n, channels 16 dt + 4 g + {0..3}
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[f][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-1e30f, -1e30f}, l_part[2] = {0.f, 0.f};

  int t = next_tile(0), cur = 0;
  if (t < nt) {
    request(t, 0);
    deposit(0);
  }
  while (t < nt) {
    dma_barrier();  // tile t has landed for every wave, and every wave is done with the other buffers
    const int tn = next_tile(t + 1);
    if (tn < nt) request(tn, cur ^ 1);
    const uint32_t t_or = ksb[4 * t], t_and = ksb[4 * t + 1];
    const bool weigh = W && !ksb[4 * t + 2];  // some key of this tile has lw != 0 (uniform over the workgroup)
    if (live && (t_or & w_or)) {
      // S^T = K Q^T: group (ks, j) of the header comment, both fragments off one operand read
      const char* kt = smem + cur * AG_TILE;
      f32x4 sc[2][4];
#pragma unroll
      for (int grp = 0; grp < 4; ++grp) {
        sc[0][grp] = sc[1][grp] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int r = 32 * (grp >> 1) + (n & 7) + 8 * (grp & 1) + 16 * (n >> 3);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(kt + r * 256 + (((4 * s + g) ^ n) << 4));
          sc[0][grp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[0][s], sc[0][grp], 0, 0, 0);
          sc[1][grp] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[1][s], sc[1][grp], 0, 0, 0);
        }
      }
      // the keys' terms, where this tile has one: t = s * scale log2e + lw on the 2^-14 grid, for both fragments off one LDS read
      if (weigh) {
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
          const float4 c = *reinterpret_cast<const float4*>(smem + AG_LW + cur * 256 + (32 * (grp >> 1) + 8 * g + 4 * (grp & 1)) * 4);
          const float cr[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            sc[0][grp][r] = fmaf(sc[0][grp][r], a.sl, cr[r]) - AG_BIAS;
            sc[1][grp][r] = fmaf(sc[1][grp][r], a.sl, cr[r]) - AG_BIAS;
          }
        }
      }
      // the words of the lane's 16 keys, where this tile needs the mask (wave-uniform): ragged, or not every pair visible
      const bool mask = t * 64 + 64 > Lk || !(t_and & w_and);
      uint32_t kw[4][4];
      if (mask) {
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
          const uint4 u = *reinterpret_cast<const uint4*>(smem + AG_KW + cur * 256 + (32 * (grp >> 1) + 8 * g + 4 * (grp & 1)) * 4);
          kw[grp][0] = u.x, kw[grp][1] = u.y, kw[grp][2] = u.z, kw[grp][3] = u.w;
        }
      }
      uint32_t pw[2][4][2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        float mx = -INFINITY;
#pragma unroll
        for (int grp = 0; grp < 4; ++grp)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float s = weigh ? sc[f][grp][r] : sc[f][grp][r] * a.sl;
            if (mask && !(kw[grp][r] & qword[f])) s = -INFINITY;
            sc[f][grp][r] = s;
            mx = fmaxf(mx, s);
          }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run[f], mx);  // finite: m_run starts finite, so a row this tile hides from gets p = 0 and alpha = 1
        const float alpha = __builtin_amdgcn_exp2f(m_run[f] - m_new);
        m_run[f] = m_new;
        // P = 2^(s - m) rounded to bf16 once: the rounded values feed both the row sum and P V
        float psum = 0.f;
#pragma unroll
        for (int grp = 0; grp < 4; ++grp)
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const uint32_t u = pack_bf16x2(__builtin_amdgcn_exp2f(sc[f][grp][2 * r] - m_new), __builtin_amdgcn_exp2f(sc[f][grp][2 * r + 1] - m_new));
            pw[f][grp][r] = u;
            psum += __uint_as_float(u << 16) + __uint_as_float(u & 0xffff0000u);
          }
        l_part[f] = fmaf(l_part[f], alpha, psum);
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[f][dt] *= alpha;
      }
      // O^T += V^T P^T: k-step ks = positions 32 ks .. + 31, the lane's k entries are positions 32 ks + 8 g .. + 7 = groups (ks, 0), (ks, 1)
      const char* vt = smem + AG_VT + cur * AG_TILE;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_t pf[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const uint32_t pk[4] = {pw[f][2 * ks][0], pw[f][2 * ks][1], pw[f][2 * ks + 1][0], pw[f][2 * ks + 1][1]};
          __builtin_memcpy(&pf[f], pk, 16);
        }
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
          const int r = 16 * dt + n;
          const bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(vt + r * 128 + (((4 * ks + g) ^ ((r >> 1) & 7)) << 4));
          o[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[0], o[0][dt], 0, 0, 0);
          o[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[1], o[1][dt], 0, 0, 0);
        }
      }
    }
    if (tn < nt) deposit(cur ^ 1);
    t = tn, cur ^= 1;
  }

  // ---- epilogue: the row sums joined over the four g lanes, O / l as bf16, 4 channels a store
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    float l = l_part[f];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const int qi = qw + 16 * f + n;
    if (qi >= Lq) continue;
    const float inv = 1.0f / l;
    const AttnOut& out = a.out;
    bf16_t* op;
    if (out.head_major) op = out.p1 + ((int64_t)bh * Lq + qi) * 128;
    else if (qi < out.rows0) op = out.p0 + (int64_t)b * out.bstride0 + (int64_t)qi * out.ld0 + h * 128;
    else op = out.p1 + (int64_t)b * out.bstride1 + (int64_t)(qi - out.rows0) * out.ld1 + h * 128;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
      *reinterpret_cast<uint2*>(op + 16 * dt + 4 * g) =
          uint2{pack_bf16x2(o[f][dt][0] * inv, o[f][dt][1] * inv), pack_bf16x2(o[f][dt][2] * inv, o[f][dt][3] * inv)};
  }
}

// OR and AND of the key words of every 64-key tile, and whether every key of it has lw == 0 (no lw: yes): one wave a tile, the keys past Lk left out of all three
__global__ __launch_bounds__(64) void key_tile_summary_kernel(const uint32_t* __restrict kg, const float* __restrict lw, int Lk, int nt, uint32_t* __restrict ksum) {
  const int t = blockIdx.x, b = blockIdx.y, key = t * 64 + (int)threadIdx.x;
  const uint32_t w = key < Lk ? kg[(int64_t)b * Lk + key] : 0u;
  uint32_t v_or = w, v_and = key < Lk ? w : ~0u, v_flat = !lw || key >= Lk || lw[(int64_t)b * Lk + key] == 0.f;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v_or |= __shfl_xor(v_or, o, 64), v_and &= __shfl_xor(v_and, o, 64), v_flat &= __shfl_xor(v_flat, o, 64);
  if (threadIdx.x == 0) *reinterpret_cast<uint4*>(ksum + ((int64_t)b * nt + t) * 4) = uint4{v_or, v_and, v_flat, 0u};
}

// lw = log2 w as exponent + log2(mantissa), the second rounded to the 2^-14 grid: w == 1 gives 0, and w * 2^k gives lw + k, both exactly.  w finite and > 0.
__global__ __launch_bounds__(256) void key_weight_log2_kernel(const float* __restrict w, int64_t n, float* __restrict lw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int e;
  const float f = frexpf(w[i], &e);  // [0.5, 1)
  lw[i] = (float)(e - 1) + rintf(log2f(2.f * f) * AG_GRID) * (1.f / AG_GRID);
}

}  // namespace

size_t attention_groups_summary_bytes(int groups_batch, int Lk) {
  if (groups_batch <= 0 || Lk <= 0) return 0;
  return (size_t)groups_batch * cdiv(Lk, 64) * 4 * sizeof(uint32_t);
}

int launch_key_weight_log2(const float* w, int64_t n, float* lw, hipStream_t stream) {
  if (!w || !lw || n <= 0 || n > ((int64_t)1 << 38)) return fail(FMI_ERR_INVALID, "attention_groups: key weights: null pointer or bad count");
  if (((uintptr_t)w | (uintptr_t)lw) & 3) return fail(FMI_ERR_INVALID, "attention_groups: key weights must be 4-byte aligned");
  hipLaunchKernelGGL(key_weight_log2_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, stream, w, n, lw);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

int launch_key_tile_summary(const uint32_t* k_groups, const float* k_lw, int groups_batch, int Lk, uint32_t* ksum, hipStream_t stream) {
  if (!k_groups || !ksum) return fail(FMI_ERR_INVALID, "attention_groups: null group words or summaries");
  if (groups_batch <= 0 || groups_batch > 65535 || Lk <= 0) return fail(FMI_ERR_INVALID, "attention_groups: groups_batch must be 1 .. 65535 and Lk positive");
  if ((((uintptr_t)k_groups | (uintptr_t)k_lw) & 3) || ((uintptr_t)ksum & 15))
    return fail(FMI_ERR_INVALID, "attention_groups: group words and key weights must be 4-byte, summaries 16-byte aligned");
  const int nt = cdiv(Lk, 64);
  hipLaunchKernelGGL(key_tile_summary_kernel, dim3(nt, groups_batch), dim3(64), 0, stream, k_groups, k_lw, Lk, nt, ksum);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

int launch_attention_groups(const bf16_t* q, const bf16_t* k, const bf16_t* vt, const AttnOut& out, int B, int H, int Lq, int Lk, int Lkpad, float scale,
                            const uint32_t* q_groups, const uint32_t* k_groups, const uint32_t* ksum, const float* k_lw, int groups_batch, hipStream_t stream) {
  if (!q || !k || !vt || !q_groups || !k_groups || !ksum || !out.p1 || (!out.head_major && out.rows0 > 0 && !out.p0))
    return fail(FMI_ERR_INVALID, "attention_groups: null pointer");
  if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return fail(FMI_ERR_INVALID, "attention_groups: empty problem");
  if (Lkpad % 64 != 0 || Lkpad < Lk) return fail(FMI_ERR_INVALID, "attention_groups: Lkpad must be a multiple of 64 and >= Lk");
  if (groups_batch != 1 && groups_batch != B) return fail(FMI_ERR_INVALID, "attention_groups: groups_batch must be 1 or B");
  if (!std::isfinite(scale)) return fail(FMI_ERR_INVALID, "attention_groups: scale must be finite");
  // the tiles arrive by LDS-DMA and the output leaves in 8-byte stores: there is no 2-byte form of this kernel
  if (!all_aligned16({q, k, vt}) || ((uintptr_t)out.p0 | (uintptr_t)out.p1) & 7 || (!out.head_major && ((out.ld0 | out.ld1 | out.bstride0 | out.bstride1) & 3)))
    return fail(FMI_ERR_INVALID, "attention_groups: q, k and the V^T image must be 16-byte aligned, the output rows 8-byte aligned");
  if (((uintptr_t)q_groups | (uintptr_t)k_groups | (uintptr_t)k_lw) & 3 || (uintptr_t)ksum & 15)
    return fail(FMI_ERR_INVALID, "attention_groups: group words and key weights must be 4-byte, summaries 16-byte aligned");
  const int64_t blocks = (int64_t)cdiv(Lq, AG_QBLK) * B * H;
  if (blocks > 0x7fffffff) return fail(FMI_ERR_INVALID, "attention_groups: too many workgroups");
  GroupArgs a{};
  a.q = q, a.k = k, a.vt = vt, a.out = out, a.qg = q_groups, a.kg = k_groups, a.ksum = ksum, a.lw = k_lw;
  a.H = H, a.Lq = Lq, a.Lk = Lk, a.Lkpad = Lkpad, a.nt = cdiv(Lk, 64);
  a.qg_bs = groups_batch == 1 ? 0 : Lq, a.kg_bs = groups_batch == 1 ? 0 : Lk, a.ksum_bs = groups_batch == 1 ? 0 : 4 * (int64_t)a.nt;
  a.sl = scale * LOG2E;
  if (k_lw) hipLaunchKernelGGL(attention_groups_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(attention_groups_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

}  // namespace fmi
