// attention_blocks.hip — joint attention at head dim 128 with a BLOCK-SPARSE mask given as a list of key tiles per query block, on
// v_mfma_f32_16x16x32_bf16: local windows, sliding tiles, any mask that is a property of (query block, key tile).  DESIGN.md 4.26.
//
//   O = softmax(Q K^T * scale + M) V,   M[i][j] = 0 where key tile j / 64 is in the list of query block i / 128, else -inf
//
// The mask is CSR over query blocks: row_ptr int32 (nqb + 1), cols int32 (row_ptr[nqb]), nqb = ceil(Lq / 128), tile indices in [0, ceil(Lk / 64)), strictly
// ascending inside a row, no empty row; one set for all samples and heads.  A listed tile is visible to the whole query block, an unlisted one is never
// touched: there is no per-element mask but the index test that hides the keys past Lk in the last tile.  q, k head-major (B H, L, 128) bf16 and V as
// launch_v_transpose's image (B H, 128, Lpad), output through AttnOut: the operands of attention_groups.hip, so the kernel stands in at the same two call
// sites of forward_core without a relayout.
//
// Work split and operand reuse: attention_groups.hip's, the part of it that carries over.  A workgroup of 4 waves owns the 128 queries of one query block of
// one (batch, head); a wave owns 32 of them as TWO 16-query fragments, so every K and V^T operand read from LDS feeds two MFMAs.  Q stays in registers as B
// operands (2 x 4 k-steps), S^T = K Q^T and O^T = V^T P^T: a result lane (n = lane & 15, g = lane >> 4) holds ONE query of each fragment, the row reductions
// are the lane's own values and two shuffles.  Key identity through the V^T permutation, the score groups (ks, j) and both swizzles (K chunk c of row r at
// c ^ ((r & 7) | ((r >> 4 & 1) << 3)), V^T chunk c of row r at c ^ ((r >> 1) & 7)) are that file's, to the letter.
//
// The list drives the fetch.  The workgroup copies its row of cols into LDS once, 256 entries per coalesced vector load (a row of 264 tiles, the 2048^2
// maximum, takes two; longer rows loop; AB_CAP entries bound Lk at 131072).  The first tile index alone comes by a scalar load, so the first fetch does not
// wait for the copy.  Every later index is an LDS read (all lanes one address, then readfirstlane) issued ONE TILE AHEAD of the LDS-DMA that needs it: while
// tile i is multiplied, tile i + 1 is in flight and the index of tile i + 2 is already in a scalar register.  No scalar global load sits between two tile
// fetches, there are no tile summaries and no key words in LDS.  K (64 rows x 256 B) and V^T (128 rows x 128 B) tiles are double-buffered by LDS-DMA (16 B a
// lane, 1-KiB pieces, 8 per wave and tile); one barrier per tile.  LDS: 64 KiB of tiles + 8 KiB of list, two workgroups a CU.
//
// Launch order.  Rows differ in length by up to the full ratio (a text query block lists every tile, an image block its window), so the launcher takes a third
// array, order int32 (nqb): the query blocks by descending list length, ties by ascending index (attention_blocks_order computes it on the host).  Inside each
// (batch, head) — heads keep the chunked XCD mapping of the other attention kernels, so that a head's K and V^T stay in one L2 — workgroup r takes query block
// order[r]: the long rows start first and the short ones fill in behind them.  The mapping is a pure function of blockIdx: the same bits from run to run, and
// the same bits for any order (a workgroup's arithmetic does not depend on which workgroup id runs it).
//
// Arithmetic: a visited tile is processed exactly as attention_groups.hip's unmasked path processes it — s * (scale log2e), a running maximum from -1e30,
// p = 2^(s - m) rounded to bf16 once with the rounded values feeding both the row sum and P V, tiles in ascending order.  For any list that a group-word
// assignment can express the output is fmi_sdpa_groups_bf16's bit for bit (tests/test_gpu_attention_blocks.py).
//
// List contents are device data and are taken as they are; indices are clamped into the problem (tile into [0, nt), block into [0, nqb), the row into cols and
// into AB_CAP) so that a wrong list computes a wrong answer and does not read outside the operands.  Vector loads and stores only; no workspace beyond the V^T
// image; asynchronous.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "common.h"

namespace fmi {
namespace {

constexpr int AB_QBLK = 128;          // queries per workgroup = one query block of the list
constexpr int AB_TILE = 16384;        // bytes of a K tile and of a V^T tile
constexpr int AB_VT = 2 * AB_TILE;    // V^T tiles [2] behind the K tiles [2]
constexpr int AB_LIST = 4 * AB_TILE;  // the workgroup's row of cols behind them
constexpr int AB_CAP = 2048;          // entries of that row: every tile of Lk = 131072
constexpr float LOG2E = 1.44269504088896340736f;

struct BlockArgs {
  const bf16_t *q, *k, *vt;
  AttnOut out;
  const int *row_ptr, *cols, *order;
  int H, Lq, Lk, Lkpad, nt, nqb, ncols;
  float sl;  // scale * log2(e)
};

__device__ __forceinline__ int vt_perm16(int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); }

__global__ __launch_bounds__(256, 2) void attention_blocks_kernel(const BlockArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[AB_LIST + AB_CAP * 4];
  const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nqb = a.nqb, id = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = id / nqb, qb = min(max(a.order[id % nqb], 0), nqb - 1);
  const int q0 = qb * AB_QBLK, b = bh / a.H, h = bh % a.H, qw = q0 + wave * 32;
  const int Lq = a.Lq, Lk = a.Lk, nt = a.nt;
  const bf16_t* Kb = a.k + (int64_t)bh * Lk * 128;
  const bf16_t* Vb = a.vt + (int64_t)bh * 128 * a.Lkpad;
  const bool live = qw < Lq;  // a wave without a query still stages its share of every tile

  // ---- the workgroup's row of the list (uniform: scalar loads, once)
  const int beg = min(max(a.row_ptr[qb], 0), a.ncols), cnt = min(min(max(a.row_ptr[qb + 1], beg), a.ncols) - beg, AB_CAP);
  const int* row = a.cols + beg;
  int* lst = reinterpret_cast<int*>(smem + AB_LIST);
  auto clamp_tile = [&](int t) { return min(max(t, 0), nt - 1); };

  // ---- staging.  K piece p = 4 wave + i is rows 4 p .. 4 p + 3 (lane >> 4), LDS chunk lane & 15; V^T piece p is rows 8 p .. 8 p + 7 (lane >> 3), chunk lane & 7
  auto request = [&](int t, int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = wave * 4 + i, kr = p * 4 + (lane >> 4), vr = p * 8 + (lane >> 3);
      const bf16_t* ks = Kb + (int64_t)min(t * 64 + kr, Lk - 1) * 128 + (((lane & 15) ^ ((kr & 7) | (((kr >> 4) & 1) << 3))) << 3);
      __builtin_amdgcn_global_load_lds((glb_void*)ks, (lds_void*)(smem + buf * AB_TILE + p * 1024), 16, 0, 0);
      const bf16_t* vs = Vb + (int64_t)vr * a.Lkpad + t * 64 + (((lane & 7) ^ ((vr >> 1) & 7)) << 3);
      __builtin_amdgcn_global_load_lds((glb_void*)vs, (lds_void*)(smem + AB_VT + buf * AB_TILE + p * 1024), 16, 0, 0);
    }
  };
  int t = 0, tn = 0;  // the tile being multiplied and the one behind it
  if (cnt > 0) {
    t = clamp_tile(__builtin_amdgcn_readfirstlane(row[0]));
    request(t, 0);
  }
  for (int i = tid; i < cnt; i += 256) lst[i] = row[i];  // visible behind the first tile's barrier

  // ---- Q fragments (B operands).  Rows past Lq read row Lq - 1 and are not stored.
  bf16x8_t qf[2][4];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int r = min(qw + 16 * f + n, Lq - 1);
    const bf16_t* qp = a.q + ((int64_t)bh * Lq + r) * 128 + 8 * g;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[f][s] = *reinterpret_cast<const bf16x8_t*>(qp + 32 * s);
  }

  f32x4 o[2][8];  // O^T: fragment f, query n, channels 16 dt + 4 g + {0..3}
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[f][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[2] = {-1e30f, -1e30f}, l_part[2] = {0.f, 0.f};

  int cur = 0;
  for (int i = 0; i < cnt; ++i) {
    dma_barrier();  // tile i has landed for every wave, every wave is done with the other buffers, and (i == 0) the list is in LDS
    if (i == 0 && cnt > 1) tn = clamp_tile(__builtin_amdgcn_readfirstlane(lst[1]));
    if (i + 1 < cnt) request(tn, cur ^ 1);
    // the index of tile i + 2: read now, needed by the request of the next iteration
    const int tnn = i + 2 < cnt ? clamp_tile(__builtin_amdgcn_readfirstlane(lst[i + 2])) : 0;
    if (live) {
      // S^T = K Q^T: group (ks, j) of attention_groups.hip's header, both fragments off one operand read
      const char* kt = smem + cur * AB_TILE;
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
      // the one mask there is: the keys past Lk of a ragged last tile, by index.  Result register r of group grp is the key at position
      // 32 (grp >> 1) + 8 g + 4 (grp & 1) + r of the tile, and position p holds key vt_perm16(p).
      const bool ragged = t * 64 + 64 > Lk;
      uint32_t pw[2][4][2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        float mx = -INFINITY;
#pragma unroll
        for (int grp = 0; grp < 4; ++grp)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float s = sc[f][grp][r] * a.sl;
            if (ragged && t * 64 + vt_perm16(32 * (grp >> 1) + 8 * g + 4 * (grp & 1) + r) >= Lk) s = -INFINITY;
            sc[f][grp][r] = s;
            mx = fmaxf(mx, s);
          }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run[f], mx);
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
      const char* vt = smem + AB_VT + cur * AB_TILE;
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
    t = tn, tn = tnn, cur ^= 1;
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

}  // namespace

int attention_blocks_check_lists(const int* row_ptr, const int* cols, int n_query_blocks, int n_tiles, const std::string& who) {
  if (!row_ptr || !cols || n_query_blocks < 1 || n_tiles < 1) return fail(FMI_ERR_INVALID, who + "row_ptr (n_query_blocks + 1) and cols with n_query_blocks >= 1");
  if (row_ptr[0] != 0) return fail(FMI_ERR_INVALID, who + "row_ptr[0] must be 0");
  for (int r = 0; r < n_query_blocks; ++r) {
    const int lo = row_ptr[r], hi = row_ptr[r + 1];
    if (hi <= lo) return fail(FMI_ERR_INVALID, who + "query block " + std::to_string(r) + " lists no key tile (every row needs one, and row_ptr must ascend)");
    if (hi - lo > n_tiles) return fail(FMI_ERR_INVALID, who + "query block " + std::to_string(r) + " lists " + std::to_string(hi - lo) + " tiles of " + std::to_string(n_tiles));
    for (int i = lo; i < hi; ++i) {
      if (cols[i] < 0 || cols[i] >= n_tiles)
        return fail(FMI_ERR_INVALID, who + "query block " + std::to_string(r) + " lists key tile " + std::to_string(cols[i]) + " outside [0, " + std::to_string(n_tiles) + ")");
      if (i > lo && cols[i] <= cols[i - 1])
        return fail(FMI_ERR_INVALID, who + "the key tiles of query block " + std::to_string(r) + " are not strictly ascending (" + std::to_string(cols[i - 1]) + " then " +
                                         std::to_string(cols[i]) + ")");
    }
  }
  return FMI_OK;
}

std::vector<int> attention_blocks_order(const int* row_ptr, int n_query_blocks) {
  std::vector<int> order(std::max(n_query_blocks, 0));
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return row_ptr[x + 1] - row_ptr[x] > row_ptr[y + 1] - row_ptr[y]; });
  return order;
}

int launch_attention_blocks(const bf16_t* q, const bf16_t* k, const bf16_t* vt, const AttnOut& out, int B, int H, int Lq, int Lk, int Lkpad, float scale,
                            const int* row_ptr, const int* cols, const int* order, int n_query_blocks, int n_cols, hipStream_t stream) {
  if (!q || !k || !vt || !row_ptr || !cols || !order || !out.p1 || (!out.head_major && out.rows0 > 0 && !out.p0))
    return fail(FMI_ERR_INVALID, "attention_blocks: null pointer");
  if (B <= 0 || H <= 0 || Lq <= 0 || Lk <= 0) return fail(FMI_ERR_INVALID, "attention_blocks: empty problem");
  if (Lkpad % 64 != 0 || Lkpad < Lk) return fail(FMI_ERR_INVALID, "attention_blocks: Lkpad must be a multiple of 64 and >= Lk");
  const int nt = cdiv(Lk, 64);
  if (n_query_blocks != cdiv(Lq, AB_QBLK))
    return fail(FMI_ERR_INVALID, "attention_blocks: the lists are for " + std::to_string(n_query_blocks) + " query blocks, Lq = " + std::to_string(Lq) + " has " +
                                     std::to_string(cdiv(Lq, AB_QBLK)));
  if (nt > AB_CAP) return fail(FMI_ERR_UNSUPPORTED, "attention_blocks: Lk above " + std::to_string(AB_CAP * 64) + " keys");
  if (n_cols < n_query_blocks || (int64_t)n_cols > (int64_t)n_query_blocks * nt)
    return fail(FMI_ERR_INVALID, "attention_blocks: n_cols must be n_query_blocks .. n_query_blocks * ceil(Lk / 64) (no empty row, no tile twice)");
  if (!std::isfinite(scale)) return fail(FMI_ERR_INVALID, "attention_blocks: scale must be finite");
  // the tiles arrive by LDS-DMA and the output leaves in 8-byte stores: there is no 2-byte form of this kernel
  if (!all_aligned16({q, k, vt}) || ((uintptr_t)out.p0 | (uintptr_t)out.p1) & 7 || (!out.head_major && ((out.ld0 | out.ld1 | out.bstride0 | out.bstride1) & 3)))
    return fail(FMI_ERR_INVALID, "attention_blocks: q, k and the V^T image must be 16-byte aligned, the output rows 8-byte aligned");
  if (((uintptr_t)row_ptr | (uintptr_t)cols | (uintptr_t)order) & 3) return fail(FMI_ERR_INVALID, "attention_blocks: row_ptr, cols and order must be 4-byte aligned");
  const int64_t blocks = (int64_t)n_query_blocks * B * H;
  if (blocks > 0x7fffffff) return fail(FMI_ERR_INVALID, "attention_blocks: too many workgroups");
  BlockArgs a{};
  a.q = q, a.k = k, a.vt = vt, a.out = out, a.row_ptr = row_ptr, a.cols = cols, a.order = order;
  a.H = H, a.Lq = Lq, a.Lk = Lk, a.Lkpad = Lkpad, a.nt = nt, a.nqb = n_query_blocks, a.ncols = n_cols;
  a.sl = scale * LOG2E;
  hipLaunchKernelGGL(attention_blocks_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

}  // namespace fmi
