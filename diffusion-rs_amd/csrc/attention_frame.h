// attention_frame.h — the frame the attention kernels share around their KV loops / generated streams (included by attention.hip in
// front of the kernels; same translation unit): workgroup decode, output row pointer, the one-wave kernels' LDS-DMA set-up, Q fragment
// load, base-pointer split and LDS-staged epilogue, and the 8-wave kernels' softmax tile.
// Plain inlined functions: nothing here owns LDS — a kernel's `smem` stays its only __shared__ object at LDS byte 0 (FMI_LDS_GUARD) and is
// handed in as a pointer — and the order in which a kernel calls them is the order of side effects its schedule depends on.
#pragma once

namespace fmi {

typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef int i32x32 __attribute__((ext_vector_type(32)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// ---- workgroup decode.  1-D grid, XCD-aware: block b runs on XCD b % 8, so each XCD gets a contiguous range of (head, q-block) ids — all
// q-blocks of a head then share that head's K / Vt in ONE L2 instead of pulling it into all eight.  lid = xcd_remap(blockIdx.x, gridDim.x)
// (attention_w4_kernel's key-split launch takes its part index out of it first).
struct AttnBlock {
  int bh, b, h;  // (batch, head) id and its two coordinates
  int q0;        // first query row of this wave
};
__device__ __forceinline__ AttnBlock attn_block(int lid, int H, int Lq, int wave, int rows_per_wave) {
  const int nqb = (Lq + ATT_QBLK - 1) / ATT_QBLK;
  AttnBlock blk;
  blk.bh = lid / nqb;
  blk.b = blk.bh / H, blk.h = blk.bh % H;
  blk.q0 = (lid % nqb) * ATT_QBLK + wave * rows_per_wave;
  return blk;
}

// ---- output row of query q (AttnOut, common.h): head-major, or token-major with rows [0, rows0) in p0 and the rest in p1.
// attn_out_row: the whole address as one expression, for a loop written in the kernel itself (attention_w16l_kernel).
__device__ __forceinline__ bf16_t* attn_out_row(const AttnOut& out, const AttnBlock& blk, int q, int Lq) {
  bf16_t* op;
  if (out.head_major)
    op = out.p1 + ((int64_t)blk.bh * Lq + q) * HD;
  else if (q < out.rows0)
    op = out.p0 + (int64_t)blk.b * out.bstride0 + (int64_t)q * out.ld0 + blk.h * HD;
  else
    op = out.p1 + (int64_t)blk.b * out.bstride1 + (int64_t)(q - out.rows0) * out.ld1 + blk.h * HD;
  return op;
}
// AttnOutRows: the same addresses for the shared read-back loop, with their wave-uniform part computed once; row(q) adds one product.  (With
// attn_out_row inside that loop the compiler recomputes the 64-bit products of the uniform part for every row.)
struct AttnOutRows {
  bf16_t *hm, *tm0, *tm1;  // row 0 of the head-major output / of this head's columns in p0 / the same in p1
  int head_major, rows0, ld0, ld1;
  __device__ __forceinline__ AttnOutRows(const AttnOut& out, const AttnBlock& blk, int Lq)
      : hm(out.p1 + (int64_t)blk.bh * Lq * HD),
        tm0(out.p0 + (int64_t)blk.b * out.bstride0 + blk.h * HD),
        tm1(out.p1 + (int64_t)blk.b * out.bstride1 + blk.h * HD),
        head_major(out.head_major), rows0(out.rows0), ld0(out.ld0), ld1(out.ld1) {}
  __device__ __forceinline__ bf16_t* row(int q) const {
    if (head_major) return hm + (int64_t)q * HD;
    if (q < rows0) return tm0 + (int64_t)q * ld0;
    return tm1 + (int64_t)(q - rows0) * ld1;
  }
};

// ---- a wave-uniform pointer as the two scalar halves the generated streams take
struct AttnBase {
  uint32_t lo, hi;
};
__device__ __forceinline__ AttnBase attn_split_base(const void* p) {
  const uint64_t p64 = (uint64_t)(uintptr_t)p;
  return {(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)p64), (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(p64 >> 32))};
}

// =====================================================================================================================================
// One wave per SIMD (attention_w16 / _w16l / _w32): K ring [4][64 keys] at LDS byte 0, V^T ring [4] at 64 KiB, 16-KiB slots.
// =====================================================================================================================================
constexpr int AW_TILE = 16384, AW_VT_RING = 4 * AW_TILE;

// LDS-DMA of the rings: 16 one-KiB pieces per tile and operand (8 for the e4m3 ones), split evenly over the four waves.  The destination is
// lane-linear, the swizzle sits in the per-lane source offsets (loop invariants, handed to the stream as well); a tile index past the end is
// clamped in the stream (the last tile is fetched again: identical bytes).
//   QK8: K rows are 128 B of e4m3, a piece is 8 rows (else 4 rows of 256 B).  PV8: V^T rows are Lkpad B of e4m3, a piece is 16 rows of 64 B.
//   KSwz()(row) = the kernel's K swizzle: 16-byte slot p of row r holds global slot p ^ KSwz()(r).
template <bool QK8, bool PV8, class KSwz>
struct OneWaveDma {
  static constexpr int KROW = QK8 ? 128 : 256, TILE_K = 64 * KROW;  // bytes of a K row / of a K tile (HBM and LDS)
  static constexpr int KP = QK8 ? 2 : 4, VP = PV8 ? 2 : 4;          // 1-KiB DMA pieces of a K / V^T tile per wave
  const char *Kb, *Vb;                                              // this (batch, head)'s K and V^T
  char* smem;
  int wave, ntiles;
  int k_last_rows;  // keys in the last tile (1..64): rows beyond are fetched from the last key
  uint32_t k_voff[4], k_voffc[4], v_voff[4];  // (k_voffc: the last tile's offsets, with that clamp)

  // bases and counts ...
  __device__ __forceinline__ void init_bases(const void* K, const void* Vt, char* smem_, int bh, int Lk, int Lkpad, int wave_) {
    Kb = reinterpret_cast<const char*>(K) + (int64_t)bh * Lk * KROW;
    Vb = reinterpret_cast<const char*>(Vt) + (int64_t)bh * HD * Lkpad * (PV8 ? 1 : 2);
    smem = smem_, wave = wave_;
    ntiles = (Lk + ATT_KV - 1) / ATT_KV;  // >= 2 (the launcher sends single-tile problems to the 8-wave kernel)
    k_last_rows = Lk - (ntiles - 1) * ATT_KV;
  }
  // ... and the per-lane offsets (attention_w16l_kernel fills the three arrays itself, see there)
  __device__ __forceinline__ void init(const void* K, const void* Vt, char* smem_, int bh, int Lk, int Lkpad, int wave_, int lane) {
    init_bases(K, Vt, smem_, bh, Lk, Lkpad, wave_);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (PV8) {  // slot p of row r holds global slot p ^ ((r >> 2) & 3)
        const int vr = (wave * 2 + (i & 1)) * 16 + (lane >> 2);
        v_voff[i] = (uint32_t)(vr * Lkpad + (((lane & 3) ^ ((vr >> 2) & 3)) << 4));
      } else {  // piece = 8 rows of 128 B; slot p of row r holds global slot p ^ ((r >> 1) & 7)
        const int vr = (wave * 4 + i) * 8 + (lane >> 3);
        v_voff[i] = (uint32_t)(vr * Lkpad * 2 + (((lane & 7) ^ ((vr >> 1) & 7)) << 4));
      }
      constexpr int SLOTS = KROW / 16, ROWS = 1024 / KROW;  // 16-byte slots of a K row, K rows of a piece
      const int kr = (wave * KP + (i & (KP - 1))) * ROWS + lane / SLOTS;
      const int slot = ((lane & (SLOTS - 1)) ^ KSwz()(kr)) << 4;
      k_voff[i] = (uint32_t)(kr * KROW + slot);
      k_voffc[i] = kr >= k_last_rows ? (uint32_t)((k_last_rows - 1) * KROW + slot) : k_voff[i];
    }
  }
  __device__ __forceinline__ void stage_k(int tile, int i) const {
    const char* base = Kb + (int64_t)tile * TILE_K;
    const uint32_t off = (tile == ntiles - 1) ? k_voffc[i] : k_voff[i];
    __builtin_amdgcn_global_load_lds((glb_void*)(base + off), (lds_void*)(smem + (tile & 3) * TILE_K + (wave * KP + i) * 1024), 16, 0, 0);
  }
  __device__ __forceinline__ void stage_v(int tile, int i) const {
    const char* base = Vb + (int64_t)tile * (PV8 ? ATT_KV : ATT_KV * 2);
    __builtin_amdgcn_global_load_lds((glb_void*)(base + v_voff[i]), (lds_void*)(smem + AW_VT_RING + (tile & 3) * AW_TILE + (wave * VP + i) * 1024), 16, 0, 0);
  }
  // prologue: K(0 .. NK-1), V^T(0 .. NV-1) in flight
  template <int NK, int NV>
  __device__ __forceinline__ void prologue() const {
#pragma unroll
    for (int t = 0; t < NK; ++t)
      if (t < ntiles) {
#pragma unroll
        for (int i = 0; i < KP; ++i) stage_k(t, i);
      }
#pragma unroll
    for (int t = 0; t < NV; ++t)
      if (t < ntiles) {
#pragma unroll
        for (int i = 0; i < VP; ++i) stage_v(t, i);
      }
  }
};

// everything the prologue issued has landed and is published: the last thing in front of a stream
__device__ __forceinline__ void attn_publish_prologue() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// eight bf16 of Q times scale * log2(e), rounded to bf16 once: the streams' scores then need no per-score multiply
__device__ __forceinline__ void attn_scale_round_pack(const bf16_t* qp, float scale_log2e, i32x32& dst, int at) {
  const uint4 raw = *reinterpret_cast<const uint4*>(qp);
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = __uint_as_float(w[e] << 16) * scale_log2e, hi = __uint_as_float(w[e] & 0xffff0000u) * scale_log2e;
    dst[at + e] = (int)pack_bf16x2(lo, hi);
  }
}

// Q fragments of the 16x16x32 layout (MFMA B operand, rows = d), lane (g, n), query block q = 2 b + c = 0..3 of the wave's 64 rows:
//   bf16: QA[b][(4 c + s) * 4 ..] = bf16(Q[q0 + 16 q + n][32 s + 8 g .. + 7] * scale * log2(e))
//   e4m3: QA[0][8 q ..] = the 32 bytes Q8[q0 + 16 q + n][32 g .. + 31] as they are (the scale rides in the MFMA's block scale)
template <bool QK8>
__device__ __forceinline__ void attn_load_q16(i32x32 (&QA)[2], const bf16_t* Q, int bh, int q0, int Lq, int g, int n16, float scale_log2e) {
#pragma unroll
  for (int r = 0; r < 32; ++r) QA[1][r] = 0;
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int qr = min(q0 + 32 * b + 16 * c + n16, Lq - 1);
      if constexpr (QK8) {
        const char* qp = reinterpret_cast<const char*>(Q) + ((int64_t)bh * Lq + qr) * 128 + 32 * g;
        const uint4 lo = *reinterpret_cast<const uint4*>(qp), hi = *reinterpret_cast<const uint4*>(qp + 16);
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) QA[0][(2 * b + c) * 8 + e] = (int)w[e];
      } else {
        const bf16_t* qp = Q + ((int64_t)bh * Lq + qr) * HD + 8 * g;
#pragma unroll
        for (int s = 0; s < 4; ++s) attn_scale_round_pack(qp + 32 * s, scale_log2e, QA[b], (c * 4 + s) * 4);
      }
    }
}

// ---- LDS-staged epilogue: O = O^T / l leaves as whole 256-byte rows.  Staging tile of a wave = 64 rows x 256 B in its own 16 KiB of the (drained)
// rings, 16-byte slot s of row r at s ^ (r & 15).
__device__ __forceinline__ void attn_drain_rings() {  // the streams end drained; every wave must be done with the rings before they are reused
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}
__device__ __forceinline__ void attn_stage_put(char* stg, int r, int d, float a0, float a1, float a2, float a3, float inv) {
  const uint2 v = make_uint2(pack_bf16x2(a0 * inv, a1 * inv), pack_bf16x2(a2 * inv, a3 * inv));
  *reinterpret_cast<uint2*>(stg + r * 256 + ((((d * 2) >> 4) ^ (r & 15)) << 4) + ((d * 2) & 15)) = v;
}
// Where a lane's accumulators O[0..3] (128 registers, as runs of four consecutive d) sit in the tile.  A map splits them into GROUPS query rows
// of RUNS runs each: row(grp, lane), at(grp, j) = index of run j's first register in the 128, d(j, lane) = its first head dimension.
struct AttnMap16 {  // 16x16 accumulators, lane (g, n): O^T[d = 16 dt + 4 g + i][query 16 (2 b + c) + n] in register ((8 b + dt) * 2 + c) * 4 + i
  static constexpr int GROUPS = 4, RUNS = 8;
  static __device__ __forceinline__ int row(int grp, int lane) { return 16 * grp + (lane & 15); }
  static __device__ __forceinline__ int at(int grp, int dt) { return ((8 * (grp >> 1) + dt) * 2 + (grp & 1)) * 4; }
  static __device__ __forceinline__ int d(int dt, int lane) { return 16 * dt + 4 * (lane >> 4); }
};
struct AttnMap32 {  // 32x32 accumulators (attention_w32; attention_w16l's all-e4m3 form writes the same map out itself), lane (hl, q): O^T[d = 32 dt + 8 (r >> 2) + 4 hl + (r & 3)][query 32 b + q] in register (4 b + dt) * 16 + r
  static constexpr int GROUPS = 2, RUNS = 16;
  static __device__ __forceinline__ int row(int grp, int lane) { return 32 * grp + (lane & 31); }
  static __device__ __forceinline__ int at(int grp, int j) { return 64 * grp + 4 * j; }
  static __device__ __forceinline__ int d(int j, int lane) { return 8 * j + 4 * (lane >> 5); }
};
// normalise my accumulators (inv_of(grp) = 1 / row sum of my row of the group) and write them into the staging tile
template <class Map, class InvOf>
__device__ __forceinline__ void attn_stage_rows(char* stg, const f32x32 (&O)[4], int lane, InvOf inv_of) {
#pragma unroll
  for (int grp = 0; grp < Map::GROUPS; ++grp) {
    const float inv = inv_of(grp);
    const int r = Map::row(grp, lane);
#pragma unroll
    for (int j = 0; j < Map::RUNS; ++j) {
      const int idx = Map::at(grp, j);
      const f32x32& acc = O[idx >> 5];
      const int o = idx & 31;
      attn_stage_put(stg, r, Map::d(j, lane), acc[o], acc[o + 1], acc[o + 2], acc[o + 3], inv);
    }
  }
}
// read the tile back and store it: four whole rows per wave-instruction
__device__ __forceinline__ void attn_store_staged(const char* stg, const AttnOut& out, const AttnBlock& blk, int Lq, int lane) {
  const AttnOutRows rows(out, blk, Lq);
  __syncthreads();  // (each wave reads back only its own region; the barrier also orders the LDS writes before the reads)
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int r = it * 4 + (lane >> 4), c = lane & 15;
    const int q = blk.q0 + r;
    const uint4 v = *reinterpret_cast<const uint4*>(stg + r * 256 + ((c ^ (r & 15)) << 4));
    if (q < Lq) *reinterpret_cast<uint4*>(rows.row(q) + c * 8) = v;
  }
}

// =====================================================================================================================================
// Eight waves (attention_kernel, attention_pp_kernel): a wave owns 32 query rows, lane (hl, l31) one row and half of a tile's keys.
// =====================================================================================================================================
// (Their bf16 staging and direct epilogue stay in the kernels: hipcc schedules those kernels' loops itself, and with either behind a shared function
// attention_pp_kernel measured 1.5 % slower.)
// Online softmax of tile t (exp2 domain, lane-local row): S^T -> P as four bf16x8 B operands; deferred rescale of O^T by THR_X16 / 16.
// A lane's score r of half u is key 32 u + (r & 3) + 8 (r >> 2) + 4 hl of the tile.
template <int THR_X16>
__device__ __forceinline__ void attn_softmax_tile(f32x16 (&sc)[2], f32x16 (&ot)[4], bf16x8_t (&pf)[4], float& m_run, float& l_run, int t, int Lk, int hl,
                                                  float scale_log2e) {
  if ((t + 1) * ATT_KV > Lk) {  // mask the ragged tail (kv >= Lk)
    const int kvb = t * ATT_KV + 4 * hl;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kvb + 32 * u + (r & 3) + 8 * (r >> 2) >= Lk) sc[u][r] = -1e30f;
  }
  float pmax = sc[0][0];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) pmax = fmaxf(pmax, sc[u][r]);
  pmax = fmaxf(pmax, __shfl_xor(pmax, 32, 64));
  const float ps = pmax * scale_log2e;
  if (__any(ps - m_run > (float)THR_X16 * 0.0625f)) {
    const float mn = fmaxf(m_run, ps);
    const float alpha = fast_exp2(m_run - mn);
    m_run = mn;
    l_run *= alpha;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) ot[i][r] *= alpha;
  }
  float lsum = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    uint32_t pk[8];
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const float p0 = fast_exp2(sc[u][r] * scale_log2e - m_run);
      const float p1 = fast_exp2(sc[u][r + 1] * scale_log2e - m_run);
      lsum += p0 + p1;
      pk[r >> 1] = pack_bf16x2(p0, p1);
    }
    uint4 lo = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    uint4 hi = make_uint4(pk[4], pk[5], pk[6], pk[7]);
    __builtin_memcpy(&pf[2 * u], &lo, 16);
    __builtin_memcpy(&pf[2 * u + 1], &hi, 16);
  }
  l_run += lsum;
}

}  // namespace fmi
