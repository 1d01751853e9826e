// gemm_frame.h — the frame the GEMM kernels share in front of their K loops (included by gemm_bf16.hip behind its tile constants and GemmBatch;
// same translation unit): which problem and tile a workgroup computes, the LDS-DMA source offsets of an operand tile, the swizzled fragment
// offsets of a lane, accumulator zeroing.  (slot_barrier() and the bf16x8_t / lds_void / glb_void typedefs, which the attention kernels use
// as well, are in common.h.)
// Plain inlined functions: nothing here owns LDS or issues a load — the LDS-DMA itself (builtin in gemm_pp_kernel and gemm_w4q_kernel,
// inline asm in gemm_w4_kernel) and the K loops stay in the kernels.
//
// Every extraction was made on its own and kept only where it left the kernel's registers, scratch, inline-asm regions and K loop where they
// were (profiles/gemm_frame_ab.txt).  Left out, for the product kernels they moved (these keep the text in their bodies):
//   TileDma in gemm_pp_kernel: behind the struct (or any inlined function that fills the eight offsets) its bf16 form <0, .> came out with 40
//     instead of 48 bytes of scratch (9 instead of 11 spilled registers; the e4m3 / int8 forms did not move);
//   TileDma in gemm_w4q_kernel: every resource figure held, but in the K loop (443 instructions, 64 MFMAs) 46 instructions sat elsewhere — a
//     packed-W global_load_dwordx4, the absmax load, the v_xor + ds_write_b128 of the expansion, 20 - 40 slots away — and the AGPR assignment changed;
//   zero() on the bf16 accumulators of gemm_pp_kernel: <0, 1..3> got another accumulator assignment, their K loop 161 instead of 163 instructions.
//   the body of gemm_pp_kernel as a function over the LDS array's address (for its two tile heights): every instantiation moved, the 8-bit forms included
//     (<0, .> scratch 48 -> 0 B, <1, .> 44 -> 24, <2, 1> 524 -> 588, <2, 3> 420 -> 356) — it is included text, gemm_pp_body.inc, inside the kernel that owns the array.
// So TileDma serves gemm_w4_kernel (test build) only.  With these three left out every K loop of both builds is the parent's, instruction for instruction.
#pragma once

namespace fmi {

// Logical tile t of a problem -> (tm, tn).  Tiles are numbered band by band (gh tile-rows each), column by column inside a band, so
// the ~32 consecutive tiles an XCD runs at any time form a compact gh x (32 / gh) patch: gh + 32 / gh distinct A / W panels per K
// step instead of 33 (L2 hits).  Bijective for any gh >= 1.
__device__ __forceinline__ void tile_coords(int t, int tiles_m, int tiles_n, int gh, int& tm, int& tn) {
  const int band = t / (gh * tiles_n);
  const int band_h = min(gh, tiles_m - band * gh);
  const int tin = t - band * gh * tiles_n;
  tn = tin / band_h;
  tm = band * gh + tin % band_h;
}

// ---- which problem / tile: 1-D grid over the tiles of all problems of the group, XCD-aware (xcd_remap), band / patch order inside a problem.
struct GemmTile {
  const GemmProblem& P;
  int pi, m0, n0, nk;  // index of the problem in the batch; first row / column of the BM x BN tile; number of 128-byte K tiles
  int rows;            // tile height: BM, or BM_SHORT in the short region of a mixed launch (gemm_tile_rows)
};
// es = operand element size in bytes (2: bf16, 1: e4m3 / int8)
template <int BN>
__device__ __forceinline__ GemmTile gemm_tile(const GemmBatch& batch, int es) {
  const int total = batch.tile_start[batch.nprob];
  const int lid = xcd_remap(blockIdx.x, total);
  int pi = 0;
#pragma unroll
  for (int i = 1; i < MAX_PROBLEMS; ++i)
    if (i < batch.nprob && lid >= batch.tile_start[i]) pi = i;
  const GemmProblem& P = batch.p[pi];
  const int t = lid - batch.tile_start[pi];
  const int tiles_m = (P.M + BM - 1) / BM;
  const int tiles_n = (P.N + BN - 1) / BN;
  int tm, tn;
  tile_coords(t, tiles_m, tiles_n, batch.band[pi], tm, tn);
  return {P, pi, tm * BM, tn * BN, P.K * es / (BK * 2), BM};
}
// The same for a launch of mixed heights (GemmBatch::n256): workgroups [0, ntall) are the 256-row tiles of all problems, the rest the 192-row
// tiles.  Each height region has its own bijective XCD remap (one over the whole grid would hand whole XCDs nothing but short tiles) and,
// per problem, its own band / patch order.  The height is uniform per workgroup.  The short region's remap runs on bid - ntall while the hardware
// places workgroup bid on XCD bid % 8: when ntall is no multiple of 8 the remap's XCD numbers are a rotation of the real ones — still a bijection, still
// one contiguous run of tiles per XCD, so results and locality hold (at the headline cuts ntall is 576 and 504, multiples of 8).
template <int BN>
__device__ __forceinline__ GemmTile gemm_tile_rows(const GemmBatch& batch, int es) {
  const int ntall = batch.tile_start[batch.nprob], total = batch.short_start[batch.nprob];
  const int bid = blockIdx.x;
  const bool tall = bid < ntall;
  const int lid = tall ? xcd_remap(bid, ntall) : ntall + xcd_remap(bid - ntall, total - ntall);
  const int* start = tall ? batch.tile_start : batch.short_start;
  int pi = 0;
#pragma unroll
  for (int i = 1; i < MAX_PROBLEMS; ++i)
    if (i < batch.nprob && lid >= start[i]) pi = i;
  const GemmProblem& P = batch.p[pi];
  const int t = lid - start[pi];
  const int rows_tall = batch.n256[pi] * BM;
  const int tiles_m = tall ? batch.n256[pi] : (P.M - rows_tall + BM_SHORT - 1) / BM_SHORT;
  const int tiles_n = (P.N + BN - 1) / BN;
  int tm, tn;
  tile_coords(t, tiles_m, tiles_n, tall ? batch.band[pi] : batch.band_s[pi], tm, tn);
  return {P, pi, tall ? tm * BM : rows_tall + tm * BM_SHORT, tn * BN, P.K * es / (BK * 2), tall ? BM : BM_SHORT};
}

// ---- LDS-DMA sources of the A and W tiles: this wave stages the 1-KiB chunks (8 rows of 128 B) a_chunk0 / w_chunk0 .. + PIECES - 1 of them, lane l
// the 16-byte slot (l & 7) ^ ((row >> 1) & 7) of row chunk * 8 + (l >> 3) (the LDS image is lane-linear: the swizzle sits in the source address).
// Per-lane BYTE offsets (32-bit) from the uniform tile base, so that the DMA uses the saddr + voffset form: one VGPR per piece instead
// of two for a pointer (gemm_pp_kernel sits at the 256-register limit and a spilled pointer costs a vmcnt(0) reload — a full pipeline drain).
// The offsets are relative to the tile's first row and the bases carry m0 / n0 in 64 bits: an operand may exceed 4 GiB — the fused modulation
// matrix of FLUX.1 is 6.5 GB — but a tile's 256 rows never do.  Rows past the operand's last are clamped to it (their results are never stored).
template <int PIECES>
struct TileDma {
  uint32_t a_off[PIECES], w_off[PIECES];
  const char *a_base, *w_base;  // row m0 / n0, k = 0; K tile kt is 128 kt bytes further
  // es = operand element size in bytes
  __device__ __forceinline__ TileDma(const GemmProblem& P, int m0, int n0, int es, int a_chunk0, int w_chunk0, int lane) {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int ra = (a_chunk0 + i) * 8 + (lane >> 3), rw = (w_chunk0 + i) * 8 + (lane >> 3);
      a_off[i] = (uint32_t)((int64_t)(min(m0 + ra, P.M - 1) - m0) * P.lda * es + (((lane & 7) ^ ((ra >> 1) & 7)) << 4));
      w_off[i] = (uint32_t)((int64_t)(min(n0 + rw, P.N - 1) - n0) * P.ldw * es + (((lane & 7) ^ ((rw >> 1) & 7)) << 4));
    }
    a_base = reinterpret_cast<const char*>(P.A) + (int64_t)m0 * P.lda * es;
    w_base = reinterpret_cast<const char*>(P.W) + (int64_t)n0 * P.ldw * es;
  }
};

// ---- where a lane's MFMA fragments sit in a tile's LDS image (128-byte rows, 16-byte slot c of row r at c ^ ((r >> 1) & 7)).  A fragment
// block is ROWS rows: 16 (v_mfma_f32_16x16x32_bf16: k-step s = slot 4 s + (lane >> 4), two steps per tile) or 32 (32x32x16_bf16 and the
// 8-bit 32x32x64 / 32x32x32 forms: slot 2 s + (lane >> 5), four 16-byte steps per tile).
template <int ROWS>
struct FragSlots {
  static constexpr int GROUPS = 64 / ROWS, STEPS = 8 / GROUPS;
  int rl;           // the lane's row inside a block
  int koff[STEPS];  // byte offset of k-step s inside the row
  __device__ __forceinline__ int row_off(int block_row0) const { return (block_row0 + rl) * 128; }
};
template <int ROWS>
__device__ __forceinline__ FragSlots<ROWS> frag_slots(int lane) {
  FragSlots<ROWS> f;
  f.rl = lane & (ROWS - 1);
  const int sw = (f.rl >> 1) & 7;
#pragma unroll
  for (int s = 0; s < f.STEPS; ++s) f.koff[s] = ((s * f.GROUPS + lane / ROWS) ^ sw) << 4;
  return f;
}

// ---- accumulators: an I x J array of MFMA result vectors (f32x4, f32x16, i32x16)
template <class V, int I, int J>
__device__ __forceinline__ void zero(V (&acc)[I][J]) {
#pragma unroll
  for (int i = 0; i < I; ++i)
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int r = 0; r < (int)(sizeof(V) / 4); ++r) acc[i][j][r] = 0;
}

}  // namespace fmi
