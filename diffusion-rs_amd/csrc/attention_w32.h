// attention_w32.h — joint attention on v_mfma_f32_32x32x16_bf16, one wave per SIMD (included by attention.hip; same
// translation unit).  Round 3's kernel, the sibling of attention_w16.h (read that header and tools/gen_attention_w32.py first:
// Q pre-multiplied by scale * log2(e) and -m accumulated by the first d-step of the score product, exp2 in place, no cross-lane
// traffic on the common softmax path, row sums from a ones-row MFMA, the whole KV stream one generated asm statement) on the
// 32 x 32 shape: a 32-clock MFMA hides ~19 clocks of the softmax's instructions, a 16-clock one ~8 (tools/gen_issue_model.py),
// and half as many MFMAs and waits are issued — with one wave per SIMD the kernel is bound by what sits between the MFMAs.
//
// Replaces scaled_dot_product_attention (diffusion_rs_core/src/models/flux/model.rs:40-50) -> backend::ops::sdpa
// (diffusion_rs_backend/src/ops.rs:247-262: softmax((q k^T) * scale) v, f32, scores materialised).
//
// Layouts are attention_w4_kernel's (block b = 32 queries, a lane owns one query and 32 of a tile's 64 keys; K ring slot c of
// row r at c ^ (r & 15); V^T with the k-permutation of attention.hip: vt_perm).  Not bit-identical to the 8-wave kernels: the
// scores differ by the rounding of q * scale * log2(e) to bf16 and the row sum is that of the rounded p.
#pragma once
#ifndef FMI_AW32_LOOP_INC  // (tools/run_attn_w16_ablations.sh points this at a timing-experiment variant of the generated stream)
#define FMI_AW32_LOOP_INC "attention_w32_loop.inc"
#endif
#include FMI_AW32_LOOP_INC

namespace fmi {

constexpr int AW32_THREADS = 256;

struct Aw32KSwz {  // attention_w4_kernel's K image: 16-byte slot c of row r at c ^ (r & 15)
  __device__ __forceinline__ int operator()(int r) const { return r & 15; }
};

template <int THR_X16>
__global__ __launch_bounds__(AW32_THREADS, 1) void attention_w32_kernel(const bf16_t* __restrict Q, const bf16_t* __restrict K, const bf16_t* __restrict Vt,
                                                                        AttnOut out, int H, int Lq, int Lk, int Lkpad, float scale_log2e) {
  constexpr int TILE = AW_TILE, VT_RING = AW_VT_RING;
  __shared__ __attribute__((aligned(16))) char smem[8 * TILE];  // K ring [4][64 x 128] at 0, V^T ring [4][128 x 64] at 64 KiB
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const AttnBlock blk = attn_block(xcd_remap(blockIdx.x, gridDim.x), H, Lq, wave, 64);
  const int hl = lane >> 5, l31 = lane & 31;

  // ---- Q fragments (MFMA B operand): QF[b][s] = bf16(Q[q0 + 32 b + l31][16 s + 8 hl .. + 7] * scale * log2(e))
  i32x32 QA[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int qr = min(blk.q0 + 32 * b + l31, Lq - 1);
    const bf16_t* qp = Q + ((int64_t)blk.bh * Lq + qr) * HD + 8 * hl;
#pragma unroll
    for (int s = 0; s < 8; ++s) attn_scale_round_pack(qp + 16 * s, scale_log2e, QA[b], s * 4);
  }

  i32x16 R0, R1;
  i32x32 NMR;
  OneWaveDma<false, false, Aw32KSwz> dma;  // (attention_frame.h: the rings' LDS-DMA offsets and pieces)
  dma.init(K, Vt, smem, blk.bh, Lk, Lkpad, wave, lane);
  // (smem sits at LDS byte 0 — the ring-slot xor rely on it: it is the kernel's only __shared__ object, which the host checks before the first launch, FMI_LDS_GUARD)
  // Fragment read addresses: K fragment (key half u, d-step s) at KAD[s] + 8192 u, V^T fragment (d block dt, k-step c) at VAD[c] + 4096 dt
  {
#pragma unroll
    for (int s = 0; s < 8; ++s) R0[s] = (l31 * 256 + ((hl ^ (lane & 15)) << 4)) ^ (s << 5);
#pragma unroll
    for (int c = 0; c < 4; ++c) R0[8 + c] = VT_RING + ((l31 * 128 + ((hl ^ ((l31 >> 1) & 7)) << 4)) ^ (c << 5));
#pragma unroll
    for (int i = 0; i < 4; ++i) R0[12 + i] = (int)dma.k_voff[i], R1[i] = (int)dma.v_voff[i], R1[4 + i] = (int)dma.k_voffc[i];
    R1[8] = 4 * hl;  // LKEY: the lane's part of a score's key index
    R1[9] = 0;
    R1[10] = R1[11] = __float_as_int(-1e30f);  // M
#pragma unroll
    for (int i = 0; i < 4; ++i) R1[12 + i] = l31 == 0 ? 0x3f803f80 : 0;  // the ones fragment: row 0 = bf16 1.0
#pragma unroll
    for (int i = 0; i < 32; ++i) NMR[i] = 0;  // NM = 0: the first tile's fold is m = 0 (it always takes the rescale block)
  }

  // ---- prologue: K(0..2), V^T(0..1) in flight; everything landed and published before the first read
  dma.template prologue<3, 2>();
  attn_publish_prologue();

  // ---- the KV stream: one generated asm statement (tools/gen_attention_w32.py), every array pinned to the registers its text names
  f32x32 O[4], OL;
  i32x32 SP0, SP1, FP;  // S^T (v[0:63]), P (v[64:95]) and the fragment buffers (v[96:127]): written before read inside the statement
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    O[0][r] = O[1][r] = O[2][r] = O[3][r] = OL[r] = 0.f;
    SP0[r] = SP1[r] = 0;
    FP[r] = 0;
  }
  i32x32 FB = FP;
  {
    const AttnBase kb = attn_split_base(dma.Kb), vb = attn_split_base(dma.Vb);
    const float thr = (float)THR_X16 * 0.0625f;
    asm volatile(FMI_AW32_LOOP_ASM
                 : "+{a[0:31]}"(O[0]), "+{a[32:63]}"(O[1]), "+{a[64:95]}"(O[2]), "+{a[96:127]}"(O[3]), "+{a[192:223]}"(OL), "+{v[0:31]}"(SP0), "+{v[32:63]}"(SP1),
                   "+{v[64:95]}"(FP), "+{v[96:127]}"(FB), "+{v[128:143]}"(R0), "+{v[144:159]}"(R1), "+{v[160:191]}"(NMR)
                 : "{a[128:159]}"(QA[0]), "{a[160:191]}"(QA[1]), [kb_lo] "s"(kb.lo), [kb_hi] "s"(kb.hi), [vb_lo] "s"(vb.lo), [vb_hi] "s"(vb.hi),
                   [ntm1] "s"(dma.ntiles - 1), [thr] "s"(thr), [woff] "s"(wave * 4096), [rag] "s"(dma.k_last_rows)
                 : "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209",
                   "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219", "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87",
                   "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "vcc", "scc", "memory");
  }

  // ---- epilogue.  Lane (hl, q) holds O^T in the 32 x 32 layout (AttnMap32); the row sum of query 32 b + q is register 16 b of OL in lane q
  // (row 0 of the ones product); the statement ends drained.
  attn_drain_rings();
  char* stg = smem + wave * TILE;
  attn_stage_rows<AttnMap32>(stg, O, lane, [&](int b) { return 1.0f / __shfl(OL[16 * b], l31, 64); });
  attn_store_staged(stg, out, blk, Lq, lane);
}

}  // namespace fmi
