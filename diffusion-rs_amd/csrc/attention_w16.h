// attention_w16.h — joint attention on v_mfma_f32_16x16x32_bf16, one wave per SIMD (included by attention.hip; same
// translation unit).  Round 3's kernel; replaces attention_w4_kernel as the default bf16 path.
//
// Replaces scaled_dot_product_attention (diffusion_rs_core/src/models/flux/model.rs:40-50) -> backend::ops::sdpa
// (diffusion_rs_backend/src/ops.rs:247-262: softmax((q k^T) * scale) v, f32, scores materialised).
//
// The machine mapping is attention_w4_kernel's (4 waves, one per SIMD, 64 query rows per wave as two blocks that run half a KV
// tile apart; K / V^T tiles by LDS-DMA into 4-deep rings, one barrier per tile; transposed products S^T = K Q^T,
// O^T = V^T P^T with P fed from the S registers through the k-permutation baked into V^T); what changed, and why, is written
// up in tools/gen_attention_w16.py, which generates the WHOLE KV stream (first tile to last) as one asm statement:
//   * both products on the 16x16x32 MFMA (a lane owns 4 keys x 1 query of a 16 x 16 score tile);
//   * Q pre-multiplied by scale * log2(e) (rounded to bf16 once, here, when the fragments are loaded) and -m accumulated by
//     the first d-step of the score product, so p = exp2(s') with no per-score fma;
//   * no cross-lane traffic on the common softmax path; row sums from the bf16-rounded probabilities (v_dot2c_f32_bf16).
// This file is the frame around that statement: Q fragments, the K ring's DMA offsets (this kernel's own swizzle: slot p of row
// r holds global slot p ^ f(r), f(r) = (r & 7) | ((r >> 4) & 1) << 3), the first DMA pieces, and the epilogue (row sums
// reduced over the four lane groups, O = O^T / l staged through LDS into whole 256-byte rows).
//
// Numerics vs the 8-wave kernels: same f32 accumulation inside a product; the scores differ by the rounding of q * scale *
// log2(e) to bf16 (relative 2^-9 per element of q) and the row sum by the rounding of p — both far inside the stated
// tolerance against the f32 oracle (tests/test_gpu_ops.py: rel-L2 <= 6e-3), not bit-identical to attention_pp_kernel.
#pragma once
#ifndef FMI_AW16_LOOP_INC  // (tools/run_attn_w16_ablations.sh points this at a timing-experiment variant of the generated stream)
#define FMI_AW16_LOOP_INC "attention_w16_loop.inc"
#endif
#include FMI_AW16_LOOP_INC
#ifndef FMI_AW16F8_LOOP_INC  // the fp8-QK^T stream (AW16_MODE=fp8qk of the same generator)
#define FMI_AW16F8_LOOP_INC "attention_w16f8_loop.inc"
#endif
#include FMI_AW16F8_LOOP_INC

namespace fmi {

constexpr int AW16_THREADS = 256;

// this kernel's K swizzle: 16-byte slot p of row r holds global slot p ^ f(r); f8(r) for rows of 128 e4m3 bytes (8 slots)
template <bool QK8>
struct Aw16KSwz {
  __device__ __forceinline__ int operator()(int r) const { return QK8 ? ((r & 7) >> 1) | (((r >> 4) & 1) << 2) : (r & 7) | (((r >> 4) & 1) << 3); }
};

// QK8 = true (the model's fp8 mode): Q and K point to OCP e4m3 bytes, rows of 128 B, with their static scales folded
// into scale_log2e, which the launcher guarantees to be an exact power of two 2^-n (the host picks the q scale accordingly): the
// score product is one v_mfma_scale_f32_16x16x128_f8f6f4 per 16 x 16 tile whose E8M0 block scale carries 2^-n.  P, V^T and the
// second product are the bf16 ones.
template <int THR_X16, bool QK8 = false>
__global__ __launch_bounds__(AW16_THREADS, 1) void attention_w16_kernel(const bf16_t* __restrict Q, const bf16_t* __restrict K, const bf16_t* __restrict Vt,
                                                                        AttnOut out, int H, int Lq, int Lk, int Lkpad, float scale_log2e) {
  constexpr int TILE = AW_TILE, VT_RING = AW_VT_RING;
  __shared__ __attribute__((aligned(16))) char smem[8 * TILE];  // K ring [4][64 x 128] at 0, V^T ring [4][128 x 64] at 64 KiB
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const AttnBlock blk = attn_block(xcd_remap(blockIdx.x, gridDim.x), H, Lq, wave, 64);
  const int g = lane >> 4, n16 = lane & 15;

  typedef __attribute__((ext_vector_type(4))) int frag_t;
  typedef int i32x8 __attribute__((ext_vector_type(8)));

  i32x16 R0, R1;
  i32x8 R2;
  frag_t R3;  // the ones fragment: A operand whose row 0 is bf16 1.0 (V^T extended by a row of ones -> the row sums)
  OneWaveDma<QK8, false, Aw16KSwz<QK8>> dma;  // (attention_frame.h: the rings' LDS-DMA offsets and pieces)
  dma.init(K, Vt, smem, blk.bh, Lk, Lkpad, wave, lane);
  // (smem sits at LDS byte 0 — the ring-slot xor rely on it: it is the kernel's only __shared__ object, which the host checks before the first launch, FMI_LDS_GUARD)
  // Fragment read addresses.  K fragment (key block a, d-step s): lane (g, m) reads row 32 (a >> 1) + 8 (a & 1) + (m & 7) + 16 (m >> 3)
  // — the key whose score the V^T k-permutation expects in row m of block a — global slot 4 s + g, at KAD[s] + the block's
  // immediate offset.  V^T fragment (d block dt, k-step kk): row 16 dt + m, slot 4 kk + g, at VAD[kk] + 2048 dt.
  {
    const int m = n16, krow = (m & 7) + 16 * (m >> 3);
    if constexpr (QK8) {  // fp8 K fragment (key block a): the row's bytes 32 g .. + 31 = global slots 2 g, 2 g + 1; f8(row) = ((m & 7) >> 1) | (m >> 3) << 2
      const int f8 = ((m & 7) >> 1) | ((m >> 3) << 2);
      R0[0] = krow * 128 + (((2 * g) ^ f8) << 4);
      R0[1] = R0[0] ^ 16;
      R0[2] = R0[3] = 0;
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) R0[s] = krow * 256 + (((4 * s + g) ^ m) << 4);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) R0[4 + kk] = VT_RING + m * 128 + (((4 * kk + g) ^ ((m >> 1) & 7)) << 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) R0[6 + i] = (int)dma.k_voff[i], R0[10 + i] = (int)dma.v_voff[i];
    R0[14] = (int)dma.k_voffc[0], R0[15] = (int)dma.k_voffc[1];
    R1[0] = (int)dma.k_voffc[2], R1[1] = (int)dma.k_voffc[3];
    R1[2] = 16 * (g >> 1) + 4 * (g & 1);  // LKEY: the lane's part of a score's key index
    R1[3] = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) R1[4 + i] = 0;  // NM = 0: the first tile's fold is m = 0 (it always takes the rescale block)
#pragma unroll
    for (int i = 0; i < 4; ++i) R2[i] = 0, R2[4 + i] = __float_as_int(-1e30f);  // NM[12..15], M = -1e30
#pragma unroll
    for (int i = 0; i < 4; ++i) R3[i] = n16 == 0 ? 0x3f803f80 : 0;
  }

  // ---- prologue: K(0..2), V^T(0..1) in flight; everything landed and published before the first read
  dma.template prologue<3, 2>();
  __builtin_amdgcn_sched_barrier(0);
  // (after the first DMA pieces have been issued: the loads and the scale-and-round of Q run while those are in flight)
  i32x32 QA[2];
  attn_load_q16<QK8>(QA, Q, blk.bh, blk.q0, Lq, g, n16, scale_log2e);
  attn_publish_prologue();

  // ---- the KV stream: one generated asm statement (tools/gen_attention_w16.py), every array pinned to the registers its text names
  f32x32 O[4];
  i32x32 SP0, SP1, FP;  // S^T (v[0:63]), P + fragment buffers (v[64:127]): written before read inside the statement
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    O[0][r] = O[1][r] = O[2][r] = O[3][r] = 0.f;
    SP0[r] = SP1[r] = 0;
    FP[r] = 0;
  }
  i32x32 FB = FP;
  frag_t R4;  // fp8: E8M0 block scales of the score product (byte = biased exponent): 2^-n on the K side, 1 on the Q side
  R4[0] = (int)(((__float_as_uint(scale_log2e) >> 23) & 0xffu) * 0x01010101u), R4[1] = 0x7f7f7f7f, R4[2] = R4[3] = 0;
  i32x32 KF = FP;  // fp8 mode: the four 32-byte K fragment buffers (a[208:239]); named here so that the registers belong to the kernel
  f32x16 OL;  // ones-row accumulators: OL[(2 b + c) * 4] in lanes 0..15 = the row sum of query 32 b + 16 c + n
#pragma unroll
  for (int r = 0; r < 16; ++r) OL[r] = 0.f;
  {
    const AttnBase kb = attn_split_base(dma.Kb), vb = attn_split_base(dma.Vb);
    const float thr = (float)THR_X16 * 0.0625f;
#define FMI_AW16_OPERANDS                                                                                                                      \
    : "+{a[0:31]}"(O[0]), "+{a[32:63]}"(O[1]), "+{a[64:95]}"(O[2]), "+{a[96:127]}"(O[3]), "+{v[0:31]}"(SP0), "+{v[32:63]}"(SP1), "+{v[64:95]}"(FP), \
      "+{v[96:127]}"(FB), "+{v[128:143]}"(R0), "+{v[144:159]}"(R1), "+{v[160:167]}"(R2), "+{v[168:171]}"(R3), "+{v[172:175]}"(R4),               \
      "+{a[192:207]}"(OL), "+{a[208:239]}"(KF)                                                                                                       \
    : "{a[128:159]}"(QA[0]), "{a[160:191]}"(QA[1]), [kb_lo] "s"(kb.lo), [kb_hi] "s"(kb.hi), [vb_lo] "s"(vb.lo), [vb_hi] "s"(vb.hi),                \
      [ntm1] "s"(dma.ntiles - 1), [thr] "s"(thr), [woffk] "s"(wave * dma.KP * 1024), [woffv] "s"(VT_RING + wave * 4096), [rag] "s"(dma.k_last_rows)  \
    : "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201",  \
      "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "s80", "s81", "s82", "s83", "s84", "s85",      \
      "s86", "s87", "s88", "s89", "s90", "s91", "s92", "s93", "s94", "s95", "vcc", "scc", "memory"
    if constexpr (QK8) asm volatile(FMI_AW16F8_LOOP_ASM FMI_AW16_OPERANDS);
    else asm volatile(FMI_AW16_LOOP_ASM FMI_AW16_OPERANDS);
#undef FMI_AW16_OPERANDS
  }

  // ---- epilogue.  Lane (g, n) holds O^T in the 16 x 16 layout (AttnMap16) and the row sums in OL (lanes 0..15); the statement ends drained
  // (nothing in flight).
  attn_drain_rings();
  char* stg = smem + wave * TILE;
  attn_stage_rows<AttnMap16>(stg, O, lane, [&](int q) { return 1.0f / __shfl(OL[q * 4], n16, 64); });  // row 0 of the ones product lives in lane group 0
  attn_store_staged(stg, out, blk, Lq, lane);
}

}  // namespace fmi
