// gemm_pp_body.inc — the body of gemm_pp_kernel (gemm_bf16.hip) behind its tile decode, as text: included once per tile height with
//   RB    (constexpr int) 16-row MFMA blocks per wave: 8 = the 256-row tile, 6 = the 192-row tile (bf16 only),
//   tile  (GemmTile) the workgroup's problem / tile, smem (the kernel's own __shared__ array of 5 operand tiles), Q8 and ACT in scope.
// Text and not a function: behind a forced-inline function that took the LDS array by address every instantiation, the 8-bit forms included,
// comes out with other registers and scratch (gemm_frame.h, the exception list).
  constexpr bool FP8 = Q8 != 0;  // 8-bit operands: 1 = OCP e4m3, 2 = int8 (GemmProblem::fp8)
  constexpr bool I8 = Q8 == 2;
  static_assert(RB == 8 || (RB == 6 && !FP8), "the 192-row tile is bf16 only");
  constexpr int NJ = 2, BN = 256;
  constexpr int ES = FP8 ? 1 : 2;  // operand element size
  constexpr int A_RING = 0, W_RING = 2 * A_TILE_BYTES, TILE = A_TILE_BYTES;  // 2 x 32 KiB + 3 x 32 KiB
  constexpr int RG = 16 * RB;  // rows per wave group
  constexpr int AP = RB / 2;   // A-tile DMA pieces per wave: the other group's RG / 8 chunks over 4 waves
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wave >> 2, wn = wave & 3;  // group = row half (wm)

  const GemmProblem& P = tile.P;
  const int m0 = tile.m0, n0 = tile.n0, nk = tile.nk;

  // fp8: v_mfma_f32_32x32x64_f8f6f4, accumulators acc[4][NJ] of 32 x 32 (Acc32).  bf16: v_mfma_f32_16x16x32_bf16, accumulators
  // acc16[8][2 NJ] of 16 x 16 (Acc16) — on this power-capped part the 16 x 16 x 32 form sustains 14 % more than 32 x 32 x 16
  // (tools/mfma_peak); same LDS image, the fragment of a 16-row block is rows lane & 15 at k slot 4 s + (lane >> 4).
  // int8: v_mfma_i32_32x32x32_i8, two per 32-byte fragment pair (each 16-byte fragment is one instruction's 32-k operand), accumulators
  // acci of the same shape and lane layout as acc; the sums are exact integers, converted once behind the K loop.
  f32x16 acc[FP8 ? 4 : 1][NJ];
  i32x16_t acci[I8 ? 4 : 1][NJ];
  f32x4 acc16[FP8 ? 1 : RB][2 * NJ];
  if constexpr (I8) zero(acci);
  else if constexpr (FP8) zero(acc);
  else {  // (written out: behind zero() hipcc assigned the accumulators of <0, 1..3> other registers and their K loop lost two v_mov_b64, gemm_frame.h)
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int j = 0; j < 2 * NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc16[i][j][r] = 0.f;
  }

  // fragment blocks of 32 rows (8-bit: 16-byte k slots 2 s + (lane >> 5), s = 0..3) or 16 (bf16: slots 4 s + (lane >> 4), s = 0..1)
  const auto frag = frag_slots<FP8 ? 32 : 16>(lane);
  const auto& koff = frag.koff;
  const int a_row_off = frag.row_off(g * RG);
  const int w_row_off = frag.row_off(wn * 64);

  // chunks (8 rows, 1 KiB) this wave stages: AP A chunks of the other group's rows ((wave ^ 4) * 4 in the 256-row tile), W chunks wave*4+i
  const int a_chunk0 = ((g ^ 1) * 4 + wn) * AP, w_chunk0 = wave * 4;
  // per-lane BYTE offsets (32-bit) from the uniform tile base, so the DMA uses the saddr + voffset form: 8 VGPRs instead of 16 for
  // pointers (the kernel sits at the 256-register limit and a spilled pointer costs a vmcnt(0) reload — a full pipeline drain).
  // The text of TileDma (gemm_frame.h), kept here: behind the struct this kernel's bf16 form came out with another scratch size.
  uint32_t a_off[AP], w_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ra = (a_chunk0 + i) * 8 + (lane >> 3), rw = (w_chunk0 + i) * 8 + (lane >> 3);
    if (i < AP) a_off[i] = (uint32_t)((int64_t)(min(m0 + ra, P.M - 1) - m0) * P.lda * ES + (((lane & 7) ^ ((ra >> 1) & 7)) << 4));
    w_off[i] = (uint32_t)((int64_t)(min(n0 + rw, P.N - 1) - n0) * P.ldw * ES + (((lane & 7) ^ ((rw >> 1) & 7)) << 4));
  }
  const char* const a_base = reinterpret_cast<const char*>(P.A) + (int64_t)m0 * P.lda * ES;
  const char* const w_base = reinterpret_cast<const char*>(P.W) + (int64_t)n0 * P.ldw * ES;
  auto dma_a = [&](int kt, int i) {
    const char* base = a_base + (int64_t)kt * (BK * 2);  // uniform
    __builtin_amdgcn_global_load_lds((glb_void*)(base + a_off[i]), (lds_void*)(smem + A_RING + (kt & 1) * TILE + (a_chunk0 + i) * 1024), 16, 0, 0);
  };
  auto dma_w = [&](int kt, int slot, int i) {
    const char* base = w_base + (int64_t)kt * (BK * 2);
    __builtin_amdgcn_global_load_lds((glb_void*)(base + w_off[i]), (lds_void*)(smem + W_RING + slot * TILE + (w_chunk0 + i) * 1024), 16, 0, 0);
  };

  // ---- prologue: what the steady-state rule would have issued before LOAD(0): A(0) (both
  // halves), W(0), W(1), and the rows group 0 reads of A(1) (staged by group 1)
#pragma unroll
  for (int i = 0; i < AP; ++i) dma_a(0, i);
#pragma unroll
  for (int i = 0; i < 4; ++i) dma_w(0, 0, i);
  if (nk > 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dma_w(1, 1, i);
    if (g == 1) {
#pragma unroll
      for (int i = 0; i < AP; ++i) dma_a(1, i);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  slot_barrier();
  if (g == 1) slot_barrier();  // group 1 starts one slot late

  bf16x8_t xf[2][RB], wf[2][2 * NJ];  // bf16: fragments of the 2 k-steps of 32: RB row blocks of A, 2 NJ of W (16 rows each)
  i32x8_t xq[2][4], wq[2][NJ];    // fp8: fragments of the 2 k-steps (two 16-byte reads each)
  int wr = 0;  // W slot of tile t = t % 3
  int wi = 2;  // W slot of tile t + 2
  auto ktile = [&](int t, auto main_tag) {
    constexpr bool MAIN = decltype(main_tag)::value;  // steady state: both issues are in range
    // ---- LOAD(t): fragments -> registers, then this wave's DMA pieces (issuing them first was
    // measured 8-10 % slower: the ds_reads queue up behind DMA instructions blocked on a full queue)
    const bool a_ok = MAIN || (t + 1 + g < nk);
    const bool w_ok = MAIN || (t + 2 < nk);
    auto issue_dma = [&]() {
      if (a_ok) {
#pragma unroll
        for (int i = 0; i < AP; ++i) dma_a(t + 1 + g, i);
      }
      if (w_ok) {
#pragma unroll
        for (int i = 0; i < 4; ++i) dma_w(t + 2, wi, i);
      }
    };
    {
      const char* la = smem + A_RING + (t & 1) * TILE + a_row_off;
      const char* lw = smem + W_RING + wr * TILE + w_row_off;
      if constexpr (FP8) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            wq[s][j] = __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(lw + j * 32 * 128 + koff[2 * s]),
                                               *reinterpret_cast<const i32x4_t*>(lw + j * 32 * 128 + koff[2 * s + 1]), 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            xq[s][i] = __builtin_shufflevector(*reinterpret_cast<const i32x4_t*>(la + i * 32 * 128 + koff[2 * s]),
                                               *reinterpret_cast<const i32x4_t*>(la + i * 32 * 128 + koff[2 * s + 1]), 0, 1, 2, 3, 4, 5, 6, 7);
        }
      } else {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
          for (int j = 0; j < 2 * NJ; ++j) wf[s][j] = *reinterpret_cast<const bf16x8_t*>(lw + j * 16 * 128 + koff[s]);
#pragma unroll
          for (int i = 0; i < RB; ++i) xf[s][i] = *reinterpret_cast<const bf16x8_t*>(la + i * 16 * 128 + koff[s]);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    issue_dma();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (RB == 8) {
      if (MAIN) {
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      } else {  // tail: wait for everything but what was issued just now
        if (a_ok && w_ok)
          asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (a_ok || w_ok)
          asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    } else {  // 192-row tile: AP = 3 A pieces + 4 W pieces per LOAD
      if (MAIN || (a_ok && w_ok))
        asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
      else if (w_ok)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else if (a_ok)
        asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    slot_barrier();
    // ---- COMPUTE(t): the matrix pipe only
    if constexpr (I8) {
      // two instructions per 32-byte fragment pair, the halves in separate sweeps over the 8 accumulators (no instruction follows one on its own accumulator)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
              acci[i][j] = h == 0 ? __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_shufflevector(wq[s][j], wq[s][j], 0, 1, 2, 3),
                                                                         __builtin_shufflevector(xq[s][i], xq[s][i], 0, 1, 2, 3), acci[i][j], 0, 0, 0)
                                  : __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_shufflevector(wq[s][j], wq[s][j], 4, 5, 6, 7),
                                                                         __builtin_shufflevector(xq[s][i], xq[s][i], 4, 5, 6, 7), acci[i][j], 0, 0, 0);
    } else if constexpr (FP8) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wq[s][j], xq[s][i], acc[i][j], 0, 0, 0, 0, 0, 0);  // e4m3 x e4m3, unscaled
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
          for (int j = 0; j < 2 * NJ; ++j) acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s][j], xf[s][i], acc16[i][j], 0, 0, 0);
    }
    slot_barrier();
    wr = wr == 2 ? 0 : wr + 1;
    wi = wi == 2 ? 0 : wi + 1;
  };
  const int nmain = nk > 2 ? nk - 2 : 0;  // t + 2 < nk  (and t + 1 + g < nk)
  for (int t = 0; t < nmain; ++t) ktile(t, std::true_type{});
  for (int t = nmain; t < nk; ++t) ktile(t, std::false_type{});
  if (g == 0) slot_barrier();  // group 0 finished one slot early

  if constexpr (I8) {  // the exact integer sums as f32 (v_cvt_f32_i32: round to nearest even beyond 2^24, as the oracle's (float) cast)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = (float)acci[i][j][r];
  }
  if constexpr (FP8) {  // dequantise: per-token scale of the row, per-channel scale of the 4 consecutive columns
    float sa[4], oa[4];
    const bool off = I8 && P.a_off != nullptr;  // int8, post-GELU form of the row codes: + a_off[m] * w_sum[n] (uniform per problem)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = min(m0 + g * 128 + i * 32 + (lane & 31), P.M - 1);
      sa[i] = P.a_scale[r];
      oa[i] = off ? P.a_off[r] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + wn * 64 + j * 32 + 8 * q + 4 * (lane >> 5);
        float sn[4], wsn[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          sn[c] = P.w_scale[min(n + c, P.N - 1)];
          wsn[c] = off ? P.w_sum[min(n + c, P.N - 1)] : 0.f;
        }
        if (off) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][j][4 * q + c] = acc[i][j][4 * q + c] * (sa[i] * sn[c]) + oa[i] * wsn[c];
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[i][j][4 * q + c] *= sa[i] * sn[c];
        }
      }
  }
  // the lane id is laundered (as in w4_epilogue): what the epilogue derives from it is then computed here, not hoisted above the
  // K loop, held across 256 registers of loop state, spilled and reloaded (a scratch reload waits vmcnt(0): the stores serialise)
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  if constexpr (FP8) gemm_epilogue<NJ, 4, ACT>(P, Acc32<NJ>{acc, lane_e}, smem, m0, n0, wave, lane_e);
  else gemm_epilogue<NJ, 4, ACT>(P, Acc16<NJ, RB>{acc16, lane_e}, smem, m0, n0, wave, lane_e);
