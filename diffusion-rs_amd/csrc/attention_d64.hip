// attention_d64.hip — flash attention at head dim 64 on v_mfma_f32_16x16x32_bf16 with an additive f32 bias and a causal mask: the attention of the encoders
// in front of the denoise loop (T5: d_kv 64, relative-position bias, no 1 / sqrt(d); CLIP text: causal; CLIP vision) and the op-level seam fmi_sdpa_d64_bf16.
// DESIGN.md 4.22.
//
//   O = softmax(Q K^T * scale + bias [+ causal]) V      q, k, v, o bf16 token-major (B, T, H, 64) with independent strides; bias f32 (H, Tq, Tk), shared by the batch
//
// Work split.  A workgroup of 4 waves owns 64 consecutive queries of one (batch, head): wave w owns queries 16 w .. 16 w + 15 and keeps its Q as two MFMA B
// operands in registers.  The keys come by in tiles of 64.  Causal launches stop behind the diagonal tile (the tiles wholly in the future are never fetched);
// the -inf mask is applied by index inside the tiles that need it only: the diagonal one and a ragged last one.  Nothing is padded, nothing is allocated.
//
// Data movement.  K tile: 64 rows of 128 B in LDS, the 16-byte chunk c of row r at chunk c ^ (r & 7) (the 16 rows of an operand read spread over all eight
// chunk positions).  With 16-byte aligned operands the tile arrives by LDS-DMA (__builtin_amdgcn_global_load_lds, 16 B a lane, two 1-KiB pieces per wave) —
// the swizzle is in the GLOBAL address a lane fetches, its LDS slot is fixed by the instruction; otherwise by guarded 2-byte loads through registers into the
// same image.  Rows past Tk fetch row Tk - 1 again (valid memory, masked by index).  V is transposed ON THE WAY IN: a thread loads 8 channels of two
// neighbouring keys and writes eight 4-byte (channel, key pair) words, so LDS holds V^T (64 channels x 64 keys, rows of 136 B) and an A operand of P V is
// two 8-byte reads.  Both tiles are double-buffered: tile t + 1 is requested (K: DMA in flight, V: global loads into registers) before tile t's products and
// V's registers are written behind them; one barrier per tile.
//
// Products.  S^T = K Q^T (A = K rows, B = Q rows: a lane of the 16 x 16 result holds ONE query, n = lane & 15, and keys 4 g .. 4 g + 3 of each 16-key block,
// g = lane >> 4), two k-steps of 32 channels per block.  The softmax is f32 in the log2 domain: s = acc * (scale * log2 e) + bias * log2 e, masked keys -inf,
// row maximum over the lane's 16 values and the four g lanes (two shuffles), p = 2^(s - m) rounded to bf16 ONCE — the rounded values are what both the row sum
// and P V see, so the weights of a row sum to 1 — and the running sum is kept per lane (the four g lanes share every rescale factor) and joined once at the
// end.  O^T = V^T P^T (A = V^T rows = channels, B = P^T): the lane's 8 values of a 32-key step (4 of each of its two blocks) are its B operand as they stand —
// the key order inside a k-step is a permutation both operands share — and the result lane again holds query n, channels 4 g .. 4 g + 3 of each 16-channel block.
//
// Fully masked rows cannot occur: the causal mask always leaves key 0 and every tile a workgroup visits holds a visible key for each of its rows, so there is no
// branch for them (the running maximum starts at -1e30, finite, and is finite after the first tile).
#include <math.h>
#include <stdlib.h>

#include <cmath>

#include "common.h"

namespace fmi {
namespace {

constexpr int D64_KTILE = 64 * 128;  // bytes of a K tile
constexpr int D64_VROW = 136;        // bytes of a V^T row: 64 keys + 8 bytes that keep the 8-byte operand reads of neighbouring channels on different banks
constexpr int D64_VTILE = 64 * D64_VROW;
constexpr float LOG2E = 1.44269504088896340736f;

struct D64Args {
  const bf16_t *q, *k, *v;
  bf16_t* o;
  const float* bias;
  int64_t sq[3], sk[3], sv[3], so[3];  // element strides of batch, token, head
  int Tq, Tk, causal, bias_vec;        // bias_vec: rows of the bias can be read as float4 (Tk % 4 == 0, 16-byte aligned)
  float sl;                            // scale * log2(e)
};

// 8 consecutive bf16: one 16-byte load, or 2-byte loads where the operand is not 16-byte aligned
template <bool ALIGNED>
__device__ __forceinline__ uint4 load8(const bf16_t* p) {
  if (ALIGNED) return *reinterpret_cast<const uint4*>(p);
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)p[2 * i] | ((uint32_t)p[2 * i + 1] << 16);
  return uint4{w[0], w[1], w[2], w[3]};
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void attention_d64_kernel(const D64Args a) {
  __shared__ __attribute__((aligned(16))) char smem[2 * D64_KTILE + 2 * D64_VTILE];  // K tiles [2] at 0, V^T tiles [2] behind them
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z, qw = q0 + wave * 16;
  const int Tq = a.Tq, Tk = a.Tk;
  const bf16_t* Qb = a.q + (int64_t)b * a.sq[0] + (int64_t)h * a.sq[2];
  const bf16_t* Kb = a.k + (int64_t)b * a.sk[0] + (int64_t)h * a.sk[2];
  const bf16_t* Vb = a.v + (int64_t)b * a.sv[0] + (int64_t)h * a.sv[2];
  const int nt_all = (Tk + 63) >> 6;
  const int nt = a.causal ? min(nt_all, (q0 >> 6) + 1) : nt_all;  // causal: the tiles behind the diagonal one lie wholly in the future
  const bool live = qw < Tq;                                      // a wave without a query still stages its share of every tile

  // ---- staging.  K: piece p = 2 wave + j is rows 8 p .. 8 p + 7; lane -> row 8 p + (lane >> 3), LDS chunk lane & 7 = global chunk (lane & 7) ^ (row & 7)
  auto k_src = [&](int t, int j) {
    const int key = min(t * 64 + (2 * wave + j) * 8 + (lane >> 3), Tk - 1);
    return Kb + (int64_t)key * a.sk[1] + (((lane & 7) ^ (lane >> 3)) << 3);
  };
  auto k_dst = [&](int buf, int j) { return smem + buf * D64_KTILE + (2 * wave + j) * 1024; };
  // V: thread -> channels 8 c .. 8 c + 7 (c = tid & 7) of keys 2 kp, 2 kp + 1 (kp = tid >> 3)
  const int vc = tid & 7, vkp = tid >> 3;
  auto v_src = [&](int t, int j) { return Vb + (int64_t)min(t * 64 + 2 * vkp + j, Tk - 1) * a.sv[1] + 8 * vc; };
  uint4 kreg[2], vreg[2];
  auto request = [&](int t, int buf) {  // tile t on its way: K by DMA into `buf`, or K and V into registers
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (ALIGNED)
        __builtin_amdgcn_global_load_lds((glb_void*)k_src(t, j), (lds_void*)k_dst(buf, j), 16, 0, 0);
      else
        kreg[j] = load8<false>(k_src(t, j));
      vreg[j] = load8<ALIGNED>(v_src(t, j));
    }
  };
  auto deposit = [&](int buf) {  // the registers of request() into `buf`
    if (!ALIGNED) {
#pragma unroll
      for (int j = 0; j < 2; ++j) *reinterpret_cast<uint4*>(k_dst(buf, j) + lane * 16) = kreg[j];
    }
    char* vt = smem + 2 * D64_KTILE + buf * D64_VTILE + (8 * vc) * D64_VROW + vkp * 4;
    const uint32_t w0[4] = {vreg[0].x, vreg[0].y, vreg[0].z, vreg[0].w}, w1[4] = {vreg[1].x, vreg[1].y, vreg[1].z, vreg[1].w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<uint32_t*>(vt + (2 * i) * D64_VROW) = (w0[i] & 0xffffu) | (w1[i] << 16);
      *reinterpret_cast<uint32_t*>(vt + (2 * i + 1) * D64_VROW) = (w0[i] >> 16) | (w1[i] & 0xffff0000u);
    }
  };

  // ---- Q fragments (B operand): query qw + n, channels 32 s + 8 g .. + 7.  Rows past Tq read row Tq - 1 and are not stored.
  bf16x8_t qf[2];
  {
    const bf16_t* qp = Qb + (int64_t)min(qw + n, Tq - 1) * a.sq[1] + 8 * g;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint4 u = load8<ALIGNED>(qp + 32 * s);
      __builtin_memcpy(&qf[s], &u, 16);
    }
  }
  const int qi = qw + n;                                                                           // the lane's query (the causal bound)
  const float* brow = a.bias ? a.bias + ((int64_t)h * Tq + min(qi, Tq - 1)) * (int64_t)Tk : nullptr;  // its bias row

  f32x4 o[4];  // O^T: query n, channels 16 dt + 4 g + {0..3}
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_part = 0.f;

  request(0, 0);
  deposit(0);
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1, k0 = t * 64;
    dma_barrier();  // tile t has landed for every wave, and every wave is done with the other buffers
    if (t + 1 < nt) request(t + 1, cur ^ 1);
    if (live) {
      // the lane's bias values of this tile, requested ahead of the score MFMAs: block kb, keys k0 + 16 kb + 4 g + {0..3}
      f32x4 bv[4];
      if (brow) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          const int key = k0 + 16 * kb + 4 * g;
          if (a.bias_vec && key < Tk) {
            bv[kb] = *reinterpret_cast<const f32x4*>(brow + key);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) bv[kb][r] = key + r < Tk ? brow[key + r] : 0.f;
          }
        }
      }
      // S^T = K Q^T
      const char* kt = smem + cur * D64_KTILE;
      f32x4 sc[4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        sc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int r = 16 * kb + n;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(kt + r * 128 + (((4 * s + g) ^ (r & 7)) << 4));
          sc[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], sc[kb], 0, 0, 0);
        }
      }
      // scores in the log2 domain, the index mask where this tile needs one (wave-uniform)
      const bool mask = k0 + 64 > Tk || (a.causal && k0 + 63 > qw);
      float mx = -INFINITY;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = sc[kb][r] * a.sl;
          if (brow) s = fmaf(bv[kb][r], LOG2E, s);
          if (mask) {
            const int key = k0 + 16 * kb + 4 * g + r;
            if (key >= Tk || (a.causal && key > qi)) s = -INFINITY;
          }
          sc[kb][r] = s;
          mx = fmaxf(mx, s);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      // P = 2^(s - m) rounded to bf16 once: the rounded values feed both the row sum and P V
      uint32_t pw[4][2];
      float psum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const uint32_t u = pack_bf16x2(__builtin_amdgcn_exp2f(sc[kb][2 * r] - m_new), __builtin_amdgcn_exp2f(sc[kb][2 * r + 1] - m_new));
          pw[kb][r] = u;
          psum += __uint_as_float(u << 16) + __uint_as_float(u & 0xffff0000u);
        }
      l_part = fmaf(l_part, alpha, psum);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
      // O^T += V^T P^T: k-step ks holds key blocks 2 ks, 2 ks + 1; the lane's k entries are keys 16 (2 ks) + 4 g + {0..3}, 16 (2 ks + 1) + 4 g + {0..3}
      const char* vt = smem + 2 * D64_KTILE + cur * D64_VTILE;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const uint32_t pk[4] = {pw[2 * ks][0], pw[2 * ks][1], pw[2 * ks + 1][0], pw[2 * ks + 1][1]};
        bf16x8_t pf;
        __builtin_memcpy(&pf, pk, 16);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const char* vp = vt + (16 * dt + n) * D64_VROW + (32 * ks + 4 * g) * 2;
          const uint2 v0 = *reinterpret_cast<const uint2*>(vp), v1 = *reinterpret_cast<const uint2*>(vp + 32);
          const uint32_t vk[4] = {v0.x, v0.y, v1.x, v1.y};
          bf16x8_t vf;
          __builtin_memcpy(&vf, vk, 16);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
        }
      }
    }
    if (t + 1 < nt) deposit(cur ^ 1);
  }

  // ---- epilogue: the row sum joined over the four g lanes, O / l as bf16, 4 channels a store
  float l = l_part;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (!live || qi >= Tq) return;
  const float inv = 1.0f / l;
  bf16_t* op = a.o + (int64_t)b * a.so[0] + (int64_t)qi * a.so[1] + (int64_t)h * a.so[2] + 4 * g;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const uint32_t lo = pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv), hi = pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv);
    if (ALIGNED) {
      *reinterpret_cast<uint2*>(op + 16 * dt) = uint2{lo, hi};
    } else {
      op[16 * dt] = (bf16_t)(lo & 0xffffu), op[16 * dt + 1] = (bf16_t)(lo >> 16);
      op[16 * dt + 2] = (bf16_t)(hi & 0xffffu), op[16 * dt + 3] = (bf16_t)(hi >> 16);
    }
  }
}

int g_encoder_attention = [] {
  const char* e = getenv("FMI_ENCODER_ATTENTION");
  return e && e[0] == '1' && !e[1] ? 1 : 0;
}();

}  // namespace

int encoder_attention_kind() { return g_encoder_attention; }
void set_encoder_attention_kind(int kind) { g_encoder_attention = kind; }

int launch_attention_d64(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, int B, int H, int Tq, int Tk, const int64_t* sq, const int64_t* sk,
                         const int64_t* sv, const int64_t* so, float scale, const float* bias, int causal, hipStream_t stream) {
  if (!q || !k || !v || !out) return fail(FMI_ERR_INVALID, "sdpa_d64: null pointer");
  if (B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0) return fail(FMI_ERR_INVALID, "sdpa_d64: empty problem");
  if (B > 65535 || H > 65535) return fail(FMI_ERR_INVALID, "sdpa_d64: B and H must be at most 65535");
  if (!std::isfinite(scale)) return fail(FMI_ERR_INVALID, "sdpa_d64: scale must be finite");
  if (bias && ((uintptr_t)bias & 3)) return fail(FMI_ERR_INVALID, "sdpa_d64: bias must be 4-byte aligned");
  D64Args a{};
  a.q = q, a.k = k, a.v = v, a.o = out, a.bias = bias;
  bool aligned = all_aligned16({q, k, v, out});
  for (int i = 0; i < 3; ++i) {
    a.sq[i] = sq[i], a.sk[i] = sk[i], a.sv[i] = sv[i], a.so[i] = so[i];
    aligned = aligned && !((sq[i] | sk[i] | sv[i] | so[i]) & 7);
  }
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 1) return fail(FMI_ERR_INVALID, "sdpa_d64: operands must be 2-byte aligned");
  a.Tq = Tq, a.Tk = Tk, a.causal = causal ? 1 : 0, a.bias_vec = bias && Tk % 4 == 0 && aligned16(bias);
  a.sl = scale * LOG2E;
  const dim3 grid((Tq + 63) / 64, H, B);
  if (aligned)
    hipLaunchKernelGGL(attention_d64_kernel<true>, grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(attention_d64_kernel<false>, grid, dim3(256), 0, stream, a);
  FMI_LAUNCH_CHECK();
  return FMI_OK;
}

}  // namespace fmi
