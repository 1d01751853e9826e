// ip_adapter.h — the FLUX IP-Adapter handle, shared by ip_adapter.hip (the handle, its kernels, the once-per-call projection) and
// flux_model.hip (validation, the hoisting in the loop, the hook of forward_core).
#pragma once
#include "common.h"

// An IP-Adapter for a FLUX transformer of width D = H * 128 with nd double blocks: image_proj (Linear(E -> N * J) + LayerNorm(J)) and one to_k_ip / to_v_ip
// Linear(J -> D) per double block.  It owns its weights and the per-call buffers the projection fills; the main model only reads kv.
struct fmi_ip_adapter {
  int device = 0;
  int D = 0, H = 0, J = 0, nd = 0, E = 0, N = 0;
  fmi::DeviceBuffer weights;             // one block: the six arrays below
  fmi::bf16_t *proj_w = nullptr, *proj_b = nullptr;  // image_proj.image_embeds (N * J, E), (N * J)
  float *ln_w = nullptr, *ln_b = nullptr;            // image_proj.norm (J), kept in f32
  fmi::bf16_t *kv_w = nullptr, *kv_b = nullptr;      // rows (i * 2 + which) * D + d of (nd * 2 * D, J): to_k_ip (which 0) / to_v_ip (1) of block i; biases zero unless set
  fmi::MissingSet missing;
  // per call, sized by the first call and regrown when a larger batch comes (ip_prepare)
  fmi::DeviceBuffer emb;     // f32 (Bt, E): the prompt halves' embeds, then the negative halves'
  fmi::DeviceBuffer tok;     // f32 2 x (Bt * N, J): the projection before and after the LayerNorm
  fmi::DeviceBuffer kv_f32;  // f32 (Bt * N, nd * 2 * D)
  fmi::DeviceBuffer kv;      // bf16 (nd, 2, Bt, H, N, 128): what the kernel reads
  int kv_B = 0;              // Bt of the last projection
  const fmi::bf16_t* k_of(int block) const { return kv.as<fmi::bf16_t>() + (size_t)(block * 2) * kv_B * D * N; }
  const fmi::bf16_t* v_of(int block) const { return kv.as<fmi::bf16_t>() + (size_t)(block * 2 + 1) * kv_B * D * N; }
};

namespace fmi {
constexpr int IP_MAX_TOKENS = 32;
// tok = LayerNorm(Linear(embeds)) and every block's K / V for Bt = (with_negative ? 2 : 1) * Bs samples: rows [0, Bs) from embeds (Bs, E), rows [Bs, 2 Bs) from
// neg_embeds, or from all-zero embeddings when it is null.  Once per call: nothing here depends on the state or on t.
int ip_prepare(fmi_ip_adapter* a, const void* embeds, const void* neg_embeds, fmi_dtype dt, int Bs, bool with_negative, hipStream_t s);
// x[b, r, h * 128 + e] += c * (softmax_n(rmsnorm(q[b, r, h, :]) . K[b, h, n, :] / sqrt(128)) . V[b, h, :, e]) — see ip_adapter.hip for the recipe.
int launch_ip_attention(const bf16_t* q, int ldq, int64_t q_bs, const bf16_t* wq, const bf16_t* K, const bf16_t* V, float* x, int64_t x_bs, int B, int H, int S, int N,
                        float c, int max_row_blocks, hipStream_t stream);
}  // namespace fmi
