"""Inputs for which ops.sdpa_d64's exact output is known (tests/test_gpu_sdpa_d64_exact.py), built on the CPU; tests/test_host_sdpa_d64_inputs.py proves in
float64 what the GPU test takes for granted.

The softmax of every query is one-hot in the kernel's f32 arithmetic: the selected key pi[h, i] has the row's largest score, so its weight is 2^0 = 1, and
every other visible key lies at least MARGIN below it in the log2 domain, where an f32 exp2 is exactly 0 (the smallest f32 denormal is 2^-149).  The row sum is 1
and out[b, i, h, :] is v[b, pi[h, i], h, :] bit for bit.  Everything here is a CPU tensor."""
import math

import numpy as np
import torch

B, H = 2, 3
MARGIN = 200.0  # log2-domain gap the host test demands between the selected key and every other visible key
LOG2E = math.log2(math.e)

SHAPES = [(1, 1), (16, 64), (64, 65), (70, 68), (130, 257), (257, 130), (200, 1000)]
MAPS = ["identity", "reversal", "first", "last", "random", "tile_edges"]
ODD_OFFSET_SHAPES = [(70, 68), (130, 257)]  # run in the odd-offset operand layout as well
# (Tq, Tk, map, causal): what the GPU file runs for both builders and the host file proves
ROUTING_CASES = [(Tq, Tk, m, causal) for Tq, Tk in SHAPES for m in MAPS for causal in (False, True)]
LADDER_SHAPES = [(70, 256), (130, 250)]  # four key tiles each, the last one ragged in the second


def key_map(name, Tq, Tk, causal, seed=0):
    """pi (H, Tq) int64: the key each query selects.  Under causal every pi[h, i] <= i: the map is folded into the n_i = min(i, Tk - 1) + 1 visible keys
    ("last" becomes the last visible one, the diagonal).  Only "random" differs between the heads."""
    i = np.arange(Tq, dtype=np.int64)
    n_vis = np.minimum(i, Tk - 1) + 1 if causal else np.full(Tq, Tk, np.int64)
    if name == "identity":
        pi = i % Tk
    elif name == "reversal":
        pi = (Tk - 1 - i) % Tk
    elif name == "first":
        pi = np.zeros(Tq, np.int64)
    elif name == "last":
        pi = n_vis - 1
    elif name == "tile_edges":
        pi = (64 * i + 63) % Tk
    elif name == "random":
        pi = np.random.default_rng(seed + 1000 * Tq + Tk).integers(0, 1 << 30, (H, Tq)).astype(np.int64)
    else:
        raise ValueError(name)
    return torch.from_numpy(np.broadcast_to(pi % n_vis, (H, Tq)).copy())


def key_code(j):
    """(..., 64) f32: key j < 1024 as 16 (e_{j mod 32} + e_{32 + j div 32}).  Two codes share 2, 1 or 0 of their ones: dot products 512, 256, 0."""
    j = torch.as_tensor(j, dtype=torch.int64)
    assert int(j.max()) < 1024 and int(j.min()) >= 0
    code = torch.zeros(tuple(j.shape) + (64,))
    code.scatter_(-1, (j % 32).unsqueeze(-1), 16.0)
    code.scatter_(-1, (32 + j // 32).unsqueeze(-1), 16.0)
    return code


def values(Tk, seed):
    """v (B, Tk, H, 64) bf16: randn + key 2^-7 rounded to bf16, no zeros (a sum of +0 products cannot give back a -0).  The host test proves that the Tk rows
    of a (batch, head) differ pairwise as bit patterns."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn((B, Tk, H, 64), generator=g) + torch.arange(Tk)[None, :, None, None] * 2.0 ** -7).to(torch.bfloat16)
    return torch.where(v == 0, torch.ones_like(v), v)


def select_by_qk(Tq, Tk, pi):
    """Builder (a): q (B, Tq, H, 64), k (B, Tk, H, 64) bf16 and scale 1.0, no bias.  Query i of head h carries the code of key pi[h, i]."""
    k = key_code(torch.arange(Tk))[None, :, None, :].expand(B, Tk, H, 64)
    q = key_code(pi).permute(1, 0, 2)[None].expand(B, Tq, H, 64)
    return q.to(torch.bfloat16).contiguous(), k.to(torch.bfloat16).contiguous(), 1.0


def select_by_bias(Tq, Tk, pi, seed):
    """Builder (b): small random q, k (randn x 0.1), the default scale 1 / 8, and an f32 bias (H, Tq, Tk) of 1000 at [h, i, pi[h, i]], 0 elsewhere."""
    g = torch.Generator().manual_seed(seed)
    q, k = ((torch.randn((B, T, H, 64), generator=g) * 0.1).to(torch.bfloat16) for T in (Tq, Tk))
    bias = torch.zeros((H, Tq, Tk))
    bias.scatter_(2, pi.unsqueeze(-1), 1000.0)
    return q, k, 0.125, bias


def ladder_bias(Tq, Tk):
    """A bias under which every row's running maximum moves in every key tile: tile t holds one key with a bias of 300 (t + 1), 300 above the best of the tile
    before it (433 in the log2 domain), at a place that changes with the row and the head; 0 elsewhere.  Returns (bias (H, Tq, Tk), pi (H, Tq)): the
    selected key is the last tile's."""
    nt = (Tk + 63) // 64
    h, i = torch.arange(H)[:, None], torch.arange(Tq)[None, :]
    bias, pi = torch.zeros((H, Tq, Tk)), None
    for t in range(nt):
        pi = torch.minimum(64 * t + (7 * i + 13 * t + 29 * h) % 64, torch.tensor(Tk - 1))
        bias.scatter_(2, pi.unsqueeze(-1), 300.0 * (t + 1))
    return bias, pi


def log2_scores(q, k, scale, bias, causal):
    """float64 (B, H, Tq, Tk): the scores as the kernel forms them, in the log2 domain; masked keys -inf."""
    s = torch.einsum("bihc,bjhc->bhij", q.double(), k.double()) * (scale * LOG2E)
    if bias is not None:
        s = s + bias.double()[None] * LOG2E
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool).triu(1), float("-inf"))
    return s


def selection_margin(q, k, scale, bias, causal, pi):
    """The smallest gap, over all (b, h, i), between the score of key pi[h, i] and the best other visible key (+inf when there is no other); -inf if a
    selected key is masked."""
    s = log2_scores(q, k, scale, bias, causal)
    idx = pi[None, :, :, None].expand(s.shape[0], -1, -1, 1)
    chosen = s.gather(3, idx)
    others = s.scatter(3, idx, float("-inf")).amax(3, keepdim=True)
    gap = torch.where(torch.isinf(chosen), torch.full_like(chosen, float("-inf")), chosen - others)
    return float(gap.min())
