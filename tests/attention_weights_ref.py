"""Float64 NumPy reference of the attention with token group masks and per-key weights, and the weight patterns its tests use.  A helper, not a test."""
import numpy as np

from tests import attention_groups_ref as G


def weighted_attention(q, k, v, qg, kg, kw, scale):
    """O_i = sum_j w_j e^(s_ij) v_j / sum_j w_j e^(s_ij) over the keys j query i sees, s = scale q.k, in float64; operands and words as
    attention_groups_ref.masked_attention, kw (Bg, Lk) positive weights."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    s = q @ k.transpose(0, 1, 3, 2) * scale
    seen = (np.asarray(qg, np.uint32)[:, None, :, None] & np.asarray(kg, np.uint32)[:, None, None, :]) != 0
    p = np.where(seen, np.exp(s - s.max(-1, keepdims=True)) * np.asarray(kw, np.float64)[:, None, None, :], 0.0)
    return (p / p.sum(-1, keepdims=True)) @ v


def weights(pattern, Lk, Bg):
    """(Bg, Lk) float32, different per sample: "random" = 2 ** uniform(-6, 3); "ones-but-one-tile" = 1 but for the keys 64 .. 127 (the first 64 where there is
    one tile only), so that tiles with and without a term meet in one row's running maximum."""
    w = (2.0 ** np.random.default_rng(Lk + 7).uniform(-6, 3, (Bg, Lk))).astype(np.float32)
    if pattern == "ones-but-one-tile":
        lo = 64 if Lk > 64 else 0
        w[:, :lo], w[:, lo + 64:] = 1, 1
    return w


def flux_forward(sd, cfg, *args, weights, groups=None):
    """attention_groups_ref.flux_forward — the oracle's forward restated on its primitives — with weighted_attention as every block's joint attention; weights
    (Bw, T + S)."""
    plain = G.masked_attention
    G.masked_attention = lambda q, k, v, qg, kg, scale: weighted_attention(q, k, v, qg, kg, weights, scale)
    try:
        return G.flux_forward(sd, cfg, *args, groups=groups)
    finally:
        G.masked_attention = plain
