"""Float64 NumPy reference of the attention with token group masks, and the word patterns its tests use.  A helper, not a test."""
import numpy as np


def masked_attention(q, k, v, qg, kg, scale):
    """softmax(q k^T * scale + M) v in float64; q (B,H,Lq,d), k, v (B,H,Lk,d); qg (Bg,Lq), kg (Bg,Lk) unsigned words, Bg 1 or B; M = -inf where the words share no bit."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    s = q @ k.transpose(0, 1, 3, 2) * scale
    seen = (np.asarray(qg, np.uint32)[:, None, :, None] & np.asarray(kg, np.uint32)[:, None, None, :]) != 0
    s = np.where(seen, s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)) @ v


def words(pattern, Lq, Lk, B=2):
    """(qg, kg) uint32 (B, L), different per sample, every query with a visible key (key i itself where Lq == Lk)."""
    i, j = np.arange(Lq), np.arange(Lk)
    if pattern == "all":
        return np.stack([np.full(Lq, 1 + 2 * b, np.uint32) for b in range(B)]), np.stack([np.full(Lk, 1 << b, np.uint32) for b in range(B)])
    if pattern in ("block64", "block24"):  # block-diagonal (queries past the last key block see that one); the odd samples' queries see the first block as well
        n = 64 if pattern == "block64" else 24
        qg = np.stack([(1 << (np.minimum(i, Lk - 1) // n + b)) | ((b & 1) << b) for b in range(B)]).astype(np.uint32)
        return qg, np.stack([1 << (j // n + b) for b in range(B)]).astype(np.uint32)
    assert pattern == "random"
    rng = np.random.default_rng(Lq * 1000 + Lk)
    word = lambda L: rng.integers(0, 2 ** 32, (B, L), dtype=np.uint64).astype(np.uint32)
    sparse = lambda L: word(L) & word(L) & word(L)  # a bit is set with probability 1 / 8: two tokens share one in about 40 % of the pairs
    return sparse(Lq) | (1 << (i % 32)).astype(np.uint32), sparse(Lk) | (1 << (j % 32)).astype(np.uint32)


def flux_forward(sd, cfg, x, ids, txt, txt_ids, t, y, g, groups=None):
    """Flux::forward restated on the oracle's f32 primitives with masked_attention as every block's joint attention (groups: words (Bg, T + S), None = all
    visible).  The oracle's own blocks are compiled, so its attention has no mask to set; unmasked, this restatement is held equal to oracle.Flux.forward."""
    from oracle import oracle as orc
    from tests.controlnet_ref import _vec
    H = cfg["num_attention_heads"]
    D, B, T = H * 128, x.shape[0], txt.shape[1]
    lin = lambda a, p: orc.linear(np.ascontiguousarray(a, np.float32), sd[p + ".weight"], sd[p + ".bias"])
    vec = _vec(orc, sd, cfg, t, y, g)
    pe = orc.rope_table(np.concatenate([txt_ids, ids], 1), cfg["axes_dim"], cfg["theta"])
    words = np.ones((1, T + x.shape[1]), np.uint32) if groups is None else groups
    mod = lambda p, n: np.split(lin(orc.silu(vec), p)[:, None, :], n, -1)
    norm = lambda a, sc, sh: (orc.layer_norm(np.ascontiguousarray(a, np.float32), None, None, 1e-6) * (1 + sc) + sh).astype(np.float32)

    def heads(a, p, proj, nrm):  # q, k (normed) and v of rows a: (B, H, n, 128)
        qkv = [lin(a, p + proj[i]).reshape(B, -1, H, 128) for i in range(3)]
        qkv[0], qkv[1] = orc.rms_norm_slow(qkv[0], sd[p + nrm[0] + ".weight"], 1e-6), orc.rms_norm_slow(qkv[1], sd[p + nrm[1] + ".weight"], 1e-6)
        return [np.ascontiguousarray(a.transpose(0, 2, 1, 3), np.float32) for a in qkv]

    def attend(q, k, v):  # rope on q and k, the masked attention, back to (B, L, D)
        q, k = (np.stack([orc.apply_rope(a[b], pe[b]) for b in range(B)]) for a in (q, k))
        return masked_attention(q, k, v, words, words, 128 ** -0.5).transpose(0, 2, 1, 3).reshape(B, -1, D).astype(np.float32)

    xi, xt = lin(x, "x_embedder"), lin(txt, "context_embedder")
    for i in range(cfg["num_layers"]):
        p = f"transformer_blocks.{i}."
        mi, mt = mod(p + "norm1.linear", 6), mod(p + "norm1_context.linear", 6)
        hi = heads(norm(xi, mi[1], mi[0]), p + "attn.", ("to_q", "to_k", "to_v"), ("norm_q", "norm_k"))
        ht = heads(norm(xt, mt[1], mt[0]), p + "attn.", ("add_q_proj", "add_k_proj", "add_v_proj"), ("norm_added_q", "norm_added_k"))
        a = attend(*(np.concatenate([b, c], 2) for b, c in zip(ht, hi)))
        for s, (xs, m, out, ff) in enumerate(((xi, mi, "attn.to_out.0", "ff"), (xt, mt, "attn.to_add_out", "ff_context"))):
            xs = xs + m[2] * lin(a[:, T:] if s == 0 else a[:, :T], p + out)
            xs = (xs + m[5] * lin(orc.gelu(lin(norm(xs, m[4], m[3]), p + ff + ".net.0.proj")), p + ff + ".net.2")).astype(np.float32)
            xi, xt = (xs, xt) if s == 0 else (xi, xs)
    xx = np.concatenate([xt, xi], 1)
    for j in range(cfg["num_single_layers"]):
        p = f"single_transformer_blocks.{j}."
        m = mod(p + "norm.linear", 3)
        xm = norm(xx, m[1], m[0])
        a = attend(*heads(xm, p + "attn.", ("to_q", "to_k", "to_v"), ("norm_q", "norm_k")))
        xx = (xx + m[2] * lin(np.concatenate([a, orc.gelu(lin(xm, p + "proj_mlp"))], -1), p + "proj_out")).astype(np.float32)
    m = mod("norm_out.linear", 2)
    return lin(norm(xx[:, T:], m[0], m[1]), "proj_out")
