"""The f32 reference of the first-block step cache: the denoise loop composed from the oracle's block hooks in numpy, with the cache's
semantics written out — every step runs img_in and double block 0, takes r = X1 - X0, measures per sample sum|r - r_ref| / sum|r_ref| in double against the
last COMPUTED step's residual, and either adds the cached output residual of the other blocks (XF = X1 + delta) or runs them and refreshes delta and r_ref.
Without reuse it is om.denoise (tests/test_host_step_cache.py holds it to 1e-6).

Also the shared configuration of the step-cache tests: SMALL_FLUX, Philox weights of seed 0, flux_inputs(..., seed=7), guidance 3.5, B = 2, T = 32 and the two
shape sets of the Kontext tests (ragged: S = 4x6, R = 5x7 — odd row counts, the stand-alone relayout kernels; aligned: S = 8x8, R = 6x8 — the fused epilogues)."""
import functools

import numpy as np

from tests.util import SMALL_FLUX, flux_inputs

f32 = np.float32
B, T = 2, 32
SHAPES = {"ragged": ((4, 6), (5, 7)), "aligned": ((8, 8), (6, 8))}
THRESHOLD = 0.235  # every compared distance of both shape sets is >= 9 % away from it on the oracle (test_host_step_cache.py asserts >= 5 %)
THRESHOLD_DECISIONS = [0, 1, 1, 1, 1, 0, 1, 1]
MASK_A = [0, 0, 1, 1, 0, 1, 0, 1]
MASK_B = [0, 1, 1, 1, 1, 1, 1, 1]
REPEAT_TS = [1.0, 1.0, 0.6, 0.6, 0.25, 0.25, 0.0]  # steps 1, 3, 5 see the very state and time of the step before (dt = 0)
REPEAT_FORCE = [0, 1, 0, 1, 0, 1]


def np_ids(Bn, h2, w2, id0=0.0):
    ids = np.zeros((Bn, h2 * w2, 3), np.float32)
    ids[:, :, 0] = f32(id0)
    ids[:, :, 1] = np.repeat(np.arange(h2), w2).astype(np.float32)[None]
    ids[:, :, 2] = np.tile(np.arange(w2), h2).astype(np.float32)[None]
    return ids


@functools.lru_cache(maxsize=None)
def state_dict():
    import diffusion_rs_amd as d
    return d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)


@functools.lru_cache(maxsize=None)
def oracle_model():
    from oracle import oracle as orc
    om = orc.Flux(SMALL_FLUX)
    om.load(state_dict())
    return om


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """The inputs of one shape set (read-only: shared by every test)."""
    s_hw, r_hw = SHAPES[shape]
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, s_hw, T, seed=7)
    ctx = flux_inputs(SMALL_FLUX, B, r_hw, T, seed=8)[0]
    s = dict(S=s_hw[0] * s_hw[1], R=r_hw[0] * r_hw[1], img=img, ids=ids, txt=txt, txt_ids=txt_ids, y=y, ctx=ctx, rids=np_ids(B, r_hw[0], r_hw[1], 1.0),
             g=np.full(B, 3.5, np.float32))
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def schedule(shape, n=8):
    from oracle import oracle as orc
    S = inputs(shape)["S"]
    return list(orc.get_timesteps(n, True, orc.calculate_shift(S)))


def composed_denoise(om, sd, cfg, img, ids, txt, txt_ids, y, g, ts, threshold=0.0, force=None, ctx=None, ctx_ids=None, sl=slice(None)):
    """(latents (B,S,C) f32, decisions (n,) int, distances (n,B) f64, -1 where not measured).  threshold 0 and no force: the plain loop."""
    from oracle import oracle as orc
    img, ids, txt, txt_ids, y, g = (a[sl] for a in (img, ids, txt, txt_ids, y, g))
    D = cfg["num_attention_heads"] * 128
    n = len(ts) - 1
    Bn, S, _ = img.shape
    Tn = txt.shape[1]

    def emb(p, v):
        h = orc.silu(orc.linear(v, sd[p + ".linear_1.weight"], sd[p + ".linear_1.bias"]))
        return orc.linear(h, sd[p + ".linear_2.weight"], sd[p + ".linear_2.bias"])

    all_ids = ids if ctx is None else np.concatenate([ids, ctx_ids[sl]], 1)
    pe = orc.rope_table(np.concatenate([txt_ids, all_ids], 1), cfg["axes_dim"], cfg["theta"])
    x_txt0 = orc.linear(txt, sd["context_embedder.weight"], sd["context_embedder.bias"])
    static = emb("time_text_embed.guidance_embedder", orc.timestep_embedding(g)) + emb("time_text_embed.text_embedder", y)
    x = np.array(img, np.float32)
    decisions = np.zeros(n, np.int64)
    distances = np.full((n, Bn), -1.0, np.float64)
    valid, r_ref, delta = False, None, None
    for i in range(n):
        t = np.full(Bn, f32(ts[i]), np.float32)
        vec = emb("time_text_embed.timestep_embedder", orc.timestep_embedding(t)) + static
        xin = x if ctx is None else np.concatenate([x, ctx[sl]], 1)
        X0 = orc.linear(xin, sd["x_embedder.weight"], sd["x_embedder.bias"])
        X1, xt = om.double_block(0, X0, x_txt0, vec, pe)
        r = (X1 - X0).astype(np.float32)
        if valid:
            num = np.abs(r.astype(np.float64) - r_ref).sum(axis=(1, 2))
            den = np.abs(r_ref.astype(np.float64)).sum(axis=(1, 2))
            with np.errstate(divide="ignore", invalid="ignore"):
                distances[i] = np.where(den == 0, np.inf, num / den)
        f = -1 if force is None else int(force[i])
        reuse = valid and (f == 1 or (f < 0 and threshold > 0 and distances[i].max() < threshold))
        decisions[i] = int(reuse)
        if reuse:
            XF = (X1 + delta).astype(np.float32)
        else:
            xi = X1
            for k in range(1, cfg["num_layers"]):
                xi, xt = om.double_block(k, xi, xt, vec, pe)
            xx = np.concatenate([xt, xi], 1)
            for k in range(cfg["num_single_layers"]):
                xx = om.single_block(k, xx, vec, pe)
            XF = xx[:, Tn:]
            delta, r_ref, valid = (XF - X1).astype(np.float32), r, True
        ss = orc.linear(orc.silu(vec), sd["norm_out.linear.weight"], sd["norm_out.linear.bias"])
        xn = orc.layer_norm(XF[:, :S], None, None, 1e-6) * (1 + ss[:, None, :D]) + ss[:, None, D:]
        pred = orc.linear(xn.astype(np.float32), sd["proj_out.weight"], sd["proj_out.bias"])
        x = (x + pred * f32(ts[i + 1] - ts[i])).astype(np.float32)
    return x, decisions, distances


@functools.lru_cache(maxsize=None)
def reference(shape, kind, with_context=False):
    """The composed reference of one shape set, computed once and shared (read-only).  kind: "plain", "mask_a", "mask_b", "threshold" on the 8-step schedule;
    "repeat_plain" / "repeat_cached" on REPEAT_TS."""
    s = inputs(shape)
    kw = dict(ctx=s["ctx"], ctx_ids=s["rids"]) if with_context else {}
    ts = REPEAT_TS if kind.startswith("repeat") else schedule(shape)
    kw.update({"plain": {}, "repeat_plain": {}, "mask_a": dict(force=MASK_A), "mask_b": dict(force=MASK_B), "threshold": dict(threshold=THRESHOLD),
               "repeat_cached": dict(force=REPEAT_FORCE)}[kind])
    out = composed_denoise(oracle_model(), state_dict(), SMALL_FLUX, s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], ts, **kw)
    for a in out:
        a.setflags(write=False)
    return out
