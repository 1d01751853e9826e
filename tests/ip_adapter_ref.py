"""The FLUX IP-Adapter composed on the CPU oracle's op-level functions and block hooks, in f32:

  project              tok = LayerNorm(Linear(embeds)) (B,N,J) and every double block's K_i / V_i (B,H,N,128), rounded to bf16 as the library stores them;
  image_queries        q = norm_q_i(to_q_i(LayerNorm-modulated image rows)) of a block's INPUT rows, before RoPE;
  forward              the main model's evaluation with x_img += c * ip after double block i — `ip` depends on the block's input rows only, so a block with the
                       adapter is double_block(x) + c * ip(x_in) and the oracle needs no change — and the final layer as orc_flux_forward writes it;
  ip_loop              the denoise loop on it with tests/true_cfg_ref.py's combine / euler / blend, optionally with a ControlNet's samples (tests/controlnet_ref.py).

With c = 0 `forward` is oracle.Flux.forward (tests/test_host_ip_adapter.py holds it to 1e-5), which is what licenses the composition as a reference.
VARIANTS are the plumbing mistakes an IP-Adapter can make; the GPU test measures its result's distance to each of them on this same reference
(tests/test_gpu_ip_adapter.py) and the CPU self-test shows that they are far enough from the correct loop for that to mean something.

ip_attention_recipe is the kernel's recipe (csrc/ip_adapter.hip) in numpy, in float32 or float64: the op-level reference and the source of its bar."""
import functools

import numpy as np

from tests import controlnet_ref as CR
from tests import true_cfg_ref as R
from tests.util import SMALL_FLUX, bf16_round, flux_inputs

f32 = np.float32

VARIANTS = ("rotated_q", "unnormed_q", "norm_k_on_ip_keys", "through_out_proj", "into_txt_rows", "scale_dropped", "next_block_kv", "k_viewed_hn", "neg_uses_pos_embeds",
            "singles_too")

# the shared configuration of the IP-Adapter tests
MAIN_CFG = dict(SMALL_FLUX, num_layers=3)
B, T, E, N = 2, 32, 48, 4
GRIDS = {"aligned": (6, 4), "ragged": (5, 7)}
FUSED_GRID = {"fused": (8, 4)}  # 32 image rows: without an adapter the image stream's q|k|v projection takes the fused relayout epilogue at this shape
TS4 = [1.0, 0.8, 0.55, 0.3, 0.0]
# Chosen on the CPU oracle so that every variant lies at least 10 x the GPU loop bar (3e-2) from the correct loop (tests/test_host_ip_adapter.py lists the distances):
# the image prompt must weigh about as much as the stream it is added to (a dropped scale or a missing output projection must show through the final LayerNorm),
# the scores must be spread enough for the softmax to tell a rotated or un-normed q and foreign keys from the right ones, and the negative's embedding must differ
# from the prompt's.
IP_SCALE = 4.0     # the adapter scale of the tests
CFG_SCALE = 4.0    # the true-CFG scale of the cfg runs
PROJ_STD = 0.2     # synth.ip_adapter_state_dict_numpy's std of the image projection
K_STD = 0.25       # of to_k_ip
V_STD = 0.006     # of to_v_ip
NEG_MULT = 3.0     # the negative prompt's embeddings, times this (as tests/controlnet_ref.py)
IMG_MULT = 0.15    # the initial latents, times this
CN_SCALE = 1.0     # the ControlNet's conditioning scale in the combined case
CN_NET = "2+0"     # the ControlNet of the combined case: two double blocks on a main model of three (kd = 2)


def keep(n, start, end):
    """diffusers' keep over n steps, as control_guidance_start / _end"""
    return [0.0 if (i / n < start or (i + 1) / n > end) else 1.0 for i in range(n)]


# ---- the kernel's recipe in numpy (dtype float32: the recipe as the kernel states it; float64: the same formula without f32 roundings)
def ip_attention_recipe(q_raw, norm_q, K, V, x, c, dtype=np.float32):
    """q_raw (B,S,H,128), norm_q (128), K / V (B,H,N,128): bf16 values; x (B,S,H*128) f32; returns x + c * ip in `dtype`."""
    dt = np.dtype(dtype).type
    v = q_raw.astype(dtype)
    inv = dt(1.0) / np.sqrt((v * v).mean(-1, keepdims=True, dtype=dtype) + dt(1e-6))
    qn = v * inv * norm_q.astype(dtype)
    s = np.einsum("bshd,bhnd->bshn", qn, K.astype(dtype)) * dt(0.08838834764831845)
    e = np.exp(s - s.max(-1, keepdims=True))
    den = e.sum(-1, keepdims=True, dtype=dtype)
    ip = np.einsum("bshn,bhnd->bshd", e, V.astype(dtype)) * (dt(1.0) / den)
    ip = ip.reshape(x.shape).astype(dtype)
    return (x.astype(dtype) + (dt(c) * ip).astype(dtype)).astype(dtype)


# ---- the projection
def project(asd, cfg, embeds, variant=None):
    """([K_i], [V_i]) for the double blocks of cfg, each (B,H,N,128) f32 holding bf16 values; embeds (B,E)."""
    from oracle import oracle as orc
    J, H = cfg["joint_attention_dim"], cfg["num_attention_heads"]
    Bn = embeds.shape[0]
    raw = orc.linear(embeds, asd["image_proj.image_embeds.weight"], asd["image_proj.image_embeds.bias"]).reshape(-1, J)
    n = raw.shape[0] // Bn
    tok = orc.layer_norm(raw, asd["image_proj.norm.weight"], asd["image_proj.norm.bias"], 1e-5)
    Ks, Vs = [], []
    for i in range(cfg["num_layers"]):
        out = []
        for kv in ("to_k_ip", "to_v_ip"):
            a = bf16_round(orc.linear(tok, asd[f"ip_adapter.{i}.{kv}.weight"], asd.get(f"ip_adapter.{i}.{kv}.bias")))  # (B * n, D)
            if variant == "k_viewed_hn" and kv == "to_k_ip":
                out.append(np.ascontiguousarray(a.reshape(Bn, H, n, 128)))  # the wrong view: (H,N,128) of a (N,H,128) array
            else:
                out.append(np.ascontiguousarray(a.reshape(Bn, n, H, 128).transpose(0, 2, 1, 3)))
        Ks.append(out[0]), Vs.append(out[1])
    return Ks, Vs


def _modulated(orc, x, vec, w, b, D):
    """LayerNorm(eps 1e-6, no affine)(x) * (1 + scale) + shift with (shift, scale) the first two D-chunks of lin(silu(vec))"""
    mod = orc.linear(orc.silu(vec), w, b)
    return (orc.layer_norm(x, None, None, 1e-6) * (1 + mod[:, None, D:2 * D]) + mod[:, None, :D]).astype(np.float32)


def image_queries(sd, cfg, i, x_in, vec, pe_img=None, variant=None, single=False):
    """(B,S,H,128): the image rows' queries of double block i (single: single block i) on its input rows x_in (B,S,D)."""
    from oracle import oracle as orc
    H = cfg["num_attention_heads"]
    D = H * 128
    p = f"single_transformer_blocks.{i}." if single else f"transformer_blocks.{i}."
    n1 = p + ("norm.linear" if single else "norm1.linear")
    xm = _modulated(orc, x_in, vec, sd[n1 + ".weight"], sd[n1 + ".bias"], D)
    q = orc.linear(xm, sd[p + "attn.to_q.weight"], sd[p + "attn.to_q.bias"]).reshape(x_in.shape[0], x_in.shape[1], H, 128)
    if variant != "unnormed_q":
        q = orc.rms_norm_slow(q, sd[p + "attn.norm_q.weight"], 1e-6)
    if variant == "rotated_q":
        q = np.stack([orc.apply_rope(np.ascontiguousarray(q[b].transpose(1, 0, 2)), pe_img[b]).transpose(1, 0, 2) for b in range(q.shape[0])])
    return np.ascontiguousarray(q, np.float32)


def ip_attention(q, K, V):
    """softmax(q K^T / sqrt(128)) V per sample and head: q (B,S,H,128), K / V (B,H,N,128) -> (B,S,H*128)"""
    from oracle import oracle as orc
    s = (np.einsum("bshd,bhnd->bshn", q, K) * f32(1.0 / np.sqrt(128.0))).astype(np.float32)
    p = orc.softmax_last_dim(s)
    return np.ascontiguousarray(np.einsum("bshn,bhnd->bshd", p, V).reshape(q.shape[0], q.shape[1], -1), np.float32)


def forward(om, sd, cfg, x, ids, txt, txt_ids, t, y, g, Ks=(), Vs=(), c=0.0, variant=None, ds=(), ss=(), cn_c=1.0):
    """One evaluation of the main model `om` (an oracle.Flux holding sd) with the adapter's K / V at scale c; c == 0 (or no K / V): the plain forward.  ds / ss / cn_c:
    a ControlNet's samples, injected after the image prompt as tests/controlnet_ref.py does."""
    from oracle import oracle as orc
    H = cfg["num_attention_heads"]
    D = H * 128
    nd = cfg["num_layers"]
    Tn, S = txt.shape[1], x.shape[1]
    on = len(Ks) > 0 and c != 0
    c = f32(1.0 if variant == "scale_dropped" else c)
    dmap, smap = CR.index_map(nd, len(ds)), CR.index_map(cfg["num_single_layers"], len(ss))
    xi = orc.linear(x, sd["x_embedder.weight"], sd["x_embedder.bias"])
    xt = orc.linear(txt, sd["context_embedder.weight"], sd["context_embedder.bias"])
    vec = CR._vec(orc, sd, cfg, t, y, g)
    pe = orc.rope_table(np.concatenate([txt_ids, ids], 1), cfg["axes_dim"], cfg["theta"])
    for i in range(nd):
        ip = None
        if on:
            k = (i + 1) % nd if variant == "next_block_kv" else i
            Ki = Ks[k]
            if variant == "norm_k_on_ip_keys":
                Ki = orc.rms_norm_slow(Ki, sd[f"transformer_blocks.{i}.attn.norm_k.weight"], 1e-6)
            ip = ip_attention(image_queries(sd, cfg, i, xi, vec, pe[:, Tn:], variant), Ki, Vs[k])
            if variant == "through_out_proj":
                ip = orc.linear(ip, sd[f"transformer_blocks.{i}.attn.to_out.0.weight"], sd[f"transformer_blocks.{i}.attn.to_out.0.bias"])
        xi, xt = om.double_block(i, xi, xt, vec, pe)
        if ip is not None:
            if variant == "into_txt_rows":  # the result lands in the text stream's leading rows
                r = min(S, Tn)
                xt[:, :r] = (xt[:, :r] + c * ip[:, :r]).astype(np.float32)
            else:
                xi = (xi + c * ip).astype(np.float32)
        if dmap:
            xi = (xi + f32(cn_c) * ds[dmap[i]]).astype(np.float32)
    xx = np.concatenate([xt, xi], 1)
    for j in range(cfg["num_single_layers"]):
        ip = None
        if on and variant == "singles_too":
            ip = ip_attention(image_queries(sd, cfg, j, np.ascontiguousarray(xx[:, Tn:]), vec, None, None, single=True), Ks[j % nd], Vs[j % nd])
        xx = om.single_block(j, xx, vec, pe)
        if ip is not None:
            xx[:, Tn:] = (xx[:, Tn:] + c * ip).astype(np.float32)
        if smap:
            xx[:, Tn:] = (xx[:, Tn:] + f32(cn_c) * ss[smap[j]]).astype(np.float32)
    mod = orc.linear(orc.silu(vec), sd["norm_out.linear.weight"], sd["norm_out.linear.bias"])
    xn = orc.layer_norm(np.ascontiguousarray(xx[:, Tn:]), None, None, 1e-6) * (1 + mod[:, None, :D]) + mod[:, None, D:]
    return orc.linear(xn.astype(np.float32), sd["proj_out.weight"], sd["proj_out.bias"])


def ip_loop(om, sd, cfg, asd, x, ids, txt, txt_ids, y, g, ts, embeds, c=1.0, step_scales=None, neg_txt=None, neg_y=None, neg_embeds=None, scale=None, x0=None,
            noise=None, mask=None, variant=None, cn=None):
    """The final latents (B,S,C) f32 of the composed loop over the schedule `ts` (len n + 1).  The projection runs once.  Step i adds the image prompt at
    c * step_scales[i]; a step whose scale is 0 is the plain evaluation.  neg_txt / neg_y / scale: true CFG — the negative half attends to neg_embeds, or to zero
    embeddings through the same projection.  x0 / noise / mask: the inpainting blend after every step.  cn: dict(on=, nsd=, ncfg=, cond=, c=) — a ControlNet
    evaluated at every step (for the negative too), its samples injected after the image prompt.  variant: None for the correct loop, or one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    x = np.ascontiguousarray(x, np.float32).copy()
    Ks, Vs = project(asd, cfg, embeds, variant)
    if neg_txt is not None:
        ne = embeds if variant == "neg_uses_pos_embeds" else (np.zeros_like(embeds) if neg_embeds is None else neg_embeds)
        nKs, nVs = project(asd, cfg, ne, variant)
    for i in range(len(ts) - 1):
        t = np.full(x.shape[0], f32(ts[i]), np.float32)
        ci = f32(c) * f32(1.0 if step_scales is None else step_scales[i])

        def ev(txt_, y_, K_, V_):
            kw = {}
            if cn is not None:
                ds, ss = CR.controlnet_samples(cn["on"], cn["nsd"], cn["ncfg"], x, cn["cond"], ids, txt_, txt_ids, t, y_, g)
                kw = dict(ds=ds, ss=ss, cn_c=cn["c"])
            return forward(om, sd, cfg, x, ids, txt_, txt_ids, t, y_, g, K_, V_, ci, variant, **kw)

        gd = ev(txt, y, Ks, Vs)
        if neg_txt is not None:
            gd = R.combine(gd, ev(neg_txt, neg_y, nKs, nVs), scale)
        x = R.euler(x, gd, f32(ts[i + 1] - ts[i]))
        if mask is not None:
            x = R.blend(x, x0, noise, mask, ts[i + 1])
    return x


# ---- shared, read-only fixtures
@functools.lru_cache(maxsize=None)
def main_state_dict():
    import diffusion_rs_amd as d
    return d.synth.flux_state_dict_numpy(MAIN_CFG, seed=0)


@functools.lru_cache(maxsize=None)
def adapter_state_dict():
    import diffusion_rs_amd as d
    return d.synth.ip_adapter_state_dict_numpy(MAIN_CFG, E, N, seed=5, proj_std=PROJ_STD, k_std=K_STD, v_std=V_STD)


@functools.lru_cache(maxsize=None)
def main_oracle():
    from oracle import oracle as orc
    om = orc.Flux(MAIN_CFG)
    om.load(main_state_dict())
    return om


@functools.lru_cache(maxsize=None)
def inputs(grid):
    hw = dict(GRIDS, **FUSED_GRID)[grid]
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, hw, T, seed=61)
    _, _, ntxt, _, ny = flux_inputs(SMALL_FLUX, B, hw, T, seed=63)
    ntxt, ny = bf16_round(ntxt * f32(NEG_MULT)), (ny * f32(NEG_MULT)).astype(np.float32)
    img = (img * f32(IMG_MULT)).astype(np.float32)
    rng = np.random.default_rng(65)
    emb = rng.standard_normal((B, E)).astype(np.float32)
    nemb = rng.standard_normal((B, E)).astype(np.float32)
    cond = rng.standard_normal(img.shape).astype(np.float32)
    x0 = (rng.standard_normal(img.shape) * IMG_MULT).astype(np.float32)
    mask = rng.random(img.shape).astype(np.float32)
    mask[rng.random(img.shape) < 0.05] = 0.0
    mask[rng.random(img.shape) < 0.7] = 1.0
    s = dict(S=hw[0] * hw[1], img=img, ids=ids, txt=txt, txt_ids=txt_ids, y=y, ntxt=ntxt, ny=ny, emb=emb, nemb=nemb, cond=cond, x0=x0, mask=mask,
             g=np.full(B, 3.5, np.float32))
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


STEP_SCALES = (1.0, 1.5, 0.0, 1.25)  # the "steps" mode: a plain step in the middle, and scales that are not 1
MODES = ("plain", "cfg", "cfg_neg", "steps", "blend", "controlnet")


def mode_kwargs(mode, s):
    """ip_loop's keywords of a mode: "plain"; "cfg" (a negative prompt, zero negative embeddings); "cfg_neg" (negative embeddings given); "steps" (STEP_SCALES);
    "blend" (inpainting); "controlnet" (the ControlNet CN_NET of tests/controlnet_ref.py next to it)."""
    if mode == "cfg":
        return dict(neg_txt=s["ntxt"], neg_y=s["ny"], scale=CFG_SCALE)
    if mode == "cfg_neg":
        return dict(neg_txt=s["ntxt"], neg_y=s["ny"], scale=CFG_SCALE, neg_embeds=s["nemb"])
    if mode == "steps":
        return dict(step_scales=STEP_SCALES)
    if mode == "blend":
        return dict(x0=s["x0"], noise=s["img"], mask=s["mask"])
    if mode == "controlnet":
        return dict(cn=dict(on=CR.net_oracle(CN_NET), nsd=CR.net_state_dict(CN_NET), ncfg=CR.net_cfg(CN_NET), cond=s["cond"], c=CN_SCALE))
    return {}


@functools.lru_cache(maxsize=None)
def loop_reference(grid, mode, variant=None):
    """The 4-step composed loop of one grid and mode, computed once and shared (read-only)."""
    s = inputs(grid)
    out = ip_loop(main_oracle(), main_state_dict(), MAIN_CFG, adapter_state_dict(), s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], TS4, s["emb"], c=IP_SCALE,
                  variant=variant, **mode_kwargs(mode, s))
    out.setflags(write=False)
    return out
