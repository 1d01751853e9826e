"""The FLUX ControlNet composed on the CPU oracle's op-level functions and block hooks, in f32:

  controlnet_samples   the ControlNet's evaluation — x = x_embedder(img) + controlnet_x_embedder(cond), its blocks through oracle.Flux.double_block /
                       single_block of an oracle.Flux built with the NET's block counts, one Linear(D, D) per block on the image rows;
  forward              the main model's evaluation with x_img += c * d[i // ceil(ND / nd)] after double block i and xs[:, T:] += c * s[j // ceil(NS / ns)] after
                       single block j, and the final layer as orc_flux_forward writes it;
  controlnet_loop      the denoise loop on them with tests/true_cfg_ref.py's combine / euler / blend.

With every sample zero `forward` is oracle.Flux.forward (tests/test_host_controlnet.py holds it to 1e-5), which is what licenses the composition as a reference.
VARIANTS are the plumbing mistakes a ControlNet loop can make; the GPU test measures its result's distance to each of them on this same reference
(tests/test_gpu_controlnet.py) and the CPU self-test shows that they are far enough from the correct loop for that to mean something."""
import functools

import numpy as np

from tests import true_cfg_ref as R
from tests.util import SMALL_FLUX, bf16_round, flux_inputs

f32 = np.float32

VARIANTS = ("index_floor", "single_into_txt_rows", "samples_swapped", "scale_dropped", "cond_zeroed", "neg_uses_pos_text")

# the shared configuration of the ControlNet tests
MAIN_CFG = dict(SMALL_FLUX, num_layers=5, num_single_layers=3)
NETS = {"2+2": (2, 2), "2+0": (2, 0)}  # nd + ns: kd = ceil(5 / 2) = 3, ks = ceil(3 / 2) = 2 — both ceilings bite; and a net without single blocks
B, T = 2, 32
GRIDS = {"aligned": (6, 4), "ragged": (5, 7)}
TS4 = [1.0, 0.8, 0.55, 0.3, 0.0]
# Chosen on the CPU oracle so that every variant lies at least 9e-2 from the correct loop (tests/test_host_controlnet.py lists the distances).  The samples must
# neither drown the main stream (the final LayerNorm would hide a dropped scale) nor vanish in it; the ControlNet must depend on its text strongly enough for the
# negative's text to be told from the prompt's — hence the std of its modulation linears and a negative prompt three times the prompt's magnitude.
CN_SCALE = 4.0      # the conditioning scale of the loop tests
CFG_SCALE = 4.0     # the true-CFG scale of the cfg runs
CN_STD = 0.008      # synth.controlnet_state_dict_numpy's std of the controlnet_* weights
CN_X_STD = 0.05     # of controlnet_x_embedder's
NET_MOD_STD = 0.5   # and of the net's modulation linears
NEG_MULT = 3.0      # the negative prompt's embeddings, times this


def net_cfg(name):
    nd, ns = NETS[name]
    return dict(SMALL_FLUX, num_layers=nd, num_single_layers=ns)


def index_map(n_main, n_net, floor=False):
    """which of the net's n_net samples each of the main model's n_main blocks takes: i // ceil(n_main / n_net); floor=True: the wrong i // floor(n_main / n_net).
    (The other floor one may write, i * n_net // n_main, IS the correct map at the shapes of these tests — (5,2), (3,2), and at FLUX.1-dev's (19,5) — so it could
    not be told from it; it differs at (38,10).  tests/test_host_controlnet.py asserts both facts.)"""
    if n_net == 0:
        return []
    if floor:  # the interval floored instead of ceiled (and the index kept in range)
        return [min(i // max(n_main // n_net, 1), n_net - 1) for i in range(n_main)]
    k = -(-n_main // n_net)
    return [i // k for i in range(n_main)]


def keep(n, start, end):
    """diffusers' controlnet_keep over n steps"""
    return [0.0 if (i / n < start or (i + 1) / n > end) else 1.0 for i in range(n)]


def _emb(orc, sd, p, v):
    h = orc.silu(orc.linear(v, sd[p + ".linear_1.weight"], sd[p + ".linear_1.bias"]))
    return orc.linear(h, sd[p + ".linear_2.weight"], sd[p + ".linear_2.bias"])


def _vec(orc, sd, cfg, t, y, g):
    v = _emb(orc, sd, "time_text_embed.timestep_embedder", orc.timestep_embedding(t))
    if cfg["guidance_embeds"]:
        v = v + _emb(orc, sd, "time_text_embed.guidance_embedder", orc.timestep_embedding(g))
    return (v + _emb(orc, sd, "time_text_embed.text_embedder", y)).astype(np.float32)


def controlnet_samples(on, nsd, ncfg, x, cond, ids, txt, txt_ids, t, y, g):
    """(double samples [nd x (B,S,D)], single samples [ns x (B,S,D)]) of the ControlNet `on` (an oracle.Flux of the net's block counts holding nsd's block weights)"""
    from oracle import oracle as orc
    Tn = txt.shape[1]
    xi = (orc.linear(x, nsd["x_embedder.weight"], nsd["x_embedder.bias"]) + orc.linear(cond, nsd["controlnet_x_embedder.weight"], nsd["controlnet_x_embedder.bias"])).astype(np.float32)
    xt = orc.linear(txt, nsd["context_embedder.weight"], nsd["context_embedder.bias"])
    vec = _vec(orc, nsd, ncfg, t, y, g)
    pe = orc.rope_table(np.concatenate([txt_ids, ids], 1), ncfg["axes_dim"], ncfg["theta"])
    ds, ss = [], []
    for i in range(ncfg["num_layers"]):
        xi, xt = on.double_block(i, xi, xt, vec, pe)
        ds.append(orc.linear(xi, nsd[f"controlnet_blocks.{i}.weight"], nsd[f"controlnet_blocks.{i}.bias"]))
    xx = np.concatenate([xt, xi], 1)
    for j in range(ncfg["num_single_layers"]):
        xx = on.single_block(j, xx, vec, pe)
        ss.append(orc.linear(np.ascontiguousarray(xx[:, Tn:]), nsd[f"controlnet_single_blocks.{j}.weight"], nsd[f"controlnet_single_blocks.{j}.bias"]))
    return ds, ss


def forward(om, sd, cfg, x, ids, txt, txt_ids, t, y, g, ds=(), ss=(), c=1.0, variant=None):
    """One evaluation of the main model `om` (an oracle.Flux holding sd) with the samples ds / ss injected at scale c; no samples: the plain forward."""
    from oracle import oracle as orc
    D = cfg["num_attention_heads"] * 128
    Tn, S = txt.shape[1], x.shape[1]
    c = f32(1.0 if variant == "scale_dropped" else c)
    floor = variant == "index_floor"
    dmap, smap = index_map(cfg["num_layers"], len(ds), floor), index_map(cfg["num_single_layers"], len(ss), floor)
    xi = orc.linear(x, sd["x_embedder.weight"], sd["x_embedder.bias"])
    xt = orc.linear(txt, sd["context_embedder.weight"], sd["context_embedder.bias"])
    vec = _vec(orc, sd, cfg, t, y, g)
    pe = orc.rope_table(np.concatenate([txt_ids, ids], 1), cfg["axes_dim"], cfg["theta"])
    for i in range(cfg["num_layers"]):
        xi, xt = om.double_block(i, xi, xt, vec, pe)
        if dmap:
            xi = (xi + c * ds[dmap[i]]).astype(np.float32)
    xx = np.concatenate([xt, xi], 1)
    for j in range(cfg["num_single_layers"]):
        xx = om.single_block(j, xx, vec, pe)
        if smap:
            r0 = 0 if variant == "single_into_txt_rows" else Tn
            xx[:, r0:r0 + S] = (xx[:, r0:r0 + S] + c * ss[smap[j]]).astype(np.float32)
    mod = orc.linear(orc.silu(vec), sd["norm_out.linear.weight"], sd["norm_out.linear.bias"])
    xn = orc.layer_norm(np.ascontiguousarray(xx[:, Tn:]), None, None, 1e-6) * (1 + mod[:, None, :D]) + mod[:, None, D:]
    return orc.linear(xn.astype(np.float32), sd["proj_out.weight"], sd["proj_out.bias"])


def conditioned_forward(om, sd, cfg, on, nsd, ncfg, x, cond, ids, txt, txt_ids, t, y, g, c, variant=None):
    """The ControlNet on (x, cond), then the main model with its samples."""
    if variant == "cond_zeroed":
        cond = np.zeros_like(cond)
    ds, ss = controlnet_samples(on, nsd, ncfg, x, cond, ids, txt, txt_ids, t, y, g)
    if variant == "samples_swapped":
        ds, ss = [np.ascontiguousarray(a[::-1]) for a in ds], [np.ascontiguousarray(a[::-1]) for a in ss]
    return forward(om, sd, cfg, x, ids, txt, txt_ids, t, y, g, ds, ss, c, variant)


def controlnet_loop(om, sd, cfg, on, nsd, ncfg, x, cond, ids, txt, txt_ids, y, g, ts, c=1.0, step_scales=None, neg_txt=None, neg_y=None, scale=None, x0=None,
                    noise=None, mask=None, variant=None):
    """The final latents (B,S,C) f32 of the composed loop over the schedule `ts` (len n + 1).  Step i injects at c * step_scales[i]; a step whose scale is 0 is
    the plain evaluation.  neg_txt / neg_y / scale: true CFG — the ControlNet is evaluated for the negative as well, on the negative's txt / y and the same
    state and cond.  x0 / noise / mask: the inpainting blend after every step.  variant: None for the correct loop, or one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    x = np.ascontiguousarray(x, np.float32).copy()
    for i in range(len(ts) - 1):
        t = np.full(x.shape[0], f32(ts[i]), np.float32)
        ci = f32(c) * f32(1.0 if step_scales is None else step_scales[i])

        def ev(txt_, y_, cn_txt, cn_y):
            if ci == 0:
                return forward(om, sd, cfg, x, ids, txt_, txt_ids, t, y_, g)
            if variant == "cond_zeroed":
                cnd = np.zeros_like(cond)
            else:
                cnd = cond
            ds, ss = controlnet_samples(on, nsd, ncfg, x, cnd, ids, cn_txt, txt_ids, t, cn_y, g)
            if variant == "samples_swapped":
                ds, ss = [np.ascontiguousarray(a[::-1]) for a in ds], [np.ascontiguousarray(a[::-1]) for a in ss]
            return forward(om, sd, cfg, x, ids, txt_, txt_ids, t, y_, g, ds, ss, ci, variant)

        gd = ev(txt, y, txt, y)
        if neg_txt is not None:
            neg = ev(neg_txt, neg_y, txt, y) if variant == "neg_uses_pos_text" else ev(neg_txt, neg_y, neg_txt, neg_y)
            gd = R.combine(gd, neg, scale)
        x = R.euler(x, gd, f32(ts[i + 1] - ts[i]))
        if mask is not None:
            x = R.blend(x, x0, noise, mask, ts[i + 1])
    return x


# ---- the injection kernel in numpy: one rounded product, one rounded sum
def add_scaled_rows(x, src_bf16_as_f32, scale):
    return (x + (f32(scale) * src_bf16_as_f32).astype(np.float32)).astype(np.float32)


# ---- shared, read-only fixtures
@functools.lru_cache(maxsize=None)
def main_state_dict():
    import diffusion_rs_amd as d
    return d.synth.flux_state_dict_numpy(MAIN_CFG, seed=0)


@functools.lru_cache(maxsize=None)
def net_state_dict(name):
    import diffusion_rs_amd as d
    return d.synth.controlnet_state_dict_numpy(net_cfg(name), seed=3, cn_std=CN_STD, cn_x_std=CN_X_STD, mod_std=NET_MOD_STD)


@functools.lru_cache(maxsize=None)
def main_oracle():
    from oracle import oracle as orc
    om = orc.Flux(MAIN_CFG)
    om.load(main_state_dict())
    return om


@functools.lru_cache(maxsize=None)
def net_oracle(name):
    """an oracle.Flux of the net's block counts: only its block hooks are used (it has no norm_out / proj_out, and the controlnet_* tensors stay in numpy)"""
    from oracle import oracle as orc
    on = orc.Flux(net_cfg(name))
    on.load({k: v for k, v in net_state_dict(name).items() if not k.startswith("controlnet_")})
    return on


@functools.lru_cache(maxsize=None)
def inputs(grid):
    hw = GRIDS[grid]
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, hw, T, seed=51)
    _, _, ntxt, _, ny = flux_inputs(SMALL_FLUX, B, hw, T, seed=53)
    ntxt, ny = bf16_round(ntxt * f32(NEG_MULT)), (ny * f32(NEG_MULT)).astype(np.float32)
    rng = np.random.default_rng(55)
    cond = rng.standard_normal(img.shape).astype(np.float32)
    x0 = rng.standard_normal(img.shape).astype(np.float32)
    mask = rng.random(img.shape).astype(np.float32)
    mask[rng.random(img.shape) < 0.05] = 0.0  # mixed: kept elements (0), repainted ones (1) and soft ones in between
    mask[rng.random(img.shape) < 0.7] = 1.0
    s = dict(S=hw[0] * hw[1], img=img, ids=ids, txt=txt, txt_ids=txt_ids, y=y, ntxt=ntxt, ny=ny, cond=cond, x0=x0, mask=mask, g=np.full(B, 3.5, np.float32))
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def loop_reference(net, grid, mode, variant=None):
    """The 4-step composed loop of one net and grid, computed once and shared (read-only).  mode: "plain", "cfg" (negative prompt at CFG_SCALE) or "blend"."""
    s = inputs(grid)
    kw = {}
    if mode == "cfg":
        kw = dict(neg_txt=s["ntxt"], neg_y=s["ny"], scale=CFG_SCALE)
    elif mode == "blend":
        kw = dict(x0=s["x0"], noise=s["img"], mask=s["mask"])
    out = controlnet_loop(main_oracle(), main_state_dict(), MAIN_CFG, net_oracle(net), net_state_dict(net), net_cfg(net), s["img"], s["cond"], s["ids"], s["txt"],
                          s["txt_ids"], s["y"], s["g"], TS4, c=CN_SCALE, variant=variant, **kw)
    out.setflags(write=False)
    return out
