"""The second-order solvers of the denoise loop composed on a model evaluation in numpy, in the library's expressions.  Flow matching:
sigma = t, alpha = 1 - t; g is the prediction, or under a negative prompt tests/true_cfg_ref.py's combine(pos, neg, scale).

    euler      x = x + g * dt
    heun       g1 = g(x, t_i);  xp = blend(x + g1 * dt);  t_{i+1} == 0: x = xp — else g2 = g(xp, t_{i+1}),  x = blend(x + ((g1 + g2) * 0.5) * dt)
    dpmpp_2m   D = x - t_i * g;  D' = D + w * (D - hist) (w == 0: D' = D);  x = blend(a * x + c * D');  hist = D          (a, c, w: coefficients())

`solve` takes the model as a callable evaluate(x, t, i) -> (pos, neg or None) — t the time of the evaluation, i the step it belongs to — so the same loops run on
the CPU oracle (oracle_eval), on its ControlNet and step-cache compositions, and on an analytic field (the order-of-convergence test, in float64).  Every product
and sum is rounded to `dtype` on its own; the library fuses each product into the following sum, which moves a value by an ulp.

VARIANTS are the plumbing mistakes a solver loop can make; the GPU test measures its result's distance to each of them on this same reference
(tests/test_gpu_solvers.py), and the CPU self-test (tests/test_host_solvers.py) shows they are far enough from the correct loop for that to mean something."""
import functools
import math

import numpy as np

from tests import true_cfg_ref as R
from tests.util import SMALL_FLUX, bf16_round, flux_inputs

f32 = np.float32

SOLVERS = ("heun", "dpmpp_2m")
VARIANTS = ("euler", "heun_second_eval_at_t_i", "heun_second_eval_on_x", "heun_no_euler_last", "heun_predictor_unblended", "dpmpp_no_history", "dpmpp_history_is_Dprime",
            "dpmpp_history_from_pos_only")


def variants_for(solver, cfg=False, mask=False, ends_at_zero=True):
    """the VARIANTS that are another loop than the correct one for this solver and these options: "euler" (the solver ignored) always, the solver's own, and of
    those heun_predictor_unblended only under a mask, heun_no_euler_last only on a schedule that ends at 0, dpmpp_history_from_pos_only only under CFG"""
    out = ["euler"]
    for v in VARIANTS[1:]:
        if not v.startswith(solver.split("_")[0]):
            continue
        if (v == "heun_predictor_unblended" and not mask) or (v == "heun_no_euler_last" and not ends_at_zero) or (v == "dpmpp_history_from_pos_only" and not cfg):
            continue
        out.append(v)
    return out


def check_schedule(ts):
    return len(ts) >= 1 and ts[0] <= 1.0 and ts[-1] >= 0.0 and all(b < a for a, b in zip(ts, ts[1:]))


def coefficients(ts, i):
    """(a, c, w) of 2M's step i in Python floats (f64): a = t_{i+1} / t_i, c = 1 - a, w = (l_{i+1} - l_i) / (2 (l_i - l_{i-1})) with l = ln((1 - t) / t);
    w = 0 at i == 0, after t_{i-1} == 1 (l = -inf: the limit) and into t_{i+1} == 0 (the last step is first order)"""
    t0, t1 = float(ts[i]), float(ts[i + 1])
    a = t1 / t0
    w = 0.0
    if i > 0 and float(ts[i - 1]) != 1.0 and t1 != 0.0:
        lam = lambda t: math.log((1.0 - t) / t)
        w = (lam(t1) - lam(t0)) / (2.0 * (lam(t0) - lam(float(ts[i - 1]))))
    return a, 1.0 - a, w


def _blend(e, x0, noise, mask, s, dtype):
    if mask is None:
        return e
    if dtype == np.float32:
        return R.blend(e, x0, noise, mask, s)
    return mask * e + (1 - mask) * ((1 - s) * x0 + s * noise)


def solve(evaluate, x, ts, solver, scale=None, x0=None, noise=None, mask=None, variant=None, dtype=np.float32, force_w0=False):
    """The final state of the loop over the schedule ts (len n + 1).  solver: "euler" | "heun" | "dpmpp_2m".  scale: the true-CFG scale when evaluate returns a
    negative's prediction.  x0 / noise / mask: the inpainting blend at every step's target time.  variant: None or one of VARIANTS.  force_w0: 2M with every w = 0
    (in exact arithmetic the Euler loop)."""
    assert solver in ("euler",) + SOLVERS and (variant is None or variant in VARIANTS)
    T = dtype
    x = np.array(x, dtype)
    if variant == "euler":
        solver = "euler"

    def g_of(state, t, i):
        pos, neg = evaluate(state, t, i)
        pos = np.asarray(pos, T)
        if neg is None:
            return pos, pos
        neg = np.asarray(neg, T)
        return (R.combine(pos, neg, scale) if T == np.float32 else neg + scale * (pos - neg)), pos

    hist = None
    for i in range(len(ts) - 1):
        t0, t1 = ts[i], ts[i + 1]
        dt = T(t1 - t0)
        g, pos = g_of(x, t0, i)
        if solver == "euler":
            x = _blend((x + (g * dt).astype(T)).astype(T), x0, noise, mask, t1, T)
        elif solver == "heun":
            e = (x + (g * dt).astype(T)).astype(T)
            xp = e if variant == "heun_predictor_unblended" else _blend(e, x0, noise, mask, t1, T)
            if t1 == 0.0 and variant != "heun_no_euler_last":
                x = _blend(e, x0, noise, mask, t1, T)
                continue
            g2, _ = g_of(x if variant == "heun_second_eval_on_x" else xp, t0 if variant == "heun_second_eval_at_t_i" else t1, i)
            h = ((g + g2).astype(T) * T(0.5)).astype(T)
            x = _blend((x + (h * dt).astype(T)).astype(T), x0, noise, mask, t1, T)
        else:
            a, c, w = (T(v) for v in coefficients(ts, i))
            if force_w0 or variant == "dpmpp_no_history":
                w = T(0)
            D = (x - (T(t0) * g).astype(T)).astype(T)
            Dp = D if w == 0 else (D + (w * (D - hist).astype(T)).astype(T)).astype(T)
            hist = Dp if variant == "dpmpp_history_is_Dprime" else D
            if variant == "dpmpp_history_from_pos_only":  # the data prediction of the prompt's half alone goes into the history
                hist = (x - (T(t0) * pos).astype(T)).astype(T)
            x = _blend(((a * x).astype(T) + (c * Dp).astype(T)).astype(T), x0, noise, mask, t1, T)
    return x


# ---- evaluations
def oracle_eval(om, ids, txt, txt_ids, y, g, neg_txt=None, neg_y=None, ctx=None, rids=None):
    """evaluate(x, t, i) on the CPU oracle: the prompt's prediction and — with a negative — the negative's, on the same state, ids, guidance and context rows"""
    def evaluate(x, t, i):
        tv = np.full(x.shape[0], f32(t), np.float32)
        pos = R._forward(om, x, ids, txt, txt_ids, tv, y, g, ctx, rids)
        neg = None if neg_txt is None else R._forward(om, x, ids, neg_txt, txt_ids, tv, neg_y, g, ctx, rids)
        return pos, neg
    return evaluate


CN_CFG = dict(SMALL_FLUX, num_layers=1, num_single_layers=1)  # the 1 + 1-block ControlNet of the solver tests: every block of the main model takes its one sample
CN_SCALE = 4.0
CN_STEP_SCALES = [1.0, 0.5, 0.0, 1.0]  # (a step whose scale is 0 is the plain step, at both of Heun's evaluations)


@functools.lru_cache(maxsize=None)
def controlnet_state_dict():
    import diffusion_rs_amd as d
    from tests import controlnet_ref as CR
    return d.synth.controlnet_state_dict_numpy(CN_CFG, seed=3, cn_std=CR.CN_STD, cn_x_std=CR.CN_X_STD, mod_std=CR.NET_MOD_STD)


@functools.lru_cache(maxsize=None)
def controlnet_oracle():
    from oracle import oracle as orc
    on = orc.Flux(CN_CFG)
    on.load({k: v for k, v in controlnet_state_dict().items() if not k.startswith("controlnet_")})
    return on


def controlnet_eval(s, cond, c=CN_SCALE, step_scales=CN_STEP_SCALES):
    """evaluate on tests/controlnet_ref.py's composition: the ControlNet on the evaluation's own state and time, injected at step i's scale into the main model"""
    from tests import controlnet_ref as CR
    om, sd, on, nsd = oracle_model(), state_dict(), controlnet_oracle(), controlnet_state_dict()

    def evaluate(x, t, i):
        tv = np.full(x.shape[0], f32(t), np.float32)
        ci = f32(c) * f32(1.0 if step_scales is None else step_scales[i])
        if ci == 0:
            return CR.forward(om, sd, SMALL_FLUX, x, s["ids"], s["txt"], s["txt_ids"], tv, s["y"], s["g"]), None
        return CR.conditioned_forward(om, sd, SMALL_FLUX, on, nsd, CN_CFG, x, cond, s["ids"], s["txt"], s["txt_ids"], tv, s["y"], s["g"], ci), None
    return evaluate


def step_cache_eval(om, sd, cfg, ids, txt, txt_ids, y, g, force):
    """evaluate with the first-block step cache under a forced mask, tests/step_cache_ref.py's semantics one evaluation at a time: step i reuses the cached
    output residual of the blocks after double block 0 when force[i] == 1, else runs them and refreshes it"""
    from oracle import oracle as orc
    D = cfg["num_attention_heads"] * 128
    Tn = txt.shape[1]

    def emb(p, v):
        h = orc.silu(orc.linear(v, sd[p + ".linear_1.weight"], sd[p + ".linear_1.bias"]))
        return orc.linear(h, sd[p + ".linear_2.weight"], sd[p + ".linear_2.bias"])

    pe = orc.rope_table(np.concatenate([txt_ids, ids], 1), cfg["axes_dim"], cfg["theta"])
    x_txt0 = orc.linear(txt, sd["context_embedder.weight"], sd["context_embedder.bias"])
    static = emb("time_text_embed.guidance_embedder", orc.timestep_embedding(g)) + emb("time_text_embed.text_embedder", y)
    state = {}

    def evaluate(x, t, i):
        S = x.shape[1]
        tv = np.full(x.shape[0], f32(t), np.float32)
        vec = emb("time_text_embed.timestep_embedder", orc.timestep_embedding(tv)) + static
        X0 = orc.linear(x, sd["x_embedder.weight"], sd["x_embedder.bias"])
        X1, xt = om.double_block(0, X0, x_txt0, vec, pe)
        if force[i] == 1:
            XF = (X1 + state["delta"]).astype(np.float32)
        else:
            xi = X1
            for k in range(1, cfg["num_layers"]):
                xi, xt = om.double_block(k, xi, xt, vec, pe)
            xx = np.concatenate([xt, xi], 1)
            for k in range(cfg["num_single_layers"]):
                xx = om.single_block(k, xx, vec, pe)
            XF = xx[:, Tn:]
            state["delta"] = (XF - X1).astype(np.float32)
        ss = orc.linear(orc.silu(vec), sd["norm_out.linear.weight"], sd["norm_out.linear.bias"])
        xn = orc.layer_norm(np.ascontiguousarray(XF[:, :S]), None, None, 1e-6) * (1 + ss[:, None, :D]) + ss[:, None, D:]
        return orc.linear(xn.astype(np.float32), sd["proj_out.weight"], sd["proj_out.bias"]), None
    return evaluate


# ---- the analytic field of the order-of-convergence test (the oracle is not involved; float64)
def field(x, t):
    return np.cos(3.0 * t) * x + 0.5 * np.sin(2.0 * x) - 0.3


def field_eval(x, t, i):
    return field(x, t), None


def rk4(x, t_from, t_to, n=4096):
    x = np.array(x, np.float64)
    h = (t_to - t_from) / n
    for k in range(n):
        t = t_from + k * h
        k1 = field(x, t)
        k2 = field(x + 0.5 * h * k1, t + 0.5 * h)
        k3 = field(x + 0.5 * h * k2, t + 0.5 * h)
        k4 = field(x + h * k3, t + h)
        x = x + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


# ---- the shared configuration of the solver tests: SMALL_FLUX, Philox weights of seed 0, B = 2, T = 32, the two grids of the Kontext / true-CFG tests
B, T = 2, 32
SHAPES = {"ragged": ((4, 6), (5, 7)), "aligned": ((8, 8), (6, 8))}
TS4 = [1.0, 0.8, 0.55, 0.3, 0.0]        # 2M: first order at steps 0, 1 (t_0 == 1) and 3 (into 0), history at step 2; Heun: 7 evaluations
TS_CUT = [0.9, 0.7, 0.5, 0.3, 0.1]      # a schedule cut at both ends, as image to image starts one: 2M's history from step 1 on; Heun: 8 evaluations
SCHEDULES = {"full": TS4, "cut": TS_CUT}
# which schedule the comparisons against the oracle run a solver on: Heun the one that ends at 0 (its last step is Euler's: heun_no_euler_last is another loop),
# 2M the cut one (on the full one its history is read once, after a first-order step, and dpmpp_history_is_Dprime IS the correct loop)
SOLVER_SCHEDULE = {"heun": "full", "dpmpp_2m": "cut"}
SCALE = 2.0     # the true-CFG scale of the cfg case
NEG_MULT = 3.0  # the negative prompt's embeddings, times this (tests/controlnet_ref.py's device: a negative the model can tell from the prompt)
CACHE_FORCE = [0, 1, 0, 1]
# What bf16 evaluations resolve at these shapes, from DESIGN.md 5 (the true-CFG row, same B, T, grids and 4 steps): "the plain loops sit at about 3e-4", and the
# CFG loop at scale 4 at 1.3e-3 — g = s * pos + (1 - s) * neg carries sqrt(s^2 + (s - 1)^2) times one evaluation's error: 5 at s = 4 (1.5e-3 predicted, 1.3e-3
# measured), sqrt(5) = 2.24 at SCALE = 2.
BF16_FLOOR = 3e-4
BF16_FLOOR_CFG = 3e-4 * math.sqrt(SCALE ** 2 + (SCALE - 1) ** 2)
BF16_FLOOR_CN = 6e-4  # the 4-step ControlNet loop at conditioning scale 4 ("Checked by": "measured 6e-4 plain")


def bf16_floor(case):
    return {"cfg": BF16_FLOOR_CFG, "controlnet": BF16_FLOOR_CN}.get(case, BF16_FLOOR)
# A variant every other one is told from the correct loop by distance; this one is reported only: the synthetic model depends on t so weakly that evaluating
# Heun's second slope at t_i moves the result by 2e-4 .. 3e-4, below BF16_FLOOR.  Its exact test: one Heun step IS forward(x, t), heun_predict, forward(xp, t'),
# heun_correct bit for bit, and the same composition with t in place of t' is another result (tests/test_gpu_solvers.py).
DEMOTED_VARIANT = "heun_second_eval_at_t_i"
CASES = ("plain", "context+mask", "cfg", "controlnet", "cache")


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
    """The inputs of one grid (read-only: shared by every test)."""
    s_hw, r_hw = SHAPES[shape]
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, s_hw, T, seed=61)
    _, _, ntxt, _, ny = flux_inputs(SMALL_FLUX, B, s_hw, T, seed=63)
    ntxt, ny = bf16_round(ntxt * f32(NEG_MULT)), (ny * f32(NEG_MULT)).astype(np.float32)
    ctx = flux_inputs(SMALL_FLUX, B, r_hw, T, seed=62)[0]
    rng = np.random.default_rng(65)
    x0 = rng.standard_normal(img.shape).astype(np.float32)
    cond = rng.standard_normal(img.shape).astype(np.float32)
    mask = rng.random(img.shape).astype(np.float32)
    mask[rng.random(img.shape) < 0.3] = 0.0  # mixed: kept elements (0), repainted ones (1) and soft ones in between
    mask[rng.random(img.shape) < 0.3] = 1.0
    s = dict(S=s_hw[0] * s_hw[1], R=r_hw[0] * r_hw[1], img=img, ids=ids, txt=txt, txt_ids=txt_ids, y=y, ntxt=ntxt, ny=ny, ctx=ctx, rids=np_ids(B, r_hw[0], r_hw[1], 1.0),
             x0=x0, cond=cond, mask=mask, g=np.full(B, 3.5, np.float32))
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def case_options(case):
    """(cfg, mask) of a case"""
    return case == "cfg", case == "context+mask"


@functools.lru_cache(maxsize=None)
def reference(solver, shape, case="plain", schedule=None, variant=None):
    """The composed loop of one solver, grid, case and schedule on the oracle, computed once and shared (read-only).  case: "plain"; "context+mask" (the grid's
    reference rows and the mixed mask); "cfg" (the negative at SCALE); "controlnet" (the 1 + 1-block net at CN_SCALE * CN_STEP_SCALES); "cache" (the step cache forced to CACHE_FORCE)."""
    s, om = inputs(shape), oracle_model()
    schedule = schedule or SOLVER_SCHEDULE.get(solver, "full")
    kw = {}
    if case == "context+mask":
        ev = oracle_eval(om, s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], ctx=s["ctx"], rids=s["rids"])
        kw = dict(x0=s["x0"], noise=s["img"], mask=s["mask"])
    elif case == "cfg":
        ev = oracle_eval(om, s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], neg_txt=s["ntxt"], neg_y=s["ny"])
        kw = dict(scale=SCALE)
    elif case == "controlnet":
        ev = controlnet_eval(s, s["cond"])
    elif case == "cache":
        ev = step_cache_eval(om, state_dict(), SMALL_FLUX, s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], CACHE_FORCE)
    else:
        ev = oracle_eval(om, s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"])
    out = solve(ev, s["img"], SCHEDULES[schedule], solver, variant=variant, **kw)
    out.setflags(write=False)
    return out
