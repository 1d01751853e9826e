"""True classifier-free guidance in the denoise loop: fmi_flux_denoise_cfg / fmi_cfg_euler_step and the pipeline's negative_prompt= /
negative_embeddings= / true_cfg_scale=.

The exact tests carry the weight.  On the CPU oracle at the shapes below (4 steps, scale 4) every plumbing mistake — the prompt only, the negative only, the
halves swapped, the negative's text with the prompt's y, the other sample's negative rows — moves the final latents by 5e-3 .. 2e-2 (tests/test_host_true_cfg.py
measures it), all under the project's 3e-2 loop bar, so that bar alone proves nothing here.  What the semantics promise exactly is compared bit for bit: a negative
equal to the prompt IS the plain loop at any scale, scale 0 IS the plain loop on the negative, one step IS a forward on the stacked 2B batch followed by
fmi_cfg_euler_step, the loop IS the chain of its one-step loops, a batch IS its single-sample runs.  Against the oracle the result must also lie at most a
third as far from the correct composition (tests/true_cfg_ref.py) as from each wrong one.

B = 2, T = 32 and the two shape sets of tests/test_gpu_kontext.py: ragged S = 4x6 = 24, R = 5x7 = 35; aligned S = 8x8 = 64, R = 6x8 = 48.  The negatives are
flux_inputs(seed=43)'s txt and y next to seed 41 for the prompt's."""
import ctypes as C

import numpy as np
import pytest

from tests import true_cfg_ref as R
from tests.util import SMALL_FLUX, SMALL_VAE, bf16_round, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu

f32 = np.float32
B, T = 2, 32
SHAPES = {"ragged": ((4, 6), (5, 7)), "aligned": ((8, 8), (6, 8))}
TS4 = [1.0, 0.8, 0.55, 0.3, 0.0]
SCALE = 4.0


def _np_ids(Bn, h2, w2, id0=0.0):
    ids = np.empty((Bn, h2 * w2, 3), np.float32)
    ids[:, :, 0] = f32(id0)
    ids[:, :, 1] = np.repeat(np.arange(h2), w2).astype(np.float32)[None]
    ids[:, :, 2] = np.tile(np.arange(w2), h2).astype(np.float32)[None]
    return ids


@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    sd = d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    gm = d.FluxModel(SMALL_FLUX)
    gm.load_state_dict(sd)
    om = orc.Flux(SMALL_FLUX)
    om.load(sd)
    sets = {}
    for name, (s_hw, r_hw) in SHAPES.items():
        img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, s_hw, T, seed=41)
        _, _, ntxt, _, ny = flux_inputs(SMALL_FLUX, B, s_hw, T, seed=43)
        ctx = flux_inputs(SMALL_FLUX, B, r_hw, T, seed=42)[0]
        rng = np.random.default_rng(45)
        x0 = rng.standard_normal(img.shape).astype(np.float32)
        mask = rng.random(img.shape).astype(np.float32)
        mask[rng.random(img.shape) < 0.3] = 0.0  # mixed: kept elements (0), repainted ones (1) and soft ones in between
        mask[rng.random(img.shape) < 0.3] = 1.0
        sets[name] = dict(S=s_hw[0] * s_hw[1], R=r_hw[0] * r_hw[1], img=img, ids=ids, txt=txt, txt_ids=txt_ids, y=y, ntxt=ntxt, ny=ny, ctx=ctx,
                          rids=_np_ids(B, r_hw[0], r_hw[1], id0=1.0), x0=x0, mask=mask)
    return dict(torch=torch, d=d, orc=orc, sd=sd, gm=gm, om=om, sets=sets, g=np.full(B, 3.5, np.float32))


def _loop(env, s, ts, txt=None, y=None, neg=None, scale=None, sl=slice(None), img=None, gm=None, **extra):
    """gm.denoise on the set's image (or `img`) with the prompt (txt, y) — default the set's —, the negative neg = (txt, y) or None, and extra per-sample inputs"""
    torch = env["torch"]
    txt, y = (s["txt"] if txt is None else txt), (s["y"] if y is None else y)
    extra = {k: dev(v[sl]) for k, v in extra.items()}
    if neg is not None:
        extra.update(negative_txt=dev(neg[0][sl], torch.bfloat16), negative_y=dev(neg[1][sl]), true_cfg_scale=scale)
    return host((gm or env["gm"]).denoise(dev((s["img"] if img is None else img)[sl]), dev(s["ids"][sl]), dev(txt[sl], torch.bfloat16), dev(s["txt_ids"][sl]),
                                          dev(y[sl]), dev(env["g"][sl]), ts, **extra))


def _pinned(env, gm=None):
    """the modulation precompute picks its kernel by row count, and CFG doubles the rows: pinned to the GEMV passes wherever bits are compared across row counts"""
    from diffusion_rs_amd import _lib as L
    gm = gm or env["gm"]

    class Pin:
        def __enter__(self):
            L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 0))

        def __exit__(self, *exc):
            L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 1))
            return False

    return Pin()


def _extras(s, kind):
    blend = dict(x0=s["x0"], noise=s["img"], mask=s["mask"])
    ctx = dict(context=s["ctx"], context_ids=s["rids"])
    return {"plain": {}, "context": ctx, "mask": blend, "context+mask": dict(ctx, **blend)}[kind]


# ------------------------------------------------------------------------------------------------ 1. a negative equal to the prompt
@pytest.mark.parametrize("kind", ["plain", "context", "mask"])
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_negative_equal_to_the_prompt_is_the_plain_loop(env, shape, kind):
    s = env["sets"][shape]
    if kind == "context":
        s = dict(s, ctx=env["sets"]["ragged"]["ctx"], rids=env["sets"]["ragged"]["rids"])  # the ragged context (R = 35) at both state shapes
    extra = _extras(s, kind)
    with _pinned(env):
        plain = _loop(env, s, TS4, **extra)
        assert np.isfinite(plain).all()
        for scale in (0.0, 1.0, 4.0):
            got = _loop(env, s, TS4, neg=(s["txt"], s["y"]), scale=scale, **extra)
            np.testing.assert_array_equal(got, plain, err_msg=f"scale {scale}")


# ------------------------------------------------------------------------------------------------ 2. scale 0
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_scale_zero_is_the_plain_loop_on_the_negative(env, shape):
    s = env["sets"][shape]
    with _pinned(env):
        want = _loop(env, s, TS4, txt=s["ntxt"], y=s["ny"])
        got = _loop(env, s, TS4, neg=(s["ntxt"], s["ny"]), scale=0.0)
        np.testing.assert_array_equal(got, want)
        assert not np.array_equal(got, _loop(env, s, TS4))  # (the negative is another prompt)
        # the y of the negative half is the negative's: with the prompt's y in its place the loop is another one
        assert not np.array_equal(got, _loop(env, s, TS4, txt=s["ntxt"], y=s["y"]))


# ------------------------------------------------------------------------------------------------ 3. one step
@pytest.mark.parametrize("with_context", [False, True])
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_one_step_is_a_forward_on_the_stacked_batch_and_the_cfg_step(env, shape, with_context):
    torch, d, gm, s = env["torch"], env["d"], env["gm"], env["sets"][shape]
    t0, t1 = 0.8, 0.55
    two = lambda a: np.concatenate([a, a], 0)
    ctx = dict(context=dev(two(s["ctx"])), context_ids=dev(two(s["rids"]))) if with_context else {}
    pred = gm.forward(dev(two(s["img"])), dev(two(s["ids"])), dev(np.concatenate([s["txt"], s["ntxt"]], 0), torch.bfloat16), dev(two(s["txt_ids"])),
                      dev(np.full(2 * B, t0, np.float32)), dev(np.concatenate([s["y"], s["ny"]], 0)), dev(two(env["g"])), **ctx)
    assert tuple(pred.shape) == (2 * B, s["S"], 64)
    x = dev(s["img"]).clone()
    d.cfg_euler_step(x, pred[:B].contiguous(), pred[B:].contiguous(), SCALE, float(f32(t1 - t0)))
    got = _loop(env, s, [t0, t1], neg=(s["ntxt"], s["ny"]), scale=SCALE, **(_extras(s, "context") if with_context else {}))
    np.testing.assert_array_equal(got, host(x))
    assert not np.array_equal(got, s["img"])


# ------------------------------------------------------------------------------------------------ 4. the chain, 5. batch against single
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_loop_is_the_chain_of_its_one_step_loops_and_a_batch_is_its_single_runs(env, shape):
    s = env["sets"][shape]
    neg = (s["ntxt"], s["ny"])
    with _pinned(env):
        x = s["img"]
        for i in range(4):
            x = _loop(env, s, TS4[i:i + 2], img=x)
        np.testing.assert_array_equal(_loop(env, s, TS4), x, err_msg="plain loop vs its one-step chain")
        x = s["img"]
        for i in range(4):
            x = _loop(env, s, TS4[i:i + 2], img=x, neg=neg, scale=SCALE)
        both = _loop(env, s, TS4, neg=neg, scale=SCALE)
        assert np.isfinite(both).all()
        np.testing.assert_array_equal(both, x, err_msg="CFG loop vs its one-step chain")
        for b in range(B):
            one = _loop(env, s, TS4, neg=neg, scale=SCALE, sl=slice(b, b + 1))
            np.testing.assert_array_equal(one, both[b:b + 1], err_msg=f"sample {b}")
        assert not np.array_equal(both[0], both[1])


# ------------------------------------------------------------------------------------------------ 6. masks
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_masks(env, shape):
    s = env["sets"][shape]
    neg = (s["ntxt"], s["ny"])
    plain = _loop(env, s, TS4, neg=neg, scale=SCALE)
    ones = _loop(env, s, TS4, neg=neg, scale=SCALE, x0=s["x0"], noise=s["img"], mask=np.ones_like(s["x0"]))
    np.testing.assert_array_equal(ones, plain)
    zeros = _loop(env, s, TS4, neg=neg, scale=SCALE, x0=s["x0"], noise=s["img"], mask=np.zeros_like(s["x0"]))
    np.testing.assert_array_equal(zeros, s["x0"])
    mixed = _loop(env, s, TS4, neg=neg, scale=SCALE, x0=s["x0"], noise=s["img"], mask=s["mask"])
    keep = s["mask"] == 0
    assert keep.any() and TS4[-1] == 0.0
    np.testing.assert_array_equal(mixed[keep], s["x0"][keep])
    assert not np.array_equal(mixed[~keep], s["x0"][~keep]) and not np.array_equal(mixed, plain)


# ------------------------------------------------------------------------------------------------ 7. null cfg, 9. refusals
def _ctypes_cfg(env, s, cfg_struct, blend=(None, None, None), entry="cfg", inputs=None):
    """fmi_flux_denoise_cfg (or fmi_flux_denoise_context) at the ctypes level on a copy of the set's image; returns (status, result, the copy before)"""
    torch, gm = env["torch"], env["gm"]
    s = inputs or s
    img = dev(s["img"]).clone()
    g = dev(np.full(s["img"].shape[0], 3.5, np.float32))
    inp, keep = gm._inputs(None, dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), None, dev(s["y"]), g)
    ts = (C.c_double * 5)(*TS4)
    p = [None if e is None else C.c_void_p(e.data_ptr()) for e in blend]
    if entry == "cfg":
        rc = gm.lib.fmi_flux_denoise_cfg(gm.h, C.byref(inp), None, None if cfg_struct is None else C.byref(cfg_struct), C.c_void_p(img.data_ptr()), ts, 4, p[0], p[1], p[2], None)
    else:
        rc = gm.lib.fmi_flux_denoise_context(gm.h, C.byref(inp), None, C.c_void_p(img.data_ptr()), ts, 4, p[0], p[1], p[2], None)
    torch.cuda.synchronize()
    return rc, host(img)


@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_null_cfg_is_the_context_entry(env, shape):
    s = env["sets"][shape]
    for blend in ((None, None, None), (dev(s["x0"]), dev(s["img"]), dev(s["mask"]))):
        rc, want = _ctypes_cfg(env, s, None, blend, entry="context")
        assert rc == 0
        rc, got = _ctypes_cfg(env, s, None, blend)
        assert rc == 0
        np.testing.assert_array_equal(got, want)
        assert not np.array_equal(got, s["img"])


@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_refusals_leave_the_state_untouched(env, shape):
    from diffusion_rs_amd import _lib as L
    torch, s = env["torch"], env["sets"][shape]
    ntxt, ny = dev(s["ntxt"], torch.bfloat16), dev(s["ny"])
    pt, py = C.c_void_p(ntxt.data_ptr()), C.c_void_p(ny.data_ptr())

    def refused(code, cfg_struct, blend=(None, None, None), inputs=None):
        rc, after = _ctypes_cfg(env, s, cfg_struct, blend, inputs=inputs)
        assert rc == code, (rc, code)
        np.testing.assert_array_equal(after.view(np.uint32), (inputs or s)["img"].view(np.uint32))  # bit for bit

    refused(L.ERR_INVALID, L.FluxTrueCfg(pt, L.BF16, py, L.F32, float("nan")))
    refused(L.ERR_INVALID, L.FluxTrueCfg(pt, L.BF16, py, L.F32, -1.0))
    refused(L.ERR_INVALID, L.FluxTrueCfg(pt, L.BF16, py, L.F32, float("inf")))
    refused(L.ERR_INVALID, L.FluxTrueCfg(pt, L.BF16, None, L.F32, 4.0))  # null neg_y
    refused(L.ERR_INVALID, L.FluxTrueCfg(None, L.BF16, py, L.F32, 4.0))  # null neg_txt
    refused(L.ERR_INVALID, L.FluxTrueCfg(pt, L.F16, py, L.F32, 4.0))  # a dtype that is neither F32 nor BF16
    refused(L.ERR_INVALID, L.FluxTrueCfg(pt, L.BF16, py, L.U8, 4.0))
    x0 = dev(s["x0"])
    refused(L.ERR_INVALID, L.FluxTrueCfg(pt, L.BF16, py, L.F32, 4.0), (x0, None, x0))  # x0 / noise / mask in part
    img5, ids5, txt5, txt_ids5, y5 = flux_inputs(SMALL_FLUX, 5, SHAPES[shape][0], T, seed=47)
    five = dict(img=img5, ids=ids5, txt=txt5, txt_ids=txt_ids5, y=y5)
    n5 = dev(txt5, torch.bfloat16), dev(y5)
    refused(L.ERR_UNSUPPORTED, L.FluxTrueCfg(C.c_void_p(n5[0].data_ptr()), L.BF16, C.c_void_p(n5[1].data_ptr()), L.F32, 4.0), inputs=five)  # 2B = 10 > 8
    # the Python layer refuses the same before it reaches the library
    with pytest.raises(ValueError, match="B = 5 > 4"):
        env["gm"].denoise(dev(img5), dev(ids5), dev(txt5, torch.bfloat16), dev(txt_ids5), dev(y5), dev(np.full(5, 3.5, np.float32)), TS4,
                          negative_txt=n5[0], negative_y=n5[1], true_cfg_scale=4.0)
    with pytest.raises(ValueError, match="step cache"):
        env["gm"].denoise(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(s["y"]), dev(env["g"]), TS4, negative_txt=ntxt,
                          negative_y=ny, cache_threshold=0.1)
    rc, got = _ctypes_cfg(env, s, L.FluxTrueCfg(pt, L.BF16, py, L.F32, 4.0))  # the model is as it was
    assert rc == 0
    np.testing.assert_array_equal(got, _loop(env, s, TS4, neg=(s["ntxt"], s["ny"]), scale=4.0))


# ------------------------------------------------------------------------------------------------ 8. int8 mode
def test_int8_mode_negative_equal_to_the_prompt(env):
    d, s = env["d"], env["sets"]["ragged"]
    gq = d.FluxModel(SMALL_FLUX)
    gq.load_state_dict(env["sd"])
    gq.quantize_int8()
    try:
        with _pinned(env, gq):
            plain = _loop(env, s, TS4, gm=gq)
            assert np.isfinite(plain).all() and not np.array_equal(plain, _loop(env, s, TS4))  # (it is the int8 model)
            for scale in (0.0, 1.0, 4.0):
                np.testing.assert_array_equal(_loop(env, s, TS4, gm=gq, neg=(s["txt"], s["y"]), scale=scale), plain, err_msg=f"scale {scale}")
    finally:
        gq.close()


# ------------------------------------------------------------------------------------------------ fmi_cfg_euler_step against numpy
GRID_CAP_ITEMS = 256 * 8 * 256  # small_ops.hip map_grid: at most 256 * 8 blocks of 256 threads; one item more and the grid-stride loop wraps
STEP_SIZES = {"aligned": 2 * 64 * 64, "odd": 105, "wrap_float4": 4 * (GRID_CAP_ITEMS + 1), "wrap_scalar": GRID_CAP_ITEMS + 1}


def _offset(torch, a):
    """a copy of `a` on the device that starts one float past a 16-byte boundary: the scalar path"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("size", ["aligned", "odd", "offset", "wrap_float4", "wrap_scalar"])
def test_cfg_euler_step_against_numpy(size, masked):
    import torch
    import diffusion_rs_amd as d
    n = STEP_SIZES.get(size, STEP_SIZES["aligned"])
    rng = np.random.default_rng(7)
    img, pos, neg, x0, noise = (rng.standard_normal(n).astype(np.float32) for _ in range(5))
    mask = rng.random(n).astype(np.float32)
    scale, dt, s = 3.5, -0.2, 0.55
    put = (lambda a: _offset(torch, a)) if size == "offset" else dev
    blend_np = (x0, noise, mask) if masked else ()

    def run(p, q, sc, place=put):
        x = place(img)  # (a fresh device copy: the step is in place)
        kw = dict(zip(("x0", "noise", "mask"), (place(a) for a in blend_np)))
        out = d.cfg_euler_step(x, place(p), place(q), sc, dt, s=s, **kw)
        assert out is x
        return host(x)

    got = run(pos, neg, scale)
    # numpy in float64 from the f32-rounded difference and the f32 scalars
    u = 2.0 ** -24
    df = (pos - neg).astype(np.float32).astype(np.float64)
    sc64, dt64, s64, a64 = float(f32(scale)), float(f32(dt)), float(f32(s)), float(f32(1) - f32(s))
    want = img.astype(np.float64) + (neg.astype(np.float64) + sc64 * df) * dt64
    mag = np.abs(img) + abs(dt64) * (np.abs(neg) + sc64 * (np.abs(pos) + np.abs(neg)))
    if masked:
        m64 = mask.astype(np.float64)
        want = m64 * want + (1.0 - m64) * (a64 * x0.astype(np.float64) + s64 * noise.astype(np.float64))
        mag = mag + np.abs(x0) + np.abs(noise)
    err = np.abs(got.astype(np.float64) - want)
    print(f"cfg_euler_step {size} n={n} masked={masked}: max err / bound {float((err / (4 * u * mag)).max()):.3f}")
    assert np.isfinite(got).all() and (err <= 4 * u * mag.astype(np.float64)).all()
    # exact: pos IS neg at any scale, and scale 0 with any pos, step along neg — the same bits; a second run is identical
    along_neg = run(neg, neg, 0.0)
    for sc in (1.0, 7.5):
        np.testing.assert_array_equal(run(neg, neg, sc), along_neg, err_msg=f"pos is neg, scale {sc}")
    np.testing.assert_array_equal(run(pos, neg, 0.0), along_neg, err_msg="scale 0")
    np.testing.assert_array_equal(run(pos, neg, scale), got, err_msg="second run")
    if size == "aligned":  # the same values through the scalar path
        np.testing.assert_array_equal(run(pos, neg, scale, place=lambda a: _offset(torch, a)), got, err_msg="scalar path vs 16-byte path")


def test_cfg_euler_step_argument_errors():
    import torch
    import diffusion_rs_amd as d
    x = torch.zeros(8, device="cuda")
    with pytest.raises(ValueError, match="go together"):
        d.cfg_euler_step(x, x.clone(), x.clone(), 1.0, 0.1, x0=x.clone())
    with pytest.raises(TypeError):
        d.cfg_euler_step(x, x.clone()[:4], x.clone(), 1.0, 0.1)
    with pytest.raises(d.FmiError):
        d.cfg_euler_step(x, x.clone(), x.clone(), -1.0, 0.1)


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_loop_matches_the_oracle_composition_and_no_wrong_one(env, shape):
    """Final latents within the project's 3e-2 of the correct composed reference, and at most ONE THIRD as far from it as from each of the five wrong
    compositions, computed on the oracle itself.  Measured on an MI355X: see DESIGN.md 5."""
    om, s = env["om"], env["sets"][shape]
    got = _loop(env, s, TS4, neg=(s["ntxt"], s["ny"]), scale=SCALE)
    ref = lambda variant=None: R.cfg_loop(om, s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["ntxt"], s["ny"], env["g"], TS4, SCALE, variant=variant)
    err = rel_l2(got, ref())
    print(f"CFG loop {shape} (4 steps, scale 4, B=2, S={s['S']}, T=32): final latents rel-L2 {err:.3e} vs the correct composition")
    far = {v: rel_l2(got, ref(v)) for v in R.VARIANTS}
    for v, dist in far.items():
        print(f"    {v}: rel-L2 {dist:.3e} ({dist / err:.1f} x)")
    assert np.isfinite(got).all() and err <= 3e-2
    for v, dist in far.items():
        assert err <= dist / 3, v


def test_loop_with_context_and_mask_matches_the_oracle_composition(env):
    om, s = env["om"], env["sets"]["ragged"]
    got = _loop(env, s, TS4, neg=(s["ntxt"], s["ny"]), scale=SCALE, **_extras(s, "context+mask"))
    ref = lambda variant=None: R.cfg_loop(om, s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["ntxt"], s["ny"], env["g"], TS4, SCALE, ctx=s["ctx"],
                                          rids=s["rids"], x0=s["x0"], noise=s["img"], mask=s["mask"], variant=variant)
    err = rel_l2(got, ref())
    print(f"CFG loop ragged with the R=35 context and a mixed mask: final latents rel-L2 {err:.3e} vs the correct composition")
    far = {v: rel_l2(got, ref(v)) for v in R.VARIANTS}
    for v, dist in far.items():
        print(f"    {v}: rel-L2 {dist:.3e} ({dist / err:.1f} x)")
    assert np.isfinite(got).all() and err <= 3e-2
    for v, dist in far.items():
        assert err <= dist / 3, v
    np.testing.assert_array_equal(got[s["mask"] == 0], s["x0"][s["mask"] == 0])


# ------------------------------------------------------------------------------------------------ the pipeline
H, W, STEPS, GUIDANCE, TP, SEED = 128, 192, 4, 3.5, 24, 11


@pytest.fixture(scope="module")
def pipe_env():
    """the synthetic source without text encoders at the small configuration, holding the weights the oracle holds"""
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    sd = d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    vsd = d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0)
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=SMALL_FLUX, vae_cfg=SMALL_VAE))
    pipe.flux.load_state_dict(sd)
    pipe.vae.load_state_dict(vsd)
    om, ov = orc.Flux(SMALL_FLUX), orc.Vae(SMALL_VAE)
    om.load(sd)
    ov.load(vsd)
    rng = np.random.default_rng(51)
    J, P = SMALL_FLUX["joint_attention_dim"], SMALL_FLUX["pooled_projection_dim"]
    t5 = bf16_round(rng.standard_normal((B, TP, J)).astype(np.float32))
    clip = rng.standard_normal((B, P)).astype(np.float32)
    nt5 = bf16_round(rng.standard_normal((1, TP, J)).astype(np.float32))
    nclip = rng.standard_normal((1, P)).astype(np.float32)
    params = d.DiffusionGenerationParams(height=H, width=W, num_steps=STEPS, guidance_scale=GUIDANCE)
    return dict(torch=torch, d=d, orc=orc, pipe=pipe, om=om, ov=ov, t5=t5, clip=clip, nt5=nt5, nclip=nclip, params=params,
                emb=(dev(t5, torch.bfloat16), dev(clip)), nemb=(dev(nt5, torch.bfloat16), dev(nclip)))


def test_pipeline_true_cfg_matches_the_oracle_pipeline(pipe_env):
    env = pipe_env
    torch, orc, om, ov, pipe = env["torch"], env["orc"], env["om"], env["ov"], env["pipe"]
    u8, final = pipe.forward(["a", "b"], env["params"], output="tensor", seed=SEED, embeddings=env["emb"], negative_embeddings=env["nemb"], true_cfg_scale=4.0,
                             return_latents=True)
    assert tuple(final.shape) == (B, (H // 16) * (W // 16), 64) and tuple(u8.shape) == (B, 3, H, W)
    # the oracle pipeline: Philox noise -> pack -> the composed CFG loop with the ONE negative in both samples' rows -> unpack -> decode -> u8
    h, w = H // 8, W // 8
    lat = orc.randn(16 * h * w, B, SEED).reshape(B, 16, h, w).astype(np.float32)
    noise, ids = orc.pack_latents(lat)
    sched = pipe.scheduler
    mu = orc.calculate_shift(noise.shape[1], sched.base_image_seq_len, sched.max_image_seq_len, sched.base_shift, sched.max_shift)
    ts = orc.get_timesteps(STEPS, sched.use_dynamic_shifting, mu, sched.shift)
    txt_ids = np.zeros((B, TP, 3), np.float32)
    ref = R.cfg_loop(om, noise, ids, env["t5"], txt_ids, env["clip"], np.repeat(env["nt5"], B, 0), np.repeat(env["nclip"], B, 0), np.full(B, GUIDANCE, np.float32),
                     ts, 4.0)
    err = rel_l2(host(final), ref)
    z = orc.unpack_latents(ref, 16, h, w) * f32(1.0 / SMALL_VAE["scaling_factor"]) + f32(SMALL_VAE["shift_factor"])
    ref_u8 = orc.postprocess_u8(ov.decode(z.astype(np.float32)))
    diff = np.abs(u8.cpu().numpy().astype(np.int32) - ref_u8.astype(np.int32))
    share, worst = float((diff <= 2).mean()), int(diff.max())
    print(f"pipeline true CFG (128 x 192, {STEPS} steps, B=2, scale 4): final latents rel-L2 {err:.3e}; u8 within 2 on {share:.4f}, max |d| {worst}")
    assert err <= 3e-2
    assert share >= 0.99
    plain = pipe.forward(["a", "b"], env["params"], output="tensor", seed=SEED, embeddings=env["emb"])
    assert not torch.equal(u8, plain)
    # a negative with true_cfg_scale = 1 is ignored (diffusers' do_true_cfg): the request without it, bit for bit
    ignored = pipe.forward(["a", "b"], env["params"], output="tensor", seed=SEED, embeddings=env["emb"], negative_embeddings=env["nemb"], true_cfg_scale=1.0)
    assert torch.equal(ignored, plain)


def test_pipeline_five_prompts_run_as_chunks_of_four_and_one(pipe_env):
    env = pipe_env
    torch, pipe = env["torch"], env["pipe"]
    prompts = ["a", "b", "c", "d", "e"]
    kw = dict(output="tensor", seed=SEED, negative_prompt="x", true_cfg_scale=4.0)
    whole = pipe.forward(prompts, env["params"], **kw)
    first = pipe.forward(prompts[:4], env["params"], **kw)
    last = pipe.forward(prompts[4:], env["params"], first_sample=4, **kw)
    assert tuple(whole.shape) == (5, 3, H, W)
    assert torch.equal(whole, torch.cat([first, last], 0))
    # the negative prompt matters
    assert not torch.equal(first, pipe.forward(prompts[:4], env["params"], output="tensor", seed=SEED))
    with pytest.raises(ValueError, match="needs a negative"):
        pipe.forward(prompts, env["params"], output="tensor", seed=SEED, true_cfg_scale=4.0)
