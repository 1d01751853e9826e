"""Channel-concatenated conditioning (FLUX.1 Fill / Canny / Depth): fmi_flux_create_cond, fmi_flux_forward_control / fmi_flux_denoise_control,
the glue kernels fmi_cast_cols_bf16 / fmi_mask_image / fmi_fill_condition, and the pipeline's control_image= / control_mask=.

The glue is compared bit for bit with numpy.  What the semantics promise exactly is compared bit for bit too: conditioning columns of x_embedder that are zero —
or a conditioning that is zero — ARE the plain 64-channel model (exact zeros added to f32 accumulators change nothing), the loop IS the chain of forward_control
and the Euler step, a batch IS its single-sample runs, a negative equal to the prompt IS the plain control loop, mask == 1 IS the control loop and mask == 0
returns x0, a null control on a plain model IS fmi_flux_denoise_cfg.  Against the oracle (tests/control_ref.py: oracle.Flux at in_channels = 64 + Cc with proj_out
zero-padded) one evaluation is within the project's 2e-2, the 4-step loop within its 3e-2, and the loop lies at most a third as far from the correct composition
as from each wrong one — which tests/test_host_control.py shows to be at least 9e-2 away from it.

SMALL_FLUX with in_channels 128 (Cc = 64: Canny / Depth) and 384 (Cc = 320: Fill), out_channels 64; B = 2, T = 32; token grids 6x4 (aligned) and 5x7 (ragged)."""
import ctypes as C

import numpy as np
import pytest

from tests import control_ref as CR
from tests.util import SMALL_FLUX, SMALL_VAE, bf16_round, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu

f32 = np.float32
B, T = 2, 32
GRIDS = {"aligned": (6, 4), "ragged": (5, 7)}
WIDTHS = (128, 384)
TS4 = [1.0, 0.8, 0.55, 0.3, 0.0]
SCALE = 4.0
GRID_CAP_ITEMS = 256 * 8 * 256  # small_ops.hip map_grid: at most 256 * 8 blocks of 256 threads; one item more and the grid-stride loop wraps


def _cfg(K):
    return dict(SMALL_FLUX, in_channels=K, out_channels=64)


def _bf16_bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _offset(torch, a):
    """a copy of `a` on the device that starts one float past a 16-byte boundary: the scalar path"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    assert v.data_ptr() % 16 == 4
    return v.view(a.shape)


# ------------------------------------------------------------------------------------------------ the glue kernels, bit for bit
@pytest.mark.parametrize("col0", [0, 64])
@pytest.mark.parametrize("dst_ld", [128, 384])
@pytest.mark.parametrize("rows", [24, 35, 70000])
def test_cast_cols_bf16_is_bf16_round_in_the_window_and_nothing_outside(rows, dst_ld, col0):
    import torch
    import diffusion_rs_amd as d
    cols = 64 if col0 == 0 else dst_ld - 64  # the state's window, or the conditioning's
    if rows == 70000:
        assert rows * (cols // 8) > GRID_CAP_ITEMS  # beyond the grid cap: the grid-stride loop wraps
    rng = np.random.default_rng(rows + dst_ld + col0)
    fill = rng.integers(0, 1 << 16, (rows, dst_ld), dtype=np.uint16)  # what the destination held: any bits, NaN patterns included
    for rows_src in (rows, rows // 2 if rows % 2 == 0 else rows // 5):  # every row its own source; the source wrapped (true CFG: both halves from one)
        src = rng.standard_normal((rows_src, cols)).astype(np.float32) * f32(3)
        src[0, :4] = [0.0, -0.0, 1.00390625, 1.01171875]  # signed zeros and two ties of the bf16 rounding (to even: down, up)
        for dtype in (torch.float32, torch.bfloat16):
            s = dev(src).to(dtype)
            want_rows = bf16_round(src) if dtype == torch.float32 else host(s)
            want = fill.copy()
            want[:, col0:col0 + cols] = (np.ascontiguousarray(want_rows[np.arange(rows) % rows_src]).view(np.uint32) >> 16).astype(np.uint16)
            dst = dev(fill.view(np.int16)).view(torch.bfloat16)
            out = d.cast_cols_bf16(s, dst, col0)
            assert out is dst
            np.testing.assert_array_equal(_bf16_bits(dst), want, err_msg=f"rows_src {rows_src} {dtype}")
            d.cast_cols_bf16(s, dst, col0)  # a second run
            np.testing.assert_array_equal(_bf16_bits(dst), want, err_msg=f"second run, rows_src {rows_src} {dtype}")
    if rows == 24:  # the same bits through the scalar path (a source one float past a 16-byte boundary)
        dst = dev(fill.view(np.int16)).view(torch.bfloat16)
        d.cast_cols_bf16(_offset(torch, src), dst, col0)
        want = fill.copy()
        want[:, col0:col0 + cols] = (bf16_round(src)[np.arange(rows) % src.shape[0]].view(np.uint32) >> 16).astype(np.uint16)
        np.testing.assert_array_equal(_bf16_bits(dst), want, err_msg="scalar path")


def _soft_mask(rng, Bn, H, W):
    m = rng.random((Bn, H, W)).astype(np.float32)
    m[rng.random(m.shape) < 0.2] = 0.5  # exactly the threshold: counts as 1
    m[rng.random(m.shape) < 0.2] = 0.0
    m[rng.random(m.shape) < 0.2] = 1.0
    m[0, 0, :3] = [0.5, np.nextafter(f32(0.5), f32(0)), np.nextafter(f32(0.5), f32(1))]
    return m


@pytest.mark.parametrize("hw", [(48, 80), (16, 16)])
def test_mask_image_and_fill_condition_against_numpy(hw):
    import torch
    import diffusion_rs_amd as d
    H, W = hw
    rng = np.random.default_rng(H)
    m = _soft_mask(rng, 2, H, W)
    img = rng.standard_normal((2, 3, H, W)).astype(np.float32)
    S = (H // 16) * (W // 16)
    lat = rng.standard_normal((2, S, 64)).astype(np.float32)
    want_img, want_cond = CR.mask_image(img, m), CR.fill_condition(lat, m)
    assert {0.0, 0.5, 1.0} <= set(np.unique(m)) and want_cond[:, :, 64:].mean() > 0.3
    for place in (dev, lambda a: _offset(torch, a)):  # the 16-byte path and the scalar one
        got_img = d.mask_image(place(img), place(m))
        np.testing.assert_array_equal(host(got_img).view(np.uint32), want_img.view(np.uint32))  # (the sign of a masked zero included)
        got = d.fill_condition(place(lat), place(m))
        assert tuple(got.shape) == (2, S, 320)
        np.testing.assert_array_equal(host(got).view(np.uint32), want_cond.view(np.uint32))
    with pytest.raises(ValueError, match="multiples of 16"):
        d.fill_condition(dev(lat), dev(m[:, :H - 8]))
    with pytest.raises(ValueError, match="masked_latents is"):
        d.fill_condition(dev(lat[:, :, :32]), dev(m))
    with pytest.raises(ValueError, match="mask is"):
        d.mask_image(dev(img), dev(m[:1]))


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    models = {}
    for K in WIDTHS:
        cfg = _cfg(K)
        sd = d.synth.flux_state_dict_numpy(cfg, seed=0)
        gm = d.FluxModel(cfg)
        gm.load_state_dict(sd)
        om = orc.Flux(CR.oracle_cfg(cfg))
        om.load(CR.oracle_state_dict(sd, cfg))
        models[K] = dict(cfg=cfg, sd=sd, gm=gm, om=om)
    sets = {}
    for name, hw in GRIDS.items():
        img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, hw, T, seed=41)
        _, _, ntxt, _, ny = flux_inputs(SMALL_FLUX, B, hw, T, seed=43)
        rng = np.random.default_rng(45)
        x0 = rng.standard_normal(img.shape).astype(np.float32)
        mask = rng.random(img.shape).astype(np.float32)
        mask[rng.random(img.shape) < 0.3] = 0.0  # mixed: kept elements (0), repainted ones (1) and soft ones in between
        mask[rng.random(img.shape) < 0.3] = 1.0
        cond = {K: np.random.default_rng(44).standard_normal((B, hw[0] * hw[1], K - 64)).astype(np.float32) for K in WIDTHS}
        sets[name] = dict(S=hw[0] * hw[1], img=img, ids=ids, txt=txt, txt_ids=txt_ids, y=y, ntxt=ntxt, ny=ny, x0=x0, mask=mask, cond=cond)
    return dict(torch=torch, d=d, orc=orc, models=models, sets=sets, g=np.full(B, 3.5, np.float32))


def _plain_twin(env, K, sd=None):
    """the 64-channel model holding the conditioned model's weights, x_embedder cut to its state columns"""
    sd = dict(sd or env["models"][K]["sd"])
    sd["x_embedder.weight"] = np.ascontiguousarray(sd["x_embedder.weight"][:, :64])
    gp = env["d"].FluxModel(SMALL_FLUX)
    gp.load_state_dict(sd)
    return gp


def _loop(env, gm, s, ts, cond=None, neg=None, scale=None, sl=slice(None), img=None, **extra):
    torch = env["torch"]
    extra = {k: dev(v[sl]) for k, v in extra.items()}
    if cond is not None:
        extra.update(control=dev(cond[sl]))
    if neg is not None:
        extra.update(negative_txt=dev(neg[0][sl], torch.bfloat16), negative_y=dev(neg[1][sl]), true_cfg_scale=scale)
    return host(gm.denoise(dev((s["img"] if img is None else img)[sl]), dev(s["ids"][sl]), dev(s["txt"][sl], torch.bfloat16), dev(s["txt_ids"][sl]), dev(s["y"][sl]),
                           dev(env["g"][sl]), ts, **extra))


def _forward(env, gm, s, t, cond=None, img=None):
    torch = env["torch"]
    kw = {} if cond is None else dict(control=dev(cond))
    return gm.forward(dev(s["img"] if img is None else img), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(np.full(B, t, np.float32)),
                      dev(s["y"]), dev(env["g"]), **kw)


class _pinned:
    """the modulation precompute picks its kernel by row count (steps x samples): pinned to the GEMV passes wherever bits are compared across row counts"""

    def __init__(self, *models):
        self.models = models

    def __enter__(self):
        from diffusion_rs_amd import _lib as L
        for gm in self.models:
            L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 0))

    def __exit__(self, *exc):
        from diffusion_rs_amd import _lib as L
        for gm in self.models:
            L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 1))
        return False


def test_shapes_and_sizes_follow_the_two_widths(env):
    d = env["d"]
    plain = d.FluxModel(SMALL_FLUX)
    D = 256
    try:
        for K in WIDTHS:
            gm = env["models"][K]["gm"]
            assert gm.state_channels == 64 and gm.cond_channels == K - 64 and gm.lib.fmi_flux_cond_channels(gm.h) == K - 64
            w = gm.get_tensor("x_embedder.weight")
            assert tuple(w.shape) == (D, K) and tuple(gm.get_tensor("proj_out.weight").shape) == (64, D)
            np.testing.assert_array_equal(host(w), env["models"][K]["sd"]["x_embedder.weight"])
            with pytest.raises(d.FmiError, match="shape mismatch"):
                gm.set_tensor("x_embedder.weight", np.zeros((D, 64), np.float32))
            with pytest.raises(d.FmiError, match="shape mismatch"):
                gm.set_tensor("proj_out.weight", np.zeros((K, D), np.float32))
            # a LoRA pair on x_embedder is checked against the wide shape, like any other Linear
            with pytest.raises(d.FmiError, match="the Linear is"):
                gm.lora_add("a", "x_embedder", np.zeros((4, 64), np.float32), np.zeros((D, 4), np.float32))
            # the wider embedder is the whole difference in weight bytes (the BASE arena rounds to 256 B)
            extra = gm.state_buffers()[0][1] - plain.state_buffers()[0][1]
            assert abs(extra - D * (K - 64) * 2) <= 512, extra
        assert plain.cond_channels == 0 and plain.lib.fmi_flux_cond_channels(plain.h) == 0
    finally:
        plain.close()


@pytest.mark.parametrize("grid", ["aligned", "ragged"])
@pytest.mark.parametrize("K", WIDTHS)
def test_zero_conditioning_columns_or_zero_conditioning_is_the_plain_model(env, K, grid):
    """bf16 and after quantize_int8(): forward and the 4-step loop, bit for bit"""
    d, s, m = env["d"], env["sets"][grid], env["models"][K]
    cond = s["cond"][K]
    zsd = dict(m["sd"])
    zw = zsd["x_embedder.weight"].copy()
    zw[:, 64:] = 0
    zsd["x_embedder.weight"] = zw
    gz = d.FluxModel(m["cfg"])  # conditioning columns zero
    gz.load_state_dict(zsd)
    ga = d.FluxModel(m["cfg"])  # any weights (a model of its own: it is quantised below)
    ga.load_state_dict(m["sd"])
    gp = _plain_twin(env, K)
    try:
        for mode in ("bf16", "int8"):
            if mode == "int8":
                for g in (gz, ga, gp):
                    g.quantize_int8()
            want_f, want_l = host(_forward(env, gp, s, 0.8)), _loop(env, gp, s, TS4)
            assert np.isfinite(want_l).all() and not np.array_equal(want_l, s["img"])
            np.testing.assert_array_equal(host(_forward(env, gz, s, 0.8, cond)), want_f, err_msg=f"{mode}: forward, zero columns")
            np.testing.assert_array_equal(_loop(env, gz, s, TS4, cond), want_l, err_msg=f"{mode}: loop, zero columns")
            zero = np.zeros_like(cond)
            np.testing.assert_array_equal(host(_forward(env, ga, s, 0.8, zero)), want_f, err_msg=f"{mode}: forward, zero conditioning")
            np.testing.assert_array_equal(_loop(env, ga, s, TS4, zero), want_l, err_msg=f"{mode}: loop, zero conditioning")
            assert not np.array_equal(_loop(env, ga, s, TS4, cond), want_l)  # (the conditioning matters)
            if mode == "int8":
                assert not np.array_equal(want_l, _loop(env, m["gm"], s, TS4, zero))  # (it is the int8 model)
    finally:
        for g in (gz, ga, gp):
            g.close()


def test_e4m3_mode_zero_conditioning_is_the_plain_model(env):
    """x_embedder is no block linear: after quantize_fp8() the conditioned model at cond == 0 is still the plain e4m3 model, bit for bit, and a cond still matters"""
    d, s, m = env["d"], env["sets"]["ragged"], env["models"][384]
    ga = d.FluxModel(m["cfg"])
    ga.load_state_dict(m["sd"])
    gp = _plain_twin(env, 384)
    try:
        for g in (ga, gp):
            g.quantize_fp8()
        want = _loop(env, gp, s, TS4)
        assert np.isfinite(want).all() and not np.array_equal(want, _loop(env, m["gm"], s, TS4, np.zeros_like(s["cond"][384])))  # (it is the e4m3 model)
        np.testing.assert_array_equal(_loop(env, ga, s, TS4, np.zeros_like(s["cond"][384])), want)
        np.testing.assert_array_equal(host(_forward(env, ga, s, 0.8, np.zeros_like(s["cond"][384]))), host(_forward(env, gp, s, 0.8)))
        got = _loop(env, ga, s, TS4, s["cond"][384])
        assert np.isfinite(got).all() and not np.array_equal(got, want)
    finally:
        ga.close()
        gp.close()


@pytest.mark.parametrize("grid", ["aligned", "ragged"])
@pytest.mark.parametrize("K", WIDTHS)
def test_loop_is_the_chain_of_forward_control_and_the_euler_step_and_a_batch_is_its_single_runs(env, K, grid):
    torch, d, s, gm = env["torch"], env["d"], env["sets"][grid], env["models"][K]["gm"]
    cond = s["cond"][K]
    with _pinned(gm):
        both = _loop(env, gm, s, TS4, cond)
        assert np.isfinite(both).all()
        x = dev(s["img"]).clone()
        for i in range(4):
            pred = _forward(env, gm, s, TS4[i], cond, img=host(x))
            assert tuple(pred.shape) == (B, s["S"], 64)
            d.cfg_euler_step(x, pred, pred.clone(), 1.0, float(f32(TS4[i + 1] - TS4[i])))  # pos == neg: img + pred * dt, the plain loop's update bit for bit
        np.testing.assert_array_equal(both, host(x), err_msg="loop vs forward_control + Euler chain")
        for b in range(B):
            np.testing.assert_array_equal(_loop(env, gm, s, TS4, cond, sl=slice(b, b + 1)), both[b:b + 1], err_msg=f"sample {b}")
        assert not np.array_equal(both[0], both[1])
        # a bf16 conditioning holding the same values is the same loop
        got = host(gm.denoise(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(s["y"]), dev(env["g"]), TS4,
                              control=dev(bf16_round(cond), torch.bfloat16)))
        np.testing.assert_array_equal(got, _loop(env, gm, s, TS4, bf16_round(cond)))


@pytest.mark.parametrize("grid", ["aligned", "ragged"])
@pytest.mark.parametrize("K", WIDTHS)
def test_negative_equal_to_the_prompt_and_the_masks(env, K, grid):
    s, gm = env["sets"][grid], env["models"][K]["gm"]
    cond = s["cond"][K]
    with _pinned(gm):
        plain = _loop(env, gm, s, TS4, cond)
        np.testing.assert_array_equal(_loop(env, gm, s, TS4, cond, neg=(s["txt"], s["y"]), scale=SCALE), plain, err_msg="negative == prompt, scale 4")
        assert not np.array_equal(_loop(env, gm, s, TS4, cond, neg=(s["ntxt"], s["ny"]), scale=SCALE), plain)
    plain = _loop(env, gm, s, TS4, cond)  # (unpinned like the masked loops below: the same row count, the same modulation kernel)
    ones = _loop(env, gm, s, TS4, cond, x0=s["x0"], noise=s["img"], mask=np.ones_like(s["x0"]))
    np.testing.assert_array_equal(ones, plain)
    zeros = _loop(env, gm, s, TS4, cond, x0=s["x0"], noise=s["img"], mask=np.zeros_like(s["x0"]))
    np.testing.assert_array_equal(zeros, s["x0"])
    mixed = _loop(env, gm, s, TS4, cond, x0=s["x0"], noise=s["img"], mask=s["mask"])
    keep = s["mask"] == 0
    assert keep.any() and TS4[-1] == 0.0
    np.testing.assert_array_equal(mixed[keep], s["x0"][keep])
    assert not np.array_equal(mixed[~keep], s["x0"][~keep]) and not np.array_equal(mixed, plain)


# ------------------------------------------------------------------------------------------------ the entries at the ctypes level
def _inp(env, gm, s):
    torch = env["torch"]
    g = dev(np.full(s["img"].shape[0], 3.5, np.float32))
    return gm._inputs(None, dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), None, dev(s["y"]), g)


def _denoise_entry(env, gm, s, entry, ctl=None, cfg=None, blend=(None, None, None)):
    """one of the denoise entries on a copy of the set's image; returns (status, the copy afterwards)"""
    from diffusion_rs_amd import _lib as L
    torch, lib = env["torch"], gm.lib
    img = dev(s["img"]).clone()
    inp, keep = _inp(env, gm, s)
    ts = (C.c_double * 5)(*TS4)
    p, ip = [None if e is None else C.c_void_p(e.data_ptr()) for e in blend], C.c_void_p(img.data_ptr())
    ref = lambda x: None if x is None else C.byref(x)
    if entry == "control":
        rc = lib.fmi_flux_denoise_control(gm.h, C.byref(inp), ref(ctl), ref(cfg), ip, ts, 4, *p, None)
    elif entry == "cfg":
        rc = lib.fmi_flux_denoise_cfg(gm.h, C.byref(inp), None, ref(cfg), ip, ts, 4, *p, None)
    elif entry == "context":
        rc = lib.fmi_flux_denoise_context(gm.h, C.byref(inp), None, ip, ts, 4, *p, None)
    elif entry == "cached":
        sc = L.FluxStepCache(0.1, None, None, None)
        rc = lib.fmi_flux_denoise_cached(gm.h, C.byref(inp), None, ip, ts, 4, *p, C.byref(sc), None)
    elif entry == "inpaint":
        rc = lib.fmi_flux_denoise_inpaint(gm.h, C.byref(inp), ip, ts, 4, *p, None)
    else:
        rc = lib.fmi_flux_denoise(gm.h, C.byref(inp), ip, ts, 4, None)
    torch.cuda.synchronize()
    return rc, host(img)


@pytest.mark.parametrize("grid", ["aligned", "ragged"])
def test_null_control_and_null_cfg_on_a_plain_model_is_the_cfg_entry(env, grid):
    from diffusion_rs_amd import _lib as L
    torch, d, s = env["torch"], env["d"], env["sets"][grid]
    gp = d.FluxModel(SMALL_FLUX)
    gp.load_state_dict(d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0))
    try:
        ntxt, ny = dev(s["ntxt"], torch.bfloat16), dev(s["ny"])
        tc = L.FluxTrueCfg(C.c_void_p(ntxt.data_ptr()), L.BF16, C.c_void_p(ny.data_ptr()), L.F32, SCALE)
        for cfg in (None, tc):
            for blend in ((None, None, None), (dev(s["x0"]), dev(s["img"]), dev(s["mask"]))):
                rc, want = _denoise_entry(env, gp, s, "cfg", cfg=cfg, blend=blend)
                assert rc == 0
                rc, got = _denoise_entry(env, gp, s, "control", cfg=cfg, blend=blend)
                assert rc == 0
                np.testing.assert_array_equal(got, want)
                assert not np.array_equal(got, s["img"])
        # a control given to a model without conditioning channels is refused, the state untouched
        cond = dev(s["cond"][128])
        rc, after = _denoise_entry(env, gp, s, "control", ctl=L.FluxControl(C.c_void_p(cond.data_ptr()), L.F32))
        assert rc == L.ERR_INVALID
        np.testing.assert_array_equal(after.view(np.uint32), s["img"].view(np.uint32))
        with pytest.raises(ValueError, match="channel-conditioned model"):
            _loop(env, gp, s, TS4, s["cond"][128])
    finally:
        gp.close()


@pytest.mark.parametrize("K", WIDTHS)
def test_refusals_leave_the_state_untouched(env, K):
    from diffusion_rs_amd import _lib as L
    torch, d, s, gm = env["torch"], env["d"], env["sets"]["ragged"], env["models"][K]["gm"]
    cond = dev(s["cond"][K])
    cp = C.c_void_p(cond.data_ptr())
    good = L.FluxControl(cp, L.F32)

    def refused(code, entry, ctl=None, blend=(None, None, None)):
        rc, after = _denoise_entry(env, gm, s, entry, ctl=ctl, blend=blend)
        assert rc == code, (entry, rc, code)
        np.testing.assert_array_equal(after.view(np.uint32), s["img"].view(np.uint32))  # bit for bit

    refused(L.ERR_INVALID, "control", None)  # a null control
    refused(L.ERR_INVALID, "control", L.FluxControl(None, L.F32))  # a null cond
    refused(L.ERR_INVALID, "control", L.FluxControl(cp, L.F16))  # a dtype that is neither F32 nor BF16
    refused(L.ERR_INVALID, "control", L.FluxControl(cp, L.U8))
    x0 = dev(s["x0"])
    refused(L.ERR_INVALID, "control", good, (x0, None, x0))  # x0 / noise / mask in part
    for entry in ("denoise", "inpaint", "context", "cached", "cfg"):  # every existing entry refuses a conditioned model
        refused(L.ERR_INVALID, entry, blend=(x0, x0, x0) if entry == "inpaint" else (None, None, None))
    # ... and so do the forwards: pred_out stays as it was
    inp, keep = gm._inputs(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(np.full(B, 0.8, np.float32)), dev(s["y"]), dev(env["g"]))
    pred = torch.full(s["img"].shape, 7.0, device="cuda")
    pp = C.c_void_p(pred.data_ptr())
    assert gm.lib.fmi_flux_forward(gm.h, C.byref(inp), pp, None) == L.ERR_INVALID
    assert gm.lib.fmi_flux_forward_context(gm.h, C.byref(inp), None, pp, None) == L.ERR_INVALID
    assert gm.lib.fmi_flux_forward_control(gm.h, C.byref(inp), None, pp, None) == L.ERR_INVALID
    assert gm.lib.fmi_flux_forward_control(gm.h, C.byref(inp), C.byref(L.FluxControl(None, L.F32)), pp, None) == L.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((pred == 7.0).all())
    # under sequence parallelism a control is refused before anything runs (the exchange callback is never called: world 2 needs a second device)
    called = []
    cb = L.ALL_TO_ALL_FN(lambda *a: called.append(a) or 1)
    L.check(gm.lib.fmi_flux_set_sequence_parallel(gm.h, 0, 2, cb, None))
    try:
        refused(L.ERR_UNSUPPORTED, "control", good)
        assert gm.lib.fmi_flux_forward_control(gm.h, C.byref(inp), C.byref(good), pp, None) == L.ERR_UNSUPPORTED
    finally:
        L.check(gm.lib.fmi_flux_set_sequence_parallel(gm.h, 0, 1, L.ALL_TO_ALL_FN(), None))
    assert not called and bool((pred == 7.0).all())
    # the Python layer refuses the same, and a context or the step cache next to a control, before it reaches the library
    a = (dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(s["y"]), dev(env["g"]), TS4)
    with pytest.raises(ValueError, match="is required"):
        gm.denoise(*a)
    with pytest.raises(ValueError, match="control is"):
        gm.denoise(*a, control=cond[:, :, :32])
    with pytest.raises(ValueError, match="context="):
        gm.denoise(*a, control=cond, context=dev(s["img"]), context_ids=dev(s["ids"]))
    with pytest.raises(ValueError, match="step cache"):
        gm.denoise(*a, control=cond, cache_threshold=0.1)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        gm.denoise(*a, control=cond.to(torch.float16))
    rc, got = _denoise_entry(env, gm, s, "control", ctl=good)  # the model is as it was
    assert rc == 0
    np.testing.assert_array_equal(got, _loop(env, gm, s, TS4, s["cond"][K]))


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("grid", ["aligned", "ragged"])
@pytest.mark.parametrize("K", WIDTHS)
def test_forward_and_loop_match_the_oracle_composition_and_no_wrong_one(env, K, grid):
    """One evaluation within the project's 2e-2 and the final latents of the 4-step loop within its 3e-2 of the composed reference, and at most ONE THIRD as far
    from it as from each of the four wrong compositions, computed on the oracle itself.  Measured on an MI355X: see DESIGN.md 5."""
    s, m = env["sets"][grid], env["models"][K]
    om, cond = m["om"], s["cond"][K]
    got_f = host(_forward(env, m["gm"], s, 0.8, cond))
    err_f = rel_l2(got_f, CR.forward(om, s["img"], cond, s["ids"], s["txt"], s["txt_ids"], np.full(B, 0.8, np.float32), s["y"], env["g"]))
    got = _loop(env, m["gm"], s, TS4, cond)
    ref = lambda variant=None: CR.control_loop(om, s["img"], cond, s["ids"], s["txt"], s["txt_ids"], s["y"], env["g"], TS4, variant=variant)
    err = rel_l2(got, ref())
    print(f"control K={K} {grid} (B=2, S={s['S']}, T=32): forward rel-L2 {err_f:.3e}; 4-step loop final latents rel-L2 {err:.3e} vs the correct composition")
    far = {v: rel_l2(got, ref(v)) for v in CR.VARIANTS}
    for v, dist in far.items():
        print(f"    {v}: rel-L2 {dist:.3e} ({dist / err:.1f} x)")
    assert np.isfinite(got_f).all() and err_f <= 2e-2
    assert np.isfinite(got).all() and err <= 3e-2
    for v, dist in far.items():
        assert err <= dist / 3, v


def test_loop_with_cfg_and_a_mixed_mask_matches_the_oracle_composition(env):
    s, m = env["sets"]["ragged"], env["models"][384]
    om, cond = m["om"], s["cond"][384]
    got = _loop(env, m["gm"], s, TS4, cond, neg=(s["ntxt"], s["ny"]), scale=SCALE, x0=s["x0"], noise=s["img"], mask=s["mask"])
    ref = lambda variant=None: CR.control_loop(om, s["img"], cond, s["ids"], s["txt"], s["txt_ids"], s["y"], env["g"], TS4, neg_txt=s["ntxt"], neg_y=s["ny"],
                                               scale=SCALE, x0=s["x0"], noise=s["img"], mask=s["mask"], variant=variant)
    err = rel_l2(got, ref())
    print(f"control K=384 ragged with CFG (scale 4) and a mixed mask: final latents rel-L2 {err:.3e} vs the correct composition")
    far = {v: rel_l2(got, ref(v)) for v in CR.VARIANTS}
    for v, dist in far.items():
        print(f"    {v}: rel-L2 {dist:.3e} ({dist / err:.1f} x)")
    assert np.isfinite(got).all() and err <= 3e-2
    for v, dist in far.items():
        assert err <= dist / 3, v
    np.testing.assert_array_equal(got[s["mask"] == 0], s["x0"][s["mask"] == 0])


# ------------------------------------------------------------------------------------------------ the pipeline
H, W, STEPS, GUIDANCE, TP, SEED = 128, 192, 4, 3.5, 24, 11
VSCALE, VSHIFT = f32(SMALL_VAE["scaling_factor"]), f32(SMALL_VAE["shift_factor"])


@pytest.fixture(scope="module", params=WIDTHS)
def pipe_env(request):
    """the synthetic source without text encoders at the small configuration with a wide embedder, holding the weights the oracle holds"""
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    K = request.param
    cfg = _cfg(K)
    sd = d.synth.flux_state_dict_numpy(cfg, seed=0)
    vsd = d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0, encoder=True)
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=cfg, vae_cfg=SMALL_VAE))
    pipe.flux.load_state_dict(sd)
    pipe.vae.load_state_dict(vsd)
    om, ov = orc.Flux(CR.oracle_cfg(cfg)), orc.Vae(SMALL_VAE)
    om.load(CR.oracle_state_dict(sd, cfg))
    ov.load(vsd)
    rng = np.random.default_rng(51)
    J, P = SMALL_FLUX["joint_attention_dim"], SMALL_FLUX["pooled_projection_dim"]
    t5 = bf16_round(rng.standard_normal((B, TP, J)).astype(np.float32))
    clip = rng.standard_normal((B, P)).astype(np.float32)
    image_u8 = rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)  # (H,W,3): a picture of 8x8 blocks
    pmask = (rng.random((H // 16, W // 16)) < 0.5).repeat(16, 0).repeat(16, 1)  # (H,W) bool, 1 = fill
    params = d.DiffusionGenerationParams(height=H, width=W, num_steps=STEPS, guidance_scale=GUIDANCE)
    ctl = dict(control_image=image_u8, **(dict(control_mask=pmask) if K == 384 else {}))
    return dict(torch=torch, d=d, orc=orc, K=K, pipe=pipe, om=om, ov=ov, t5=t5, clip=clip, params=params, image_u8=image_u8, pmask=pmask, ctl=ctl,
                emb=(dev(t5, torch.bfloat16), dev(clip)))


def _oracle_condition(env):
    """preprocess (numpy) -> [mask] -> Vae.encode (posterior mean) -> affine -> pack -> [mask channels], one row"""
    orc, ov = env["orc"], env["ov"]
    img = ((env["image_u8"].transpose(2, 0, 1)[None].astype(np.float32) + f32(0.5)) / f32(127.5) - f32(1)).astype(np.float32)
    m = env["pmask"][None].astype(np.float32)
    if env["K"] == 384:
        img = CR.mask_image(img, m)
    lat = orc.pack_latents(((ov.encode(img, noise=None) - VSHIFT) * VSCALE).astype(np.float32))[0]
    return CR.fill_condition(lat, m) if env["K"] == 384 else lat


def test_pipeline_control_matches_the_oracle_pipeline(pipe_env):
    env = pipe_env
    torch, orc, om, ov, pipe, K = env["torch"], env["orc"], env["om"], env["ov"], env["pipe"], env["K"]
    u8, final = pipe.forward(["a", "b"], env["params"], output="tensor", seed=SEED, embeddings=env["emb"], return_latents=True, **env["ctl"])
    assert tuple(final.shape) == (B, (H // 16) * (W // 16), 64) and tuple(u8.shape) == (B, 3, H, W)
    # the oracle pipeline, encoder included: the condition, Philox noise -> pack -> the composed control loop -> unpack -> decode -> u8
    cond = np.repeat(_oracle_condition(env), B, 0)
    assert cond.shape == (B, (H // 16) * (W // 16), K - 64)
    h, w = H // 8, W // 8
    noise, ids = orc.pack_latents(orc.randn(16 * h * w, B, SEED).reshape(B, 16, h, w).astype(np.float32))
    sched = pipe.scheduler
    mu = orc.calculate_shift(noise.shape[1], sched.base_image_seq_len, sched.max_image_seq_len, sched.base_shift, sched.max_shift)
    ts = orc.get_timesteps(STEPS, sched.use_dynamic_shifting, mu, sched.shift)
    ref = CR.control_loop(om, noise, cond, ids, env["t5"], np.zeros((B, TP, 3), np.float32), env["clip"], np.full(B, GUIDANCE, np.float32), ts)
    err = rel_l2(host(final), ref)
    z = orc.unpack_latents(ref, 16, h, w) * f32(1.0 / SMALL_VAE["scaling_factor"]) + VSHIFT
    ref_u8 = orc.postprocess_u8(ov.decode(z.astype(np.float32)))
    diff = np.abs(u8.cpu().numpy().astype(np.int32) - ref_u8.astype(np.int32))
    share, worst = float((diff <= 2).mean()), int(diff.max())
    print(f"pipeline control K={K} (128 x 192, {STEPS} steps, B=2): final latents rel-L2 {err:.3e}; u8 within 2 on {share:.4f}, max |d| {worst}")
    assert err <= 3e-2
    assert share >= 0.99
    # the GPU's own condition is the oracle's to the VAE encoder's precision, and exact in the mask channels
    with pipe._lock:
        gcond = host(pipe._control_condition(pipe._control(env["ctl"]["control_image"], env["ctl"].get("control_mask"), env["params"], None, None), B))
    assert rel_l2(gcond[:, :, :64], cond[:, :, :64]) <= 2e-2
    np.testing.assert_array_equal(gcond[:, :, 64:], cond[:, :, 64:])
    # the f32 form of the same picture is the same request; another picture is another result
    f32_image = env["d"].preprocess_u8(dev(env["image_u8"][None]), interleaved=True)
    again = pipe.forward(["a", "b"], env["params"], output="tensor", seed=SEED, embeddings=env["emb"], **dict(env["ctl"], control_image=f32_image))
    assert torch.equal(again, u8)
    other = pipe.forward(["a", "b"], env["params"], output="tensor", seed=SEED, embeddings=env["emb"], **dict(env["ctl"], control_image=255 - env["image_u8"]))
    assert not torch.equal(other, u8)


def test_pipeline_five_prompts_run_as_chunks_of_four_and_one_and_combine_with_image_and_mask(pipe_env):
    env = pipe_env
    torch, pipe = env["torch"], env["pipe"]
    prompts = ["a", "b", "c", "d", "e"]
    kw = dict(output="tensor", seed=SEED, negative_prompt="x", true_cfg_scale=4.0, **env["ctl"])
    whole = pipe.forward(prompts, env["params"], **kw)
    first = pipe.forward(prompts[:4], env["params"], **kw)
    last = pipe.forward(prompts[4:], env["params"], first_sample=4, **kw)
    assert tuple(whole.shape) == (5, 3, H, W)
    assert torch.equal(whole, torch.cat([first, last], 0))
    assert not torch.equal(first, pipe.forward(prompts[:4], env["params"], output="tensor", seed=SEED, **env["ctl"]))  # the negative prompt matters
    # image= / strength= / mask= keep their meaning next to the control: kept latents end as the source's
    src = env["image_u8"][::-1].copy()
    keep_right = np.zeros((H, W), np.float32)
    keep_right[:, :W // 2] = 1.0  # repaint the left half
    u8, final = pipe.forward(prompts[:2], env["params"], output="tensor", seed=SEED, image=src, strength=0.75, mask=keep_right, return_latents=True, **env["ctl"])
    gx0, _ = env["d"].encode_latents(pipe.vae.encode(env["d"].preprocess_u8(dev(src[None]), interleaved=True)), pipe.vae.scale_factor(), pipe.vae.shift_factor())
    lm = host(env["d"].latent_mask(dev(keep_right[None]), 16))[0]
    got = host(final)
    for b in range(2):
        np.testing.assert_array_equal(got[b][lm == 0], host(gx0)[0][lm == 0])
        assert not np.array_equal(got[b][lm == 1], host(gx0)[0][lm == 1])


def test_pipeline_error_cases(pipe_env):
    env = pipe_env
    d, pipe, K = env["d"], env["pipe"], env["K"]
    run = lambda **kw: pipe.forward(["a"], env["params"], output="tensor", seed=SEED, **kw)
    with pytest.raises(ValueError, match="control_image= is required"):
        run()
    with pytest.raises(ValueError, match="reference="):
        run(reference=env["image_u8"], **env["ctl"])
    with pytest.raises(ValueError, match="step cache"):
        run(cache_threshold=0.1, **env["ctl"])
    with pytest.raises(ValueError, match="control_image must be"):
        run(**dict(env["ctl"], control_image=env["image_u8"][:64]))
    if K == 384:
        with pytest.raises(ValueError, match="needs control_mask="):
            run(control_image=env["image_u8"])
        with pytest.raises(ValueError, match="control_mask must be"):
            run(control_image=env["image_u8"], control_mask=env["pmask"][:64])
    else:
        with pytest.raises(ValueError, match="goes with a Fill model"):
            run(control_image=env["image_u8"], control_mask=env["pmask"])
        with pytest.raises(ValueError, match="multiples of 16"):
            pipe.forward(["a"], d.DiffusionGenerationParams(height=120, width=W, num_steps=STEPS, guidance_scale=GUIDANCE), output="tensor",
                         control_image=env["image_u8"][:120])
        # a plain model takes no control
        plain = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=SMALL_FLUX, vae_cfg=SMALL_VAE))
        with pytest.raises(ValueError, match="need a channel-conditioned model"):
            plain.forward(["a"], env["params"], output="tensor", control_image=env["image_u8"])
        with pytest.raises(ValueError, match="need a channel-conditioned model"):
            plain.forward(["a"], env["params"], output="tensor", control_mask=env["pmask"])
    pipe._sp = object()
    try:
        with pytest.raises(ValueError, match="sequence parallelism"):
            run(**env["ctl"])
    finally:
        pipe._sp = None
    assert tuple(run(**env["ctl"]).shape) == (1, 3, H, W)  # the pipeline is as it was


def test_int8_pipeline_calibrates_with_the_control(pipe_env):
    """ModelDType.I8: the first request's calibration forwards take the control; the model is quantised afterwards and the request runs in int8 mode"""
    env = pipe_env
    d, torch = env["d"], env["torch"]
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=_cfg(env["K"]), vae_cfg=SMALL_VAE), dtype=d.ModelDType.I8)
    assert pipe._int8_pending
    u8 = pipe.forward(["a", "b"], env["params"], output="tensor", seed=SEED, **env["ctl"])
    assert not pipe._int8_pending and tuple(u8.shape) == (B, 3, H, W)
    with pytest.raises(d.FmiError):  # quantised: the weights are fixed
        pipe.flux.set_tensor("x_embedder.weight", np.zeros((256, env["K"]), np.float32))
    assert torch.equal(u8, pipe.forward(["a", "b"], env["params"], output="tensor", seed=SEED, **env["ctl"]))


# ------------------------------------------------------------------------------------------------ a checkpoint directory
def _write_diffusers_dir(root, class_name, cfg, sd, vsd):
    """a diffusers directory as tests/test_gpu_pipeline.py writes it, with the pipeline class and the transformer's in_channels / out_channels of a conditioned checkpoint"""
    import json
    import os
    import torch
    from safetensors.torch import save_file
    for sub in ("transformer", "vae", "scheduler"):
        os.makedirs(os.path.join(root, sub))
    json.dump({"_class_name": class_name}, open(os.path.join(root, "model_index.json"), "w"))
    json.dump({"_class_name": "FlowMatchEulerDiscreteScheduler", "base_image_seq_len": 256, "base_shift": 0.5, "max_image_seq_len": 4096,
               "max_shift": 1.15, "shift": 3.0, "use_dynamic_shifting": True}, open(os.path.join(root, "scheduler", "scheduler_config.json"), "w"))
    json.dump({k: cfg[k] for k in ("in_channels", "out_channels", "pooled_projection_dim", "joint_attention_dim", "num_attention_heads", "num_layers",
                                   "num_single_layers", "guidance_embeds")}, open(os.path.join(root, "transformer", "config.json"), "w"))
    json.dump({k: SMALL_VAE[k] for k in SMALL_VAE}, open(os.path.join(root, "vae", "config.json"), "w"))
    save_file({k: torch.from_numpy(v).to(torch.bfloat16) for k, v in sd.items()}, os.path.join(root, "transformer", "diffusion_pytorch_model.safetensors"))
    save_file({k: torch.from_numpy(v) for k, v in vsd.items()}, os.path.join(root, "vae", "diffusion_pytorch_model.safetensors"))


def test_a_fill_checkpoint_directory_loads_and_is_the_synthetic_pipeline(pipe_env, tmp_path):
    """model_index.json says FluxFillPipeline / FluxControlPipeline, transformer/config.json in_channels 384 / 128 and out_channels 64: the loaded pipeline gives the
    images of the fixture's pipeline, which holds the same weights; a class that disagrees with the channels is refused."""
    env = pipe_env
    d, torch, K = env["d"], env["torch"], env["K"]
    cfg = _cfg(K)
    sd = d.synth.flux_state_dict_numpy(cfg, seed=0)
    vsd = d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0, encoder=True)
    good, bad = ("FluxFillPipeline", "FluxControlPipeline") if K == 384 else ("FluxControlPipeline", "FluxFillPipeline")
    root = str(tmp_path / "tiny")
    _write_diffusers_dir(root, good, cfg, sd, vsd)
    pipe = d.Pipeline(d.ModelSource.ModelId(root))
    assert pipe.flux.cond_channels == K - 64 and pipe.flux.state_channels == 64 and not pipe.flux.missing()
    kw = dict(output="tensor", seed=SEED, embeddings=env["emb"], **env["ctl"])
    assert torch.equal(pipe.forward(["a", "b"], env["params"], **kw), env["pipe"].forward(["a", "b"], env["params"], **kw))
    for cls in (bad, "FluxPipeline"):
        other = str(tmp_path / cls)
        _write_diffusers_dir(other, cls, cfg, sd, vsd)
        with pytest.raises(ValueError, match="conditioning channels"):
            d.Pipeline(d.ModelSource.ModelId(other))
    with pytest.raises(ValueError, match="Only FluxPipeline is supported"):
        unknown = str(tmp_path / "unknown")
        _write_diffusers_dir(unknown, "FluxControlNetPipeline", cfg, sd, vsd)
        d.Pipeline(d.ModelSource.ModelId(unknown))
