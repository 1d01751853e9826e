"""FLUX ControlNets: fmi_flux_create_controlnet, fmi_flux_forward_controlnet / fmi_flux_denoise_controlnet, the injection kernel
fmi_add_scaled_rows_bf16 and the pipeline's controlnet_image=.

The injection kernel is compared bit for bit with numpy (one rounded product, one rounded sum).  What the semantics promise exactly is compared as values (==):
scale 0 or step scales all 0 IS the plain loop, a net whose controlnet_* tensors are zero IS the plain model, the loop IS the chain of forward_controlnet and
the Euler step, a batch IS its single-sample runs, step_scales [1,1,0,0] IS two conditioned steps followed by the plain loop, a NULL ControlNet through the new
entry IS fmi_flux_denoise_with.  Against the composed CPU reference (tests/controlnet_ref.py) the ControlNet's samples and one conditioned evaluation are within
the project's 2e-2, the 4-step loop within its 3e-2, and the loop lies at most a third as far from the correct composition as from each wrong one — which
tests/test_host_controlnet.py shows to be at least 9e-2 away from it.

Main model SMALL_FLUX with 5 double and 3 single blocks; nets 2+2 (kd = 3, ks = 2) and 2+0; B = 2, T = 32; token grids 6x4 (aligned) and 5x7 (ragged)."""
import ctypes as C

import numpy as np
import pytest

from tests import controlnet_ref as CR
from tests.util import SMALL_VAE, bf16_round, dev, host, rel_l2

pytestmark = pytest.mark.gpu

f32 = np.float32
B, T, TS4 = CR.B, CR.T, CR.TS4
D = 256
GRID_CAP_ITEMS = 256 * 8 * 256  # at most 256 * 8 blocks of 256 threads; one item (8 elements) more and the grid-stride loop wraps


# ------------------------------------------------------------------------------------------------ the injection kernel, bit for bit
def _src(rng, Bn, rows):
    """bf16 values (as f32) with signed zeros and the operands of ties of the f32 sum: next to x = 1, 2^-24 is half an ulp (to even: down) and 3 * 2^-24 one and a
    half (to even: up)"""
    s = bf16_round(rng.standard_normal((Bn, rows, D)).astype(np.float32) * f32(2))
    s[0, 0, :4] = [0.0, -0.0, 2.0 ** -24, 3 * 2.0 ** -24]
    s[-1, -1, -4:] = [-0.0, 0.0, -(2.0 ** -24), 1.0]
    return s


def _x(rng, Bn, Lx):
    x = rng.standard_normal((Bn, Lx, D)).astype(np.float32)
    x[0, :, :4] = [1.0, -0.0, 1.0, 1.0]  # (row 0 of the window meets the ties and the zeros above: -0 + 1 * -0 stays -0)
    x[-1, :, -4:] = [-0.0, 0.0, -1.0, 0.5]
    return x


def _placed(torch, a, misaligned):
    """a copy of `a` on the device: on a 16-byte boundary, or one float past it (the scalar path)"""
    if not misaligned:
        t = dev(a)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    assert v.data_ptr() % 16 == 4
    return v.view(a.shape)


@pytest.mark.parametrize("rows", [24, 35, 8200])
def test_add_scaled_rows_bf16_is_numpy_bit_for_bit_and_touches_nothing_else(rows):
    import torch
    import diffusion_rs_amd as d
    rng = np.random.default_rng(rows)
    big = rows == 8200
    if big:
        assert B * rows * (D // 8) > GRID_CAP_ITEMS  # beyond the grid cap: the grid-stride loop wraps
    src = _src(rng, B, rows)
    sb = dev(src, torch.bfloat16)
    np.testing.assert_array_equal(host(sb), src)
    # contiguous: the image stream of the double blocks; strided: rows [T, T + rows) of every (T + rows + 3)-row sample (a batch stride and a row offset)
    for Lx, row0 in ((rows, 0),) if big else ((rows, 0), (T + rows + 3, T)):
        x = _x(rng, B, Lx)
        for misaligned in (False,) if big else (False, True):
            for scale in (0.7,) if big else (0.7, 1.0, -2.0):
                want = x.copy()
                want[:, row0:row0 + rows] = CR.add_scaled_rows(x[:, row0:row0 + rows], src, scale)
                xd = _placed(torch, x, misaligned)
                out = d.add_scaled_rows_bf16(xd, sb, scale, row0=row0)
                assert out is xd
                np.testing.assert_array_equal(host(xd).view(np.uint32), want.view(np.uint32), err_msg=f"Lx {Lx} row0 {row0} misaligned {misaligned} scale {scale}")
    if not big:  # the ties and the zeros did what they must at scale 1 (contiguous): 1 + 2^-24 -> 1, 1 + 3 * 2^-24 -> 1 + 2^-22, -0 + -0 -> -0
        x = _x(rng, B, rows)
        got = host(d.add_scaled_rows_bf16(dev(x), sb, 1.0))
        assert got[0, 0, 0] == 1.0 and np.signbit(got[0, 0, 1]) and got[0, 0, 2] == 1.0 and got[0, 0, 3] == f32(1.0) + f32(2.0 ** -22)
    with pytest.raises(ValueError, match="does not fit"):
        d.add_scaled_rows_bf16(dev(_x(rng, B, rows)), sb, 1.0, row0=1)
    with pytest.raises(TypeError):
        d.add_scaled_rows_bf16(dev(_x(rng, B, rows)), dev(src), 1.0)  # an f32 source


# ------------------------------------------------------------------------------------------------ the models
@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    gm = d.FluxModel(CR.MAIN_CFG)
    gm.load_state_dict(CR.main_state_dict())
    nets = {}
    for name in CR.NETS:
        gn = d.FluxControlNetModel(CR.net_cfg(name))
        gn.load_state_dict(CR.net_state_dict(name))
        nets[name] = gn
    return dict(torch=torch, d=d, gm=gm, nets=nets)


def _loop(env, gm, s, ts, net=None, cond=None, scale=CR.CN_SCALE, step_scales=None, neg=None, blend=False, sl=slice(None), img=None):
    torch = env["torch"]
    kw = {}
    if net is not None:
        kw.update(controlnet=net, controlnet_cond=dev((s["cond"] if cond is None else cond)[sl]), controlnet_scale=scale, controlnet_step_scales=step_scales)
    if neg is not None:
        kw.update(negative_txt=dev(neg[0][sl], torch.bfloat16), negative_y=dev(neg[1][sl]), true_cfg_scale=CR.CFG_SCALE)
    if blend:
        kw.update(x0=dev(s["x0"][sl]), noise=dev(s["img"][sl]), mask=dev(s["mask"][sl]))
    return host(gm.denoise(dev((s["img"] if img is None else img)[sl]), dev(s["ids"][sl]), dev(s["txt"][sl], torch.bfloat16), dev(s["txt_ids"][sl]), dev(s["y"][sl]),
                           dev(s["g"][sl]), ts, **kw))


def _forward(env, gm, s, t, net=None, scale=CR.CN_SCALE, img=None):
    torch = env["torch"]
    kw = {} if net is None else dict(controlnet=net, controlnet_cond=dev(s["cond"]), controlnet_scale=scale)
    return gm.forward(dev(s["img"] if img is None else img), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(np.full(B, t, np.float32)),
                      dev(s["y"]), dev(s["g"]), **kw)


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


def test_the_handle_kind_names_and_sizes(env):
    d, gm = env["d"], env["gm"]
    assert gm.lib.fmi_flux_is_controlnet(gm.h) == 0
    for name, gn in env["nets"].items():
        nd, ns = CR.NETS[name]
        assert gn.lib.fmi_flux_is_controlnet(gn.h) == 1 and gn.missing() == []
        w = gn.get_tensor("controlnet_blocks.1.weight")
        np.testing.assert_array_equal(host(w), CR.net_state_dict(name)["controlnet_blocks.1.weight"])
        np.testing.assert_array_equal(host(gn.get_tensor("controlnet_x_embedder.bias")), CR.net_state_dict(name)["controlnet_x_embedder.bias"])
        with pytest.raises(d.FmiError, match="unknown tensor name"):
            gn.set_tensor("proj_out.weight", np.zeros((64, D), np.float32))
        with pytest.raises(d.FmiError, match="unknown tensor name"):
            gn.set_tensor(f"controlnet_single_blocks.{ns}.weight", np.zeros((D, D), np.float32))
    fresh = d.FluxControlNetModel(CR.net_cfg("2+0"))
    try:
        assert "controlnet_blocks.0.weight" in fresh.missing() and "controlnet_x_embedder.bias" in fresh.missing() and "proj_out.weight" not in fresh.missing()
    finally:
        fresh.close()


@pytest.mark.parametrize("grid", list(CR.GRIDS))
@pytest.mark.parametrize("net", list(CR.NETS))
def test_samples_against_the_reference(env, net, grid):
    torch, gn, s = env["torch"], env["nets"][net], CR.inputs(grid)
    t = np.full(B, 0.8, np.float32)
    want_d, want_s = CR.controlnet_samples(CR.net_oracle(net), CR.net_state_dict(net), CR.net_cfg(net), s["img"], s["cond"], s["ids"], s["txt"], s["txt_ids"], t, s["y"], s["g"])
    before = gn.size_in_bytes()
    got_d, got_s = gn.eval(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(t), dev(s["y"]), dev(s["g"]), cond=dev(s["cond"]))
    assert len(got_d) == len(want_d) == CR.NETS[net][0] and len(got_s) == len(want_s) == CR.NETS[net][1]
    for kind, got, want in (("double", got_d, want_d), ("single", got_s, want_s)):
        for i, (g_, w_) in enumerate(zip(got, want)):
            g_ = host(g_)
            err = rel_l2(g_, w_)
            print(f"{net} {grid}: {kind} sample {i}: rel-L2 {err:.3e}")
            assert g_.shape == (B, s["S"], D) and err <= 2e-2, (kind, i, err)
            np.testing.assert_array_equal(g_, bf16_round(g_))  # the samples are stored as bf16
    assert gn.size_in_bytes() >= before  # (the sample buffers are reported)
    assert gn.size_in_bytes() >= sum(CR.NETS[net]) * B * s["S"] * D * 2


@pytest.mark.parametrize("mode", ["plain", "cfg", "blend"])
@pytest.mark.parametrize("grid", list(CR.GRIDS))
@pytest.mark.parametrize("net", list(CR.NETS))
def test_forward_and_loop_against_the_reference_and_its_wrong_variants(env, net, grid, mode):
    gm, gn, s = env["gm"], env["nets"][net], CR.inputs(grid)
    if mode == "plain":  # one conditioned evaluation
        t = np.full(B, 0.8, np.float32)
        want = CR.conditioned_forward(CR.main_oracle(), CR.main_state_dict(), CR.MAIN_CFG, CR.net_oracle(net), CR.net_state_dict(net), CR.net_cfg(net), s["img"], s["cond"],
                                      s["ids"], s["txt"], s["txt_ids"], t, s["y"], s["g"], CR.CN_SCALE)
        err = rel_l2(host(_forward(env, gm, s, 0.8, gn)), want)
        print(f"{net} {grid}: conditioned forward rel-L2 {err:.3e}")
        assert err <= 2e-2, err
    got = _loop(env, gm, s, TS4, gn, neg=(s["ntxt"], s["ny"]) if mode == "cfg" else None, blend=mode == "blend")
    correct = rel_l2(got, CR.loop_reference(net, grid, mode))
    print(f"{net} {grid} {mode}: 4-step loop rel-L2 {correct:.3e}")
    assert correct <= 3e-2, correct
    for v in CR.VARIANTS:
        if (v == "single_into_txt_rows" and CR.NETS[net][1] == 0) or (v == "neg_uses_pos_text" and mode != "cfg"):
            continue  # (there the variant IS the correct loop: tests/test_host_controlnet.py)
        wrong = rel_l2(got, CR.loop_reference(net, grid, mode, v))
        print(f"{net} {grid} {mode}: distance to {v}: {wrong:.3e}")
        assert 3 * correct <= wrong, (v, correct, wrong)


# ------------------------------------------------------------------------------------------------ the exact promises
@pytest.mark.parametrize("grid", list(CR.GRIDS))
def test_scale_zero_and_zero_step_scales_are_the_plain_loop(env, grid):
    gm, gn, s = env["gm"], env["nets"]["2+2"], CR.inputs(grid)
    plain = _loop(env, gm, s, TS4)
    assert np.isfinite(plain).all() and not np.array_equal(plain, s["img"])
    before = gn.size_in_bytes()
    assert (_loop(env, gm, s, TS4, gn, scale=0.0) == plain).all()
    assert (_loop(env, gm, s, TS4, gn, step_scales=[0, 0, 0, 0]) == plain).all()
    assert (_loop(env, gm, s, TS4, gn, scale=-0.0) == plain).all()
    assert (host(_forward(env, gm, s, 0.8, gn, scale=0.0)) == host(_forward(env, gm, s, 0.8))).all()
    assert gn.size_in_bytes() == before  # (nothing of the ControlNet was prepared)
    assert not np.array_equal(_loop(env, gm, s, TS4, gn), plain)  # (the ControlNet matters)
    neg = (s["ntxt"], s["ny"])
    assert (_loop(env, gm, s, TS4, gn, scale=0.0, neg=neg, blend=True) == _loop(env, gm, s, TS4, neg=neg, blend=True)).all()


@pytest.mark.parametrize("net", list(CR.NETS))
def test_a_net_with_zero_controlnet_tensors_is_the_plain_model(env, net):
    d, gm, s = env["d"], env["gm"], CR.inputs("ragged")
    sd = {k: (np.zeros_like(v) if k.startswith("controlnet_blocks") or k.startswith("controlnet_single_blocks") else v) for k, v in CR.net_state_dict(net).items()}
    gz = d.FluxControlNetModel(CR.net_cfg(net))  # zero-initialised zero-linears, weights and biases: what a ControlNet is before training
    gz.load_state_dict(sd)
    ga = d.FluxControlNetModel(CR.net_cfg(net))  # every controlnet_* tensor zero, the control embedder included
    ga.load_state_dict({k: (np.zeros_like(v) if k.startswith("controlnet_") else v) for k, v in CR.net_state_dict(net).items()})
    try:
        want_f, want_l = host(_forward(env, gm, s, 0.8)), _loop(env, gm, s, TS4)
        for g in (gz, ga):
            assert (host(_forward(env, gm, s, 0.8, g)) == want_f).all()
            assert (_loop(env, gm, s, TS4, g) == want_l).all()
            assert (_loop(env, gm, s, TS4, g, scale=-2.0, neg=(s["ntxt"], s["ny"])) == _loop(env, gm, s, TS4, neg=(s["ntxt"], s["ny"]))).all()
    finally:
        gz.close()
        ga.close()


@pytest.mark.parametrize("grid", list(CR.GRIDS))
@pytest.mark.parametrize("net", list(CR.NETS))
def test_loop_is_the_chain_of_forward_controlnet_and_a_batch_is_its_single_runs(env, net, grid):
    torch, d, gm, gn, s = env["torch"], env["d"], env["gm"], env["nets"][net], CR.inputs(grid)
    with _pinned(gm, gn):
        both = _loop(env, gm, s, TS4, gn)
        assert np.isfinite(both).all()
        x = dev(s["img"]).clone()
        for i in range(4):
            pred = _forward(env, gm, s, TS4[i], gn, img=host(x))
            d.cfg_euler_step(x, pred, pred.clone(), 1.0, float(f32(TS4[i + 1] - TS4[i])))  # pos == neg: img + pred * dt, the plain loop's update bit for bit
        assert (both == host(x)).all(), "loop vs forward_controlnet + Euler chain"
        for b in range(B):
            assert (_loop(env, gm, s, TS4, gn, sl=slice(b, b + 1)) == both[b:b + 1]).all(), f"sample {b}"
        assert not np.array_equal(both[0], both[1])
        # a bf16 cond holding the same values is the same loop
        got = host(gm.denoise(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(s["y"]), dev(s["g"]), TS4, controlnet=gn,
                              controlnet_cond=dev(bf16_round(s["cond"]), torch.bfloat16), controlnet_scale=CR.CN_SCALE))
        assert (got == _loop(env, gm, s, TS4, gn, cond=bf16_round(s["cond"]))).all()
        # step_scales [1,1,0,0] IS two conditioned steps followed by the plain loop on the remaining schedule
        two = _loop(env, gm, s, TS4[:3], gn)
        assert (_loop(env, gm, s, TS4, gn, step_scales=[1, 1, 0, 0]) == _loop(env, gm, s, TS4[2:], img=two)).all()
        # and a step scale is a factor of the scale: 0.5 * [2, 2, 2, 2] is the scale 1 loop (0.5 * 2 is exact)
        assert (_loop(env, gm, s, TS4, gn, scale=0.5, step_scales=[2, 2, 2, 2]) == _loop(env, gm, s, TS4, gn, scale=1.0)).all()


def _inp(env, gm, s):
    torch = env["torch"]
    return gm._inputs(None, dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), None, dev(s["y"]), dev(s["g"]))


def _entry(env, gm, s, cn=None, opts=None, with_entry=False, n_steps=4):
    """fmi_flux_denoise_controlnet (or fmi_flux_denoise_with) on a copy of the set's image; returns (status, the copy afterwards)"""
    img = dev(s["img"]).clone()
    inp, keep = _inp(env, gm, s)
    ts = (C.c_double * 5)(*TS4)
    st = torch_stream()
    if with_entry:
        rc = gm.lib.fmi_flux_denoise_with(gm.h, C.byref(inp), C.byref(opts) if opts is not None else None, C.c_void_p(img.data_ptr()), ts, n_steps, st)
    else:
        rc = gm.lib.fmi_flux_denoise_controlnet(gm.h, C.byref(inp), C.byref(opts) if opts is not None else None, C.byref(cn) if cn is not None else None,
                                                C.c_void_p(img.data_ptr()), ts, n_steps, st)
    return rc, host(img)


def torch_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cn(env, net, s, scale=CR.CN_SCALE, cond="default", dtype=None, step_scales=None):
    from diffusion_rs_amd import _lib as L
    c = dev(s["cond"]) if isinstance(cond, str) else cond
    ss = None if step_scales is None else (C.c_float * len(step_scales))(*step_scales)
    return L.FluxControlNet(net.h if net is not None else None, C.c_void_p(c.data_ptr()) if c is not None else None, L.F32 if dtype is None else dtype, scale, ss), (c, ss)


def test_null_controlnet_through_the_new_entry_is_denoise_with(env):
    from diffusion_rs_amd import _lib as L
    gm, s = env["gm"], CR.inputs("ragged")
    rc_a, a = _entry(env, gm, s)
    rc_b, b = _entry(env, gm, s, with_entry=True)
    assert rc_a == rc_b == 0 and (a == b).all() and (a == _loop(env, gm, s, TS4)).all()
    x0, noise, mask = dev(s["x0"]), dev(s["img"]), dev(s["mask"])
    opts = L.FluxDenoiseOptions(None, None, None, None, C.c_void_p(x0.data_ptr()), C.c_void_p(noise.data_ptr()), C.c_void_p(mask.data_ptr()))
    rc_a, a = _entry(env, gm, s, opts=opts)
    rc_b, b = _entry(env, gm, s, opts=opts, with_entry=True)
    assert rc_a == rc_b == 0 and (a == b).all() and (a == _loop(env, gm, s, TS4, blend=True)).all()
    bad = L.FluxDenoiseOptions(None, None, None, None, C.c_void_p(x0.data_ptr()), None, None)  # the same error, too
    assert _entry(env, gm, s, opts=bad)[0] == _entry(env, gm, s, opts=bad, with_entry=True)[0] == L.ERR_INVALID


def test_int8_main_model_accepts_a_controlnet(env):
    """the main model in int8 mode: the injection touches only its f32 stream.  The conditioned loop stays within the 8-bit bar of its own plain run's distance: as
    far from the conditioned reference as the int8 model's plain loop is from the plain reference, plus the bf16 loop bar (3e-2) for the ControlNet's part."""
    d, gn, s = env["d"], env["nets"]["2+2"], CR.inputs("aligned")
    g8 = d.FluxModel(CR.MAIN_CFG)
    g8.load_state_dict(CR.main_state_dict())
    try:
        g8.quantize_int8()
        plain_ref = CR.main_oracle().denoise(s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], TS4)
        plain = rel_l2(_loop(env, g8, s, TS4), plain_ref)
        got = _loop(env, g8, s, TS4, gn)
        cond = rel_l2(got, CR.loop_reference("2+2", "aligned", "plain"))
        print(f"int8 main model: plain loop {plain:.3e}, conditioned loop {cond:.3e}")
        assert np.isfinite(got).all() and cond <= plain + 3e-2, (plain, cond)
        assert not np.array_equal(got, _loop(env, env["gm"], s, TS4, gn))  # (it is the int8 model)
        assert (_loop(env, g8, s, TS4, gn, scale=0.0) == _loop(env, g8, s, TS4)).all()
    finally:
        g8.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_state_untouched(env):
    from diffusion_rs_amd import _lib as L
    torch, d, gm, gn, s = env["torch"], env["d"], env["gm"], env["nets"]["2+2"], CR.inputs("ragged")
    lib = gm.lib

    def refused(code, cn, opts=None, model=gm, match=None):
        rc, img = _entry(env, model, s, cn=cn[0], opts=opts)
        assert rc == code, (rc, lib.fmi_last_error())
        if match:
            assert match in lib.fmi_last_error().decode()
        np.testing.assert_array_equal(img, s["img"])

    # the struct's own refusals
    refused(L.ERR_INVALID, _cn(env, None, s), match="not a ControlNet")
    refused(L.ERR_INVALID, _cn(env, gm, s), match="not a ControlNet")  # a handle that is no ControlNet
    refused(L.ERR_INVALID, _cn(env, gn, s, cond=None), match="cond")
    refused(L.ERR_INVALID, _cn(env, gn, s, dtype=L.F16), match="cond_dtype")
    for bad in (float("nan"), float("inf")):
        refused(L.ERR_INVALID, _cn(env, gn, s, scale=bad), match="scale must be finite")
        refused(L.ERR_INVALID, _cn(env, gn, s, step_scales=[1, bad, 1, 1]), match="step_scales")
    # a net of another geometry
    for k, v in (("num_attention_heads", 4), ("joint_attention_dim", 256), ("pooled_projection_dim", 128), ("axes_dim", [16, 48, 64]), ("theta", 5000), ("in_channels", 128)):
        other = d.FluxControlNetModel(dict(CR.net_cfg("2+0"), **{k: v}))
        try:
            refused(L.ERR_INVALID, _cn(env, other, s), match="must be the main model's")
        finally:
            other.close()
    # a net with missing tensors
    empty = d.FluxControlNetModel(CR.net_cfg("2+0"))
    try:
        refused(L.ERR_STATE, _cn(env, empty, s), match="tensors not set")
    finally:
        empty.close()
    # the combination table's cn row
    ctx, rids = dev(s["img"]), dev(np.zeros((B, s["S"], 3), np.float32))
    fctx = L.FluxContext(C.c_void_p(ctx.data_ptr()), L.F32, C.c_void_p(rids.data_ptr()), s["S"])
    refused(L.ERR_UNSUPPORTED, _cn(env, gn, s), opts=L.FluxDenoiseOptions(C.pointer(fctx), None, None, None, None, None, None), match="context")
    cache = L.FluxStepCache(0.1, None, None, None)
    refused(L.ERR_UNSUPPORTED, _cn(env, gn, s), opts=L.FluxDenoiseOptions(None, None, None, C.pointer(cache), None, None, None), match="step cache")
    gc = d.FluxModel(dict(CR.MAIN_CFG, in_channels=128, out_channels=64))  # a cond_channels > 0 model
    gc.load_state_dict(d.synth.flux_state_dict_numpy(dict(CR.MAIN_CFG, in_channels=128, out_channels=64), seed=0))
    try:
        ctl = L.FluxControl(C.c_void_p(ctx.data_ptr()), L.F32)
        refused(L.ERR_UNSUPPORTED, _cn(env, gn, s), opts=L.FluxDenoiseOptions(None, C.pointer(ctl), None, None, None, None, None), model=gc, match="channel-conditioned")
    finally:
        gc.close()
    # sequence parallelism on the main model
    gs = d.FluxModel(CR.MAIN_CFG)
    gs.load_state_dict(CR.main_state_dict())
    try:
        gs.set_sequence_parallel(0, 2, lambda *a: None)
        refused(L.ERR_UNSUPPORTED, _cn(env, gn, s), model=gs, match="sequence parallelism")
    finally:
        gs.close()
    # the same through the Python checks, before the library is reached
    for kw, msg in ((dict(context=ctx, context_ids=rids), "context="), (dict(cache_threshold=0.1), "step cache")):
        with pytest.raises(ValueError, match=msg):
            gm.denoise(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(s["y"]), dev(s["g"]), TS4, controlnet=gn,
                       controlnet_cond=dev(s["cond"]), **kw)
    # and the forward entry refuses alike, pred untouched
    inp, keep = gm._inputs(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(np.full(B, 0.8, np.float32)), dev(s["y"]), dev(s["g"]))
    pred = torch.full(s["img"].shape, 7.0, dtype=torch.float32, device="cuda")
    cn, keep_cn = _cn(env, gn, s, scale=float("nan"))
    assert lib.fmi_flux_forward_controlnet(gm.h, C.byref(inp), C.byref(cn), C.c_void_p(pred.data_ptr()), torch_stream()) == L.ERR_INVALID
    assert (host(pred) == 7.0).all()


def test_a_controlnet_handle_refuses_what_it_does_not_support(env):
    from diffusion_rs_amd import _lib as L
    torch, d, s = env["torch"], env["d"], CR.inputs("aligned")
    gn = d.FluxControlNetModel(CR.net_cfg("2+0"))
    gn.load_state_dict(CR.net_state_dict("2+0"))
    try:
        def unsupported(fn, *a, **kw):
            with pytest.raises(d.FmiError) as e:
                fn(*a, **kw)
            assert e.value.code == L.ERR_UNSUPPORTED, e.value

        unsupported(gn.quantize_fp8)
        unsupported(gn.quantize_int8)
        unsupported(gn.calibrate_int8, True)
        unsupported(gn.lora_add, "a", "controlnet_blocks.0", np.zeros((4, D), np.float32), np.zeros((D, 4), np.float32))
        unsupported(gn.lora_set_weight, "a", 0.5)
        unsupported(gn.lora_remove)
        unsupported(gn.set_linear_bnb4, "controlnet_blocks.0", np.zeros(D * D // 2, np.uint8), np.zeros(D * D // 64, np.float32), 64, "nf4", D, D)
        unsupported(gn.set_linear_int8, "controlnet_blocks.0", np.zeros((D, D), np.int8), np.zeros(D, np.float32), D, D)
        unsupported(gn.set_sequence_parallel, 0, 2, lambda *a: None)
        args = (dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]))
        unsupported(FluxModel_forward(d), gn, *args, dev(np.full(B, 0.8, np.float32)), dev(s["y"]), dev(s["g"]))
        unsupported(FluxModel_denoise(d), gn, *args, dev(s["y"]), dev(s["g"]), TS4)
        unsupported(FluxModel_denoise(d), gn, *args, dev(s["y"]), dev(s["g"]), TS4, cache_threshold=0.1)  # (and with them the step cache)
        # it still evaluates afterwards
        got_d, _ = gn.eval(*args, dev(np.full(B, 0.8, np.float32)), dev(s["y"]), dev(s["g"]), cond=dev(s["cond"]))
        assert np.isfinite(host(got_d[0])).all()
    finally:
        gn.close()


def FluxModel_forward(d):
    return d.FluxModel.forward


def FluxModel_denoise(d):
    return d.FluxModel.denoise


# ------------------------------------------------------------------------------------------------ the pipeline
def test_pipeline_controlnet_image_is_the_denoise_call_it_should_make():
    import torch
    import diffusion_rs_amd as d
    H, W = 64, 96  # a 4 x 6 token grid
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=CR.MAIN_CFG, vae_cfg=SMALL_VAE))
    pipe.flux.load_state_dict(CR.main_state_dict())
    pipe.vae.load_state_dict(d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0, encoder=True))
    params = d.DiffusionGenerationParams(height=H, width=W, num_steps=4, guidance_scale=3.5)
    rng = np.random.default_rng(9)
    ctrl = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    prompts = ["a", "b"]
    s = CR.inputs("aligned")
    t5, clip = dev(s["txt"], torch.bfloat16), dev(s["y"])
    fwd = lambda **kw: pipe.forward(prompts, params, output="tensor", seed=3, embeddings=(t5, clip), **kw)
    with pytest.raises(ValueError, match="load_controlnet"):
        fwd(controlnet_image=ctrl)
    net = pipe.load_controlnet((CR.net_cfg("2+2"), CR.net_state_dict("2+2")))
    assert pipe.controlnet is net and net.lib.fmi_flux_is_controlnet(net.h) == 1
    _, lat = fwd(controlnet_image=ctrl, controlnet_conditioning_scale=CR.CN_SCALE, return_latents=True)
    _, plain = fwd(return_latents=True)
    assert not np.array_equal(host(lat), host(plain))  # (loaded and given: it conditions; loaded and not given: it does not)
    # the call it should make: the control image encoded as image= is (the posterior mean), one row expanded over the prompts
    cond, _ = d.encode_latents(pipe.vae.encode(d.preprocess_u8(dev(ctrl).unsqueeze(0), interleaved=True)), pipe.vae.scale_factor(), pipe.vae.shift_factor())
    img, ids = d.pack_latents(d.randn_latents(2, 16, H // 8, W // 8, 3, 0, pipe.device))
    ts = pipe.scheduler.get_timesteps(4, pipe.scheduler.calculate_shift(img.shape[1]))
    g = torch.full((2,), 3.5, dtype=torch.float32, device=pipe.device)
    txt_ids = torch.zeros((2, T, 3), dtype=torch.float32, device=pipe.device)

    def direct(**kw):
        return host(pipe.flux.denoise(img, ids, t5, txt_ids, clip, g, ts, controlnet=net, controlnet_cond=cond.expand(2, -1, -1).contiguous(), **kw))

    assert (host(lat) == direct(controlnet_scale=CR.CN_SCALE, controlnet_step_scales=[1, 1, 1, 1])).all()
    # control_guidance_end = 0.5 equals the step scales it implies
    _, half = fwd(controlnet_image=ctrl, controlnet_conditioning_scale=CR.CN_SCALE, control_guidance_end=0.5, return_latents=True)
    assert (host(half) == direct(controlnet_scale=CR.CN_SCALE, controlnet_step_scales=[1, 1, 0, 0])).all() and not np.array_equal(host(half), host(lat))
    # the f32 form of the same image is the same request
    _, again = fwd(controlnet_image=host(d.preprocess_u8(dev(ctrl).unsqueeze(0), interleaved=True)), controlnet_conditioning_scale=CR.CN_SCALE, return_latents=True)
    assert (host(again) == host(lat)).all()
    # it combines with a negative prompt and with image= / strength= / mask=
    out = fwd(controlnet_image=ctrl, negative_embeddings=(dev(s["ntxt"][:1], torch.bfloat16), dev(s["ny"][:1])), true_cfg_scale=2.0, image=ctrl, strength=0.75,
              mask=np.ones((H, W), np.float32))
    assert tuple(out.shape) == (2, 3, H, W)
    for kw, msg in ((dict(reference=ctrl), "reference="), (dict(cache_threshold=0.1), "step cache")):
        with pytest.raises(ValueError, match=msg):
            fwd(controlnet_image=ctrl, **kw)
    pipe.unload_controlnet()
    assert pipe.controlnet is None
    with pytest.raises(ValueError, match="load_controlnet"):
        fwd(controlnet_image=ctrl)
