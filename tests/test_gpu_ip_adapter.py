"""FLUX IP-Adapter: fmi_ip_adapter_*, fmi_flux_forward_ip / fmi_flux_denoise_ip, the image-prompt attention kernel fmi_ip_attention and the
pipeline's ip_adapter_image_embeds=.

The kernel is compared with its recipe in numpy (tests/ip_adapter_ref.py: ip_attention_recipe).  Its bar comes from the recipe's own rounding noise: the recipe is
evaluated in float64 and in float32 on the CPU, and the GPU — whose reduction order and exp differ, nothing else — may lie 4 x that distance from the float64 result
(profiles/ip_adapter.txt records both numbers).  What the semantics promise exactly is compared as values (==): the grid does not matter, rows and samples outside
the call are untouched, a NULL adapter through the new entries IS the existing entries, scale 0 or step scales all 0 IS the plain loop and prepares nothing.
Against the composed CPU reference one conditioned evaluation is within the project's 2e-2 and the 4-step loop within its 3e-2 (the bars of
tests/test_gpu_controlnet.py), and the loop lies at most a third as far from the correct composition as from each wrong one — which tests/test_host_ip_adapter.py
shows to be at least 0.3 away from it.

Main model SMALL_FLUX with 3 double and 2 single blocks; adapter E = 48, N = 4; B = 2, T = 32; token grids 6x4 and 5x7 (both take the un-fused relayout anyway) and
8x4 (where the image stream's q|k|v projection would be fused without an adapter)."""
import ctypes as C

import numpy as np
import pytest

from tests import controlnet_ref as CR
from tests import ip_adapter_ref as IR
from tests.util import SMALL_VAE, bf16_round, dev, host, rel_l2

pytestmark = pytest.mark.gpu

f32 = np.float32
B, T, TS4 = IR.B, IR.T, IR.TS4
H, D = 2, 256


# ------------------------------------------------------------------------------------------------ the kernel against its recipe
@pytest.mark.parametrize("N", [1, 4, 5, 32])
@pytest.mark.parametrize("S", [24, 35, 1030])
def test_ip_attention_against_the_numpy_recipe(S, N):
    import torch
    import diffusion_rs_amd as d
    rng = np.random.default_rng(1000 * S + N)
    qkv = bf16_round(rng.standard_normal((B, S, 3, H, 128)) * rng.uniform(0.2, 3.0, (B, S, 1, H, 1)))  # the q third is read; row stride 3 * D
    wq = bf16_round(1.0 + 0.1 * rng.standard_normal(128))
    K = bf16_round(1.5 * rng.standard_normal((B, H, N, 128)))  # per-sample keys and values
    V = bf16_round(rng.standard_normal((B, H, N, 128)))
    pad = 3  # x lies in a (B, S + pad, D) buffer: batch stride (S + pad) * D > S * D, and the pad rows are canaries
    xbuf = rng.standard_normal((B, S + pad, D)).astype(f32)
    q = qkv[:, :, 0]
    tq, tw, tk, tv = dev(qkv, torch.bfloat16), dev(wq, torch.bfloat16), dev(K, torch.bfloat16), dev(V, torch.bfloat16)

    def run(x0, c, max_row_blocks=0):
        tx = dev(x0)
        d.ip_attention(tq[:, :, 0], tw, tk, tv, tx[:, :S], c, max_row_blocks)
        return host(tx)

    for label, x0, c in (("x = 0, c = 1 (ip itself)", np.zeros_like(xbuf), 1.0), ("random x, c = 0.7", xbuf, 0.7)):
        w64 = IR.ip_attention_recipe(q, wq, K, V, x0[:, :S], c, np.float64)
        w32 = IR.ip_attention_recipe(q, wq, K, V, x0[:, :S], c, np.float32)
        own = rel_l2(w32, w64)
        got = run(x0, c)
        err = rel_l2(got[:, :S], w64)
        print(f"ip_attention S={S} N={N} {label}: float32 recipe vs float64 {own:.3e}, GPU vs float64 {err:.3e} (bar {4 * own:.3e}), GPU vs float32 recipe "
              f"{rel_l2(got[:, :S], w32):.3e}")
        assert np.isfinite(got).all() and err <= 4 * own, (label, err, own)
        np.testing.assert_array_equal(got[:, S:], x0[:, S:])  # nothing outside the S rows of a sample
        for cap in (1, 3):  # the grid's row dimension does not matter: more than one pass per workgroup, the same bits
            assert (run(x0, c, cap) == got).all(), cap
    np.testing.assert_array_equal(host(tq.float()), qkv)  # (the projection is only read)


def test_ip_attention_refuses_other_token_counts_by_name():
    import torch
    import diffusion_rs_amd as d
    from diffusion_rs_amd import _lib as L
    S = 24
    q, w = torch.zeros((B, S, H, 128), dtype=torch.bfloat16, device="cuda"), torch.ones(128, dtype=torch.bfloat16, device="cuda")
    x = torch.full((B, S, D), 7.0, dtype=torch.float32, device="cuda")
    for n in (0, 33):
        kv = torch.zeros((B, H, n, 128), dtype=torch.bfloat16, device="cuda")
        rc = L.load().fmi_ip_attention(C.c_void_p(q.data_ptr()), D, S * D, C.c_void_p(w.data_ptr()), C.c_void_p(kv.data_ptr() or q.data_ptr()),
                                       C.c_void_p(kv.data_ptr() or q.data_ptr()), C.c_void_p(x.data_ptr()), S * D, B, H, S, n, 1.0, 0, None)
        assert rc == L.ERR_UNSUPPORTED and f"N = {n}" in L.load().fmi_last_error().decode()
    assert (host(x) == 7.0).all()
    with pytest.raises(d.FmiError, match="N = 33") as e:
        d.FluxIPAdapter(IR.MAIN_CFG, IR.E, 33)
    assert e.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="do not fit"):
        d.ip_attention(q, w, torch.zeros((B, H + 1, 4, 128), dtype=torch.bfloat16, device="cuda"), torch.zeros((B, H + 1, 4, 128), dtype=torch.bfloat16, device="cuda"), x, 1.0)


# ------------------------------------------------------------------------------------------------ the models
@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    gm = d.FluxModel(IR.MAIN_CFG)
    gm.load_state_dict(IR.main_state_dict())
    ada = d.FluxIPAdapter(IR.MAIN_CFG, IR.E, IR.N)
    ada.load_state_dict(IR.adapter_state_dict())
    gn = d.FluxControlNetModel(CR.net_cfg(IR.CN_NET))
    gn.load_state_dict(CR.net_state_dict(IR.CN_NET))
    return dict(torch=torch, d=d, gm=gm, ada=ada, gn=gn)


def _mode_kw(env, s, mode):
    """FluxModel.denoise's keywords of a mode of tests/ip_adapter_ref.py (without the adapter's own)"""
    torch = env["torch"]
    kw = {}
    if mode in ("cfg", "cfg_neg"):
        kw.update(negative_txt=dev(s["ntxt"], torch.bfloat16), negative_y=dev(s["ny"]), true_cfg_scale=IR.CFG_SCALE)
    if mode == "blend":
        kw.update(x0=dev(s["x0"]), noise=dev(s["img"]), mask=dev(s["mask"]))
    if mode == "controlnet":
        kw.update(controlnet=env["gn"], controlnet_cond=dev(s["cond"]), controlnet_scale=IR.CN_SCALE)
    return kw


def _ip_kw(env, s, mode="plain", scale=IR.IP_SCALE, step_scales=None):
    kw = dict(ip_adapter=env["ada"], ip_adapter_image_embeds=dev(s["emb"]), ip_adapter_scale=scale, ip_adapter_step_scales=step_scales)
    if mode == "cfg_neg":
        kw.update(negative_ip_adapter_image_embeds=dev(s["nemb"]))
    if mode == "steps":
        kw.update(ip_adapter_step_scales=list(IR.STEP_SCALES))
    return kw


def _loop(env, s, **kw):
    torch, gm = env["torch"], env["gm"]
    return host(gm.denoise(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(s["y"]), dev(s["g"]), TS4, **kw))


def _forward(env, s, t, **kw):
    torch, gm = env["torch"], env["gm"]
    return host(gm.forward(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(np.full(B, t, np.float32)), dev(s["y"]), dev(s["g"]), **kw))


def _ref_forward(s, t, c=IR.IP_SCALE):
    Ks, Vs = IR.project(IR.adapter_state_dict(), IR.MAIN_CFG, s["emb"])
    return IR.forward(IR.main_oracle(), IR.main_state_dict(), IR.MAIN_CFG, s["img"], s["ids"], s["txt"], s["txt_ids"], np.full(B, t, np.float32), s["y"], s["g"], Ks, Vs, c)


@pytest.mark.parametrize("grid", list(IR.GRIDS) + list(IR.FUSED_GRID))
def test_forward_against_the_reference(env, grid):
    s = IR.inputs(grid)
    got = _forward(env, s, 0.8, ip_adapter=env["ada"], ip_adapter_image_embeds=dev(s["emb"]), ip_adapter_scale=IR.IP_SCALE)
    err = rel_l2(got, _ref_forward(s, 0.8))
    plain = rel_l2(got, _ref_forward(s, 0.8, 0.0))
    print(f"{grid}: conditioned forward rel-L2 {err:.3e} (to the plain reference: {plain:.3e})")
    assert err <= 2e-2 and 3 * err <= plain, (err, plain)
    # bf16 embeddings are the same request when the values are bf16
    eb = bf16_round(s["emb"])
    a = _forward(env, s, 0.8, ip_adapter=env["ada"], ip_adapter_image_embeds=dev(eb), ip_adapter_scale=IR.IP_SCALE)
    b = _forward(env, s, 0.8, ip_adapter=env["ada"], ip_adapter_image_embeds=dev(eb, env["torch"].bfloat16), ip_adapter_scale=IR.IP_SCALE)
    assert (a == b).all()


@pytest.mark.parametrize("mode", list(IR.MODES))
@pytest.mark.parametrize("grid", list(IR.GRIDS))
def test_loop_against_the_reference_and_its_wrong_variants(env, grid, mode):
    s = IR.inputs(grid)
    got = _loop(env, s, **_mode_kw(env, s, mode), **_ip_kw(env, s, mode))
    correct = rel_l2(got, IR.loop_reference(grid, mode))
    print(f"{grid} {mode}: 4-step loop rel-L2 {correct:.3e}")
    assert correct <= 3e-2, correct
    for v in IR.VARIANTS:
        if v == "neg_uses_pos_embeds" and mode not in ("cfg", "cfg_neg"):
            continue  # (there the variant IS the correct loop)
        wrong = rel_l2(got, IR.loop_reference(grid, mode, v))
        print(f"{grid} {mode}: distance to {v}: {wrong:.3e}")
        assert 3 * correct <= wrong, (v, correct, wrong)


def test_the_fused_shape_loop_and_a_plain_step_in_the_middle(env):
    """8x4 tokens: a step with the adapter un-fuses the image stream's q|k|v relayout, the plain step in the middle of STEP_SCALES keeps it fused"""
    s = IR.inputs("fused")
    got = _loop(env, s, **_ip_kw(env, s, "steps"))
    want = IR.ip_loop(IR.main_oracle(), IR.main_state_dict(), IR.MAIN_CFG, IR.adapter_state_dict(), s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], TS4, s["emb"],
                      c=IR.IP_SCALE, step_scales=IR.STEP_SCALES)
    err = rel_l2(got, want)
    print(f"fused steps: 4-step loop rel-L2 {err:.3e}")
    assert err <= 3e-2, err


# ------------------------------------------------------------------------------------------------ the exact promises
@pytest.mark.parametrize("grid", ["ragged", "fused"])
def test_scale_zero_and_zero_step_scales_are_the_plain_loop(env, grid):
    s = IR.inputs(grid)
    d = env["d"]
    fresh = d.FluxIPAdapter(IR.MAIN_CFG, IR.E, IR.N)
    fresh.load_state_dict(IR.adapter_state_dict())
    try:
        kw = lambda **k: dict(ip_adapter=fresh, ip_adapter_image_embeds=dev(s["emb"]), **k)
        plain = _loop(env, s)
        before = fresh.size_in_bytes()
        assert (_loop(env, s, **kw(ip_adapter_scale=0.0)) == plain).all()
        assert (_loop(env, s, **kw(ip_adapter_scale=-0.0)) == plain).all()
        assert (_loop(env, s, **kw(ip_adapter_step_scales=[0, 0, 0, 0])) == plain).all()
        assert (_forward(env, s, 0.8, **kw(ip_adapter_scale=0.0)) == _forward(env, s, 0.8)).all()
        assert fresh.size_in_bytes() == before  # (nothing of the adapter was projected)
        cond = _loop(env, s, **kw(ip_adapter_scale=IR.IP_SCALE))
        assert not np.array_equal(cond, plain) and fresh.size_in_bytes() > before
        # a step scale is a factor of the scale (0.5 * 2 is exact), and the projection of one call does not leak into the next
        assert (_loop(env, s, **kw(ip_adapter_scale=0.5 * IR.IP_SCALE, ip_adapter_step_scales=[2, 2, 2, 2])) == cond).all()
        assert (_loop(env, s, **kw(ip_adapter_scale=0.0)) == plain).all()
        neg = _mode_kw(env, s, "cfg")
        assert (_loop(env, s, **neg, **kw(ip_adapter_scale=0.0)) == _loop(env, s, **neg)).all()
        # zero negative embeddings given explicitly are the default
        z = _loop(env, s, **neg, **kw(ip_adapter_scale=IR.IP_SCALE))
        assert (_loop(env, s, **neg, **kw(ip_adapter_scale=IR.IP_SCALE, negative_ip_adapter_image_embeds=dev(np.zeros_like(s["emb"])))) == z).all()
    finally:
        fresh.close()


def torch_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _entry(env, gm, s, ip=None, cn=None, opts=None, entry="ip", n_steps=4):
    """fmi_flux_denoise_ip (or _controlnet / _with) on a copy of the set's image; returns (status, the copy afterwards)"""
    torch = env["torch"]
    img = dev(s["img"]).clone()
    inp, keep = gm._inputs(None, dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), None, dev(s["y"]), dev(s["g"]))
    ts = (C.c_double * 5)(*TS4)
    o = C.byref(opts) if opts is not None else None
    if entry == "with":
        rc = gm.lib.fmi_flux_denoise_with(gm.h, C.byref(inp), o, C.c_void_p(img.data_ptr()), ts, n_steps, torch_stream())
    elif entry == "controlnet":
        rc = gm.lib.fmi_flux_denoise_controlnet(gm.h, C.byref(inp), o, C.byref(cn) if cn is not None else None, C.c_void_p(img.data_ptr()), ts, n_steps, torch_stream())
    else:
        rc = gm.lib.fmi_flux_denoise_ip(gm.h, C.byref(inp), o, C.byref(cn) if cn is not None else None, C.byref(ip) if ip is not None else None,
                                        C.c_void_p(img.data_ptr()), ts, n_steps, torch_stream())
    return rc, host(img)


def _ip(ada, s, scale=IR.IP_SCALE, embeds="default", dtype=None, step_scales=None):
    from diffusion_rs_amd import _lib as L
    e = dev(s["emb"]) if isinstance(embeds, str) else embeds
    ss = None if step_scales is None else (C.c_float * len(step_scales))(*step_scales)
    return L.FluxIp(ada.h if ada is not None else None, C.c_void_p(e.data_ptr()) if e is not None else None, L.F32 if dtype is None else dtype, None, scale, ss), (e, ss)


def test_null_adapter_through_the_new_entries_is_the_existing_entries(env):
    from diffusion_rs_amd import _lib as L
    torch, gm, gn, s = env["torch"], env["gm"], env["gn"], IR.inputs("fused")
    rc_a, a = _entry(env, gm, s)
    rc_b, b = _entry(env, gm, s, entry="with")
    assert rc_a == rc_b == 0 and (a == b).all() and (a == _loop(env, s)).all()
    cond = dev(s["cond"])
    cn = L.FluxControlNet(gn.h, C.c_void_p(cond.data_ptr()), L.F32, IR.CN_SCALE, None)
    x0, noise, mask = dev(s["x0"]), dev(s["img"]), dev(s["mask"])
    opts = L.FluxDenoiseOptions(None, None, None, None, C.c_void_p(x0.data_ptr()), C.c_void_p(noise.data_ptr()), C.c_void_p(mask.data_ptr()))
    rc_a, a = _entry(env, gm, s, cn=cn, opts=opts)
    rc_b, b = _entry(env, gm, s, cn=cn, opts=opts, entry="controlnet")
    assert rc_a == rc_b == 0 and (a == b).all()
    bad = L.FluxDenoiseOptions(None, None, None, None, C.c_void_p(x0.data_ptr()), None, None)  # the same error, too
    assert _entry(env, gm, s, opts=bad)[0] == _entry(env, gm, s, opts=bad, entry="with")[0] == L.ERR_INVALID
    # and the forward entry
    inp, keep = gm._inputs(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(np.full(B, 0.8, np.float32)), dev(s["y"]), dev(s["g"]))
    pred = torch.empty(s["img"].shape, dtype=torch.float32, device="cuda")
    assert gm.lib.fmi_flux_forward_ip(gm.h, C.byref(inp), None, None, None, C.c_void_p(pred.data_ptr()), torch_stream()) == 0
    assert (host(pred) == _forward(env, s, 0.8)).all()
    assert gm.lib.fmi_flux_forward_ip(gm.h, C.byref(inp), None, C.byref(cn), None, C.c_void_p(pred.data_ptr()), torch_stream()) == 0
    assert (host(pred) == _forward(env, s, 0.8, controlnet=gn, controlnet_cond=cond, controlnet_scale=IR.CN_SCALE)).all()


def test_the_handle_names_and_both_namings(env):
    d, ada = env["d"], env["ada"]
    from diffusion_rs_amd import loader
    assert ada.missing() == [] and ada.size_in_bytes() > 0
    with pytest.raises(d.FmiError, match="unknown tensor name"):
        ada.set_tensor(f"ip_adapter.{IR.MAIN_CFG['num_layers']}.to_k_ip.weight", np.zeros((D, 128), np.float32))
    with pytest.raises(d.FmiError, match="must be"):
        ada.set_tensor("ip_adapter.0.to_k_ip.weight", np.zeros((D, 64), np.float32))
    fresh = d.FluxIPAdapter(IR.MAIN_CFG, IR.E, IR.N)
    try:
        m = fresh.missing()
        assert "image_proj.norm.bias" in m and "ip_adapter.2.to_v_ip.weight" in m and "ip_adapter.0.to_k_ip.bias" not in m  # (the k / v biases are optional)
        # XLabs names, without the optional biases: a zero bias is the same adapter
        sd = IR.adapter_state_dict()
        xl = {}
        for k, v in sd.items():
            if k.startswith("ip_adapter.") and k.endswith(".bias"):
                continue
            p = k.split(".")
            xl[f"ip_adapter_proj_model.{'proj' if p[1] == 'image_embeds' else 'norm'}.{p[2]}" if p[0] == "image_proj" else
               f"double_blocks.{p[1]}.processor.ip_adapter_double_stream_{p[2][3]}_proj.{p[3]}"] = v
        E, N, conv = loader.ip_adapter_from_tensors(IR.MAIN_CFG, xl)
        assert (E, N) == (IR.E, IR.N)
        fresh.load_state_dict(conv)
        nobias = dict(sd, **{k: np.zeros_like(v) for k, v in sd.items() if k.startswith("ip_adapter.") and k.endswith(".bias")})
        other = d.FluxIPAdapter(IR.MAIN_CFG, IR.E, IR.N)
        try:
            other.load_state_dict(nobias)
            s = IR.inputs("ragged")
            a = _forward(env, s, 0.8, ip_adapter=fresh, ip_adapter_image_embeds=dev(s["emb"]), ip_adapter_scale=IR.IP_SCALE)
            b = _forward(env, s, 0.8, ip_adapter=other, ip_adapter_image_embeds=dev(s["emb"]), ip_adapter_scale=IR.IP_SCALE)
            assert (a == b).all()
        finally:
            other.close()
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_state_untouched(env):
    from diffusion_rs_amd import _lib as L
    torch, d, gm, ada, s = env["torch"], env["d"], env["gm"], env["ada"], IR.inputs("ragged")
    lib = gm.lib

    def refused(code, ip, opts=None, model=gm, match=None):
        rc, img = _entry(env, model, s, ip=ip[0], opts=opts)
        assert rc == code, (rc, lib.fmi_last_error())
        if match:
            assert match in lib.fmi_last_error().decode(), lib.fmi_last_error()
        np.testing.assert_array_equal(img, s["img"])

    refused(L.ERR_INVALID, _ip(None, s), match="adapter is NULL")
    refused(L.ERR_INVALID, _ip(ada, s, embeds=None), match="embeds")
    refused(L.ERR_INVALID, _ip(ada, s, dtype=L.F16), match="embeds_dtype")
    for bad in (float("nan"), float("inf")):
        refused(L.ERR_INVALID, _ip(ada, s, scale=bad), match="scale must be finite")
        refused(L.ERR_INVALID, _ip(ada, s, step_scales=[1, bad, 1, 1]), match="step_scales")
    for k, v in (("num_attention_heads", 4), ("joint_attention_dim", 256), ("num_layers", 2)):  # an adapter of another geometry
        other = d.FluxIPAdapter(dict(IR.MAIN_CFG, **{k: v}), IR.E, IR.N)
        try:
            refused(L.ERR_INVALID, _ip(other, s), match="must be the main model's")
        finally:
            other.close()
    empty = d.FluxIPAdapter(IR.MAIN_CFG, IR.E, IR.N)
    try:
        refused(L.ERR_STATE, _ip(empty, s), match="tensors not set")
    finally:
        empty.close()
    # the combination table's ip row
    ctx, rids = dev(s["img"]), dev(np.zeros((B, s["S"], 3), np.float32))
    fctx = L.FluxContext(C.c_void_p(ctx.data_ptr()), L.F32, C.c_void_p(rids.data_ptr()), s["S"])
    refused(L.ERR_UNSUPPORTED, _ip(ada, s), opts=L.FluxDenoiseOptions(C.pointer(fctx), None, None, None, None, None, None), match="context")
    cache = L.FluxStepCache(0.1, None, None, None)
    refused(L.ERR_UNSUPPORTED, _ip(ada, s), opts=L.FluxDenoiseOptions(None, None, None, C.pointer(cache), None, None, None), match="step cache")
    for what, match in (("sp", "sequence parallelism"), ("fp8", "fp8 mode"), ("int8", "int8 mode"), ("fp8_attn", "fp8 attention")):
        g2 = d.FluxModel(IR.MAIN_CFG)
        g2.load_state_dict(IR.main_state_dict())
        try:
            if what == "sp":
                g2.set_sequence_parallel(0, 2, lambda *a: None)
            elif what == "fp8":
                g2.quantize_fp8()
            elif what == "int8":
                g2.quantize_int8()
            else:
                g2.set_fp8_attention(2)
            refused(L.ERR_UNSUPPORTED, _ip(ada, s), model=g2, match=match)
            if what in ("fp8", "int8"):  # the same through the Python check, before the library is reached
                with pytest.raises(ValueError, match=what):
                    g2.denoise(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(s["y"]), dev(s["g"]), TS4, ip_adapter=ada,
                               ip_adapter_image_embeds=dev(s["emb"]))
        finally:
            g2.close()
    for kw, msg in ((dict(context=ctx, context_ids=rids), "context="), (dict(cache_threshold=0.1), "step cache")):
        with pytest.raises(ValueError, match=msg):
            _loop(env, s, ip_adapter=ada, ip_adapter_image_embeds=dev(s["emb"]), **kw)
    # and the forward entry refuses alike, pred untouched
    inp, keep = gm._inputs(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(np.full(B, 0.8, np.float32)), dev(s["y"]), dev(s["g"]))
    pred = torch.full(s["img"].shape, 7.0, dtype=torch.float32, device="cuda")
    ip, keep_ip = _ip(ada, s, scale=float("nan"))
    assert lib.fmi_flux_forward_ip(gm.h, C.byref(inp), None, None, C.byref(ip), C.c_void_p(pred.data_ptr()), torch_stream()) == L.ERR_INVALID
    assert (host(pred) == 7.0).all()


def test_channel_conditioned_model_takes_an_adapter(env):
    """FLUX.1 Fill / Canny / Depth (a cond_channels > 0 model) next to the adapter: it runs, it conditions, and scale 0 is the controlled loop"""
    torch, d, ada, s = env["torch"], env["d"], env["ada"], IR.inputs("aligned")
    cfg = dict(IR.MAIN_CFG, in_channels=128, out_channels=64)
    gc = d.FluxModel(cfg)
    gc.load_state_dict(d.synth.flux_state_dict_numpy(cfg, seed=0))
    try:
        run = lambda **kw: host(gc.denoise(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(s["y"]), dev(s["g"]), TS4,
                                           control=dev(s["cond"]), **kw))
        plain = run()
        cond = run(ip_adapter=ada, ip_adapter_image_embeds=dev(s["emb"]), ip_adapter_scale=IR.IP_SCALE)
        assert np.isfinite(cond).all() and not np.array_equal(cond, plain)
        assert (run(ip_adapter=ada, ip_adapter_image_embeds=dev(s["emb"]), ip_adapter_scale=0.0) == plain).all()
    finally:
        gc.close()


# ------------------------------------------------------------------------------------------------ the pipeline
def test_pipeline_image_embeds_is_the_denoise_call_it_should_make_and_the_reference_image():
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    Hp, Wp = 64, 96  # a 4 x 6 token grid
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=IR.MAIN_CFG, vae_cfg=SMALL_VAE))
    pipe.flux.load_state_dict(IR.main_state_dict())
    vsd = d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0, encoder=True)
    pipe.vae.load_state_dict(vsd)
    params = d.DiffusionGenerationParams(height=Hp, width=Wp, num_steps=4, guidance_scale=3.5)
    s = IR.inputs("aligned")
    t5, clip = dev(s["txt"], torch.bfloat16), dev(s["y"])
    lat = (np.random.default_rng(11).standard_normal((2, 16, Hp // 8, Wp // 8)) * IR.IMG_MULT).astype(np.float32)
    emb = s["emb"][0]
    fwd = lambda **kw: pipe.forward(["a", "b"], params, output="tensor", embeddings=(t5, clip), latents=dev(lat), **kw)
    with pytest.raises(ValueError, match="load_ip_adapter"):
        fwd(ip_adapter_image_embeds=emb)
    ada = pipe.load_ip_adapter(IR.adapter_state_dict())
    assert pipe.ip_adapter is ada and (ada.embed_dim, ada.num_tokens) == (IR.E, IR.N)
    u8, latents = fwd(ip_adapter_image_embeds=emb, ip_adapter_scale=IR.IP_SCALE, return_latents=True)
    u8_plain, plain = fwd(return_latents=True)
    assert not np.array_equal(host(latents), host(plain)) and not torch.equal(u8, u8_plain)  # (loaded and given: it conditions; loaded and not given: it does not)
    # the call it should make: one embedding row expanded over the prompts
    img, ids = d.pack_latents(dev(lat))
    ts = pipe.scheduler.get_timesteps(4, pipe.scheduler.calculate_shift(img.shape[1]))
    g = torch.full((2,), 3.5, dtype=torch.float32, device=pipe.device)
    txt_ids = torch.zeros((2, T, 3), dtype=torch.float32, device=pipe.device)
    e2 = dev(np.stack([emb, emb]))
    direct = lambda **kw: host(pipe.flux.denoise(img, ids, t5, txt_ids, clip, g, ts, ip_adapter=ada, ip_adapter_image_embeds=e2, ip_adapter_scale=IR.IP_SCALE, **kw))
    assert (host(latents) == direct(ip_adapter_step_scales=[1, 1, 1, 1])).all()
    _, half = fwd(ip_adapter_image_embeds=emb[None], ip_adapter_scale=IR.IP_SCALE, ip_adapter_start=0.25, ip_adapter_end=0.75, return_latents=True)
    assert (host(half) == direct(ip_adapter_step_scales=[0, 1, 1, 0])).all() and not np.array_equal(host(half), host(latents))
    # the image equals the reference loop's, decoded by the oracle's VAE, within the u8 bar of tests/test_gpu_pipeline.py
    pimg, pids = orc.pack_latents(lat)
    want = IR.ip_loop(IR.main_oracle(), IR.main_state_dict(), IR.MAIN_CFG, IR.adapter_state_dict(), pimg, pids, s["txt"], np.zeros((2, T, 3), np.float32), s["y"],
                      np.full(2, 3.5, np.float32), ts, np.stack([emb, emb]), c=IR.IP_SCALE)
    print(f"pipeline latents rel-L2 {rel_l2(host(latents), want):.3e}")
    ov = orc.Vae(SMALL_VAE)
    ov.load(vsd)
    z = orc.unpack_latents(want, 16, Hp // 8, Wp // 8) * np.float32(1.0 / SMALL_VAE["scaling_factor"]) + np.float32(SMALL_VAE["shift_factor"])
    diff = np.abs(u8.cpu().numpy().astype(np.int32) - orc.postprocess_u8(ov.decode(z.astype(np.float32))).astype(np.int32))
    print(f"pipeline u8: max |d| {diff.max()}, frac<=2 {float((diff <= 2).mean()):.4f}")
    assert float((diff <= 2).mean()) >= 0.99
    # it combines with a negative prompt and with image= / strength= / mask=
    rgb = np.random.default_rng(9).integers(0, 256, (Hp, Wp, 3), dtype=np.uint8)
    neg = (dev(s["ntxt"][:1], torch.bfloat16), dev(s["ny"][:1]))
    out = fwd(ip_adapter_image_embeds=emb, negative_ip_adapter_image_embeds=s["nemb"][0], negative_embeddings=neg, true_cfg_scale=2.0, image=rgb, strength=0.75,
              mask=np.ones((Hp, Wp), np.float32))
    assert tuple(out.shape) == (2, 3, Hp, Wp)
    for kw, msg in ((dict(reference=rgb), "reference="), (dict(cache_threshold=0.1), "step cache"), (dict(negative_ip_adapter_image_embeds=emb), "negative prompt")):
        with pytest.raises(ValueError, match=msg):
            fwd(ip_adapter_image_embeds=emb, **kw)
    pipe.unload_ip_adapter()
    assert pipe.ip_adapter is None
    with pytest.raises(ValueError, match="load_ip_adapter"):
        fwd(ip_adapter_image_embeds=emb)
