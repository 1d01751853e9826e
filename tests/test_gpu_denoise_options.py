"""The denoise loop's options: fmi_flux_denoise_with against the six entries that came before it, at the ctypes level.

Every comparison is bit for bit — the older entries ARE the new one with the fields they name set, so nothing here has a tolerance: NULL options and an all-NULL
struct are fmi_flux_denoise; each older entry with a representative argument set gives the status, the state and (the cached loop) the decisions and distances of
fmi_flux_denoise_with with the same options; and every refusal — the three pairs of options that do not combine, a blend given in part, a control on a plain
model, none on a conditioned one — comes back with its code, the state untouched and, where a step cache was among the options, nothing allocated for it.
Every refusal is an argument check that returns before a launch.

SMALL_FLUX plain and with in_channels 128 (the narrowest of test_gpu_control's widths), seed 0; B = 2, T = 32; token grids 6x4 (aligned) and 5x7 (ragged); 4 steps."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_control import GRIDS, SCALE, TS4, WIDTHS, B, T, _cfg, _inp
from tests.util import SMALL_FLUX, dev, flux_inputs, host

pytestmark = pytest.mark.gpu

K = min(WIDTHS)
R_HW = (3, 7)  # the context's token grid: 21 rows, no multiple of 8 or 16
FORCE = [0, 1, -1, 1]  # the cached loop's forced mask: steps 1 and 3 reuse, step 2 is left to the threshold (0: compute)


def _model(d, cfg):
    gm = d.FluxModel(cfg)
    gm.load_state_dict(d.synth.flux_state_dict_numpy(cfg, seed=0))
    return gm


@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    sets = {}
    for name, hw in GRIDS.items():
        img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, hw, T, seed=41)
        _, _, ntxt, _, ny = flux_inputs(SMALL_FLUX, B, hw, T, seed=43)
        rng = np.random.default_rng(45)
        x0 = rng.standard_normal(img.shape).astype(np.float32)
        mask = (rng.random(img.shape) < 0.5).astype(np.float32)  # mixed 0 / 1
        cond = rng.standard_normal((B, hw[0] * hw[1], K - 64)).astype(np.float32)
        ctx = rng.standard_normal((B, R_HW[0] * R_HW[1], 64)).astype(np.float32)
        sets[name] = dict(S=hw[0] * hw[1], img=img, ids=ids, txt=txt, txt_ids=txt_ids, y=y, ntxt=ntxt, ny=ny, x0=x0, mask=mask, cond=cond, ctx=ctx)
    e = dict(torch=torch, d=d, sets=sets, plain=_model(d, SMALL_FLUX), cond=_model(d, _cfg(K)))
    yield e
    e["plain"].close(), e["cond"].close()


class _Args:
    """the option structs of one argument set over a set's device tensors (which it keeps alive); cache() makes a fresh step-cache struct with its own outputs"""

    def __init__(self, env, s, names):
        from diffusion_rs_amd import _lib as L
        torch, d = env["torch"], env["d"]
        vp = lambda t: C.c_void_p(t.data_ptr())
        self.keep = dict(x0=dev(s["x0"]), noise=dev(s["img"]), mask=dev(s["mask"]), ntxt=dev(s["ntxt"], torch.bfloat16), ny=dev(s["ny"]), cond=dev(s["cond"]),
                         ctx=dev(s["ctx"]), ctx_ids=d.latent_ids(B, *R_HW, id0=1.0))
        k = self.keep
        self.ctx = L.FluxContext(vp(k["ctx"]), L.F32, vp(k["ctx_ids"]), R_HW[0] * R_HW[1]) if "ctx" in names else None
        self.ctl = L.FluxControl(vp(k["cond"]), L.F32) if "ctl" in names else None
        self.cfg = L.FluxTrueCfg(vp(k["ntxt"]), L.BF16, vp(k["ny"]), L.F32, SCALE) if "cfg" in names else None
        self.blend = [vp(k[n]) for n in ("x0", "noise", "mask")] if "blend" in names else [None, None, None]
        self.cached = "cache" in names

    def cache(self):
        from diffusion_rs_amd import _lib as L
        if not self.cached:
            return None, None
        force, out = np.array(FORCE, np.int8), (np.full(4, -7, np.int32), np.full((4, B), -7.0, np.float32))
        sc = L.FluxStepCache(0.0, force.ctypes.data_as(C.POINTER(C.c_int8)), out[0].ctypes.data_as(C.POINTER(C.c_int32)), out[1].ctypes.data_as(C.POINTER(C.c_float)))
        return sc, (force,) + out


def _run(env, gm, s, entry, a, opts="struct"):
    """`entry` on a copy of the set's image: (status, the copy afterwards, the cached loop's (decisions, distances) or None)"""
    from diffusion_rs_amd import _lib as L
    torch, lib = env["torch"], gm.lib
    img = dev(s["img"]).clone()
    inp, keep = _inp(env, gm, s)
    ts, ip, io = (C.c_double * 5)(*TS4), C.c_void_p(img.data_ptr()), C.byref(inp)
    ref = lambda x: None if x is None else C.byref(x)
    ptr = lambda x: None if x is None else C.pointer(x)
    sc, out = a.cache()
    if entry == "with":
        o = None if opts is None else C.byref(L.FluxDenoiseOptions(ptr(a.ctx), ptr(a.ctl), ptr(a.cfg), ptr(sc), *a.blend))
        rc = lib.fmi_flux_denoise_with(gm.h, io, o, ip, ts, 4, None)
    elif entry == "denoise":
        rc = lib.fmi_flux_denoise(gm.h, io, ip, ts, 4, None)
    elif entry == "inpaint":
        rc = lib.fmi_flux_denoise_inpaint(gm.h, io, ip, ts, 4, *a.blend, None)
    elif entry == "context":
        rc = lib.fmi_flux_denoise_context(gm.h, io, ref(a.ctx), ip, ts, 4, *a.blend, None)
    elif entry == "cached":
        rc = lib.fmi_flux_denoise_cached(gm.h, io, ref(a.ctx), ip, ts, 4, *a.blend, ref(sc), None)
    elif entry == "cfg":
        rc = lib.fmi_flux_denoise_cfg(gm.h, io, ref(a.ctx), ref(a.cfg), ip, ts, 4, *a.blend, None)
    else:
        assert entry == "control"
        rc = lib.fmi_flux_denoise_control(gm.h, io, ref(a.ctl), ref(a.cfg), ip, ts, 4, *a.blend, None)
    torch.cuda.synchronize()
    return rc, host(img), None if out is None else out[1:]


@pytest.mark.parametrize("grid", list(GRIDS))
def test_null_options_and_an_all_null_struct_are_the_plain_loop(env, grid):
    s, gm = env["sets"][grid], env["plain"]
    a = _Args(env, s, ())
    rc, want, _ = _run(env, gm, s, "denoise", a)
    assert rc == 0 and not np.array_equal(want, s["img"])
    for opts in (None, "struct"):
        rc, got, _ = _run(env, gm, s, "with", a, opts=opts)
        assert rc == 0
        np.testing.assert_array_equal(got, want, err_msg=str(opts))


# (the model, the older entry, the options its arguments name)
LEGACY_CASES = {
    "inpaint": ("plain", "inpaint", ("blend",)),
    "context": ("plain", "context", ("ctx",)),
    "cached": ("plain", "cached", ("cache",)),
    "cfg": ("plain", "cfg", ("cfg",)),
    "cfg+context+mask": ("plain", "cfg", ("cfg", "ctx", "blend")),
    "control": ("cond", "control", ("ctl",)),
    "control+mask": ("cond", "control", ("ctl", "blend")),
    "control+cfg": ("cond", "control", ("ctl", "cfg")),
    "control+cfg+mask": ("cond", "control", ("ctl", "cfg", "blend")),
}


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("case", list(LEGACY_CASES))
def test_each_older_entry_is_the_new_one_with_its_fields_set(env, case, grid):
    model, entry, names = LEGACY_CASES[case]
    s, gm = env["sets"][grid], env[model]
    a = _Args(env, s, names)
    rc, want, want_out = _run(env, gm, s, entry, a)
    assert rc == 0
    assert not np.array_equal(want, s["img"])
    rc, got, got_out = _run(env, gm, s, "with", a)
    assert rc == 0
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    if "cache" in names:
        assert want_out[0].tolist() == [0, 1, 0, 1]  # the forced mask reused two steps
        np.testing.assert_array_equal(got_out[0], want_out[0])
        np.testing.assert_array_equal(got_out[1].view(np.uint32), want_out[1].view(np.uint32))
    if "cfg" in names:  # the negative differs from the prompt: the loop without it is another image
        rc, other, _ = _run(env, gm, s, "with", _Args(env, s, tuple(n for n in names if n != "cfg")))
        assert rc == 0 and not np.array_equal(other, want)


def test_refusals_come_with_their_code_before_any_launch_or_allocation(env):
    from diffusion_rs_amd import _lib as L
    d, s = env["d"], env["sets"]["ragged"]
    # fresh models: no cached call has succeeded on them, so the step cache holds nothing yet
    models = dict(plain=_model(d, SMALL_FLUX), cond=_model(d, _cfg(K)))
    try:
        for model, names, code in (("cond", ("ctl", "cache"), L.ERR_UNSUPPORTED), ("cond", ("ctl", "ctx"), L.ERR_UNSUPPORTED),
                                   ("plain", ("cfg", "cache"), L.ERR_UNSUPPORTED), ("plain", ("ctl",), L.ERR_INVALID), ("cond", (), L.ERR_INVALID),
                                   ("cond", ("cache",), L.ERR_INVALID)):
            gm = models[model]
            assert gm.step_cache_bytes() == 0
            rc, after, out = _run(env, gm, s, "with", _Args(env, s, names))
            assert rc == code, (model, names, rc)
            np.testing.assert_array_equal(after.view(np.uint32), s["img"].view(np.uint32), err_msg=str(names))  # bit for bit
            assert gm.step_cache_bytes() == 0, names
            if out is not None:  # the cache's outputs are as the caller left them
                assert (out[0] == -7).all() and (out[1] == -7.0).all()
        for part in ((0,), (0, 1), (2,), (1, 2)):  # x0 / noise / mask given in part
            a = _Args(env, s, ("blend",))
            a.blend = [p if i in part else None for i, p in enumerate(a.blend)]
            rc, after, _ = _run(env, models["plain"], s, "with", a)
            assert rc == L.ERR_INVALID, part
            np.testing.assert_array_equal(after.view(np.uint32), s["img"].view(np.uint32))
        # the models are as they were: the loops run, and give what the module's models give
        for model, names in (("plain", ()), ("cond", ("ctl",))):
            rc, got, _ = _run(env, models[model], s, "with", _Args(env, s, names))
            assert rc == 0
            np.testing.assert_array_equal(got, _run(env, env[model], s, "with", _Args(env, s, names))[1])
    finally:
        for gm in models.values():
            gm.close()


# ------------------------------------------------------------------------------------------------ Python's table against the library's
PAIR_NAMES = dict(ctx="context", ctl="control", cfg="true_cfg", cache="cache", blend="blend", cn="controlnet", ip="ip_adapter")  # the struct's names -> flux.REFUSED_PAIRS'


def test_the_library_refuses_exactly_the_pairs_python_refuses(env):
    """flux.REFUSED_PAIRS against validate(): of the 21 pairs of {ctx, ctl, cfg, cache, x0 / noise / mask, cn, ip}, handed to fmi_flux_denoise_ip as ctypes structs, the
    library answers FMI_ERR_UNSUPPORTED — before any launch, the state untouched — exactly for the pairs Python's table holds, and runs the others (one step).
    B = 1, the 6x4 grid, T = 32; the conditioned twin for the pairs with ctl; a 1+1-block ControlNet and a 4-token adapter.  The rows of flux.REFUSED_MODES
    (sequence parallelism, the 8-bit modes) are held against the library by the refusal tests of test_gpu_step_cache, test_gpu_true_cfg, test_gpu_control,
    test_gpu_controlnet and test_gpu_ip_adapter, and against this table by tests/test_host_denoise_options.py."""
    import itertools
    from diffusion_rs_amd import _lib as L
    from diffusion_rs_amd import flux as F
    torch, d = env["torch"], env["d"]
    E, R = 16, R_HW[0] * R_HW[1]
    s = dict(zip(("img", "ids", "txt", "txt_ids", "y"), flux_inputs(SMALL_FLUX, 1, GRIDS["aligned"], T, seed=41)))
    rng = np.random.default_rng(47)
    vp = lambda t: C.c_void_p(t.data_ptr())
    k = dict(x0=dev(rng.standard_normal(s["img"].shape).astype(np.float32)), noise=dev(s["img"]), mask=dev((rng.random(s["img"].shape) < 0.5).astype(np.float32)),
             ntxt=dev(rng.standard_normal(s["txt"].shape).astype(np.float32), torch.bfloat16), ny=dev(rng.standard_normal(s["y"].shape).astype(np.float32)),
             cond=dev(rng.standard_normal(s["img"].shape[:2] + (K - 64,)).astype(np.float32)), ctx=dev(rng.standard_normal((1, R, 64)).astype(np.float32)),
             ctx_ids=d.latent_ids(1, *R_HW, id0=1.0), cn_cond=dev(rng.standard_normal(s["img"].shape).astype(np.float32)),
             emb=dev(rng.standard_normal((1, E)).astype(np.float32)))
    net_cfg = dict(SMALL_FLUX, num_layers=1, num_single_layers=1)
    net, ada = d.FluxControlNetModel(net_cfg), d.FluxIPAdapter(SMALL_FLUX, E, 4)
    refused_in_python = {frozenset(r) for r in F.REFUSED_PAIRS}
    try:
        net.load_state_dict(d.synth.controlnet_state_dict_numpy(net_cfg, seed=3))
        ada.load_state_dict(d.synth.ip_adapter_state_dict_numpy(SMALL_FLUX, E, 4, seed=5))
        for pair in itertools.combinations(PAIR_NAMES, 2):
            gm = env["cond" if "ctl" in pair else "plain"]
            dec, dist = np.zeros(1, np.int32), np.zeros((1, 1), np.float32)
            st = dict(ctx=L.FluxContext(vp(k["ctx"]), L.F32, vp(k["ctx_ids"]), R), ctl=L.FluxControl(vp(k["cond"]), L.F32),
                      cfg=L.FluxTrueCfg(vp(k["ntxt"]), L.BF16, vp(k["ny"]), L.F32, SCALE),
                      cache=L.FluxStepCache(0.1, None, dec.ctypes.data_as(C.POINTER(C.c_int32)), dist.ctypes.data_as(C.POINTER(C.c_float))),
                      cn=L.FluxControlNet(net.h, vp(k["cn_cond"]), L.F32, 1.0, None), ip=L.FluxIp(ada.h, vp(k["emb"]), L.F32, None, 1.0, None))
            opts = L.FluxDenoiseOptions(*[C.pointer(st[n]) if n in pair else None for n in ("ctx", "ctl", "cfg", "cache")],
                                        *[vp(k[n]) if "blend" in pair else None for n in ("x0", "noise", "mask")])
            img = dev(s["img"]).clone()
            inp, keep = _inp(env, gm, s)
            rc = gm.lib.fmi_flux_denoise_ip(gm.h, C.byref(inp), C.byref(opts), C.byref(st["cn"]) if "cn" in pair else None, C.byref(st["ip"]) if "ip" in pair else None,
                                            C.c_void_p(img.data_ptr()), (C.c_double * 2)(1.0, 0.0), 1, None)
            torch.cuda.synchronize()
            if frozenset(PAIR_NAMES[n] for n in pair) in refused_in_python:
                assert rc == L.ERR_UNSUPPORTED, (pair, rc, gm.lib.fmi_last_error())
                np.testing.assert_array_equal(host(img).view(np.uint32), s["img"].view(np.uint32), err_msg=str(pair))
            else:
                assert rc == 0, (pair, rc, gm.lib.fmi_last_error())
                assert np.isfinite(host(img)).all() and not np.array_equal(host(img), s["img"]), pair
    finally:
        net.close(), ada.close()
