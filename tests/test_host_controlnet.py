"""FLUX ControlNets, the parts that need no device: the C-ABI additions and their ctypes mirror, the refusals that come before any launch, the
index maps and the keep formula, the loader, the pure argument checks, and a self-test of the composed CPU reference tests/controlnet_ref.py that the GPU tests
measure against.

Without the feature every test here fails at import (tests/controlnet_ref.py needs synth.controlnet_state_dict_numpy) or at symbol lookup."""
import ctypes as C
import dataclasses
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from diffusion_rs_amd import _lib as L
from diffusion_rs_amd import flux as F
from diffusion_rs_amd import loader
from diffusion_rs_amd import pipeline as pl
from diffusion_rs_amd import synth
from tests import controlnet_ref as CR
from tests.lora_util import write_safetensors
from tests.util import SMALL_FLUX, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fmi_flux_create_controlnet", "fmi_flux_is_controlnet", "fmi_flux_forward_controlnet", "fmi_flux_denoise_controlnet", "fmi_flux_controlnet_eval",
               "fmi_flux_controlnet_sample", "fmi_add_scaled_rows_bf16")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = L.load()
    for s in NEW_SYMBOLS:
        assert s in L.EXPORTED
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None
    assert re.search(r"typedef\s+struct\s+fmi_flux_controlnet\s*\{", code)
    assert lib.fmi_abi_version() == 6 and "#define FMI_ABI_VERSION 6" in hdr
    # the ControlNet is an argument of its own: the options struct keeps its 7 fields and 56 bytes
    assert len(L.FluxDenoiseOptions._fields_) == 7 and C.sizeof(L.FluxDenoiseOptions) == 56
    T = L.FluxControlNet  # pointer, pointer, int, float, pointer — with C's padding
    assert [f[0] for f in T._fields_] == ["net", "cond", "cond_dtype", "scale", "step_scales"]
    assert (T.net.offset, T.cond.offset, T.cond_dtype.offset, T.scale.offset, T.step_scales.offset, C.sizeof(T)) == (0, 8, 16, 20, 24, 32)
    a = lib.fmi_flux_denoise_controlnet.argtypes
    assert len(a) == 8 and a[2] == C.POINTER(L.FluxDenoiseOptions) and a[3] == C.POINTER(L.FluxControlNet)
    a = lib.fmi_flux_forward_controlnet.argtypes
    assert len(a) == 5 and a[2] == C.POINTER(L.FluxControlNet)
    a = lib.fmi_add_scaled_rows_bf16.argtypes
    assert len(a) == 8 and a[1] == C.c_int64 and a[4] == C.c_int64 and a[6] == C.c_float
    # the header's combination table has its cn row, and the out-of-scope list stands where the calls refuse
    assert re.search(r"\n \*   cn\s+ctx: FMI_ERR_UNSUPPORTED", hdr) and "controlnet_blocks_repeat" in hdr


def test_refusals_before_any_launch():
    lib = L.load()
    buf = (C.c_float * 64)()
    h = C.c_void_p()
    assert lib.fmi_flux_create_controlnet(None, L.MODEL_BF16, C.byref(h)) == L.ERR_INVALID
    cfg = L.FluxConfig(64, 64, 128, 2, 0, 2, 1, (C.c_int * 3)(16, 56, 56), 10000)  # no double block
    assert lib.fmi_flux_create_controlnet(C.byref(cfg), L.MODEL_BF16, C.byref(h)) == L.ERR_INVALID and h.value is None
    assert b"at least one double block" in lib.fmi_last_error()
    assert lib.fmi_flux_is_controlnet(None) == 0
    # a null handle is refused by every evaluation entry
    assert lib.fmi_flux_forward_controlnet(None, None, None, None, None) == L.ERR_INVALID
    assert lib.fmi_flux_denoise_controlnet(None, None, None, None, None, None, 0, None) == L.ERR_INVALID
    assert lib.fmi_flux_controlnet_eval(None, None, None, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_flux_controlnet_sample(None, 0, 0, buf) == L.ERR_INVALID
    add = lib.fmi_add_scaled_rows_bf16
    assert add(None, 64, buf, 1, 1, 64, 1.0, None) == L.ERR_INVALID
    assert add(buf, 64, None, 1, 1, 64, 1.0, None) == L.ERR_INVALID
    assert add(buf, 64, buf, -1, 1, 64, 1.0, None) == L.ERR_INVALID
    assert add(buf, 64, buf, 1, 1, 0, 1.0, None) == L.ERR_INVALID
    assert add(buf, 32, buf, 1, 1, 64, 1.0, None) == L.ERR_INVALID  # a batch stride below rows * D: the samples' rows would overlap
    assert add(buf, 64, buf, 0, 1, 64, 1.0, None) == 0 and add(buf, 64, buf, 1, 0, 64, 1.0, None) == 0  # nothing to do


# ------------------------------------------------------------------------------------------------ index maps and the keep formula
def test_index_maps_stay_in_range_and_match_diffusers():
    for ND, nd in ((19, 5), (38, 10), (5, 2), (3, 2), (4, 4), (2, 1)):
        m = F.controlnet_index_map(ND, nd)
        assert m == CR.index_map(ND, nd) and len(m) == ND and min(m) == 0 and max(m) <= nd - 1 and m == sorted(m)
        k = int(np.ceil(ND / nd))  # diffusers: interval_control = ceil(len(blocks) / len(samples)); samples[index_block // interval_control]
        assert m == [i // k for i in range(ND)]
    # diffusers' table for FLUX.1-dev with a 5 + 10 ControlNet: kd = ks = 4
    assert F.controlnet_index_map(19, 5) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4]
    assert F.controlnet_index_map(38, 10) == [i // 4 for i in range(38)] and max(F.controlnet_index_map(38, 10)) == 9
    assert F.controlnet_index_map(5, 2) == [0, 0, 0, 1, 1] and F.controlnet_index_map(3, 2) == [0, 0, 1]  # both ceilings bite: 5 / 2 and 3 / 2 are no integers
    assert F.controlnet_index_map(3, 0) == [] and CR.index_map(3, 0) == []
    # the wrong map of the index_floor variant differs from the correct one at both of the test's pairs, in range ...
    for ND, nd in ((5, 2), (3, 2)):
        w = CR.index_map(ND, nd, floor=True)
        assert w != CR.index_map(ND, nd) and max(w) <= nd - 1
    # ... whereas i * nd // ND, another floor one may write, IS the correct map there (and at FLUX.1-dev's 19 / 5): it could not serve as a variant
    for ND, nd in ((5, 2), (3, 2), (19, 5)):
        assert [i * nd // ND for i in range(ND)] == CR.index_map(ND, nd)
    assert [i * 10 // 38 for i in range(38)] != CR.index_map(38, 10)


def test_keep_formula():
    n = 4
    for start in (0, 0.25, 0.5, 1):
        for end in (0, 0.25, 0.5, 1):
            want = [0.0 if (i / n < start or (i + 1) / n > end) else 1.0 for i in range(n)]
            assert F.controlnet_step_scales(n, start, end) == want == CR.keep(n, start, end), (start, end)
    assert F.controlnet_step_scales(4, 0.0, 1.0) == [1, 1, 1, 1]
    assert F.controlnet_step_scales(4, 0.0, 0.5) == [1, 1, 0, 0]
    assert F.controlnet_step_scales(4, 0.25, 0.5) == [0, 1, 0, 0]
    assert F.controlnet_step_scales(4, 0.5, 1.0) == [0, 0, 1, 1]
    assert F.controlnet_step_scales(4, 0.5, 0.25) == [0, 0, 0, 0] and F.controlnet_step_scales(4, 1, 1) == [0, 0, 0, 0]
    assert F.controlnet_step_scales(0) == []


# ------------------------------------------------------------------------------------------------ synthetic weights
def test_controlnet_tensor_shapes_and_the_untouched_generators():
    D = 256
    for name, (nd, ns) in CR.NETS.items():
        cfg = CR.net_cfg(name)
        t = synth.controlnet_tensor_shapes(cfg)
        flux = synth.flux_tensor_shapes(cfg)
        assert not any(k.startswith("norm_out.") or k.startswith("proj_out.") for k in t)
        extra = [k for k in t if k not in flux]
        assert extra == [f"controlnet_x_embedder.{p}" for p in ("weight", "bias")] + [f"controlnet_blocks.{i}.{p}" for i in range(nd) for p in ("weight", "bias")] + \
            [f"controlnet_single_blocks.{j}.{p}" for j in range(ns) for p in ("weight", "bias")]
        assert t["controlnet_x_embedder.weight"] == (D, 64) and t["controlnet_blocks.0.weight"] == (D, D) and t["controlnet_blocks.1.bias"] == (D,)
        assert set(flux) - set(t) == {"norm_out.linear.weight", "norm_out.linear.bias", "proj_out.weight", "proj_out.bias"}
        sd = CR.net_state_dict(name)
        assert list(sd) == list(t) and all(sd[k].shape == tuple(v) and sd[k].dtype == np.float32 for k, v in t.items())
    # the existing synthetic checkpoint draws what it drew: the first values of the default generator's stream, scaled
    ref = (0.02 * np.random.default_rng(0).standard_normal((D, 64))).astype(np.float32)
    np.testing.assert_array_equal(synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)["x_embedder.weight"], synth.to_bf16_f32(ref))


# ------------------------------------------------------------------------------------------------ the composed reference
def test_composition_with_zero_samples_is_the_oracle_forward():
    """Measured: rel-L2 1.2e-7 (ragged) / 1.1e-7 (aligned) to oracle.Flux.forward — f32 rounding of the final layer written in numpy, five orders below the 2e-2
    evaluation bar.  The same holds with explicit all-zero samples at any scale (exact zeros added to f32 values change nothing)."""
    om, sd = CR.main_oracle(), CR.main_state_dict()
    for grid in CR.GRIDS:
        s = CR.inputs(grid)
        t = np.full(CR.B, 0.8, np.float32)
        want = om.forward(s["img"], s["ids"], s["txt"], s["txt_ids"], t, s["y"], s["g"])
        got = CR.forward(om, sd, CR.MAIN_CFG, s["img"], s["ids"], s["txt"], s["txt_ids"], t, s["y"], s["g"])
        err = rel_l2(got, want)
        print(f"{grid}: composed forward vs oracle.Flux.forward: rel-L2 {err:.3e}")
        assert err <= 1e-5, err
        z = np.zeros((CR.B, s["S"], 256), np.float32)
        np.testing.assert_array_equal(CR.forward(om, sd, CR.MAIN_CFG, s["img"], s["ids"], s["txt"], s["txt_ids"], t, s["y"], s["g"], [z, z], [z, z], 0.7), got)


@pytest.mark.parametrize("grid", list(CR.GRIDS))
@pytest.mark.parametrize("net", list(CR.NETS))
def test_every_variant_is_far_from_the_correct_loop(net, grid):
    """The precondition of the GPU test's one-third criterion: every wrong variant's 4-step result is at least 9e-2 (3 x the loop's 3e-2 bar) from the correct
    loop, plain, under true CFG and with the blend.  Measured rel-L2, smallest over the two grids (plain / cfg / blend):
      2+2: index_floor .141 / .159 / .129   single_into_txt_rows .162 / .188 / .147   samples_swapped .393 / .433 / .357   scale_dropped .124 / .128 / .109
           cond_zeroed .295 / .361 / .272   neg_uses_pos_text - / .121 / -
      2+0: index_floor .122 / .136 / .111   samples_swapped .399 / .438 / .364   scale_dropped .140 / .144 / .122   cond_zeroed .294 / .345 / .269
           neg_uses_pos_text - / .105 / -
    single_into_txt_rows needs single samples (not the 2+0 net) and neg_uses_pos_text a negative (cfg only): elsewhere they ARE the correct loop."""
    s = CR.inputs(grid)
    for mode in ("plain", "cfg", "blend"):
        correct = CR.loop_reference(net, grid, mode)
        assert correct.dtype == np.float32 and correct.shape == s["img"].shape and np.isfinite(correct).all()
        for v in CR.VARIANTS:
            applies = not (v == "single_into_txt_rows" and CR.NETS[net][1] == 0) and not (v == "neg_uses_pos_text" and mode != "cfg")
            dist = rel_l2(CR.loop_reference(net, grid, mode, v), correct)
            print(f"{net} {grid} {mode}: {v}: rel-L2 {dist:.3e} from the correct loop")
            if applies:
                assert dist >= 9e-2, (v, mode, dist)
            else:
                assert dist == 0.0, (v, mode, dist)
    # scale 0, or step scales all 0, is the plain loop of the main model exactly
    args = (CR.main_oracle(), CR.main_state_dict(), CR.MAIN_CFG, CR.net_oracle(net), CR.net_state_dict(net), CR.net_cfg(net), s["img"], s["cond"], s["ids"], s["txt"],
            s["txt_ids"], s["y"], s["g"], CR.TS4)
    plain = CR.main_oracle().denoise(s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], CR.TS4)
    off = CR.controlnet_loop(*args, c=0.0)
    np.testing.assert_array_equal(off, CR.controlnet_loop(*args, c=CR.CN_SCALE, step_scales=[0, 0, 0, 0]))
    assert rel_l2(off, plain) <= 1e-5
    assert rel_l2(CR.loop_reference(net, grid, "plain"), plain) >= 9e-2  # (the ControlNet matters)


# ------------------------------------------------------------------------------------------------ the loader
def _write_net(path, cfg, sd, **config):
    os.makedirs(path, exist_ok=True)
    conf = dict(_class_name="FluxControlNetModel", in_channels=cfg["in_channels"], pooled_projection_dim=cfg["pooled_projection_dim"],
                joint_attention_dim=cfg["joint_attention_dim"], num_attention_heads=cfg["num_attention_heads"], attention_head_dim=128,
                num_layers=cfg["num_layers"], num_single_layers=cfg["num_single_layers"], guidance_embeds=cfg["guidance_embeds"], axes_dims_rope=cfg["axes_dim"],
                num_mode=None, conditioning_embedding_channels=None)
    conf.update(config)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(conf, f)
    names = list(sd)
    half = len(names) // 2  # two shards: diffusion_pytorch_model-0000x-of-00002.safetensors
    write_safetensors(os.path.join(path, "diffusion_pytorch_model-00001-of-00002.safetensors"), {k: sd[k] for k in names[:half]})
    write_safetensors(os.path.join(path, "diffusion_pytorch_model-00002-of-00002.safetensors"), {k: sd[k] for k in names[half:]})


def test_loader_round_trip_and_unsupported_configs(tmp_path):
    cfg, sd = CR.net_cfg("2+2"), CR.net_state_dict("2+2")
    _write_net(str(tmp_path / "net"), cfg, sd)
    got_cfg, got = loader.load_controlnet(str(tmp_path / "net"))
    assert got_cfg == dict(cfg, theta=10000) and list(got_cfg["axes_dim"]) == [16, 56, 56]
    assert set(got) == set(sd)
    for k, v in sd.items():
        np.testing.assert_array_equal(got[k].to(torch.float32).numpy(), v, err_msg=k)
    for field, value in (("num_mode", 10), ("conditioning_embedding_channels", 16), ("attention_head_dim", 64)):
        _write_net(str(tmp_path / field), cfg, sd, **{field: value})
        with pytest.raises(ValueError, match=field):
            loader.load_controlnet(str(tmp_path / field))
    _write_net(str(tmp_path / "cls"), cfg, sd, _class_name="FluxTransformer2DModel")
    with pytest.raises(ValueError, match="_class_name"):
        loader.load_controlnet(str(tmp_path / "cls"))
    _write_net(str(tmp_path / "short"), cfg, {k: v for k, v in sd.items() if k != "controlnet_blocks.1.bias"})
    with pytest.raises(ValueError, match="missing.*controlnet_blocks.1.bias"):
        loader.load_controlnet(str(tmp_path / "short"))
    _write_net(str(tmp_path / "extra"), cfg, dict(sd, **{"controlnet_blocks.9.bias": np.zeros(256, np.float32)}))
    with pytest.raises(ValueError, match="controlnet_blocks.9.bias is not part"):
        loader.load_controlnet(str(tmp_path / "extra"))
    with pytest.raises(FileNotFoundError):
        loader.load_controlnet(str(tmp_path / "nothing"))


# ------------------------------------------------------------------------------------------------ the argument checks
def test_check_controlnet_args():
    chk = F.check_controlnet_args
    main, net = CR.MAIN_CFG, CR.net_cfg("2+0")
    img = (2, 24, 64)
    assert chk(main) is None and chk(main, net, img, (2, 24, 64)) is None
    ss = chk(main, net, img, (2, 24, 64), 0.7, [1, 1, 0, 0], 4)
    assert ss.dtype == np.float32 and ss.tolist() == [1, 1, 0, 0] and ss.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError, match="controlnet_cond= needs controlnet="):
        chk(main, None, img, (2, 24, 64))
    with pytest.raises(ValueError, match="controlnet_step_scales= needs controlnet="):
        chk(main, None, img, None, 1.0, [1.0])
    with pytest.raises(ValueError, match="needs controlnet_cond="):
        chk(main, net, img)
    for bad in ((2, 24, 128), (1, 24, 64), (2, 23, 64), (2, 24)):
        with pytest.raises(ValueError, match="controlnet_cond is"):
            chk(main, net, img, bad)
    for k, v in (("num_attention_heads", 4), ("joint_attention_dim", 256), ("pooled_projection_dim", 128), ("axes_dim", [16, 48, 64]), ("theta", 5000), ("in_channels", 128)):
        with pytest.raises(ValueError, match=k):
            chk(main, dict(net, **{k: v}), img, (2, 24, 64 if k != "in_channels" else 128))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="controlnet_scale must be finite"):
            chk(main, net, img, (2, 24, 64), bad)
        with pytest.raises(ValueError, match="entries must be finite"):
            chk(main, net, img, (2, 24, 64), 1.0, [1, bad, 1, 1], 4)
    with pytest.raises(ValueError, match="one entry per step"):
        chk(main, net, img, (2, 24, 64), 1.0, [1, 1, 1], 4)
    with pytest.raises(ValueError, match="context="):
        F.check_combination({"controlnet", "context"})
    with pytest.raises(ValueError, match="channel-conditioned"):
        F.check_combination({"controlnet", "control"})
    with pytest.raises(ValueError, match="step cache"):
        F.check_combination({"controlnet", "cache"})
    with pytest.raises(ValueError, match="sequence parallelism"):
        F.check_combination({"controlnet", "sequence_parallel"})
    # a negative scale is a scale: -2 passes
    assert chk(main, net, img, (2, 24, 64), -2.0) is None


def test_check_controlnet_request_and_the_request_path():
    chk = pl.check_controlnet_request
    assert chk(False, 64, 64) is None and chk(True, 64, 64) is None  # no controlnet_image=: an unconditioned request, whatever is loaded
    assert chk(True, 64, 96, (64, 96, 3), True) is None and chk(True, 64, 96, (1, 3, 64, 96), False, -2.0, 0.25, 0.5) is None
    with pytest.raises(ValueError, match="load_controlnet"):
        chk(False, 64, 64, (64, 64, 3), True)
    with pytest.raises(ValueError, match="multiples of 16"):
        chk(True, 72, 64, (72, 64, 3), True)
    for shape, u8 in (((64, 64), True), ((32, 32, 3), True), ((2, 3, 64, 64), False), ((64, 64, 3), False)):  # (nothing is resized; one image per request)
        with pytest.raises(ValueError, match="controlnet_image must be"):
            chk(True, 64, 64, shape, u8)
    with pytest.raises(ValueError, match="controlnet_conditioning_scale"):
        chk(True, 64, 64, (64, 64, 3), True, float("nan"))
    for start, end in ((-0.1, 1.0), (0.0, 1.5), (0.75, 0.5)):
        with pytest.raises(ValueError, match="control_guidance_start"):
            chk(True, 64, 64, (64, 64, 3), True, 1.0, start, end)
    for other, msg in (("context", "reference="), ("cache", "step cache"), ("control", "channel-conditioned"), ("sequence_parallel", "sequence parallelism")):
        with pytest.raises(ValueError, match=msg):
            F.check_combination({"controlnet", other}, pl.REQUEST_NAMES)
    # the control image is ONE per request: a per-request object like the negative and the control, never a field of _Samples
    assert "controlnet_image" not in [f.name for f in dataclasses.fields(pl._Samples)]
    assert [f.name for f in dataclasses.fields(pl._ControlNetInput)] == ["image", "scale", "start", "end"]
    for fn in (pl.Pipeline.forward, pl.Pipeline.generate_tensor):
        p = inspect.signature(fn).parameters
        assert (p["controlnet_image"].default, p["controlnet_conditioning_scale"].default, p["control_guidance_start"].default, p["control_guidance_end"].default) == \
            (None, 1.0, 0.0, 1.0)
    assert "controlnet" in inspect.signature(pl.Pipeline._generate_chunk).parameters  # a keyword of its own, like every shared option
    assert "control" not in [f.name for f in dataclasses.fields(pl._IpAdapterInput)]  # ... and none of them carries another inside
    assert hasattr(pl.Pipeline, "load_controlnet") and hasattr(pl.Pipeline, "unload_controlnet")
    for fn, names in ((F.FluxModel.forward, ("controlnet", "controlnet_cond", "controlnet_scale")),
                      (F.FluxModel.denoise, ("controlnet", "controlnet_cond", "controlnet_scale", "controlnet_step_scales"))):
        p = inspect.signature(fn).parameters
        assert all(n in p for n in names) and p["controlnet_scale"].default == 1.0
