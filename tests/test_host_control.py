"""Channel-concatenated conditioning (FLUX.1 Fill / Canny / Depth), the parts that need no device: the C-ABI additions and their ctypes mirror,
the refusals that come before any launch, the loader's class / channel agreement, out_channels in the tensor shapes, the pure argument checks, the request path
of the pipeline (the control is ONE per request: a keyword of controlled chunks only, never a field of _Samples), the numpy mask-pack reference against
diffusers' view chain, and a self-test of the composed CPU reference tests/control_ref.py that the GPU tests measure against.

One test here passes on the code before the feature too, on purpose: test_mask_pack_reference_is_the_view_chain (both sizes) tests the numpy reference, not
the library — it is the precondition of the GPU test's bit-for-bit comparison.  Every other test of this file, and every test of tests/test_gpu_control.py, fails
without the feature (missing symbol, keyword or function; test_composed_reference_self_test because the weights' proj_out needs out_channels)."""
import ctypes as C
import dataclasses
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
from tests import control_ref as CR
from tests.util import SMALL_FLUX, flux_inputs, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fmi_flux_create_cond", "fmi_flux_cond_channels", "fmi_flux_forward_control", "fmi_flux_denoise_control", "fmi_cast_cols_bf16", "fmi_mask_image",
               "fmi_fill_condition")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = L.load()
    for s in NEW_SYMBOLS:
        assert s in L.EXPORTED
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None
    assert re.search(r"typedef\s+struct\s+fmi_flux_control\s*\{", code)
    assert lib.fmi_abi_version() == 6 and "#define FMI_ABI_VERSION 6" in hdr
    # fmi_flux_config is unchanged: the conditioning width is an argument of the new constructor
    assert [f[0] for f in L.FluxConfig._fields_] == ["in_channels", "pooled_projection_dim", "joint_attention_dim", "num_attention_heads", "num_layers",
                                                     "num_single_layers", "guidance_embeds", "axes_dim", "theta"]
    assert C.sizeof(L.FluxConfig) == 44
    # the ctypes mirror of fmi_flux_control: pointer, int with C's padding
    T = L.FluxControl
    assert [f[0] for f in T._fields_] == ["cond", "cond_dtype"]
    assert (T.cond.offset, T.cond_dtype.offset, C.sizeof(T)) == (0, 8, 16)
    assert len(lib.fmi_flux_create_cond.argtypes) == 4
    assert len(lib.fmi_flux_forward_control.argtypes) == 5 and lib.fmi_flux_forward_control.argtypes[2] == C.POINTER(L.FluxControl)
    a = lib.fmi_flux_denoise_control.argtypes
    assert len(a) == 11 and a[2] == C.POINTER(L.FluxControl) and a[3] == C.POINTER(L.FluxTrueCfg)
    a = lib.fmi_cast_cols_bf16.argtypes
    assert len(a) == 9 and a[2] == C.c_int64 and a[3] == C.c_int64
    assert len(lib.fmi_mask_image.argtypes) == 8 and len(lib.fmi_fill_condition.argtypes) == 7


def test_refusals_before_any_launch():
    lib = L.load()
    buf = (C.c_float * 64)()  # non-null pointers: the refusals below come from the other arguments (nothing is launched, nothing allocated)
    cfg = L.FluxConfig(64, 64, 128, 2, 2, 2, 1, (C.c_int * 3)(16, 56, 56), 10000)
    h = C.c_void_p()
    for bad in (-64, 32, 100, 512):  # negative; no multiple of 64 (twice); 64 + 512 > 512
        assert lib.fmi_flux_create_cond(C.byref(cfg), bad, L.MODEL_BF16, C.byref(h)) == L.ERR_INVALID, bad
        assert h.value is None
    assert lib.fmi_flux_create_cond(None, 64, L.MODEL_BF16, C.byref(h)) == L.ERR_INVALID
    assert lib.fmi_flux_cond_channels(None) == 0
    cast = lib.fmi_cast_cols_bf16
    assert cast(None, L.F32, 8, 8, 8, buf, 16, 0, None) == L.ERR_INVALID
    assert cast(buf, L.F32, 8, 8, 8, None, 16, 0, None) == L.ERR_INVALID
    assert cast(buf, L.F32, 8, 8, 4, buf, 16, 0, None) == L.ERR_INVALID  # cols no multiple of 8
    assert cast(buf, L.F32, 8, 8, 8, buf, 20, 0, None) == L.ERR_INVALID  # dst_ld
    assert cast(buf, L.F32, 8, 8, 8, buf, 16, 4, None) == L.ERR_INVALID  # col0
    assert cast(buf, L.F32, 8, 8, 8, buf, 16, 16, None) == L.ERR_INVALID  # the window leaves the row
    assert cast(buf, L.F32, 8, 3, 8, buf, 16, 0, None) == L.ERR_INVALID  # rows_src does not divide rows
    assert cast(buf, L.F32, 8, 0, 8, buf, 16, 0, None) == L.ERR_INVALID
    assert cast(buf, L.F16, 8, 8, 8, buf, 16, 0, None) == L.ERR_INVALID  # F32 | BF16 only
    assert cast(buf, L.F32, 0, 8, 8, buf, 16, 0, None) == 0  # no rows: nothing to do
    assert lib.fmi_mask_image(None, buf, 1, 3, 4, 4, buf, None) == L.ERR_INVALID
    assert lib.fmi_mask_image(buf, None, 1, 3, 4, 4, buf, None) == L.ERR_INVALID
    assert lib.fmi_mask_image(buf, buf, 1, 0, 4, 4, buf, None) == L.ERR_INVALID
    assert lib.fmi_mask_image(buf, buf, 0, 3, 4, 4, buf, None) == 0
    assert lib.fmi_fill_condition(None, buf, 1, 16, 16, buf, None) == L.ERR_INVALID
    assert lib.fmi_fill_condition(buf, buf, 1, 24, 16, buf, None) == L.ERR_INVALID  # H no multiple of 16
    assert lib.fmi_fill_condition(buf, buf, 1, 16, 8, buf, None) == L.ERR_INVALID
    assert lib.fmi_fill_condition(buf, buf, 0, 16, 16, buf, None) == 0
    # a null handle is refused by both evaluation entries
    assert lib.fmi_flux_forward_control(None, None, None, None, None) == L.ERR_INVALID
    assert lib.fmi_flux_denoise_control(None, None, None, None, None, None, 0, None, None, None, None) == L.ERR_INVALID


# ------------------------------------------------------------------------------------------------ the loader
def test_pipeline_conditioning_and_the_channel_agreement():
    pc = loader.pipeline_conditioning
    assert (pc("FluxPipeline"), pc("FluxKontextPipeline"), pc("FluxControlPipeline"), pc("FluxFillPipeline")) == (None, None, "control", "fill")
    for other in ("StableDiffusionPipeline", "FluxControlNetPipeline", None, ""):
        with pytest.raises(ValueError, match="Only FluxPipeline is supported"):
            pc(other)
    assert loader.SUPPORTED_PIPELINES == ("FluxPipeline", "FluxKontextPipeline")  # check_pipeline_class keeps refusing what it refused
    with pytest.raises(ValueError, match="Only FluxPipeline is supported"):
        loader.check_pipeline_class("FluxFillPipeline")
    chk = loader.check_conditioning_channels
    assert chk("FluxPipeline", 64) is None and chk("FluxPipeline", 64, None) is None and chk("FluxKontextPipeline", 64, 64) is None
    assert chk("FluxControlPipeline", 128, 64) == "control" and chk("FluxFillPipeline", 384, 64) == "fill"
    for cls, cin, cout in (("FluxPipeline", 128, 64), ("FluxControlPipeline", 64, None), ("FluxControlPipeline", 384, 64), ("FluxFillPipeline", 128, 64),
                           ("FluxFillPipeline", 384, None), ("FluxKontextPipeline", 384, 64)):
        with pytest.raises(ValueError, match="conditioning channels"):
            chk(cls, cin, cout)
    with pytest.raises(ValueError, match="Only FluxPipeline is supported"):
        chk("StableDiffusionPipeline", 64, 64)


def test_out_channels_in_the_tensor_shapes():
    plain = synth.flux_tensor_shapes(SMALL_FLUX)
    assert synth.flux_tensor_shapes(dict(SMALL_FLUX, out_channels=None)) == plain and synth.flux_tensor_shapes(dict(SMALL_FLUX, out_channels=64)) == plain
    assert list(synth.flux_tensor_shapes(dict(SMALL_FLUX, out_channels=None))) == list(plain)  # and in the same order
    D = SMALL_FLUX["num_attention_heads"] * 128
    for K in (128, 384):
        t = synth.flux_tensor_shapes(dict(SMALL_FLUX, in_channels=K, out_channels=64))
        assert t["x_embedder.weight"] == (D, K) and t["proj_out.weight"] == (64, D) and t["proj_out.bias"] == (64,)
        assert {k: v for k, v in t.items() if k != "x_embedder.weight"} == {k: v for k, v in plain.items() if k != "x_embedder.weight"}
        sd = synth.flux_state_dict_numpy(dict(SMALL_FLUX, in_channels=K, out_channels=64), seed=0)
        assert sd["x_embedder.weight"].shape == (D, K) and sd["proj_out.weight"].shape == (64, D)
    assert F.state_channels(SMALL_FLUX) == 64 and F.state_channels(dict(SMALL_FLUX, in_channels=384, out_channels=64)) == 64
    assert F.state_channels(dict(SMALL_FLUX, in_channels=128, out_channels=None)) == 128


# ------------------------------------------------------------------------------------------------ the argument checks
def test_check_control_args():
    chk = F.check_control_args
    img = (2, 24, 64)
    assert chk(0, img) is None and chk(64, img, (2, 24, 64)) is None and chk(320, img, [2, 24, 320]) is None
    with pytest.raises(ValueError, match="control= .* is required"):
        chk(320, img)
    with pytest.raises(ValueError, match="channel-conditioned model"):
        chk(0, img, (2, 24, 64))
    for bad in ((2, 24, 320), (1, 24, 64), (2, 23, 64), (2, 24), (2, 24, 64, 1)):
        with pytest.raises(ValueError, match="control is"):
            chk(64, img, bad)
    with pytest.raises(ValueError, match="context="):
        F.check_combination({"control", "context"})
    with pytest.raises(ValueError, match="step cache"):
        F.check_combination({"control", "cache"})
    with pytest.raises(ValueError, match="sequence parallelism"):
        F.check_combination({"control", "sequence_parallel"})


def test_check_control_request():
    chk, kind = pl.check_control_request, pl.control_kind
    assert (kind(0), kind(64), kind(320)) == (None, "control", "fill")
    with pytest.raises(ValueError, match="neither"):
        kind(128)
    H, W = 32, 48
    assert chk(None, H, W) is None
    assert chk("control", H, W, (1, 3, H, W)) is None and chk("control", H, W, (H, W, 3), True) is None
    assert chk("fill", H, W, (H, W, 3), True, (H, W)) is None
    with pytest.raises(ValueError, match="need a channel-conditioned model"):
        chk(None, H, W, (1, 3, H, W))
    with pytest.raises(ValueError, match="need a channel-conditioned model"):
        chk(None, H, W, None, False, (H, W))
    with pytest.raises(ValueError, match="control_image= is required"):
        chk("control", H, W)
    with pytest.raises(ValueError, match="control_image= is required"):
        chk("fill", H, W, None, False, (H, W))
    with pytest.raises(ValueError, match="needs control_mask="):
        chk("fill", H, W, (1, 3, H, W))
    with pytest.raises(ValueError, match="goes with a Fill model"):
        chk("control", H, W, (1, 3, H, W), False, (H, W))
    with pytest.raises(ValueError, match="multiples of 16"):
        chk("control", 40, W, (1, 3, 40, W))
    for shape, u8 in (((2, 3, H, W), False), ((3, H, W), False), ((1, H, W, 3), True), ((W, H, 3), True), ((H, W, 3), False)):
        with pytest.raises(ValueError, match="control_image must be"):
            chk("control", H, W, shape, u8)
    with pytest.raises(ValueError, match="control_mask must be"):
        chk("fill", H, W, (1, 3, H, W), False, (1, H, W))
    with pytest.raises(ValueError, match="reference="):
        F.check_combination({"control", "context"}, pl.REQUEST_NAMES)
    with pytest.raises(ValueError, match="step cache"):
        F.check_combination({"control", "cache"}, pl.REQUEST_NAMES)
    with pytest.raises(ValueError, match="sequence parallelism"):
        F.check_combination({"control", "sequence_parallel"}, pl.REQUEST_NAMES)


# ------------------------------------------------------------------------------------------------ the request path
H = W = 16


class _Flux:
    def __init__(self, cond_channels):
        self.cond_channels = cond_channels


class RecordingPipeline(pl.Pipeline):
    def __init__(self, cond_channels):  # no GPU: only the request path in front of the chunk body is under test
        self.device = torch.device("cpu")
        self.flux = _Flux(cond_channels)
        self.calls = []

    def _generate_chunk(self, s, *a, **kw):
        self.calls.append((s, a, kw))
        return torch.stack([torch.full((3, H, W), i % 256, dtype=torch.uint8) for i in s.sample_ids])


def _params():
    return pl.DiffusionGenerationParams(H, W, 2, 3.5)


def _prompts(B):
    return [f"p{b}" for b in range(B)]


def test_samples_has_no_control_field_and_the_chunk_signature_ends_with_it():
    import inspect
    assert [f.name for f in dataclasses.fields(pl._Samples)] == ["prompts", "sample_ids", "embeddings", "token_ids", "latents", "image", "mask", "reference"]
    assert [f.name for f in dataclasses.fields(pl._Control)] == ["kind", "image", "mask"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        pl._Control("control", torch.zeros(1, 3, H, W)).kind = "fill"
    assert list(inspect.signature(pl.Pipeline._generate_chunk).parameters) == ["self", "s", "params", "seed", "strength", "return_latents", "cache_threshold", "stats",
                                                                               "negative", "control", "controlnet", "ip_adapter"]


def test_one_control_is_shared_by_every_chunk():
    pipe = RecordingPipeline(320)
    image, mask = torch.rand(1, 3, H, W) * 2 - 1, np.random.default_rng(0).random((H, W)) > 0.5
    out = pipe.generate_tensor(_prompts(11), _params(), seed=3, control_image=image, control_mask=mask)
    assert [len(s.prompts) for s, _, _ in pipe.calls] == [8, 3] and out[:, 0, 0, 0].tolist() == list(range(11))
    assert all(set(kw) == {"control"} for _, _, kw in pipe.calls) and all(len(a) == 6 for _, a, _ in pipe.calls)
    c = pipe.calls[0][2]["control"]
    assert all(kw["control"] is c for _, _, kw in pipe.calls)  # ONE object, shared by all chunks
    assert c.kind == "fill" and tuple(c.image.shape) == (1, 3, H, W) and c.image.dtype == torch.float32 and torch.equal(c.image, image)
    assert tuple(c.mask.shape) == (1, H, W) and c.mask.dtype == torch.float32 and np.array_equal(c.mask[0].numpy(), mask.astype(np.float32))
    # with a negative both keywords ride, in chunks of four
    pipe.calls.clear()
    pipe.generate_tensor(_prompts(5), _params(), control_image=image, control_mask=mask, negative_prompt="x", true_cfg_scale=4.0)
    assert [len(s.prompts) for s, _, _ in pipe.calls] == [4, 1] and all(set(kw) == {"control", "negative"} for _, _, kw in pipe.calls)
    # a Canny / Depth model: the image alone, numpy accepted
    pipe = RecordingPipeline(64)
    pipe.generate_tensor(_prompts(2), _params(), control_image=image.numpy())
    c = pipe.calls[0][2]["control"]
    assert c.kind == "control" and c.mask is None and torch.equal(c.image, image)
    # image= / strength= / mask= keep their meaning next to the control: per-sample fields as ever
    pipe.calls.clear()
    pipe.generate_tensor(_prompts(2), _params(), control_image=image, image=torch.zeros(1, 3, H, W), strength=0.5, mask=torch.ones(H, W))
    s, a, kw = pipe.calls[0]
    assert tuple(s.image.shape) == (2, 3, H, W) and tuple(s.mask.shape) == (2, H, W) and a[2] == 0.5 and set(kw) == {"control"}


def test_without_a_control_the_chunk_call_is_todays():
    pipe = RecordingPipeline(0)
    pipe.generate_tensor(_prompts(3), _params(), seed=3)
    assert [(len(a), kw) for _, a, kw in pipe.calls] == [(6, {})]


def test_control_request_errors():
    image, mask = torch.zeros(1, 3, H, W), torch.zeros(H, W)
    plain, ctl, fill = RecordingPipeline(0), RecordingPipeline(64), RecordingPipeline(320)
    with pytest.raises(ValueError, match="need a channel-conditioned model"):
        plain.generate_tensor(_prompts(1), _params(), control_image=image)
    with pytest.raises(ValueError, match="need a channel-conditioned model"):
        plain.generate_tensor(_prompts(1), _params(), control_mask=mask)
    with pytest.raises(ValueError, match="control_image= is required"):
        ctl.generate_tensor(_prompts(1), _params())
    with pytest.raises(ValueError, match="control_image= is required"):
        fill.generate_tensor(_prompts(1), _params(), control_mask=mask)
    with pytest.raises(ValueError, match="needs control_mask="):
        fill.generate_tensor(_prompts(1), _params(), control_image=image)
    with pytest.raises(ValueError, match="goes with a Fill model"):
        ctl.generate_tensor(_prompts(1), _params(), control_image=image, control_mask=mask)
    with pytest.raises(ValueError, match="control_image must be"):
        ctl.generate_tensor(_prompts(2), _params(), control_image=torch.zeros(2, 3, H, W))  # one control per request, not one per prompt
    with pytest.raises(ValueError, match="control_image must be uint8 or float"):
        ctl.generate_tensor(_prompts(1), _params(), control_image=torch.zeros(1, 3, H, W, dtype=torch.int32))
    with pytest.raises(ValueError, match="control_mask must be a bool or float"):
        fill.generate_tensor(_prompts(1), _params(), control_image=image, control_mask=torch.zeros(H, W, dtype=torch.int32))
    with pytest.raises(ValueError, match="numpy array or a torch tensor"):
        ctl.generate_tensor(_prompts(1), _params(), control_image=[[0.0]])
    with pytest.raises(ValueError, match="reference="):
        ctl.generate_tensor(_prompts(1), _params(), control_image=image, reference=torch.zeros(1, 3, 32, 16))
    with pytest.raises(ValueError, match="step cache"):
        ctl.generate_tensor(_prompts(1), _params(), control_image=image, cache_threshold=0.1)
    ctl._sp = object()
    with pytest.raises(ValueError, match="sequence parallelism"):
        ctl.generate_tensor(_prompts(1), _params(), control_image=image)
    with pytest.raises(ValueError, match="multiples of 16"):
        RecordingPipeline(64).generate_tensor(_prompts(1), pl.DiffusionGenerationParams(24, 16, 2, 3.5), control_image=torch.zeros(1, 3, 24, 16))
    assert not plain.calls and not ctl.calls and not fill.calls  # every check raised before any chunk ran


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("hw", [(48, 80), (16, 16)])
def test_mask_pack_reference_is_the_view_chain(hw):
    from oracle import oracle as orc
    m = np.random.default_rng(3).random((2, *hw)).astype(np.float32)
    m[0, :8, :8], m[1, 3, 5], m[1, 4, 6], m[1, 5, 7] = 0.5, 0.5, 0.0, 1.0
    a, b = CR.pack_mask(m), CR.pack_mask_view_chain(m, orc.pack_latents)
    assert a.shape == (2, (hw[0] // 16) * (hw[1] // 16), 256) and set(np.unique(a)) == {0.0, 1.0}
    np.testing.assert_array_equal(a, b)
    assert a[0, 0, 0] == 1.0  # exactly 0.5 counts as 1
    lat = np.random.default_rng(4).standard_normal((2, a.shape[1], 64)).astype(np.float32)
    c = CR.fill_condition(lat, m)
    assert c.shape == (2, a.shape[1], 320) and np.array_equal(c[:, :, :64], lat) and np.array_equal(c[:, :, 64:], a)
    img = np.random.default_rng(5).standard_normal((2, 3, *hw)).astype(np.float32)
    mi = CR.mask_image(img, m)
    assert np.array_equal(mi[:, :, m[0] < 0.5][0], img[:, :, m[0] < 0.5][0]) and (mi[0][:, m[0] >= 0.5] == 0).all()


TS4 = [1.0, 0.8, 0.55, 0.3, 0.0]


@pytest.mark.parametrize("hw", [(6, 4), (5, 7)])
@pytest.mark.parametrize("K", [128, 384])
def test_composed_reference_self_test(K, hw):
    """Each wrong composition lies at least 9e-2 from the correct loop — 3 x the 3e-2 loop bar, so that the GPU test's one-third criterion means something —
    and the zero-padded rows of proj_out come back exactly 0.  Measured here: 0.22 .. 0.41 over both widths and both grids."""
    from oracle import oracle as orc
    cfg = dict(SMALL_FLUX, in_channels=K, out_channels=64)
    sd = synth.flux_state_dict_numpy(cfg, seed=0)
    om = orc.Flux(CR.oracle_cfg(cfg))
    om.load(CR.oracle_state_dict(sd, cfg))
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, 2, hw, 32, seed=41)
    cond = np.random.default_rng(44).standard_normal((2, hw[0] * hw[1], K - 64)).astype(np.float32)
    g = np.full(2, 3.5, np.float32)
    full = om.forward(np.concatenate([img, cond], 2), ids, txt, txt_ids, np.full(2, 0.8, np.float32), y, g)
    assert full.shape == (2, hw[0] * hw[1], K) and not full[:, :, 64:].any() and np.abs(full[:, :, :64]).max() > 0.1
    ref = CR.control_loop(om, img, cond, ids, txt, txt_ids, y, g, TS4)
    assert ref.shape == img.shape and np.isfinite(ref).all()
    for v in CR.VARIANTS:
        dist = rel_l2(CR.control_loop(om, img, cond, ids, txt, txt_ids, y, g, TS4, variant=v), ref)
        print(f"K={K} grid {hw}: {v} rel-L2 {dist:.3f}")
        assert dist >= 9e-2, v
