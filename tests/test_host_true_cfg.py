"""True classifier-free guidance, the parts that need no device: the C-ABI additions and their ctypes mirror, the pure argument check,
the request path of the pipeline (the negative is ONE per request: a keyword of true-CFG chunks only, never a field of _Samples), and a self-test of the
composed CPU reference tests/true_cfg_ref.py that the GPU tests measure against.

Three cases here pass on the code before the feature too, on purpose: test_composed_reference_self_test (both shapes) tests the reference, not the library — it
is the precondition of the GPU test's one-third criterion — and the case without any CFG argument of test_without_cfg_the_chunk_call_is_todays pins today's
chunk call.  Every other test of this file, and every test of tests/test_gpu_true_cfg.py, fails without the feature (missing symbol or keyword)."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from diffusion_rs_amd import _lib as L
from diffusion_rs_amd import flux as F
from diffusion_rs_amd import pipeline as pl
from tests import true_cfg_ref as R
from tests.util import SMALL_FLUX, flux_inputs, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = L.load()
    for s in ("fmi_flux_denoise_cfg", "fmi_cfg_euler_step"):
        assert s in L.EXPORTED
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None
    assert re.search(r"typedef\s+struct\s+fmi_flux_true_cfg\s*\{", code)
    assert lib.fmi_abi_version() == 6 and "#define FMI_ABI_VERSION 6" in hdr
    # the ctypes mirror of fmi_flux_true_cfg: pointer, int, pointer, int, float with C's padding
    assert [f[0] for f in L.FluxTrueCfg._fields_] == ["neg_txt", "neg_txt_dtype", "neg_y", "neg_y_dtype", "scale"]
    T = L.FluxTrueCfg
    assert (T.neg_txt.offset, T.neg_txt_dtype.offset, T.neg_y.offset, T.neg_y_dtype.offset, T.scale.offset) == (0, 8, 16, 24, 28)
    assert C.sizeof(T) == 32
    assert len(lib.fmi_flux_denoise_cfg.argtypes) == 11 and lib.fmi_flux_denoise_cfg.argtypes[3] == C.POINTER(L.FluxTrueCfg)
    assert len(lib.fmi_cfg_euler_step.argtypes) == 11 and lib.fmi_cfg_euler_step.argtypes[5] == C.c_int64


def test_cfg_euler_step_rejects_bad_arguments_before_any_launch():
    lib = L.load()
    buf = (C.c_float * 8)()  # non-null pointers: the refusals below come from the other arguments (nothing is launched)
    assert lib.fmi_cfg_euler_step(None, buf, buf, 1.0, 0.1, 8, None, None, None, 0.0, None) == L.ERR_INVALID
    assert lib.fmi_cfg_euler_step(buf, buf, None, 1.0, 0.1, 8, None, None, None, 0.0, None) == L.ERR_INVALID
    assert lib.fmi_cfg_euler_step(buf, buf, buf, 1.0, 0.1, -1, None, None, None, 0.0, None) == L.ERR_INVALID
    for bad in (-0.5, float("nan"), float("inf")):
        assert lib.fmi_cfg_euler_step(buf, buf, buf, bad, 0.1, 8, None, None, None, 0.0, None) == L.ERR_INVALID
    assert lib.fmi_cfg_euler_step(buf, buf, buf, 1.0, 0.1, 8, buf, None, buf, 0.0, None) == L.ERR_INVALID  # x0 / noise / mask in part
    assert lib.fmi_cfg_euler_step(buf, buf, buf, 1.0, 0.1, 0, None, None, None, 0.0, None) == 0  # n = 0: nothing to do


# ------------------------------------------------------------------------------------------------ check_true_cfg_args
def test_check_true_cfg_args():
    txt, y = (2, 32, 128), (2, 64)
    chk = F.check_true_cfg_args
    assert chk(txt, y) is None  # no negative: the plain loop
    assert chk(txt, y, txt, y) == 1.0 and chk(txt, y, txt, y, 4) == 4.0 and chk(txt, y, txt, y, 0.0) == 0.0
    assert isinstance(chk(txt, y, list(txt), list(y), 2), float)
    assert chk((4, 32, 128), (4, 64), (4, 32, 128), (4, 64), 2.5) == 2.5  # B = 4 is the largest
    with pytest.raises(ValueError, match="needs negative_txt"):
        chk(txt, y, true_cfg_scale=4.0)
    with pytest.raises(ValueError, match="go together"):
        chk(txt, y, txt, None, 4.0)
    with pytest.raises(ValueError, match="go together"):
        chk(txt, y, None, y, 4.0)
    with pytest.raises(ValueError, match="T included"):
        chk(txt, y, (2, 16, 128), y, 4.0)  # another T
    with pytest.raises(ValueError, match="T included"):
        chk(txt, y, (1, 32, 128), y, 4.0)  # one row for two samples: the C ABI takes B rows
    with pytest.raises(ValueError, match="negative_y is"):
        chk(txt, y, txt, (2, 32), 4.0)
    with pytest.raises(ValueError, match="B = 5 > 4"):
        chk((5, 32, 128), (5, 64), (5, 32, 128), (5, 64), 4.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and >= 0"):
            chk(txt, y, txt, y, bad)
    with pytest.raises(ValueError, match="step cache"):
        F.check_combination({"true_cfg", "cache"})
    with pytest.raises(ValueError, match="sequence parallelism"):
        F.check_combination({"true_cfg", "sequence_parallel"})


# ------------------------------------------------------------------------------------------------ the request path
H = W = 16


class RecordingPipeline(pl.Pipeline):
    def __init__(self):  # no GPU: only the request path in front of the chunk body is under test
        self.device = torch.device("cpu")
        self.calls = []

    def _generate_chunk(self, s, *a, **kw):
        self.calls.append((s, a, kw))
        return torch.stack([torch.full((3, H, W), i % 256, dtype=torch.uint8) for i in s.sample_ids])


def _params():
    return pl.DiffusionGenerationParams(H, W, 2, 3.5)


def _prompts(B):
    return [f"p{b}" for b in range(B)]


def test_samples_has_no_negative_field():
    assert [f.name for f in dataclasses.fields(pl._Samples)] == ["prompts", "sample_ids", "embeddings", "token_ids", "latents", "image", "mask", "reference"]
    assert [f.name for f in dataclasses.fields(pl._Negative)] == ["scale", "prompt", "embeddings", "token_ids"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        pl._Negative(4.0, "x").scale = 2.0


@pytest.mark.parametrize("B,sizes", [(5, [4, 1]), (8, [4, 4]), (3, [3]), (9, [4, 4, 1])])
def test_cfg_chunks_hold_half_a_batch_and_share_one_negative(B, sizes):
    pipe = RecordingPipeline()
    assert pipe.MAX_BATCH // 2 == 4
    out = pipe.generate_tensor(_prompts(B), _params(), seed=3, negative_prompt="x", true_cfg_scale=4.0)
    assert [len(s.prompts) for s, _, _ in pipe.calls] == sizes
    assert out[:, 0, 0, 0].tolist() == list(range(B))
    negs = [kw["negative"] for _, _, kw in pipe.calls]
    assert all(set(kw) == {"negative"} for _, _, kw in pipe.calls)
    assert all(n is negs[0] for n in negs)  # ONE object, shared by all chunks
    assert negs[0] == pl._Negative(4.0, "x", None, None)
    assert all(len(a) == 6 for _, a, _ in pipe.calls)  # the pinned positional arguments: params, seed, strength, return_latents, cache_threshold, stats


def test_negative_embeddings_and_token_ids_reach_the_chunks_as_given():
    pipe = RecordingPipeline()
    B = 2
    emb = (torch.zeros(B, 4, 6), torch.zeros(B, 5))
    neg = (torch.ones(1, 4, 6), torch.ones(1, 5))
    pipe.generate_tensor(_prompts(B), _params(), embeddings=emb, negative_embeddings=neg, true_cfg_scale=2.0)
    n = pipe.calls[0][2]["negative"]
    assert n.scale == 2.0 and n.prompt is None and n.token_ids is None and n.embeddings[0] is neg[0] and n.embeddings[1] is neg[1]
    pipe.calls.clear()
    ids = (np.zeros((B, 7), np.int32), np.zeros((B, 3), np.int32))
    nids = (np.ones((1, 7), np.int32), np.ones((1, 3), np.int32))
    pipe.generate_tensor(_prompts(B), _params(), token_ids=ids, negative_token_ids=nids, true_cfg_scale=2.0)
    n = pipe.calls[0][2]["negative"]
    assert n.embeddings is None and n.token_ids[0] is nids[0] and n.token_ids[1] is nids[1]


@pytest.mark.parametrize("kw", [dict(), dict(negative_prompt="x"), dict(negative_prompt="x", true_cfg_scale=1.0), dict(negative_prompt="x", true_cfg_scale=0.5),
                                dict(negative_embeddings=(torch.ones(1, 4, 6), torch.ones(1, 5)), true_cfg_scale=1.0), dict(true_cfg_scale=0.0)])
def test_without_cfg_the_chunk_call_is_todays(kw):
    """no negative, or a scale <= 1 (diffusers' do_true_cfg is off): chunks of MAX_BATCH and NO negative keyword — the exact call of a request without CFG"""
    pipe = RecordingPipeline()
    pipe.generate_tensor(_prompts(11), _params(), seed=5, **kw)
    assert [len(s.prompts) for s, _, _ in pipe.calls] == [8, 3]
    assert all(k == {} and len(a) == 6 for _, a, k in pipe.calls)


def test_request_refusals_come_before_any_chunk():
    pipe = RecordingPipeline()
    go = lambda **kw: pipe.generate_tensor(_prompts(2), _params(), **kw)
    with pytest.raises(ValueError, match="needs a negative"):
        go(true_cfg_scale=4.0)
    with pytest.raises(ValueError, match="finite and >= 0"):
        go(negative_prompt="x", true_cfg_scale=float("nan"))
    with pytest.raises(ValueError, match="finite and >= 0"):
        go(negative_prompt="x", true_cfg_scale=-2.0)
    with pytest.raises(ValueError, match="step cache"):
        go(negative_prompt="x", true_cfg_scale=4.0, cache_threshold=0.1)
    with pytest.raises(ValueError, match="exclude one another"):
        go(negative_prompt="x", negative_embeddings=(torch.ones(1, 4, 6), torch.ones(1, 5)), true_cfg_scale=4.0)
    ids = (np.zeros((2, 7), np.int32), np.zeros((2, 3), np.int32))
    with pytest.raises(ValueError, match="takes the prompt's T"):
        go(token_ids=ids, negative_token_ids=(np.ones((1, 9), np.int32), np.ones((1, 3), np.int32)), true_cfg_scale=4.0)
    emb = (torch.zeros(2, 4, 6), torch.zeros(2, 5))
    with pytest.raises(ValueError, match="takes the prompt's T"):
        go(embeddings=emb, negative_embeddings=(torch.ones(1, 3, 6), torch.ones(1, 5)), true_cfg_scale=4.0)
    with pytest.raises(ValueError, match="ONE row each"):
        go(embeddings=emb, negative_embeddings=(torch.ones(2, 4, 6), torch.ones(2, 5)), true_cfg_scale=4.0)  # per-prompt negatives are out of scope
    with pytest.raises(ValueError, match="negative_embeddings="):
        go(embeddings=emb, negative_prompt="x", true_cfg_scale=4.0)
    with pytest.raises(ValueError, match="negative_token_ids="):
        go(token_ids=ids, negative_prompt="x", true_cfg_scale=4.0)
    with pytest.raises(ValueError, match="goes with token_ids="):
        go(negative_token_ids=(np.ones((1, 7), np.int32), np.ones((1, 3), np.int32)), true_cfg_scale=4.0)
    with pytest.raises(ValueError, match="takes the prompt's T"):
        go(token_ids=ids, negative_token_ids=(np.ones((1, 7), np.int32), np.ones((1, 4), np.int32)), true_cfg_scale=4.0)  # the clip member's length
    pipe._sp = object()  # what enable_sequence_parallel leaves behind
    try:
        with pytest.raises(ValueError, match="sequence parallelism"):
            go(negative_prompt="x", true_cfg_scale=4.0)
        go(negative_prompt="x", true_cfg_scale=1.0)  # CFG off: the request runs, one sample per chunk
        assert [len(s.prompts) for s, _, _ in pipe.calls] == [1, 1] and all(k == {} for _, _, k in pipe.calls)
    finally:
        pipe._sp = None
    assert len(pipe.calls) == 2  # none of the refused requests reached a chunk


def test_forward_hands_the_shared_negative_through():
    pipe = RecordingPipeline()
    out = pipe.forward(_prompts(5), _params(), output="tensor", negative_prompt="x", true_cfg_scale=3.0, seed=1)
    assert out.shape[0] == 5 and [len(s.prompts) for s, _, _ in pipe.calls] == [4, 1]
    assert all(kw["negative"] == pl._Negative(3.0, "x") for _, _, kw in pipe.calls)
    pipe.calls.clear()
    pipe.forward(_prompts(5), _params(), output="tensor", seed=1)
    assert [len(s.prompts) for s, _, _ in pipe.calls] == [5] and pipe.calls[0][2] == {}


# ------------------------------------------------------------------------------------------------ the composed reference
B, T = 2, 32
SHAPES = {"ragged": (4, 6), "aligned": (8, 8)}
TS4 = [1.0, 0.8, 0.55, 0.3, 0.0]


@pytest.fixture(scope="module")
def oracle_model():
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    om = orc.Flux(SMALL_FLUX)
    om.load(d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0))
    return om


@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_composed_reference_self_test(oracle_model, shape):
    """The exact cases of the combine, and the precondition of the GPU test's one-third criterion: every wrong variant is at least 5e-3 from the correct loop."""
    om = oracle_model
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, SHAPES[shape], T, seed=41)
    _, _, ntxt, _, ny = flux_inputs(SMALL_FLUX, B, SHAPES[shape], T, seed=43)
    g = np.full(B, 3.5, np.float32)
    run = lambda scale, nt=ntxt, nyy=ny, **kw: R.cfg_loop(om, img, ids, txt, txt_ids, y, nt, nyy, g, TS4, scale, **kw)
    correct = run(4.0)
    assert correct.dtype == np.float32 and correct.shape == img.shape and np.isfinite(correct).all()
    np.testing.assert_array_equal(run(4.0), correct)  # the reference is deterministic
    neg_only = run(4.0, variant="negative_only")
    pos_only = run(4.0, variant="positive_only")
    np.testing.assert_array_equal(run(0.0), neg_only)  # scale 0: the negative's loop, exactly
    for scale in (0.0, 1.0, 4.0):
        np.testing.assert_array_equal(run(scale, nt=txt, nyy=y), pos_only)  # identical negatives: the prompt's loop, exactly
    for v in R.VARIANTS:
        dist = rel_l2(run(4.0, variant=v), correct)
        print(f"{shape}: {v}: rel-L2 {dist:.3e} from the correct loop")
        assert dist >= 5e-3, v
    print(f"{shape}: {R.SCALE_VARIANT}: rel-L2 {rel_l2(run(4.0, variant=R.SCALE_VARIANT), correct):.3e} from the correct loop (reported: it is no plumbing mistake)")
