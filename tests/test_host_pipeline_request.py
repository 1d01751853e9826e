"""The request path of Pipeline.generate_tensor without a GPU: every per-sample input follows its prompt through _Samples.take — into the
MAX_BATCH chunks, the single samples of sequence parallelism and the broadcast of one image — and the checks raise before any chunk runs.  The chunk body is
replaced by a recorder; image / reference are float tensors (the u8 form needs the GPU op and stays in the GPU tests)."""
import dataclasses

import numpy as np
import pytest
import torch

from diffusion_rs_amd import flux as F
from diffusion_rs_amd import pipeline as pl

H = W = 16
S = 1  # packed latent rows of a 16 x 16 image


class RecordingPipeline(pl.Pipeline):
    def __init__(self):  # no GPU: only the request path in front of the chunk body is under test
        self.device = torch.device("cpu")
        self.chunks = []

    def _generate_chunk(self, s, params, seed, strength, return_latents, cache_threshold, stats):
        self.chunks.append((s, dict(params=params, seed=seed, strength=strength, return_latents=return_latents, cache_threshold=cache_threshold, stats=stats)))
        u8 = torch.stack([torch.full((3, params.height, params.width), i % 256, dtype=torch.uint8) for i in s.sample_ids])
        return (u8, torch.tensor(s.sample_ids, dtype=torch.float32)[:, None, None].expand(-1, S, 64)) if return_latents else u8


def _params():
    return pl.DiffusionGenerationParams(H, W, 2, 3.5)


def _ramp(B, *trailing, dtype=torch.float32):
    """(B, *trailing) whose row b holds the value b"""
    return torch.arange(B, dtype=dtype).reshape(B, *[1] * len(trailing)).expand(B, *trailing).clone()


def _inputs(B):
    """Every per-sample input of generate_tensor with row b = b, each with trailing dimensions of its own."""
    return dict(embeddings=(_ramp(B, 4, 6), _ramp(B, 5)), token_ids=(_ramp(B, 7, dtype=torch.int32).numpy(), _ramp(B, 3, dtype=torch.int32).tolist()),
                latents=_ramp(B, 16, 2, 2), image=_ramp(B, 3, H, W), mask=_ramp(B, H, W), reference=_ramp(B, 3, 32, 16))


def _assert_rows(value, rows, what):
    if isinstance(value, tuple):
        for member in value:
            _assert_rows(member, rows, what)
        return
    got = np.asarray(value)
    assert got.shape[0] == len(rows), what
    for r, b in enumerate(rows):
        assert np.all(got[r] == (f"p{b}" if got.dtype.kind == "U" else b)), (what, r, b)


def _assert_samples(s, rows, first=0):
    for f in dataclasses.fields(pl._Samples):  # a field take() or the request path forgets holds other rows, or the whole batch
        value = getattr(s, f.name)
        assert value is not None, f.name
        _assert_rows(value, [first + b for b in rows] if f.name == "sample_ids" else rows, f.name)


@pytest.mark.parametrize("idx", [slice(1, 4), [4, 0, 2]])
def test_take_selects_the_rows_of_every_field(idx):
    B = 5
    s = pl._Samples([f"p{b}" for b in range(B)], list(range(B)), **_inputs(B))
    assert {f.name for f in dataclasses.fields(s)} == {"prompts", "sample_ids", *_inputs(B)}  # _inputs fills every field: none is skipped as None below
    rows = list(range(B))[idx] if isinstance(idx, slice) else idx
    _assert_samples(s.take(idx), rows)
    _assert_samples(s, list(range(B)))  # the source is left as it was
    sub = pl._Samples(["a", "b"], [3, 4]).take(idx if isinstance(idx, slice) else [1, 0])
    assert all(getattr(sub, f.name) is None for f in dataclasses.fields(sub) if f.name not in ("prompts", "sample_ids"))
    assert "prompts" not in s.kwargs() and set(s.kwargs()) == {f.name for f in dataclasses.fields(s)} - {"prompts"}


def test_index_sets():
    assert pl._index_sets(3, 8, False) == [slice(0, 8)] and pl._index_sets(8, 8, False) == [slice(0, 8)]
    assert pl._index_sets(11, 8, False) == [slice(0, 8), slice(8, 16)]
    assert pl._index_sets(3, 8, True) == [slice(0, 1), slice(1, 2), slice(2, 3)] and pl._index_sets(1, 8, True) == [slice(0, 1)]


@pytest.mark.parametrize("return_latents", [False, True])
def test_more_prompts_than_max_batch_run_in_chunks_of_every_input(return_latents):
    B, pipe = 11, RecordingPipeline()
    out = pipe.generate_tensor([f"p{b}" for b in range(B)], _params(), first_sample=100, seed=5, strength=0.75, return_latents=return_latents,
                               cache_threshold=0.25, **_inputs(B))
    assert len(pipe.chunks) == 2
    _assert_samples(pipe.chunks[0][0], list(range(8)), first=100)
    _assert_samples(pipe.chunks[1][0], [8, 9, 10], first=100)
    shared = pipe.chunks[0][1]
    assert shared == dict(params=_params(), seed=5, strength=0.75, return_latents=return_latents, cache_threshold=0.25, stats=[])
    assert all(pipe.chunks[1][1][k] is v or pipe.chunks[1][1][k] == v for k, v in shared.items()) and pipe.chunks[1][1]["stats"] is shared["stats"]
    u8, lat = out if return_latents else (out, None)
    assert u8.dtype == torch.uint8 and u8.shape == (B, 3, H, W) and [int(u8[b, 0, 0, 0]) for b in range(B)] == [100 + b for b in range(B)]
    assert (u8 == u8[:, :1, :1, :1]).all()
    if return_latents:
        assert lat.shape == (B, S, 64) and lat[:, 0, 0].tolist() == [100.0 + b for b in range(B)]


def test_one_image_mask_and_reference_are_broadcast_over_the_prompts():
    pipe = RecordingPipeline()
    image, mask, reference = torch.full((1, 3, H, W), 0.5), torch.full((H, W), 0.25), torch.full((1, 3, 16, 32), -0.5)
    pipe.generate_tensor(["a", "b", "c"], _params(), image=image, mask=mask, reference=reference)
    (s, _), = pipe.chunks
    assert torch.equal(s.image, image.expand(3, 3, H, W)) and torch.equal(s.mask, mask.expand(3, H, W)) and torch.equal(s.reference, reference.expand(3, 3, 16, 32))
    assert s.sample_ids == [0, 1, 2] and s.embeddings is None and s.token_ids is None and s.latents is None


def test_sequence_parallel_runs_one_sample_per_chunk_and_rejects_what_it_does_not_carry():
    pipe = RecordingPipeline()
    pipe._sp = object()
    B = 3
    given = {k: v for k, v in _inputs(B).items() if k in ("embeddings", "token_ids", "latents")}
    out = pipe.generate_tensor([f"p{b}" for b in range(B)], _params(), sample_ids=[7, 3, 5], seed=2, **given)
    assert len(pipe.chunks) == 3 and out[:, 0, 0, 0].tolist() == [7, 3, 5]
    for b, (s, shared) in enumerate(pipe.chunks):
        assert s.prompts == [f"p{b}"] and s.sample_ids == [[7, 3, 5][b]] and shared["seed"] == 2
        for k in given:
            _assert_rows(getattr(s, k), [b], k)
    pipe.chunks.clear()
    for kw, message in ((dict(image=torch.zeros(1, 3, H, W)), "image= is not wired through sequence parallelism: disable_sequence_parallel\\(\\) first"),
                        (dict(reference=torch.zeros(1, 3, H, W)), "reference= is not wired through sequence parallelism: disable_sequence_parallel\\(\\) first"),
                        (dict(cache_threshold=0.1), "the step cache \\(cache_threshold= / cache_force=\\) is not supported under sequence parallelism")):
        with pytest.raises(ValueError, match=message):
            pipe.generate_tensor(["a", "b"], _params(), **kw)
    assert pipe.chunks == []


def test_an_empty_request_returns_empties_before_any_image_check():
    pipe = RecordingPipeline()
    bad = torch.zeros(2, 5)  # would not pass as an image or a reference
    u8 = pipe.generate_tensor([], _params(), image=bad, reference=bad)
    assert u8.dtype == torch.uint8 and u8.shape == (0, 3, H, W)
    u8, lat = pipe.generate_tensor([], _params(), image=bad, return_latents=True)
    assert u8.shape == (0, 3, H, W) and lat.dtype == torch.float32 and lat.shape == (0, S, 64)
    assert pipe.chunks == []


@pytest.mark.parametrize("kw, message", [
    (dict(sample_ids=[0]), "sample_ids must name one stream per prompt"),
    (dict(mask=torch.ones(H, W)), "mask= needs image=: inpainting repaints part of a source image"),
    (dict(strength=0.5), "strength= needs image=: text to image always runs the whole schedule"),
    (dict(sample_ids=[0], mask=torch.ones(H, W)), "sample_ids must name one stream per prompt"),  # the order of the checks
    (dict(cache_threshold=-1.0, sample_ids=[0]), "cache_threshold must be >= 0"),
])
def test_a_bad_request_raises_before_any_chunk(kw, message):
    pipe = RecordingPipeline()
    with pytest.raises(ValueError, match=message):
        pipe.generate_tensor(["a", "b"], _params(), **kw)
    assert pipe.chunks == []


def test_denoise_shape_check_of_x0_noise_mask():
    img = torch.zeros(2, 4, 64)
    assert F._like_img(None, "x0", img) is None
    for name in ("x0", "noise", "mask"):
        with pytest.raises(ValueError, match=f"denoise: {name} is \\(2, 4, 63\\), img is \\(2, 4, 64\\)"):
            F._like_img(torch.zeros(2, 4, 63), name, img)
    t = F._like_img(torch.ones(2, 64, 4, dtype=torch.float64).transpose(1, 2), "mask", img)
    assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == img.shape and bool((t == 1).all())
