"""Attention key weights on the host: the request's refusals, the dict -> (txt, img) assembly and the request path in front of the chunk body,
without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from diffusion_rs_amd import _lib, pipeline as pl
from tests.test_host_regions import H, W, J, RecordingPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = dict(prompt=np.full(4, 1.3), image=np.full((H // 16, W // 16), 0.5))


@pytest.mark.parametrize("kw,match", [(dict(key_weights=[1.0]), "takes a dict"), (dict(key_weights=dict(text=1.0)), "takes a dict"), (dict(height=40), "multiples of 16"),
                                      (dict(key_weights=dict(prompt=[1.0, 0.0])), "finite and > 0"), (dict(key_weights=dict(image=np.full((2, 3), np.nan))), "finite and > 0"),
                                      (dict(key_weights=dict(image=np.ones((3, 2)))), r"image weights must be \(2,3\)"), (dict(key_weights=dict(redux=2.0)), "without Redux"),
                                      (dict(key_weights=dict(redux=np.ones(5)), redux_rows=729), r"scalar or \(729,\)"),
                                      (dict(present=[("option", pl.REQUEST_NAMES["true_cfg"])]), "not combined with true CFG"),
                                      (dict(present=[("mode", pl.REQUEST_NAMES["int8"])]), "is not supported on a transformer in the int8 mode"),
                                      (dict(text_rows=12, prompt_rows=6), r"must be \(6,\) or \(12,\)")])
def test_check_key_weights_request_refuses_by_name(kw, match):
    ok = dict(key_weights=OK, height=H, width=W)
    assert pl.check_key_weights_request(**ok, text_rows=12, prompt_rows=4) is None
    with pytest.raises(ValueError, match=match):
        pl.check_key_weights_request(**dict(ok, **kw))


def test_key_weight_rows_name_by_name():
    image = np.arange(1, 7, dtype=np.float32).reshape(2, 3)
    txt, img = pl.key_weight_rows(dict(prompt=[2, 3], redux=torch.tensor(0.25), image=image), 6, H, W, redux_rows=3)  # two regions behind a prompt of 2 rows
    assert txt.dtype == img.dtype == np.float32
    assert txt.tolist() == [2, 3, 1, 1, 1, 1, 0.25, 0.25, 0.25] and img.tolist() == [1, 2, 3, 4, 5, 6]
    txt, img = pl.key_weight_rows(dict(redux=[4, 5, 6]), 2, H, W, redux_rows=3)
    assert txt.tolist() == [1, 1, 4, 5, 6] and img.tolist() == [1] * 6
    assert pl.key_weight_rows(dict(prompt=np.arange(1, 7)), 6, H, W)[0].tolist() == [1, 2, 3, 4, 5, 6]


class Recording(RecordingPipeline):
    def __init__(self, fail=False):
        super().__init__(fail)
        self.flux.set_attention_key_weights = lambda t, i: self.calls.append(("weights", t, i))
        self.flux.clear_attention_key_weights = lambda: self.calls.append("unweighted")


def _request(pipe, **kw):
    return pipe.generate_tensor([f"p{b}" for b in range(9)], pl.DiffusionGenerationParams(H, W, 2, 3.5), **kw)


def test_request_installs_the_weights_around_the_chunks_with_and_without_regions():
    pipe = Recording()
    assert tuple(_request(pipe, key_weights=dict(prompt=np.full(512, 2.0))).shape) == (9, 3, H, W)
    assert [c if isinstance(c, str) else c[0] if c[0] == "weights" else len(c[0].prompts) for c in pipe.calls] == ["weights", 8, 1, "unweighted"]
    assert pipe.calls[0][1].tolist() == [2.0] * 512 and pipe.calls[0][2].tolist() == [1.0] * 6
    assert tuple(pipe.calls[1][0].embeddings[0].shape) == (8, 512, J)  # the prompts were encoded once, in front of the chunks: one T for the request
    pipe = Recording()
    _request(pipe, regions=[("a", np.ones((H, W)))], key_weights=dict(prompt=np.full(512, 2.0), image=np.full((2, 3), 3.0)))
    assert [c if isinstance(c, str) else c[0] for c in pipe.calls[:2] + pipe.calls[-2:]] == ["set", "weights", "unweighted", "clear"]
    assert pipe.calls[1][1].tolist() == [2.0] * 512 + [1.0] * 512 and pipe.calls[1][2].tolist() == [3.0] * 6
    quiet = Recording()
    assert _request(quiet).shape[0] == 9 and [len(c[0].prompts) for c in quiet.calls] == [8, 1] and quiet.calls[0][0].embeddings is None  # no key_weights=: the calls it always made


def test_weights_are_cleared_after_a_chunk_raises_and_refusals_install_nothing():
    pipe = Recording(fail=True)
    with pytest.raises(RuntimeError, match="chunk failed"):
        _request(pipe, key_weights=OK | dict(prompt=np.ones(512)))
    assert pipe.calls[0][0] == "weights" and pipe.calls[-1] == "unweighted"
    for kw, match in [(dict(negative_prompt="n", true_cfg_scale=2.0), "not combined with true CFG"), (dict(reference=np.zeros((16, 16, 3), np.uint8)), "reference="),
                      (dict(key_weights=dict(prompt=np.ones(7))), r"must be \(512,\)")]:
        quiet = Recording()
        with pytest.raises(ValueError, match=match):
            _request(quiet, **dict(dict(key_weights=OK | dict(prompt=np.ones(512))), **kw))
        assert quiet.calls == []


def test_new_symbols_are_exported_and_declared_and_null_weights_are_the_unweighted_call():
    header = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    for name in ("fmi_sdpa_groups_weighted_bf16", "fmi_flux_set_attention_key_weights"):
        assert name in _lib.EXPORTED and re.search(r"^int " + name + r"\(", header, re.M)
    assert "k_weights == NULL is exactly fmi_sdpa_groups_bf16" in header
