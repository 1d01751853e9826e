"""Block-sparse attention on the host: the local-window lists against a token-level loop, the new symbols, and the request path in front of
the chunk body, without a GPU."""
import os
import re

import numpy as np
import pytest

from diffusion_rs_amd import _lib, flux as F, pipeline as pl
from tests.test_host_regions import H, W, RecordingPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("T,h,w,r", [(64, 8, 16, 1), (40, 12, 20, 2), (512, 6, 6, 9)])
def test_local_attention_tiles_against_the_token_level_loop(T, h, w, r):
    n = T + h * w
    sees = np.ones((n, n), bool)  # a text token sees everything, and everything sees the text
    for i in range(h * w):
        for j in range(h * w):
            sees[T + i, T + j] = max(abs(i // w - j // w), abs(i % w - j % w)) <= r
    nqb, nt = -(-n // 128), -(-n // 64)
    row_ptr, cols = F.local_attention_tiles(T, h, w, r)
    assert row_ptr.dtype == cols.dtype == np.int32 and row_ptr.shape == (nqb + 1,) and row_ptr[0] == 0 and row_ptr[-1] == cols.size
    for b in range(nqb):
        want = [t for t in range(nt) if sees[128 * b:128 * b + 128, 64 * t:64 * t + 64].any()]
        assert cols[row_ptr[b]:row_ptr[b + 1]].tolist() == want  # listed <=> some pair visible, ascending
        assert 128 * b >= T or want == list(range(nt))           # a block with a text token lists every tile
    if r >= max(h, w):
        assert cols.tolist() == list(range(nt)) * nqb
    assert F.attention_blocks_order(row_ptr).tolist() == sorted(range(nqb), key=lambda b: (row_ptr[b] - row_ptr[b + 1], b))


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    lib = _lib.load()
    for name in ("fmi_sdpa_blocks_bf16", "fmi_flux_set_attention_blocks"):
        assert name in _lib.EXPORTED and re.search(r"^int " + name + r"\(", header, re.M) and getattr(lib, name).argtypes


class Recording(RecordingPipeline):
    def __init__(self, fail=False):
        super().__init__(fail)
        self.flux.set_attention_blocks = lambda rp, cl: self.calls.append(("blocks", rp, cl))
        self.flux.clear_attention_blocks = lambda: self.calls.append("unblocked")


def _request(pipe, **kw):
    return pipe.generate_tensor([f"p{b}" for b in range(9)], pl.DiffusionGenerationParams(H, W, 2, 3.5), **kw)


def test_request_installs_the_lists_around_the_chunks_and_refuses_by_name():
    pipe = Recording()
    assert tuple(_request(pipe, attention_window=1).shape) == (9, 3, H, W)
    assert [c if isinstance(c, str) else c[0] if c[0] == "blocks" else len(c[0].prompts) for c in pipe.calls] == ["blocks", 8, 1, "unblocked"]
    want = F.local_attention_tiles(512, H // 16, W // 16, 1)  # the placeholder prompts' 512 text rows
    assert all(np.array_equal(a, b) for a, b in zip(pipe.calls[0][1:], want))
    quiet = Recording()
    assert _request(quiet).shape[0] == 9 and [len(c[0].prompts) for c in quiet.calls] == [8, 1] and quiet.calls[0][0].embeddings is None  # no attention_window=: the calls it always made
    pipe = Recording(fail=True)
    with pytest.raises(RuntimeError, match="chunk failed"):
        _request(pipe, attention_window=0)
    assert pipe.calls[0][0] == "blocks" and pipe.calls[-1] == "unblocked"
    for kw, match in [(dict(regions=[("a", np.ones((H, W)))]), "not combined with regions="), (dict(key_weights=dict(prompt=np.ones(512))), "not combined with key_weights="),
                      (dict(negative_prompt="n", true_cfg_scale=2.0), "not combined with true CFG"), (dict(attention_window=-1), "integer >= 0"),
                      (dict(attention_window=1.5), "integer >= 0")]:
        quiet = Recording()
        with pytest.raises(ValueError, match=match):
            _request(quiet, **dict(dict(attention_window=1), **kw))
        assert quiet.calls == []
