"""Regional prompts on the host: the group words, the request's refusals and the request path in front of the chunk body, without a GPU."""
import threading

import numpy as np
import pytest
import torch

from diffusion_rs_amd import pipeline as pl

H, W, J, P = 32, 48, 8, 4  # a 2 x 3 token image


def test_region_groups_word_for_word():
    left, corner = np.zeros((H, W)), np.zeros((H, W))
    left[:, :16] = 1         # the left column of tokens
    corner[16:, 32:] = 1     # the bottom right token ...
    corner[:16, 16:24] = 1   # ... and exactly half of the top middle one: a mean of 0.5 counts
    corner[:7, 32:] = 1      # less than half of the top right one does not
    txt, img = pl.region_groups([left, torch.from_numpy(corner)], 2, H, W)
    assert txt.dtype == img.dtype == np.uint32
    assert txt.tolist() == [1, 1, 2, 2, 4, 4] and img.tolist() == [1 | 2, 1 | 4, 1, 1 | 2, 1, 1 | 4]
    assert pl.region_groups([np.ones((16, 16))] * 31, 1, 16, 16)[1].tolist() == [0xFFFFFFFF]


@pytest.mark.parametrize("kw,match", [(dict(n_regions=0), "1 .. 31"), (dict(n_regions=32), "1 .. 31"), (dict(height=40), "multiples of 16"),
                                      (dict(mask_shapes=[(H, W), (H, W + 1)]), "mask of region 2"), (dict(present=["reference="]), "not combined with reference="),
                                      (dict(text_rows=pl.REGIONS_MAX_TEXT_ROWS + 1), "text rows")])
def test_check_regions_request_refuses_by_name(kw, match):
    ok = dict(n_regions=2, mask_shapes=[(H, W)] * 2, height=H, width=W)
    assert pl.check_regions_request(**ok, text_rows=pl.REGIONS_MAX_TEXT_ROWS) is None
    with pytest.raises(ValueError, match=match):
        pl.check_regions_request(**dict(ok, **kw))


class _Flux:
    cfg = dict(joint_attention_dim=J, pooled_projection_dim=P)
    cond_channels, groups, log = 0, None, None

    def is_guidance(self):
        return True

    def set_attention_groups(self, txt, img):
        self.groups = (txt, img)
        self.log.append("set")

    def clear_attention_groups(self):
        self.groups = None
        self.log.append("clear")


class RecordingPipeline(pl.Pipeline):
    def __init__(self, fail=False):  # no GPU: placeholder embeddings, and only the request path in front of the chunk body is under test
        self.device, self.flux, self.t5, self.clip, self.source_kind = torch.device("cpu"), _Flux(), None, None, "synthetic"
        self._lock, self.calls, self.fail = threading.Lock(), [], fail
        self.flux.log = self.calls

    def _generate_chunk(self, s, params, seed, strength, return_latents, cache_threshold, stats):  # the pinned signature, no shared option
        self.calls.append((s, self.flux.groups))
        if self.fail:
            raise RuntimeError("chunk failed")
        return torch.zeros((len(s.prompts), 3, H, W), dtype=torch.uint8)


def _request(pipe, **kw):
    masks = [np.ones((H, W)), np.zeros((H, W))]
    return pipe.generate_tensor([f"p{b}" for b in range(9)], pl.DiffusionGenerationParams(H, W, 2, 3.5), regions=[("a", masks[0]), ("b", masks[1])], **kw)


def test_request_concatenates_the_text_rows_and_installs_the_words_around_the_chunks():
    pipe = RecordingPipeline()
    assert tuple(_request(pipe).shape) == (9, 3, H, W)
    assert [c if isinstance(c, str) else len(c[0].prompts) for c in pipe.calls] == ["set", 8, 1, "clear"] and pipe.flux.groups is None
    base, _ = pl.placeholder_embeddings(["p0", "p8"], 512, J, P, pipe.device)
    reg, _ = pl.placeholder_embeddings(["a", "b"], 512, J, P, pipe.device)
    (s0, words), (s1, _) = pipe.calls[1:3]
    assert s0.token_ids is None and tuple(s0.embeddings[0].shape) == (8, 3 * 512, J) and tuple(s0.embeddings[1].shape) == (8, P)
    assert torch.equal(s0.embeddings[0][0], torch.cat([base[0], reg[0], reg[1]])) and torch.equal(s1.embeddings[0][0], torch.cat([base[1], reg[0], reg[1]]))
    want = pl.region_groups([np.ones((H, W)), np.zeros((H, W))], 512, H, W)
    assert all(np.array_equal(a, b) for a, b in zip(words, want))


def test_words_are_cleared_after_a_chunk_raises_and_refusals_install_nothing():
    pipe = RecordingPipeline(fail=True)
    with pytest.raises(RuntimeError, match="chunk failed"):
        _request(pipe)
    assert pipe.calls[0] == "set" and pipe.calls[-1] == "clear" and pipe.flux.groups is None
    for kw, match in [(dict(negative_prompt="n"), "negative_prompt="), (dict(cache_threshold=0.1), "cache_threshold="), (dict(token_ids=(None, None)), "token_ids="),
                      (dict(reference=np.zeros((16, 16, 3), np.uint8)), "reference=")]:
        quiet = RecordingPipeline()
        with pytest.raises(ValueError, match="not combined with " + match):
            _request(quiet, **kw)
        assert quiet.calls == []
