"""Joint attention with token group masks at d = 128.  The op is held to 1.5 x the rel-L2 that fmi_sdpa_bf16 shows against float64 on the same
q, k, v unmasked, computed here (tests/test_gpu_sdpa_d64.py's margin for a new kernel); the model to tests/test_gpu_flux.py's 1e-2 against a masked restatement
of the oracle's forward (attention_groups_ref.flux_forward); what the mask promises through every block is checked as values (==)."""
import functools

import numpy as np
import pytest

from tests import attention_groups_ref as R
from tests.util import SMALL_FLUX, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu
B, H, SCALE = 2, 2, 128 ** -0.5


@functools.lru_cache(maxsize=None)
def _problem(Lq, Lk):
    """q, k, v on the device, and the rel-L2 of fmi_sdpa_bf16 against float64 on them, unmasked: computed once per shape, never changed."""
    import torch
    from diffusion_rs_amd import _lib as L
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    q, k, v = (torch.randn((B, H, n, 128), generator=g).to(torch.bfloat16).cuda() for n in (Lq, Lk, Lk))
    o = torch.empty_like(q)
    L.check(L.load().fmi_sdpa_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Lq, Lk, 128, SCALE, 0, None))
    f = [host(t.float()) for t in (q, k, v)]
    base = rel_l2(host(o.float()), R.masked_attention(*f, np.ones((1, Lq), np.uint32), np.ones((1, Lk), np.uint32), SCALE))
    return q, k, v, f, base


@pytest.mark.parametrize("pattern", ["all", "block64", "block24", "random"])
@pytest.mark.parametrize("Lq,Lk", [(64, 64), (100, 100), (192, 130), (257, 321)])
def test_op_against_float64(Lq, Lk, pattern):
    import diffusion_rs_amd as d
    q, k, v, f, base = _problem(Lq, Lk)
    qg, kg = R.words(pattern, Lq, Lk, B)
    want = R.masked_attention(*f, qg, kg, SCALE)
    for token_major in (False, True):
        got = host(d.ops.sdpa_groups(q, k, v, qg.astype(np.int64), kg.astype(np.int64), out_token_major=token_major).float())
        got = got.reshape(B, Lq, H, 128).transpose(0, 2, 1, 3) if token_major else got
        err = rel_l2(got, want)
        print(f"sdpa_groups Lq={Lq} Lk={Lk} {pattern} token_major={token_major}: rel-L2 {err:.3e} (fmi_sdpa_bf16 unmasked {base:.3e}, bound {1.5 * base:.3e})")
        assert np.isfinite(got).all() and err <= 1.5 * base


def test_masked_keys_contribute_exactly_nothing():
    """Keys no query sees — twenty inside a tile that is visited, and two whole tiles that are never fetched — hold 1e4 in k and v: not one output bit moves.
    One word set for both samples (the broadcast form)."""
    import torch
    import diffusion_rs_amd as d
    q, k, v, _, _ = _problem(192, 321)
    qg = (1 << (np.arange(192) // 64)).astype(np.int64)
    kg = (1 << (np.arange(321) // 64)).astype(np.int64)
    kg[192:] = 1 << 20
    kg[70:90] = 1 << 21
    hidden = (qg[:, None] & kg[None, :]).max(0) == 0
    assert hidden.sum() == 20 + 129
    want = d.ops.sdpa_groups(q, k, v, qg, kg)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, dev(hidden)] = 1e4
    v2[:, :, dev(hidden)] = 1e4
    got = d.ops.sdpa_groups(q, k2, v2, qg, kg)
    assert np.isfinite(host(got.float())).all()
    np.testing.assert_array_equal(host(got.view(torch.int16)), host(want.view(torch.int16)))


T0, GRID = 16, (6, 4)  # text rows per prompt; the image grid: S = 24, with three prompts L = 72 (two key tiles)


@pytest.fixture(scope="module")
def model():
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    sd = d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    gm = d.FluxModel(SMALL_FLUX)
    gm.load_state_dict(sd)
    om = orc.Flux(SMALL_FLUX)
    om.load(sd)
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, GRID, 3 * T0)
    t, g = np.linspace(0.9, 0.4, B).astype(np.float32), np.full(B, 3.5, np.float32)

    def run(txt_rows=txt):
        out = gm.forward(dev(img), dev(ids), dev(txt_rows, torch.bfloat16), dev(txt_ids), dev(t), dev(y), dev(g))
        torch.cuda.synchronize()
        return host(out)
    return dict(d=d, gm=gm, run=run, txt=txt, plain=run(), oracle=om.forward(img, ids, txt, txt_ids, t, y, g), sd=sd, args=(img, ids, txt, txt_ids, t, y, g))


def _region_words(right_half_region=True):
    """[base | region 1 | region 2] text rows; region 1 = the left two columns of the grid, region 2 = the right two (or no image token at all)."""
    txt = np.repeat(np.array([1, 2, 4], np.uint32), T0)
    col = np.tile(np.arange(GRID[1]), GRID[0])
    return txt, np.where(col < 2, 1 | 2, 1 | (4 if right_half_region else 0)).astype(np.uint32)


def test_model_against_the_masked_restatement_and_clearing_restores_the_plain_forward(model):
    """Two regions, laid out differently in the two samples (the words' sample stride), against attention_groups_ref.flux_forward — held first, unmasked, to the
    compiled oracle it restates.  Bar: tests/test_gpu_flux.py's for one evaluation."""
    gm, run, args = model["gm"], model["run"], model["args"]
    assert rel_l2(R.flux_forward(model["sd"], SMALL_FLUX, *args), model["oracle"]) <= 1e-5
    txt_w, img_w = _region_words()
    txt_w, img_w = np.stack([txt_w, txt_w]), np.stack([img_w, np.where(img_w == 3, 5, 3).astype(np.uint32)])
    want = R.flux_forward(model["sd"], SMALL_FLUX, *args, groups=np.concatenate([txt_w, img_w], 1))
    try:
        gm.set_attention_groups(txt_w, img_w)
        got = run()
    finally:
        gm.clear_attention_groups()
    err = rel_l2(got, want)
    print(f"forward with two regions: rel-L2 {err:.3e} against the masked restatement ({rel_l2(got, model['oracle']):.3e} against the unmasked oracle)")
    assert np.isfinite(got).all() and err <= 1e-2
    np.testing.assert_array_equal(run(), model["plain"])


def test_a_region_without_image_tokens_is_isolated_through_every_block(model):
    gm, run = model["gm"], model["run"]
    other = model["txt"].copy()
    other[:, 2 * T0:] += 1.0  # region 2's text rows
    assert np.abs(run(other) - model["plain"]).max() > 0  # without groups the image prediction follows them
    try:
        gm.set_attention_groups(*_region_words(right_half_region=False))
        np.testing.assert_array_equal(run(other), run())
    finally:
        gm.clear_attention_groups()


def test_refusals(model):
    import torch
    d, gm, run = model["d"], model["gm"], model["run"]
    from diffusion_rs_amd import _lib as L

    def refused(code, call):
        with pytest.raises(d.FmiError) as e:
            call()
        assert e.value.code == code, e.value
    txt_w, img_w = _region_words()
    zero = txt_w.copy()
    zero[3] = 0
    refused(L.ERR_INVALID, lambda: gm.set_attention_groups(zero, img_w))
    restore = [(gm.set_split_k, True, False), (gm.set_fp8_attention, 2, 1), (lambda w: gm.set_sequence_parallel(0, w, lambda *a: None), 2, 1)]
    for setter, on, off in restore:  # the setter's refusals, by mode
        setter(on)
        try:
            refused(L.ERR_UNSUPPORTED, lambda: gm.set_attention_groups(txt_w, img_w))
        finally:
            setter(off)
    q8 = d.FluxModel(SMALL_FLUX)
    q8.load_state_dict(model["sd"])
    q8.quantize_fp8()
    refused(L.ERR_UNSUPPORTED, lambda: q8.set_attention_groups(txt_w, img_w))
    q8.close()
    try:  # the evaluation's refusals while a set is installed
        gm.set_attention_groups(txt_w[:-1], img_w)
        refused(L.ERR_INVALID, run)  # another T
        gm.set_attention_groups(txt_w, img_w)
        for setter, on, off in restore[:2]:
            setter(on)
            try:
                refused(L.ERR_UNSUPPORTED, run)
            finally:
                setter(off)
        img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, GRID, 3 * T0)
        refused(L.ERR_UNSUPPORTED, lambda: gm.forward(dev(img), dev(ids), dev(txt, torch.bfloat16), dev(txt_ids), dev(np.ones(B, np.float32)), dev(y), dev(np.ones(B, np.float32)),
                                                      context=dev(img[:, :4]), context_ids=dev(ids[:, :4])))
    finally:
        gm.clear_attention_groups()
