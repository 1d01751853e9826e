"""Joint attention with per-key weights at d = 128.  The op is held to 1.5 x the rel-L2 that fmi_sdpa_bf16 shows against float64 on the same
q, k, v, unweighted (tests/test_gpu_attention_groups.py's rule, and its operands); what the summary flag and the score grid promise is checked as bits; the model
to tests/test_gpu_flux.py's 1e-2 against the oracle's forward restated with the weighted float64 attention."""
import numpy as np
import pytest

from tests import attention_groups_ref as G, attention_weights_ref as R
from tests.test_gpu_attention_groups import B, GRID, SCALE, T0, _problem, _region_words, model  # noqa: F401  (the operands, their float64 error, the model fixture)
from tests.util import SMALL_FLUX, dev, flux_inputs, rel_l2, host

pytestmark = pytest.mark.gpu
SHAPES = [(64, 64), (100, 100), (192, 130), (257, 321)]  # one tile; a ragged tail; Lq != Lk; several tiles and a ragged last one


def _bits(t):
    import torch
    return host(t.view(torch.int16))


@pytest.mark.parametrize("weights", ["ones-but-one-tile", "random"])
@pytest.mark.parametrize("pattern", ["all", "block24"])
@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_op_against_float64(Lq, Lk, pattern, weights):
    import diffusion_rs_amd as d
    q, k, v, f, base = _problem(Lq, Lk)
    for Bg in (1, B):
        qg, kg = (g[:Bg] for g in G.words(pattern, Lq, Lk, B))
        kw = R.weights(weights, Lk, Bg)
        got = host(d.ops.sdpa_groups(q, k, v, qg.astype(np.int64), kg.astype(np.int64), k_weights=kw).float())
        err = rel_l2(got, R.weighted_attention(*f, qg, kg, kw, SCALE))
        print(f"sdpa_groups weighted Lq={Lq} Lk={Lk} {pattern} {weights} Bg={Bg}: rel-L2 {err:.3e} (fmi_sdpa_bf16 unweighted {base:.3e}, bound {1.5 * base:.3e})")
        assert np.isfinite(got).all() and err <= 1.5 * base


@pytest.mark.parametrize("pattern", ["all", "block24"])
@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_ones_are_the_unweighted_call_and_a_power_of_two_moves_no_bit(Lq, Lk, pattern):
    """Weights of 1 flag every tile, which then takes the unweighted path: the bits of sdpa_groups without weights.  Four times every weight moves every score
    and the maximum by exactly 2: a term added behind the maximum, or left out of the row sum, would show."""
    import diffusion_rs_amd as d
    q, k, v, _, _ = _problem(Lq, Lk)
    qg, kg = (g.astype(np.int64) for g in G.words(pattern, Lq, Lk, B))
    run = lambda kw: _bits(d.ops.sdpa_groups(q, k, v, qg, kg, k_weights=kw, out_token_major=True))
    np.testing.assert_array_equal(run(np.ones((B, Lk), np.float32)), run(None))
    kw = R.weights("random", Lk, B)
    np.testing.assert_array_equal(run(4 * kw), run(kw))
    assert (run(kw) != run(None)).any()


def test_model_against_the_weighted_restatement_and_the_two_setters_are_independent(model):
    gm, run, args = model["gm"], model["run"], model["args"]
    rng = np.random.default_rng(5)
    txt_w, img_w = (2.0 ** rng.uniform(-2, 2, (B, 3 * T0))).astype(np.float32), (2.0 ** rng.uniform(-2, 2, (B, GRID[0] * GRID[1]))).astype(np.float32)
    txt_w[:, :T0] = 1  # a text stretch without a term
    want = R.flux_forward(model["sd"], SMALL_FLUX, *args, weights=np.concatenate([txt_w, img_w], 1))
    try:
        gm.set_attention_key_weights(txt_w, img_w)
        got = run()  # no group words: the all-ones word is implied
        gm.set_attention_groups(*_region_words())
        both = run()
        gm.clear_attention_groups()  # leaves the weights
        np.testing.assert_array_equal(run(), got)
    finally:
        gm.clear_attention_key_weights()
    err = rel_l2(got, want)
    print(f"forward with key weights: rel-L2 {err:.3e} against the weighted restatement ({rel_l2(got, model['oracle']):.3e} against the unweighted oracle)")
    assert np.isfinite(got).all() and err <= 1e-2
    assert np.abs(both - got).max() > 0
    np.testing.assert_array_equal(run(), model["plain"])


def test_refusals_install_nothing(model):
    import torch
    d, gm, run = model["d"], model["gm"], model["run"]
    from diffusion_rs_amd import _lib as L
    from tests import controlnet_ref as CR

    def refused(code, call):
        with pytest.raises(d.FmiError) as e:
            call()
        assert e.value.code == code, e.value
    txt_w, img_w = np.full(3 * T0, 2.0, np.float32), np.full(GRID[0] * GRID[1], 0.5, np.float32)
    for bad in (0.0, np.nan, -1.0, np.inf):
        refused(L.ERR_INVALID, lambda: gm.set_attention_key_weights(np.where(np.arange(3 * T0) == 5, bad, txt_w).astype(np.float32), img_w))
    q8 = d.FluxModel(SMALL_FLUX)
    q8.load_state_dict(model["sd"])
    q8.quantize_int8()
    cn = d.FluxControlNetModel(CR.net_cfg("2+0"))
    for handle in (q8, cn):
        refused(L.ERR_UNSUPPORTED, lambda: handle.set_attention_key_weights(txt_w, img_w))
        handle.close()
    np.testing.assert_array_equal(run(), model["plain"])  # nothing of the above installed anything
    img, ids, txt, txt_ids, y = (dev(a) for a in flux_inputs(SMALL_FLUX, B, GRID, 3 * T0))
    try:
        gm.set_attention_key_weights(txt_w, img_w)
        refused(L.ERR_UNSUPPORTED, lambda: gm.denoise(img, ids, txt.to(torch.bfloat16), txt_ids, y, dev(np.full(B, 3.5, np.float32)), [1.0, 0.5, 0.0],
                                                      negative_txt=txt.to(torch.bfloat16), negative_y=y, true_cfg_scale=2.0))
    finally:
        gm.clear_attention_key_weights()
