"""The denoise loop's step updates are one family: the Euler step IS the Heun predictor's state, and the Heun corrector with equal slopes IS the
Euler step — bit for bit, with and without the blend, on the 16-byte path and on the scalar path.  Only op-level entries: cfg_euler_step, heun_predict,
heun_correct.

Every update is element-wise, so the only structure that can go wrong is the choice between the 16-byte and the scalar path and the tail: n = 4096 on a 16-byte
base (wide), n = 4099 (n % 4 != 0: scalar) and n = 4096 starting one float past a 16-byte boundary (scalar), 16 blocks of 256 threads each way."""
import functools

import numpy as np
import pytest

from tests.util import dev, host

pytestmark = pytest.mark.gpu

SIZES = {"aligned": 4096, "odd": 4099, "offset": 4096}
SCALE, DT, S = 3.5, -0.2, 0.55
eq = np.testing.assert_array_equal


def _offset(torch, a):
    """a copy of `a` on the device that starts one float past a 16-byte boundary: the scalar path (as in test_gpu_true_cfg.py)"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(7)
    n = max(SIZES.values())
    img, pos, neg, x0, noise = (rng.standard_normal(n).astype(np.float32) for _ in range(5))
    return dict(img=img, pos=pos, neg=neg, x0=x0, noise=noise, mask=rng.random(n).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _results(size, masked):
    """every update this file compares, once per (size, masked): "aligned" and "offset" run the same values (the first 4096 of "odd"'s)"""
    import torch
    import diffusion_rs_amd as d
    n = SIZES[size]

    def put(name):  # (a fresh device copy each time: two of the updates are in place)
        a = _inputs()[name][:n]
        t = _offset(torch, a) if size == "offset" else dev(a)
        assert t.data_ptr() % 16 == (4 if size == "offset" else 0)
        return t

    def blend():
        return dict(x0=put("x0"), noise=put("noise"), mask=put("mask"), s=S) if masked else {}

    pos, neg = put("pos"), put("neg")
    r = {}
    r["euler"] = host(d.cfg_euler_step(put("img"), pos, neg, SCALE, DT, **blend()))
    xt, g1 = d.heun_predict(put("img"), pos, neg, SCALE, DT, **blend())
    r["xt"], r["g1"] = host(xt), host(g1)
    r["g1_again"] = host(d.heun_predict(put("img"), pos, neg, SCALE, DT, **blend())[1])
    r["corrected"] = host(d.heun_correct(put("img"), g1, pos, neg, SCALE, DT, **blend()))
    r["euler_pos_is_neg"] = host(d.cfg_euler_step(put("img"), pos, put("pos"), SCALE, DT, **blend()))
    r["xt_unguided"] = host(d.heun_predict(put("img"), pos, None, SCALE, DT, **blend())[0])
    assert all(np.isfinite(v).all() and v.shape == (n,) for v in r.values())
    return r


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("size", list(SIZES))
def test_euler_step_is_the_heun_predictors_state(size, masked):
    r = _results(size, masked)
    eq(r["euler"], r["xt"], err_msg="cfg_euler_step vs heun_predict's x_pred")
    eq(r["g1"], r["g1_again"], err_msg="g1 of a second identical heun_predict")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("size", list(SIZES))
def test_heun_corrector_with_equal_slopes_is_the_euler_step(size, masked):
    r = _results(size, masked)  # g1 == g2: (g + g) * 0.5 is exact
    eq(r["corrected"], r["euler"], err_msg="heun_correct with g2 == g1 vs cfg_euler_step")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("size", list(SIZES))
def test_unguided_predictor_is_the_euler_step_with_the_negative_equal_to_the_prompt(size, masked):
    r = _results(size, masked)  # pos == neg gives neg bit for bit
    eq(r["xt_unguided"], r["euler_pos_is_neg"], err_msg="heun_predict(neg=None)'s x_pred vs cfg_euler_step(pos, pos)")


@pytest.mark.parametrize("masked", [False, True])
def test_sixteen_byte_path_equals_the_scalar_path(masked):
    wide, scalar = _results("aligned", masked), _results("offset", masked)
    for k in wide:
        eq(wide[k], scalar[k], err_msg=f"{k}: 16-byte path vs scalar path")
