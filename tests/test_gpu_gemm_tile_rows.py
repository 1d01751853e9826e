"""Tile heights of the bf16 ping-pong GEMM: a launch cut into 192-row tiles, or into 256-row and 192-row tiles, writes the bytes the
all-256 launch writes.  A 192-row tile splits rows, never K, so the check is a byte comparison of the whole output buffers (guard rows and columns
included), no tolerance.  Through the op-level entry and the case builders of tests/test_gpu_gemm_epilogues.py; the height is set with
fmi_set_gemm_rows: 0 automatic, 256, 192, 448 = 256-row tiles while at least 448 rows remain and 192-row tiles for the rest (the setting that gives a
mixed launch at sizes where the automatic choice is all-256: M = 448 -> 1 + 1, 640 -> 1 + 2, 192 and 100 -> 0 + 1).

The fused q|k|v relayout epilogue has no op-level descriptor (fmi_gemm_desc carries none of its fields), so it is compared through the model that
issues it: SMALL_FLUX has 2 heads (N = 768); 384 and 448 image rows with 64 text rows give the joint-order offset 64 and a padded V^T stride; a
FLUX.1-dev-wide model of one double and one single block runs the grouped 4096 + 512 x 9216 x 3072 launch under the automatic cut."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gemm_reference as G
from tests import test_gpu_gemm_epilogues as E

pytestmark = pytest.mark.gpu

AUTO, TALL, SHORT, MIXED = 0, 256, 192, 448
S = G.spec


@pytest.fixture(scope="module")
def env():
    import torch
    from diffusion_rs_amd import _lib as L
    lib = L.load()
    L.check(lib.fmi_init(0))
    yield dict(torch=torch, L=L, lib=lib, cus=torch.cuda.get_device_properties(0).multi_processor_count)
    lib.fmi_set_gemm_rows(AUTO)


def split_of(env, specs, mode):
    n = len(specs)
    arr = lambda v: (C.c_int * len(v))(*v)  # noqa: E731
    a, b, ts, ss, q = arr([0] * n), arr([0] * n), arr([0] * (n + 1)), arr([0] * (n + 1)), C.c_int(0)
    env["L"].check(env["lib"].fmi_gemm_tile_rows(arr([s["M"] for s in specs]), arr([s["N"] for s in specs]), n, env["cus"], 0, mode, a, b, ts, ss, C.byref(q)),
                   env["lib"])
    return list(a), list(b)


def run_modes(env, specs, modes):
    """One grouped launch per mode from the same initial buffers; returns {mode: [raw output tensor per problem]}."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    built = [E.build(torch, L, s, G.make(s)) for s in specs]
    descs = [d for d, _ in built]
    out = {}
    try:
        for mode in modes:
            L.check(lib.fmi_set_gemm_rows(mode), lib)
            for _, keep in built:
                keep["out"].copy_(keep["init"])
            torch.cuda.synchronize()
            L.check(E.launch(lib, L, descs), lib)
            torch.cuda.synchronize()
            out[mode] = [keep["out"].view(torch.int32 if keep["f32_out"] else torch.int16).clone() for _, keep in built]
    finally:
        lib.fmi_set_gemm_rows(AUTO)
    out["init"] = [keep["init"].view(torch.int32 if keep["f32_out"] else torch.int16) for _, keep in built]
    return out


SB, GE, GFC, RG = G.STORE_BF16, G.GELU_BF16, G.GELU_FROM_COL, G.RESID_GATE_F32
SMALL = {
    # row splits (N = 512: two tile columns, one band; K = 128: two K tiles)
    "m192_one_short": ([S(192, 512, 128, SB)], (AUTO, SHORT, MIXED)),
    "m448_tall_short": ([S(448, 512, 128, SB)], (AUTO, SHORT, MIXED)),
    "m640_tall_two_short": ([S(640, 512, 128, SB)], (AUTO, SHORT, MIXED)),
    "m400_two_short_and_16_rows": ([S(400, 512, 128, SB)], (SHORT, MIXED)),
    "m100_one_clamped": ([S(100, 512, 128, SB)], (AUTO, SHORT, MIXED)),
    # three K tiles: the W ring wraps, the A ring is read a second time; one K tile: the prologue alone
    "m448_k192": ([S(448, 512, 192, SB)], (SHORT, MIXED)),
    "m448_k64": ([S(448, 512, 64, SB)], (SHORT, MIXED)),
    "m448_k320": ([S(448, 512, 320, RG)], (SHORT, MIXED)),
    # epilogues
    "m448_bias_gelu": ([S(448, 512, 128, GE)], (SHORT, MIXED)),
    "m448_gelu_from_256": ([S(448, 512, 128, GFC, gelu_from=256)], (SHORT, MIXED)),
    "m448_gate_resid_batches_of_224": ([S(448, 512, 128, RG, rpb=224)], (SHORT, MIXED)),
    "m448_gate_resid_batches_of_100": ([S(448, 512, 128, RG, rpb=100)], (SHORT, MIXED)),
    "m448_store_f32": ([S(448, 512, 128, G.STORE_F32, alpha=0.125)], (SHORT, MIXED)),
    "m448_direct_path_n260": ([S(448, 260, 128, RG, rpb=100)], (SHORT, MIXED)),
    # grouped: 1 + 1 and 0 + 1 under MIXED
    "group_448_192": ([S(448, 512, 128, SB), S(192, 512, 128, SB, seed=1)], (SHORT, MIXED)),
    "group_13_tall_tiles": ([S(640, 768, 64, SB), S(300, 512, 64, RG, seed=1)], (SHORT, MIXED)),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_same_bytes_as_the_256_row_launch(env, name):
    specs, modes = SMALL[name]
    out = run_modes(env, specs, (TALL,) + modes)
    torch = env["torch"]
    for i in range(len(specs)):  # the 256-row launch wrote its result over the NaN / residual image the buffers start from
        assert not torch.equal(out[TALL][i], out["init"][i]), (name, i)
    for mode in modes:
        for i in range(len(specs)):
            assert torch.equal(out[mode][i], out[TALL][i]), (name, "rows mode", mode, "problem", i, split_of(env, specs, mode))


def test_the_forced_settings_cut_as_the_cases_assume(env):
    assert split_of(env, SMALL["m448_tall_short"][0], MIXED) == ([1], [1])
    assert split_of(env, SMALL["m640_tall_two_short"][0], MIXED) == ([1], [2])
    assert split_of(env, SMALL["m400_two_short_and_16_rows"][0], SHORT) == ([0], [3])
    assert split_of(env, SMALL["group_448_192"][0], MIXED) == ([1, 0], [1, 1])


FULL = {
    "mlp_in_gelu_4608x12288x3072": [S(4608, 12288, 3072, GE)],
    "qkv_shape_4096+512x9216x3072": [S(4096, 9216, 3072, SB), S(512, 9216, 3072, SB, seed=1)],
}


@pytest.mark.parametrize("name", list(FULL))
def test_full_depth_automatic_split_same_bytes(env, name):
    """The only shapes at which the automatic split, its tall-first order and the band regions of both heights run: single launches."""
    specs = FULL[name]
    if env["cus"] == 256:
        a, b = split_of(env, specs, AUTO)
        assert sum(b) > 0, (a, b)  # on the part this is written for the automatic choice does cut these shapes
    out = run_modes(env, specs, (TALL, AUTO, SHORT))
    for mode in (AUTO, SHORT):
        for i in range(len(specs)):
            assert env["torch"].equal(out[mode][i], out[TALL][i]), (name, mode, i, split_of(env, specs, mode))


def test_full_depth_fused_qkv_relayout_automatic_split_same_bytes(env):
    """The double blocks' grouped q|k|v launch at the headline shape — 4096 image + 512 text rows x 9216 x 3072, 24 heads, fused relayout epilogue — under
    the automatic cut (12 + 6 | 2 + 0 on 256 CUs: the last short image tile clamped to 64 rows, image rows at joint offset 512) against all-256, through a
    FLUX.1-dev-wide model of one double and one single block (the same model also runs MLP-in and linear1 at their headline shapes)."""
    import diffusion_rs_amd as d
    from tests import test_gpu_production_shapes as PS
    from tests.util import dev, flux_inputs, host
    torch, L, lib = env["torch"], env["L"], env["lib"]
    if env["cus"] == 256:
        a, b = split_of(env, FULL["qkv_shape_4096+512x9216x3072"], AUTO)
        assert sum(b) > 0 and b[0] > 0, (a, b)
    cfg = dict(d.FLUX_DEV, num_layers=1, num_single_layers=1)
    gm = d.FluxModel(cfg)
    try:
        for name, shape in d.synth.flux_tensor_shapes(cfg).items():
            gm.set_tensor(name, PS._seeded_weight(torch, name, shape, d))
        gm.assert_complete()
        img, ids, txt, txt_ids, y = flux_inputs(cfg, 1, (64, 64), 512, seed=29)
        args = (dev(img), dev(ids), dev(txt, torch.bfloat16), dev(txt_ids), dev(np.full(1, 0.7, np.float32)), dev(y), dev(np.full(1, 3.5, np.float32)))
        got = {}
        try:
            for mode in (TALL, AUTO, SHORT):
                L.check(lib.fmi_set_gemm_rows(mode), lib)
                got[mode] = host(gm.forward(*args))
        finally:
            lib.fmi_set_gemm_rows(AUTO)
    finally:
        gm.close()
    assert np.isfinite(got[TALL]).all() and np.abs(got[TALL]).max() > 0
    for mode in (AUTO, SHORT):
        assert got[mode].dtype == got[TALL].dtype and got[mode].tobytes() == got[TALL].tobytes(), mode


@pytest.mark.parametrize("S_hw", [(16, 24), (16, 28)])
def test_fused_qkv_relayout_same_bytes_through_the_model(env, S_hw):
    """q|k|v projections with the fused RMS-norm / RoPE / transposed-V epilogue: 384 (two short tiles) or 448 (1 + 1) image rows, 64 text rows."""
    import diffusion_rs_amd as d
    from tests.util import SMALL_FLUX, dev, flux_inputs, host
    torch, L, lib = env["torch"], env["L"], env["lib"]
    gm = d.FluxModel(SMALL_FLUX)
    gm.load_state_dict(d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0))
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, 1, S_hw, 64, seed=23)
    args = (dev(img), dev(ids), dev(txt, torch.bfloat16), dev(txt_ids), dev(np.full(1, 0.7, np.float32)), dev(y), dev(np.full(1, 3.5, np.float32)))
    got = {}
    try:
        for mode in (TALL, SHORT, MIXED):
            L.check(lib.fmi_set_gemm_rows(mode), lib)
            got[mode] = host(gm.forward(*args))
    finally:
        lib.fmi_set_gemm_rows(AUTO)
    assert np.isfinite(got[TALL]).all() and np.abs(got[TALL]).max() > 0
    for mode in (SHORT, MIXED):
        assert got[mode].dtype == got[TALL].dtype and got[mode].tobytes() == got[TALL].tobytes(), mode
