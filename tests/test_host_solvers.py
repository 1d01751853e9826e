"""The second-order solvers, the parts that need no device: the reference loops of tests/solver_ref.py converge at their order on an analytic
field, the library's 2M scalars against a double-precision restatement, every wrong composition lies far enough from the correct one on the CPU oracle for the
GPU test's distances to mean something, the Python-side refusals, and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from diffusion_rs_amd import _lib as L
from diffusion_rs_amd import flux as F
from tests import solver_ref as SR
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


# ------------------------------------------------------------------------------------------------ 2. order of convergence
def _uniform(n, t_from=0.9, t_to=0.1):
    return [t_from + (t_to - t_from) * k / n for k in range(n + 1)]


@pytest.fixture(scope="module")
def field_errors():
    """|solve - RK4| at N = 16, 32, 64 on v(x, t) = cos(3t) x + 0.5 sin(2x) - 0.3, 64 Gaussian values, the uniform schedule 0.9 -> 0.1, in float64"""
    x = np.random.default_rng(0).standard_normal(64)
    exact = SR.rk4(x, 0.9, 0.1)
    return {s: [float(np.linalg.norm(SR.solve(SR.field_eval, x, _uniform(n), s, dtype=np.float64) - exact)) for n in (16, 32, 64)] for s in ("euler",) + SR.SOLVERS}


def test_order_of_convergence(field_errors):
    """halving the step divides the error by 2^p: below 2^1.5 for Euler (p = 1), above it for Heun and 2M (p = 2)"""
    bar = 2.0 ** 1.5
    for s, e in field_errors.items():
        ratios = [e[0] / e[1], e[1] / e[2]]
        print(f"{s}: errors {e[0]:.3e} {e[1]:.3e} {e[2]:.3e}, ratios {ratios[0]:.2f} / {ratios[1]:.2f}")
        for r in ratios:
            assert (r < bar) if s == "euler" else (r > bar), (s, ratios)


def test_heun_on_a_constant_field_is_euler_and_2m_without_w_is_euler_to_rounding():
    x = np.random.default_rng(1).standard_normal(64).astype(np.float32)
    const = np.random.default_rng(2).standard_normal(64).astype(np.float32)
    ts = SR.TS_CUT
    ev = lambda s, t, i: (const, None)
    np.testing.assert_array_equal(SR.solve(ev, x, ts, "heun"), SR.solve(ev, x, ts, "euler"))
    np.testing.assert_array_equal(SR.solve(ev, x, SR.TS4, "heun"), SR.solve(ev, x, SR.TS4, "euler"))
    # a * x + c * (x - t g) == x + g * dt in exact arithmetic: 4 steps of a handful of f32 roundings each
    fe = lambda s, t, i: (SR.field(s.astype(np.float64), t).astype(np.float32), None)
    for sched in (ts, SR.TS4):
        a, b = SR.solve(fe, x, sched, "dpmpp_2m", force_w0=True), SR.solve(fe, x, sched, "euler")
        assert np.abs(a.astype(np.float64) - b).max() <= 4 * 8 * 2.0 ** -24 * max(1.0, float(np.abs(b).max()))
        np.testing.assert_allclose(SR.solve(fe, x, sched, "dpmpp_2m", force_w0=True, dtype=np.float64), SR.solve(fe, x, sched, "euler", dtype=np.float64), rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------ 3. coefficients
def _ulps(a, b):
    a, b = f32(a), f32(b)
    return 0.0 if a == b else abs(float(a) - float(b)) / float(np.spacing(np.abs(b)))


def test_coefficients_against_the_double_restatement():
    rng = np.random.default_rng(3)
    schedules = [SR.TS4, SR.TS_CUT, [1.0, 0.5], [0.3, 0.0], [0.999, 0.998, 0.001, 0.0]]
    for n in (3, 8, 50):
        cut = np.sort(rng.random(n + 1))[::-1]
        schedules += [list(cut), [1.0] + list(cut[1:-1]) + [0.0]]
    worst = 0.0
    for ts in schedules:
        assert SR.check_schedule(ts)
        for i in range(len(ts) - 1):
            got, want = F.dpmpp_2m_coefficients(ts, i), SR.coefficients(ts, i)
            for g, w in zip(got, want):
                worst = max(worst, _ulps(g, w))
                assert _ulps(g, w) <= 2, (ts, i, got, want)
            if i == 0 or ts[i - 1] == 1.0 or ts[i + 1] == 0.0:  # the three first-order cases, exactly
                assert got[2] == 0.0 and want[2] == 0.0
            else:
                assert got[2] != 0.0
    print(f"fmi_dpmpp_2m_coefficients vs f64: worst {worst:.2f} ulp of f32")
    assert F.dpmpp_2m_coefficients([1.0, 0.8, 0.55, 0.3, 0.0], 1)[2] == 0.0  # after t = 1
    assert F.dpmpp_2m_coefficients([1.0, 0.8, 0.55, 0.3, 0.0], 2)[2] > 0.0
    assert F.dpmpp_2m_coefficients([1.0, 0.8, 0.55, 0.3, 0.0], 3) == (0.0, 1.0, 0.0)  # into t = 0: x = D


def test_coefficients_argument_checks():
    lib = L.load()
    a, c, w = C.c_float(), C.c_float(), C.c_float()
    out = (C.byref(a), C.byref(c), C.byref(w))
    ts = lambda *v: (C.c_double * len(v))(*v)
    assert lib.fmi_dpmpp_2m_coefficients(ts(0.9, 0.5, 0.1), 2, 1, *out) == 0
    assert lib.fmi_dpmpp_2m_coefficients(None, 2, 0, *out) == L.ERR_INVALID
    assert lib.fmi_dpmpp_2m_coefficients(ts(0.9, 0.5, 0.1), 2, 0, None, C.byref(c), C.byref(w)) == L.ERR_INVALID
    assert lib.fmi_dpmpp_2m_coefficients(ts(0.9, 0.5, 0.1), 2, 2, *out) == L.ERR_INVALID  # i == n_steps
    assert lib.fmi_dpmpp_2m_coefficients(ts(0.9, 0.5, 0.1), 2, -1, *out) == L.ERR_INVALID
    assert lib.fmi_dpmpp_2m_coefficients(ts(0.9, 0.5, 0.5), 2, 0, *out) == L.ERR_INVALID  # not strictly decreasing
    assert lib.fmi_dpmpp_2m_coefficients(ts(0.5, 0.9, 0.1), 2, 0, *out) == L.ERR_INVALID
    assert lib.fmi_dpmpp_2m_coefficients(ts(1.5, 0.5, 0.1), 2, 0, *out) == L.ERR_INVALID  # ts[0] > 1
    assert lib.fmi_dpmpp_2m_coefficients(ts(0.9, 0.5, -0.1), 2, 0, *out) == L.ERR_INVALID  # ts[n] < 0
    assert lib.fmi_dpmpp_2m_coefficients(ts(0.9, float("nan"), 0.1), 2, 0, *out) == L.ERR_INVALID
    assert b"schedule" in lib.fmi_last_error()


def test_check_solver_args():
    assert F.check_solver_args(None, [1.0, 2.0, 0.5]) is None and F.check_solver_args("euler", [1.0, 2.0]) is None  # the plain loop accepts what it accepted
    assert F.check_solver_args("heun", SR.TS4) == L.SOLVER_HEUN == 1 and F.check_solver_args("dpmpp_2m", SR.TS_CUT, cache=True) == L.SOLVER_DPMPP_2M == 2
    for bad in ("unipc", "Heun", 1, ""):
        with pytest.raises(ValueError, match="solver must be"):
            F.check_solver_args(bad, SR.TS4)
    for ts in ([1.0, 0.5, 0.5, 0.0], [0.5, 0.8, 0.0], [1.2, 0.5, 0.0], [0.9, 0.5, -0.1], [0.9, float("nan"), 0.1]):
        for s in SR.SOLVERS:
            with pytest.raises(ValueError, match="strictly decreasing"):
                F.check_solver_args(s, ts)
    with pytest.raises(ValueError, match="heun.*step cache"):
        F.check_solver_args("heun", SR.TS4, cache=True)
    for s in SR.SOLVERS:
        with pytest.raises(ValueError, match=s + ".*sequence parallelism"):
            F.check_solver_args(s, SR.TS4, sequence_parallel=True)


def test_flux_model_and_pipeline_refuse_before_any_library_call():
    """a FluxModel without a handle or a library, as in tests/test_host_denoise_options.py: a call that got past the Python checks would fail on the missing attribute"""
    import torch
    from diffusion_rs_amd import pipeline as pl
    from tests.util import SMALL_FLUX

    def model(sp=False):
        m = object.__new__(F.FluxModel)
        m.cfg, m.state_channels, m.cond_channels = dict(SMALL_FLUX), 64, 0
        if sp:
            m._sp_world = 2
        return m

    img, ids, txt, txt_ids = torch.zeros(1, 4, 64), torch.zeros(1, 4, 3), torch.zeros(1, 2, SMALL_FLUX["joint_attention_dim"]), torch.zeros(1, 2, 3)
    y, g = torch.zeros(1, SMALL_FLUX["pooled_projection_dim"]), torch.zeros(1)
    with pytest.raises(ValueError, match="heun.*step cache"):
        model().denoise(img, ids, txt, txt_ids, y, g, [1.0, 0.5, 0.0], solver="heun", cache_threshold=0.1)
    with pytest.raises(ValueError, match="sequence parallelism"):
        model(sp=True).denoise(img, ids, txt, txt_ids, y, g, [1.0, 0.5, 0.0], solver="dpmpp_2m")
    with pytest.raises(ValueError, match="strictly decreasing"):
        model().denoise(img, ids, txt, txt_ids, y, g, [1.0, 1.0, 0.0], solver="dpmpp_2m")
    with pytest.raises(ValueError, match="solver must be"):
        model().denoise(img, ids, txt, txt_ids, y, g, [1.0, 0.5, 0.0], solver="unipc")

    class RecordingPipeline(pl.Pipeline):
        def __init__(self):  # no GPU: only the request path in front of the chunk body is under test
            class _Flux:
                cond_channels = 0
            self.device, self.flux, self.calls = torch.device("cpu"), _Flux(), []

        def _generate_chunk(self, s, *a, **kw):
            self.calls.append(kw)
            return torch.zeros(len(s.prompts), 3, 16, 16, dtype=torch.uint8)

        def _generate_chunk_solver(self, solver, s, *a, **kw):
            self.calls.append(dict(kw, solver=solver))
            return torch.zeros(len(s.prompts), 3, 16, 16, dtype=torch.uint8)

    params = pl.DiffusionGenerationParams(16, 16, 2, 3.5)
    pipe = RecordingPipeline()
    with pytest.raises(ValueError, match="heun.*step cache"):
        pipe.generate_tensor(["p"], params, solver="heun", cache_threshold=0.1)
    with pytest.raises(ValueError, match="solver must be"):
        pipe.generate_tensor(["p"], params, solver="dpm")
    pipe._sp = object()
    with pytest.raises(ValueError, match="sequence parallelism"):
        pipe.generate_tensor(["p"], params, solver="heun")
    assert not pipe.calls
    pipe = RecordingPipeline()  # the solver's chunk call is made only when a solver is asked for: any other request makes exactly the call it always made
    pipe.generate_tensor(["p"], params)
    pipe.generate_tensor(["p"], params, solver="euler")
    pipe.forward(["p"], params, output="tensor", solver=None)
    pipe.generate_tensor(["p"], params, solver="dpmpp_2m", cache_threshold=0.1)
    pipe.forward(["p"], params, output="tensor", solver="heun")
    assert pipe.calls == [{}, {}, {}, {"solver": "dpmpp_2m"}, {"solver": "heun"}]


# ------------------------------------------------------------------------------------------------ 4. variant distances
@pytest.mark.parametrize("case", SR.CASES)
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_every_variant_is_far_from_the_correct_loop(shape, case):
    """At the GPU test's inputs every wrong composition but the demoted one lies at least 3 x the plain loop's bf16 error (SR.bf16_floor) from the correct loop.
    Measured on the oracle (ragged / aligned, plain): Heun — euler 8.0e-3, second_eval_on_x 8.0e-3, no_euler_last 4.2e-3, second_eval_at_t_i 2.5e-4 (demoted);
    2M — euler and no_history 7.8e-3, history_is_Dprime 3.2e-3; under the mask 1.1e-2 .. 6e-2, predictor_unblended 1.8e-2; under CFG from_pos_only 2.5e-3."""
    cfg, mask = SR.case_options(case)
    for solver in SR.SOLVERS:
        if case == "cache" and solver == "heun":  # (refused)
            continue
        ts = SR.SCHEDULES[SR.SOLVER_SCHEDULE[solver]]
        ref = SR.reference(solver, shape, case)
        assert np.isfinite(ref).all()
        for v in SR.variants_for(solver, cfg, mask, ts[-1] == 0.0):
            dist = rel_l2(SR.reference(solver, shape, case, None, v), ref)
            print(f"{shape} {case} {solver} {v}: {dist:.3e} ({dist / SR.bf16_floor(case):.1f} x the bf16 floor {SR.bf16_floor(case):.1e})")
            if v != SR.DEMOTED_VARIANT:
                assert dist >= 3 * SR.bf16_floor(case), (solver, v, dist)
    assert set(v for s in SR.SOLVERS for v in SR.variants_for(s, True, True, True)) == set(SR.VARIANTS)


def test_variants_that_are_the_correct_loop_where_they_do_not_apply():
    """why variants_for leaves them out: without a mask the unblended predictor, without a negative the prompt-only history, on a schedule that does not end at 0 the
    missing Euler step, are the correct loop; and on the full schedule 2M reads its history once, after a first-order step, where D' is D"""
    s, om = SR.inputs("ragged"), SR.oracle_model()
    ev = SR.oracle_eval(om, s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"])
    np.testing.assert_array_equal(SR.solve(ev, s["img"], SR.TS4, "heun", variant="heun_predictor_unblended"), SR.reference("heun", "ragged"))
    np.testing.assert_array_equal(SR.solve(ev, s["img"], SR.TS_CUT, "dpmpp_2m", variant="dpmpp_history_from_pos_only"), SR.reference("dpmpp_2m", "ragged"))
    np.testing.assert_array_equal(SR.solve(ev, s["img"], SR.TS4, "dpmpp_2m", variant="dpmpp_history_is_Dprime"), SR.solve(ev, s["img"], SR.TS4, "dpmpp_2m"))


# ------------------------------------------------------------------------------------------------ 5. ABI
def test_abi():
    code, lib = _header_code(), L.load()
    nargs = dict(fmi_flux_denoise_solver=10, fmi_heun_predict=13, fmi_heun_correct=12, fmi_dpmpp_2m_step=15, fmi_dpmpp_2m_coefficients=6, fmi_flux_solver_bytes=1)
    for sym, n in nargs.items():
        assert sym in L.EXPORTED
        assert re.search(r"\b(int|size_t)\s+" + sym + r"\s*\(", code), sym
        assert hasattr(lib, sym) and len(getattr(lib, sym).argtypes) == n, sym
        decl = re.search(r"\b" + sym + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(decl.split(",")) == n, (sym, decl)
    assert lib.fmi_flux_denoise_solver.argtypes == lib.fmi_flux_denoise_ip.argtypes[:5] + [C.POINTER(L.FluxSolver)] + lib.fmi_flux_denoise_ip.argtypes[5:]
    body = re.search(r"typedef\s+struct\s+fmi_flux_solver\s*\{(.*?)\}\s*fmi_flux_solver\s*;", code, flags=re.S).group(1)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["int kind"]
    assert [f[0] for f in L.FluxSolver._fields_] == ["kind"] and L.FluxSolver._fields_[0][1] is C.c_int and C.sizeof(L.FluxSolver) == 4
    enum = re.search(r"enum\s*\{\s*FMI_SOLVER_EULER\s*=\s*(\d+)\s*,\s*FMI_SOLVER_HEUN\s*=\s*(\d+)\s*,\s*FMI_SOLVER_DPMPP_2M\s*=\s*(\d+)\s*\}", code)
    assert tuple(int(v) for v in enum.groups()) == (L.SOLVER_EULER, L.SOLVER_HEUN, L.SOLVER_DPMPP_2M) == (0, 1, 2)
    assert F.SOLVERS == dict(euler=0, heun=1, dpmpp_2m=2)
    assert lib.fmi_abi_version() == 6 and C.sizeof(L.FluxDenoiseOptions) == 56
    assert len(F.REFUSED_PAIRS) == 8 and len(F.REFUSED_MODES) == 7  # the solver's two refusals are its own check's, not rows of the tables
    # a null handle is refused through the new entry as through the older ones, and a null solver is no error of its own
    inp, buf, ts = L.FluxInputs(), (C.c_float * 8)(), (C.c_double * 2)(1.0, 0.0)
    for sv in (None, C.byref(L.FluxSolver(L.SOLVER_HEUN))):
        assert lib.fmi_flux_denoise_solver(None, C.byref(inp), None, None, None, sv, buf, ts, 1, None) == L.ERR_INVALID
    assert lib.fmi_flux_solver_bytes(None) == 0
