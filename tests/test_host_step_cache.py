"""First-block step cache, the parts that need no device: the composed f32 reference of tests/step_cache_ref.py against the oracle's own
loop, the preconditions the GPU tests rely on (which steps a threshold of 0.235 reuses, and how far every distance is from it), the argument checker, and the
new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

from diffusion_rs_amd import _lib as L
from diffusion_rs_amd.flux import check_combination, check_step_cache_args
from tests import step_cache_ref as R
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fmi_flux_denoise_cached", "fmi_flux_step_cache_bytes")


@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_composed_loop_without_reuse_is_the_oracle_loop(shape):
    s, ts = R.inputs(shape), R.schedule(shape)
    lat, dec, dist = R.reference(shape, "plain")
    want = R.oracle_model().denoise(s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], ts)
    err = rel_l2(lat, want)
    print(f"[step cache] {shape}: composed loop vs om.denoise rel-L2 {err:.3e}")
    assert err <= 1e-6
    assert not dec.any() and (dist[0] == -1).all() and np.isfinite(dist[1:]).all() and (dist[1:] > 0).all()


@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_threshold_decisions_and_their_margin(shape):
    """What tests/test_gpu_step_cache.py's threshold test relies on: the decisions, and that no compared distance sits within 5 % of the threshold (the GPU's
    distances differ from these by the bf16 operands of block 0, about 1e-2 relative)."""
    lat, dec, dist = R.reference(shape, "threshold")
    print(f"[step cache] {shape}: threshold {R.THRESHOLD} decisions {dec.tolist()} max distances {np.round(dist.max(1), 4).tolist()}")
    assert dec.tolist() == R.THRESHOLD_DECISIONS
    assert (np.abs(dist[1:] / R.THRESHOLD - 1) >= 0.05).all()
    plain = R.reference(shape, "plain")[0]
    for kind in ("mask_a", "mask_b", "threshold"):  # reuse moves the trajectory, by far less than the 3e-2 loop bar
        moved = rel_l2(R.reference(shape, kind)[0], plain)
        print(f"[step cache] {shape}: {kind} vs plain rel-L2 {moved:.3e}")
        assert 1e-5 < moved < 1e-2


@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_repeated_schedule_reuse_is_exact_in_the_reference(shape):
    """Steps 1, 3, 5 of [1, 1, 0.6, 0.6, 0.25, 0.25, 0] repeat the state and time of the step before: their residual IS the reference residual, and reusing
    them changes the result only by the rounding of X1 + (XF - X1)."""
    plain = R.reference(shape, "repeat_plain")[0]
    lat, dec, dist = R.reference(shape, "repeat_cached")
    assert dec.tolist() == R.REPEAT_FORCE
    assert (dist[[1, 3, 5]] == 0.0).all() and (dist[[2, 4]] > 0).all() and (dist[0] == -1).all()
    assert rel_l2(lat, plain) <= 1e-6


def test_argument_checker():
    assert check_step_cache_args(8) == (None, None)
    assert check_step_cache_args(8, 0) == (0.0, None)
    thr, f = check_step_cache_args(3, None, [0, 1, -1])
    assert thr == 0.0 and f.dtype == np.int8 and f.tolist() == [0, 1, -1] and f.flags.c_contiguous
    assert check_step_cache_args(3, 0.5, np.array([-1, -1, 1]))[0] == 0.5
    for bad in (-0.1, float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="cache_threshold"):
            check_step_cache_args(8, bad)
    for bad in ([0, 1], [0, 1, 0, 1], [[0, 1, 0]], []):
        with pytest.raises(ValueError, match="one entry per step"):
            check_step_cache_args(3, 0.1, bad)
    with pytest.raises(ValueError, match="-1 .* 0 .* 1"):
        check_step_cache_args(3, 0.1, [0, 2, 0])
    with pytest.raises(ValueError, match=r"cache_force\[0\]"):
        check_step_cache_args(3, 0.1, [1, 0, 0])
    for n, thr, force in ((8, 0.1, None), (3, None, [0, 0, 0])):  # either of them asks for the cache (a threshold comes back): "cache" is present
        assert check_step_cache_args(n, thr, force)[0] is not None
        with pytest.raises(ValueError, match="sequence parallelism"):
            check_combination({"cache", "sequence_parallel"})
    assert check_step_cache_args(8, None, None) == (None, None) and check_combination({"sequence_parallel"}) is None  # no cache asked for: nothing to refuse


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+struct\s+fmi_flux_step_cache\s*\{[^}]*float\s+threshold;[^}]*const\s+int8_t\s*\*\s*force;[^}]*int32_t\s*\*\s*decisions_out;"
                     r"[^}]*float\s*\*\s*distances_out;[^}]*\}\s*fmi_flux_step_cache\s*;", code)
    assert re.search(r"\bint\s+fmi_flux_denoise_cached\s*\(", code) and re.search(r"\bsize_t\s+fmi_flux_step_cache_bytes\s*\(", code)
    assert "#define FMI_ABI_VERSION 6" in hdr  # an addition under the same number
    lib = L.load()
    for s in NEW_SYMBOLS:
        assert s in L.EXPORTED and hasattr(lib, s), s
    # the ctypes mirror: float, then three pointers with C's padding
    assert [f[0] for f in L.FluxStepCache._fields_] == ["threshold", "force", "decisions_out", "distances_out"]
    assert (L.FluxStepCache.force.offset, L.FluxStepCache.decisions_out.offset, L.FluxStepCache.distances_out.offset) == (8, 16, 24)
