"""First-block step cache of the denoise loop: fmi_flux_denoise_cached, FluxModel.denoise's cache_threshold= / cache_force= and the
pipeline's cache_threshold=.

Reuse moves a trajectory by 4.5e-4 .. 1.5e-3 on the CPU oracle (tests/test_host_step_cache.py) — far below the 3e-2 loop bar, which therefore cannot see
whether a step was reused, or with which sample's delta.  The exact properties carry the weight: a threshold of 0 IS the old loop bit for bit; on a schedule
that repeats its values the reused steps measure a distance of exactly 0 and the result is the plain loop's up to the rounding of X1 + (XF - X1); under a
forced mask a sample of a batch IS its single-sample run, latents and distances, bit for bit.  The composed f32 reference (tests/step_cache_ref.py) is the sanity
check of the whole: decisions, distances, and the final latents at the project's loop bar.

SMALL_FLUX, B = 2, T = 32, inputs of seed 7, guidance 3.5, 8 steps of the real schedule.  ragged: S = 4x6 = 24 (R = 35) — odd row counts, the stand-alone
relayout kernels; aligned: S = 8x8 = 64 (R = 48) — the fused q|k|v epilogues."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import step_cache_ref as R
from tests.util import SMALL_FLUX, SMALL_VAE, bf16_round, dev, host, rel_l2

pytestmark = pytest.mark.gpu

f32 = np.float32
B = R.B
# Bars set from what an MI355X measures (the tests print the figures; DESIGN.md section 5 records them).
# Exact reuse against the plain loop on the repeated schedule: 4 x the measured rel-L2, capped at 2e-4.  Measured: 0 in all four cases — X1 + (XF - X1) gave
# XF back wherever the final layer's bf16 rounding could have seen a difference — so the bar is equality.
# Distances against the f32 reference's: 3 x the measured relative error (1.84e-3 ragged, 1.93e-3 aligned: the bf16 operands of block 0), capped at 5e-2.
EXACT_REUSE_MEASURED, DISTANCE_MEASURED = 0.0, 1.931e-3
EXACT_REUSE_BAR = min(4 * EXACT_REUSE_MEASURED, 2e-4)
DISTANCE_BAR = min(3 * DISTANCE_MEASURED, 5e-2)


def _dev(a, dtype=None):
    return dev(np.array(a), dtype)  # (a copy: the shared inputs and references are read-only arrays)


@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    gm = d.FluxModel(SMALL_FLUX)
    gm.load_state_dict(R.state_dict())
    return dict(torch=torch, d=d, gm=gm)


def _run(env, shape, ts, sl=slice(None), gm=None, context=False, **kw):
    """FluxModel.denoise on samples `sl` of a shape set; returns host arrays: latents, or (latents, stats) with return_cache_stats"""
    torch, s = env["torch"], R.inputs(shape)
    kw = {k: (_dev(v[sl]) if isinstance(v, np.ndarray) and k in ("x0", "noise", "mask") else v) for k, v in kw.items()}
    if context:
        kw.update(context=_dev(s["ctx"][sl]), context_ids=_dev(s["rids"][sl]))
    out = (gm or env["gm"]).denoise(_dev(s["img"][sl]), _dev(s["ids"][sl]), _dev(s["txt"][sl], torch.bfloat16), _dev(s["txt_ids"][sl]), _dev(s["y"][sl]),
                                    _dev(s["g"][sl]), ts, **kw)
    return (host(out[0]), out[1]) if isinstance(out, tuple) else host(out)


def _inpaint_args(shape, seed=45):
    s = R.inputs(shape)
    rng = np.random.default_rng(seed)
    return dict(x0=rng.standard_normal(s["img"].shape).astype(np.float32), noise=np.array(s["img"]),
                mask=(rng.random(s["img"].shape) < 0.5).astype(np.float32))


def _ctypes_cached(env, shape, ts, cache, gm=None, sl=slice(None)):
    """fmi_flux_denoise_cached at the ctypes level (no context, no inpainting); `cache`: a FluxStepCache or None.  Returns (status, latents)"""
    torch, s = env["torch"], R.inputs(shape)
    gm = gm or env["gm"]
    img = _dev(s["img"][sl])
    inp, keep = gm._inputs(None, _dev(s["ids"][sl]), _dev(s["txt"][sl], torch.bfloat16), _dev(s["txt_ids"][sl]), None, _dev(s["y"][sl]), _dev(s["g"][sl]))
    tsc = (C.c_double * len(ts))(*ts)
    rc = gm.lib.fmi_flux_denoise_cached(gm.h, C.byref(inp), None, C.c_void_p(img.data_ptr()), tsc, len(ts) - 1, None, None, None,
                                        None if cache is None else C.byref(cache), None)
    torch.cuda.synchronize()
    return rc, host(img)


# ------------------------------------------------------------------------------------------------ 1. the hooks are inert
@pytest.mark.parametrize("variant", ["plain", "inpaint", "context"])
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_threshold_zero_is_the_old_loop_bit_for_bit(env, shape, variant):
    ts = R.schedule(shape)
    kw = _inpaint_args(shape) if variant == "inpaint" else {}
    ctx = variant == "context"
    want = _run(env, shape, ts, context=ctx, **kw)
    got, st = _run(env, shape, ts, context=ctx, cache_threshold=0, return_cache_stats=True, **kw)
    np.testing.assert_array_equal(got, want)
    assert st["decisions"].tolist() == [0] * 8
    assert st["distances"].shape == (8, B) and (st["distances"][0] == -1).all()
    assert np.isfinite(st["distances"][1:]).all() and (st["distances"][1:] > 0).all()
    if variant == "plain":  # a NULL cache is fmi_flux_denoise_context, which without a context is fmi_flux_denoise
        rc, null = _ctypes_cached(env, shape, ts, None)
        assert rc == 0
        np.testing.assert_array_equal(null, want)


# ------------------------------------------------------------------------------------------------ 2. exact reuse
@pytest.mark.parametrize("case", ["ragged", "aligned", "ragged-context", "ragged-int8"])
def test_reuse_on_a_repeated_schedule_is_exact(env, case):
    """Steps 1, 3, 5 of [1, 1, 0.6, 0.6, 0.25, 0.25, 0] see the very state and time of the step before (dt = 0): their residual IS the reference residual —
    distance exactly 0 for every sample — and reusing them gives the plain loop's latents up to the rounding of X1 + (XF - X1).  A wrong sample, row or stride
    in the delta is O(1) here."""
    from diffusion_rs_amd import _lib as L
    shape, ctx = case.split("-")[0], case.endswith("context")
    gm = None
    if case.endswith("int8"):
        gm = env["d"].FluxModel(SMALL_FLUX)
        gm.load_state_dict(R.state_dict())
        gm.quantize_int8()
    plain = _run(env, shape, R.REPEAT_TS, gm=gm, context=ctx)
    got, st = _run(env, shape, R.REPEAT_TS, gm=gm, context=ctx, cache_force=R.REPEAT_FORCE, return_cache_stats=True)
    err = rel_l2(got, plain)
    print(f"[step cache] exact reuse, {case}: cached vs plain loop rel-L2 {err:.3e} (bar {EXACT_REUSE_BAR:.1e}); distances {st['distances'].max(1).tolist()}")
    assert st["decisions"].tolist() == R.REPEAT_FORCE
    assert (st["distances"][[1, 3, 5]] == 0.0).all()
    assert (st["distances"][[2, 4]] > 0).all() and (st["distances"][0] == -1).all()
    assert np.isfinite(got).all() and err <= EXACT_REUSE_BAR
    if gm is not None:
        assert not np.array_equal(plain, _run(env, shape, R.REPEAT_TS))  # (it is the int8 model)
        gm.close()


# ------------------------------------------------------------------------------------------------ 3. against the oracle, forced
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_forced_mask_matches_the_composed_reference(env, shape):
    ts = R.schedule(shape)
    ref, rdec, rdist = R.reference(shape, "mask_a")
    got, st = _run(env, shape, ts, cache_force=R.MASK_A, return_cache_stats=True)
    err = rel_l2(got, ref)
    derr = float(np.abs(st["distances"][1:] / rdist[1:] - 1).max())
    print(f"[step cache] forced {R.MASK_A}, {shape}: final latents rel-L2 {err:.3e} vs the composed reference; distances within {derr:.3e} (bar {DISTANCE_BAR:.1e})")
    assert st["decisions"].tolist() == R.MASK_A == rdec.tolist()
    assert (st["distances"][0] == -1).all()
    assert err <= 3e-2
    assert derr <= DISTANCE_BAR
    # seven reused steps: the two references are 1.5e-3 apart and the loop's own error is about 4e-4, so the result must be nearer the cached one
    ref_b, ref_plain = R.reference(shape, "mask_b")[0], R.reference(shape, "plain")[0]
    got_b, st_b = _run(env, shape, ts, cache_force=R.MASK_B, return_cache_stats=True)
    near, far = rel_l2(got_b, ref_b), rel_l2(got_b, ref_plain)
    print(f"[step cache] forced {R.MASK_B}, {shape}: rel-L2 {near:.3e} vs the cached reference, {far:.3e} vs the uncached one ({rel_l2(ref_b, ref_plain):.3e} apart)")
    assert st_b["decisions"].tolist() == R.MASK_B
    assert near <= 3e-2 and near < far


# ------------------------------------------------------------------------------------------------ 4. threshold
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_threshold_decides_as_the_reference_does(env, shape):
    ts = R.schedule(shape)
    ref, rdec, rdist = R.reference(shape, "threshold")
    got, st = _run(env, shape, ts, cache_threshold=R.THRESHOLD, return_cache_stats=True)
    print(f"[step cache] threshold {R.THRESHOLD}, {shape}: decisions {st['decisions'].tolist()}, max distances {np.round(st['distances'].max(1), 4).tolist()}, "
          f"final latents rel-L2 {rel_l2(got, ref):.3e}")
    assert st["decisions"].tolist() == rdec.tolist() == R.THRESHOLD_DECISIONS
    for i in range(8):  # the decision is the stated rule on the reported values
        assert bool(st["decisions"][i]) == (i > 0 and bool(st["distances"][i].max() < R.THRESHOLD))
    assert rel_l2(got, ref) <= 3e-2


# ------------------------------------------------------------------------------------------------ 5. batch and run independence
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_samples_of_a_batch_are_their_single_sample_runs_and_runs_repeat(env, shape):
    from diffusion_rs_amd import _lib as L
    gm, ts = env["gm"], R.schedule(shape)
    L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 0))  # the modulation precompute picks its kernel by row count: pinned to the GEMV passes
    try:
        both, st = _run(env, shape, ts, cache_force=R.MASK_A, return_cache_stats=True)
        for b in range(B):
            one, st1 = _run(env, shape, ts, slice(b, b + 1), cache_force=R.MASK_A, return_cache_stats=True)
            np.testing.assert_array_equal(one, both[b:b + 1], err_msg=f"latents of sample {b}")
            np.testing.assert_array_equal(st1["distances"][:, 0], st["distances"][:, b], err_msg=f"distances of sample {b}")
        assert not np.array_equal(st["distances"][1:, 0], st["distances"][1:, 1])
    finally:
        L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 1))
    a, sa = _run(env, shape, ts, cache_threshold=R.THRESHOLD, return_cache_stats=True)
    b_, sb = _run(env, shape, ts, cache_threshold=R.THRESHOLD, return_cache_stats=True)
    np.testing.assert_array_equal(a, b_)
    np.testing.assert_array_equal(sa["decisions"], sb["decisions"])
    np.testing.assert_array_equal(sa["distances"], sb["distances"])


# ------------------------------------------------------------------------------------------------ 6. inpainting
def test_cached_loop_with_the_inpainting_step(env):
    shape = "ragged"
    ts, a = R.schedule(shape), _inpaint_args(shape)
    cached = _run(env, shape, ts, cache_force=R.MASK_A)
    ones = _run(env, shape, ts, cache_force=R.MASK_A, x0=a["x0"], noise=a["noise"], mask=np.ones_like(a["x0"]))
    np.testing.assert_array_equal(ones, cached)
    zeros, st = _run(env, shape, ts, cache_force=R.MASK_A, x0=a["x0"], noise=a["noise"], mask=np.zeros_like(a["x0"]), return_cache_stats=True)
    np.testing.assert_array_equal(zeros, a["x0"])
    assert st["decisions"].tolist() == R.MASK_A
    mixed = _run(env, shape, ts, cache_force=R.MASK_A, **a)  # kept latents end as x0, bit for bit
    np.testing.assert_array_equal(mixed[a["mask"] == 0], a["x0"][a["mask"] == 0])
    assert ts[-1] == 0.0 and not np.array_equal(cached, a["x0"]) and not np.array_equal(mixed[a["mask"] == 1], cached[a["mask"] == 1])


# ------------------------------------------------------------------------------------------------ 7. errors
def test_cached_entry_errors(env):
    from diffusion_rs_amd import _lib as L
    d, gm, shape = env["d"], env["gm"], "ragged"
    ts = R.schedule(shape)
    plain = _run(env, shape, ts)

    def cache(threshold=0.0, force=None):
        f = None if force is None else (C.c_int8 * len(force))(*force)
        return L.FluxStepCache(threshold, f if f is None else C.cast(f, C.POINTER(C.c_int8)), None, None), f

    for thr in (-0.5, float("nan")):
        assert _ctypes_cached(env, shape, ts, cache(thr)[0])[0] == L.ERR_INVALID
    for force in ([1, 0, 0, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0, 0], [0, 0, 0, -2, 0, 0, 0, 0]):
        sc, keep = cache(0.1, force)
        rc, lat = _ctypes_cached(env, shape, ts, sc)
        assert rc == L.ERR_INVALID
        np.testing.assert_array_equal(lat, R.inputs(shape)["img"])  # nothing ran
    # no double block: there is no block 0 to measure
    cfg0 = dict(SMALL_FLUX, num_layers=0)
    g0 = d.FluxModel(cfg0)
    g0.load_state_dict(d.synth.flux_state_dict_numpy(cfg0, seed=0))
    assert _ctypes_cached(env, shape, ts, cache(0.1)[0], gm=g0)[0] == L.ERR_UNSUPPORTED
    g0.close()
    # sequence parallelism (the exchange callback is never called: world 2 needs a second device)
    called = []
    cb = L.ALL_TO_ALL_FN(lambda *a: called.append(a) or 1)
    L.check(gm.lib.fmi_flux_set_sequence_parallel(gm.h, 0, 2, cb, None))
    try:
        assert _ctypes_cached(env, shape, ts, cache(0.1)[0], sl=slice(0, 1))[0] == L.ERR_UNSUPPORTED
    finally:
        L.check(gm.lib.fmi_flux_set_sequence_parallel(gm.h, 0, 1, L.ALL_TO_ALL_FN(), None))
    assert not called
    # int8 calibration recording
    gm.calibrate_int8(True)
    try:
        assert _ctypes_cached(env, shape, ts, cache(0.1)[0])[0] == L.ERR_STATE
    finally:
        gm.calibrate_int8(False)
    with pytest.raises(ValueError, match="cache_force"):
        _run(env, shape, ts, cache_force=[0, 1])
    with pytest.raises(ValueError, match="return_cache_stats"):
        _run(env, shape, ts, return_cache_stats=True)
    np.testing.assert_array_equal(_run(env, shape, ts), plain)  # the model is as it was


# ------------------------------------------------------------------------------------------------ 8. memory
def test_cache_buffers_come_with_the_first_cached_call_and_grow(env):
    d = env["d"]
    gm = d.FluxModel(SMALL_FLUX)
    gm.load_state_dict(R.state_dict())
    Dm = SMALL_FLUX["num_attention_heads"] * 128
    small, large = R.inputs("ragged")["S"], R.inputs("aligned")["S"]
    _run(env, "ragged", R.schedule("ragged"), gm=gm)
    _run(env, "ragged", R.schedule("ragged"), gm=gm, context=True, **_inpaint_args("ragged"))
    assert gm.step_cache_bytes() == 0  # the plain entries never allocate it
    got = _run(env, "ragged", R.schedule("ragged"), gm=gm, cache_force=R.MASK_A)
    have = gm.step_cache_bytes()
    assert 4 * B * small * Dm * 4 <= have <= 4 * B * small * Dm * 4 + 4096
    np.testing.assert_array_equal(got, _run(env, "ragged", R.schedule("ragged"), cache_force=R.MASK_A))
    got = _run(env, "aligned", R.schedule("aligned"), gm=gm, cache_force=R.MASK_A)  # a larger shape after a smaller one
    assert 4 * B * large * Dm * 4 <= gm.step_cache_bytes() <= 4 * B * large * Dm * 4 + 4096
    np.testing.assert_array_equal(got, _run(env, "aligned", R.schedule("aligned"), cache_force=R.MASK_A))
    got = _run(env, "ragged", R.schedule("ragged"), gm=gm, cache_force=R.MASK_A)  # and the smaller one again, in the larger buffers
    np.testing.assert_array_equal(got, _run(env, "ragged", R.schedule("ragged"), cache_force=R.MASK_A))
    gm.close()


# ------------------------------------------------------------------------------------------------ 9. the pipeline
H, W, STEPS, GUIDANCE, TP = 128, 192, 4, 3.5, 24


def test_pipeline_cache_threshold(tmp_path):
    import torch
    from safetensors.torch import save_file
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    sd, vsd = R.state_dict(), d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0)
    root = str(tmp_path / "tiny-flux")
    for sub in ("transformer", "vae", "scheduler"):
        os.makedirs(os.path.join(root, sub))
    json.dump({"_class_name": "FluxPipeline"}, open(os.path.join(root, "model_index.json"), "w"))
    json.dump({"_class_name": "FlowMatchEulerDiscreteScheduler", "base_image_seq_len": 256, "base_shift": 0.5, "max_image_seq_len": 4096,
               "max_shift": 1.15, "shift": 3.0, "use_dynamic_shifting": True}, open(os.path.join(root, "scheduler", "scheduler_config.json"), "w"))
    json.dump({k: SMALL_FLUX[k] for k in ("in_channels", "pooled_projection_dim", "joint_attention_dim", "num_attention_heads", "num_layers",
                                          "num_single_layers", "guidance_embeds")}, open(os.path.join(root, "transformer", "config.json"), "w"))
    json.dump(dict(SMALL_VAE), open(os.path.join(root, "vae", "config.json"), "w"))
    save_file({k: torch.from_numpy(v).to(torch.bfloat16) for k, v in sd.items()}, os.path.join(root, "transformer", "diffusion_pytorch_model.safetensors"))
    save_file({k: torch.from_numpy(v) for k, v in vsd.items()}, os.path.join(root, "vae", "diffusion_pytorch_model.safetensors"))
    pipe = d.Pipeline(d.ModelSource.ModelId(root))
    rng = np.random.default_rng(61)
    t5 = bf16_round(rng.standard_normal((B, TP, SMALL_FLUX["joint_attention_dim"])).astype(np.float32))
    clip = rng.standard_normal((B, SMALL_FLUX["pooled_projection_dim"])).astype(np.float32)
    lat = rng.standard_normal((B, 16, H // 8, W // 8)).astype(np.float32)
    params = d.DiffusionGenerationParams(height=H, width=W, num_steps=STEPS, guidance_scale=GUIDANCE)
    kw = dict(embeddings=(dev(t5, torch.bfloat16), dev(clip)), latents=dev(lat), output="tensor")
    plain = pipe.forward(["a", "b"], params, **kw)
    assert pipe.last_cache_stats == []
    zero = pipe.forward(["a", "b"], params, cache_threshold=0, **kw)
    assert torch.equal(zero, plain)
    assert len(pipe.last_cache_stats) == 1 and pipe.last_cache_stats[0]["decisions"].tolist() == [0] * STEPS
    u8, final = pipe.forward(["a", "b"], params, cache_threshold=1e9, return_latents=True, **kw)
    assert len(pipe.last_cache_stats) == 1 and pipe.last_cache_stats[0]["decisions"].tolist() == [0, 1, 1, 1]
    assert pipe.last_cache_stats[0]["distances"].shape == (STEPS, B)
    assert not torch.equal(u8, plain)
    # the oracle pipeline: pack -> the composed cached loop -> unpack -> decode -> u8
    om, ov = R.oracle_model(), orc.Vae(SMALL_VAE)
    ov.load(vsd)
    sched = pipe.scheduler
    mu = orc.calculate_shift((H // 16) * (W // 16), sched.base_image_seq_len, sched.max_image_seq_len, sched.base_shift, sched.max_shift)
    ts = orc.get_timesteps(STEPS, sched.use_dynamic_shifting, mu, sched.shift)
    noise, ids = orc.pack_latents(lat)
    ref, rdec, _ = R.composed_denoise(om, sd, SMALL_FLUX, noise, ids, t5, np.zeros((B, TP, 3), np.float32), clip, np.full(B, GUIDANCE, np.float32), ts, threshold=1e9)
    assert rdec.tolist() == [0, 1, 1, 1]
    err = rel_l2(host(final), ref)
    z = orc.unpack_latents(ref, 16, H // 8, W // 8) * f32(1.0 / SMALL_VAE["scaling_factor"]) + f32(SMALL_VAE["shift_factor"])
    ref_u8 = orc.postprocess_u8(ov.decode(z.astype(np.float32)))
    diff = np.abs(u8.cpu().numpy().astype(np.int32) - ref_u8.astype(np.int32))
    share = float((diff <= 2).mean())
    print(f"[step cache] pipeline cache_threshold=1e9 ({H} x {W}, {STEPS} steps, B=2): final latents rel-L2 {err:.3e}; u8 within 2 on {share:.4f}, max |d| {int(diff.max())}")
    assert err <= 3e-2 and share >= 0.99
    with pytest.raises(ValueError, match="cache_threshold"):
        pipe.forward(["a", "b"], params, cache_threshold=-1.0, **kw)
    pipe._sp = object()  # what enable_sequence_parallel leaves behind (its wiring needs a second device)
    try:
        with pytest.raises(ValueError, match="sequence parallel"):
            pipe.forward(["a", "b"], params, cache_threshold=0.1, **kw)
    finally:
        pipe._sp = None
