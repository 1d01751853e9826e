"""Reference-image (FLUX.1 Kontext) conditioning: fmi_flux_forward_context / fmi_flux_denoise_context / fmi_latent_ids and the
pipeline's reference=.

What the semantics promise exactly is compared bit for bit: an evaluation with a context IS the evaluation on the concatenated tokens, rows [0, S);
the loop IS the chain of one-step loops on the concatenated state with the context rows restored after each step; no context IS the old entry.
Zero tolerance is what catches a misplaced row, id or stride: on the CPU oracle at the ragged shapes below, dropping the context moves a prediction
by only 3.4e-3 and reversing its rows by 1.2e-3 — the 3e-2 loop bar sees neither.  The distance to the oracle is the sanity check of the whole
composition, with the project's existing bars (tests/test_gpu_flux.py: rel-L2 <= 3e-2 after the loop; tests/test_gpu_pipeline.py: u8 within 2 on
>= 99 %).

B = 2, T = 32.  ragged: S = 4x6 = 24, R = 5x7 = 35 — no token count or offset is a multiple of 16, so the stand-alone relayout kernels run and the row
counts are odd.  aligned: S = 8x8 = 64, R = 6x8 = 48 — the fused q|k|v epilogues run."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.util import SMALL_FLUX, SMALL_VAE, bf16_round, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu

f32 = np.float32
SCALE, SHIFT = f32(SMALL_VAE["scaling_factor"]), f32(SMALL_VAE["shift_factor"])
B, T = 2, 32
SHAPES = {"ragged": ((4, 6), (5, 7)), "aligned": ((8, 8), (6, 8))}


def _np_ids(Bn, h2, w2, id0=0.0, row0=0.0, col0=0.0):
    ids = np.empty((Bn, h2 * w2, 3), np.float32)
    ids[:, :, 0] = f32(id0)
    ids[:, :, 1] = (f32(row0) + np.repeat(np.arange(h2), w2).astype(np.float32))[None]
    ids[:, :, 2] = (f32(col0) + np.tile(np.arange(w2), h2).astype(np.float32))[None]
    return ids


def _offset_view(torch, a):
    """a copy of `a` on the device that starts one float past a 16-byte boundary: the scalar path of the row cast"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    sd = d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    gm = d.FluxModel(SMALL_FLUX)
    gm.load_state_dict(sd)
    om = orc.Flux(SMALL_FLUX)
    om.load(sd)
    sets = {}
    for name, (s_hw, r_hw) in SHAPES.items():
        img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, s_hw, T, seed=41)
        ctx = flux_inputs(SMALL_FLUX, B, r_hw, T, seed=42)[0]  # another seed than the image's
        rids = _np_ids(B, r_hw[0], r_hw[1], id0=1.0)
        sets[name] = dict(S=s_hw[0] * s_hw[1], R=r_hw[0] * r_hw[1], img=img, ids=ids, txt=txt, txt_ids=txt_ids, y=y, ctx=ctx, rids=rids,
                          cat=np.concatenate([img, ctx], 1), cat_ids=np.concatenate([ids, rids], 1))
    g = np.full(B, 3.5, np.float32)
    t = np.full(B, 0.7, np.float32)
    return dict(torch=torch, d=d, orc=orc, sd=sd, gm=gm, om=om, sets=sets, g=g, t=t, ts4=[1.0, 0.8, 0.55, 0.3, 0.0])


def _fwd(env, gm, s, img, ids, sl=slice(None), **ctx):
    torch = env["torch"]
    return host(gm.forward(dev(img[sl]), dev(ids[sl]), dev(s["txt"][sl], torch.bfloat16), dev(s["txt_ids"][sl]), dev(env["t"][sl]), dev(s["y"][sl]),
                           dev(env["g"][sl]), **ctx))


def _loop(env, s, img, ids, ts, sl=slice(None), **extra):
    torch = env["torch"]
    extra = {k: (v if v is None or isinstance(v, torch.Tensor) else dev(v[sl])) for k, v in extra.items()}
    return host(env["gm"].denoise(dev(img[sl]), dev(ids[sl]), dev(s["txt"][sl], torch.bfloat16), dev(s["txt_ids"][sl]), dev(s["y"][sl]), dev(env["g"][sl]),
                                  ts, **extra))


# ------------------------------------------------------------------------------------------------ 1. latent_ids
def test_latent_ids_is_the_numpy_expression_and_pack_latents_ids_at_the_defaults():
    import diffusion_rs_amd as d
    for (Bn, h2, w2, id0, r0, c0) in ((2, 5, 7, 1.0, 0.0, 0.0), (1, 3, 4, 2.0, 0.5, -3.25), (3, 1, 1, 0.0, 100.0, 7.0), (1, 40, 33, 1.0, 0.0, 64.0)):
        got = host(d.latent_ids(Bn, h2, w2, id0=id0, row0=r0, col0=c0))
        np.testing.assert_array_equal(got, _np_ids(Bn, h2, w2, id0, r0, c0))
    z = np.zeros((2, 16, 8, 12), np.float32)
    np.testing.assert_array_equal(host(d.latent_ids(2, 4, 6)), host(d.pack_latents(dev(z))[1]))


# ------------------------------------------------------------------------------------------------ 2. one evaluation, exact
@pytest.mark.parametrize("form", ["f32", "bf16", "offset"])
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_forward_with_context_is_the_forward_on_the_concatenation(env, shape, form):
    torch, gm, s = env["torch"], env["gm"], env["sets"][shape]
    want = _fwd(env, gm, s, s["cat"], s["cat_ids"])[:, :s["S"]]
    ctx = {"f32": lambda: dev(s["ctx"]), "bf16": lambda: dev(s["ctx"], torch.bfloat16), "offset": lambda: _offset_view(torch, s["ctx"])}[form]()
    got = _fwd(env, gm, s, s["img"], s["ids"], context=ctx, context_ids=dev(s["rids"]))
    assert got.shape == s["img"].shape and np.isfinite(got).all()
    np.testing.assert_array_equal(got, want)
    if form == "f32":  # the context matters, and which rows are the state's matters
        assert not np.array_equal(got, _fwd(env, gm, s, s["img"], s["ids"]))


def test_forward_with_context_after_quantize_int8(env):
    d, s = env["d"], env["sets"]["aligned"]
    gq = d.FluxModel(SMALL_FLUX)
    gq.load_state_dict(env["sd"])
    gq.quantize_int8()
    want = _fwd(env, gq, s, s["cat"], s["cat_ids"])[:, :s["S"]]
    got = _fwd(env, gq, s, s["img"], s["ids"], context=dev(s["ctx"]), context_ids=dev(s["rids"]))
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, _fwd(env, env["gm"], s, s["img"], s["ids"], context=dev(s["ctx"]), context_ids=dev(s["rids"])))  # (it is the int8 model)
    gq.close()


# ------------------------------------------------------------------------------------------------ 3. no context is the old path
def _ctypes_loop(env, s, ctx_struct, extra=(None, None, None)):
    """fmi_flux_denoise_context at the ctypes level on a copy of the ragged image; returns (status, result)"""
    from diffusion_rs_amd import _lib as L
    torch, gm = env["torch"], env["gm"]
    img = dev(s["img"]).clone()
    inp, keep = gm._inputs(None, dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), None, dev(s["y"]), dev(env["g"]))
    ts = (C.c_double * 5)(*env["ts4"])
    p = [None if e is None else C.c_void_p(e.data_ptr()) for e in extra]
    rc = gm.lib.fmi_flux_denoise_context(gm.h, C.byref(inp), None if ctx_struct is None else C.byref(ctx_struct), C.c_void_p(img.data_ptr()), ts, 4,
                                         p[0], p[1], p[2], None)
    torch.cuda.synchronize()
    return rc, host(img)


def test_no_context_is_the_old_loop_bit_for_bit(env):
    from diffusion_rs_amd import _lib as L
    s = env["sets"]["ragged"]
    plain = _loop(env, s, s["img"], s["ids"], env["ts4"])
    np.testing.assert_array_equal(_loop(env, s, s["img"], s["ids"], env["ts4"], context=None, context_ids=None), plain)
    for ctx_struct in (None, L.FluxContext(None, 0, None, 0), L.FluxContext(C.c_void_p(dev(s["ctx"]).data_ptr()), 7, None, 0)):  # R = 0: nothing else is read
        rc, got = _ctypes_loop(env, s, ctx_struct)
        assert rc == 0
        np.testing.assert_array_equal(got, plain)
    x0 = np.random.default_rng(43).standard_normal(s["img"].shape).astype(np.float32)
    mask = (np.random.default_rng(44).random(s["img"].shape) < 0.5).astype(np.float32)
    inpaint = _loop(env, s, s["img"], s["ids"], env["ts4"], x0=x0, noise=s["img"], mask=mask)
    assert not np.array_equal(inpaint, plain)
    for ctx_struct in (None, L.FluxContext(None, 0, None, 0)):
        rc, got = _ctypes_loop(env, s, ctx_struct, (dev(x0), dev(s["img"]), dev(mask)))
        assert rc == 0
        np.testing.assert_array_equal(got, inpaint)


# ------------------------------------------------------------------------------------------------ 4. the loop, exact
@pytest.mark.parametrize("shape", ["ragged", "aligned"])
def test_loop_with_context_is_the_chain_of_one_step_loops_on_the_concatenation(env, shape):
    from diffusion_rs_amd import _lib as L
    gm, s, ts = env["gm"], env["sets"][shape], env["ts4"]
    S = s["S"]
    L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 0))  # the modulation precompute picks its kernel by row count: pinned to the GEMV passes
    try:
        # the plain loop has the chain property: 4 steps == four one-step loops (the hoisted txt_in and the per-image modulation passes keep the bits)
        x = s["img"]
        for i in range(4):
            x = _loop(env, s, x, s["ids"], ts[i:i + 2])
        np.testing.assert_array_equal(_loop(env, s, s["img"], s["ids"], ts), x, err_msg="plain loop vs its one-step chain")
        # with a context: the chain runs on the (B, S + R, C) state, and the context rows — which the one-step loop updates too — are restored
        x = s["cat"].copy()
        for i in range(4):
            x = _loop(env, s, x, s["cat_ids"], ts[i:i + 2])
            x[:, S:] = s["ctx"]
        both = _loop(env, s, s["img"], s["ids"], ts, context=s["ctx"], context_ids=s["rids"])
        assert both.shape == s["img"].shape and np.isfinite(both).all()
        np.testing.assert_array_equal(both, x[:, :S])
        for b in range(B):  # samples of a batch are independent trajectories
            one = _loop(env, s, s["img"], s["ids"], ts, slice(b, b + 1), context=s["ctx"], context_ids=s["rids"])
            np.testing.assert_array_equal(one, both[b:b + 1], err_msg=f"sample {b}")
    finally:
        L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 1))


# ------------------------------------------------------------------------------------------------ 5. the loop against the oracle
def _oracle_loop(om, s, x, ts, g, with_context=True):
    """om.forward on the concatenated tokens, rows [0, S), then the Euler step in numpy f32"""
    S = x.shape[1]
    for i in range(len(ts) - 1):
        t = np.full(x.shape[0], f32(ts[i]), np.float32)
        if with_context:
            pred = om.forward(np.concatenate([x, s["ctx"]], 1), np.concatenate([s["ids"], s["rids"]], 1), s["txt"], s["txt_ids"], t, s["y"], g)[:, :S]
        else:
            pred = om.forward(x, s["ids"], s["txt"], s["txt_ids"], t, s["y"], g)
        x = (x + pred * f32(ts[i + 1] - ts[i])).astype(np.float32)
    return x


def test_loop_with_context_matches_the_oracle_composition(env):
    d, om, s = env["d"], env["om"], env["sets"]["ragged"]
    sched = d.SchedulerConfig()
    ts = sched.get_timesteps(4, sched.calculate_shift(s["S"]))
    got = _loop(env, s, s["img"], s["ids"], ts, context=s["ctx"], context_ids=s["rids"])
    ref = _oracle_loop(om, s, s["img"].copy(), ts, env["g"])
    ref_plain = _oracle_loop(om, s, s["img"].copy(), ts, env["g"], with_context=False)
    err = rel_l2(got, ref)
    print(f"context loop, 4 steps, B=2, S=24 + R=35 + T=32: final latents rel-L2 {err:.3e} vs the oracle composition; "
          f"the oracle's own with-context vs without-context distance {rel_l2(ref, ref_plain):.3e}")
    assert err <= 3e-2
    assert not np.array_equal(got, _loop(env, s, s["img"], s["ids"], ts))


# ------------------------------------------------------------------------------------------------ 6. with the inpainting step
def test_context_loop_with_the_inpainting_step(env):
    s, ts = env["sets"]["ragged"], env["ts4"]
    kw = dict(context=s["ctx"], context_ids=s["rids"])
    x0 = np.random.default_rng(45).standard_normal(s["img"].shape).astype(np.float32)
    plain = _loop(env, s, s["img"], s["ids"], ts, **kw)
    ones = _loop(env, s, s["img"], s["ids"], ts, x0=x0, noise=s["img"], mask=np.ones_like(x0), **kw)
    np.testing.assert_array_equal(ones, plain)
    zeros = _loop(env, s, s["img"], s["ids"], ts, x0=x0, noise=s["img"], mask=np.zeros_like(x0), **kw)
    np.testing.assert_array_equal(zeros, x0)
    assert ts[-1] == 0.0 and not np.array_equal(plain, x0)


# ------------------------------------------------------------------------------------------------ 7. errors
def test_context_errors(env):
    from diffusion_rs_amd import _lib as L
    torch, gm, s = env["torch"], env["gm"], env["sets"]["ragged"]
    ctx, rids = dev(s["ctx"]), dev(s["rids"])
    pc, pr = C.c_void_p(ctx.data_ptr()), C.c_void_p(rids.data_ptr())
    assert _ctypes_loop(env, s, L.FluxContext(pc, L.F32, None, s["R"]))[0] == L.ERR_INVALID      # no ctx_ids
    assert _ctypes_loop(env, s, L.FluxContext(None, L.F32, pr, s["R"]))[0] == L.ERR_INVALID      # no ctx
    assert _ctypes_loop(env, s, L.FluxContext(pc, L.F32, pr, -1))[0] == L.ERR_INVALID            # negative R
    assert _ctypes_loop(env, s, L.FluxContext(pc, L.F16, pr, s["R"]))[0] == L.ERR_INVALID        # a dtype that is neither F32 nor BF16
    x0 = dev(s["img"])
    assert _ctypes_loop(env, s, L.FluxContext(pc, L.F32, pr, s["R"]), (x0, None, x0))[0] == L.ERR_INVALID  # x0 / noise / mask in part
    assert _ctypes_loop(env, s, None, (None, x0, None))[0] == L.ERR_INVALID
    fwd = lambda **k: gm.forward(dev(s["img"]), dev(s["ids"]), dev(s["txt"], torch.bfloat16), dev(s["txt_ids"]), dev(env["t"]), dev(s["y"]), dev(env["g"]), **k)
    with pytest.raises(ValueError, match="go together"):
        fwd(context=ctx)
    with pytest.raises(ValueError, match="channels"):
        fwd(context=ctx[:, :, :32].contiguous(), context_ids=rids)  # (B,R,32): the library would read past it
    with pytest.raises(ValueError, match="is on cpu"):
        fwd(context=ctx.cpu(), context_ids=rids)
    # under sequence parallelism a context is refused before anything runs (the exchange callback is never called: world 2 needs a second device)
    called = []
    cb = L.ALL_TO_ALL_FN(lambda *a: called.append(a) or 1)
    L.check(gm.lib.fmi_flux_set_sequence_parallel(gm.h, 0, 2, cb, None))
    try:
        sl = slice(0, 1)
        one = L.FluxContext(C.c_void_p(ctx.data_ptr()), L.F32, C.c_void_p(rids.data_ptr()), s["R"])
        img = dev(s["img"][sl])
        inp, keep = gm._inputs(img, dev(s["ids"][sl]), dev(s["txt"][sl], torch.bfloat16), dev(s["txt_ids"][sl]), dev(env["t"][sl]), dev(s["y"][sl]), dev(env["g"][sl]))
        pred = torch.empty_like(img)
        assert gm.lib.fmi_flux_forward_context(gm.h, C.byref(inp), C.byref(one), C.c_void_p(pred.data_ptr()), None) == L.ERR_UNSUPPORTED
        ts = (C.c_double * 5)(*env["ts4"])
        assert gm.lib.fmi_flux_denoise_context(gm.h, C.byref(inp), C.byref(one), C.c_void_p(img.data_ptr()), ts, 4, None, None, None, None) == L.ERR_UNSUPPORTED
    finally:
        L.check(gm.lib.fmi_flux_set_sequence_parallel(gm.h, 0, 1, L.ALL_TO_ALL_FN(), None))
    assert not called
    np.testing.assert_array_equal(_ctypes_loop(env, s, None)[1], _loop(env, s, s["img"], s["ids"], env["ts4"]))  # the model is as it was


# ------------------------------------------------------------------------------------------------ 8. the pipeline
H, W, HR, WR, STEPS, GUIDANCE, TP = 128, 192, 96, 64, 4, 3.5, 24


def _np_preprocess(u):
    return (u.astype(np.float32) + f32(0.5)) / f32(127.5) - f32(1)


def _structured_u8(rng, Bn, Hh, Ww, phase):
    yy, xx = np.mgrid[0:Hh, 0:Ww]
    base = np.stack([127.5 + 100 * np.sin(xx / 17.0 + b + phase) * np.cos(yy / 11.0 + c) for b in range(Bn) for c in range(3)]).reshape(Bn, 3, Hh, Ww)
    return np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1).copy()


@pytest.fixture(scope="module")
def pipe_env(tmp_path_factory):
    """a diffusers directory of a small flux and a small VAE with encoder whose model_index.json names FluxKontextPipeline"""
    import torch
    from safetensors.torch import save_file
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    sd = d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    vsd = d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0, encoder=True)
    root = str(tmp_path_factory.mktemp("kontext") / "tiny-kontext")
    for sub in ("transformer", "vae", "scheduler"):
        os.makedirs(os.path.join(root, sub))
    json.dump({"_class_name": "FluxKontextPipeline"}, open(os.path.join(root, "model_index.json"), "w"))
    json.dump({"_class_name": "FlowMatchEulerDiscreteScheduler", "base_image_seq_len": 256, "base_shift": 0.5, "max_image_seq_len": 4096,
               "max_shift": 1.15, "shift": 3.0, "use_dynamic_shifting": True}, open(os.path.join(root, "scheduler", "scheduler_config.json"), "w"))
    json.dump({k: SMALL_FLUX[k] for k in ("in_channels", "pooled_projection_dim", "joint_attention_dim", "num_attention_heads", "num_layers",
                                          "num_single_layers", "guidance_embeds")}, open(os.path.join(root, "transformer", "config.json"), "w"))
    json.dump(dict(SMALL_VAE), open(os.path.join(root, "vae", "config.json"), "w"))
    save_file({k: torch.from_numpy(v).to(torch.bfloat16) for k, v in sd.items()}, os.path.join(root, "transformer", "diffusion_pytorch_model.safetensors"))
    save_file({k: torch.from_numpy(v) for k, v in vsd.items()}, os.path.join(root, "vae", "diffusion_pytorch_model.safetensors"))
    pipe = d.Pipeline(d.ModelSource.ModelId(root))
    om, ov = orc.Flux(SMALL_FLUX), orc.Vae(SMALL_VAE)
    om.load(sd)
    ov.load(vsd)
    rng = np.random.default_rng(51)
    t5 = bf16_round(rng.standard_normal((B, TP, SMALL_FLUX["joint_attention_dim"])).astype(np.float32))
    clip = rng.standard_normal((B, SMALL_FLUX["pooled_projection_dim"])).astype(np.float32)
    lat = rng.standard_normal((B, 16, H // 8, W // 8)).astype(np.float32)
    ref_u8 = _structured_u8(rng, B, HR, WR, 0.0)   # 96 x 64: another size than the 128 x 192 output
    src_u8 = _structured_u8(rng, B, H, W, 1.5)
    params = d.DiffusionGenerationParams(height=H, width=W, num_steps=STEPS, guidance_scale=GUIDANCE)
    sched = pipe.scheduler
    mu = orc.calculate_shift((H // 16) * (W // 16), sched.base_image_seq_len, sched.max_image_seq_len, sched.base_shift, sched.max_shift)  # from S alone
    ts = orc.get_timesteps(STEPS, sched.use_dynamic_shifting, mu, sched.shift)
    kw = dict(embeddings=(dev(t5, torch.bfloat16), dev(clip)), latents=dev(lat))
    return dict(torch=torch, d=d, orc=orc, pipe=pipe, om=om, ov=ov, t5=t5, clip=clip, lat=lat, ref_u8=ref_u8, src_u8=src_u8, params=params, ts=ts, kw=kw,
                g=np.full(B, GUIDANCE, np.float32))


@pytest.mark.parametrize("hw", [(HR, WR), (16, 16), (64, 64)])  # 12 x 8 = 96 and 2 x 2 = 4 latent positions: no multiple of the GEMM's K tile; 8 x 8 = 64: one
def test_vae_encodes_a_reference_of_any_multiple_of_16(pipe_env, hw):
    """the mid-block attention pads its key dimension to 64 (the zero pad adds nothing to P V); bar: tests/test_gpu_vae.py::test_vae_encode_matches_oracle's 2e-2"""
    env = pipe_env
    img = _np_preprocess(_structured_u8(np.random.default_rng(52), B, hw[0], hw[1], 0.7).transpose(0, 3, 1, 2))
    rz, rm = env["ov"].encode(img, noise=None, return_moments=True)
    gz, gm = env["pipe"].vae.encode(dev(img), return_moments=True)
    gz, gm = host(gz), host(gm)
    print(f"vae encode {hw[0]} x {hw[1]} ({hw[0] // 8 * (hw[1] // 8)} latent positions): moments rel-L2 {rel_l2(gm, rm):.3e}, mean rel-L2 {rel_l2(gz, rz):.3e}")
    assert np.isfinite(gm).all() and rel_l2(gm, rm) <= 2e-2 and rel_l2(gz, rz) <= 2e-2


def test_vae_decode_and_mid_attention_at_96_latent_positions(pipe_env):
    """the padded key dimension behind the other two callers of the mid-block attention: the decoder (bar: the 2e-2 of tests/test_gpu_vae.py) and
    fmi_vae_mid_attention (bars: the 4e-3 / 2e-2 on the branch alone of tests/test_gpu_production_shapes.py), at 12 x 8 = 96 positions"""
    env = pipe_env
    torch, ov, gv = env["torch"], env["ov"], env["pipe"].vae
    rng = np.random.default_rng(53)
    z = rng.standard_normal((B, 16, HR // 8, WR // 8)).astype(np.float32)
    derr = rel_l2(host(gv.decode(dev(z))), ov.decode(z))
    x = bf16_round((1.5 * rng.standard_normal((B, SMALL_VAE["block_out_channels"][-1], HR // 8, WR // 8))).astype(np.float32))
    ref = ov.mid_attention(x)
    got = host(gv.mid_attention(dev(x.transpose(0, 2, 3, 1).copy(), torch.bfloat16))).transpose(0, 3, 1, 2)
    err, delta = rel_l2(got, ref), rel_l2(got - x, ref - x)
    print(f"12 x 8 latent positions: vae decode rel-L2 {derr:.3e}; AttnBlock rel-L2 {err:.3e}, of the attention branch alone {delta:.3e}")
    assert derr <= 2e-2
    assert np.isfinite(got).all() and err <= 4e-3 and delta <= 2e-2


def test_pipeline_reference_matches_the_oracle_pipeline(pipe_env):
    env = pipe_env
    orc, om, ov, pipe, ts = env["orc"], env["om"], env["ov"], env["pipe"], env["ts"]
    u8, final = pipe.forward(["a", "b"], env["params"], output="tensor", reference=env["ref_u8"], return_latents=True, **env["kw"])
    assert tuple(final.shape) == (B, (H // 16) * (W // 16), 64) and tuple(u8.shape) == (B, 3, H, W)
    # the oracle pipeline: encode (posterior mean) -> affine -> pack; ids with 1 in axis 0; the composed loop from the same noise; unpack -> decode -> u8
    ref_f32 = _np_preprocess(env["ref_u8"].transpose(0, 3, 1, 2))
    ctx, rids = orc.pack_latents(((ov.encode(ref_f32, noise=None) - SHIFT) * SCALE).astype(np.float32))
    rids = rids.copy()
    rids[:, :, 0] = 1
    np.testing.assert_array_equal(rids, _np_ids(B, HR // 16, WR // 16, id0=1.0))
    noise, ids = orc.pack_latents(env["lat"])
    s = dict(ctx=ctx, rids=rids, ids=ids, txt=env["t5"], txt_ids=np.zeros((B, TP, 3), np.float32), y=env["clip"])
    ref = _oracle_loop(om, s, noise.copy(), ts, env["g"])
    err = rel_l2(host(final), ref)
    z = orc.unpack_latents(ref, 16, H // 8, W // 8) * f32(1.0 / SMALL_VAE["scaling_factor"]) + SHIFT
    ref_u8 = orc.postprocess_u8(ov.decode(z.astype(np.float32)))
    diff = np.abs(u8.cpu().numpy().astype(np.int32) - ref_u8.astype(np.int32))
    share, worst = float((diff <= 2).mean()), int(diff.max())
    print(f"pipeline reference= (96 x 64 reference, 128 x 192 output, {STEPS} steps, B=2): final latents rel-L2 {err:.3e}; u8 within 2 on {share:.4f}, max |d| {worst}")
    assert err <= 3e-2
    assert share >= 0.99
    plain = pipe.forward(["a", "b"], env["params"], output="tensor", **env["kw"])
    assert not env["torch"].equal(u8, plain)
    # the f32 (B,3,Hr,Wr) form of the same reference is the same request
    u8_f = pipe.forward(["a", "b"], env["params"], output="tensor", reference=dev(ref_f32), **env["kw"])
    assert env["torch"].equal(u8, u8_f)


def test_pipeline_one_reference_broadcasts_over_the_prompts(pipe_env):
    env = pipe_env
    pipe, one = env["pipe"], env["ref_u8"][0]
    bcast = pipe.forward(["a", "b"], env["params"], output="tensor", reference=one, **env["kw"])
    explicit = pipe.forward(["a", "b"], env["params"], output="tensor", reference=np.stack([one, one]), **env["kw"])
    assert env["torch"].equal(bcast, explicit)
    assert not env["torch"].equal(bcast[0], bcast[1])


def test_pipeline_reference_with_image_and_mask_keeps_the_kept_latents(pipe_env):
    env = pipe_env
    pipe, d, orc = env["pipe"], env["d"], env["orc"]
    mask = np.zeros((B, H, W), bool)
    mask[0, 24:88, 40:136] = True
    mask[1, :, 96:] = True
    u8, final = pipe.forward(["a", "b"], env["params"], output="tensor", image=env["src_u8"], strength=0.75, mask=mask, reference=env["ref_u8"],
                             return_latents=True, **env["kw"])
    lat_m = mask.reshape(B, H // 8, 8, W // 8, 8).mean((2, 4)).astype(np.float32)
    m = orc.pack_latents(np.ascontiguousarray(np.broadcast_to(lat_m[:, None], (B, 16, H // 8, W // 8)), dtype=np.float32))[0]
    gx0, _ = d.encode_latents(pipe.vae.encode(d.preprocess_u8(dev(env["src_u8"]), interleaved=True)), pipe.vae.scale_factor(), pipe.vae.shift_factor())
    got = host(final)
    np.testing.assert_array_equal(got[m == 0], host(gx0)[m == 0])
    assert not np.array_equal(got[m == 1], host(gx0)[m == 1])
    no_ref = pipe.forward(["a", "b"], env["params"], output="tensor", image=env["src_u8"], strength=0.75, mask=mask, **env["kw"])
    assert not env["torch"].equal(u8, no_ref)


def test_pipeline_rejects_bad_reference_arguments(pipe_env):
    env = pipe_env
    pipe, ref = env["pipe"], env["ref_u8"]
    go = lambda r: pipe.forward(["a", "b"], env["params"], output="tensor", reference=r, **env["kw"])
    with pytest.raises(ValueError, match="multiples of 16"):
        go(np.zeros((72, 64, 3), np.uint8))
    with pytest.raises(ValueError, match="uint8 reference must be"):
        go(np.zeros((96, 64), np.uint8))  # rank
    with pytest.raises(ValueError, match="uint8 or float"):
        go(np.zeros((96, 64, 3), np.int32))  # dtype
    with pytest.raises(ValueError, match="samples for"):
        go(np.concatenate([ref, ref[:1]]))  # three references for two prompts
    pipe._sp = object()  # what enable_sequence_parallel leaves behind (its wiring needs a second device)
    try:
        with pytest.raises(ValueError, match="sequence parallel"):
            go(ref)
    finally:
        pipe._sp = None
    assert go(None).shape == (B, 3, H, W)  # the pipeline is as it was
