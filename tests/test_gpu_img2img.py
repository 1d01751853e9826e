"""Image-to-image and inpainting: the tensor glue bit for bit against numpy, the masked denoise loop
(fmi_flux_denoise_inpaint) against the oracle composed step by step, and the pipeline's image= / strength= / mask= against the oracle pipeline.

Tolerances are the project's existing ones: rel-L2 <= 3e-2 on the latents after the Euler loop (tests/test_gpu_flux.py), u8 within 2 on >= 99 % of
the pixels end to end (tests/test_gpu_pipeline.py).  Everything that the semantics promise exactly (mask 1 / mask 0, t = 1 / t = 0, kept latents,
strength 1) is compared bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.util import SMALL_FLUX, SMALL_VAE, bf16_round, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu

f32 = np.float32
SCALE, SHIFT = f32(SMALL_VAE["scaling_factor"]), f32(SMALL_VAE["shift_factor"])


def _np_preprocess(u):
    return (u.astype(np.float32) + f32(0.5)) / f32(127.5) - f32(1)


def _np_scale_noise(x0, noise, t):
    t = f32(t)
    return (f32(1) - t) * x0 + t * noise


def _packed_mask(lat_mask, Cc=16):
    """latent-resolution mask (B,h,w) -> the packed (B,hw/4,4*Cc) layout, through the oracle's pack_latents"""
    from oracle import oracle as orc
    B, h, w = lat_mask.shape
    return orc.pack_latents(np.ascontiguousarray(np.broadcast_to(lat_mask[:, None], (B, Cc, h, w)), dtype=np.float32))[0]


def _offset_view(torch, a):
    """a copy of `a` on the device that starts one float past a 16-byte boundary: the kernels' scalar paths"""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == 4
    return v


# ------------------------------------------------------------------------------------------------ 1. glue
@pytest.mark.parametrize("shape", [(2, 3, 16, 24), (1, 3, 5, 7)])  # rows of four pixels / a pixel count that is no multiple of 4
def test_preprocess_u8_is_the_bin_centre_and_inverts_postprocess(shape):
    import torch
    import diffusion_rs_amd as d
    n = int(np.prod(shape))
    u = np.random.default_rng(0).permutation(np.arange(n) % 256).astype(np.uint8).reshape(shape)
    if n >= 256:
        assert len(np.unique(u)) == 256
    want = _np_preprocess(u)
    got = d.preprocess_u8(dev(u))
    np.testing.assert_array_equal(host(got), want)
    hwc = np.ascontiguousarray(u.transpose(0, 2, 3, 1))
    got_i = d.preprocess_u8(dev(hwc), interleaved=True)
    assert tuple(got_i.shape) == shape
    np.testing.assert_array_equal(host(got_i), want)
    np.testing.assert_array_equal(d.postprocess_u8(got).cpu().numpy(), u)
    np.testing.assert_array_equal(d.postprocess_u8(got_i, interleave=True).cpu().numpy(), hwc)
    # an output that is not 16-byte aligned: same values through the four scalar stores
    from diffusion_rs_amd import _lib as L
    out = _offset_view(torch, np.zeros(shape, np.float32))
    B, Cc, H, W = shape
    L.check(L.load().fmi_preprocess_u8(C.c_void_p(dev(u).data_ptr()), B, Cc, H, W, 0, C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(out), want)


def test_encode_latents_mirrors_unpack_latents():
    import torch
    import diffusion_rs_amd as d
    from diffusion_rs_amd import _lib as L
    from oracle import oracle as orc
    z = np.random.default_rng(1).standard_normal((2, 16, 8, 12)).astype(np.float32)
    want, want_ids = orc.pack_latents((z - SHIFT) * SCALE)
    x0, ids = d.encode_latents(dev(z), SMALL_VAE["scaling_factor"], SMALL_VAE["shift_factor"])
    assert tuple(x0.shape) == (2, 24, 64) and tuple(ids.shape) == (2, 24, 3)
    np.testing.assert_array_equal(host(x0), want)
    np.testing.assert_array_equal(host(ids), want_ids)
    np.testing.assert_array_equal(host(ids), host(d.pack_latents(dev(z))[1]))
    back = host(d.unpack_latents(x0, 16, 8, 12, SMALL_VAE["scaling_factor"], SMALL_VAE["shift_factor"]))
    err = float(np.abs(back - z).max())
    print(f"unpack_latents(encode_latents(z)) - z: max |d| {err:.2e} at max |z| {np.abs(z).max():.2f}")
    assert err <= 1e-6  # four f32 roundings of values below 4: 4 * 2^-24 * 4 = 9.5e-7
    # unaligned output, no img_ids
    out = _offset_view(torch, np.zeros(want.shape, np.float32))
    L.check(L.load().fmi_encode_latents(C.c_void_p(dev(z).data_ptr()), 2, 16, 8, 12, SMALL_VAE["scaling_factor"], SMALL_VAE["shift_factor"],
                                        C.c_void_p(out.data_ptr()), None, None))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(out), want)
    with pytest.raises(d.FmiError):
        d.encode_latents(dev(z[:, :, :7]), 0.3611, 0.1159)  # odd h


def test_latent_mask_is_block_mean_in_packed_layout():
    import torch
    import diffusion_rs_amd as d
    rng = np.random.default_rng(2)
    B, H, W = 2, 64, 96
    for kind in ("binary", "soft"):
        m = (rng.random((B, H, W)) < 0.5).astype(np.float32) if kind == "binary" else rng.random((B, H, W)).astype(np.float32)
        pooled = torch.nn.functional.avg_pool2d(torch.from_numpy(m)[:, None], 8)[:, 0].numpy()  # (B, H/8, W/8)
        want = _packed_mask(pooled)
        for name, src in (("aligned", dev(m)), ("offset view", _offset_view(torch, m))):
            got = host(d.latent_mask(src, 16))
            assert got.shape == (B, (H // 16) * (W // 16), 64)
            if kind == "binary":
                np.testing.assert_array_equal(got, want, err_msg=name)
            else:
                err = float(np.abs(got - want).max())
                print(f"latent_mask soft ({name}): max |d| {err:.2e}")
                assert err <= 1e-6
    with pytest.raises(ValueError):
        d.latent_mask(dev(np.zeros((1, 24, 32), np.float32)))
    from diffusion_rs_amd import _lib as L
    assert L.load().fmi_latent_mask(C.c_void_p(dev(m).data_ptr()), 1, 16, 24, 32, C.c_void_p(dev(m).data_ptr()), None) == L.ERR_INVALID


@pytest.mark.parametrize("n,offset", [(2 * 256 * 64, False), (1027, True)])  # the float4 path / the scalar path
def test_scale_noise(n, offset):
    import torch
    import diffusion_rs_amd as d
    rng = np.random.default_rng(3)
    x0, noise = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    put = (lambda a: _offset_view(torch, a)) if offset else dev
    gx, gn = put(x0), put(noise)
    t = 0.37
    got = host(d.scale_noise(gx, gn, t))
    want = (1.0 - float(f32(t))) * x0.astype(np.float64) + float(f32(t)) * noise.astype(np.float64)
    err = np.abs(got - want)
    print(f"scale_noise n={n}: max |d| {err.max():.2e}")
    assert (err <= 1e-6 + 1e-6 * np.abs(want)).all()
    np.testing.assert_array_equal(host(d.scale_noise(gx, gn, 1.0)), noise)
    np.testing.assert_array_equal(host(d.scale_noise(gx, gn, 0.0)), x0)


# ------------------------------------------------------------------------------------------------ 2. the masked loop
@pytest.fixture(scope="module")
def loop():
    """256 image + 32 text tokens, 4 steps (the precomputed-modulation path), B = 2; the oracle composition is computed once for the mixed mask."""
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    sd = d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    gm = d.FluxModel(SMALL_FLUX)
    gm.load_state_dict(sd)
    om = orc.Flux(SMALL_FLUX)
    om.load(sd)
    B, S_hw, T = 2, (16, 16), 32
    noise, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, S_hw, T, seed=21)
    x0 = np.random.default_rng(22).standard_normal(noise.shape).astype(np.float32)
    g = np.full(B, 3.5, np.float32)
    sched = d.SchedulerConfig()
    ts = sched.get_timesteps(5, sched.calculate_shift(256))[1:]  # a cut schedule: 4 steps from t < 1
    start = _np_scale_noise(x0, noise, ts[0])
    # (c)'s masks at latent resolution (32 x 32): half zeros, half ones, a two-latent-pixel ramp between them; columns for sample 0, rows for sample 1
    ramp = np.zeros(32, np.float32)
    ramp[15], ramp[16], ramp[17:] = 1 / 3, 2 / 3, 1
    mixed = _packed_mask(np.stack([np.broadcast_to(ramp[None, :], (32, 32)), np.broadcast_to(ramp[::-1, None], (32, 32))]))
    assert (mixed == 0).mean() > 0.4 and (mixed == 1).mean() > 0.4 and ((mixed > 0) & (mixed < 1)).any()
    return dict(torch=torch, d=d, gm=gm, om=om, B=B, noise=noise, x0=x0, ids=ids, txt=txt, txt_ids=txt_ids, y=y, g=g, ts=ts, start=start, mixed=mixed)


def _run(lp, sl=slice(None), **extra):
    torch = lp["torch"]
    return host(lp["gm"].denoise(dev(lp["start"][sl]), dev(lp["ids"][sl]), dev(lp["txt"][sl], torch.bfloat16), dev(lp["txt_ids"][sl]), dev(lp["y"][sl]),
                                 dev(lp["g"][sl]), lp["ts"], **{k: (None if v is None else dev(v[sl])) for k, v in extra.items()}))


def test_masked_loop_mask_of_ones_is_the_plain_loop(loop):
    plain = _run(loop)
    ones = _run(loop, x0=loop["x0"], noise=loop["noise"], mask=np.ones_like(loop["x0"]))
    assert np.isfinite(plain).all() and not np.array_equal(plain, loop["start"])
    np.testing.assert_array_equal(ones, plain)


def test_masked_loop_mask_of_zeros_returns_the_source(loop):
    zeros = _run(loop, x0=loop["x0"], noise=loop["noise"], mask=np.zeros_like(loop["x0"]))
    np.testing.assert_array_equal(zeros, loop["x0"])


def test_masked_loop_matches_oracle_composition(loop):
    om, ts, x0, noise, m, B = loop["om"], loop["ts"], loop["x0"], loop["noise"], loop["mixed"], loop["B"]
    got = _run(loop, x0=x0, noise=noise, mask=m)
    img = loop["start"].copy()
    for i in range(len(ts) - 1):  # the oracle's model evaluation, then the step of the issue in numpy f32
        pred = om.forward(img, loop["ids"], loop["txt"], loop["txt_ids"], np.full(B, f32(ts[i]), np.float32), loop["y"], loop["g"])
        e = img + pred * f32(ts[i + 1] - ts[i])
        k = _np_scale_noise(x0, noise, ts[i + 1])
        img = (m * e + (f32(1) - m) * k).astype(np.float32)
    err = rel_l2(got, img)
    print(f"masked loop, 4 steps, B=2, mixed mask: final latents rel-L2 {err:.3e} vs the oracle composition")
    assert err <= 3e-2
    assert ts[-1] == 0.0
    np.testing.assert_array_equal(got[m == 0], x0[m == 0])  # kept latents end as the source's, exactly
    assert not np.array_equal(got[m == 1], x0[m == 1])
    # Samples of a batch are independent trajectories.  The modulation precompute picks its kernel by row count (steps x batch: 8 rows -> one GEMM on
    # bf16 silu(vec); 4 rows -> f32 GEMV passes), so — as tests/test_gpu_production_shapes.py does for the plain loop — bit-identity is asked for
    # with that choice pinned, and the default choice is compared to rounding.
    from diffusion_rs_amd import _lib as L
    gm = loop["gm"]
    L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 0))
    try:
        both = _run(loop, x0=x0, noise=noise, mask=m)
        for b in range(B):
            one = _run(loop, slice(b, b + 1), x0=x0, noise=noise, mask=m)
            np.testing.assert_array_equal(one, both[b:b + 1], err_msg=f"sample {b}")
    finally:
        L.check(gm.lib.fmi_flux_set_modulation_gemm(gm.h, 1))
    print(f"masked loop: batch samples == single runs (GEMV modulation passes); one-GEMM modulation vs GEMV passes rel-L2 {rel_l2(got, both):.2e}")
    assert rel_l2(got, both) <= 2e-3  # the bar tests/test_gpu_flux.py::test_modulation_gemm_matches_gemv_passes sets for that rounding


@pytest.mark.parametrize("missing", ["x0", "noise", "mask"])
def test_masked_loop_needs_all_three(loop, missing):
    from diffusion_rs_amd import _lib as L
    extra = dict(x0=loop["x0"], noise=loop["noise"], mask=loop["mixed"])
    extra[missing] = None
    with pytest.raises(loop["d"].FmiError) as ei:
        _run(loop, **extra)
    assert ei.value.code == L.ERR_INVALID


# ------------------------------------------------------------------------------------------------ 3. the pipeline
H, W, STEPS, GUIDANCE = 128, 192, 4, 3.5


def _write_diffusers_dir(root, sd, vsd):
    """a diffusers directory as tests/test_gpu_pipeline.py writes it (vsd carries the encoder tensors or not)"""
    import torch
    from safetensors.torch import save_file
    for sub in ("transformer", "vae", "scheduler"):
        os.makedirs(os.path.join(root, sub))
    json.dump({"_class_name": "FluxPipeline"}, open(os.path.join(root, "model_index.json"), "w"))
    json.dump({"_class_name": "FlowMatchEulerDiscreteScheduler", "base_image_seq_len": 256, "base_shift": 0.5, "max_image_seq_len": 4096,
               "max_shift": 1.15, "shift": 3.0, "use_dynamic_shifting": True}, open(os.path.join(root, "scheduler", "scheduler_config.json"), "w"))
    json.dump({k: SMALL_FLUX[k] for k in ("in_channels", "pooled_projection_dim", "joint_attention_dim", "num_attention_heads", "num_layers",
                                          "num_single_layers", "guidance_embeds")}, open(os.path.join(root, "transformer", "config.json"), "w"))
    json.dump({k: SMALL_VAE[k] for k in SMALL_VAE}, open(os.path.join(root, "vae", "config.json"), "w"))
    names = list(sd)
    half = len(names) // 2
    save_file({k: torch.from_numpy(sd[k]).to(torch.bfloat16) for k in names[:half]}, os.path.join(root, "transformer", "diffusion_pytorch_model-00001-of-00002.safetensors"))
    save_file({k: torch.from_numpy(sd[k]).to(torch.bfloat16) for k in names[half:]}, os.path.join(root, "transformer", "diffusion_pytorch_model-00002-of-00002.safetensors"))
    save_file({k: torch.from_numpy(v) for k, v in vsd.items()}, os.path.join(root, "vae", "diffusion_pytorch_model.safetensors"))


@pytest.fixture(scope="module")
def pipe_env(tmp_path_factory):
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    sd = d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    vsd = d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0, encoder=True)
    root = str(tmp_path_factory.mktemp("img2img") / "tiny-flux")
    _write_diffusers_dir(root, sd, vsd)
    pipe = d.Pipeline(d.ModelSource.ModelId(root))
    om, ov = orc.Flux(SMALL_FLUX), orc.Vae(SMALL_VAE)
    om.load(sd)
    ov.load(vsd)
    B, T = 2, 24
    rng = np.random.default_rng(31)
    t5 = bf16_round(rng.standard_normal((B, T, SMALL_FLUX["joint_attention_dim"])).astype(np.float32))
    clip = rng.standard_normal((B, SMALL_FLUX["pooled_projection_dim"])).astype(np.float32)
    lat = rng.standard_normal((B, 16, H // 8, W // 8)).astype(np.float32)
    # a source with structure (what an encoder is for), as the u8 HWC arrays output="rgb" returns
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([127.5 + 100 * np.sin(xx / 17.0 + b) * np.cos(yy / 11.0 + c) for b in range(B) for c in range(3)]).reshape(B, 3, H, W)
    src_u8 = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1).copy()
    params = d.DiffusionGenerationParams(height=H, width=W, num_steps=STEPS, guidance_scale=GUIDANCE)
    sched = pipe.scheduler
    mu = orc.calculate_shift((H // 16) * (W // 16), sched.base_image_seq_len, sched.max_image_seq_len, sched.base_shift, sched.max_shift)
    ts = orc.get_timesteps(STEPS, sched.use_dynamic_shifting, mu, sched.shift)
    # the oracle's source latents: preprocess (numpy) -> Vae.encode (posterior mean) -> affine -> pack
    src_f32 = _np_preprocess(src_u8.transpose(0, 3, 1, 2))
    x0_ref, ids = orc.pack_latents(((ov.encode(src_f32, noise=None) - SHIFT) * SCALE).astype(np.float32))
    noise = orc.pack_latents(lat)[0]
    kw = dict(embeddings=(dev(t5, torch.bfloat16), dev(clip)), latents=dev(lat))
    return dict(torch=torch, d=d, orc=orc, pipe=pipe, om=om, ov=ov, sd=sd, B=B, T=T, t5=t5, clip=clip, lat=lat, src_u8=src_u8, src_f32=src_f32, params=params,
                ts=ts, x0_ref=x0_ref, ids=ids, noise=noise, kw=kw, g=np.full(B, GUIDANCE, np.float32), txt_ids=np.zeros((B, T, 3), np.float32))


def _oracle_decode(env, img):
    orc = env["orc"]
    z = orc.unpack_latents(img, 16, H // 8, W // 8) * f32(1.0 / SMALL_VAE["scaling_factor"]) + SHIFT
    return orc.postprocess_u8(env["ov"].decode(z.astype(np.float32)))


def _u8_share(got_u8, ref_u8):
    diff = np.abs(got_u8.cpu().numpy().astype(np.int32) - ref_u8.astype(np.int32))
    return float((diff <= 2).mean()), int(diff.max())


def test_pipeline_strength_one_is_text_to_image(pipe_env):
    pipe, params, kw = pipe_env["pipe"], pipe_env["params"], pipe_env["kw"]
    plain = pipe.forward(["a", "b"], params, output="tensor", **kw)
    with_image = pipe.forward(["a", "b"], params, output="tensor", image=pipe_env["src_u8"], strength=1.0, **kw)
    assert pipe_env["torch"].equal(plain, with_image)
    seeded = pipe.forward(["a", "b"], params, output="tensor", embeddings=kw["embeddings"], seed=9)
    seeded_image = pipe.forward(["a", "b"], params, output="tensor", embeddings=kw["embeddings"], seed=9, image=pipe_env["src_u8"])
    assert pipe_env["torch"].equal(seeded, seeded_image)


def test_pipeline_img2img_matches_oracle_pipeline(pipe_env):
    env = pipe_env
    pipe, om, ts = env["pipe"], env["om"], env["ts"]
    u8, final = pipe.forward(["a", "b"], env["params"], output="tensor", image=env["src_u8"], strength=0.5, return_latents=True, **env["kw"])
    assert tuple(final.shape) == (env["B"], (H // 16) * (W // 16), 64) and final.dtype == env["torch"].float32
    assert list(ts[2:]) == env["d"].img2img_timesteps(list(ts), 0.5)
    start = _np_scale_noise(env["x0_ref"], env["noise"], ts[2])
    ref = om.denoise(start, env["ids"], env["t5"], env["txt_ids"], env["clip"], env["g"], ts[2:])
    err = rel_l2(host(final), ref)
    share, worst = _u8_share(u8, _oracle_decode(env, ref))
    print(f"img2img strength 0.5 ({len(ts) - 3} of {STEPS} steps): final latents rel-L2 {err:.3e}; u8 within 2 on {share:.4f}, max |d| {worst}")
    assert err <= 3e-2
    assert share >= 0.99
    # the f32 (B,3,H,W) form of the same source gives the same image
    u8_f = pipe.forward(["a", "b"], env["params"], output="tensor", image=dev(env["src_f32"]), strength=0.5, **env["kw"])
    assert env["torch"].equal(u8, u8_f)


def test_pipeline_inpaint_matches_oracle_composition(pipe_env):
    env = pipe_env
    pipe, om, ts, d, B = env["pipe"], env["om"], env["ts"], env["d"], env["B"]
    mask = np.zeros((B, H, W), bool)  # edges on 8-pixel boundaries (and not all on 16-pixel ones: tokens with kept and repainted latents)
    mask[0, 24:88, 40:136] = True
    mask[1, :, 96:] = True
    u8, final = pipe.forward(["a", "b"], env["params"], output="tensor", image=env["src_u8"], strength=0.75, mask=mask, return_latents=True, **env["kw"])
    lat_m = mask.reshape(B, H // 8, 8, W // 8, 8).mean((2, 4)).astype(np.float32)
    assert set(np.unique(lat_m)) == {0.0, 1.0}
    m = _packed_mask(lat_m)
    x0, noise = env["x0_ref"], env["noise"]
    cut = list(ts[1:])  # int(4 * 0.75) = 3 steps
    img = _np_scale_noise(x0, noise, cut[0])
    for i in range(len(cut) - 1):
        pred = om.forward(img, env["ids"], env["t5"], env["txt_ids"], np.full(B, f32(cut[i]), np.float32), env["clip"], env["g"])
        e = img + pred * f32(cut[i + 1] - cut[i])
        k = _np_scale_noise(x0, noise, cut[i + 1])
        img = (m * e + (f32(1) - m) * k).astype(np.float32)
    got = host(final)
    err = rel_l2(got, img)
    share, worst = _u8_share(u8, _oracle_decode(env, img))
    print(f"inpaint strength 0.75 (3 steps), {m.mean():.2f} of the latents repainted: final latents rel-L2 {err:.3e}; u8 within 2 on {share:.4f}, max |d| {worst}")
    assert err <= 3e-2
    assert share >= 0.99
    # kept latents are the GPU's own source latents, bit for bit
    gx0, _ = d.encode_latents(pipe.vae.encode(d.preprocess_u8(dev(env["src_u8"]), interleaved=True)), pipe.vae.scale_factor(), pipe.vae.shift_factor())
    np.testing.assert_array_equal(got[m == 0], host(gx0)[m == 0])
    assert not np.array_equal(got[m == 1], host(gx0)[m == 1])
    # a float mask in [0,1] of the same values is the same request
    u8_f = pipe.forward(["a", "b"], env["params"], output="tensor", image=env["src_u8"], strength=0.75, mask=dev(mask.astype(np.float32)), **env["kw"])
    assert env["torch"].equal(u8, u8_f)


def test_pipeline_single_image_broadcasts_over_the_prompts(pipe_env):
    env = pipe_env
    pipe = env["pipe"]
    one, mask1 = env["src_u8"][0], np.zeros((H, W), np.float32)
    mask1[:, :64] = 1
    bcast = pipe.forward(["a", "b"], env["params"], output="tensor", image=one, strength=0.75, mask=mask1, **env["kw"])
    explicit = pipe.forward(["a", "b"], env["params"], output="tensor", image=np.stack([one, one]), strength=0.75, mask=np.stack([mask1, mask1]), **env["kw"])
    assert env["torch"].equal(bcast, explicit)
    assert not env["torch"].equal(bcast[0], bcast[1])  # two prompts, two noises


def test_pipeline_rejects_bad_img2img_arguments(pipe_env):
    env = pipe_env
    pipe, params, kw, d = env["pipe"], env["params"], env["kw"], env["d"]
    src, go = env["src_u8"], lambda **k: pipe.forward(["a", "b"], k.pop("params", params), output="tensor", **dict(kw, **k))
    with pytest.raises(ValueError, match="multiples of 16"):
        go(params=d.DiffusionGenerationParams(height=72, width=64, num_steps=4, guidance_scale=3.5), image=np.zeros((72, 64, 3), np.uint8),
           latents=None, seed=1)
    with pytest.raises(ValueError, match="as params say"):
        go(image=src[:, :64])  # another size
    with pytest.raises(ValueError, match="as params say"):
        go(image=dev(np.zeros((2, 3, H, W + 16), np.float32)))
    with pytest.raises(ValueError, match="as params say"):
        go(image=src, mask=np.ones((H, W // 2), np.float32))
    with pytest.raises(ValueError, match="samples for"):
        go(image=np.concatenate([src, src[:1]]))  # three images for two prompts
    with pytest.raises(ValueError, match="mask= needs image="):
        go(mask=np.ones((H, W), np.float32))
    with pytest.raises(ValueError, match="strength= needs image="):
        go(strength=0.5)
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="strength must be in"):
            go(image=src, strength=bad)
    with pytest.raises(ValueError, match="no step"):
        go(image=src, strength=0.2)  # int(4 * 0.2) == 0
    pipe._sp = object()  # what enable_sequence_parallel leaves behind (its wiring needs a second device)
    try:
        with pytest.raises(ValueError, match="sequence parallel"):
            go(image=src, strength=0.5)
    finally:
        pipe._sp = None
    assert go().shape == (2, 3, H, W)  # the pipeline is as it was


def test_pipeline_decoder_only_vae_cannot_start_from_an_image(pipe_env, tmp_path):
    env = pipe_env
    d = env["d"]
    root = str(tmp_path / "tiny-flux-decoder-only")
    _write_diffusers_dir(root, env["sd"], d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0))
    pipe = d.Pipeline(d.ModelSource.ModelId(root))
    params = d.DiffusionGenerationParams(height=64, width=64, num_steps=2, guidance_scale=3.5)
    t5, clip = env["kw"]["embeddings"]
    kw = dict(embeddings=(t5[:1], clip[:1]), seed=3, output="tensor")
    assert pipe.forward(["a"], params, **kw).shape == (1, 3, 64, 64)
    with pytest.raises(d.FmiError, match="encoder"):
        pipe.forward(["a"], params, image=np.zeros((64, 64, 3), np.uint8), strength=0.5, **kw)
