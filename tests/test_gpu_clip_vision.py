"""CLIP vision encoder on the GPU against tests/clip_vision_ref.py, the CPU restatement that tests/test_host_clip_vision.py pins to PIL and
to HuggingFace transformers: the bicubic resize and the preprocess as values, the tower at the project's encoder bar (rel-L2 <= 1e-2, tests/test_gpu_text.py:
bf16 operands, f32 accumulate, f32 residual stream), and ip_adapter_image= through the pipeline as the embedding it becomes."""
import time

import numpy as np
import pytest

from tests import clip_vision_ref as R
from tests import ip_adapter_ref as IR
from tests.util import SMALL_VAE, dev, host, rel_l2

pytestmark = pytest.mark.gpu

ENCODER_BAR = 1e-2  # tests/test_gpu_text.py
REAL_CASE = ((301, 517), (224, 384), "noise")  # a real size: what CLIP's rule makes of a 301 x 517 picture at image_size 224


def _model(name, layers=None):
    import diffusion_rs_amd as d
    cfg = dict(R.CONFIGS[name]) if layers is None else dict(R.CONFIGS[name], num_hidden_layers=layers)
    m = d.ClipVisionModel(cfg)
    m.load_state_dict(R.state_dict(cfg))
    return m, cfg


@pytest.fixture(scope="module")
def resizer():
    m, _ = _model("s56p14", layers=1)  # (resize and preprocess are the model's methods; its weights play no part)
    yield m
    m.close()


def _distance(got, want):
    diff = np.abs(got.astype(int) - want.astype(int))
    return int(diff.max()), float((diff > 0).mean())


@pytest.mark.parametrize("case", list(R.RESIZE_CASES) + ["real"])
def test_resize_against_the_recipe_and_pil(resizer, case):
    """fmi_resize_bicubic_u8 against the CPU recipe (float32) and, on the committed pictures, against PIL itself: every value within 1, at most 2e-3 of them
    different; rows past the output keep their canary; a second run gives the same bits."""
    import torch
    (h, w), (nh, nw), kind = REAL_CASE if case == "real" else R.RESIZE_CASES[case]
    src = R.picture((h, w), kind, seed=100 + (len(R.RESIZE_CASES) if case == "real" else list(R.RESIZE_CASES).index(case)))
    lib, rows = resizer.lib, nh + 3
    buf = torch.full((rows, nw, 3), 77, dtype=torch.uint8, device="cuda")  # the output and three canary rows behind it
    t = dev(src)
    from diffusion_rs_amd import _lib as L
    from diffusion_rs_amd.flux import _ptr, _stream
    L.check(lib.fmi_resize_bicubic_u8(_ptr(t), h, w, _ptr(buf), nh, nw, _stream()), lib)
    got = buf.cpu().numpy()
    assert (got[nh:] == 77).all()
    got = got[:nh]
    again = resizer.resize(src, nh, nw).cpu().numpy()
    assert np.array_equal(again, got)
    mx, share = _distance(got, R.resize_bicubic_u8(src, nh, nw, np.float32))
    print(f"resize {case} {h}x{w} -> {nh}x{nw}: vs recipe max {mx}, share {share:.2e}")
    assert mx <= 1 and share <= 2e-3
    if case != "real":
        z = np.load(R.GOLDEN)
        assert np.array_equal(z[f"resize_in/{case}"], src)
        mx, share = _distance(got, z[f"resize_out/{case}"])
        print(f"resize {case}: vs PIL max {mx}, share {share:.2e}")
        assert mx <= 1 and share <= 2e-3
    if case == "noop":
        assert np.array_equal(got, src)


def test_resize_and_preprocess_refuse_bad_sizes_by_name(resizer):
    import torch
    import diffusion_rs_amd as d
    from diffusion_rs_amd import _lib as L
    from diffusion_rs_amd.flux import _ptr, _stream
    lib = resizer.lib
    a, b = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda"), torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    for h, w, nh, nw in ((0, 8, 8, 8), (8, -1, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0)):
        with pytest.raises(d.FmiError, match="h, w, nh, nw must be positive"):
            L.check(lib.fmi_resize_bicubic_u8(_ptr(a), h, w, _ptr(b), nh, nw, _stream()), lib)
    out = torch.zeros((3, 8, 8), dtype=torch.float32, device="cuda")
    mean, std = (L.C.c_float * 3)(*R.CLIP_MEAN), (L.C.c_float * 3)(*R.CLIP_STD)
    for nh, nw in ((7, 8), (8, 7)):
        with pytest.raises(d.FmiError, match="nh and nw must be at least S = 8"):
            L.check(lib.fmi_clip_preprocess_u8(_ptr(a), nh, nw, 8, mean, std, _ptr(out), _stream()), lib)
    with pytest.raises(ValueError, match="must be uint8"):
        resizer.preprocess(np.zeros((8, 8, 3), np.float32))


@pytest.mark.parametrize("shape", [(67, 45), (31, 45), (56, 56), (9, 13)])
def test_preprocess_is_the_reference(resizer, shape):
    """Resize to the shortest edge 56, centre crop, (v / 255 - mean) / std: equal to the reference AS VALUES wherever the resized pictures agree — the three f32
    operations are IEEE division, subtraction, division, none of them contractible — and the kernel alone, on the reference's own resized picture, everywhere."""
    import torch
    from diffusion_rs_amd import _lib as L
    from diffusion_rs_amd.flux import _ptr, _stream
    S = resizer.cfg["image_size"]
    src = R.picture(shape, seed=7)
    nh, nw = R.resize_shape(shape[0], shape[1], S)
    resized = R.resize_bicubic_u8(src, nh, nw)
    out = torch.empty((3, S, S), dtype=torch.float32, device="cuda")
    mean, std = (L.C.c_float * 3)(0.5, 0.25, 0.125), (L.C.c_float * 3)(0.3, 0.2, 0.7)
    L.check(resizer.lib.fmi_clip_preprocess_u8(_ptr(dev(resized)), nh, nw, S, mean, std, _ptr(out), _stream()), resizer.lib)
    assert np.array_equal(out.cpu().numpy(), R.preprocess(resized, S, (0.5, 0.25, 0.125), (0.3, 0.2, 0.7)))
    got = resizer.preprocess(src)
    assert tuple(got.shape) == (1, 3, S, S) and got.dtype == torch.float32
    want = R.image_processor(src, S)
    gpu_resized = resizer.resize(src, nh, nw).cpu().numpy()
    top, left = (nh - S) // 2, (nw - S) // 2
    same = (gpu_resized == resized)[top:top + S, left:left + S].transpose(2, 0, 1)[None]
    print(f"preprocess {shape}: {float(same.mean()):.4f} of the cropped values come from equal resized values")
    assert same.any() and np.array_equal(got.cpu().numpy()[same], want[same])
    assert np.array_equal(got.cpu().numpy(), R.preprocess(gpu_resized, S)[None])


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_tower_against_the_reference(name):
    """image_embeds and the hidden output against clip_vision_ref (f32) on bf16-valued weights, B = 3 and B = 1 (B T is then no multiple of 4 rows per block);
    a batch's embeddings are its samples' bit for bit; the class row of the returned hidden output is what the embeddings were made of."""
    m, cfg = _model(name)
    sd = R.state_dict(cfg)
    want_e, want_h = R.reference(name, 3)
    pix = R.pixel_values(cfg, 3)
    got_e, got_h = m.forward(pix, return_hidden=True)
    got_e, got_h = host(got_e), host(got_h)
    T = 1 + (cfg["image_size"] // cfg["patch_size"]) ** 2
    assert got_e.shape == (3, cfg["projection_dim"]) and got_h.shape == (3, T, cfg["hidden_size"]) and np.isfinite(got_e).all() and np.isfinite(got_h).all()
    print(f"tower {name} B=3 T={T}: image_embeds rel-L2 {rel_l2(got_e, want_e):.3e}, hidden {rel_l2(got_h, want_h):.3e}")
    assert rel_l2(got_e, want_e) <= ENCODER_BAR and rel_l2(got_h, want_h) <= ENCODER_BAR
    for b in range(3):
        one_e, one_h = m.forward(pix[b:b + 1], return_hidden=True)
        assert np.array_equal(host(one_e)[0], got_e[b]) and np.array_equal(host(one_h)[0], got_h[b])
        assert rel_l2(host(one_e), want_e[b:b + 1]) <= ENCODER_BAR
    assert np.array_equal(host(m.forward(pix)), got_e)  # without the hidden output: the same embeddings
    tail = R.tail(sd, got_h)
    print(f"tower {name}: image_embeds vs the host tail of the returned hidden {rel_l2(got_e, tail):.3e}")
    assert rel_l2(got_e, tail) <= 1e-2
    m.close()


def test_refusals_by_name():
    import diffusion_rs_amd as d
    cfg = R.CONFIGS["s56p14"]
    with pytest.raises(d.FmiError, match="head dim .* must be 64"):
        d.ClipVisionModel(dict(cfg, num_attention_heads=4))
    with pytest.raises(d.FmiError, match="multiples of 64"):
        d.ClipVisionModel(dict(cfg, projection_dim=48))
    with pytest.raises(d.FmiError, match="multiple of patch_size"):
        d.ClipVisionModel(dict(cfg, image_size=57))
    with pytest.raises(d.FmiError, match="1025 tokens .* are more than the encoder attention's 1024"):
        d.ClipVisionModel(dict(cfg, image_size=448, patch_size=14))
    d.ClipVisionModel(dict(cfg, image_size=434, patch_size=14, num_hidden_layers=1)).close()  # 962 tokens: accepted
    half = d.ClipVisionModel(dict(cfg, num_hidden_layers=1))
    with pytest.raises(d.FmiError, match="tensors not set, first: vision_model"):
        half.forward(R.pixel_values(cfg, 1))
    with pytest.raises(d.FmiError, match="shape mismatch for vision_model.embeddings.patch_embedding.weight .*128,3,14,14"):
        half.set_tensor("vision_model.embeddings.patch_embedding.weight", np.zeros((128, 588), np.float32))
    with pytest.raises(d.FmiError, match="unknown tensor name"):
        half.set_tensor("vision_model.pre_layernorm.weight", np.zeros(128, np.float32))
    half.close()
    m, _ = _model("s56p14", layers=1)
    for bad in (np.zeros((1, 3, 56, 42), np.float32), np.zeros((3, 56, 56), np.float32), np.zeros((1, 1, 56, 56), np.float32), np.zeros((1, 3, 64, 64), np.float32)):
        with pytest.raises(ValueError, match="pixel_values must be float \\(B,3,56,56\\)"):
            m.forward(bad)
    with pytest.raises(ValueError, match="pixel_values must be float"):
        m.forward(np.zeros((1, 3, 56, 56), np.uint8))
    m.close()


def test_real_config_runs_and_is_deterministic():
    """openai/clip-vit-large-patch14's tower (24 x 1024, 257 tokens) on random weights: finite, the same bits twice, and what one encode of a picture costs."""
    import torch
    import diffusion_rs_amd as d
    m = d.ClipVisionModel()
    d.synth.fill_text_random_device(m, seed=4)
    assert m.missing() == []
    pic = R.picture((301, 517), seed=9)
    a = m.encode(pic)
    b = m.encode(pic)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (1, 768) and a.dtype == torch.float32 and torch.isfinite(a).all() and torch.equal(a, b)
    pv = m.preprocess(pic)
    e, h = m.forward(pv, return_hidden=True)
    assert tuple(h.shape) == (1, 257, 1024) and torch.isfinite(h).all() and torch.equal(e, a)
    t0 = time.perf_counter()
    m.encode(pic)
    torch.cuda.synchronize()
    print(f"CLIP ViT-L/14 vision tower, one encode of a 301 x 517 picture: {(time.perf_counter() - t0) * 1e3:.1f} ms, resident {m.size_in_bytes() / 2**20:.0f} MiB")
    m.close()


def test_pipeline_takes_a_picture_as_the_embedding_it_becomes():
    """forward(ip_adapter_image=) == forward(ip_adapter_image_embeds=encode_image(.)) bit for bit, for a u8 picture of odd size and for pixel_values, on either
    side of a negative prompt; a request without the new keywords does not see the encoder; unloading it refuses the picture."""
    import torch
    import diffusion_rs_amd as d
    name = "s56p14"
    cfg = R.CONFIGS[name]
    E = cfg["projection_dim"]
    Hp, Wp = 64, 96
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=IR.MAIN_CFG, vae_cfg=SMALL_VAE))
    pipe.flux.load_state_dict(IR.main_state_dict())
    pipe.vae.load_state_dict(d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0, encoder=True))
    params = d.DiffusionGenerationParams(height=Hp, width=Wp, num_steps=4, guidance_scale=3.5)
    s = IR.inputs("aligned")
    t5, clip = dev(s["txt"], torch.bfloat16), dev(s["y"])
    lat = (np.random.default_rng(11).standard_normal((2, 16, Hp // 8, Wp // 8)) * IR.IMG_MULT).astype(np.float32)
    fwd = lambda **kw: pipe.forward(["a", "b"], params, output="tensor", embeddings=(t5, clip), latents=dev(lat), return_latents=True, **kw)
    plain_before = fwd()
    pipe.load_ip_adapter(d.synth.ip_adapter_state_dict_numpy(IR.MAIN_CFG, E, IR.N, seed=5, proj_std=IR.PROJ_STD, k_std=IR.K_STD, v_std=IR.V_STD))
    pic, npic = R.picture((67, 45), seed=21), R.picture((31, 53), seed=22)
    with pytest.raises(ValueError, match="load_image_encoder"):
        fwd(ip_adapter_image=pic)
    with pytest.raises(ValueError, match="load_image_encoder"):
        pipe.encode_image(pic)
    enc = pipe.load_image_encoder((cfg, R.state_dict(cfg)))
    assert pipe.image_encoder is enc and enc.projection_dim == E
    emb = pipe.encode_image(pic)
    assert tuple(emb.shape) == (1, E) and emb.dtype == torch.float32 and emb.is_cuda
    S = cfg["image_size"]
    resized = enc.resize(pic, *R.resize_shape(67, 45, S)).cpu().numpy()  # (the tower's bar is for the tower: the reference starts from the same resized picture)
    want = R.vision_forward(R.state_dict(cfg), cfg, R.preprocess(resized, S)[None])[0]
    print(f"encode_image of a 67 x 45 picture vs the CPU reference: rel-L2 {rel_l2(host(emb), want):.3e}")
    assert rel_l2(host(emb), want) <= ENCODER_BAR
    equal = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    by_embeds = fwd(ip_adapter_image_embeds=emb, ip_adapter_scale=IR.IP_SCALE)
    assert equal(fwd(ip_adapter_image=pic, ip_adapter_scale=IR.IP_SCALE), by_embeds)
    assert equal(fwd(ip_adapter_image=torch.from_numpy(pic).cuda(), ip_adapter_scale=IR.IP_SCALE), by_embeds)
    assert not equal(by_embeds, plain_before)
    pv = enc.preprocess(pic)
    assert torch.equal(pipe.encode_image(pv), emb) and torch.equal(pipe.encode_image(pv.cpu().numpy()), emb)
    assert equal(fwd(ip_adapter_image=pv, ip_adapter_scale=IR.IP_SCALE), by_embeds)
    # under a negative prompt: the negative picture is the negative embedding
    neg = (dev(s["ntxt"][:1], torch.bfloat16), dev(s["ny"][:1]))
    nemb = pipe.encode_image(npic)
    cfg_kw = dict(negative_embeddings=neg, true_cfg_scale=2.0, ip_adapter_scale=IR.IP_SCALE)
    by_embeds = fwd(ip_adapter_image_embeds=emb, negative_ip_adapter_image_embeds=nemb, **cfg_kw)
    assert equal(fwd(ip_adapter_image=pic, negative_ip_adapter_image=npic, **cfg_kw), by_embeds)
    assert equal(fwd(ip_adapter_image_embeds=emb, negative_ip_adapter_image=npic, **cfg_kw), by_embeds)
    assert not equal(fwd(ip_adapter_image=pic, **cfg_kw), by_embeds)  # (without it the negative half attends to zero embeddings)
    # a request without the new keywords: what it was on a pipeline with no encoder (and no adapter) loaded
    assert equal(fwd(), plain_before)
    for kw, msg in ((dict(ip_adapter_image=pic, ip_adapter_image_embeds=emb), "exclude one another"), (dict(ip_adapter_image=pic, negative_ip_adapter_image=npic), "negative prompt"),
                    (dict(ip_adapter_image=pic, reference=np.zeros((Hp, Wp, 3), np.uint8)), "reference="), (dict(ip_adapter_image=pic, cache_threshold=0.1), "step cache"),
                    (dict(ip_adapter_image=np.zeros((1, 3, 64, 64), np.float32)), "ip_adapter_image must be")):
        with pytest.raises(ValueError, match=msg):
            fwd(**kw)
    wide = pipe.load_image_encoder((dict(cfg, projection_dim=128), R.state_dict(dict(cfg, projection_dim=128))))  # it replaces the loaded one
    assert pipe.image_encoder is wide and enc.h is None
    with pytest.raises(ValueError, match="projection_dim is 128, the IP-Adapter's embed_dim 64"):
        fwd(ip_adapter_image=pic)
    pipe.unload_image_encoder()
    assert pipe.image_encoder is None
    with pytest.raises(ValueError, match="load_image_encoder"):
        fwd(ip_adapter_image=pic)
    assert equal(fwd(ip_adapter_image_embeds=emb, negative_ip_adapter_image_embeds=nemb, **cfg_kw), by_embeds)  # the embedding route needs no encoder
