"""FLUX.1 Redux on the GPU against tests/redux_ref.py, the CPU restatement that tests/test_host_redux.py pins to HuggingFace transformers and to
PIL: the SigLIP tower at the project's encoder bar (rel-L2 <= 1e-2, tests/test_gpu_text.py: bf16 operands, f32 accumulate, f32 residual stream) with its heads
padded to 128 in the weights, the Redux embedder, the direct-to-square resize, and redux_image= through the pipeline as the text rows it becomes."""
import time

import numpy as np
import pytest

from tests import redux_ref as R
from tests.util import SMALL_FLUX, SMALL_VAE, dev, host, rel_l2

pytestmark = pytest.mark.gpu

ENCODER_BAR = 1e-2  # tests/test_gpu_text.py
FLUX_CFG = dict(SMALL_FLUX, joint_attention_dim=R.REDUX_J)  # the embedder's txt_in_features is the transformer's joint_attention_dim
TOWER = "h72_t16"  # the tower of the pipeline tests: head dim 72, 16 image tokens


def _model(name, layers=None):
    import diffusion_rs_amd as d
    cfg = dict(R.CONFIGS[name]) if layers is None else dict(R.CONFIGS[name], num_hidden_layers=layers)
    m = d.SiglipVisionModel(cfg)
    m.load_state_dict(R.state_dict(cfg))
    return m, cfg


def _embedder(D):
    import diffusion_rs_amd as d
    e = d.ReduxImageEmbedder(D, R.REDUX_J)
    e.load_state_dict(R.redux_state_dict(D))
    return e


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_tower_against_the_reference(name):
    """last_hidden_state against redux_ref (f32) on bf16-valued weights, B = 2 and B = 1; a batch's rows are its samples' bit for bit."""
    m, cfg = _model(name)
    want = R.reference(name, 2)
    pix = R.pixel_values(cfg, 2)
    got = host(m.forward(pix))
    assert got.shape == (2, R.num_patches(cfg), cfg["hidden_size"]) and np.isfinite(got).all()
    print(f"tower {name} B=2 Np={R.num_patches(cfg)}: last_hidden_state rel-L2 {rel_l2(got, want):.3e}")
    assert rel_l2(got, want) <= ENCODER_BAR
    for b in range(2):
        one = host(m.forward(pix[b:b + 1]))
        print(f"tower {name} B=1 sample {b}: rel-L2 {rel_l2(one, want[b:b + 1]):.3e}")
        assert rel_l2(one, want[b:b + 1]) <= ENCODER_BAR and np.array_equal(one[0], got[b])
    import torch
    assert rel_l2(host(m.forward(pix, dtype=torch.bfloat16)), got) <= 4e-3  # (one bf16 rounding of the same rows: 2^-9 per value at the most)
    m.close()


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_pad_lanes_are_inert(name):
    """The head lanes [hd, 128), the MLP columns [F, Fp), the patch columns [3 P^2, Kpad) and V^T's key tail are zero by the weights or are written before they
    are read: with every byte of the workspace 0xff (NaNs in bf16 and f32) before the call, the output is finite and the bits of a clean run."""
    m, cfg = _model(name)
    pix = R.pixel_values(cfg, 2)
    clean = host(m.forward(pix))
    m.poison_workspace(2)
    got = host(m.forward(pix))
    assert np.isfinite(got).all() and np.array_equal(got, clean)
    m.poison_workspace(2)
    assert np.array_equal(host(m.forward(pix[:1]))[0], clean[0])  # a smaller batch in the larger, poisoned workspace
    m.close()


@pytest.mark.parametrize("name", ["h72_t81", "h64_t16"])
def test_embedder_against_the_reference(name):
    """scale * redux_down(silu(redux_up(h))) on the reference's own hidden states (81 rows of 576, 16 rows of 128) at scale 1 and 0.5, f32 and bf16 out.  A scale
    of 0.5 is exact in both formats, so its result is 0.5 x the scale-1 result bit for bit."""
    import torch
    cfg = R.CONFIGS[name]
    e = _embedder(cfg["hidden_size"])
    rsd = R.redux_state_dict(cfg["hidden_size"])
    hidden = np.array(R.reference(name, 1))
    one = e.forward(hidden)
    assert tuple(one.shape) == (1, R.num_patches(cfg), R.REDUX_J) and one.dtype == torch.float32 and torch.isfinite(one).all()
    for scale in (1.0, 0.5):
        got = e.forward(hidden, scale)
        err = rel_l2(host(got), R.redux_forward(rsd, hidden, scale))
        print(f"embedder on {name} scale {scale}: rel-L2 {err:.3e}")
        assert err <= ENCODER_BAR
        assert torch.equal(got, one * scale)
        gb = e.forward(hidden, scale, dtype=torch.bfloat16)
        assert gb.dtype == torch.bfloat16 and torch.equal(gb, (one * scale).to(torch.bfloat16))
    assert torch.equal(e.forward(hidden[0]), one[0]) and not torch.count_nonzero(e.forward(hidden, 0.0))
    print(f"embedder D = {cfg['hidden_size']}, J = {R.REDUX_J}: resident {e.size_in_bytes() / 2**20:.1f} MiB")
    e.close()


@pytest.mark.parametrize("case", list(R.RESIZE_CASES))
def test_direct_to_square_resize(case):
    """fmi_resize_bicubic_u8 straight to S x S (what SiglipVisionModel.preprocess calls) against the CPU recipe and against PIL's committed output: every value
    within 1, at most 2e-3 of them different; and the pixel_values are the recipe's normalisation of the GPU's own resized picture."""
    m, cfg = _model("h64_t16", layers=1)
    shape, kind, seed = R.RESIZE_CASES[case]
    src = R.picture(shape, kind, seed=seed)
    S = R.RESIZE_S
    got = m.resize(src, S, S).cpu().numpy()
    z = np.load(R.GOLDEN)
    assert np.array_equal(z[f"resize_in/{case}"], src)
    for what, want in (("recipe", R.resize_bicubic_u8(src, S, S)), ("PIL", z[f"resize_out/{case}"])):
        diff = np.abs(got.astype(int) - want.astype(int))
        print(f"resize {case} {shape} -> {S} x {S} vs {what}: max {int(diff.max())}, share {float((diff > 0).mean()):.2e}")
        assert diff.max() <= 1 and (diff > 0).mean() <= 2e-3
    S = cfg["image_size"]
    pv = m.preprocess(src).cpu().numpy()
    mine = m.resize(src, S, S).cpu().numpy().astype(np.float32).transpose(2, 0, 1)
    assert pv.shape == (1, 3, S, S) and np.array_equal(pv[0], (mine / np.float32(255) - np.float32(0.5)) / np.float32(0.5))
    m.close()


def test_refusals_by_name():
    import diffusion_rs_amd as d
    cfg = R.CONFIGS["h64_t16"]
    for bad, msg in ((dict(cfg, num_attention_heads=32), "head dim .* must be a multiple of 8 up to 128, got 4"), (dict(cfg, hidden_size=96, num_attention_heads=2), "multiple of 64"),
                     (dict(cfg, hidden_size=256, num_attention_heads=1), "up to 128, got 256"), (dict(cfg, intermediate_size=0), "intermediate_size must be positive"),
                     (dict(cfg, image_size=15), "image_size in patch_size"), (dict(cfg, layer_norm_eps=0.0), "layer_norm_eps")):
        with pytest.raises(d.FmiError, match=msg):
            d.SiglipVisionModel(bad)
    half = d.SiglipVisionModel(dict(cfg, num_hidden_layers=1))
    with pytest.raises(d.FmiError, match="tensors not set, first: vision_model"):
        half.forward(R.pixel_values(cfg, 1))
    with pytest.raises(d.FmiError, match=r"shape mismatch for vision_model.encoder.layers.0.self_attn.q_proj.weight \(expected \(128,128\)\)"):
        half.set_tensor("vision_model.encoder.layers.0.self_attn.q_proj.weight", np.zeros((256, 128), np.float32))
    with pytest.raises(d.FmiError, match="unknown tensor name"):
        half.set_tensor("vision_model.head.probe", np.zeros((1, 1, 128), np.float32))
    with pytest.raises(ValueError, match=r"pixel_values must be float \(B,3,64,64\)"):
        half.forward(np.zeros((1, 3, 64, 48), np.float32))
    half.close()
    with pytest.raises(d.FmiError, match="multiples of 64"):
        d.ReduxImageEmbedder(100, 256)
    e = d.ReduxImageEmbedder(128, 256)
    with pytest.raises(d.FmiError, match="tensors not set, first: redux_"):
        e.forward(np.zeros((4, 128), np.float32))
    with pytest.raises(ValueError, match=r"hidden must be float \(.., 128\)"):
        e.forward(np.zeros((4, 64), np.float32))
    e.close()


def test_real_config_runs_and_is_deterministic():
    """google/siglip-so400m-patch14-384's tower (27 x 1152, 729 tokens, head dim 72, F = 4304) on random weights: one encode of a 301 x 517 picture is (1, 729,
    1152), finite, and the same bits twice."""
    import torch
    import diffusion_rs_amd as d
    m = d.SiglipVisionModel()
    d.synth.fill_text_random_device(m, seed=4)
    assert m.missing() == []
    pic = R.picture((301, 517), seed=9)
    a = m.encode(pic)
    b = m.encode(pic)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (1, 729, 1152) and a.dtype == torch.float32 and torch.isfinite(a).all() and torch.equal(a, b)
    t0 = time.perf_counter()
    m.encode(pic)
    torch.cuda.synchronize()
    print(f"SigLIP so400m-patch14-384 vision tower, one encode of a 301 x 517 picture: {(time.perf_counter() - t0) * 1e3:.1f} ms, resident "
          f"{m.size_in_bytes() / 2**20:.0f} MiB (size_in_bytes {m.size_in_bytes()})")
    assert m.size_in_bytes() > 27 * (4 * 1152 * 1152 + 2 * 4304 * 1152) * 2
    m.close()


# ------------------------------------------------------------------------------------------ the pipeline
HP, WP, T5_T = 64, 96, 512  # (the synthetic dev pipeline's placeholder prompts have 512 T5 rows)


@pytest.fixture(scope="module")
def rig():
    """The small synthetic pipeline of the other pipeline tests, with joint_attention_dim = the embedder's J; `plain`: two requests made before Redux is loaded."""
    import torch
    import diffusion_rs_amd as d
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=FLUX_CFG, vae_cfg=SMALL_VAE))
    pipe.flux.load_state_dict(d.synth.flux_state_dict_numpy(FLUX_CFG, seed=0))
    pipe.vae.load_state_dict(d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0, encoder=True))
    params = d.DiffusionGenerationParams(height=HP, width=WP, num_steps=3, guidance_scale=3.5)
    lat = dev((np.random.default_rng(11).standard_normal((2, 16, HP // 8, WP // 8)) * 0.15).astype(np.float32))

    def fwd(prompts=("a", "b"), **kw):
        prompts = list(prompts)
        return pipe.forward(prompts, params, output="tensor", latents=lat[:len(prompts)], return_latents=True, **kw)

    def text_rows(prompts):
        from diffusion_rs_amd.pipeline import placeholder_embeddings
        return placeholder_embeddings(list(prompts), T5_T, FLUX_CFG["joint_attention_dim"], FLUX_CFG["pooled_projection_dim"], pipe.device)

    plain = dict(text=fwd(), cfg=fwd(negative_prompt="n", true_cfg_scale=2.0))
    with pytest.raises(ValueError, match="needs a loaded Redux"):
        fwd(redux_image=R.picture((67, 45), seed=21))
    cfg = R.CONFIGS[TOWER]
    tower, emb = pipe.load_redux(R.redux_state_dict(cfg["hidden_size"]), image_encoder=(cfg, R.state_dict(cfg)))
    assert pipe.redux == (tower, emb) and emb.txt_dim == R.REDUX_J and tower.num_patches == 16
    yield dict(pipe=pipe, fwd=fwd, text_rows=text_rows, plain=plain, cfg=cfg, pic=R.picture((67, 45), seed=21), torch=torch)
    pipe.unload_redux()
    assert pipe.redux is None and tower.h is None and emb.h is None


def _equal(a, b):
    import torch
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_encode_redux_image_is_the_reference(rig):
    torch, pipe, cfg, pic = rig["torch"], rig["pipe"], rig["cfg"], rig["pic"]
    tok = pipe.encode_redux_image(pic)
    assert tuple(tok.shape) == (1, 16, R.REDUX_J) and tok.dtype == torch.float32 and tok.is_cuda and torch.isfinite(tok).all()
    tower = pipe.redux[0]
    S = cfg["image_size"]
    resized = tower.resize(pic, S, S).cpu().numpy()  # (the tower's bar is for the tower: the reference starts from the same resized picture)
    pv = ((resized.astype(np.float32).transpose(2, 0, 1) / np.float32(255) - np.float32(0.5)) / np.float32(0.5))[None]
    want = R.redux_forward(R.redux_state_dict(cfg["hidden_size"]), R.siglip_forward(R.state_dict(cfg), cfg, pv))
    print(f"encode_redux_image of a 67 x 45 picture vs the CPU reference: rel-L2 {rel_l2(host(tok), want):.3e}")
    assert rel_l2(host(tok), want) <= ENCODER_BAR
    pvd = tower.preprocess(pic)
    assert torch.equal(pipe.encode_redux_image(pvd), tok) and torch.equal(pipe.encode_redux_image(pvd.cpu().numpy()), tok)


@pytest.mark.parametrize("prompts", [("a",), ("a", "b")])
@pytest.mark.parametrize("max_batch", [8, 1])
def test_pipeline_identity(rig, prompts, max_batch, monkeypatch):
    """redux_image= == redux_image_embeds=encode_redux_image(.) == the explicit embeddings= request with the tokens behind the T5 rows, bit for bit: for one
    prompt, for two sharing the picture, and when the request is cut into chunks of one (the picture is still encoded once)."""
    torch, pipe, fwd, pic = rig["torch"], rig["pipe"], rig["fwd"], rig["pic"]
    monkeypatch.setattr(pipe, "MAX_BATCH", max_batch)
    tok = pipe.encode_redux_image(pic)
    calls = []
    tower = pipe.redux[0]
    monkeypatch.setattr(tower, "encode", lambda img, _f=tower.encode: (calls.append(1), _f(img))[1])
    by_picture = fwd(prompts, redux_image=pic)
    assert len(calls) == 1
    by_embeds = fwd(prompts, redux_image_embeds=tok)
    t5, clip = rig["text_rows"](prompts)
    explicit = fwd(prompts, embeddings=(torch.cat([t5, tok.to(t5.dtype).expand(len(prompts), -1, -1)], 1), clip))
    assert len(calls) == 1 and tuple(by_picture[0].shape) == (len(prompts), 3, HP, WP)
    assert _equal(by_picture, by_embeds) and _equal(by_picture, explicit)
    assert _equal(fwd(prompts, redux_image_embeds=tok[0].cpu().numpy()), by_picture)  # (Np,J) on the host
    assert _equal(fwd(prompts, redux_image=tower.preprocess(pic)), by_picture)  # pixel_values
    assert not torch.equal(by_picture[1], rig["plain"]["text"][1][:len(prompts)])  # ... and the tokens are seen
    # with the prompt as embeddings= the tokens go behind the caller's rows all the same
    short = (t5[:, :40].contiguous(), clip)
    assert _equal(fwd(prompts, embeddings=short, redux_image=pic),
                  fwd(prompts, embeddings=(torch.cat([short[0], tok.to(t5.dtype).expand(len(prompts), -1, -1)], 1), clip)))


def test_scale_and_zero_scale(rig):
    """redux_scale multiplies the tokens once, in f32; at 0 the rows are still appended, as zeros: T stays T_prompt + Np."""
    torch, pipe, fwd, pic = rig["torch"], rig["pipe"], rig["fwd"], rig["pic"]
    tok = pipe.encode_redux_image(pic)
    t5, clip = rig["text_rows"](("a", "b"))
    for scale in (0.5, 0.0):
        rows = (tok * scale).to(t5.dtype).expand(2, -1, -1)
        explicit = fwd(embeddings=(torch.cat([t5, rows], 1), clip))
        assert _equal(fwd(redux_image=pic, redux_scale=scale), explicit) and _equal(fwd(redux_image_embeds=tok, redux_scale=scale), explicit)
    assert not torch.equal(explicit[1], rig["plain"]["text"][1])  # zero rows are rows: the other tokens attend to them


def test_negative_half_receives_zero_rows(rig):
    """Under a negative prompt both halves keep one T: the request equals the explicit embeddings= / negative_embeddings= request whose negative ends with Np
    zero rows, bit for bit."""
    torch, pipe, fwd, pic = rig["torch"], rig["pipe"], rig["fwd"], rig["pic"]
    tok = pipe.encode_redux_image(pic)
    t5, clip = rig["text_rows"](("a", "b"))
    nt5, nclip = rig["text_rows"](("n",))
    rows = tok.to(t5.dtype)
    explicit = fwd(embeddings=(torch.cat([t5, rows.expand(2, -1, -1)], 1), clip), negative_embeddings=(torch.cat([nt5, torch.zeros_like(rows)], 1), nclip),
                   true_cfg_scale=2.0)
    got = fwd(redux_image=pic, negative_prompt="n", true_cfg_scale=2.0)
    assert _equal(got, explicit) and _equal(fwd(redux_image_embeds=tok, negative_prompt="n", true_cfg_scale=2.0), explicit)
    assert not torch.equal(got[1], rig["plain"]["cfg"][1])
    mirrored = fwd(embeddings=(torch.cat([t5, rows.expand(2, -1, -1)], 1), clip), negative_embeddings=(torch.cat([nt5, rows], 1), nclip), true_cfg_scale=2.0)
    assert not _equal(got, mirrored)  # (the negative does not see the picture)


def test_requests_without_redux_are_unchanged_and_redux_combines(rig):
    """A request without the new keywords returns the bits it returned before Redux was loaded; Redux combines with image= / strength= and the step cache; the
    refusals name their argument."""
    torch, pipe, fwd, pic = rig["torch"], rig["pipe"], rig["fwd"], rig["pic"]
    assert _equal(fwd(), rig["plain"]["text"]) and _equal(fwd(negative_prompt="n", true_cfg_scale=2.0), rig["plain"]["cfg"])
    tok = pipe.encode_redux_image(pic)
    src = np.random.default_rng(5).integers(0, 256, (HP, WP, 3)).astype(np.uint8)
    for kw in (dict(image=src, strength=0.7), dict(cache_threshold=0.05), dict(reference=src)):
        assert _equal(fwd(redux_image=pic, **kw), fwd(redux_image_embeds=tok, **kw))
    for kw, msg in ((dict(redux_image=pic, redux_image_embeds=tok), "exclude one another"), (dict(redux_image=np.zeros((1, 3, 64, 64), np.float32)), "redux_image= must be"),
                    (dict(redux_image_embeds=tok[:, :8]), "redux_image_embeds= must be"), (dict(redux_image=pic, redux_scale=float("inf")), "redux_scale")):
        with pytest.raises(ValueError, match=msg):
            fwd(**kw)
    import diffusion_rs_amd as d
    cfg = rig["cfg"]
    with pytest.raises(ValueError, match="txt_in_features is 128, the transformer's joint_attention_dim is 256"):
        pipe.load_redux(R.redux_state_dict(cfg["hidden_size"], J=128), image_encoder=(cfg, R.state_dict(cfg)))
    with pytest.raises(ValueError, match="redux_dim is 128, the SigLIP tower's hidden_size is 576"):
        pipe.load_redux(R.redux_state_dict(128), image_encoder=(cfg, R.state_dict(cfg)))
    assert pipe.redux is not None and pipe.redux[0].h is not None  # a refused load leaves the loaded one in place
