"""CLIP vision encoder, the parts that need no GPU: the CPU restatements of tests/clip_vision_ref.py are pinned to committed PIL and
transformers outputs (tests/golden/clip_vision.npz; neither package is needed here), the loader's name handling, every request-level refusal of the Python
layer, the crop offsets and the resize-shape rule."""
import json

import numpy as np
import pytest
import torch

import diffusion_rs_amd as d
from diffusion_rs_amd import _lib as L
from diffusion_rs_amd import flux as F
from diffusion_rs_amd import loader
from diffusion_rs_amd import pipeline as P
from diffusion_rs_amd import text
from tests import clip_vision_ref as R
from tests.util import rel_l2

SYMBOLS = ("fmi_resize_bicubic_u8", "fmi_clip_preprocess_u8", "fmi_clip_vision_default_config", "fmi_clip_vision_create", "fmi_clip_vision_destroy",
           "fmi_clip_vision_set_tensor", "fmi_clip_vision_missing_count", "fmi_clip_vision_missing_name", "fmi_clip_vision_size_in_bytes", "fmi_clip_vision_forward")


def test_symbols_are_exported_and_bound():
    lib = L.load()
    for s in SYMBOLS:
        assert s in L.EXPORTED and hasattr(lib, s), s
    assert [f[0] for f in L.ClipVisionConfig._fields_] == list(text.CLIP_VISION_L)
    c = L.ClipVisionConfig()
    lib.fmi_clip_vision_default_config(L.C.byref(c))  # (fills a struct: no device)
    assert {k: getattr(c, k) for k in text.CLIP_VISION_L} == text.CLIP_VISION_L == dict(image_size=224, patch_size=14, hidden_size=1024, intermediate_size=4096,
                                                                                       num_hidden_layers=24, num_attention_heads=16, projection_dim=768)


# ------------------------------------------------------------------------------------------ the two pins
@pytest.mark.parametrize("case", list(R.RESIZE_CASES))
def test_reference_resize_is_pil_bicubic(case):
    """The two-pass recipe against PIL 12.2's Image.resize(BICUBIC) on the committed pictures: every value within 1, at most 2e-3 of them different (PIL works
    in 22-bit fixed point and rounds half up; the recipe is float and rounds half to even).  Measured, float32 / float64 recipe: down 3.0e-4 / 6.0e-4, tall
    2.9e-4 / 0, one_pass 6.6e-4 / 2.6e-4, noop 0 / 0, up3 8.9e-4 / 8.9e-4 (3 of 3360 values), binary 0 / 0 — all under 1e-3, all differences 1."""
    z = np.load(R.GOLDEN)
    (h, w), (nh, nw), kind = R.RESIZE_CASES[case]
    src, want = z[f"resize_in/{case}"], z[f"resize_out/{case}"]
    assert src.shape == (h, w, 3) and want.shape == (nh, nw, 3) and src.dtype == want.dtype == np.uint8
    i = list(R.RESIZE_CASES).index(case)
    assert np.array_equal(src, R.picture((h, w), kind, seed=100 + i))  # the committed picture is the seeded one the GPU test regenerates
    if kind == "binary":
        assert set(np.unique(src)) == {0, 255}
    for dtype in (np.float32, np.float64):
        got = R.resize_bicubic_u8(src, nh, nw, dtype)
        diff = np.abs(got.astype(int) - want.astype(int))
        print(f"{case} {dtype.__name__}: max {diff.max()}, share of differing values {(diff > 0).mean():.2e}")
        assert diff.max() <= 1 and (diff > 0).mean() <= 2e-3
        assert (diff > 0).mean() <= 1e-3  # the reference's own margin under the bar the kernel is held to
    if case == "noop":
        assert np.array_equal(R.resize_bicubic_u8(src, nh, nw), src)


def test_single_pass_float_bicubic_is_not_pil():
    """What the rounding and the clamp between the passes are for: without them (one float pass over both axes, rounded once) the binary picture is off by far
    more than 1 — the committed PIL output tells the two recipes apart."""
    z = np.load(R.GOLDEN)
    (h, w), (nh, nw), _ = R.RESIZE_CASES["binary"]
    src, want = z["resize_in/binary"], z["resize_out/binary"]
    one = np.einsum("oh,hwc->owc", R.resize_weights(h, nh), np.einsum("ow,hwc->hoc", R.resize_weights(w, nw), src.astype(np.float32)))
    one = np.clip(np.rint(one), 0, 255).astype(int)
    assert np.abs(one - want.astype(int)).max() > 1


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_reference_tower_is_transformers(name):
    """clip_vision_ref.vision_forward against transformers 5.15's CLIPVisionModelWithProjection (torch CPU, float32) on the seeded weights and inputs, B = 2.
    Measured rel-L2, float32 / float64 restatement: s56p14 embeds 4.1e-7 / 4.0e-7, hidden 5.6e-7 / 4.7e-7; s126p14 3.5e-7 / 3.6e-7, 4.8e-7 / 4.2e-7; s64p16
    4.7e-7 / 4.5e-7, 6.0e-7 / 5.4e-7 — float32 noise of the committed outputs themselves.  The bar is 1e-5: 20 x that noise, 1000 x under the GPU bar."""
    z = np.load(R.GOLDEN)
    cfg = R.CONFIGS[name]
    T = 1 + (cfg["image_size"] // cfg["patch_size"]) ** 2
    assert z[f"embeds/{name}"].shape == (2, cfg["projection_dim"]) and z[f"hidden/{name}"].shape == (2, T, cfg["hidden_size"])
    for dtype in (np.float32, np.float64):
        e, h = R.vision_forward(R.state_dict(cfg), cfg, R.pixel_values(cfg, 2), dtype)
        print(f"{name} {dtype.__name__}: embeds {rel_l2(e, z[f'embeds/{name}']):.2e}, hidden {rel_l2(h, z[f'hidden/{name}']):.2e}")
        assert rel_l2(e, z[f"embeds/{name}"]) <= 1e-5 and rel_l2(h, z[f"hidden/{name}"]) <= 1e-5
    e1, h1 = R.vision_forward(R.state_dict(cfg), cfg, R.pixel_values(cfg, 2)[1:], np.float32)  # a sample does not depend on its batch
    assert rel_l2(e1, z[f"embeds/{name}"][1:]) <= 1e-5 and rel_l2(h1, z[f"hidden/{name}"][1:]) <= 1e-5


# ------------------------------------------------------------------------------- shapes, crop, synth
def test_resize_shape_rule_and_crop_offsets():
    """int(image_size * long / short) as transformers computes it (Python float division, truncation), and the centre crop's floor division."""
    for (h, w, s), want in (((480, 640, 224), (224, 298)), ((640, 480, 224), (298, 224)), ((301, 517, 224), (224, 384)), ((31, 45, 28), (28, 40)),
                            ((67, 45, 28), (41, 28)), ((9, 13, 28), (28, 40)), ((28, 90, 28), (28, 90)), ((224, 224, 224), (224, 224)), ((100, 100, 56), (56, 56)),
                            ((333, 1000, 224), (224, 672)), ((3, 1000, 224), (224, 74666))):
        assert text.clip_resize_shape(h, w, s) == want == R.resize_shape(h, w, s), (h, w, s)
    assert text.clip_resize_shape(333, 1000, 224)[1] == int(224 * 1000 / 333) == 672  # (224 * 1000 / 333 = 672.67: truncated, not rounded)
    with pytest.raises(ValueError, match="cannot be resized"):
        text.clip_resize_shape(0, 10, 224)
    assert text.clip_crop_offsets(224, 298, 224) == (0, 37) and text.clip_crop_offsets(41, 28, 28) == (6, 0) and text.clip_crop_offsets(29, 40, 28) == (0, 6)
    with pytest.raises(ValueError, match="at least that size"):
        text.clip_crop_offsets(27, 40, 28)
    img = R.picture((41, 29), seed=4)
    pv = R.preprocess(img, 28)
    top, left = text.clip_crop_offsets(41, 29, 28)
    assert (top, left) == (6, 0) and pv.shape == (3, 28, 28) and pv.dtype == np.float32
    for c in range(3):
        want = (img[top:top + 28, left:left + 28, c].astype(np.float32) / np.float32(255) - np.float32(R.CLIP_MEAN[c])) / np.float32(R.CLIP_STD[c])
        assert np.array_equal(pv[c], want)
    assert R.image_processor(R.picture((67, 45), seed=5), 28).shape == (1, 3, 28, 28)
    assert tuple(text.CLIP_IMAGE_MEAN) == R.CLIP_MEAN and tuple(text.CLIP_IMAGE_STD) == R.CLIP_STD


def test_tensor_shapes_are_huggingface_names():
    cfg = R.CONFIGS["s56p14"]
    shapes = d.synth.clip_vision_tensor_shapes(cfg)
    assert shapes["vision_model.embeddings.class_embedding"] == (128,) and shapes["vision_model.embeddings.patch_embedding.weight"] == (128, 3, 14, 14)
    assert shapes["vision_model.embeddings.position_embedding.weight"] == (17, 128) and shapes["visual_projection.weight"] == (64, 128)
    assert "vision_model.pre_layrnorm.weight" in shapes and "vision_model.pre_layernorm.weight" not in shapes  # HuggingFace's spelling
    assert "vision_model.post_layernorm.bias" in shapes and shapes["vision_model.encoder.layers.2.mlp.fc1.weight"] == (256, 128)
    assert len(shapes) == 3 + 2 + 3 * 16 + 2 + 1
    assert len(d.synth.clip_vision_tensor_shapes(text.CLIP_VISION_L)) == 3 + 2 + 24 * 16 + 2 + 1
    sd = R.state_dict(cfg)
    assert list(sd) == list(shapes) and all(sd[k].shape == shapes[k] for k in sd)
    from tests.util import bf16_round
    assert all((bf16_round(v) == v).all() for v in sd.values())


# ------------------------------------------------------------------------------------------ the loader
def _write_dir(tmp_path, name, config, tensors, pre=None):
    from safetensors.torch import save_file
    p = tmp_path / name
    p.mkdir()
    (p / "config.json").write_text(json.dumps(config))
    if pre is not None:
        (p / "preprocessor_config.json").write_text(json.dumps(pre))
    save_file({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tensors.items()}, str(p / "model.safetensors"))
    return str(p)


CFG = dict(R.CONFIGS["s56p14"], num_hidden_layers=1)
HF_VISION = dict(CFG, model_type="clip_vision_model", hidden_act="quick_gelu", layer_norm_eps=1e-5, num_channels=3, attention_dropout=0.0)
PRE = dict(crop_size={"height": 56, "width": 56}, size={"shortest_edge": 56}, do_center_crop=True, do_normalize=True, do_resize=True, do_rescale=True,
           do_convert_rgb=True, resample=3, rescale_factor=1 / 255, image_mean=[0.5, 0.4, 0.3], image_std=[0.2, 0.25, 0.3], image_processor_type="CLIPImageProcessor")


def test_loader_configs():
    assert loader.clip_vision_config(HF_VISION) == CFG == loader.clip_vision_config(CFG)
    full = dict(model_type="clip", projection_dim=64, text_config=dict(hidden_size=32), vision_config={k: v for k, v in HF_VISION.items() if k != "projection_dim"})
    assert loader.clip_vision_config(full) == CFG  # a CLIPConfig: vision_config is used, projection_dim from the top level where the nested one has none
    assert loader.clip_vision_config(dict(full, vision_config=dict(HF_VISION, projection_dim=64), projection_dim=512)) == CFG  # (the nested one wins)
    for bad, msg in ((dict(HF_VISION, hidden_act="gelu"), "hidden_act.*quick_gelu"), (dict(HF_VISION, layer_norm_eps=1e-6), "layer_norm_eps"),
                     (dict(HF_VISION, num_channels=1), "num_channels"), ({k: v for k, v in HF_VISION.items() if k != "patch_size"}, r"lacks \['patch_size'\]"),
                     (dict(HF_VISION, model_type="siglip_vision_model"), "siglip_vision_model"), (dict(model_type="clip_text_model", hidden_size=8), "clip_text_model")):
        with pytest.raises(ValueError, match=msg):
            loader.clip_vision_config(bad)


def test_loader_image_processor():
    assert loader.clip_image_processor(None, 224) == (text.CLIP_IMAGE_MEAN, text.CLIP_IMAGE_STD) == ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
    assert loader.clip_image_processor(PRE, 56) == ((0.5, 0.4, 0.3), (0.2, 0.25, 0.3))
    assert loader.clip_image_processor(dict(crop_size=224, size=224, resample=3), 224) == (text.CLIP_IMAGE_MEAN, text.CLIP_IMAGE_STD)  # the older integer form
    for bad, msg in ((dict(PRE, do_center_crop=False), "do_center_crop = false"), (dict(PRE, do_resize=False), "do_resize = false"),
                     (dict(PRE, do_normalize=False), "do_normalize = false"), (dict(PRE, do_rescale=False), "do_rescale = false"), (dict(PRE, resample=2), "resample = 2"),
                     (dict(PRE, rescale_factor=1 / 127.5), "rescale_factor"), (dict(PRE, size={"shortest_edge": 64}), "size = "),
                     (dict(PRE, size={"height": 56, "width": 56}), "size = "), (dict(PRE, crop_size={"height": 56, "width": 48}), "crop_size = "),
                     (dict(PRE, crop_size=48), "crop_size = "), (dict(PRE, image_std=[0.2, 0.0, 0.3]), "image_mean / image_std"), (dict(PRE, image_mean=[0.5]), "image_mean / image_std")):
        with pytest.raises(ValueError, match=msg):
            loader.clip_image_processor(bad, 56)


def test_loader_name_handling(tmp_path):
    sd = R.state_dict(CFG)
    assert "vision_model.pre_layrnorm.weight" in sd
    cfg, got = loader.load_clip_vision(_write_dir(tmp_path, "vision", HF_VISION, sd, PRE))
    assert cfg == dict(CFG, image_mean=(0.5, 0.4, 0.3), image_std=(0.2, 0.25, 0.3)) and set(got) == set(sd)
    assert all(np.array_equal(got[k].numpy(), sd[k]) for k in sd) and tuple(got["vision_model.embeddings.patch_embedding.weight"].shape) == (128, 3, 14, 14)
    # a full CLIP checkpoint: the text tower, its projection, the logit scale and the position_ids buffers are ignored; no preprocessor_config.json: CLIP's constants
    extra = {"text_model.embeddings.token_embedding.weight": np.zeros((5, 8), np.float32), "text_model.encoder.layers.0.mlp.fc1.bias": np.zeros(4, np.float32),
             "text_model.embeddings.position_ids": np.zeros((1, 7), np.int64), "text_projection.weight": np.zeros((4, 8), np.float32),
             "logit_scale": np.zeros((), np.float32), "vision_model.embeddings.position_ids": np.zeros((1, 17), np.int64)}
    full_cfg = dict(model_type="clip", projection_dim=64, text_config={}, vision_config=HF_VISION)
    cfg, got = loader.load_clip_vision(_write_dir(tmp_path, "full", full_cfg, dict(sd, **extra)))
    assert cfg == dict(CFG, image_mean=text.CLIP_IMAGE_MEAN, image_std=text.CLIP_IMAGE_STD) and set(got) == set(sd)
    assert loader.clip_vision_from_tensors(CFG, dict(sd, **extra)).keys() == sd.keys()
    with pytest.raises(ValueError, match=r"1 unexpected tensors.*vision_model\.pre_layernorm\.weight"):  # the corrected spelling is not HuggingFace's name
        loader.clip_vision_from_tensors(CFG, dict(sd, **{"vision_model.pre_layernorm.weight": sd["vision_model.pre_layrnorm.weight"]}))
    with pytest.raises(ValueError, match=r"unexpected tensors.*vision_model\.encoder\.layers\.1\.mlp\.fc1\.bias"):  # a layer the configuration does not have
        loader.clip_vision_from_tensors(CFG, dict(sd, **{"vision_model.encoder.layers.1.mlp.fc1.bias": sd["vision_model.encoder.layers.0.mlp.fc1.bias"]}))
    with pytest.raises(ValueError, match=r"1 image-encoder tensors missing.*visual_projection\.weight"):
        loader.clip_vision_from_tensors(CFG, {k: v for k, v in sd.items() if k != "visual_projection.weight"})
    with pytest.raises(ValueError, match=r"2 image-encoder tensors missing.*vision_model\.pre_layrnorm\.weight"):
        loader.load_clip_vision(_write_dir(tmp_path, "lacking", HF_VISION, {k: v for k, v in sd.items() if "pre_layrnorm" not in k}))
    with pytest.raises(ValueError, match=r"patch_embedding\.weight is \(128, 588\), expected \(128, 3, 14, 14\)"):
        loader.clip_vision_from_tensors(CFG, dict(sd, **{"vision_model.embeddings.patch_embedding.weight": sd["vision_model.embeddings.patch_embedding.weight"].reshape(128, -1)}))
    with pytest.raises(ValueError, match="do_center_crop = false"):
        loader.load_clip_vision(_write_dir(tmp_path, "nocrop", HF_VISION, sd, dict(PRE, do_center_crop=False)))
    with pytest.raises(FileNotFoundError):
        loader.load_clip_vision(str(tmp_path / "none"))


# ------------------------------------------------------------------------------ request-level refusals
E, S = 64, 56
U8, PV = (37, 51, 3), (1, 3, S, S)


def test_check_ip_adapter_request_with_pictures():
    ok = dict(loaded=True, embed_dim=E, encoder_dim=E, encoder_image_size=S)
    P.check_ip_adapter_request(**ok, image_shape=U8, image_is_u8=True)
    P.check_ip_adapter_request(**ok, image_shape=PV)
    P.check_ip_adapter_request(**ok, image_shape=U8, image_is_u8=True, negative_image_shape=PV, has_negative=True)
    P.check_ip_adapter_request(**ok, image_shape=PV, negative_embeds_shape=(E,), has_negative=True)  # a picture on one side, an embedding on the other
    P.check_ip_adapter_request(**ok, embeds_shape=(1, E), negative_image_shape=U8, negative_image_is_u8=True, has_negative=True)
    P.check_ip_adapter_request(True, E, (E,))  # the positional form of before: untouched
    P.check_ip_adapter_request(False)
    bad = [(dict(image_shape=U8, image_is_u8=True, encoder_dim=None), r"ip_adapter_image= needs a loaded image encoder: Pipeline.load_image_encoder"),
           (dict(image_shape=U8, image_is_u8=True, loaded=False), r"ip_adapter_image= needs a loaded IP-Adapter: Pipeline.load_ip_adapter"),
           (dict(image_shape=U8, image_is_u8=True, loaded=False, encoder_dim=None), "needs a loaded IP-Adapter"),
           (dict(image_shape=U8, image_is_u8=True, embeds_shape=(E,)), "ip_adapter_image= and ip_adapter_image_embeds= exclude one another"),
           (dict(image_shape=U8, image_is_u8=True, negative_image_shape=PV, negative_embeds_shape=(E,), has_negative=True),
            "negative_ip_adapter_image= and negative_ip_adapter_image_embeds= exclude one another"),
           (dict(image_shape=U8, image_is_u8=True, encoder_dim=E + 64), f"projection_dim is {E + 64}, the IP-Adapter's embed_dim {E}"),
           (dict(image_shape=U8, image_is_u8=True, negative_image_shape=PV), "negative_ip_adapter_image= needs a negative prompt"),
           (dict(negative_image_shape=PV, has_negative=True), "negative_ip_adapter_image= needs ip_adapter_image="),
           (dict(embeds_shape=(E,), negative_image_shape=PV, has_negative=True, encoder_dim=None), "negative_ip_adapter_image= needs a loaded image encoder"),
           (dict(image_shape=(37, 51, 4), image_is_u8=True), "ip_adapter_image must be a uint8"), (dict(image_shape=(2, 37, 51, 3), image_is_u8=True), "ip_adapter_image must be"),
           (dict(image_shape=(1, 3, S, S + 1)), "ip_adapter_image must be"), (dict(image_shape=(2, 3, S, S)), "one per request"),
           (dict(image_shape=PV, negative_image_shape=(3, S, S), has_negative=True), "negative_ip_adapter_image must be"),
           (dict(image_shape=PV, scale=float("nan")), "finite"), (dict(image_shape=PV, start=0.6, end=0.5), "0 <= start <= end <= 1")]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            P.check_ip_adapter_request(**dict(ok, **kw))


class _FakeAdapter:
    embed_dim = E


class _FakeEncoder:
    projection_dim, cfg = E, dict(image_size=S)

    def __init__(self):
        self.seen = []

    def encode(self, img):
        self.seen.append(img)
        return torch.full((1, E), float(len(self.seen)))


class _Recording(P.Pipeline):
    def __init__(self, adapter=True, encoder=True):  # no GPU: the request path in front of the chunk body
        import threading
        self.device, self._lock, self.chunks = torch.device("cpu"), threading.Lock(), []
        self.ip_adapter = _FakeAdapter() if adapter else None
        self.image_encoder = _FakeEncoder() if encoder else None

    def _generate_chunk(self, s, params, seed, strength, return_latents, cache_threshold, stats, **shared):
        self.chunks.append((s, shared))
        return torch.zeros((len(s.prompts), 3, params.height, params.width), dtype=torch.uint8)


def _params():
    return P.DiffusionGenerationParams(16, 16, 2, 3.5)


def test_a_picture_becomes_its_embedding_before_the_request_is_chunked():
    pipe = _Recording()
    pic = np.zeros(U8, np.uint8)
    pipe.generate_tensor([f"p{i}" for i in range(11)], _params(), ip_adapter_image=pic, ip_adapter_scale=0.5)
    assert len(pipe.chunks) == 2 and len(pipe.image_encoder.seen) == 1  # encoded once, whatever the number of chunks
    a, b = (c[1]["ip_adapter"] for c in pipe.chunks)
    assert a is b and isinstance(a, P._IpAdapterInput) and torch.equal(a.embeds, torch.full((1, E), 1.0)) and a.negative_embeds is None and a.scale == 0.5
    assert [f.name for f in __import__("dataclasses").fields(P._IpAdapterInput)] == ["embeds", "negative_embeds", "scale", "start", "end"]
    pipe = _Recording()
    pipe.generate_tensor(["a"], _params(), ip_adapter_image=torch.zeros(PV), negative_ip_adapter_image=pic, true_cfg_scale=2.0,
                         embeddings=(torch.zeros(1, 4, 8), torch.zeros(1, 8)), negative_embeddings=(torch.zeros(1, 4, 8), torch.zeros(1, 8)))
    ipa = pipe.chunks[0][1]["ip_adapter"]
    assert torch.equal(ipa.embeds, torch.full((1, E), 1.0)) and torch.equal(ipa.negative_embeds, torch.full((1, E), 2.0))
    assert pipe.image_encoder.seen[0].dtype == torch.float32 and pipe.image_encoder.seen[1].dtype == torch.uint8
    pipe = _Recording()
    pipe.generate_tensor(["a"], _params())  # no picture: no encoder call, no ip_adapter keyword — the call of before
    assert pipe.image_encoder.seen == [] and pipe.chunks[0][1] == {}


def test_request_refusals_without_a_device():
    pic = np.zeros(U8, np.uint8)
    for pipe, kw, msg in ((_Recording(encoder=False), dict(ip_adapter_image=pic), "needs a loaded image encoder"),
                          (_Recording(adapter=False), dict(ip_adapter_image=pic), "needs a loaded IP-Adapter"),
                          (_Recording(), dict(ip_adapter_image=pic, ip_adapter_image_embeds=np.zeros(E, np.float32)), "exclude one another"),
                          (_Recording(), dict(ip_adapter_image=pic, negative_ip_adapter_image=pic, negative_ip_adapter_image_embeds=np.zeros(E, np.float32),
                                              negative_prompt="n", true_cfg_scale=2.0), "negative_ip_adapter_image= and negative_ip_adapter_image_embeds= exclude"),
                          (_Recording(), dict(ip_adapter_image=pic, negative_ip_adapter_image=pic), "needs a negative prompt"),
                          (_Recording(), dict(negative_ip_adapter_image=pic, negative_prompt="n"), "needs ip_adapter_image="),
                          (_Recording(), dict(ip_adapter_image=np.zeros((4, 4), np.uint8)), "ip_adapter_image must be"),
                          (_Recording(), dict(ip_adapter_image=[[1, 2]]), "ip_adapter_image must be a numpy array or a torch tensor"),
                          (_Recording(), dict(ip_adapter_image=np.zeros(U8, np.int32)), "ip_adapter_image must be uint8 or float")):
        with pytest.raises(ValueError, match=msg):
            pipe.generate_tensor(["a"], _params(), **kw)
        assert pipe.chunks == [] and (pipe.image_encoder is None or pipe.image_encoder.seen == [])  # refused before anything is encoded
    enc = _FakeEncoder()
    enc.projection_dim = 768
    pipe = _Recording()
    pipe.image_encoder = enc
    with pytest.raises(ValueError, match="projection_dim is 768, the IP-Adapter's embed_dim 64"):
        pipe.generate_tensor(["a"], _params(), ip_adapter_image=pic)
    with pytest.raises(ValueError, match="encode_image needs a loaded image encoder"):
        _Recording(encoder=False).encode_image(pic)
    with pytest.raises(ValueError, match="image must be a uint8"):
        _Recording().encode_image(np.zeros((1, 3, S, S + 2), np.float32))


def test_a_picture_combines_and_is_refused_like_its_embedding():
    """One combination table (flux.REFUSED_PAIRS / REFUSED_MODES under pipeline.REQUEST_NAMES): a request names "ip_adapter" whichever form the prompt came in."""
    pic, emb = np.zeros(U8, np.uint8), np.zeros(E, np.float32)
    rows = [(a, b) for a, b in F.REFUSED_PAIRS + F.REFUSED_MODES if a == "ip_adapter"]
    assert sorted(b for _, b in rows) == ["cache", "context", "fp8", "int8", "sequence_parallel"]
    for other, kw in (("context", dict(reference=torch.zeros(1, 3, 16, 16))), ("cache", dict(cache_threshold=0.1)), ("sequence_parallel", {}), ("int8", {})):
        messages = []
        for form in (dict(ip_adapter_image=pic), dict(ip_adapter_image_embeds=emb)):
            pipe = _Recording()
            if other == "sequence_parallel":
                pipe._sp = object()
            if other == "int8":
                pipe._int8_pending = True
            with pytest.raises(ValueError) as ei:
                pipe.generate_tensor(["a"], _params(), **form, **kw)
            messages.append(str(ei.value))
            assert pipe.chunks == []
        assert messages[0] == messages[1] and messages[0].startswith("an IP-Adapter is not "), messages
    for form in (dict(ip_adapter_image=pic), dict(ip_adapter_image_embeds=emb)):  # ... and what combines, combines: image= / strength=, a negative
        pipe = _Recording()
        pipe.generate_tensor(["a", "b"], _params(), image=torch.zeros(1, 3, 16, 16), strength=0.5, negative_prompt="n", true_cfg_scale=2.0, **form)
        assert len(pipe.chunks) == 1 and set(pipe.chunks[0][1]) == {"negative", "ip_adapter"}
    sig = __import__("inspect").signature
    for name in ("ip_adapter_image", "negative_ip_adapter_image"):
        assert sig(P.Pipeline.generate_tensor).parameters[name].default is None and sig(P.Pipeline.forward).parameters[name].default is None
