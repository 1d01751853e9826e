"""FLUX.1 Redux without a device: the CPU restatement of tests/redux_ref.py pinned to committed transformers and PIL outputs, the loaders'
name handling and refusals, the request checks, and the request path in front of the chunk body."""
import dataclasses
import inspect
import json
import os
import threading

import numpy as np
import pytest
import torch

import diffusion_rs_amd as d
from diffusion_rs_amd import _lib as L
from diffusion_rs_amd import flux as F
from diffusion_rs_amd import loader
from diffusion_rs_amd import pipeline as P
from diffusion_rs_amd import synth, text
from tests import redux_ref as R
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = tuple(f"fmi_siglip_vision_{n}" for n in ("default_config", "create", "destroy", "set_tensor", "missing_count", "missing_name", "size_in_bytes", "forward",
                                                   "poison_workspace")) + \
    tuple(f"fmi_redux_{n}" for n in ("create", "destroy", "set_tensor", "missing_count", "missing_name", "size_in_bytes", "forward"))

# The f32 restatement lies 5.96e-7 (h64_t16), 5.52e-7 (h72_t16) and 4.99e-7 (h72_t81) from transformers 5.15 on the CPU (the fixture generator prints them):
# both sides are f32 and differ in summation order only.  The bar is 4 x the largest.
RESTATEMENT_BAR = 4 * 5.96e-7


def test_symbols_are_exported_bound_and_declared():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    for s in SYMBOLS:
        assert s in L.EXPORTED and hasattr(lib, s) and f" {s}(" in header, s
    assert "typedef struct fmi_siglip_vision_config" in header and "typedef struct fmi_redux fmi_redux" in header
    assert [f[0] for f in L.SiglipVisionConfig._fields_] == list(text.SIGLIP_SO400M)
    c = L.SiglipVisionConfig()
    lib.fmi_siglip_vision_default_config(L.C.byref(c))  # (fills a struct: no device)
    got = {k: getattr(c, k) for k in text.SIGLIP_SO400M}
    assert got.pop("layer_norm_eps") == np.float32(1e-6)
    assert got == {k: v for k, v in text.SIGLIP_SO400M.items() if k != "layer_norm_eps"} == dict(image_size=384, patch_size=14, hidden_size=1152, intermediate_size=4304,
                                                                                                   num_hidden_layers=27, num_attention_heads=16)
    assert all(hasattr(d, n) for n in ("SiglipVisionModel", "ReduxImageEmbedder", "SIGLIP_SO400M"))


# ------------------------------------------------------------------------------------------ the two pins
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_reference_tower_is_transformers(name):
    """redux_ref.siglip_forward (f32) against SiglipVisionModel.last_hidden_state of transformers 5.15 (torch CPU, f32) on the same seeded weights and inputs."""
    want = np.load(R.GOLDEN)[f"hidden/{name}"]
    got = R.reference(name, 2)
    cfg = R.CONFIGS[name]
    assert got.shape == want.shape == (2, R.num_patches(cfg), cfg["hidden_size"]) and got.dtype == np.float32
    err = rel_l2(got, want)
    print(f"restatement {name}: rel-L2 from transformers {err:.2e}")
    assert err <= RESTATEMENT_BAR
    # float64 says the same of the recipe: the distance does not grow with the precision of the restatement
    assert rel_l2(R.siglip_forward(R.state_dict(cfg), cfg, R.pixel_values(cfg, 2), np.float64), want) <= RESTATEMENT_BAR


@pytest.mark.parametrize("case", list(R.RESIZE_CASES))
def test_direct_to_square_resize_is_pil(case):
    """The two-pass recipe straight to S x S against PIL 12.2's Image.resize((S, S), BICUBIC) on the committed pictures: every value within 1, at most 2e-3 of
    them different — the project's criteria for the resize (tests/test_gpu_clip_vision.py)."""
    shape, kind, seed = R.RESIZE_CASES[case]
    z = np.load(R.GOLDEN)
    src = R.picture(shape, kind, seed=seed)
    assert np.array_equal(z[f"resize_in/{case}"], src)
    got = R.resize_bicubic_u8(src, R.RESIZE_S, R.RESIZE_S)
    diff = np.abs(got.astype(int) - z[f"resize_out/{case}"].astype(int))
    print(f"resize {case} {shape} -> {R.RESIZE_S} x {R.RESIZE_S}: max {int(diff.max())}, share {float((diff > 0).mean()):.2e}")
    assert got.shape == (R.RESIZE_S, R.RESIZE_S, 3) and diff.max() <= 1 and (diff > 0).mean() <= 2e-3
    pv = R.image_processor(src, R.RESIZE_S)
    assert pv.shape == (1, 3, R.RESIZE_S, R.RESIZE_S) and np.array_equal(pv[0, 1], (got[:, :, 1].astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5))


def test_redux_embedder_reference():
    rng = np.random.default_rng(0)
    rsd = R.redux_state_dict(128)
    h = rng.standard_normal((1, 5, 128)).astype(np.float32)
    up = torch.nn.Linear(128, 3 * R.REDUX_J)
    down = torch.nn.Linear(3 * R.REDUX_J, R.REDUX_J)
    with torch.no_grad():
        up.weight.copy_(torch.from_numpy(rsd["redux_up.weight"])), up.bias.copy_(torch.from_numpy(rsd["redux_up.bias"]))
        down.weight.copy_(torch.from_numpy(rsd["redux_down.weight"])), down.bias.copy_(torch.from_numpy(rsd["redux_down.bias"]))
        want = down(torch.nn.functional.silu(up(torch.from_numpy(h)))).numpy()  # diffusers' ReduxImageEncoder.forward
    assert rel_l2(R.redux_forward(rsd, h), want) <= 1e-6 and np.array_equal(R.redux_forward(rsd, h, 0.5), np.float32(0.5) * R.redux_forward(rsd, h))


def test_tensor_shapes_are_huggingface_names():
    cfg = R.CONFIGS["h72_t16"]
    sh = synth.siglip_vision_tensor_shapes(cfg)
    assert sh["vision_model.embeddings.patch_embedding.weight"] == (576, 3, 14, 14) and sh["vision_model.embeddings.patch_embedding.bias"] == (576,)
    assert sh["vision_model.embeddings.position_embedding.weight"] == (16, 576)  # no class token
    assert sh["vision_model.encoder.layers.1.mlp.fc1.weight"] == (1076, 576) and sh["vision_model.encoder.layers.1.self_attn.out_proj.bias"] == (576,)
    assert len(sh) == 3 + 16 * cfg["num_hidden_layers"] + 2 and not any("head" in k or "class_embedding" in k or "pre_layrnorm" in k for k in sh)
    assert dict(synth.redux_tensor_shapes(1152, 4096)) == {"redux_up.weight": (12288, 1152), "redux_up.bias": (12288,), "redux_down.weight": (4096, 12288),
                                                           "redux_down.bias": (4096,)}


# ------------------------------------------------------------------------------------------ the loaders
def _write_dir(tmp_path, name, config, tensors, pre=None):
    from safetensors.torch import save_file
    p = tmp_path / name
    p.mkdir(parents=True)
    (p / "config.json").write_text(json.dumps(config))
    if pre is not None:
        (p / "preprocessor_config.json").write_text(json.dumps(pre))
    save_file({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tensors.items()}, str(p / "model.safetensors"))
    return str(p)


CFG = dict(R.CONFIGS["h64_t16"], num_hidden_layers=1)
HF_VISION = dict(CFG, model_type="siglip_vision_model", hidden_act="gelu_pytorch_tanh", num_channels=3, attention_dropout=0.0)
PRE = dict(size={"height": 64, "width": 64}, do_normalize=True, do_resize=True, do_rescale=True, do_convert_rgb=None, resample=3, rescale_factor=1 / 255,
           image_mean=[0.5, 0.4, 0.3], image_std=[0.5, 0.25, 0.3], image_processor_type="SiglipImageProcessor")


def test_loader_configs():
    assert loader.siglip_vision_config(HF_VISION) == CFG == loader.siglip_vision_config(CFG)
    full = dict(model_type="siglip", text_config=dict(hidden_size=32, vocab_size=9), vision_config=dict(HF_VISION))
    assert loader.siglip_vision_config(full) == CFG  # a SiglipConfig: vision_config is used, the text tower ignored
    assert loader.siglip_vision_config({k: v for k, v in HF_VISION.items() if k != "layer_norm_eps"})["layer_norm_eps"] == 1e-6  # (HuggingFace's default)
    for bad, msg in ((dict(HF_VISION, hidden_act="gelu"), "hidden_act is 'gelu': only gelu_pytorch_tanh"), (dict(HF_VISION, hidden_act="quick_gelu"), "quick_gelu"),
                     (dict(HF_VISION, num_channels=1), "num_channels"), ({k: v for k, v in HF_VISION.items() if k != "patch_size"}, r"lacks \['patch_size'\]"),
                     (dict(HF_VISION, model_type="clip_vision_model"), "clip_vision_model"), (dict(full, model_type="clip"), "model_type 'clip'"),
                     (dict(HF_VISION, layer_norm_eps=0.0), "layer_norm_eps")):
        with pytest.raises(ValueError, match=msg):
            loader.siglip_vision_config(bad)
    with pytest.raises(ValueError, match="siglip_vision_model.*load_siglip_vision"):  # the CLIP loader's refusal stays, and points here
        loader.clip_vision_config(dict(HF_VISION, projection_dim=64))


def test_loader_image_processor():
    assert loader.siglip_image_processor(None, 384) == (text.SIGLIP_IMAGE_MEAN, text.SIGLIP_IMAGE_STD) == ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    assert loader.siglip_image_processor(PRE, 64) == ((0.5, 0.4, 0.3), (0.5, 0.25, 0.3))
    assert loader.siglip_image_processor(dict(size=384, resample=3), 384) == (text.SIGLIP_IMAGE_MEAN, text.SIGLIP_IMAGE_STD)  # (an integer size)
    for bad, msg in ((dict(PRE, resample=2), "resample = 2"), (dict(PRE, do_center_crop=True), "do_center_crop = true"), (dict(PRE, size={"height": 64, "width": 48}), "size ="),
                     (dict(PRE, size={"shortest_edge": 64}), "size ="), (dict(PRE, size={"height": 384, "width": 384}), "image_size = 64"),
                     (dict(PRE, do_resize=False), "do_resize = false"), (dict(PRE, do_normalize=False), "do_normalize = false"), (dict(PRE, rescale_factor=1.0), "rescale_factor"),
                     (dict(PRE, image_std=[0.5, 0.0, 0.5]), "image_mean / image_std")):
        with pytest.raises(ValueError, match=msg):
            loader.siglip_image_processor(bad, 64)


def test_loader_name_handling(tmp_path):
    sd = R.state_dict(CFG)
    bare = {k[len("vision_model."):]: v for k, v in sd.items()}  # what transformers 5 writes for a bare SiglipVisionModel
    head = {"head.probe": np.zeros((1, 1, 128), np.float32), "head.attention.in_proj_weight": np.zeros((384, 128), np.float32), "head.mlp.fc1.bias": np.zeros(8, np.float32)}
    for i, tensors in enumerate((sd, bare, dict(sd, **{"vision_model." + k: v for k, v in head.items()}), dict(bare, **head),
                                 dict(sd, **{"text_model.embeddings.token_embedding.weight": np.zeros((9, 32), np.float32), "logit_scale": np.zeros(1, np.float32),
                                             "logit_bias": np.zeros(1, np.float32)}))):
        cfg, got = loader.load_siglip_vision(_write_dir(tmp_path, f"ok{i}", HF_VISION, tensors, PRE if i % 2 else None))
        assert set(got) == set(sd) and all(np.array_equal(got[k].numpy(), sd[k]) for k in sd)
        assert {k: cfg[k] for k in CFG} == CFG and cfg["image_mean"] == ((0.5, 0.4, 0.3) if i % 2 else (0.5, 0.5, 0.5))
    pre_dir = tmp_path / "feature_extractor"
    pre_dir.mkdir()
    (pre_dir / "preprocessor_config.json").write_text(json.dumps(PRE))
    assert loader.load_siglip_vision(_write_dir(tmp_path, "pre_elsewhere", HF_VISION, sd), str(pre_dir))[0]["image_std"] == (0.5, 0.25, 0.3)
    with pytest.raises(ValueError, match=r"1 unexpected tensors .*\['vision_model.pre_layrnorm.weight'\]"):
        loader.load_siglip_vision(_write_dir(tmp_path, "extra", HF_VISION, dict(sd, **{"vision_model.pre_layrnorm.weight": np.zeros(128, np.float32)})))
    with pytest.raises(ValueError, match=r"1 unexpected tensors .*\['visual_projection.weight'\]"):
        loader.load_siglip_vision(_write_dir(tmp_path, "extra2", HF_VISION, dict(bare, **{"visual_projection.weight": np.zeros((8, 128), np.float32)})))
    with pytest.raises(ValueError, match=r"1 SigLIP image-encoder tensors missing, e.g. \['vision_model.embeddings.patch_embedding.bias'\]"):
        loader.load_siglip_vision(_write_dir(tmp_path, "missing", HF_VISION, {k: v for k, v in sd.items() if k != "vision_model.embeddings.patch_embedding.bias"}))
    with pytest.raises(ValueError, match=r"position_embedding.weight is \(17, 128\), expected \(16, 128\)"):
        loader.load_siglip_vision(_write_dir(tmp_path, "shape", HF_VISION, dict(sd, **{"vision_model.embeddings.position_embedding.weight": np.zeros((17, 128), np.float32)})))
    with pytest.raises(ValueError, match="resample = 2"):
        loader.load_siglip_vision(_write_dir(tmp_path, "resample", HF_VISION, sd, dict(PRE, resample=2)))
    with pytest.raises(FileNotFoundError, match="not a directory"):
        loader.load_siglip_vision(str(tmp_path / "nowhere"))


def test_redux_loader(tmp_path):
    from safetensors.torch import save_file
    rsd = R.redux_state_dict(128)
    D, J, got = loader.load_redux(_write_dir(tmp_path, "image_embedder", dict(_class_name="ReduxImageEncoder", redux_dim=128, txt_in_features=R.REDUX_J), rsd))
    assert (D, J) == (128, R.REDUX_J) and set(got) == set(rsd) and all(np.array_equal(got[k].numpy(), rsd[k]) for k in rsd)
    single = str(tmp_path / "flux1-redux-dev.safetensors")  # BFL's single file: the same four names, the dimensions read off redux_up.weight
    save_file({k: torch.from_numpy(v) for k, v in rsd.items()}, single)
    D, J, got = loader.load_redux(single)
    assert (D, J) == (128, R.REDUX_J) and set(got) == set(rsd)
    assert loader.redux_from_tensors(rsd)[:2] == (128, R.REDUX_J)
    with pytest.raises(ValueError, match=r"lacks \['txt_in_features'\]"):
        loader.load_redux(_write_dir(tmp_path, "noconf", dict(redux_dim=128), rsd))
    with pytest.raises(ValueError, match="config.json has redux_dim = 1152, redux_up.weight .* says 128"):
        loader.load_redux(_write_dir(tmp_path, "dim", dict(redux_dim=1152, txt_in_features=R.REDUX_J), rsd))
    with pytest.raises(ValueError, match="config.json has txt_in_features = 4096"):
        loader.load_redux(_write_dir(tmp_path, "dim2", dict(redux_dim=128, txt_in_features=4096), rsd))
    with pytest.raises(ValueError, match=r"1 unexpected tensors .*\['redux_mid.weight'\]"):
        loader.redux_from_tensors(dict(rsd, **{"redux_mid.weight": np.zeros((4, 4), np.float32)}))
    with pytest.raises(ValueError, match=r"1 Redux tensors missing, e.g. \['redux_down.bias'\]"):
        loader.redux_from_tensors({k: v for k, v in rsd.items() if k != "redux_down.bias"})
    with pytest.raises(ValueError, match=r"redux_down.weight is \(256, 700\), expected \(256, 768\)"):
        loader.redux_from_tensors(dict(rsd, **{"redux_down.weight": np.zeros((256, 700), np.float32)}))
    with pytest.raises(FileNotFoundError):
        loader.load_redux(str(tmp_path / "nowhere.safetensors"))


# ------------------------------------------------------------------------------------------ the request
NP, J, S = 16, 256, 64
U8, PV = (37, 51, 3), (1, 3, S, S)


def test_check_redux_request():
    ok = dict(loaded=True, num_patches=NP, txt_dim=J, image_size=S)
    P.check_redux_request(False)  # a request without Redux arguments: nothing to check, whatever is loaded
    P.check_redux_request(**ok)
    P.check_redux_request(**ok, image_shape=U8, image_is_u8=True)
    P.check_redux_request(**ok, image_shape=PV, scale=0.0)
    P.check_redux_request(**ok, embeds_shape=(NP, J))
    P.check_redux_request(**ok, embeds_shape=(1, NP, J), scale=2.5)
    bad = [(dict(image_shape=U8, image_is_u8=True, loaded=False), r"redux_image= needs a loaded Redux: Pipeline.load_redux"),
           (dict(embeds_shape=(NP, J), loaded=False), r"redux_image_embeds= needs a loaded Redux: Pipeline.load_redux"),
           (dict(image_shape=U8, image_is_u8=True, embeds_shape=(NP, J)), "redux_image= and redux_image_embeds= exclude one another"),
           (dict(embeds_shape=(NP + 1, J)), rf"redux_image_embeds= must be \({NP},{J}\) or \(1,{NP},{J}\)"), (dict(embeds_shape=(2, NP, J)), "one picture per request"),
           (dict(embeds_shape=(NP, J // 2)), "redux_image_embeds= must be"), (dict(embeds_shape=(J,)), "redux_image_embeds= must be"),
           (dict(image_shape=(37, 51, 4), image_is_u8=True), "redux_image= must be a uint8"), (dict(image_shape=(2, 37, 51, 3), image_is_u8=True), "redux_image= must be"),
           (dict(image_shape=(1, 3, S, S + 1)), "redux_image= must be"), (dict(image_shape=(2, 3, S, S)), "one picture per request"),
           (dict(image_shape=U8, image_is_u8=True, sequence_parallel=True), r"Redux \(redux_image= / redux_image_embeds=\) is not supported under sequence parallelism"),
           (dict(embeds_shape=(NP, J), sequence_parallel=True), "sequence parallelism: disable_sequence_parallel"),
           (dict(image_shape=PV, scale=float("nan")), "redux_scale must be finite and >= 0"), (dict(image_shape=PV, scale=float("inf")), "redux_scale"),
           (dict(embeds_shape=(NP, J), scale=-0.5), "redux_scale must be finite and >= 0, got -0.5")]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            P.check_redux_request(**dict(ok, **kw))
    assert "redux" in P.REQUEST_NAMES and not any("redux" in row for row in F.REFUSED_PAIRS + F.REFUSED_MODES)  # it changes the text rows only: it combines


class _FakeTower:
    cfg, num_patches = dict(image_size=S), NP

    def __init__(self):
        self.seen = []

    def encode(self, img):
        self.seen.append(img)
        return torch.full((1, NP, 8), float(len(self.seen)))


class _FakeEmbedder:
    txt_dim = J

    def forward(self, h):
        return h[..., :1].expand(1, NP, J) * 2.0


class _Recording(P.Pipeline):
    """No GPU: the request path in front of the chunk body.  The chunk's text embeddings are rows of 1 (the prompts) and of 3 (the negative), T = 4."""
    def __init__(self, loaded=True):
        self.device, self._lock, self.chunks = torch.device("cpu"), threading.Lock(), []
        self.redux = (_FakeTower(), _FakeEmbedder()) if loaded else None

    def _chunk_embeddings(self, s, negative):
        B = len(s.prompts)
        neg = None if negative is None else (torch.full((B, 4, J), 3.0), torch.full((B, 8), 3.0))
        return torch.ones(B, 4, J), torch.ones(B, 8), neg

    def _generate_chunk(self, s, params, seed, strength, return_latents, cache_threshold, stats, **shared):
        self.chunks.append((s, shared))
        return torch.zeros((len(s.prompts), 3, params.height, params.width), dtype=torch.uint8)


def _params():
    return P.DiffusionGenerationParams(16, 16, 2, 3.5)


def test_a_picture_is_encoded_once_and_its_tokens_join_the_text_rows_of_every_chunk():
    pipe = _Recording()
    pic = np.zeros(U8, np.uint8)
    pipe.generate_tensor([f"p{i}" for i in range(11)], _params(), redux_image=pic, redux_scale=0.5)
    assert [len(s.prompts) for s, _ in pipe.chunks] == [8, 3] and len(pipe.redux[0].seen) == 1  # encoded once, whatever the number of chunks
    for s, shared in pipe.chunks:
        t5, clip = s.embeddings
        B = len(s.prompts)
        assert shared == {} and s.token_ids is None and tuple(t5.shape) == (B, 4 + NP, J) and tuple(clip.shape) == (B, 8)
        assert torch.equal(t5[:, :4], torch.ones(B, 4, J)) and torch.equal(t5[:, 4:], torch.full((B, NP, J), 1.0))  # 0.5 * (2 * 1): the scale is applied
    # the embedding instead of the picture: no encoder call; (Np,J) and (1,Np,J) alike; scale 0 still appends rows, of zeros
    for emb, scale, want in ((np.full((NP, J), 4.0, np.float32), 1.0, 4.0), (torch.full((1, NP, J), 4.0), 0.25, 1.0), (torch.full((1, NP, J), 4.0), 0.0, 0.0)):
        pipe = _Recording()
        pipe.generate_tensor(["a", "b"], _params(), redux_image_embeds=emb, redux_scale=scale)
        t5 = pipe.chunks[0][0].embeddings[0]
        assert pipe.redux[0].seen == [] and tuple(t5.shape) == (2, 4 + NP, J) and torch.equal(t5[:, 4:], torch.full((2, NP, J), want))
    # under a negative: both halves keep one T, the negative's rows end with ZERO rows in place of the tokens; MAX_BATCH // 2 prompts per call
    pipe = _Recording()
    pipe.generate_tensor([f"p{i}" for i in range(5)], _params(), redux_image=torch.zeros(PV), negative_prompt="n", true_cfg_scale=2.0)
    assert [len(s.prompts) for s, _ in pipe.chunks] == [4, 1] and len(pipe.redux[0].seen) == 1 and pipe.redux[0].seen[0].dtype == torch.float32
    for s, shared in pipe.chunks:
        neg = shared["negative"]
        assert set(shared) == {"negative"} and neg.scale == 2.0 and neg.prompt is None and neg.token_ids is None
        assert tuple(neg.embeddings[0].shape) == (1, 4 + NP, J) and torch.equal(neg.embeddings[0][:, :4], torch.full((1, 4, J), 3.0))
        assert not neg.embeddings[0][:, 4:].any() and torch.equal(neg.embeddings[1], torch.full((1, 8), 3.0))
        assert torch.equal(s.embeddings[0][:, 4:], torch.full((len(s.prompts), NP, J), 2.0))
    pipe = _Recording()
    pipe.generate_tensor(["a"], _params())  # no Redux argument: no encoder call, the chunk as the caller gave it — the call of before
    assert pipe.redux[0].seen == [] and pipe.chunks[0][1] == {} and pipe.chunks[0][0].embeddings is None


def test_request_refusals_without_a_device():
    pic, emb = np.zeros(U8, np.uint8), np.zeros((NP, J), np.float32)
    for pipe, kw, msg in ((_Recording(loaded=False), dict(redux_image=pic), "needs a loaded Redux"), (_Recording(loaded=False), dict(redux_image_embeds=emb), "needs a loaded Redux"),
                          (_Recording(), dict(redux_image=pic, redux_image_embeds=emb), "exclude one another"),
                          (_Recording(), dict(redux_image_embeds=np.zeros((NP, J + 1), np.float32)), "redux_image_embeds= must be"),
                          (_Recording(), dict(redux_image_embeds=np.zeros((NP, J), np.int32)), "redux_image_embeds must be a float"),
                          (_Recording(), dict(redux_image=np.zeros((4, 4), np.uint8)), "redux_image= must be"),
                          (_Recording(), dict(redux_image=[[1, 2]]), "redux_image must be a numpy array or a torch tensor"),
                          (_Recording(), dict(redux_image=pic, redux_scale=float("nan")), "redux_scale"), (_Recording(), dict(redux_image=pic, redux_scale=-1.0), "redux_scale")):
        with pytest.raises(ValueError, match=msg):
            pipe.generate_tensor(["a"], _params(), **kw)
        assert pipe.chunks == [] and (pipe.redux is None or pipe.redux[0].seen == [])  # refused before anything is encoded
    pipe = _Recording()
    pipe._sp = object()
    for kw in (dict(redux_image=pic), dict(redux_image_embeds=emb)):
        with pytest.raises(ValueError, match=r"Redux \(redux_image= / redux_image_embeds=\) is not supported under sequence parallelism"):
            pipe.generate_tensor(["a"], _params(), **kw)
    assert pipe.chunks == [] and pipe.redux[0].seen == []
    with pytest.raises(ValueError, match="encode_redux_image needs a loaded Redux"):
        _Recording(loaded=False).encode_redux_image(pic)
    with pytest.raises(ValueError, match="image must be a uint8"):
        _Recording().encode_redux_image(np.zeros((1, 3, S, S + 2), np.float32))


def test_signatures_append_the_keywords_and_the_chunk_body_does_not_know_redux():
    for fn in (P.Pipeline.forward, P.Pipeline.generate_tensor):
        p = inspect.signature(fn).parameters
        names = [n for n in p if n != "kw"]
        assert names[-3:] == ["redux_image", "redux_image_embeds", "redux_scale"] and names[-4] == "negative_ip_adapter_image"
        assert (p["redux_image"].default, p["redux_image_embeds"].default, p["redux_scale"].default) == (None, None, 1.0)
    assert not any("redux" in n for n in inspect.signature(P.Pipeline._generate_chunk).parameters)
    assert [f.name for f in dataclasses.fields(P._ReduxInput)] == ["tokens"] and "redux" not in [f.name for f in dataclasses.fields(P._Samples)]
    assert all(hasattr(P.Pipeline, n) for n in ("load_redux", "unload_redux", "encode_redux_image"))
    assert "ZERO rows" in P.Pipeline.generate_tensor.__doc__  # the negative half's rule is stated where the keyword is
