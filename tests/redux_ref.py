"""CPU restatement of the FLUX.1 Redux path, test infrastructure only: SigLIP's image processor (PIL's bicubic resize straight to S x S
through clip_vision_ref.resize_bicubic_u8, then (v / 255 - 0.5) / 0.5), HuggingFace's SiglipVisionModel.last_hidden_state and diffusers' ReduxImageEncoder — in
float32, or float64 with dtype=np.float64.  tests/test_host_redux.py pins the tower to committed transformers outputs and the direct-to-square resize to
committed PIL outputs (tests/golden/siglip_redux.npz, written by tests/golden/gen_siglip_redux_fixtures.py); tests/test_gpu_redux.py holds the kernels to this
file."""
import os
from collections import OrderedDict

import numpy as np

from tests.clip_vision_ref import picture, resize_bicubic_u8  # noqa: F401  (the resize recipe and the test pictures are the CLIP path's)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "siglip_redux.npz")

# the small towers of the tests: the smallest at which each mechanism can still go wrong
_H72 = dict(hidden_size=576, intermediate_size=1076, num_hidden_layers=2, num_attention_heads=8, layer_norm_eps=1e-6)
CONFIGS = OrderedDict([
    ("h72_t16", dict(_H72, image_size=56, patch_size=14)),   # head dim 72 padded to 128, F 1076 padded to 1088, one KV tile, K 588 padded to 640
    ("h72_t81", dict(_H72, image_size=126, patch_size=14)),  # 81 keys: two KV tiles, the second ragged (the streaming attention kernel)
    ("h64_t16", dict(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, layer_norm_eps=1e-6, image_size=64, patch_size=16)),
    # ^ head dim 64, no F padding, K = 768: no padding
    ("h64_t9", dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, layer_norm_eps=1e-6, image_size=50, patch_size=16)),
    # ^ image_size no multiple of patch_size, as 384 / 14 of the real tower: 3 patches per side, the last 2 rows and columns of the picture are not read
])
WEIGHT_SEED = 13
REDUX_SEED = 17
REDUX_J = 256  # the embedder of the tests: up (768, D), down (256, 768)
SIGLIP_MEAN = (0.5, 0.5, 0.5)
SIGLIP_STD = (0.5, 0.5, 0.5)

# the direct-to-square resize cases at S = 28: name -> ((h, w), kind of input, picture seed)
RESIZE_CASES = OrderedDict([
    ("down", ((31, 45), "noise", 200)),
    ("tall", ((67, 45), "noise", 201)),
    ("up3", ((9, 13), "noise", 202)),
    ("binary", ((33, 47), "binary", 203)),
])
RESIZE_S = 28


def num_patches(cfg):
    return (cfg["image_size"] // cfg["patch_size"]) ** 2


def state_dict(cfg, seed=WEIGHT_SEED):
    """Seeded synthetic weights of a tower, bf16-valued f32 numpy (diffusion_rs_amd.synth's rule for encoders)."""
    from diffusion_rs_amd import synth
    return synth.text_state_dict_numpy(synth.siglip_vision_tensor_shapes(cfg), seed=seed)


def redux_state_dict(D, J=REDUX_J, seed=REDUX_SEED):
    """Seeded synthetic weights of a Redux embedder, bf16-valued f32 numpy."""
    from diffusion_rs_amd import synth
    return synth.text_state_dict_numpy(synth.redux_tensor_shapes(D, J), seed=seed)


def pixel_values(cfg, B, seed=3):
    """Seeded inputs of a tower: (B,3,S,S) f32, unit normal — the scale normalised pixels have."""
    S = cfg["image_size"]
    return np.random.default_rng(seed).standard_normal((B, 3, S, S)).astype(np.float32)


def image_processor(img, S, mean=SIGLIP_MEAN, std=SIGLIP_STD, dtype=np.float32):
    """SiglipImageProcessor: a u8 picture of any size -> pixel_values (1,3,S,S): resized straight to S x S (no aspect rule, no crop), then (v / 255 - mean) /
    std as three operations in dtype."""
    v = resize_bicubic_u8(img, S, S, dtype).astype(dtype).transpose(2, 0, 1)
    m, s = np.asarray(mean, dtype).reshape(3, 1, 1), np.asarray(std, dtype).reshape(3, 1, 1)
    return (((v / dtype(255)) - m) / s)[None].astype(np.float32)


def _layernorm(x, w, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def gelu_tanh(x, dtype=np.float32):
    """gelu_pytorch_tanh: 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)))"""
    return dtype(0.5) * x * (dtype(1) + np.tanh(dtype(np.sqrt(2.0 / np.pi)) * (x + dtype(0.044715) * x * x * x)))


def siglip_forward(sd, cfg, pix, dtype=np.float32):
    """SiglipVisionModel.forward(...).last_hidden_state on numpy weights: (B, Np, D) in dtype — post_layernorm of every row; no class token, no pre-LayerNorm."""
    g = lambda k: sd[k].astype(dtype)
    D, H, P, S, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"], cfg["image_size"], dtype(cfg["layer_norm_eps"])
    B, G, hd = pix.shape[0], S // P, D // H
    vm = "vision_model."
    # the stride-P convolution has no padding: G = S // P patches per side, the pixels past G P are not read; patches in (c, py, px) order
    patches = pix.astype(dtype)[:, :, :G * P, :G * P].reshape(B, 3, G, P, G, P).transpose(0, 2, 4, 1, 3, 5).reshape(B, G * G, 3 * P * P)
    x = patches @ g(vm + "embeddings.patch_embedding.weight").reshape(D, -1).T + g(vm + "embeddings.patch_embedding.bias")
    x = x + g(vm + "embeddings.position_embedding.weight")[None]
    T = x.shape[1]
    scale = dtype(hd ** -0.5)
    for l in range(cfg["num_hidden_layers"]):
        p = vm + f"encoder.layers.{l}."
        n = _layernorm(x, g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"), eps)
        q, k, v = ((n @ g(p + f"self_attn.{m}_proj.weight").T + g(p + f"self_attn.{m}_proj.bias")).reshape(B, T, H, hd).transpose(0, 2, 1, 3) for m in "qkv")
        s = (q @ k.transpose(0, 1, 3, 2)) * scale
        s = np.exp(s - s.max(-1, keepdims=True))
        a = ((s / s.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(B, T, D)
        x = x + a @ g(p + "self_attn.out_proj.weight").T + g(p + "self_attn.out_proj.bias")
        n = _layernorm(x, g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"), eps)
        h = gelu_tanh(n @ g(p + "mlp.fc1.weight").T + g(p + "mlp.fc1.bias"), dtype)
        x = x + h @ g(p + "mlp.fc2.weight").T + g(p + "mlp.fc2.bias")
    return _layernorm(x, g(vm + "post_layernorm.weight"), g(vm + "post_layernorm.bias"), eps).astype(dtype)


def redux_forward(rsd, hidden, scale=1.0, dtype=np.float32):
    """ReduxImageEncoder: scale * redux_down(silu(redux_up(hidden))), (.., D) -> (.., J) in dtype."""
    g = lambda k: rsd[k].astype(dtype)
    u = hidden.astype(dtype) @ g("redux_up.weight").T + g("redux_up.bias")
    u = u / (dtype(1) + np.exp(-u))
    return dtype(scale) * (u @ g("redux_down.weight").T + g("redux_down.bias"))


_CACHE = {}


def reference(name, B, dtype=np.float32):
    """last_hidden_state of config `name` on its seeded weights and inputs, computed once per process and shared by the tests: read-only."""
    key = (name, B, np.dtype(dtype).name)
    if key not in _CACHE:
        cfg = CONFIGS[name]
        out = siglip_forward(state_dict(cfg), cfg, pixel_values(cfg, B), dtype)
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]
