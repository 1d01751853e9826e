"""CPU restatement of the CLIP vision encoder path, test infrastructure only: PIL's two-pass bicubic resize as the recipe of
include/flux_mi355x.h (fmi_resize_bicubic_u8), CLIP's centre crop + normalisation, and HuggingFace's CLIPVisionModelWithProjection — in float32, or float64
with dtype=np.float64.  tests/test_host_clip_vision.py pins the resize to committed PIL outputs and the tower to committed transformers outputs
(tests/golden/clip_vision.npz, written by tests/golden/gen_clip_vision_fixtures.py); tests/test_gpu_clip_vision.py holds the kernels to this file."""
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_vision.npz")

# the small towers of the tests: D = 128, 2 heads of 64, F = 256, 3 layers, projection 64
_SMALL = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, projection_dim=64)
CONFIGS = OrderedDict([
    ("s56p14", dict(_SMALL, image_size=56, patch_size=14)),    # T = 17: one ragged key block; K = 588 padded to 640
    ("s126p14", dict(_SMALL, image_size=126, patch_size=14)),  # T = 82: two key blocks, the second ragged
    ("s64p16", dict(_SMALL, image_size=64, patch_size=16)),    # T = 17; K = 768: no padding
])
WEIGHT_SEED = 11
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

# the resize cases at short edge 28: name -> ((h, w), (nh, nw), kind of input)
RESIZE_CASES = OrderedDict([
    ("down", ((31, 45), (28, 40), "noise")),
    ("tall", ((67, 45), (41, 28), "noise")),
    ("one_pass", ((28, 135), (28, 90), "noise")),  # height unchanged: the horizontal pass alone (not a shape CLIP's rule produces)
    ("noop", ((28, 90), (28, 90), "noise")),       # the short edge is 28 already: a copy
    ("up3", ((9, 13), (28, 40), "noise")),
    ("binary", ((33, 47), (28, 39), "binary")),
])


def state_dict(cfg, seed=WEIGHT_SEED):
    """Seeded synthetic weights of a tower, bf16-valued f32 numpy (diffusion_rs_amd.synth's rule for encoders)."""
    from diffusion_rs_amd import synth
    return synth.text_state_dict_numpy(synth.clip_vision_tensor_shapes(cfg), seed=seed)


def pixel_values(cfg, B, seed=3):
    """Seeded inputs of a tower: (B,3,S,S) f32, unit normal — the scale normalised pixels have."""
    S = cfg["image_size"]
    return np.random.default_rng(seed).standard_normal((B, 3, S, S)).astype(np.float32)


def picture(shape, kind="noise", seed=0):
    """A seeded u8 (h,w,3) test picture: uniform noise, or a binary 0 / 255 image of blocks (edges overshoot: the clamp between the passes matters)."""
    rng = np.random.default_rng(seed)
    h, w = shape
    if kind == "binary":
        coarse = rng.integers(0, 2, ((h + 4) // 5, (w + 4) // 5, 3))
        return (np.kron(coarse, np.ones((5, 5, 1), dtype=np.int64))[:h, :w] * 255).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ resize
def cubic(x, dtype=np.float32):
    """Keys' cubic at a = -0.5 (PIL's bicubic_filter)."""
    a = dtype(-0.5)
    x = np.abs(x).astype(dtype)
    near = ((a + dtype(2)) * x - (a + dtype(3))) * x * x + dtype(1)
    far = (((x - dtype(5)) * x + dtype(8)) * x - dtype(4)) * a
    return np.where(x < 1, near, np.where(x < 2, far, dtype(0))).astype(dtype)


def resize_weights(n_in, n_out, dtype=np.float32):
    """(n_out, n_in) weights of one pass (PIL's precompute_coeffs): row o is zero outside [lo, hi) and sums to 1."""
    scale = dtype(n_in) / dtype(n_out)
    fs = max(scale, dtype(1))
    support = dtype(2) * fs
    W = np.zeros((n_out, n_in), dtype)
    for o in range(n_out):
        center = (dtype(o) + dtype(0.5)) * scale
        lo = max(0, int(center - support + dtype(0.5)))
        hi = min(n_in, int(center + support + dtype(0.5)))
        j = np.arange(lo, hi).astype(dtype)
        w = cubic((j - center + dtype(0.5)) / fs, dtype)
        W[o, lo:hi] = w / w.sum(dtype=dtype)
    return W


def resize_bicubic_u8(img, nh, nw, dtype=np.float32):
    """u8 (h,w,3) -> u8 (nh,nw,3): horizontal pass, then vertical, each rounded to nearest and clamped to [0, 255]; a pass whose size stays is skipped."""
    h, w, _ = img.shape
    out = img
    if nw != w:
        out = np.clip(np.rint(np.einsum("ow,hwc->hoc", resize_weights(w, nw, dtype), out.astype(dtype))), 0, 255).astype(np.uint8)
    if nh != h:
        out = np.clip(np.rint(np.einsum("oh,hwc->owc", resize_weights(h, nh, dtype), out.astype(dtype))), 0, 255).astype(np.uint8)
    return out.copy() if out is img else out


def resize_shape(h, w, size):
    """CLIP's resize target: shortest edge -> size, the long one int(size * long / short) (transformers' get_resize_output_image_size)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def preprocess(img, S, mean=CLIP_MEAN, std=CLIP_STD, dtype=np.float32):
    """u8 (nh,nw,3) -> (3,S,S): centre crop at ((nh - S) // 2, (nw - S) // 2), then (v / 255 - mean) / std, three operations in dtype."""
    nh, nw, _ = img.shape
    top, left = (nh - S) // 2, (nw - S) // 2
    v = img[top:top + S, left:left + S].astype(dtype).transpose(2, 0, 1)
    m, s = np.asarray(mean, dtype).reshape(3, 1, 1), np.asarray(std, dtype).reshape(3, 1, 1)
    return ((v / dtype(255)) - m) / s


def image_processor(img, S, mean=CLIP_MEAN, std=CLIP_STD, dtype=np.float32):
    """CLIPImageProcessor: a u8 picture of any size -> pixel_values (1,3,S,S)."""
    nh, nw = resize_shape(img.shape[0], img.shape[1], S)
    return preprocess(resize_bicubic_u8(img, nh, nw, dtype), S, mean, std, dtype)[None].astype(np.float32)


# ------------------------------------------------------------------------------------------------- tower
def _layernorm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def tail(sd, hidden, dtype=np.float32):
    """image_embeds from the encoder's output: post_layernorm of the class row, visual_projection (no bias)."""
    g = lambda k: sd[k].astype(dtype)
    cls = _layernorm(hidden[:, 0].astype(dtype), g("vision_model.post_layernorm.weight"), g("vision_model.post_layernorm.bias"))
    return cls @ g("visual_projection.weight").T


def vision_forward(sd, cfg, pix, dtype=np.float32):
    """CLIPVisionModelWithProjection.forward on numpy weights: (image_embeds (B,E), last_hidden_state (B,T,D)) in dtype."""
    g = lambda k: sd[k].astype(dtype)
    D, H, P, S = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"], cfg["image_size"]
    B, G = pix.shape[0], S // P
    vm = "vision_model."
    # the stride-P convolution: patches in (c, py, px) order against the flattened weight
    patches = pix.astype(dtype).reshape(B, 3, G, P, G, P).transpose(0, 2, 4, 1, 3, 5).reshape(B, G * G, 3 * P * P)
    emb = patches @ g(vm + "embeddings.patch_embedding.weight").reshape(D, -1).T
    x = np.concatenate([np.broadcast_to(g(vm + "embeddings.class_embedding"), (B, 1, D)), emb], 1) + g(vm + "embeddings.position_embedding.weight")[None]
    x = _layernorm(x, g(vm + "pre_layrnorm.weight"), g(vm + "pre_layrnorm.bias"))
    T = x.shape[1]
    for l in range(cfg["num_hidden_layers"]):
        p = vm + f"encoder.layers.{l}."
        n = _layernorm(x, g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"))
        q, k, v = ((n @ g(p + f"self_attn.{m}_proj.weight").T + g(p + f"self_attn.{m}_proj.bias")).reshape(B, T, H, 64).transpose(0, 2, 1, 3) for m in "qkv")
        s = (q * dtype(0.125)) @ k.transpose(0, 1, 3, 2)
        s = np.exp(s - s.max(-1, keepdims=True))
        a = ((s / s.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(B, T, D)
        x = x + a @ g(p + "self_attn.out_proj.weight").T + g(p + "self_attn.out_proj.bias")
        n = _layernorm(x, g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"))
        h = n @ g(p + "mlp.fc1.weight").T + g(p + "mlp.fc1.bias")
        h = h / (1 + np.exp(dtype(-1.702) * h))  # quick-GELU
        x = x + h @ g(p + "mlp.fc2.weight").T + g(p + "mlp.fc2.bias")
    return tail(sd, x, dtype), x


_CACHE = {}


def reference(name, B, dtype=np.float32):
    """(image_embeds, last_hidden_state) of config `name` on its seeded weights and inputs, computed once per process and shared by the tests: do not write to it."""
    key = (name, B, np.dtype(dtype).name)
    if key not in _CACHE:
        cfg = CONFIGS[name]
        _CACHE[key] = vision_forward(state_dict(cfg), cfg, pixel_values(cfg, B), dtype)
    return _CACHE[key]
