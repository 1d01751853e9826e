"""Host-side mirror of the reference's text encoders over the C-ABI:

    T5EncoderModel        <-> diffusion_rs_core::models::t5::T5EncoderModel        (t5/mod.rs:609-632)
    ClipTextTransformer   <-> diffusion_rs_core::models::clip::text::ClipTextTransformer (clip/text.rs:243-317)
    ClipVisionModel       <-> HuggingFace's CLIPVisionModelWithProjection + CLIPImageProcessor (not in the reference)
    SiglipVisionModel     <-> HuggingFace's SiglipVisionModel.last_hidden_state + SiglipImageProcessor (not in the reference)
    ReduxImageEmbedder    <-> diffusers' ReduxImageEncoder (not in the reference)
    tokenize_and_pad      <-> FluxPipeline::tokenize_and_pad (pipelines/flux/mod.rs:202-221)
    load_bpe_tokenizer    <-> diffusion_rs_common::load_bpe_tokenizer (tokenizer.rs:7-23)

Same constructor configs (the JSON keys of text_encoder{,_2}/config.json), same tensor names, same
forward contracts; compute is the HIP library only (no CPU fallback).
"""
import ctypes as C
import json
from typing import List, Sequence

import torch

from . import _lib as L
from .flux import _ptr, _stream, _tensor_arg

T5_XXL = dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, relative_attention_num_buckets=32,
              relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
CLIP_L = dict(vocab_size=49408, projection_dim=768, intermediate_size=3072, max_position_embeddings=77, num_hidden_layers=12, num_attention_heads=12)
_T5_ACT = {"relu": 0, "gated-gelu": 1, "gated-silu": 2}
# openai/clip-vit-large-patch14's vision tower and its image processor's constants (preprocessor_config.json)
CLIP_VISION_L = dict(image_size=224, patch_size=14, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, projection_dim=768)
CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)
# google/siglip-so400m-patch14-384's vision tower (the image encoder of FLUX.1 Redux) and its image processor's constants
SIGLIP_SO400M = dict(image_size=384, patch_size=14, hidden_size=1152, intermediate_size=4304, num_hidden_layers=27, num_attention_heads=16, layer_norm_eps=1e-6)
SIGLIP_IMAGE_MEAN = (0.5, 0.5, 0.5)
SIGLIP_IMAGE_STD = (0.5, 0.5, 0.5)


def _as_tensor(x):
    """A tensor as it is, anything else (a numpy array) through torch.from_numpy."""
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(x)


class _Encoder:
    _kind = ""

    def _open(self, device, create_fn, *args):
        """The constructor steps every handle shares: the library, the device, and the handle that the library's `create_fn(*args, &handle)` makes."""
        self.lib = L.load()
        L.check(self.lib.fmi_init(device), self.lib)
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        L.check(getattr(self.lib, create_fn)(*args, C.byref(h)), self.lib)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, f"fmi_{self._kind}_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tensor(self, name, t):
        p, dt, shape, keep = _tensor_arg(t)
        sh = (C.c_int64 * len(shape))(*shape)
        L.check(getattr(self.lib, f"fmi_{self._kind}_set_tensor")(self.h, name.encode(), p, dt, sh, len(shape)))

    def missing(self) -> List[str]:
        n = getattr(self.lib, f"fmi_{self._kind}_missing_count")(self.h)
        return [getattr(self.lib, f"fmi_{self._kind}_missing_name")(self.h, i).decode() for i in range(n)]

    def load_state_dict(self, tensors: dict, strict_extra: bool = False):
        """Feeds every tensor the model knows; unknown names are ignored unless strict_extra
        (checkpoints carry e.g. the T5 decoder-tied `encoder.embed_tokens.weight`)."""
        known = self.tensor_names()
        for k, v in tensors.items():
            if k in known:
                self.set_tensor(k, v)
            elif strict_extra:
                raise L.FmiError(f"unexpected tensor {k}")
        m = self.missing()
        if m:
            raise L.FmiError(f"{len(m)} {self._kind} tensors missing, e.g. {m[0]}")

    def size_in_bytes(self) -> int:
        return getattr(self.lib, f"fmi_{self._kind}_size_in_bytes")(self.h)

    @staticmethod
    def _ids(ids, device):
        t = torch.as_tensor(ids)
        if t.dim() != 2:
            raise L.FmiError("input_ids must be (batch, seq)")
        return t.to(device=device, dtype=torch.int32).contiguous()


class T5EncoderModel(_Encoder):
    _kind = "t5"

    def __init__(self, cfg: dict = None, device: int = 0):
        cfg = dict(T5_XXL if cfg is None else cfg)
        # `quantization_config` (bitsandbytes nf4 / fp4 / LLM.int8, t5/mod.rs:85-90): the quantised Linears arrive through
        # set_linear_bnb4 / set_linear_int8 (loader.load_text_encoder); nothing to configure up front
        self.cfg = cfg
        c = L.T5Config(cfg["vocab_size"], cfg["d_model"], cfg["d_kv"], cfg["d_ff"], cfg["num_layers"], cfg["num_heads"], cfg["relative_attention_num_buckets"],
                       cfg.get("relative_attention_max_distance", 128), cfg["layer_norm_epsilon"], _T5_ACT[cfg.get("feed_forward_proj", "relu")])
        self._open(device, "fmi_t5_create", C.byref(c))

    def tensor_names(self):
        from . import synth
        return synth.t5_tensor_shapes(self.cfg)

    def set_linear_bnb4(self, prefix: str, packed, absmax, blocksize: int, quant_type: str, out_features: int, in_features: int):
        """A bitsandbytes 4-bit Linear of the encoder (BnbLinear::linear_b, bitsandbytes/mod.rs:137-239; used by every T5 Linear
        when text_encoder_2/config.json carries a quantization_config, t5/mod.rs:132-173,258-261): packed codes (u8, n/2) +
        f32 absmax (n/blocksize), quant_type "nf4" | "fp4"."""
        pk = packed.to(device=self.device, dtype=torch.uint8).contiguous()
        am = absmax.to(device=self.device, dtype=torch.float32).contiguous()
        L.check(self.lib.fmi_t5_set_linear_bnb4(self.h, prefix.encode(), _ptr(pk), _ptr(am), int(blocksize), {"fp4": 1, "nf4": 2}[quant_type], int(out_features),
                                                int(in_features)))

    def set_linear_int8(self, prefix: str, weight, scb, out_features: int, in_features: int):
        """An LLM.int8 Linear (BnbLinear::Int8, bitsandbytes/mod.rs:104-134): int8 weight (out, in) + f32 SCB (out)."""
        w = weight.to(device=self.device, dtype=torch.int8).contiguous()
        sc = scb.to(device=self.device, dtype=torch.float32).contiguous()
        L.check(self.lib.fmi_t5_set_linear_int8(self.h, prefix.encode(), _ptr(w), _ptr(sc), int(out_features), int(in_features)), self.lib)

    def forward(self, input_ids, dtype=torch.bfloat16):
        """== T5EncoderModel::forward: ids (B,T) -> hidden states (B,T,d_model) in the model dtype."""
        ids = self._ids(input_ids, self.device)
        B, T = ids.shape
        out = torch.empty((B, T, self.cfg["d_model"]), dtype=dtype, device=self.device)
        L.check(self.lib.fmi_t5_forward(self.h, _ptr(ids), B, T, _ptr(out), L.BF16 if dtype == torch.bfloat16 else L.F32, _stream()), self.lib)
        return out


class ClipTextTransformer(_Encoder):
    _kind = "clip"

    def __init__(self, cfg: dict = None, device: int = 0):
        cfg = dict(CLIP_L if cfg is None else cfg)
        self.cfg = cfg
        c = L.ClipConfig(cfg["vocab_size"], cfg["projection_dim"], cfg["intermediate_size"], cfg["max_position_embeddings"], cfg["num_hidden_layers"],
                         cfg["num_attention_heads"])
        self._open(device, "fmi_clip_create", C.byref(c))

    def tensor_names(self):
        from . import synth
        return synth.clip_tensor_shapes(self.cfg)

    def forward(self, input_ids, return_hidden: bool = False):
        """== ClipTextTransformer::forward: ids (B,T) -> pooled (B,dim) f32 = final hidden state at argmax(id)."""
        ids = self._ids(input_ids, self.device)
        B, T = ids.shape
        D = self.cfg["projection_dim"]
        pooled = torch.empty((B, D), dtype=torch.float32, device=self.device)
        hid = torch.empty((B, T, D), dtype=torch.float32, device=self.device) if return_hidden else None
        L.check(self.lib.fmi_clip_forward(self.h, _ptr(ids), B, T, _ptr(pooled), L.F32, _ptr(hid) if hid is not None else None, _stream()), self.lib)
        return (pooled, hid) if return_hidden else pooled


def clip_resize_shape(h: int, w: int, size: int):
    """(nh, nw) of CLIP's resize: the shortest edge becomes `size`, the long one int(size * long / short) — transformers' get_resize_output_image_size with
    default_to_square=False, Python's float division and truncation included."""
    if h <= 0 or w <= 0 or size <= 0:
        raise ValueError(f"an image of {h} x {w} cannot be resized to a shortest edge of {size}")
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    return (new_long, size) if w <= h else (size, new_long)


def clip_crop_offsets(nh: int, nw: int, size: int):
    """(top, left) of the centre crop of an (nh, nw) image to size x size: what fmi_clip_preprocess_u8 computes."""
    if nh < size or nw < size:
        raise ValueError(f"a centre crop to {size} x {size} needs an image of at least that size, got {nh} x {nw}")
    return (nh - size) // 2, (nw - size) // 2


class _VisionTower(_Encoder):
    """What the vision towers share: the image processor on the GPU (a bicubic resize to the tower's own shape, the centre crop to image_size, (v / 255 - mean) /
    std) and the checks of what goes into forward.  A tower adds its resize rule (`_resized`), its forward and its properties."""

    def _open_tower(self, device, cfg, image_mean, image_std, default_mean, default_std, create_fn, config):
        self.cfg = cfg
        self.image_mean = tuple(float(v) for v in (default_mean if image_mean is None else image_mean))
        self.image_std = tuple(float(v) for v in (default_std if image_std is None else image_std))
        if len(self.image_mean) != 3 or len(self.image_std) != 3:
            raise ValueError("image_mean and image_std hold one value per RGB channel")
        self._open(device, create_fn, C.byref(config))

    def _pixel_values(self, pixel_values):
        """forward's input, checked, as f32 (B,3,S,S) on the device."""
        S = self.cfg["image_size"]
        t = _as_tensor(pixel_values)
        if t.dim() != 4 or tuple(t.shape[1:]) != (3, S, S) or not t.is_floating_point():
            raise ValueError(f"pixel_values must be float (B,3,{S},{S}), got {t.dtype} {tuple(t.shape)}")
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    @staticmethod
    def _picture(image_u8):
        t = _as_tensor(image_u8)
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8:
            raise ValueError(f"a picture must be uint8 (H,W,3), got {t.dtype} {tuple(t.shape)}")
        return t

    def resize(self, image_u8, nh: int, nw: int):
        """u8 (h,w,3) -> u8 (nh,nw,3) on the device, PIL's Image.resize(BICUBIC) (fmi_resize_bicubic_u8)."""
        t = self._picture(image_u8).to(self.device).contiguous()
        out = torch.empty((int(nh), int(nw), 3), dtype=torch.uint8, device=self.device)
        L.check(self.lib.fmi_resize_bicubic_u8(_ptr(t), int(t.shape[0]), int(t.shape[1]), _ptr(out), int(nh), int(nw), _stream()), self.lib)
        return out

    def preprocess(self, image_u8):
        """The tower's image processor on the device: u8 (H,W,3) of any size -> pixel_values (1,3,S,S) f32 — resized to the tower's `_resized` shape, the centre
        crop to S x S (which takes everything where the resize went straight to the square), (v / 255 - mean) / std."""
        S = self.cfg["image_size"]
        t = self._picture(image_u8)
        nh, nw = self._resized(int(t.shape[0]), int(t.shape[1]))
        r = self.resize(t, nh, nw)
        out = torch.empty((1, 3, S, S), dtype=torch.float32, device=self.device)
        mean, std = (C.c_float * 3)(*self.image_mean), (C.c_float * 3)(*self.image_std)
        L.check(self.lib.fmi_clip_preprocess_u8(_ptr(r), nh, nw, S, mean, std, _ptr(out), _stream()), self.lib)
        return out

    def encode(self, image):
        """A u8 (H,W,3) picture, or float (B,3,S,S) pixel_values that are already preprocessed -> what forward returns, f32."""
        t = _as_tensor(image)
        return self.forward(self.preprocess(t) if t.dtype == torch.uint8 else t)


class ClipVisionModel(_VisionTower):
    """CLIP's vision tower with its projection and its image processor on the GPU: a picture -> image_embeds (1, projection_dim), what
    ip_adapter_image_embeds= takes.  cfg: HuggingFace's CLIPVisionConfig keys (CLIP_VISION_L by default); image_mean / image_std: the processor's constants."""
    _kind = "clip_vision"

    def __init__(self, cfg: dict = None, device: int = 0, image_mean=None, image_std=None):
        cfg = {k: int((CLIP_VISION_L if cfg is None else cfg)[k]) for k in CLIP_VISION_L}
        self._open_tower(device, cfg, image_mean, image_std, CLIP_IMAGE_MEAN, CLIP_IMAGE_STD, "fmi_clip_vision_create",
                         L.ClipVisionConfig(*(cfg[k] for k in CLIP_VISION_L)))

    @property
    def projection_dim(self) -> int:
        return self.cfg["projection_dim"]

    def tensor_names(self):
        from . import synth
        return synth.clip_vision_tensor_shapes(self.cfg)

    def _resized(self, h: int, w: int):
        """CLIPImageProcessor's resize: the shortest edge to S (clip_resize_shape); the centre crop does the rest."""
        return clip_resize_shape(h, w, self.cfg["image_size"])

    def forward(self, pixel_values, return_hidden: bool = False):
        """== CLIPVisionModelWithProjection.forward: pixel_values (B,3,S,S) float -> image_embeds (B,projection_dim) f32; with return_hidden also the encoder's
        output before post_layernorm, (B, 1 + (S / P)^2, hidden_size) f32 (HF's last_hidden_state)."""
        S, D = self.cfg["image_size"], self.cfg["hidden_size"]
        t = self._pixel_values(pixel_values)
        B, T = int(t.shape[0]), 1 + (S // self.cfg["patch_size"]) ** 2
        out = torch.empty((B, self.cfg["projection_dim"]), dtype=torch.float32, device=self.device)
        hid = torch.empty((B, T, D), dtype=torch.float32, device=self.device) if return_hidden else None
        L.check(self.lib.fmi_clip_vision_forward(self.h, _ptr(t), B, _ptr(out), L.F32, _ptr(hid) if hid is not None else None, _stream()), self.lib)
        return (out, hid) if return_hidden else out


class SiglipVisionModel(_VisionTower):
    """SigLIP's vision tower with its image processor on the GPU: a picture -> last_hidden_state (1, Np, hidden_size), what the Redux embedder
    reads.  cfg: HuggingFace's SiglipVisionConfig keys (SIGLIP_SO400M by default); image_mean / image_std: the processor's constants.  The pooling head of the
    checkpoint is not part of the model."""
    _kind = "siglip_vision"

    def __init__(self, cfg: dict = None, device: int = 0, image_mean=None, image_std=None):
        src = SIGLIP_SO400M if cfg is None else cfg
        cfg = {k: (float(src.get(k, 1e-6)) if k == "layer_norm_eps" else int(src[k])) for k in SIGLIP_SO400M}
        self._open_tower(device, cfg, image_mean, image_std, SIGLIP_IMAGE_MEAN, SIGLIP_IMAGE_STD, "fmi_siglip_vision_create",
                         L.SiglipVisionConfig(*(cfg[k] for k in SIGLIP_SO400M)))

    @property
    def hidden_size(self) -> int:
        return self.cfg["hidden_size"]

    @property
    def num_patches(self) -> int:
        return (self.cfg["image_size"] // self.cfg["patch_size"]) ** 2

    def tensor_names(self):
        from . import synth
        return synth.siglip_vision_tensor_shapes(self.cfg)

    def _resized(self, h: int, w: int):
        """SiglipImageProcessor's resize: straight to S x S (no aspect rule, no crop)."""
        return self.cfg["image_size"], self.cfg["image_size"]

    def forward(self, pixel_values, dtype=torch.float32):
        """== SiglipVisionModel.forward(...).last_hidden_state: pixel_values (B,3,S,S) float -> (B, Np, hidden_size) f32 (or bf16): post_layernorm of every row."""
        t = self._pixel_values(pixel_values)
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16")
        B = int(t.shape[0])
        out = torch.empty((B, self.num_patches, self.cfg["hidden_size"]), dtype=dtype, device=self.device)
        L.check(self.lib.fmi_siglip_vision_forward(self.h, _ptr(t), B, _ptr(out), L.F32 if dtype == torch.float32 else L.BF16, _stream()), self.lib)
        return out

    def poison_workspace(self, B: int = 1):
        """Test seam (fmi_siglip_vision_poison_workspace): the workspace of a batch of B, every byte 0xff — NaNs wherever a forward reads what it did not write."""
        L.check(self.lib.fmi_siglip_vision_poison_workspace(self.h, int(B), _stream()), self.lib)


class ReduxImageEmbedder(_Encoder):
    """diffusers' ReduxImageEncoder on the GPU: SigLIP hidden states (.., Np, redux_dim) -> image tokens (.., Np, txt_dim) =
    scale * redux_down(silu(redux_up(h)))."""
    _kind = "redux"

    def __init__(self, redux_dim: int = 1152, txt_dim: int = 4096, device: int = 0):
        self.redux_dim, self.txt_dim = int(redux_dim), int(txt_dim)
        self._open(device, "fmi_redux_create", self.redux_dim, self.txt_dim)

    def tensor_names(self):
        from . import synth
        return synth.redux_tensor_shapes(self.redux_dim, self.txt_dim)

    def forward(self, hidden, scale: float = 1.0, dtype=torch.float32):
        """hidden (.., redux_dim) float -> (.., txt_dim) f32 (or bf16)."""
        t = _as_tensor(hidden)
        if t.dim() < 2 or t.shape[-1] != self.redux_dim or not t.is_floating_point() or t.numel() == 0:
            raise ValueError(f"hidden must be float (.., {self.redux_dim}), got {t.dtype} {tuple(t.shape)}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16")
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        rows = t.numel() // self.redux_dim
        out = torch.empty(tuple(t.shape[:-1]) + (self.txt_dim,), dtype=dtype, device=self.device)
        L.check(self.lib.fmi_redux_forward(self.h, _ptr(t), rows, float(scale), _ptr(out), L.F32 if dtype == torch.float32 else L.BF16, _stream()), self.lib)
        return out


# ---------------------------------------------------------------------------------- tokenisation
def load_bpe_tokenizer(vocab_json: str, merges_txt: str):
    """CLIP tokenizer exactly as the reference builds it (tokenizer.rs:7-23): a bare BPE model from
    vocab + merges (first line of merges skipped, malformed lines dropped) with NO normalizer,
    pre-tokenizer or post-processor — so no <|startoftext|>/<|endoftext|> are added (SURVEY F-notes)."""
    from tokenizers import Tokenizer
    from tokenizers.models import BPE
    vocab = json.loads(vocab_json)
    merges = [tuple(x.split(" ")) for x in merges_txt.split("\n")[1:]]
    merges = [m for m in merges if len(m) == 2]
    return Tokenizer(BPE(vocab, merges))


def tokenize_and_pad(prompts: Sequence[str], tokenizer) -> List[List[int]]:
    """FluxPipeline::tokenize_and_pad (flux/mod.rs:202-221): encode_batch(add_special_tokens=True),
    zero-pad every row to the longest one."""
    rows = [e.ids for e in tokenizer.encode_batch(list(prompts), add_special_tokens=True)]
    n = max(len(r) for r in rows)
    return [r + [0] * (n - len(r)) for r in rows]
