"""Python mirror of the reference's front-door API (diffusion_rs_py/src/lib.rs:13-156 and
diffusion_rs_core/src/pipelines/mod.rs:24-33,110-270) over the MI355X hot path.

    ModelSource.ModelId(model_id) / ModelSource.DdufFile(file)
    DiffusionGenerationParams(height, width, num_steps, guidance_scale)
    ModelDType.{Auto,BF16,F16,F32}    Offloading.Full
    Pipeline(source, silent=False, token=None, revision=None, offloading=None, dtype=ModelDType.Auto)
    Pipeline.forward(prompts, params) -> list[bytes]   (PNG-encoded, as the pyo3 binding returns)

Scope: text encoders (when the checkpoint ships them), the denoise loop and the VAE
decode run on the GPU through the C-ABI.  Tokenisation needs the checkpoint's tokenizer files and
the `tokenizers` package; without them pass `token_ids=(t5_ids, clip_ids)` or precomputed
`embeddings=(t5_emb, clip_emb)` — a loaded checkpoint never falls back to made-up embeddings.  Only the
Synthetic source built without text encoders (the benchmark) derives deterministic placeholder
embeddings from the prompt text: only shapes matter there.  Extensions over the reference, all keyword-only:
`latents=` / `seed=` (the reference cannot be seeded), `embeddings=`, `token_ids=`, `output=`, and image-to-image / inpainting:
`image=` / `strength=` / `mask=` / `return_latents=` (the reference has neither).

Multi-GPU: when torch.distributed is initialised (one process per GPU), the constructor loads the
DiT on rank 0 only and broadcasts its weight arenas over RCCL (dist.broadcast_state), and `forward` shards the
prompts — prompt i runs on rank i % world — and gathers the images to rank 0 (other ranks return None).
"""
import enum
import hashlib
import inspect
import json
import os
import struct
import threading
import zlib
from dataclasses import dataclass, fields, replace
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import flux as F
from . import synth


class ModelDType(enum.Enum):  # diffusion_rs_py/src/lib.rs:37-44
    Auto = 0
    BF16 = 1
    F16 = 2
    F32 = 3
    F8E4M3 = 4  # extension (not in the reference): DiT block linears on the e4m3 MFMA, DESIGN.md §4.3
    I8 = 5      # extension: the int8 MFMA on the linears of flux.INT8_DEFAULT_MASK (all but the double blocks' MLP), DESIGN.md §4.3c


class Offloading(enum.Enum):  # lib.rs:13-17.  Accepted and ignored: 288 GB of HBM hold everything.
    Full = 0


class ModelSource:
    """diffusion_rs_common/src/model_source.rs:18-85 (+ a Synthetic source for offline benchmarks)."""

    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)

    @staticmethod
    def ModelId(model_id: str) -> "ModelSource":
        return ModelSource("model_id", model_id=model_id)

    from_model_id = ModelId

    def override_transformer_model_id(self, model_id: str) -> "ModelSource":  # model_source.rs:59-69
        if self.kind != "model_id":
            raise ValueError("Expected model ID for the model source")
        return ModelSource("model_id", model_id=self.model_id, transformer_model_id=model_id)

    def override_transformer_gguf(self, file: str) -> "ModelSource":
        """The transformer from a single GGUF file (llama.cpp's block quantisations, BFL or diffusers tensor naming); model_index.json, the
        scheduler, the VAE, the text encoders and the tokenizers still come from this source's directory.  override_transformer_model_id with a path that
        ends in .gguf is the same."""
        return self.override_transformer_model_id(file)

    def override_transformer_file(self, file: str, expand: bool = False) -> "ModelSource":
        """The transformer from a single .safetensors file (BFL or diffusers tensor naming, with or without `model.diffusion_model.`; F32 / F16 / BF16 or the 8-bit
        float dtypes F8_E4M3 / F8_E5M2, plain or "scaled"); model_index.json, the scheduler, the VAE, the text encoders and the tokenizers
        still come from this source's directory — also when the file is an all-in-one that carries its own.  fp8 Linears stay resident as codes; expand=True
        dequantises them at load into an ordinary bf16 model (LoRA, the 8-bit modes).  override_transformer_model_id with a path that ends in .safetensors
        is the same as expand=False."""
        src = self.override_transformer_model_id(file)
        if expand:
            src.transformer_expand = True
        return src

    @staticmethod
    def DdufFile(file: str) -> "ModelSource":
        return ModelSource("dduf", file=file)

    dduf = DdufFile

    @staticmethod
    def Synthetic(variant: str = "dev", seed: int = 0, flux_cfg: Optional[dict] = None, vae_cfg: Optional[dict] = None,
                  text_encoders: bool = False, t5_cfg: Optional[dict] = None, clip_cfg: Optional[dict] = None) -> "ModelSource":
        """Random-init weights of the named architecture generated on the GPU (no checkpoints offline).
        text_encoders=True also builds T5 / CLIP (T5-XXL: 9 GiB of bf16 weights)."""
        return ModelSource("synthetic", variant=variant, seed=seed, flux_cfg=flux_cfg, vae_cfg=vae_cfg, text_encoders=text_encoders,
                           t5_cfg=t5_cfg, clip_cfg=clip_cfg)

    def __repr__(self):
        if self.kind == "model_id":
            return f"model id: {self.model_id}"
        if self.kind == "dduf":
            return f"dduf file: {self.file}"
        return f"synthetic FLUX.1-{self.variant} (seed {self.seed})"


@dataclass
class DiffusionGenerationParams:  # pipelines/mod.rs:24-33
    height: int
    width: int
    num_steps: int
    guidance_scale: float

    def __repr__(self):
        return (f"DiffusionGenerationParams(height = {self.height}, width = {self.width}, num_steps = {self.num_steps}, "
                f"guidance_scale = {self.guidance_scale})")


def encode_png(rgb: np.ndarray) -> bytes:
    """(H,W,3) u8 -> PNG bytes (what `image.write_to(.., ImageFormat::Png)` produces in lib.rs:144-152)."""
    h, w, c = rgb.shape
    assert c == 3 and rgb.dtype == np.uint8
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


def placeholder_embeddings(prompts: Sequence[str], T: int, joint_dim: int, pooled_dim: int, device):
    """Deterministic stand-in for T5/CLIP outputs, for the Synthetic source without text encoders only."""
    t5, clip = [], []
    for p in prompts:
        seed = int.from_bytes(hashlib.sha256(p.encode()).digest()[:8], "little")
        g = torch.Generator(device="cpu")
        g.manual_seed(seed & 0x7FFFFFFFFFFFFFFF)
        t5.append(torch.randn((T, joint_dim), generator=g))
        clip.append(torch.randn((pooled_dim,), generator=g))
    return torch.stack(t5).to(device=device, dtype=torch.bfloat16), torch.stack(clip).to(device=device, dtype=torch.float32)


def img2img_timesteps(timesteps: Sequence[float], strength: float) -> list:
    """The part of a schedule an image-to-image run walks: with N = len(timesteps) - 1 steps, the last n_run = min(int(N * strength), N) of them
    (diffusers' expression, float truncation included: int(100 * 0.29) == 28), i.e. timesteps[N - n_run:].  The source is noised to the first value."""
    n = len(timesteps) - 1
    if not (0.0 < strength <= 1.0):
        raise ValueError(f"strength must be in (0, 1], got {strength}")
    n_run = min(int(n * strength), n)
    if n_run < 1:
        raise ValueError(f"strength {strength} leaves no step of {n} to run: raise strength or num_steps")
    return list(timesteps[n - n_run:])


def check_reference(t: torch.Tensor, B: int) -> torch.Tensor:
    """The shape rules of `reference=`, on any device: uint8 (Hr,Wr,3) / (n,Hr,Wr,3) or float (n,3,Hr,Wr), Hr and Wr multiples of 16 (whatever
    params.height / width are), n = 1 (broadcast) or B.  Returns the tensor with its batch dimension; ValueError otherwise."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("reference must be a numpy array or a torch tensor")
    if t.dtype == torch.uint8:
        t = t.unsqueeze(0) if t.dim() == 3 else t
        if t.dim() != 4 or t.shape[3] != 3:
            raise ValueError(f"a uint8 reference must be (B,Hr,Wr,3) or (Hr,Wr,3), got {tuple(t.shape)}")
        Hr, Wr = int(t.shape[1]), int(t.shape[2])
    elif t.is_floating_point():
        if t.dim() != 4 or t.shape[1] != 3:
            raise ValueError(f"a float reference must be (B,3,Hr,Wr), got {tuple(t.shape)}")
        Hr, Wr = int(t.shape[2]), int(t.shape[3])
    else:
        raise ValueError(f"reference must be uint8 or float, got {t.dtype}")
    if Hr <= 0 or Wr <= 0 or Hr % 16 or Wr % 16:
        raise ValueError(f"reference needs a height and width that are positive multiples of 16, got {Hr} x {Wr}")
    if t.shape[0] not in (1, B):
        raise ValueError(f"reference holds {t.shape[0]} samples for {B} prompts (one is broadcast)")
    return t


def _host_image(x, what: str) -> torch.Tensor:
    """One image input of a request (`what`: its keyword) as a tensor where it lies: a numpy array or a torch tensor, uint8 or float; ValueError otherwise.
    The caller's shape rule comes next, then Pipeline._device_image."""
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a numpy array or a torch tensor")
    if not (t.dtype == torch.uint8 or t.is_floating_point()):
        raise ValueError(f"{what} must be uint8 or float, got {t.dtype}")
    return t


# what a request calls the options and modes of flux.REFUSED_PAIRS / REFUSED_MODES (an 8-bit transformer: "fp8" / "int8")
REQUEST_NAMES = dict(context="reference= (a context)", control="a control (a channel-conditioned checkpoint: FLUX.1 Fill / Canny / Depth)",
                     true_cfg="true CFG (a negative with true_cfg_scale > 1)", cache="the step cache (cache_threshold= / cache_force=)", controlnet="a ControlNet",
                     ip_adapter="an IP-Adapter", redux="Redux (redux_image= / redux_image_embeds=)",
                     sequence_parallel="supported under sequence parallelism: disable_sequence_parallel() first",
                     fp8="supported on a transformer in the fp8 mode", int8="supported on a transformer in the int8 mode")


def _rows(x, idx):
    """Rows `idx` (a slice or a list of ints) of one per-sample input: a tensor, a numpy array, a list, or a pair (tuple) of those; None stays None."""
    if x is None:
        return None
    if isinstance(x, tuple):
        return tuple(_rows(m, idx) for m in x)
    if isinstance(idx, slice) or isinstance(x, np.ndarray):
        return x[idx]
    return x[torch.as_tensor(idx, dtype=torch.long)] if isinstance(x, torch.Tensor) else [x[i] for i in idx]


@dataclass
class _Samples:
    """The inputs of a request that hold one row per prompt — everything else of it (params, seed, strength, return_latents, cache_threshold) is shared by
    its prompts.  Chunking, the sequence-parallel split, rank sharding and the int8 calibration sample all select rows through take(), which walks
    these fields: a new per-sample input is one field here and one use in Pipeline._generate_chunk."""
    prompts: list
    sample_ids: list  # the Philox stream of each sample
    embeddings: Optional[tuple] = None  # (t5_emb, clip_emb)
    token_ids: Optional[tuple] = None  # (t5_ids, clip_ids)
    latents: Optional[torch.Tensor] = None
    image: Optional[torch.Tensor] = None  # in device form (Pipeline._source_image), like mask and reference
    mask: Optional[torch.Tensor] = None
    reference: Optional[torch.Tensor] = None

    def take(self, idx) -> "_Samples":
        return _Samples(**{f.name: _rows(getattr(self, f.name), idx) for f in fields(self)})

    def kwargs(self) -> dict:
        """generate_tensor's keyword arguments (the prompts are its first positional one)."""
        return {f.name: getattr(self, f.name) for f in fields(self) if f.name != "prompts"}


@dataclass(frozen=True)
class _Negative:
    """The negative prompt of a true-CFG request: ONE per request, shared by its prompts like strength — not a per-sample input, so no field
    of _Samples.  Exactly one of prompt / embeddings / token_ids is set; every chunk of the request receives this same object."""
    scale: float
    prompt: Optional[str] = None
    embeddings: Optional[tuple] = None  # (t5 (1,T,J), clip (1,P))
    token_ids: Optional[tuple] = None  # (t5 (1,T'), clip (1,.))


@dataclass(frozen=True)
class _Control:
    """The control of a request to a channel-conditioned model (FLUX.1 Fill / Canny / Depth): ONE per request, shared by its prompts like the
    negative — not a per-sample input, so no field of _Samples; every chunk and every rank of the request receives this same object and expands it to its rows.
    kind "control": image is the control image (a Canny edge map, a depth map); kind "fill": image is the picture to fill and mask says where (1 = fill)."""
    kind: str  # "control" | "fill"
    image: torch.Tensor  # (1,3,H,W) f32 in [-1,1], on the device
    mask: Optional[torch.Tensor] = None  # (1,H,W) f32, on the device; kind "fill" only


@dataclass(frozen=True)
class _ControlNetInput:
    """The ControlNet conditioning of a request: ONE per request, shared by its prompts like the negative and the control — not a per-sample
    input, so no field of _Samples; every chunk and every rank of the request receives this same object and expands it to its rows."""
    image: torch.Tensor  # (1,3,H,W) f32 in [-1,1], on the device
    scale: float         # controlnet_conditioning_scale
    start: float         # control_guidance_start
    end: float           # control_guidance_end


def check_controlnet_request(loaded: bool, height: int, width: int, image_shape=None, image_is_u8: bool = False, scale: float = 1.0, start: float = 0.0,
                             end: float = 1.0):
    """The ControlNet arguments of a request, checked without a device.  ValueError: controlnet_image= without a loaded ControlNet (Pipeline.load_controlnet); a
    height or width that is no multiple of 16; an image that is not u8 (H,W,3) or float (B,3,H,W) with B == 1 at the request's size (nothing is resized); a scale
    that is not finite; control_guidance_start / _end outside 0 <= start <= end <= 1.  A request without controlnet_image= is not conditioned, whatever is loaded."""
    if image_shape is None:
        return
    if not loaded:
        raise ValueError("controlnet_image= needs a loaded ControlNet: Pipeline.load_controlnet(path) first")
    if height % 16 or width % 16:
        raise ValueError(f"controlnet_image= needs height and width that are multiples of 16, got {height} x {width}")
    want = (height, width, 3) if image_is_u8 else (1, 3, height, width)
    if tuple(image_shape) != want:
        raise ValueError(f"controlnet_image must be uint8 ({height},{width},3) or float (1,3,{height},{width}) as params say, got {tuple(image_shape)}")
    if not np.isfinite(float(scale)):
        raise ValueError(f"controlnet_conditioning_scale must be finite, got {scale!r}")
    if not (0.0 <= float(start) <= float(end) <= 1.0):
        raise ValueError(f"control_guidance_start / control_guidance_end must satisfy 0 <= start <= end <= 1, got {start!r} / {end!r}")


@dataclass(frozen=True)
class _IpAdapterInput:
    """The image prompt of a request: ONE embedding per request, shared by its prompts like the negative and the controls — not a per-sample input;
    every chunk of the request receives this same object and expands it to its rows."""
    embeds: torch.Tensor                     # (1,E) f32, on the device
    negative_embeds: Optional[torch.Tensor]  # (1,E) f32 or None (zeros)
    scale: float                             # ip_adapter_scale
    start: float                             # ip_adapter_start, a step fraction
    end: float                               # ip_adapter_end


def check_ip_adapter_request(loaded: bool, embed_dim: int = 0, embeds_shape=None, negative_embeds_shape=None, scale: float = 1.0, start: float = 0.0, end: float = 1.0,
                             has_negative: bool = False, *, image_shape=None, image_is_u8: bool = False, negative_image_shape=None, negative_image_is_u8: bool = False,
                             encoder_dim: Optional[int] = None, encoder_image_size: int = 0):
    """The IP-Adapter arguments of a request, checked without a device.  ValueError: ip_adapter_image_embeds= without a loaded adapter (Pipeline.load_ip_adapter);
    negative_ip_adapter_image_embeds= without ip_adapter_image_embeds= or without a negative prompt; embeddings that are not (embed_dim,) or (1, embed_dim) — one per
    request, shared by its prompts; a scale that is not finite; ip_adapter_start / ip_adapter_end outside 0 <= start <= end <= 1.  A request without
    ip_adapter_image_embeds= is not conditioned, whatever is loaded.

    The keyword arguments are the picture form of the same prompt: image_shape / negative_image_shape (with *_is_u8) are the shapes of
    ip_adapter_image= / negative_ip_adapter_image=, encoder_dim the loaded image encoder's projection_dim (None: none loaded) and encoder_image_size its S.
    ValueError: a picture together with the embedding of the same side; a picture without a loaded adapter or without a loaded encoder
    (Pipeline.load_image_encoder); an encoder whose projection_dim is not the adapter's embed_dim; a picture that is not u8 (H,W,3) or float (1,3,S,S); a
    negative without a positive, or without a negative prompt.  Everything else is checked as for the embeddings the pictures become."""
    for img, emb, nm in ((image_shape, embeds_shape, "ip_adapter_image"), (negative_image_shape, negative_embeds_shape, "negative_ip_adapter_image")):
        if img is not None and emb is not None:
            raise ValueError(f"{nm}= and {nm}_embeds= exclude one another: a request has one image prompt")
    if image_shape is None and embeds_shape is None:
        if negative_embeds_shape is not None:
            raise ValueError("negative_ip_adapter_image_embeds= needs ip_adapter_image_embeds=")
        if negative_image_shape is not None:
            raise ValueError("negative_ip_adapter_image= needs ip_adapter_image= (or ip_adapter_image_embeds=)")
        return
    given = "ip_adapter_image" if image_shape is not None else "ip_adapter_image_embeds"
    if not loaded:
        raise ValueError(f"{given}= needs a loaded IP-Adapter: Pipeline.load_ip_adapter(path) first")
    if image_shape is not None or negative_image_shape is not None:
        nm = "ip_adapter_image" if image_shape is not None else "negative_ip_adapter_image"
        if encoder_dim is None:
            raise ValueError(f"{nm}= needs a loaded image encoder: Pipeline.load_image_encoder(path) first (or pass {nm}_embeds=)")
        if int(encoder_dim) != int(embed_dim):
            raise ValueError(f"the image encoder's projection_dim is {encoder_dim}, the IP-Adapter's embed_dim {embed_dim}: {nm}= cannot feed this adapter")
        S = int(encoder_image_size)
        for shp, u8, what in ((image_shape, image_is_u8, "ip_adapter_image"), (negative_image_shape, negative_image_is_u8, "negative_ip_adapter_image")):
            if shp is not None and not ((len(shp) == 3 and shp[2] == 3 and min(shp[:2]) > 0) if u8 else tuple(shp) == (1, 3, S, S)):
                raise ValueError(f"{what} must be a uint8 (H,W,3) picture of any size or float (1,3,{S},{S}) pixel_values, one per request, got {tuple(shp)}")
    if negative_image_shape is not None and not has_negative:
        raise ValueError("negative_ip_adapter_image= needs a negative prompt (true classifier-free guidance)")
    for shp, nm in ((embeds_shape, "ip_adapter_image_embeds"), (negative_embeds_shape, "negative_ip_adapter_image_embeds")):
        if shp is not None and tuple(shp) not in ((embed_dim,), (1, embed_dim)):
            raise ValueError(f"{nm} must be ({embed_dim},) or (1,{embed_dim}), one embedding per request, got {tuple(shp)}")
    if negative_embeds_shape is not None and not has_negative:
        raise ValueError("negative_ip_adapter_image_embeds= needs a negative prompt (true classifier-free guidance)")
    if not np.isfinite(float(scale)):
        raise ValueError(f"ip_adapter_scale must be finite, got {scale!r}")
    if not (0.0 <= float(start) <= float(end) <= 1.0):
        raise ValueError(f"ip_adapter_start / ip_adapter_end must satisfy 0 <= start <= end <= 1, got {start!r} / {end!r}")


@dataclass(frozen=True)
class _ReduxInput:
    """The Redux image tokens of a request: ONE picture per request, shared by its prompts like the negative — not a per-sample input, so no
    field of _Samples.  Redux changes the text rows only: a chunk of such a request becomes an embeddings= chunk whose T5 rows end with these tokens
    (Pipeline._generate_chunk_redux), and _generate_chunk never learns of it."""
    tokens: torch.Tensor  # (1, Np, J) f32 on the device, redux_scale already applied


def check_redux_request(loaded: bool, num_patches: int = 0, txt_dim: int = 0, image_size: int = 0, image_shape=None, image_is_u8: bool = False, embeds_shape=None,
                        scale: float = 1.0, sequence_parallel: bool = False):
    """The Redux arguments of a request, checked without a device.  ValueError: redux_image= / redux_image_embeds= without a loaded Redux (Pipeline.load_redux);
    both of them (a picture and its embedding exclude one another); a picture that is not u8 (H,W,3) of any size or float (1,3,S,S) pixel_values, S = image_size
    of the loaded tower; embeddings that are not (Np,J) or (1,Np,J), Np = num_patches, J = txt_dim; a redux_scale that is not finite or is negative; sequence
    parallelism.  A request without either is not conditioned, whatever is loaded."""
    if image_shape is None and embeds_shape is None:
        return
    if image_shape is not None and embeds_shape is not None:
        raise ValueError("redux_image= and redux_image_embeds= exclude one another: a request has one picture, or its embedding")
    given = "redux_image" if image_shape is not None else "redux_image_embeds"
    if not loaded:
        raise ValueError(f"{given}= needs a loaded Redux: Pipeline.load_redux(path) first")
    if sequence_parallel:
        raise ValueError(f"{REQUEST_NAMES['redux']} is not {REQUEST_NAMES['sequence_parallel']}")
    if image_shape is not None:
        shp, S = tuple(image_shape), image_size
        if not ((len(shp) == 3 and shp[2] == 3 and shp[0] > 0 and shp[1] > 0) if image_is_u8 else shp == (1, 3, S, S)):
            raise ValueError(f"redux_image= must be a uint8 (H,W,3) picture of any size or float (1,3,{S},{S}) pixel_values (one picture per request), got {shp}")
    else:
        shp = tuple(embeds_shape)
        if shp not in ((num_patches, txt_dim), (1, num_patches, txt_dim)):
            raise ValueError(f"redux_image_embeds= must be ({num_patches},{txt_dim}) or (1,{num_patches},{txt_dim}) (one picture per request, shared by its prompts), "
                             f"got {shp}")
    if not (np.isfinite(scale) and scale >= 0.0):
        raise ValueError(f"redux_scale must be finite and >= 0, got {scale!r}")


def control_kind(cond_channels: int) -> Optional[str]:
    """What a model's conditioning channels hold: 0 -> None, 64 -> "control" (the control image's latents), 320 -> "fill" (masked-image latents + 256 mask
    channels); ValueError for any other width (no pipeline builds such a condition)."""
    kinds = {0: None, 64: "control", 320: "fill"}
    if cond_channels not in kinds:
        raise ValueError(f"a model with {cond_channels} conditioning channels is neither FLUX.1 Canny / Depth (64) nor Fill (320): build the condition yourself "
                         f"and call FluxModel.denoise(control=)")
    return kinds[cond_channels]


def check_control_request(kind: Optional[str], height: int, width: int, image_shape=None, image_is_u8: bool = False, mask_shape=None):
    """The control arguments of a request, checked without a device (kind: control_kind of the model).  ValueError: control_image= / control_mask= on a plain
    model; a conditioned model without control_image=; control_mask= missing on a Fill model or given to a Canny / Depth model; a height or width that is no
    multiple of 16; an image that is not u8 (H,W,3) or float (1,3,H,W) at the request's size; a mask that is not (H,W)."""
    if kind is None:
        if image_shape is not None or mask_shape is not None:
            raise ValueError("control_image= / control_mask= need a channel-conditioned model (FLUX.1 Fill / Canny / Depth)")
        return
    if image_shape is None:
        raise ValueError(f"this model is conditioned on an image ({'FLUX.1 Fill' if kind == 'fill' else 'FLUX.1 Canny / Depth'}): control_image= is required")
    if kind == "fill" and mask_shape is None:
        raise ValueError("a Fill model needs control_mask= ((H,W), 1 = fill)")
    if kind != "fill" and mask_shape is not None:
        raise ValueError("control_mask= goes with a Fill model; a Canny / Depth model takes control_image= alone")
    if height % 16 or width % 16:
        raise ValueError(f"control_image= needs height and width that are multiples of 16, got {height} x {width}")
    want = (height, width, 3) if image_is_u8 else (1, 3, height, width)
    if tuple(image_shape) != want:
        raise ValueError(f"control_image must be uint8 ({height},{width},3) or float (1,3,{height},{width}) as params say, got {tuple(image_shape)}")
    if mask_shape is not None and tuple(mask_shape) != (height, width):
        raise ValueError(f"control_mask must be ({height},{width}) as params say, got {tuple(mask_shape)}")


def _index_sets(B: int, max_batch: int, one_by_one: bool) -> list:
    """The row sets a request of any B runs in (pipelines/mod.rs:241-270): chunks of max_batch, or single samples (sequence parallel: ONE image at a time)."""
    n = 1 if one_by_one else max_batch
    return [slice(a, a + n) for a in range(0, B, n)]


class Pipeline:
    """== diffusion_rs_core::Pipeline (pipelines/mod.rs:110-270) for FluxPipeline."""

    def __init__(self, source: ModelSource, silent: bool = False, token: Optional[str] = None, revision: Optional[str] = None,
                 offloading: Optional[Offloading] = None, dtype: ModelDType = ModelDType.Auto, *, device: int = 0):
        if dtype in (ModelDType.F16, ModelDType.F32):
            raise ValueError("this build computes in bf16 on MFMA (f32 accumulate); use ModelDType.Auto or BF16")
        self.silent = silent
        self.offloading = offloading
        self.device_index = device
        self.device = torch.device("cuda", device)
        self._lock = threading.Lock()  # Arc<Mutex<dyn ModelPipeline>>, pipelines/mod.rs:110-113
        self.last_cache_stats = []  # the step-cache stats of the last request (generate_tensor's cache_threshold=), one entry per denoise call
        self.scheduler = F.SchedulerConfig()
        self.t5 = self.clip = self.t5_tokenizer = self.clip_tokenizer = None
        self.source_kind = source.kind
        from . import dist as D
        rank, world = D.world()
        # multi-GPU: the DiT (98 % of the bytes) is materialised on rank 0 and broadcast as flat arenas; the VAE and
        # the text encoders are loaded / generated by every rank itself (same files, same seeds)
        self.load_stats = {}
        self._dit_loader = None  # loads the DiT into self.flux on this rank (used by rank 0, and by every rank when the flat state cannot travel)
        err = None
        try:
            if source.kind == "synthetic":
                fcfg = source.flux_cfg or (F.FLUX_DEV if source.variant == "dev" else F.FLUX_SCHNELL)
                vcfg = source.vae_cfg or F.VAE_FLUX
                self.flux = F.FluxModel(fcfg, device)
                self._dit_loader = lambda: synth.fill_flux_random_device(self.flux, seed=source.seed, device=self.device)
                if rank == 0:
                    self._dit_loader()
                self.vae = F.AutoEncoderKl(vcfg, device)
                # (a channel-conditioned model encodes its control image at every request: the encoder's weights too — the decoder's keep their values)
                synth.fill_vae_random_device(self.vae, seed=source.seed + 1, device=self.device, encoder=bool(self.flux.cond_channels))
                if source.variant != "dev":
                    self.scheduler = F.SchedulerConfig(shift=1.0, use_dynamic_shifting=False)
                if getattr(source, "text_encoders", False):
                    from . import text
                    self.t5 = text.T5EncoderModel(source.t5_cfg, device)
                    synth.fill_text_random_device(self.t5, seed=source.seed + 2, device=self.device)
                    self.clip = text.ClipTextTransformer(source.clip_cfg, device)
                    synth.fill_text_random_device(self.clip, seed=source.seed + 3, device=self.device)
            elif source.kind == "model_id":
                self._load_checkpoint(source.model_id, getattr(source, "transformer_model_id", None), load_dit=(rank == 0),
                                      transformer_expand=bool(getattr(source, "transformer_expand", False)))
            else:
                self._load_checkpoint(source.file, None, load_dit=(rank == 0))
        except Exception as e:  # a rank that fails here must not leave the others blocked in the broadcast below
            if world == 1:
                raise
            err = e
        if world > 1:
            D.agree_or_raise(err, "Pipeline load")
            try:
                self.load_stats["broadcast"] = D.broadcast_state(self.flux, self.device)
            except D.StateExportUnsupported as e:  # raised on EVERY rank (e.g. LLM.int8 matrices are not part of the flat state)
                err = None
                try:
                    if rank != 0:
                        self._dit_loader()
                except Exception as e2:
                    err = e2
                D.agree_or_raise(err, "per-rank DiT load")
                self.load_stats["broadcast"] = {"bytes": 0, "messages": 0, "seconds": 0.0, "fallback": f"every rank loaded the DiT itself ({e})"}
        if dtype == ModelDType.F8E4M3:
            self.flux.quantize_fp8()
        elif dtype == ModelDType.I8:
            # the int8 mode is CALIBRATED (round 6: per-channel smoothing, include/flux_mi355x.h fmi_flux_calibrate_int8): the statistics come from the first
            # request — four model evaluations across its schedule on its first prompt — so the weights are quantised there, not here (generate_tensor)
            self._int8_pending = True

    # Pipeline::load (pipelines/mod.rs:120-236) for a local diffusers directory or a DDUF file:
    # model_index.json -> FluxPipeline only; scheduler / transformer / vae components, plus text_encoder (CLIP),
    # text_encoder_2 (T5) and their tokenizers when the checkpoint ships them (flux/mod.rs:74-127).
    def _load_checkpoint(self, path: str, transformer_path: Optional[str], load_dit: bool = True, transformer_expand: bool = False):
        from . import loader
        fl = loader.FileLoader(path)
        class_name = fl.read_json("model_index.json").get("_class_name")
        loader.pipeline_conditioning(class_name)  # pipelines/mod.rs:146-149; Kontext, Control (Canny / Depth) and Fill have FluxPipeline's components
        sc = fl.read_json("scheduler/scheduler_config.json")
        self.scheduler = F.SchedulerConfig(sc["base_image_seq_len"], sc["base_shift"], sc["max_image_seq_len"], sc["max_shift"], sc["shift"],
                                           sc["use_dynamic_shifting"])
        if transformer_path and transformer_path.lower().endswith(".gguf"):
            # a GGUF transformer: the configuration comes from the file's shapes — a BFL file has no config.json — and must agree with the
            # base directory's transformer/config.json where there is one
            gg = loader.GgufFile(transformer_path)
            fcfg = loader.flux_config_from_gguf(gg, fl.read_json("transformer/config.json") if fl.has("transformer/config.json") else None)
            self._dit_loader = lambda: self.load_stats.update(loader.load_flux_gguf(self.flux, gg))
        elif transformer_path and transformer_path.lower().endswith(".safetensors"):
            # a single-file transformer, fp8 or not: the configuration comes from the file's shapes, as for GGUF
            sf = loader.SingleFile(transformer_path)
            fcfg = loader.flux_config_from_single_file(sf, fl.read_json("transformer/config.json") if fl.has("transformer/config.json") else None)
            self._dit_loader = lambda: self.load_stats.update(loader.load_flux_single_file(self.flux, sf, expand=transformer_expand))
        else:
            tl = loader.FileLoader(transformer_path) if transformer_path else fl  # ModelIdWithTransformer (model_source.rs:22-25)
            tc = tl.read_json("transformer/config.json")
            fcfg = dict(F.FLUX_DEV, **{k: tc[k] for k in ("in_channels", "out_channels", "pooled_projection_dim", "joint_attention_dim", "num_attention_heads",
                                                         "num_layers", "num_single_layers", "guidance_embeds") if k in tc})
            self._dit_loader = lambda: self.load_stats.update(loader.load_flux(self.flux, tl.tensors("transformer")))
        loader.check_conditioning_channels(class_name, fcfg["in_channels"], fcfg.get("out_channels"))  # the class and the embedder's width agree
        self.flux = F.FluxModel(fcfg, self.device_index)
        if load_dit:  # (multi-GPU: the other ranks receive the weight arenas, dist.broadcast_state)
            self._dit_loader()
        vc = fl.read_json("vae/config.json")
        vcfg = dict(F.VAE_FLUX, **{k: vc[k] for k in F.VAE_FLUX if k in vc})
        self.vae = F.AutoEncoderKl(vcfg, self.device_index)
        loader.load_vae(self.vae, fl.tensors("vae"))
        # text_encoder (CLIP) / text_encoder_2 (T5) + their tokenizers (flux/mod.rs:74-127), when the checkpoint ships them
        if fl.has("text_encoder/config.json") and fl.has("text_encoder_2/config.json"):
            from . import text
            cc = fl.read_json("text_encoder/config.json")
            # ClipTextConfig reads projection_dim as the hidden width (clip/text.rs:24-33); both are 768 for CLIP-L
            self.clip = text.ClipTextTransformer({k: cc[k] for k in text.CLIP_L}, self.device_index)
            loader.load_text_encoder(self.clip, fl.tensors("text_encoder"))
            tc2 = fl.read_json("text_encoder_2/config.json")
            t5cfg = {k: tc2[k] for k in text.T5_XXL if k in tc2}
            t5cfg["quantization_config"] = tc2.get("quantization_config")
            self.t5 = text.T5EncoderModel(t5cfg, self.device_index)
            loader.load_text_encoder(self.t5, fl.tensors("text_encoder_2"))
            try:
                from tokenizers import Tokenizer
                if fl.has("tokenizer/vocab.json") and fl.has("tokenizer/merges.txt"):
                    self.clip_tokenizer = text.load_bpe_tokenizer(fl.read_text("tokenizer/vocab.json"), fl.read_text("tokenizer/merges.txt"))
                if fl.has("tokenizer_2/tokenizer.json"):
                    self.t5_tokenizer = Tokenizer.from_str(fl.read_text("tokenizer_2/tokenizer.json"))
            except ImportError:
                pass  # no `tokenizers` package: forward() then needs token_ids=

    @classmethod
    def load(cls, source, silent=False, token=None, revision=None, offloading_type=None, dtype=ModelDType.Auto, **kw):
        """Rust-style constructor name (Pipeline::load, pipelines/mod.rs:120-127)."""
        return cls(source, silent, token, revision, offloading_type, dtype, **kw)

    # ------------------------------------------------------------------------------------------
    def encode_prompts(self, prompts: List[str], token_ids=None):
        """Prompt -> (t5_emb (B,T,4096) bf16, clip_emb (B,768) f32): the first half of FluxPipeline::forward
        (flux/mod.rs:237-262).  token_ids = (t5_ids, clip_ids) overrides tokenisation (no tokenizer files offline)."""
        from . import text
        if self.t5 is None or self.clip is None:
            raise F.L.FmiError("this pipeline was built without text encoders")
        if token_ids is not None:
            t5_ids, clip_ids = token_ids
        elif self.t5_tokenizer is not None and self.clip_tokenizer is not None:
            t5_ids = text.tokenize_and_pad(prompts, self.t5_tokenizer)
            clip_ids = text.tokenize_and_pad(prompts, self.clip_tokenizer)
        else:
            raise F.L.FmiError("no tokenizers loaded: pass token_ids=(t5_ids, clip_ids)")
        t5_ids = torch.as_tensor(t5_ids, dtype=torch.int32)
        if not self.flux.is_guidance():  # schnell: zero-pad the T5 ids to 256 (flux/mod.rs:243-255)
            if t5_ids.shape[1] > 256:
                raise ValueError("T5 embedding length greater than 256, please shrink the prompt or use the -dev (with guidance distillation) version.")
            t5_ids = torch.nn.functional.pad(t5_ids, (0, 256 - t5_ids.shape[1]))
        return self.t5.forward(t5_ids), self.clip.forward(torch.as_tensor(clip_ids, dtype=torch.int32))

    MAX_BATCH = 8  # samples per denoise call (the C-ABI's per-device batch limit); longer prompt lists run in chunks

    def _source_image(self, image, mask, strength, B, params):
        """Check the image-to-image arguments and bring them to their device form: image f32 (B,3,H,W) in [-1,1], mask f32 (B,H,W) or None."""
        if image is None:
            if mask is not None:
                raise ValueError("mask= needs image=: inpainting repaints part of a source image")
            if strength != 1.0:
                raise ValueError("strength= needs image=: text to image always runs the whole schedule")
            return None, None
        if getattr(self, "_sp", None) is not None:
            raise ValueError("image= is not wired through sequence parallelism: disable_sequence_parallel() first")
        H, W = params.height, params.width
        if H % 16 or W % 16:
            raise ValueError(f"image= needs height and width that are multiples of 16, got {H} x {W}")
        img2img_timesteps([0.0] * (params.num_steps + 1), strength)  # the strength range, before any work

        def batched(t, what):
            if t.shape[0] == B:
                return t
            if t.shape[0] == 1:
                return t.expand(B, *t.shape[1:])
            raise ValueError(f"{what} holds {t.shape[0]} samples for {B} prompts (one is broadcast)")

        if isinstance(image, (list, tuple)):  # the list of (H,W,3) arrays output="rgb" returns
            image = np.stack([np.asarray(i) for i in image])
        t = _host_image(image, "image")
        if t.dtype == torch.uint8:  # (B,H,W,3) or (H,W,3): what output="rgb" returns
            t = t.unsqueeze(0) if t.dim() == 3 else t
            if t.dim() != 4 or tuple(t.shape[1:]) != (H, W, 3):
                raise ValueError(f"a uint8 image must be (B,{H},{W},3) or ({H},{W},3) as params say, got {tuple(t.shape)}")
        elif t.dim() != 4 or tuple(t.shape[1:]) != (3, H, W):  # (B,3,H,W) in [-1,1]
            raise ValueError(f"a float image must be (B,3,{H},{W}) as params say, got {tuple(t.shape)}")
        image = batched(self._device_image(t), "image")
        if mask is not None:
            m = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask
            if not isinstance(m, torch.Tensor) or not (m.dtype == torch.bool or m.is_floating_point()):
                raise ValueError("mask must be a bool or float numpy array or torch tensor")
            m = m.unsqueeze(0) if m.dim() == 2 else m
            if m.dim() != 3 or tuple(m.shape[1:]) != (H, W):
                raise ValueError(f"mask must be (B,{H},{W}) or ({H},{W}) as params say, got {tuple(m.shape)}")
            mask = batched(m.to(device=self.device, dtype=torch.float32), "mask")
        return image, mask

    def _reference_image(self, reference, B):
        """Check `reference=` and bring it to its device form, f32 (B,3,Hr,Wr) in [-1,1] (None stays None)."""
        if reference is None:
            return None
        if getattr(self, "_sp", None) is not None:
            raise ValueError("reference= is not wired through sequence parallelism: disable_sequence_parallel() first")
        t = self._device_image(check_reference(_host_image(reference, "reference"), B))
        return t if t.shape[0] == B else t.expand(B, *t.shape[1:])

    def _device_image(self, t: torch.Tensor) -> torch.Tensor:
        """An image that has passed _host_image and its caller's shape rule, in device form: uint8 (n,H,W,3) or float (n,3,H,W) -> f32 (n,3,H,W) in [-1,1]."""
        return F.preprocess_u8(t.to(self.device), interleaved=True) if t.dtype == torch.uint8 else t.to(device=self.device, dtype=torch.float32)

    def _encode(self, image: torch.Tensor) -> torch.Tensor:
        """The packed latents (n,S,64) f32 of an image in device form: VAE encode (the posterior MEAN: deterministic, no second noise stream), scale, shift, pack."""
        return F.encode_latents(self.vae.encode(image), self.vae.scale_factor(), self.vae.shift_factor())[0]

    def generate_tensor(self, prompts: List[str], params: DiffusionGenerationParams, *, embeddings=None, latents=None,
                        seed: Optional[int] = None, first_sample: int = 0, token_ids=None, sample_ids: Optional[Sequence[int]] = None,
                        image=None, strength: float = 1.0, mask=None, reference=None, return_latents: bool = False, cache_threshold: Optional[float] = None,
                        solver: Optional[str] = None, negative_prompt: Optional[str] = None, negative_embeddings=None, negative_token_ids=None, true_cfg_scale: float = 1.0,
                        control_image=None, control_mask=None, controlnet_image=None, controlnet_conditioning_scale: float = 1.0,
                        control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, ip_adapter_image_embeds=None,
                        negative_ip_adapter_image_embeds=None, ip_adapter_scale: float = 1.0, ip_adapter_start: float = 0.0, ip_adapter_end: float = 1.0,
                        ip_adapter_image=None, negative_ip_adapter_image=None, redux_image=None, redux_image_embeds=None, redux_scale: float = 1.0):
        """== ModelPipeline::forward for FluxPipeline (pipelines/flux/mod.rs:224-335) on THIS device.
        Returns (B,3,H,W) u8 on the device.  `sample_ids` (default first_sample + 0..B-1) name the Philox streams of
        the samples, so that a sample draws the same noise whichever rank / chunk it runs in.

        Image to image (`image=`; not in the reference): the source — u8 (B,H,W,3) / (H,W,3) as output="rgb" returns it, or f32 (B,3,H,W)
        in [-1,1]; numpy or torch; one image is broadcast over the prompts — is encoded by the VAE, noised to the schedule's value at `strength`
        (diffusers' FluxImg2ImgPipeline: the last min(int(num_steps * strength), num_steps) steps run; strength 1 is text to image bit for bit) with the
        noise text to image would have started from (same seed / sample ids, or `latents=`).  UNLIKE diffusers, which samples the VAE posterior, the
        source latents are the posterior MEAN: deterministic, no second noise stream.  `mask=` ((B,H,W) / (H,W), float in [0,1] or bool; 1 = repaint,
        0 = keep) makes it inpainting (FluxInpaintPipeline's step): every step blends the re-noised source back in where the 8x8-mean latent mask keeps
        it, and kept latents end as the source's exactly.  `return_latents=True` returns (u8, final packed latents (B,S,64) f32).

        Reference-image conditioning (`reference=`, FLUX.1 Kontext): u8 (Hr,Wr,3) / (B,Hr,Wr,3) or f32 (B,3,Hr,Wr) in [-1,1], numpy or torch, one
        image broadcast over the prompts; Hr and Wr are multiples of 16 and need not be params.height / width.  It is encoded like `image=` (posterior mean;
        diffusers' Kontext pipeline takes the mode too) and its tokens, with 1 in axis 0 of their ids, join the image tokens of every model evaluation; the
        schedule's mu comes from the output's token count alone.  Combines with image= / strength= / mask=.  Not resized to Kontext's preferred resolutions.

        First-block step cache (`cache_threshold=`; None: off, today's launches): FluxModel.denoise's cache_threshold — a step whose
        block-0 residual moved less than the threshold since the last computed step skips the other blocks.  The decision is per denoise CALL (a chunk of up to
        MAX_BATCH prompts reuses a step only when all its samples are under the threshold), and every call's {"decisions", "distances"} is appended to
        `pipeline.last_cache_stats` (one entry per denoise call of the request).  No value is recommended: ParaAttention suggests 0.08 for FLUX.1-dev, which
        this project has no real weights to verify.  Raises under sequence parallelism, like image=.

        True classifier-free guidance (`negative_prompt=` / `negative_embeddings=` (t5 (1,T,J), clip (1,P)) / `negative_token_ids=` (t5 (1,T'), clip (1,.)) with
        `true_cfg_scale` > 1; diffusers' `do_true_cfg`): ONE negative per request, shared by its prompts.  Every step evaluates the prompt and
        the negative in one batch on the same state and steps along neg + true_cfg_scale * (pos - neg), so a denoise call holds MAX_BATCH // 2 prompts.  The
        negative takes the prompt's T: with tokenizers it is tokenised and encoded together with the chunk's prompts; negative_embeddings= / negative_token_ids=
        must have the T of embeddings= / token_ids=.  A negative with true_cfg_scale <= 1 is ignored, as in diffusers (today's launches); true_cfg_scale > 1
        without a negative raises (diffusers only warns).  Combines with image= / strength= / mask= / reference=; raises with cache_threshold= and under
        sequence parallelism.  No scale is recommended: there are no real weights here to judge one.

        Channel-concatenated conditioning (`control_image=` / `control_mask=`; FLUX.1 Canny-dev / Depth-dev and Fill-dev, diffusers'
        FluxControlPipeline / FluxFillPipeline): ONE control per request, shared by its prompts.  control_image: u8 (H,W,3) or f32 (1,3,H,W) in [-1,1] at
        params.height x width (multiples of 16; nothing is resized).  On a Canny / Depth model it is the control image: its VAE latents (the posterior MEAN, as for
        image=; diffusers samples the posterior) are 64 more input channels of every model evaluation.  On a Fill model it is the picture to fill and
        `control_mask=` ((H,W) bool / float, 1 = fill; binarised at 0.5) says where: the latents of image * (1 - mask) and the 256 unshuffled mask channels are the
        320 more.  The loop starts from noise and runs the whole schedule; image= / strength= / mask= and the negative keep their meaning and combine with it.
        Required on such a model and refused on any other; raises with reference=, cache_threshold= and under sequence parallelism.  No guidance scale is
        recommended: there are no real weights here to judge one.

        ControlNet conditioning (`controlnet_image=` with a ControlNet loaded by load_controlnet; diffusers' FluxControlNetPipeline): ONE control
        image per request, shared by its prompts — u8 (H,W,3) or f32 (1,3,H,W) in [-1,1] at params.height x width (multiples of 16; nothing is resized), encoded
        like image= (the posterior MEAN).  Step i of the n steps actually run (after a strength= cut) evaluates the ControlNet and adds its residuals to the
        transformer's stream at controlnet_conditioning_scale * keep_i, keep_i = 0 if i / n < control_guidance_start or (i + 1) / n > control_guidance_end else
        1; a step with scale 0 is the plain step.  Combines with the negative (the ControlNet then sees it as well) and with image= / strength= / mask=;
        raises with reference=, cache_threshold=, on a Fill / Canny / Depth checkpoint, under sequence parallelism and without a loaded ControlNet.  No
        conditioning scale is recommended: there are no real weights here to judge one.

        Image prompts (`ip_adapter_image_embeds=` with an IP-Adapter loaded by load_ip_adapter; diffusers' ip_adapter_image_embeds): ONE image
        embedding per request, (E,) or (1,E), shared by its prompts — or `ip_adapter_image=`, the picture itself, with a CLIP vision encoder loaded by
        load_image_encoder: u8 (H,W,3) of any size, as output="rgb" returns it, or f32 (1,3,S,S) pixel_values that are already preprocessed; it is
        encoded once, before the request is chunked, and is from there on the embedding encode_image returns.  `negative_ip_adapter_image=` likewise for
        negative_ip_adapter_image_embeds=.  A picture and the embedding of the same side exclude one another.  Step i of the n steps
        actually run adds the image-prompt attention in every double block at ip_adapter_scale * keep_i, keep_i = 0 if i / n < ip_adapter_start or
        (i + 1) / n > ip_adapter_end else 1; a step with scale 0 is the plain step.  Under a negative prompt the negative half attends to
        negative_ip_adapter_image_embeds=, or to zero embeddings through the same projection.  Combines with the negative, image= / strength= / mask=, a Fill /
        Canny / Depth control and a ControlNet; raises with reference=, cache_threshold=, under sequence parallelism, on an 8-bit transformer and without a loaded
        adapter.

        Image variation (`redux_image=` with FLUX.1 Redux loaded by load_redux; diffusers' FluxPriorReduxPipeline): ONE picture per request,
        shared by its prompts — u8 (H,W,3) of any size, as output="rgb" returns it, or f32 (1,3,S,S) pixel_values that are already preprocessed — or
        `redux_image_embeds=`, the (Np,J) / (1,Np,J) image tokens encode_redux_image returns.  A picture and its embedding exclude one another.  The picture
        is encoded once, before the request is chunked (SigLIP tower, Redux embedder), and redux_scale * tokens are appended behind the T5 rows of every sample,
        whether the prompt came as text, token_ids= or embeddings=: the model sees T = T_prompt + Np text rows with zero txt_ids, the pooled CLIP embedding is
        unchanged, the denoise loop is untouched.  redux_scale = 0 still appends the rows, as zeros.  Under a negative prompt (true CFG) both halves keep one T:
        the negative half receives ZERO rows in place of the image tokens (the IP-Adapter's zero-embeddings rule).  Redux changes the text rows only, so it combines
        with everything the text rows combine with — image= / strength= / mask=, reference=, a control, a ControlNet, an IP-Adapter, cache_threshold=, the 8-bit
        modes; it raises under sequence parallelism and without a loaded Redux.

        Integrator (`solver=`; None | "euler": the loop as it always was): "heun" (diffusers' FlowMatchHeunDiscreteScheduler, ComfyUI's heun) or
        "dpmpp_2m" (DPMSolverMultistepScheduler with use_flow_sigmas, ComfyUI's dpmpp_2m) over the request's own schedule — after a strength= cut the schedule
        starts below 1 and "dpmpp_2m" uses its history from step 1 on.  "heun" evaluates the model twice per step but the last, "dpmpp_2m" once.  Both combine
        with everything above except "heun" with cache_threshold= and either under sequence parallelism.  A capability, not a recommendation: no step count is
        suggested for either, there are no real weights here to judge one."""
        rdx = self._redux_input(redux_image, redux_image_embeds, redux_scale)
        ipa = self._ip_adapter_input(ip_adapter_image_embeds, negative_ip_adapter_image_embeds, ip_adapter_scale, ip_adapter_start, ip_adapter_end,
                                     negative_prompt is not None or negative_embeddings is not None or negative_token_ids is not None,
                                     image=ip_adapter_image, negative_image=negative_ip_adapter_image)
        cn = self._controlnet_input(controlnet_image, controlnet_conditioning_scale, control_guidance_start, control_guidance_end, params)
        F.check_step_cache_args(params.num_steps, cache_threshold)
        # (the schedule is the scheduler's own, strictly decreasing from 1 to 0: the name and the solver's two refusals are what a request can get wrong)
        kind = F.check_solver_args(solver, [1.0, 0.0], cache=cache_threshold is not None, sequence_parallel=getattr(self, "_sp", None) is not None)
        ctl = self._control(control_image, control_mask, params)
        neg = self._negative(negative_prompt, negative_embeddings, negative_token_ids, true_cfg_scale, embeddings, token_ids)
        # the request's shared options, one keyword of _generate_chunk each, passed only by a request that has it: any other makes exactly the call it always made
        shared = {k: v for k, v in (("negative", neg), ("control", ctl), ("controlnet", cn), ("ip_adapter", ipa)) if v is not None}
        modes = {"sequence_parallel" if getattr(self, "_sp", None) is not None else None,
                 "int8" if getattr(self, "_int8_pending", False) else getattr(getattr(self, "flux", None), "_eight_bit", None)}
        present = dict(context=reference, cache=cache_threshold, true_cfg=neg, control=ctl, controlnet=cn, ip_adapter=ipa)  # (a negative at a scale <= 1: neg is None)
        F.check_combination({k for k, v in present.items() if v is not None} | modes, REQUEST_NAMES)
        s = self._samples(prompts, params, strength, first_sample, sample_ids, embeddings=embeddings, token_ids=token_ids, latents=latents, image=image,
                          mask=mask, reference=reference)
        if not s.prompts:
            u8 = torch.empty((0, 3, params.height, params.width), dtype=torch.uint8, device=self.device)
            S = ((params.height + 15) // 16) * ((params.width + 15) // 16)
            return (u8, torch.empty((0, S, 64), dtype=torch.float32, device=self.device)) if return_latents else u8
        stats = []  # one list per request, shared by the chunks it is cut into
        # a request with a solver takes the chunk body through _generate_chunk_solver; any other makes exactly the call it always made
        base = self._generate_chunk if kind is None else (lambda *a, **kw: self._generate_chunk_solver(solver, *a, **kw))
        chunk = base if rdx is None else (lambda *a, **kw: self._generate_chunk_redux(rdx, *a, **({} if kind is None else dict(chunk=base)), **kw))
        outs = [chunk(s.take(idx), params, seed, strength, return_latents, cache_threshold, stats, **shared)
                for idx in _index_sets(len(s.prompts), self.MAX_BATCH // 2 if neg is not None else self.MAX_BATCH, getattr(self, "_sp", None) is not None)]
        if len(outs) == 1:
            return outs[0]
        return (torch.cat([o[0] for o in outs], 0), torch.cat([o[1] for o in outs], 0)) if return_latents else torch.cat(outs, 0)

    def _control(self, control_image, control_mask, params, *_) -> Optional[_Control]:
        """The control of a request, checked once and brought to its device form: None on a plain model, else the object its chunks share.  (Callers from before
        check_combination pass two more arguments, about the request's other options; they are not looked at.)"""
        img = None if control_image is None else _host_image(control_image, "control_image")
        m = torch.from_numpy(np.ascontiguousarray(control_mask)) if isinstance(control_mask, np.ndarray) else control_mask
        if m is not None and not isinstance(m, torch.Tensor):
            raise ValueError("control_mask must be a numpy array or a torch tensor")
        if m is not None and not (m.dtype == torch.bool or m.is_floating_point()):
            raise ValueError("control_mask must be a bool or float numpy array or torch tensor")
        kind = control_kind(getattr(getattr(self, "flux", None), "cond_channels", 0))
        check_control_request(kind, params.height, params.width, None if img is None else tuple(img.shape), img is not None and img.dtype == torch.uint8,
                              None if m is None else tuple(m.shape))
        if kind is None:
            return None
        img = self._device_image(img.unsqueeze(0) if img.dtype == torch.uint8 else img)
        return _Control(kind, img, None if m is None else m.unsqueeze(0).to(device=self.device, dtype=torch.float32).contiguous())

    def _controlnet_input(self, image, scale, start, end, params) -> Optional[_ControlNetInput]:
        """The ControlNet conditioning of a request, checked once and brought to its device form: None without controlnet_image=, else the object its chunks share."""
        if image is None:
            return None
        img = _host_image(image, "controlnet_image")
        check_controlnet_request(getattr(self, "controlnet", None) is not None, params.height, params.width, tuple(img.shape), img.dtype == torch.uint8, scale, start, end)
        return _ControlNetInput(self._device_image(img.unsqueeze(0) if img.dtype == torch.uint8 else img), float(scale), float(start), float(end))

    def _ip_adapter_input(self, embeds, negative_embeds, scale, start, end, has_negative, *, image=None, negative_image=None) -> Optional[_IpAdapterInput]:
        """The image prompt of a request, checked once and brought to its device form: None without ip_adapter_image_embeds= / ip_adapter_image=, else the object
        its chunks share.  A picture (image= / negative_image=) is encoded here, once, by the loaded image encoder: from here on it is its embedding."""
        def as_tensor(x, what):
            t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
            if x is not None and not (isinstance(t, torch.Tensor) and t.is_floating_point()):
                raise ValueError(f"{what} must be a float numpy array or torch tensor")
            return t
        e, n = as_tensor(embeds, "ip_adapter_image_embeds"), as_tensor(negative_embeds, "negative_ip_adapter_image_embeds")
        img = None if image is None else _host_image(image, "ip_adapter_image")
        nimg = None if negative_image is None else _host_image(negative_image, "negative_ip_adapter_image")
        ada, enc = getattr(self, "ip_adapter", None), getattr(self, "image_encoder", None)
        shape, is_u8 = (lambda t: None if t is None else tuple(t.shape)), (lambda t: t is not None and t.dtype == torch.uint8)
        check_ip_adapter_request(ada is not None, 0 if ada is None else ada.embed_dim, shape(e), shape(n), scale, start, end, has_negative, image_shape=shape(img),
                                 image_is_u8=is_u8(img), negative_image_shape=shape(nimg), negative_image_is_u8=is_u8(nimg),
                                 encoder_dim=None if enc is None else enc.projection_dim, encoder_image_size=0 if enc is None else enc.cfg["image_size"])
        if img is not None or nimg is not None:
            with self._lock:
                e = e if img is None else enc.encode(img)
                n = n if nimg is None else enc.encode(nimg)
        if e is None:
            return None
        dev = lambda t: None if t is None else t.to(device=self.device, dtype=torch.float32).reshape(1, -1).contiguous()
        return _IpAdapterInput(dev(e), dev(n), float(scale), float(start), float(end))

    def load_ip_adapter(self, source):
        """Load ONE IP-Adapter next to the transformer: a .safetensors file under XLabs' names (ip_adapter_proj_model.*, double_blocks.{i}.processor.
        ip_adapter_double_stream_{k,v}_proj.*) or the diffusers-converted ones (image_proj.*, ip_adapter.{i}.to_{k,v}_ip.*), or a {name: tensor} dict of either.  The
        number of tokens and the embedding width are read from the shapes; missing and unexpected keys raise ValueError by name.  It replaces a loaded one; requests
        use it only when they pass ip_adapter_image_embeds= — or ip_adapter_image=, a picture, once load_image_encoder has loaded the CLIP vision encoder whose
        projection_dim is the adapter's embedding width."""
        from . import loader
        if isinstance(source, (str, os.PathLike)):
            E, N, sd = loader.load_ip_adapter(os.fspath(source), self.flux.cfg)
        else:
            E, N, sd = loader.ip_adapter_from_tensors(self.flux.cfg, source)
        with self._lock:
            ada = F.FluxIPAdapter(self.flux.cfg, E, N, self.device.index or 0)
            ada.load_state_dict(sd)
            old, self.ip_adapter = getattr(self, "ip_adapter", None), ada
            if old is not None:
                old.close()
        return ada

    def unload_ip_adapter(self):
        with self._lock:
            ada, self.ip_adapter = getattr(self, "ip_adapter", None), None
            if ada is not None:
                ada.close()

    def load_image_encoder(self, source):
        """Load ONE CLIP vision encoder (openai/clip-vit-large-patch14 is what the FLUX IP-Adapters were trained with): a directory (loader.
        load_clip_vision: config.json — a CLIPVisionConfig or a full CLIPConfig — next to *.safetensors and an optional preprocessor_config.json) or a (cfg,
        {name: tensor}) pair, cfg holding CLIPVisionConfig's keys and optionally image_mean / image_std.  Missing and unexpected keys raise ValueError by name; a
        full CLIP checkpoint's text tower is ignored.  It replaces a loaded one; requests use it only when they pass ip_adapter_image= /
        negative_ip_adapter_image=, and encode_image."""
        from . import loader, text
        if isinstance(source, (str, os.PathLike)):
            cfg, sd = loader.load_clip_vision(os.fspath(source))
        else:
            cfg, sd = source
            cfg = dict(loader.clip_vision_config(cfg), **{k: cfg[k] for k in ("image_mean", "image_std") if k in cfg})
            sd = loader.clip_vision_from_tensors(cfg, sd)
        with self._lock:
            enc = text.ClipVisionModel(cfg, self.device.index or 0, cfg.get("image_mean"), cfg.get("image_std"))
            enc.load_state_dict(sd)
            old, self.image_encoder = getattr(self, "image_encoder", None), enc
            if old is not None:
                old.close()
        return enc

    def unload_image_encoder(self):
        with self._lock:
            enc, self.image_encoder = getattr(self, "image_encoder", None), None
            if enc is not None:
                enc.close()

    def encode_image(self, image) -> torch.Tensor:
        """The image prompt of a picture: u8 (H,W,3) of any size, or float (1,3,S,S) pixel_values -> (1,E) f32 on the device, what ip_adapter_image_embeds= takes and
        what ip_adapter_image= passes on.  ValueError without a loaded image encoder."""
        enc = getattr(self, "image_encoder", None)
        if enc is None:
            raise ValueError("encode_image needs a loaded image encoder: Pipeline.load_image_encoder(path) first")
        img = _host_image(image, "image")
        S = enc.cfg["image_size"]
        if not ((img.dim() == 3 and img.shape[2] == 3) if img.dtype == torch.uint8 else tuple(img.shape) == (1, 3, S, S)):
            raise ValueError(f"image must be a uint8 (H,W,3) picture of any size or float (1,3,{S},{S}) pixel_values, got {tuple(img.shape)}")
        with self._lock:
            return enc.encode(img)

    def _redux_input(self, image, embeds, scale) -> Optional[_ReduxInput]:
        """The Redux tokens of a request, checked once and brought to their device form: None without redux_image= / redux_image_embeds=, else the object its
        chunks share.  A picture is encoded here, once; the scale is applied here, once (an f32 multiply)."""
        if image is None and embeds is None:
            return None
        img = None if image is None else _host_image(image, "redux_image")
        e = torch.from_numpy(np.ascontiguousarray(embeds)) if isinstance(embeds, np.ndarray) else embeds
        if e is not None and not (isinstance(e, torch.Tensor) and e.is_floating_point()):
            raise ValueError("redux_image_embeds must be a float numpy array or torch tensor")
        rdx = getattr(self, "redux", None)
        tower, emb = rdx if rdx is not None else (None, None)
        check_redux_request(rdx is not None, 0 if tower is None else tower.num_patches, 0 if emb is None else emb.txt_dim, 0 if tower is None else tower.cfg["image_size"],
                            None if img is None else tuple(img.shape), img is not None and img.dtype == torch.uint8, None if e is None else tuple(e.shape), float(scale),
                            getattr(self, "_sp", None) is not None)
        tokens = self.encode_redux_image(img) if img is not None else e.to(device=self.device, dtype=torch.float32).reshape(1, tower.num_patches, emb.txt_dim)
        return _ReduxInput((tokens * float(scale)).contiguous())

    def _generate_chunk_redux(self, redux: _ReduxInput, s: _Samples, params, seed, strength, return_latents, cache_threshold, stats, negative: Optional[_Negative] = None,
                              chunk=None, **shared):
        """One denoise call of a request with Redux tokens: the chunk's text embeddings are made as always (_chunk_embeddings: text, token_ids= or embeddings=,
        the negative with them), the tokens are appended behind the T5 rows of every sample — zero rows behind the negative's — and the chunk goes on as the
        embeddings= chunk that it now is (through `chunk`, the solver's chunk call, where the request has a solver)."""
        with self._lock:
            t5_emb, clip_emb, neg = self._chunk_embeddings(s, negative)
        tok = redux.tokens.to(t5_emb.dtype)
        s = replace(s, embeddings=(torch.cat([t5_emb, tok.expand(t5_emb.shape[0], -1, -1)], 1), clip_emb), token_ids=None)
        if neg is not None:
            negative = _Negative(negative.scale, embeddings=(torch.cat([neg[0][:1], torch.zeros_like(tok)], 1), neg[1][:1]))
        return (chunk or self._generate_chunk)(s, params, seed, strength, return_latents, cache_threshold, stats, **({} if negative is None else dict(negative=negative)),
                                               **shared)

    def load_redux(self, path, image_encoder=None):
        """Load FLUX.1 Redux: a SigLIP vision tower and the Redux embedder.  `path` is a FLUX.1-Redux-dev directory (image_encoder/,
        image_embedder/, feature_extractor/), or the embedder alone — an image_embedder/ directory, BFL's flux1-redux-dev.safetensors, or a {name: tensor} dict —
        with the tower in `image_encoder=`: a directory (loader.load_siglip_vision) or a (cfg, {name: tensor}) pair.  The embedder's txt_in_features must equal the
        transformer's joint_attention_dim and its redux_dim the tower's hidden_size: ValueError by name otherwise, as for missing and unexpected keys.  It replaces a
        loaded one; requests use it only when they pass redux_image= / redux_image_embeds=, and encode_redux_image."""
        from . import loader, text
        if isinstance(path, (str, os.PathLike)):
            path = os.fspath(path)
            if image_encoder is None:
                if not os.path.isdir(os.path.join(path, "image_encoder")) or not os.path.isdir(os.path.join(path, "image_embedder")):
                    raise ValueError(f"{path}: not a FLUX.1-Redux-dev directory (image_encoder/ and image_embedder/); pass the embedder with image_encoder=")
                image_encoder, path = (os.path.join(path, "image_encoder"), os.path.join(path, "feature_extractor")), os.path.join(path, "image_embedder")
            D, J, rsd = loader.load_redux(path)
        else:
            D, J, rsd = loader.redux_from_tensors(path)
        if image_encoder is None:
            raise ValueError("load_redux: an embedder alone needs the SigLIP tower in image_encoder=")
        if isinstance(image_encoder, tuple) and isinstance(image_encoder[0], dict):
            cfg, sd = image_encoder
            cfg = dict(loader.siglip_vision_config(cfg), **{k: cfg[k] for k in ("image_mean", "image_std") if k in cfg})
            sd = loader.siglip_vision_from_tensors(cfg, sd)
        else:
            enc_dir, pre_dir = image_encoder if isinstance(image_encoder, tuple) else (image_encoder, None)
            cfg, sd = loader.load_siglip_vision(os.fspath(enc_dir), pre_dir)
        if J != self.flux.cfg["joint_attention_dim"]:
            raise ValueError(f"the Redux embedder's txt_in_features is {J}, the transformer's joint_attention_dim is {self.flux.cfg['joint_attention_dim']}")
        if D != cfg["hidden_size"]:
            raise ValueError(f"the Redux embedder's redux_dim is {D}, the SigLIP tower's hidden_size is {cfg['hidden_size']}")
        with self._lock:
            tower = text.SiglipVisionModel(cfg, self.device.index or 0, cfg.get("image_mean"), cfg.get("image_std"))
            tower.load_state_dict(sd)
            emb = text.ReduxImageEmbedder(D, J, self.device.index or 0)
            emb.load_state_dict(rsd)
            old, self.redux = getattr(self, "redux", None), (tower, emb)
            for m in old or ():
                m.close()
        return self.redux

    def unload_redux(self):
        with self._lock:
            old, self.redux = getattr(self, "redux", None), None
            for m in old or ():
                m.close()

    def encode_redux_image(self, image) -> torch.Tensor:
        """The Redux image tokens of a picture: u8 (H,W,3) of any size, or float (1,3,S,S) pixel_values -> (1,Np,J) f32 on the device, before any scale: what
        redux_image_embeds= takes and what redux_image= passes on.  ValueError without a loaded Redux."""
        rdx = getattr(self, "redux", None)
        if rdx is None:
            raise ValueError("encode_redux_image needs a loaded Redux: Pipeline.load_redux(path) first")
        tower, emb = rdx
        img = _host_image(image, "image")
        S = tower.cfg["image_size"]
        if not ((img.dim() == 3 and img.shape[2] == 3) if img.dtype == torch.uint8 else tuple(img.shape) == (1, 3, S, S)):
            raise ValueError(f"image must be a uint8 (H,W,3) picture of any size or float (1,3,{S},{S}) pixel_values, got {tuple(img.shape)}")
        with self._lock:
            return emb.forward(tower.encode(img))

    def load_controlnet(self, source):
        """Load ONE ControlNet next to the transformer: a diffusers directory (loader.load_controlnet: config.json with _class_name
        FluxControlNetModel + diffusion_pytorch_model*.safetensors) or a (cfg, state_dict) pair.  It replaces a loaded one; requests use it only when they pass
        controlnet_image=.  ValueError for a ControlNet whose width-defining fields differ from the transformer's; union modes, the XLabs hint block and several
        ControlNets at once are out of scope."""
        from . import loader
        cfg, sd = loader.load_controlnet(os.fspath(source)) if isinstance(source, (str, os.PathLike)) else source
        for k in ("num_attention_heads", "joint_attention_dim", "pooled_projection_dim", "axes_dim", "theta"):
            if list(np.atleast_1d(cfg[k])) != list(np.atleast_1d(self.flux.cfg[k])):
                raise ValueError(f"the ControlNet's {k} is {cfg[k]!r}, the transformer's {self.flux.cfg[k]!r}")
        if int(cfg["in_channels"]) != self.flux.state_channels:
            raise ValueError(f"the ControlNet's in_channels is {cfg['in_channels']}, the transformer's state has {self.flux.state_channels}")
        with self._lock:
            net = F.FluxControlNetModel(cfg, self.device.index or 0)
            net.load_state_dict(sd)
            old, self.controlnet = getattr(self, "controlnet", None), net
            if old is not None:
                old.close()
        return net

    def unload_controlnet(self):
        with self._lock:
            net, self.controlnet = getattr(self, "controlnet", None), None
            if net is not None:
                net.close()

    def _control_condition(self, control: _Control, B: int):
        """The conditioning channels (B,S,64 | 320) f32 of a chunk of B samples: built once at one row — VAE encode (the posterior mean), pack, and for Fill the
        masked image in front of it and the mask channels behind — then expanded."""
        if control.kind == "fill":
            cond = F.fill_condition(self._encode(F.mask_image(control.image, control.mask)), control.mask)
        else:
            cond = self._encode(control.image)
        return cond.expand(B, -1, -1).contiguous()

    def _negative(self, negative_prompt, negative_embeddings, negative_token_ids, true_cfg_scale, embeddings, token_ids) -> Optional[_Negative]:
        """The negative of a request, checked once: None when true CFG is off (no negative, or a scale <= 1: diffusers' do_true_cfg), else the object its chunks share."""
        scale = float(true_cfg_scale)
        given = [x is not None for x in (negative_prompt, negative_embeddings, negative_token_ids)]
        if not scale >= 0.0 or scale == float("inf"):
            raise ValueError(f"true_cfg_scale must be finite and >= 0, got {true_cfg_scale!r}")
        if sum(given) > 1:
            raise ValueError("negative_prompt=, negative_embeddings= and negative_token_ids= exclude one another: a request has one negative")
        if not any(given):
            if scale > 1.0:
                raise ValueError("true_cfg_scale > 1 needs a negative: negative_prompt=, negative_embeddings= or negative_token_ids=")
            return None
        if scale <= 1.0:
            return None
        if embeddings is not None and negative_embeddings is None:
            raise ValueError("with embeddings= the negative comes as negative_embeddings= (t5 (1,T,J), clip (1,P))")
        if embeddings is None and token_ids is not None and negative_prompt is not None:
            raise ValueError("with token_ids= the negative comes as negative_token_ids= (or negative_embeddings=)")
        if negative_token_ids is not None and (token_ids is None or embeddings is not None):
            raise ValueError("negative_token_ids= goes with token_ids=: without them the negative comes as negative_prompt= (or negative_embeddings=)")
        pair = None
        for mine, theirs, what in ((negative_embeddings, embeddings, "embeddings"), (negative_token_ids, token_ids, "token_ids")):
            if mine is None:
                continue
            pair = tuple(mine)
            if len(pair) != 2 or any(np.shape(x)[0] != 1 for x in pair):
                raise ValueError(f"negative_{what}= is a pair (t5, clip) of ONE row each: the negative is shared by the request's prompts")
            # T of the t5 member; of token ids also the clip member's length (the rows are concatenated), of embeddings the clip vector's width
            for n, t in zip(pair, tuple(theirs) if theirs is not None else ()):
                if np.shape(n)[1] != np.shape(t)[1]:
                    raise ValueError(f"negative_{what}= has T = {np.shape(n)[1]}, {what}= has T = {np.shape(t)[1]}: the negative takes the prompt's T")
        return _Negative(scale, negative_prompt, pair if negative_embeddings is not None else None, pair if negative_token_ids is not None else None)

    def _samples(self, prompts, params, strength, first_sample=0, sample_ids=None, **given) -> _Samples:
        """A request's per-sample inputs (`given`: the other fields of _Samples as the caller passed them), checked and normalised once: the pairs as tuples,
        image / mask / reference in device form with a single one broadcast over the prompts."""
        B = len(prompts)
        s = _Samples(list(prompts), list(sample_ids) if sample_ids is not None else [first_sample + b for b in range(B)], **given)
        if len(s.sample_ids) != B:
            raise ValueError("sample_ids must name one stream per prompt")
        s.embeddings, s.token_ids = (None if pair is None else tuple(pair) for pair in (s.embeddings, s.token_ids))
        if B > 0:  # (an empty request returns before any image check)
            s.image, s.mask = self._source_image(s.image, s.mask, strength, B, params)
            s.reference = self._reference_image(s.reference, B)
        return s

    def _chunk_embeddings(self, s: _Samples, negative: Optional[_Negative]):
        """(t5_emb (B,T,J), clip_emb (B,P), the negative's two expanded to B rows or None) of a chunk.  The negative reaches the prompts' T here: tokenised and
        encoded in ONE pass with the chunk's prompts (row B), or checked against them."""
        cfg, dev, B = self.flux.cfg, self.device, len(s.prompts)
        neg_text = negative is not None and negative.embeddings is None  # the negative goes through the same source as the prompts, as row B
        if s.embeddings is not None:
            t5_emb, clip_emb = (e.to(dev) for e in s.embeddings)  # (the negative is negative_embeddings= then: Pipeline._negative)
        elif self.t5 is not None and self.clip is not None:
            prompts, token_ids = s.prompts, s.token_ids
            if neg_text and token_ids is not None:  # (Pipeline._negative has checked that the negative came as token ids of the same T)
                token_ids = tuple(torch.cat([torch.as_tensor(t, dtype=torch.int32), torch.as_tensor(n, dtype=torch.int32)], 0) for t, n in zip(token_ids, negative.token_ids))
            elif neg_text:
                prompts = list(prompts) + [negative.prompt]  # one tokenize_and_pad, one pass of B + 1 rows through the encoders
            t5_emb, clip_emb = self.encode_prompts(prompts, token_ids)
        elif self.source_kind == "synthetic":
            # schnell pads T5 ids to 256 (flux/mod.rs:243-253); dev uses the prompt length — 512 here
            T = 256 if not self.flux.is_guidance() else 512
            t5_emb, clip_emb = placeholder_embeddings(list(s.prompts) + ([negative.prompt] if neg_text else []), T, cfg["joint_attention_dim"],
                                                      cfg["pooled_projection_dim"], dev)
        else:
            raise F.L.FmiError("this checkpoint was loaded without text encoders: pass embeddings=(t5_emb, clip_emb)")
        if negative is None:
            return t5_emb, clip_emb, None
        if neg_text:
            neg, t5_emb, clip_emb = (t5_emb[B:], clip_emb[B:]), t5_emb[:B], clip_emb[:B]
        else:
            neg = tuple(e.to(dev) for e in negative.embeddings)
            if int(neg[0].shape[1]) != int(t5_emb.shape[1]):
                raise ValueError(f"negative_embeddings= has T = {int(neg[0].shape[1])}, the prompts' embeddings have T = {int(t5_emb.shape[1])}")
        neg = (neg[0].to(t5_emb.dtype).expand(B, -1, -1).contiguous(), neg[1].to(clip_emb.dtype).expand(B, -1).contiguous())
        return t5_emb, clip_emb, neg

    def _generate_chunk(self, s: _Samples, params, seed, strength, return_latents, cache_threshold, stats, negative: Optional[_Negative] = None,
                        control: Optional[_Control] = None, controlnet: Optional[_ControlNetInput] = None, ip_adapter: Optional[_IpAdapterInput] = None):
        """One denoise call of a request without a solver: _chunk, see there."""
        return self._chunk(s, params, seed, strength, return_latents, cache_threshold, stats, negative, control, controlnet, ip_adapter)

    def _generate_chunk_solver(self, solver: str, s: _Samples, params, seed, strength, return_latents, cache_threshold, stats, **shared):
        """One denoise call of a request with solver= "heun" / "dpmpp_2m" (DESIGN.md 4.21): the same chunk, integrated by that solver."""
        return self._chunk(s, params, seed, strength, return_latents, cache_threshold, stats, solver=solver, **shared)

    def _chunk(self, s: _Samples, params, seed, strength, return_latents, cache_threshold, stats, negative: Optional[_Negative] = None,
               control: Optional[_Control] = None, controlnet: Optional[_ControlNetInput] = None, ip_adapter: Optional[_IpAdapterInput] = None,
               solver: Optional[str] = None):
        """One denoise call: at most MAX_BATCH samples (one under sequence parallelism; MAX_BATCH // 2 with a negative) of a normalised request.  Returns what
        generate_tensor does.  The request's shared options, each passed only by a request that has it — negative: its true-CFG negative;
        control: the control of a request to a channel-conditioned model; controlnet: the conditioning of one with controlnet_image=
        (DESIGN.md 4.15); ip_adapter: the image prompt of one with ip_adapter_image_embeds=; solver: "heun" / "dpmpp_2m" of one with solver=
        (DESIGN.md 4.21)."""
        cfg = self.flux.cfg
        dev = self.device
        sp = getattr(self, "_sp", None)
        B, ids, latents = len(s.prompts), s.sample_ids, s.latents
        with self._lock:  # the whole forward, text encoders included, like the reference's mutex (pipelines/mod.rs:247)
            t5_emb, clip_emb, neg = self._chunk_embeddings(s, negative)
            h = (params.height + 15) // 16 * 2  # get_noise, flux/sampling.rs:12-13
            w = (params.width + 15) // 16 * 2
            if latents is None:
                sd = seed if seed is not None else 299792458
                if ids == list(range(ids[0], ids[0] + B)):
                    latents = F.randn_latents(B, 16, h, w, sd, ids[0], dev)
                else:
                    latents = torch.cat([F.randn_latents(1, 16, h, w, sd, i, dev) for i in ids], 0)
            latents = latents.to(device=dev, dtype=torch.float32)
            img, img_ids = F.pack_latents(latents)  # State::new
            txt_ids = torch.zeros((B, t5_emb.shape[1], 3), dtype=torch.float32, device=dev)
            mu = self.scheduler.calculate_shift(img.shape[1])
            timesteps = self.scheduler.get_timesteps(params.num_steps, mu)
            guidance = torch.full((B,), float(params.guidance_scale), dtype=torch.float32, device=dev) if self.flux.is_guidance() else None
            inpaint = {}
            if s.image is not None:  # start from the source noised to the cut schedule's first value (at strength 1 that is the noise itself, bit for bit)
                x0 = self._encode(s.image)
                timesteps = img2img_timesteps(timesteps, strength)
                noise = img
                img = F.scale_noise(x0, noise, timesteps[0])
                if s.mask is not None:
                    inpaint = dict(x0=x0, noise=noise, mask=F.latent_mask(s.mask, x0.shape[2] // 4))
            context = {}
            if s.reference is not None:  # its packed latents are rows of every evaluation, never of the state; mu and the schedule above know S only
                context = dict(context=self._encode(s.reference), context_ids=F.latent_ids(B, s.reference.shape[2] // 16, s.reference.shape[3] // 16, id0=1.0, device=dev))
            if control is not None:  # the same conditioning channels at every step, for every sample and for both halves of a true-CFG batch
                context = dict(control=self._control_condition(control, B))
            cn_kw = {}
            if controlnet is not None:  # the control image's packed latents, one row expanded; the scales over the steps actually run
                cn_kw = dict(controlnet=self.controlnet, controlnet_cond=self._encode(controlnet.image).expand(B, -1, -1).contiguous(), controlnet_scale=controlnet.scale,
                             controlnet_step_scales=F.controlnet_step_scales(len(timesteps) - 1, controlnet.start, controlnet.end))
            if ip_adapter is not None:  # one embedding row expanded to the chunk; the scales over the steps actually run, like the ControlNet's
                cn_kw.update(ip_adapter=self.ip_adapter, ip_adapter_image_embeds=ip_adapter.embeds.expand(B, -1).contiguous(), ip_adapter_scale=ip_adapter.scale,
                             ip_adapter_step_scales=F.controlnet_step_scales(len(timesteps) - 1, ip_adapter.start, ip_adapter.end))
                if ip_adapter.negative_embeds is not None:
                    cn_kw.update(negative_ip_adapter_image_embeds=ip_adapter.negative_embeds.expand(B, -1).contiguous())
            if solver is not None:
                cn_kw.update(solver=solver)
            if getattr(self, "_int8_pending", False):
                self._int8_calibrate_and_quantize(img[:1], img_ids[:1], t5_emb[:1], txt_ids[:1], clip_emb[:1], None if guidance is None else guidance[:1], timesteps,
                                                  {k: v[:1] for k, v in context.items()})
            if sp is not None:  # every rank holds the same inputs; each denoises its token shard, then all get the latents
                img = sp.gather(self.flux.denoise(sp.shard(img), sp.shard(img_ids), sp.shard(t5_emb), sp.shard(txt_ids), clip_emb, guidance, timesteps))
            else:
                cache = {} if cache_threshold is None else dict(cache_threshold=cache_threshold, return_cache_stats=True)
                true_cfg = {} if neg is None else dict(negative_txt=neg[0], negative_y=neg[1], true_cfg_scale=negative.scale)
                img = self.flux.denoise(img, img_ids, t5_emb, txt_ids, clip_emb, guidance, timesteps, **inpaint, **context, **cache, **true_cfg, **cn_kw)
                if cache:
                    img, st = img
                    stats.append(st)
            self.last_cache_stats = stats  # (under the lock) one entry per denoise call of this request so far; empty without cache_threshold=
            z = F.unpack_latents(img, 16, h, w, self.vae.scale_factor(), self.vae.shift_factor())
            u8 = F.postprocess_u8(self.vae.decode(z))
            return (u8, img) if return_latents else u8

    INT8_CALIBRATION_POINTS = 4

    def _int8_calibrate_and_quantize(self, img, img_ids, t5_emb, txt_ids, clip_emb, guidance, timesteps, context=None):
        """ModelDType.I8, first request: INT8_CALIBRATION_POINTS evaluations of the bf16 model on ONE sample at timesteps spread over the request's schedule
        record the per-channel absmax of every block linear's input (the outlier channels of a DiT are the same at every step and for every prompt: they
        come from the AdaLN weights), then the block linears are quantised with the smoothing factors folded in.  ~0.25 s once per model at 1024 x 1024."""
        n = len(timesteps) - 1
        pts = sorted({min(n - 1, max(0, round(i * (n - 1) / max(1, self.INT8_CALIBRATION_POINTS - 1)))) for i in range(self.INT8_CALIBRATION_POINTS)})
        self.flux.calibrate_int8(True)
        for i in pts:
            t = torch.full((1,), float(timesteps[i]), dtype=torch.float32, device=self.device)
            self.flux.forward(img, img_ids, t5_emb, txt_ids, t, clip_emb, guidance, **(context or {}))
        self.flux.quantize_int8()
        self._int8_pending = False

    # ---- LoRA adapters (lora.py reads the file, FluxModel.lora_* merge it into the resident weights).  Load-time calls under the pipeline lock; with
    # ModelDType.I8 they work until the first request has quantised the model, afterwards the library answers with its state error.  Under
    # torch.distributed every rank makes the same call on its own copy of the weights: there is no collective.
    def load_lora(self, path_or_dict, name: Optional[str] = None, weight: float = 1.0, skip_unsupported: bool = False) -> str:
        """Merge the adapter of a .safetensors file (diffusers / PEFT or kohya / BFL keys; LoRA, LoHa, LoKr, full differences, DoRA: lora.read_adapter) or
        of a {key: tensor} dict into the DiT; returns its name (default: the file's base name).  Several adapters stack; the result does not depend on the order they were loaded in."""
        from . import lora
        terms = lora.read_adapter(path_or_dict, skip_unsupported=skip_unsupported, hidden_size=self.flux.hidden)
        if name is None:
            name = os.path.splitext(os.path.basename(os.fspath(path_or_dict)))[0] if isinstance(path_or_dict, (str, os.PathLike)) else "lora"
        if not terms:
            raise ValueError(f"LoRA '{name}': no supported keys")
        shapes = self.flux._shapes()
        for prefix, term in terms.items():
            want = shapes.get(prefix + ".weight")
            if want is None or len(want) != 2:
                raise ValueError(f"LoRA '{name}': {prefix} is not a Linear of this model")
            if term.kind in ("lora", "dora"):  # (the factor shapes of the other kinds are checked by the library, which refuses before it changes anything)
                A, B = term.tensors[:2]
                if (int(B.shape[0]), int(A.shape[1])) != tuple(want):
                    raise ValueError(f"LoRA '{name}': {prefix}: B A is {(int(B.shape[0]), int(A.shape[1]))}, the Linear is {tuple(want)}")
        with self._lock:
            if name in self.flux.loras():
                raise ValueError(f"a LoRA named '{name}' is loaded already: unload_lora('{name}') first, or pass another name")
            try:
                first = True
                for prefix, term in terms.items():
                    if term.kind == "lora":
                        self.flux.lora_add(name, prefix, term.tensors[0], term.tensors[1], term.scale)
                    else:
                        self.flux.lora_add_term(name, prefix, term)
                    if first and weight != 1.0:  # before the other pairs arrive: each Linear is then merged once, at its final weight
                        self.flux.lora_set_weight(name, weight)
                    first = False
            except Exception:
                if name in self.flux.loras():
                    self.flux.lora_remove(name)
                raise
        return name

    def set_lora_weight(self, name: str, weight: float):
        with self._lock:
            self.flux.lora_set_weight(name, weight)

    def unload_lora(self, name: Optional[str] = None):
        """Drop one adapter (None: all of them): the Linears it touched are recomputed from the loaded weights and the adapters that remain."""
        with self._lock:
            self.flux.lora_remove(name)

    def loras(self) -> List[str]:
        with self._lock:
            return self.flux.loras()

    def enable_sequence_parallel(self, group=None):
        """Single-image latency mode: the ranks of `group` (default: all of torch.distributed) denoise every
        image TOGETHER, each on 1/N of its tokens (dist.SequenceParallel; two all-to-alls per transformer block), instead of
        sharding the prompt list.  Every rank must call forward / generate_tensor with the same arguments."""
        from . import dist as D
        self._sp = D.SequenceParallel(self.device, group)
        self._sp.attach(self.flux)
        return self._sp

    def disable_sequence_parallel(self):
        if getattr(self, "_sp", None) is not None:
            self._sp.detach(self.flux)
            self._sp = None

    def forward(self, prompts: List[str], params: DiffusionGenerationParams, *, output: str = "png", image=None, strength: float = 1.0, mask=None,
                reference=None, return_latents: bool = False, cache_threshold: Optional[float] = None, solver: Optional[str] = None,
                negative_prompt: Optional[str] = None, negative_embeddings=None, negative_token_ids=None, true_cfg_scale: float = 1.0, control_image=None, control_mask=None, controlnet_image=None,
                controlnet_conditioning_scale: float = 1.0, control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, ip_adapter_image_embeds=None,
                negative_ip_adapter_image_embeds=None, ip_adapter_scale: float = 1.0, ip_adapter_start: float = 0.0, ip_adapter_end: float = 1.0,
                ip_adapter_image=None, negative_ip_adapter_image=None, redux_image=None, redux_image_embeds=None, redux_scale: float = 1.0, **kw):
        """== Pipeline::forward (pipelines/mod.rs:241-270) + the PNG encode of the pyo3 binding.
        With torch.distributed initialised the batch is sharded (prompt i on rank i % world, no data-path collective) and
        the images are gathered to rank 0; every rank must make the same call, ranks != 0 return None.
        image= / strength= / mask=: image to image and inpainting, reference=: reference-image conditioning, see generate_tensor; return_latents=True
        returns (images, final packed latents).  cache_threshold=: the first-block step cache, see generate_tensor (None: off); each rank of a sharded batch
        decides for its own prompts and keeps its own `last_cache_stats`.  negative_prompt= / negative_embeddings= / negative_token_ids= / true_cfg_scale=: true
        classifier-free guidance, see generate_tensor — one negative per request, handed to every rank of a sharded batch unchanged.  control_image= /
        control_mask=: the control of a channel-conditioned model (FLUX.1 Fill / Canny / Depth), see generate_tensor — one per request, likewise.
        controlnet_image= / controlnet_conditioning_scale= / control_guidance_start= / control_guidance_end=: the ControlNet of load_controlnet, see generate_tensor —
        one control image per request, likewise (every rank loads the same ControlNet).
        ip_adapter_image_embeds= / negative_ip_adapter_image_embeds= / ip_adapter_scale= / ip_adapter_start= / ip_adapter_end=: the image prompt of the IP-Adapter of
        load_ip_adapter, see generate_tensor — one embedding per request, likewise (every rank loads the same adapter).  ip_adapter_image= /
        negative_ip_adapter_image=: the same prompt as a picture, encoded by the image encoder of load_image_encoder (every rank loads the same one and encodes
        the picture itself).
        redux_image= / redux_image_embeds= / redux_scale=: FLUX.1 Redux image variation (load_redux), see generate_tensor — one picture per request, likewise
        (every rank loads the same Redux and encodes the picture itself).
        solver=: None | "euler" | "heun" | "dpmpp_2m", the integrator of the denoise loop, see generate_tensor."""
        from . import dist as D
        rank, world = D.world()
        shared = dict(seed=kw.pop("seed", None), strength=strength, return_latents=return_latents, cache_threshold=cache_threshold)
        options = dict(negative_prompt=negative_prompt, negative_embeddings=negative_embeddings, negative_token_ids=negative_token_ids, true_cfg_scale=true_cfg_scale,
                       control_image=control_image, control_mask=control_mask, controlnet_image=controlnet_image,
                       controlnet_conditioning_scale=controlnet_conditioning_scale, control_guidance_start=control_guidance_start,
                       control_guidance_end=control_guidance_end, ip_adapter_image_embeds=ip_adapter_image_embeds,
                       negative_ip_adapter_image_embeds=negative_ip_adapter_image_embeds, ip_adapter_scale=ip_adapter_scale, ip_adapter_start=ip_adapter_start,
                       ip_adapter_end=ip_adapter_end, ip_adapter_image=ip_adapter_image, negative_ip_adapter_image=negative_ip_adapter_image,
                       redux_image=redux_image, redux_image_embeds=redux_image_embeds, redux_scale=redux_scale, solver=solver)
        defaults = inspect.signature(Pipeline.generate_tensor).parameters
        for name, value in options.items():  # only what differs from generate_tensor's own default: any other request makes exactly the call it always made
            default = defaults[name].default
            if (value is not None) if default is None else value != default:
                shared[name] = value
        per_sample = dict(kw, image=image, mask=mask, reference=reference)  # with embeddings= / token_ids= / latents= / first_sample=, which ride in **kw
        final = None  # return_latents=True: the final packed latents, returned next to the images
        if world > 1 and getattr(self, "_sp", None) is None:
            if return_latents:
                raise ValueError("return_latents= is not gathered across ranks: call generate_tensor on the rank that holds the sample")
            # normalised once (batched device tensors), so that a rank takes its rows of an image exactly as it takes its rows of `latents`
            s = self._samples(prompts, params, strength, **per_sample)

            def run_local(my_prompts, ids):
                return self.generate_tensor(my_prompts, params, **s.take(ids).kwargs(), **shared)

            if getattr(self, "_int8_pending", False) and s.prompts:
                # every rank calibrates on the SAME sample — global sample 0 of this request — so that all ranks hold the same int8 weights and an image does
                # not depend on the rank that produced it (one extra image per rank, once per model)
                run_local(s.prompts[:1], [0])
            u8 = D.generate_sharded(prompts, run_local,
                                    empty=lambda: torch.empty((0, 3, params.height, params.width), dtype=torch.uint8, device=self.device))
            assert rank != 0 or u8.shape[0] == len(prompts)
        else:  # one process, or sequence parallel: all ranks produce every image together
            u8 = self.generate_tensor(prompts, params, **per_sample, **shared)
            if return_latents:
                u8, final = u8
        if rank != 0:  # rank 0 returns the images
            return None
        if output == "tensor":
            out = u8
        else:
            hwc = u8.permute(0, 2, 3, 1).contiguous().cpu().numpy()
            out = [hwc[i] for i in range(hwc.shape[0])] if output == "rgb" else [encode_png(hwc[i]) for i in range(hwc.shape[0])]
        return (out, final) if return_latents else out
