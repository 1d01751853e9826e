"""Weight ingestion: diffusers directories, DDUF archives and HF-bitsandbytes
tensor naming, feeding the C-ABI's fmi_flux_set_tensor / fmi_flux_set_linear_bnb4 / fmi_vae_set_tensor.

  FileLoader      <-> diffusion_rs_common::model_source::FileLoader (model_source.rs:87-259):
                      a local directory, or a DDUF file = a zip whose entries are STORED
                      (uncompressed) so tensors can be sliced straight out of the mmap
                      (model_source.rs:225-232, varbuilder_loading.rs:111-117).
  load_flux       <-> FluxModel::new over a VarBuilder (model.rs:722-787) + the bnb detection of
                      diffusion_rs_backend::linear_b (lib.rs:197-266): a linear whose prefix has
                      `weight.absmax` / `weight.quant_state.bitsandbytes__{nf4,fp4}` is 4-bit
                      (bitsandbytes/mod.rs:137-222), nested absmax resolved as mod.rs:230-239.
  load_flux_gguf / load_flux_single_file
                      single-file transformers (not wired to FLUX in the reference): a .gguf of ggml blocks, or one .safetensors in BFL /
                      diffusers naming whose weights may be 8-bit floats (F8_E4M3 / F8_E5M2) — DESIGN.md 4.16 and 4.20.
There is no network here: hub model ids must already be local directories.
"""
import io
import json
import warnings
import mmap
import os
import struct
import zipfile
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch

from . import synth
from .text import CLIP_IMAGE_MEAN, CLIP_IMAGE_STD, CLIP_VISION_L, SIGLIP_IMAGE_MEAN, SIGLIP_IMAGE_STD, SIGLIP_SO400M

_ST_DTYPES = {"F32": (torch.float32, 4), "F16": (torch.float16, 2), "BF16": (torch.bfloat16, 2), "U8": (torch.uint8, 1), "I8": (torch.int8, 1),
              "I32": (torch.int32, 4), "I64": (torch.int64, 8), "F64": (torch.float64, 8),
              "F8_E4M3": (torch.float8_e4m3fn, 1), "F8_E5M2": (torch.float8_e5m2, 1)}  # (OCP e4m3fn / e5m2: single-file fp8 checkpoints)


SUPPORTED_PIPELINES = ("FluxPipeline", "FluxKontextPipeline")  # Kontext: the same components, FLUX.1-dev's transformer


def check_pipeline_class(class_name) -> str:
    """model_index.json's `_class_name` (pipelines/mod.rs:146-149): a pipeline this package loads, or ValueError."""
    if class_name not in SUPPORTED_PIPELINES:
        raise ValueError("Only FluxPipeline is supported")
    return class_name


# model_index.json's `_class_name` -> how the transformer is conditioned: None = on the text alone (a Kontext reference joins per request),
# "control" = the 64 latent channels of a control image next to the state's (FLUX.1 Canny-dev / Depth-dev), "fill" = the 64 masked-image latents and 256 mask
# channels of FLUX.1 Fill-dev.  The value is in_channels - out_channels of transformer/config.json.
PIPELINE_CONDITIONING = {"FluxPipeline": None, "FluxKontextPipeline": None, "FluxControlPipeline": "control", "FluxFillPipeline": "fill"}
CONDITIONING_CHANNELS = {None: 0, "control": 64, "fill": 320}


def pipeline_conditioning(class_name) -> Optional[str]:
    """The conditioning of a pipeline class this package loads (None | "control" | "fill"), or check_pipeline_class's ValueError for any other."""
    if class_name not in PIPELINE_CONDITIONING:
        raise ValueError("Only FluxPipeline is supported")
    return PIPELINE_CONDITIONING[class_name]


def check_conditioning_channels(class_name, in_channels: int, out_channels=None) -> Optional[str]:
    """pipeline_conditioning(class_name), checked against transformer/config.json: in_channels - out_channels (null / absent: in_channels) must be the
    class's 0 / 64 / 320, else ValueError."""
    kind = pipeline_conditioning(class_name)
    extra = int(in_channels) - int(out_channels or in_channels)
    if extra != CONDITIONING_CHANNELS[kind]:
        raise ValueError(f"{class_name} expects {CONDITIONING_CHANNELS[kind]} conditioning channels, transformer/config.json has in_channels {in_channels} and "
                         f"out_channels {out_channels} ({extra})")
    return kind


def _safetensors_from_buffer(buf) -> Iterator[Tuple[str, torch.Tensor]]:
    """Zero-copy views of every tensor in a safetensors image held in `buf` (mmap / memoryview)."""
    n = struct.unpack("<Q", bytes(buf[:8]))[0]
    header = json.loads(bytes(buf[8:8 + n]))
    base = 8 + n
    for name, meta in header.items():
        if name == "__metadata__":
            continue
        dt, _ = _ST_DTYPES[meta["dtype"]]
        a, b = meta["data_offsets"]
        with warnings.catch_warnings():  # read-only mmap views are intended: tensors are only copied to the device
            warnings.simplefilter("ignore", UserWarning)
            t = torch.frombuffer(buf, dtype=dt, count=(b - a) // _ST_DTYPES[meta["dtype"]][1], offset=base + a) if b > a else torch.empty(0, dtype=dt)
        yield name, t.reshape(meta["shape"])


class FileLoader:
    """Directory or DDUF view of a diffusers checkpoint: list_files / read_json / tensors(component)."""

    def __init__(self, path: str):
        self.path = path
        self._mm = None
        if os.path.isdir(path):
            self.kind = "dir"
            self.files = sorted(os.path.relpath(os.path.join(r, f), path) for r, _, fs in os.walk(path) for f in fs)
        elif zipfile.is_zipfile(path):
            self.kind = "dduf"
            self._f = open(path, "rb")
            self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
            self._zip = zipfile.ZipFile(path)
            self._info = {i.filename: i for i in self._zip.infolist() if not i.is_dir()}
            for i in self._info.values():
                if i.compress_type != zipfile.ZIP_STORED:
                    raise ValueError(f"{path}: DDUF entries must be stored uncompressed ({i.filename} is compressed)")
            self.files = sorted(self._info)
        else:
            raise FileNotFoundError(f"{path}: not a directory or DDUF (zip) file; hub ids need network access, which this build does not have")

    def list_files(self) -> List[str]:
        return self.files

    def _entry_view(self, name: str) -> memoryview:
        """Slice of the mmap holding a stored zip entry (data_start()..+size, model_source.rs:225-232)."""
        i = self._info[name]
        hdr = self._mm[i.header_offset:i.header_offset + 30]
        nlen, elen = struct.unpack("<HH", hdr[26:30])
        start = i.header_offset + 30 + nlen + elen
        return memoryview(self._mm)[start:start + i.file_size]

    def read_json(self, name: str) -> dict:
        if self.kind == "dir":
            with open(os.path.join(self.path, name)) as f:
                return json.load(f)
        return json.loads(bytes(self._entry_view(name)))

    def read_text(self, name: str) -> str:
        if self.kind == "dir":
            with open(os.path.join(self.path, name), encoding="utf-8") as f:
                return f.read()
        return bytes(self._entry_view(name)).decode("utf-8")

    def has(self, name: str) -> bool:
        return name in self.files

    def tensors(self, component: str) -> Iterator[Tuple[str, torch.Tensor]]:
        """All tensors of every *.safetensors shard under `component/` (shards in name order)."""
        for fn in self.files:
            if not (fn.startswith(component + "/") and fn.endswith(".safetensors")):
                continue
            if self.kind == "dir":
                with open(os.path.join(self.path, fn), "rb") as f:
                    mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
                yield from _safetensors_from_buffer(memoryview(mm))
            else:
                yield from _safetensors_from_buffer(self._entry_view(fn))


def _resolve_absmax(lib, group: Dict[str, torch.Tensor], state: dict, device) -> torch.Tensor:
    """f32 absmax of a 4-bit weight; nested (double-quantised) absmax per bitsandbytes/mod.rs:230-239:
    absmax = dequantize_int8(absmax_u8, nested_quant_map, nested_absmax, nested_blocksize) + nested_offset."""
    import ctypes as C
    absmax = group["weight.absmax"]
    if "weight.nested_absmax" not in group:
        return absmax.to(torch.float32)
    a8 = absmax.to(device=device, dtype=torch.uint8).contiguous()
    code = group["weight.nested_quant_map"].to(device=device, dtype=torch.float32).contiguous()
    nabs = group["weight.nested_absmax"].to(device=device, dtype=torch.float32).contiguous()
    out = torch.empty(a8.numel(), dtype=torch.float32, device=device)
    lib.dequantize_blockwise_f32_int8(C.c_void_p(code.data_ptr()), C.c_void_p(a8.data_ptr()), C.c_void_p(nabs.data_ptr()), C.c_void_p(out.data_ptr()),
                                      int(state["nested_blocksize"]), a8.numel(), None)
    torch.cuda.synchronize()
    return out + float(state["nested_offset"])


def _feed_linears(model, tensors: Iterator[Tuple[str, torch.Tensor]], want: dict, on_extra=None) -> dict:
    """Shared by load_flux and load_text_encoder: feed `model` (set_tensor / set_linear_bnb4 / set_linear_int8, .device) from
    (name, tensor) pairs.  bitsandbytes layers arrive as groups of tensors — "<prefix>.weight" (packed u8 or int8) with
    "<prefix>.weight.absmax", ".weight.quant_map", ".weight.quant_state.bitsandbytes__nf4|fp4" (+ the nested_* tensors of double
    quantisation), or "<prefix>.SCB" for LLM.int8 — the naming BnbLinear::linear_b reads (bitsandbytes/mod.rs:111-239).
    `on_extra(name, tensor) -> bool` may claim a name the model does not list.  Returns {"dense", "bnb4", "int8", "skipped"}."""
    from . import _lib as L
    lib = L.load()
    stats = {"dense": 0, "bnb4": 0, "int8": 0, "skipped": []}
    pending: Dict[str, Dict[str, torch.Tensor]] = {}
    for name, t in tensors:
        if ".weight." in name:
            prefix, rest = name.split(".weight.", 1)
            pending.setdefault(prefix, {})["weight." + rest] = t
            continue
        if name.endswith(".SCB"):  # LLM.int8 row scales (bitsandbytes/mod.rs:113,126)
            pending.setdefault(name[:-len(".SCB")], {})["SCB"] = t
            continue
        if name.endswith(".weight_format"):
            continue
        if name.endswith(".weight") and t.dtype in (torch.uint8, torch.int8):  # packed 4-bit / int8 weight of a bnb linear
            pending.setdefault(name[:-len(".weight")], {})["weight"] = t
            continue
        if name in want:
            model.set_tensor(name, t)
            stats["dense"] += 1
        elif on_extra is not None and on_extra(name, t):
            stats["dense"] += 1
        else:
            stats["skipped"].append(name)
    for prefix, group in pending.items():
        if prefix + ".weight" not in want:
            stats["skipped"].append(prefix + ".weight")
            continue
        out_f, in_f = want[prefix + ".weight"]
        if "SCB" in group:  # BnbLinear::Int8
            if "weight" not in group or group["weight"].dtype != torch.int8:
                raise ValueError(f"`BnbLinear` int8 layer {prefix} needs an int8 `weight` next to `SCB`")
            if tuple(group["weight"].shape) != (out_f, in_f) or group["SCB"].numel() != out_f:
                raise ValueError(f"{prefix}: int8 weight {tuple(group['weight'].shape)} / SCB {tuple(group['SCB'].shape)} != expected {(out_f, in_f)}")
            model.set_linear_int8(prefix, group["weight"], group["SCB"], out_f, in_f)
            stats["int8"] += 1
            continue
        qkey = next((k for k in group if k.startswith("weight.quant_state.bitsandbytes__")), None)
        if qkey is None or "weight" not in group or "weight.absmax" not in group:
            raise ValueError(f"`BnbLinear` expects fp4/nf4 layers: incomplete tensors for {prefix}: {sorted(group)}")  # bitsandbytes/mod.rs:120
        qt = qkey.rsplit("__", 1)[1]
        state = json.loads(bytes(group[qkey].numpy().tobytes()))
        if list(state["shape"]) != [out_f, in_f]:
            raise ValueError(f"{prefix}: quant_state shape {state['shape']} != expected {(out_f, in_f)}")
        absmax = _resolve_absmax(lib, group, state, model.device)
        model.set_linear_bnb4(prefix, group["weight"].reshape(-1), absmax, int(state["blocksize"]), qt, out_f, in_f)
        stats["bnb4"] += 1
    return stats


def load_flux(flux, tensors: Iterator[Tuple[str, torch.Tensor]]) -> dict:
    """Feed a FluxModel from (name, tensor) pairs; returns {"dense": n, "bnb4": n, "int8": n, "skipped": [...]}."""
    stats = _feed_linears(flux, tensors, synth.flux_tensor_shapes(flux.cfg))
    flux.assert_complete()
    return stats


def controlnet_config(config: dict) -> dict:
    """The FluxControlNetModel configuration of a diffusers config.json as this package's cfg dict, or ValueError naming the field: `_class_name`
    is not FluxControlNetModel; `num_mode` not null (union ControlNets); `conditioning_embedding_channels` not null (XLabs' pixel-space hint block);
    `attention_head_dim` != 128.  Out of scope, all three."""
    if config.get("_class_name") != "FluxControlNetModel":
        raise ValueError(f"_class_name is {config.get('_class_name')!r}: only FluxControlNetModel is a ControlNet this package loads")
    if config.get("num_mode") is not None:
        raise ValueError(f"num_mode = {config['num_mode']!r}: union ControlNets are not supported")
    if config.get("conditioning_embedding_channels") is not None:
        raise ValueError(f"conditioning_embedding_channels = {config['conditioning_embedding_channels']!r}: the pixel-space hint block (XLabs) is not supported")
    if int(config.get("attention_head_dim", 128)) != 128:
        raise ValueError(f"attention_head_dim = {config['attention_head_dim']!r}: only 128 is supported")
    axes = [int(v) for v in config.get("axes_dims_rope", [16, 56, 56])]
    return dict(in_channels=int(config.get("in_channels", 64)), pooled_projection_dim=int(config.get("pooled_projection_dim", 768)),
                joint_attention_dim=int(config.get("joint_attention_dim", 4096)), num_attention_heads=int(config.get("num_attention_heads", 24)),
                num_layers=int(config.get("num_layers", 19)), num_single_layers=int(config.get("num_single_layers", 38)),
                guidance_embeds=bool(config.get("guidance_embeds", False)), axes_dim=axes, theta=10000)


def load_controlnet(path: str):
    """A diffusers ControlNet directory — config.json with `_class_name` FluxControlNetModel next to diffusion_pytorch_model*.safetensors — as
    (cfg, {name: tensor}): what Pipeline.load_controlnet and FluxControlNetModel.load_state_dict take.  No device is touched.  ValueError as controlnet_config's,
    for a tensor the configuration does not list, and for one it lists that the files lack."""
    if not os.path.isdir(path):
        raise FileNotFoundError(f"{path}: not a directory (a ControlNet is a diffusers directory: config.json + diffusion_pytorch_model*.safetensors)")
    with open(os.path.join(path, "config.json")) as f:
        cfg = controlnet_config(json.load(f))
    want = synth.controlnet_tensor_shapes(cfg)
    sd = {}
    for fn in sorted(os.listdir(path)):
        if not (fn.startswith("diffusion_pytorch_model") and fn.endswith(".safetensors")):
            continue
        with open(os.path.join(path, fn), "rb") as f:
            mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        for name, t in _safetensors_from_buffer(memoryview(mm)):
            if name not in want:
                raise ValueError(f"{fn}: tensor {name} is not part of a FluxControlNetModel of this configuration (quantised ControlNets are not supported)")
            if tuple(t.shape) != tuple(want[name]):
                raise ValueError(f"{fn}: {name} is {tuple(t.shape)}, the configuration says {tuple(want[name])}")
            sd[name] = t
    missing = [k for k in want if k not in sd]
    if missing:
        raise ValueError(f"{path}: {len(missing)} ControlNet tensors missing, e.g. {missing[:3]}")
    return cfg, sd


def ip_adapter_key_map(name: str) -> Optional[str]:
    """An IP-Adapter tensor's name under either naming as the diffusers-converted one this package uses, or None for a name of neither:
      XLabs      ip_adapter_proj_model.{proj,norm}.*                    double_blocks.{i}.processor.ip_adapter_double_stream_{k,v}_proj.*
      diffusers  image_proj.{image_embeds,norm}.*                       ip_adapter.{i}.to_{k,v}_ip.*"""
    parts = name.split(".")
    if parts[-1] not in ("weight", "bias"):
        return None
    if len(parts) == 3 and parts[0] == "ip_adapter_proj_model" and parts[1] in ("proj", "norm"):
        return f"image_proj.{'image_embeds' if parts[1] == 'proj' else 'norm'}.{parts[2]}"
    if len(parts) == 3 and parts[0] == "image_proj" and parts[1] in ("image_embeds", "norm"):
        return name
    if len(parts) == 5 and parts[0] == "double_blocks" and parts[1].isdigit() and parts[2] == "processor" and \
            parts[3] in ("ip_adapter_double_stream_k_proj", "ip_adapter_double_stream_v_proj"):
        return f"ip_adapter.{int(parts[1])}.to_{parts[3][-6]}_ip.{parts[4]}"
    if len(parts) == 4 and parts[0] == "ip_adapter" and parts[1].isdigit() and parts[2] in ("to_k_ip", "to_v_ip"):
        return f"ip_adapter.{int(parts[1])}.{parts[2]}.{parts[3]}"
    return None


def ip_adapter_from_tensors(cfg: dict, tensors, where: str = "ip_adapter"):
    """(embed_dim, num_tokens, {converted name: tensor}) of an IP-Adapter's tensors under either naming, for a transformer of config cfg; N and E are read from
    the shapes.  ValueError naming the keys: a name of neither naming; a required tensor the file lacks (the biases of to_k_ip / to_v_ip are optional); a shape
    that does not fit cfg; an image projection whose rows are no multiple of joint_attention_dim."""
    sd, unexpected = {}, []
    for name, t in (tensors.items() if isinstance(tensors, dict) else tensors):
        k = ip_adapter_key_map(name)
        if k is None:
            unexpected.append(name)
        else:
            sd[k] = t
    if unexpected:
        raise ValueError(f"{where}: {len(unexpected)} unexpected tensors (neither XLabs nor diffusers IP-Adapter names), e.g. {sorted(unexpected)[:3]}")
    J = int(cfg["joint_attention_dim"])
    pw = sd.get("image_proj.image_embeds.weight")
    if pw is None or len(pw.shape) != 2:
        raise ValueError(f"{where}: 1 IP-Adapter tensors missing, e.g. ['image_proj.image_embeds.weight']")
    rows, E = int(pw.shape[0]), int(pw.shape[1])
    if rows % J or rows == 0:
        raise ValueError(f"{where}: image_proj.image_embeds.weight has {rows} rows, no multiple of joint_attention_dim = {J}")
    N = rows // J
    want = synth.ip_adapter_tensor_shapes(cfg, E, N)
    optional = {k for k in want if k.startswith("ip_adapter.") and k.endswith(".bias")}
    extra = sorted(k for k in sd if k not in want)
    if extra:
        raise ValueError(f"{where}: {len(extra)} unexpected tensors (the transformer has {cfg['num_layers']} double blocks), e.g. {extra[:3]}")
    missing = [k for k in want if k not in sd and k not in optional]
    if missing:
        raise ValueError(f"{where}: {len(missing)} IP-Adapter tensors missing, e.g. {missing[:3]}")
    for k, t in sd.items():
        if tuple(t.shape) != tuple(want[k]):
            raise ValueError(f"{where}: {k} is {tuple(t.shape)}, expected {tuple(want[k])}")
    return E, N, sd


def load_ip_adapter(path: str, cfg: dict):
    """An IP-Adapter file (.safetensors, XLabs or diffusers-converted names) for a transformer of config cfg as (embed_dim, num_tokens, {name: tensor}).  No device
    is touched.  ValueError as ip_adapter_from_tensors'."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: not a file (an IP-Adapter is one .safetensors file)")
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    return ip_adapter_from_tensors(cfg, dict(_safetensors_from_buffer(memoryview(mm))), os.path.basename(path))


CLIP_VISION_KEYS = tuple(CLIP_VISION_L)


def _safetensors_in(path: str) -> dict:
    """Every tensor of the *.safetensors files of a directory, in file-name order."""
    tensors = {}
    for fn in sorted(os.listdir(path)):
        if fn.endswith(".safetensors"):
            with open(os.path.join(path, fn), "rb") as f:
                mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            tensors.update(_safetensors_from_buffer(memoryview(mm)))
    return tensors


def _image_processor(pre: Optional[dict], defaults, switches, size_rule) -> Tuple[tuple, tuple]:
    """(image_mean, image_std) of a preprocessor_config.json (None: `defaults`, the tower's constants).  What a tower's preprocess does is fixed, so a processor
    that asks for anything else is refused by name: a switch that is not as the tower has it (switches: (flag, the value it must have, what the tower does
    instead, in the refusal's words)), a resample other than bicubic, a rescale factor other than 1 / 255, a size the tower's own size_rule(pre) raises for."""
    if pre is None:
        return defaults
    for flag, wanted, instead in switches:
        if bool(pre.get(flag, wanted)) != wanted:
            raise ValueError(f"preprocessor_config.json has {flag} = {'false' if wanted else 'true'}: {instead}")
    if int(pre.get("resample", 3)) != 3:
        raise ValueError(f"preprocessor_config.json has resample = {pre['resample']!r}: only 3 (PIL's BICUBIC) is supported")
    if abs(float(pre.get("rescale_factor", 1 / 255)) - 1 / 255) > 1e-9:
        raise ValueError(f"preprocessor_config.json has rescale_factor = {pre['rescale_factor']!r}: only 1 / 255 is supported")
    size_rule(pre)
    mean, std = pre.get("image_mean", defaults[0]), pre.get("image_std", defaults[1])
    if len(mean) != 3 or len(std) != 3 or not all(float(s) > 0 for s in std):
        raise ValueError(f"preprocessor_config.json: image_mean / image_std must hold 3 values, the std positive, got {mean!r} / {std!r}")
    return tuple(float(m) for m in mean), tuple(float(s) for s in std)


def _tower_from_tensors(want: dict, tensors, where: str, rename, ignored, model: str, part: str) -> dict:
    """{name: tensor} of the tensors `want` ({name: shape}) out of a checkpoint's.  rename(name): the model's name of a checkpoint key (a key that already is
    one wins over a key that becomes the same one); ignored(name): a key the checkpoint may carry and the model does not read.  ValueError naming the keys: an
    unexpected tensor ("not <model>'s"), a missing one ("<part> tensors missing"), a shape that does not fit."""
    sd, unexpected = {}, []
    for name, t in (tensors.items() if isinstance(tensors, dict) else tensors):
        full = rename(name)
        if full in want and (full == name or full not in sd):
            sd[full] = t
        elif not ignored(name):
            unexpected.append(name)
    if unexpected:
        raise ValueError(f"{where}: {len(unexpected)} unexpected tensors (not {model}'s), e.g. {sorted(unexpected)[:3]}")
    missing = [k for k in want if k not in sd]
    if missing:
        raise ValueError(f"{where}: {len(missing)} {part} tensors missing, e.g. {missing[:3]}")
    for k, t in sd.items():
        if tuple(t.shape) != tuple(want[k]):
            raise ValueError(f"{where}: {k} is {tuple(t.shape)}, expected {tuple(want[k])}")
    return sd


def clip_vision_config(config: dict) -> dict:
    """The vision tower's configuration (CLIP_VISION_KEYS) from a config.json: a CLIPVisionConfig, or a full CLIPConfig, whose `vision_config` is used (with the
    top level's projection_dim where the nested one has none).  ValueError by name for a missing field, an activation other than quick_gelu and a
    layer_norm_eps other than 1e-5 — what the kernels compute."""
    if not isinstance(config, dict):
        raise ValueError("config.json of an image encoder must hold an object")
    vc = config
    if isinstance(config.get("vision_config"), dict):
        vc = dict(config["vision_config"])
        vc.setdefault("projection_dim", config.get("projection_dim"))
    elif config.get("model_type") not in (None, "clip_vision_model"):
        raise ValueError(f"config.json has model_type {config.get('model_type')!r} and no vision_config: a CLIPVisionConfig or a CLIPConfig is expected "
                         f"(a SigLIP tower is FLUX.1 Redux's: load_siglip_vision; other towers are not supported)")
    missing = [k for k in CLIP_VISION_KEYS if vc.get(k) is None]
    if missing:
        raise ValueError(f"the image encoder's config.json lacks {missing}")
    if vc.get("hidden_act", "quick_gelu") != "quick_gelu":
        raise ValueError(f"the image encoder's hidden_act is {vc['hidden_act']!r}: only quick_gelu (CLIP ViT-L/14) is supported")
    if abs(float(vc.get("layer_norm_eps", 1e-5)) - 1e-5) > 1e-12:
        raise ValueError(f"the image encoder's layer_norm_eps is {vc['layer_norm_eps']!r}: only 1e-05 is supported")
    if int(vc.get("num_channels", 3)) != 3:
        raise ValueError(f"the image encoder's num_channels is {vc['num_channels']!r}: only 3 (RGB) is supported")
    return {k: int(vc[k]) for k in CLIP_VISION_KEYS}


def clip_image_processor(pre: Optional[dict], image_size: int) -> Tuple[tuple, tuple]:
    """(image_mean, image_std) of a preprocessor_config.json (None: CLIP's constants).  What ClipVisionModel.preprocess does is fixed — bicubic resize of the
    shortest edge to image_size, centre crop to image_size, rescale by 1 / 255, normalise — so a processor that asks for anything else is refused by name."""
    always = "the image encoder always resizes, centre-crops, rescales and normalises"

    def edge(v, keys):
        if isinstance(v, dict):
            vals = {int(v[k]) for k in keys if k in v}
            if len(vals) != 1 or set(v) - set(keys):
                return None
            return vals.pop()
        return None if v is None else int(v)

    def size_rule(pre):
        size, crop = pre.get("size", image_size), pre.get("crop_size", image_size)
        if edge(size, ("shortest_edge",)) != image_size:
            raise ValueError(f"preprocessor_config.json has size = {size!r}: the shortest edge is resized to the model's image_size = {image_size}")
        if edge(crop, ("height", "width")) != image_size:
            raise ValueError(f"preprocessor_config.json has crop_size = {crop!r}: the centre crop is the model's image_size = {image_size}")

    return _image_processor(pre, (CLIP_IMAGE_MEAN, CLIP_IMAGE_STD), [(f, True, always) for f in ("do_resize", "do_center_crop", "do_rescale", "do_normalize")], size_rule)


def _clip_vision_ignored(name: str) -> bool:
    """The keys of a full CLIP checkpoint (openai/clip-vit-large-patch14) the vision tower does not read: the text tower, its projection, the logit scale, and
    the position_ids buffer older checkpoints carry."""
    return name.startswith("text_model.") or name in ("text_projection.weight", "logit_scale", "vision_model.embeddings.position_ids")


def clip_vision_from_tensors(cfg: dict, tensors, where: str = "image encoder") -> dict:
    """{name: tensor} of the vision tower of configuration cfg from a CLIPVisionModelWithProjection or a full CLIPModel checkpoint's tensors.  ValueError naming
    the keys: an unexpected tensor (anything but the ignored ones of a full checkpoint), a missing one, a shape that does not fit cfg."""
    return _tower_from_tensors(synth.clip_vision_tensor_shapes(cfg), tensors, where, lambda name: name, _clip_vision_ignored, "CLIPVisionModelWithProjection", "image-encoder")


def load_clip_vision(path: str):
    """A CLIP image-encoder directory — config.json (a CLIPVisionConfig or a full CLIPConfig) next to *.safetensors, with an optional preprocessor_config.json —
    as (cfg, {name: tensor}): cfg holds CLIP_VISION_KEYS plus image_mean / image_std, what Pipeline.load_image_encoder and ClipVisionModel take.  No device is
    touched.  ValueError as clip_vision_config's, clip_image_processor's and clip_vision_from_tensors'."""
    if not os.path.isdir(path):
        raise FileNotFoundError(f"{path}: not a directory (an image encoder is a directory: config.json + *.safetensors)")
    with open(os.path.join(path, "config.json")) as f:
        cfg = clip_vision_config(json.load(f))
    pre = None
    if os.path.isfile(os.path.join(path, "preprocessor_config.json")):
        with open(os.path.join(path, "preprocessor_config.json")) as f:
            pre = json.load(f)
    mean, std = clip_image_processor(pre, cfg["image_size"])
    return dict(cfg, image_mean=mean, image_std=std), clip_vision_from_tensors(cfg, _safetensors_in(path), os.path.basename(os.path.normpath(path)))


SIGLIP_VISION_KEYS = tuple(SIGLIP_SO400M)


def siglip_vision_config(config: dict) -> dict:
    """The vision tower's configuration (SIGLIP_VISION_KEYS) from a config.json: a SiglipVisionConfig, or a full SiglipConfig, whose `vision_config` is used and
    whose text tower is ignored.  Fields a SiglipVisionConfig leaves out take HuggingFace's defaults where it has them (layer_norm_eps 1e-6, hidden_act
    gelu_pytorch_tanh, num_channels 3).  ValueError by name for a missing field, an activation other than gelu_pytorch_tanh, channels other than 3, and a
    model_type that is no SigLIP's."""
    if not isinstance(config, dict):
        raise ValueError("config.json of a SigLIP image encoder must hold an object")
    vc = config
    if isinstance(config.get("vision_config"), dict):
        if config.get("model_type") not in (None, "siglip"):
            raise ValueError(f"config.json has model_type {config.get('model_type')!r}: a SiglipVisionConfig or a SiglipConfig is expected")
        vc = dict(config["vision_config"])
    if vc.get("model_type") not in (None, "siglip_vision_model"):
        raise ValueError(f"config.json has model_type {vc.get('model_type')!r}: a SiglipVisionConfig or a SiglipConfig is expected (a CLIP tower is the "
                         f"IP-Adapter's: load_clip_vision)")
    missing = [k for k in SIGLIP_VISION_KEYS if k != "layer_norm_eps" and vc.get(k) is None]
    if missing:
        raise ValueError(f"the SigLIP image encoder's config.json lacks {missing}")
    if vc.get("hidden_act", "gelu_pytorch_tanh") != "gelu_pytorch_tanh":
        raise ValueError(f"the SigLIP image encoder's hidden_act is {vc['hidden_act']!r}: only gelu_pytorch_tanh is supported")
    if int(vc.get("num_channels", 3)) != 3:
        raise ValueError(f"the SigLIP image encoder's num_channels is {vc['num_channels']!r}: only 3 (RGB) is supported")
    eps = float(vc.get("layer_norm_eps", 1e-6))
    if not (eps > 0 and np.isfinite(eps)):
        raise ValueError(f"the SigLIP image encoder's layer_norm_eps is {vc['layer_norm_eps']!r}: it must be positive")
    return dict({k: int(vc[k]) for k in SIGLIP_VISION_KEYS if k != "layer_norm_eps"}, layer_norm_eps=eps)


def siglip_image_processor(pre: Optional[dict], image_size: int) -> Tuple[tuple, tuple]:
    """(image_mean, image_std) of a preprocessor_config.json (None: SigLIP's constants, 0.5 each).  What SiglipVisionModel.preprocess does is fixed — a bicubic
    resize straight to image_size x image_size, rescale by 1 / 255, normalise — so a processor that asks for anything else is refused by name."""
    always = "the SigLIP image encoder always resizes, rescales and normalises"
    switches = [(f, True, always) for f in ("do_resize", "do_rescale", "do_normalize")]
    switches.append(("do_center_crop", False, "the SigLIP image encoder resizes straight to the square and never crops"))

    def size_rule(pre):
        size = pre.get("size", image_size)
        hw = (size.get("height"), size.get("width")) if isinstance(size, dict) and set(size) == {"height", "width"} else (size, size) if isinstance(size, int) else None
        if hw is None or tuple(int(v) for v in hw) != (image_size, image_size):
            raise ValueError(f"preprocessor_config.json has size = {size!r}: the picture is resized to the model's image_size = {image_size}, height and width")

    return _image_processor(pre, (SIGLIP_IMAGE_MEAN, SIGLIP_IMAGE_STD), switches, size_rule)


def siglip_vision_from_tensors(cfg: dict, tensors, where: str = "SigLIP image encoder") -> dict:
    """{name: tensor} of the vision tower of configuration cfg, under the `vision_model.` names, from a SiglipVisionModel or a full SiglipModel checkpoint's
    tensors.  A checkpoint may carry the tower's keys with the `vision_model.` prefix (the published ones) or without it (what transformers 5 writes for a
    bare SiglipVisionModel); the pooling head (`head.*`) and a full checkpoint's text tower, logit_scale and logit_bias are ignored.  ValueError naming the
    keys: any other unexpected tensor, a missing one, a shape that does not fit cfg."""
    vm = "vision_model."

    def ignored(name):
        return name.startswith((vm + "head.", "head.", "text_model.")) or name in ("logit_scale", "logit_bias", vm + "embeddings.position_ids", "embeddings.position_ids")

    return _tower_from_tensors(synth.siglip_vision_tensor_shapes(cfg), tensors, where, lambda name: name if name.startswith(vm) else vm + name, ignored,
                               "SiglipVisionModel", "SigLIP image-encoder")


def load_siglip_vision(path: str, preprocessor: Optional[str] = None):
    """A SigLIP image-encoder directory — config.json (a SiglipVisionConfig or a full SiglipConfig) next to *.safetensors, with an optional
    preprocessor_config.json (in the directory, or in `preprocessor`: FLUX.1-Redux-dev keeps it in feature_extractor/) — as (cfg, {name: tensor}): cfg holds
    SIGLIP_VISION_KEYS plus image_mean / image_std, what Pipeline.load_redux and SiglipVisionModel take.  No device is touched.  ValueError as
    siglip_vision_config's, siglip_image_processor's and siglip_vision_from_tensors'."""
    if not os.path.isdir(path):
        raise FileNotFoundError(f"{path}: not a directory (a SigLIP image encoder is a directory: config.json + *.safetensors)")
    with open(os.path.join(path, "config.json")) as f:
        cfg = siglip_vision_config(json.load(f))
    pre = None
    for d in (path, preprocessor):
        if d is not None and pre is None and os.path.isfile(os.path.join(d, "preprocessor_config.json")):
            with open(os.path.join(d, "preprocessor_config.json")) as f:
                pre = json.load(f)
    mean, std = siglip_image_processor(pre, cfg["image_size"])
    return dict(cfg, image_mean=mean, image_std=std), siglip_vision_from_tensors(cfg, _safetensors_in(path), os.path.basename(os.path.normpath(path)))


def redux_from_tensors(tensors, where: str = "Redux embedder", redux_dim: Optional[int] = None, txt_dim: Optional[int] = None):
    """(redux_dim, txt_dim, {name: tensor}) of a Redux embedder's four tensors (redux_up.{weight,bias}, redux_down.{weight,bias}): the dimensions are read off
    redux_up.weight (3 J, D) and checked against the given ones (a config.json's).  ValueError naming the keys: an unexpected tensor, a missing one, a shape that
    does not fit."""
    sd = dict(tensors.items() if isinstance(tensors, dict) else tensors)
    names = tuple(synth.redux_tensor_shapes(64, 64))
    unexpected = sorted(k for k in sd if k not in names)
    if unexpected:
        raise ValueError(f"{where}: {len(unexpected)} unexpected tensors (not ReduxImageEncoder's), e.g. {unexpected[:3]}")
    missing = [k for k in names if k not in sd]
    if missing:
        raise ValueError(f"{where}: {len(missing)} Redux tensors missing, e.g. {missing[:3]}")
    up = tuple(sd["redux_up.weight"].shape)
    if len(up) != 2 or up[0] % 3:
        raise ValueError(f"{where}: redux_up.weight is {up}, expected (3 * txt_in_features, redux_dim)")
    D, J = int(up[1]), int(up[0]) // 3
    for given, got, what in ((redux_dim, D, "redux_dim"), (txt_dim, J, "txt_in_features")):
        if given is not None and int(given) != got:
            raise ValueError(f"{where}: config.json has {what} = {given}, redux_up.weight {up} says {got}")
    for k, shp in synth.redux_tensor_shapes(D, J).items():
        if tuple(sd[k].shape) != tuple(shp):
            raise ValueError(f"{where}: {k} is {tuple(sd[k].shape)}, expected {tuple(shp)}")
    return D, J, sd


def load_redux(path: str):
    """A Redux embedder — diffusers' image_embedder/ directory (config.json with redux_dim and txt_in_features next to *.safetensors) or BFL's single
    flux1-redux-dev.safetensors, which holds the same four names — as (redux_dim, txt_dim, {name: tensor}).  No device is touched.  ValueError as
    redux_from_tensors', and for a config.json that lacks redux_dim / txt_in_features."""
    where = os.path.basename(os.path.normpath(path))
    if os.path.isdir(path):
        with open(os.path.join(path, "config.json")) as f:
            config = json.load(f)
        lacking = [k for k in ("redux_dim", "txt_in_features") if not isinstance(config, dict) or config.get(k) is None]
        if lacking:
            raise ValueError(f"{where}: config.json lacks {lacking}")
        return redux_from_tensors(_safetensors_in(path), where, config["redux_dim"], config["txt_in_features"])
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: neither an image_embedder directory nor a .safetensors file")
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    return redux_from_tensors(dict(_safetensors_from_buffer(memoryview(mm))), where)


def load_vae(vae, tensors: Iterator[Tuple[str, torch.Tensor]]) -> int:
    want = synth.vae_tensor_shapes(vae.cfg, encoder=True)  # encoder tensors are loaded when the checkpoint has them
    n = 0
    for name, t in tensors:
        if name in want:
            vae.set_tensor(name, t)
            n += 1
    return n


def load_text_encoder(model, tensors: Iterator[Tuple[str, torch.Tensor]]) -> int:
    """Feed a T5EncoderModel / ClipTextTransformer from (name, tensor) pairs; names the model does not read (decoder-tied
    embeddings, position_ids buffers, CLIP's unused text_projection) are skipped.  A bitsandbytes-quantised T5 (the reference
    builds every T5 Linear through `linear_no_bias(.., &cfg.quantization_config, ..)`, t5/mod.rs:132-173,258-261 — the
    FLUX.1-dev-Q4-bnb.dduf layout of README.md:37-41) is fed through the same group logic as the DiT."""
    want = model.tensor_names()

    def extra(name, t):
        if name == "encoder.embed_tokens.weight" and "shared.weight" in model.missing():
            model.set_tensor("shared.weight", t)  # T5EncoderModel::new falls back to it (t5/mod.rs:615-621)
            return True
        return False

    stats = _feed_linears(model, tensors, want, on_extra=extra)
    m = model.missing()
    if m:
        raise ValueError(f"{len(m)} text-encoder tensors missing, e.g. {m[0]}")
    model.load_stats = stats
    return stats["dense"] + stats["bnb4"] + stats["int8"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# GGUF transformers: llama.cpp's single-file format with the ggml block quantisations, as most quantised FLUX.1
# transformers are distributed (flux1-dev-Q8_0.gguf, -Q4_K_S, ...).  The file layout is the reference's gguf_file.rs (never wired to FLUX
# there); the blocks are expanded on the device (csrc/gguf_dequant.hip).
GGML_F32, GGML_F16, GGML_BF16 = 0, 1, 30
GGML_TYPE_NAMES = {0: "F32", 1: "F16", 2: "Q4_0", 3: "Q4_1", 6: "Q5_0", 7: "Q5_1", 8: "Q8_0", 9: "Q8_1", 10: "Q2_K", 11: "Q3_K", 12: "Q4_K", 13: "Q5_K",
                   14: "Q6_K", 15: "Q8_K", 16: "IQ2_XXS", 17: "IQ2_XS", 18: "IQ3_XXS", 19: "IQ1_S", 20: "IQ4_NL", 21: "IQ3_S", 22: "IQ2_S", 23: "IQ4_XS",
                   24: "I8", 25: "I16", 26: "I32", 27: "I64", 28: "F64", 29: "IQ1_M", 30: "BF16"}
# ggml type -> (elements per block, bytes per block) of every type whose size this reader knows; the library expands the first eight block formats
GGML_BLOCKS = {2: (32, 18), 3: (32, 20), 6: (32, 22), 7: (32, 24), 8: (32, 34), 12: (256, 144), 13: (256, 176), 14: (256, 210),
               0: (1, 4), 1: (1, 2), 30: (1, 2), 9: (32, 36), 10: (256, 84), 11: (256, 110), 15: (256, 292), 24: (1, 1), 25: (1, 2), 26: (1, 4), 27: (1, 8),
               28: (1, 8)}
GGUF_QUANT_TYPES = (2, 3, 6, 7, 8, 12, 13, 14)
_GGUF_SCALARS = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}


def ggml_type_name(t: int) -> str:
    return GGML_TYPE_NAMES.get(int(t), f"type {t}")


class GgufFile:
    """mmap reader of a GGUF v2 / v3 file, little-endian (gguf_file.rs): magic and version, counts, metadata key/values of every value type (arrays
    included), tensor infos, and the data section aligned to `general.alignment` (default 32).  GGUF stores dims innermost-first: a Linear (out, in)
    arrives as [in, out]; `tensors` and iteration give the shape outer-first.  Iterating yields (name, ggml_type, shape, memoryview) without copying.
    ValueError: bad magic, version 1 (or any other than 2 / 3), a tensor running past the end of the file, a duplicate tensor name."""

    def __init__(self, path: str):
        self.path = path
        self._f = open(path, "rb")
        self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
        self._view = memoryview(self._mm)
        self._pos = 0
        size = len(self._mm)
        if size < 24 or bytes(self._view[:4]) != b"GGUF":
            raise ValueError(f"{path}: not a GGUF file (bad magic)")
        self._pos = 4
        self.version = self._scalar("<I")
        if self.version not in (2, 3):
            raise ValueError(f"{path}: GGUF version {self.version} is not supported (2 and 3 are; a value like {self.version} can also mean a big-endian file)")
        n_tensors, n_kv = self._scalar("<Q"), self._scalar("<Q")
        self.metadata = {}
        for _ in range(n_kv):
            key = self._string()
            self.metadata[key] = self._value(self._scalar("<I"))
        infos = []
        seen = set()
        for _ in range(n_tensors):
            name = self._string()
            if name in seen:
                raise ValueError(f"{path}: duplicate tensor name {name}")
            seen.add(name)
            n_dims = self._scalar("<I")
            dims = [self._scalar("<Q") for _ in range(n_dims)]
            ggml_type, offset = self._scalar("<I"), self._scalar("<Q")
            infos.append((name, ggml_type, tuple(reversed(dims)), offset))
        self.alignment = int(self.metadata.get("general.alignment", 32))
        if self.alignment <= 0:
            raise ValueError(f"{path}: general.alignment = {self.alignment}")
        self.data_offset = (self._pos + self.alignment - 1) // self.alignment * self.alignment
        self.tensors = {}
        for name, ggml_type, shape, offset in infos:
            numel = 1
            for d in shape:
                numel *= d
            nbytes = None
            if ggml_type in GGML_BLOCKS:
                be, bb = GGML_BLOCKS[ggml_type]
                if shape and shape[-1] % be:
                    raise ValueError(f"{path}: {name}: innermost dimension {shape[-1]} is not a multiple of {ggml_type_name(ggml_type)}'s {be}-element block")
                nbytes = numel // be * bb
            start = self.data_offset + offset
            if start > size or (nbytes is not None and start + nbytes > size):
                raise ValueError(f"{path}: tensor {name} runs past the end of the file ({start} + {nbytes} > {size})")
            self.tensors[name] = (ggml_type, shape, start, nbytes)

    def _need(self, n):
        if self._pos + n > len(self._mm):
            raise ValueError(f"{self.path}: truncated GGUF header")

    def _scalar(self, fmt):
        n = struct.calcsize(fmt)
        self._need(n)
        v = struct.unpack_from(fmt, self._mm, self._pos)[0]
        self._pos += n
        return v

    def _string(self):
        n = self._scalar("<Q")
        self._need(n)
        s = bytes(self._view[self._pos:self._pos + n]).decode("utf-8", errors="replace")
        self._pos += n
        return s

    def _value(self, vt):
        if vt in _GGUF_SCALARS:
            return self._scalar(_GGUF_SCALARS[vt])
        if vt == 8:
            return self._string()
        if vt == 9:
            et, n = self._scalar("<I"), self._scalar("<Q")
            return [self._value(et) for _ in range(n)]
        raise ValueError(f"{self.path}: unknown GGUF metadata value type {vt}")

    def names(self) -> List[str]:
        return list(self.tensors)

    def data(self, name: str) -> memoryview:
        ggml_type, shape, start, nbytes = self.tensors[name]
        if nbytes is None:
            raise ValueError(f"{self.path}: {name}: the size of ggml type {ggml_type_name(ggml_type)} is not known to this reader")
        return self._view[start:start + nbytes]

    def __iter__(self):
        for name, (ggml_type, shape, start, nbytes) in self.tensors.items():
            yield name, ggml_type, shape, (self._view[start:start + nbytes] if nbytes is not None else None)


_BFL_TOP = {"time_in.in_layer": "time_text_embed.timestep_embedder.linear_1", "time_in.out_layer": "time_text_embed.timestep_embedder.linear_2",
            "vector_in.in_layer": "time_text_embed.text_embedder.linear_1", "vector_in.out_layer": "time_text_embed.text_embedder.linear_2",
            "guidance_in.in_layer": "time_text_embed.guidance_embedder.linear_1", "guidance_in.out_layer": "time_text_embed.guidance_embedder.linear_2",
            "txt_in": "context_embedder", "img_in": "x_embedder", "final_layer.linear": "proj_out"}
_BFL_NORMS = {"img_attn.norm.query_norm.scale": "attn.norm_q.weight", "img_attn.norm.key_norm.scale": "attn.norm_k.weight",
              "txt_attn.norm.query_norm.scale": "attn.norm_added_q.weight", "txt_attn.norm.key_norm.scale": "attn.norm_added_k.weight"}
_BFL_SINGLE_NORMS = {"norm.query_norm.scale": "attn.norm_q.weight", "norm.key_norm.scale": "attn.norm_k.weight"}


def bfl_to_diffusers(name: str, rows: int, hidden: int):
    """One tensor of a BFL-named FLUX checkpoint (`rows` = its outer dimension) as the diffusers tensors it holds: [(diffusers name, [(r0, r1), ...])] —
    the row ranges of the source, concatenated in this order, are the diffusers tensor.  Follows diffusers' convert_flux_transformer_checkpoint_to_diffusers:
    qkv into thirds, a single block's linear1 into D, D, D, M rows, and final_layer.adaLN_modulation.1 with its two halves exchanged (BFL stores
    shift | scale, diffusers scale | shift).  None for a name that is not part of the transformer.  The block-level module map is lora.py's."""
    from . import lora
    whole = [(0, rows)]
    for suffix in (".weight", ".bias", ".scale"):
        if name.endswith(suffix):
            mod, kind = name[:-len(suffix)], suffix[1:]
            break
    else:
        return None
    if kind == "scale":
        parts = name.split(".", 2)
        if len(parts) == 3 and parts[0] == "double_blocks" and parts[2] in _BFL_NORMS:
            return [(f"transformer_blocks.{parts[1]}.{_BFL_NORMS[parts[2]]}", whole)]
        if len(parts) == 3 and parts[0] == "single_blocks" and parts[2] in _BFL_SINGLE_NORMS:
            return [(f"single_transformer_blocks.{parts[1]}.{_BFL_SINGLE_NORMS[parts[2]]}", whole)]
        return None
    if mod in _BFL_TOP:
        return [(f"{_BFL_TOP[mod]}.{kind}", whole)]
    if mod == "final_layer.adaLN_modulation.1":
        if rows % 2:
            return None
        return [(f"norm_out.linear.{kind}", [(rows // 2, rows), (0, rows // 2)])]
    parts = mod.split(".", 2)
    if len(parts) != 3 or not parts[1].isdigit():
        return None
    if parts[0] == "double_blocks" and parts[2] in lora.BFL_DOUBLE:
        targets, prefix = lora.BFL_DOUBLE[parts[2]], f"transformer_blocks.{parts[1]}."
        bounds = [rows * i // len(targets) for i in range(len(targets) + 1)]
        if rows % len(targets):
            return None
    elif parts[0] == "single_blocks" and parts[2] in lora.BFL_SINGLE:
        targets, prefix = lora.BFL_SINGLE[parts[2]], f"single_transformer_blocks.{parts[1]}."
        bounds = [0, hidden, 2 * hidden, 3 * hidden, rows] if len(targets) == 4 else [0, rows]
        if len(targets) == 4 and rows <= 3 * hidden:
            return None
    else:
        return None
    return [(f"{prefix}{t}.{kind}", [(bounds[i], bounds[i + 1])]) for i, t in enumerate(targets)]


def flux_entries_from_shapes(shapes: Dict[str, tuple], where: str):
    """The tensors of a single-file FLUX transformer ({source name: shape, outer dimension first}) under their diffusers names: [(diffusers name, shape, source
    tensor, row ranges)], and the source names that are no part of the transformer.  BFL naming or diffusers naming as is, told apart by `double_blocks.0.`
    against `transformer_blocks.0.`; an optional `model.diffusion_model.` prefix is stripped.  ValueError for a file with neither.  Shared by the GGUF and the
    single-file safetensors readers."""
    strip = "model.diffusion_model."
    names = {(n[len(strip):] if n.startswith(strip) else n): n for n in shapes}
    bfl = any(n.startswith("double_blocks.0.") for n in names)
    if not bfl and not any(n.startswith("transformer_blocks.0.") for n in names):
        raise ValueError(f"{where}: neither BFL (double_blocks.0.*) nor diffusers (transformer_blocks.0.*) FLUX transformer tensors")
    hidden = None
    for key in ("img_in.weight", "x_embedder.weight"):
        if key in names:
            hidden = shapes[names[key]][0]
    entries, skipped = [], []
    for short, full in names.items():
        shape = tuple(shapes[full])
        if not shape:
            skipped.append(full)
            continue
        if not bfl:
            entries.append((short, shape, full, [(0, shape[0])]))
            continue
        mapped = bfl_to_diffusers(short, shape[0], hidden or 0)
        if mapped is None:
            skipped.append(full)
            continue
        for dname, ranges in mapped:
            entries.append((dname, (sum(b - a for a, b in ranges),) + tuple(shape[1:]), full, ranges))
    return entries, skipped


def gguf_flux_entries(gguf: "GgufFile"):
    """flux_entries_from_shapes of a FLUX transformer GGUF, with each tensor's ggml type: [(diffusers name, ggml_type, shape, source tensor, row ranges)], and
    the source names that are no part of the transformer."""
    entries, skipped = flux_entries_from_shapes({n: gguf.tensors[n][1] for n in gguf.names()}, gguf.path)
    return [(dname, gguf.tensors[src][0], shape, src, ranges) for dname, shape, src, ranges in entries], skipped


def flux_config_from_shapes(shapes: Dict[str, tuple], where: str, base_config: Optional[dict] = None) -> dict:
    """The model configuration of a FLUX transformer from the shapes of its tensors under their diffusers names (a BFL file has no config.json): in_channels,
    out_channels, pooled_projection_dim, joint_attention_dim, num_attention_heads (D / 128), num_layers, num_single_layers, guidance_embeds; the RoPE constants
    are FLUX.1's.  base_config: a transformer/config.json the result must agree with, field by field, else a ValueError names the field."""
    from . import flux as F

    def need(name):
        if name not in shapes:
            raise ValueError(f"{where}: no {name}: cannot infer the FLUX configuration")
        return shapes[name]

    D, cin = need("x_embedder.weight")
    if D % 128:
        raise ValueError(f"{where}: hidden size {D} is not a multiple of the 128-wide attention head")

    def count(prefix):
        idx = {int(n[len(prefix):].split(".", 1)[0]) for n in shapes if n.startswith(prefix)}
        return max(idx) + 1 if idx else 0

    cfg = dict(F.FLUX_DEV, in_channels=int(cin), out_channels=int(need("proj_out.weight")[0]),
               pooled_projection_dim=int(need("time_text_embed.text_embedder.linear_1.weight")[1]), joint_attention_dim=int(need("context_embedder.weight")[1]),
               num_attention_heads=int(D // 128), num_layers=count("transformer_blocks."), num_single_layers=count("single_transformer_blocks."),
               guidance_embeds="time_text_embed.guidance_embedder.linear_1.weight" in shapes)
    if base_config is not None:
        for k in ("in_channels", "out_channels", "pooled_projection_dim", "joint_attention_dim", "num_attention_heads", "num_layers", "num_single_layers",
                  "guidance_embeds"):
            if k not in base_config:
                continue
            have = base_config[k]
            if k == "out_channels" and have is None:
                have = base_config.get("in_channels", cfg["in_channels"])
            if type(cfg[k])(have) != cfg[k]:
                raise ValueError(f"{where}: {k} = {cfg[k]} by the file's shapes, transformer/config.json says {base_config[k]}")
    return cfg


def flux_config_from_gguf(gguf: "GgufFile", base_config: Optional[dict] = None) -> dict:
    """flux_config_from_shapes of a FLUX transformer GGUF."""
    entries, _ = gguf_flux_entries(gguf)
    return flux_config_from_shapes({n: s for n, _, s, _, _ in entries}, gguf.path, base_config)


def _gguf_rows(view, row_bytes: int, ranges) -> np.ndarray:
    """Rows [r0, r1) ... of a row-major byte image, concatenated; one range: a view, no copy."""
    a = np.frombuffer(view, np.uint8)
    pieces = [a[r0 * row_bytes:r1 * row_bytes] for r0, r1 in ranges]
    return pieces[0] if len(pieces) == 1 else np.concatenate(pieces)


def load_flux_gguf(flux, gguf) -> dict:
    """Feed a FluxModel from a GGUF file (a path or a GgufFile).  Plain tensors (F32 / F16 / BF16) go through set_tensor, block-quantised Linears through
    set_linear_gguf; the row splits of the BFL naming and the exchange of the final layer's halves are done on the packed bytes (a row is a whole number
    of blocks, so no block is cut).  Returns load_flux's stats plus "gguf" (block-quantised Linears) and "types" ({ggml type name: tensors})."""
    if not isinstance(gguf, GgufFile):
        gguf = GgufFile(gguf)
    want = synth.flux_tensor_shapes(flux.cfg)
    entries, skipped = gguf_flux_entries(gguf)
    stats = {"dense": 0, "bnb4": 0, "int8": 0, "gguf": 0, "types": {}, "skipped": list(skipped)}
    plain = {GGML_F32: (np.float32, 4), GGML_F16: (np.float16, 2), GGML_BF16: (np.uint16, 2)}
    for dname, ggml_type, shape, src, ranges in entries:
        if dname not in want:
            stats["skipped"].append(src)
            continue
        if tuple(shape) != tuple(want[dname]):
            raise ValueError(f"{gguf.path}: {src} -> {dname} is {tuple(shape)}, the configuration says {tuple(want[dname])}")
        tname = ggml_type_name(ggml_type)
        inner = 1
        for d in shape[1:]:
            inner *= d
        if ggml_type in plain:
            npdt, size = plain[ggml_type]
            a = _gguf_rows(gguf.data(src), inner * size, ranges).view(npdt).reshape(shape)
            with warnings.catch_warnings():  # (read-only mmap views are intended: the tensor is only copied to the device)
                warnings.simplefilter("ignore", UserWarning)
                t = torch.from_numpy(a)
            flux.set_tensor(dname, t.view(torch.bfloat16) if ggml_type == GGML_BF16 else t)
            stats["dense"] += 1
        else:
            if ggml_type not in GGUF_QUANT_TYPES or len(shape) != 2 or not dname.endswith(".weight"):
                if ggml_type in GGUF_QUANT_TYPES:
                    raise ValueError(f"{gguf.path}: {src}: only 2-D Linear weights can be block-quantised, this is {tuple(shape)}")
                from . import _lib as L
                L.check(flux.lib.fmi_gguf_block_info(int(ggml_type), None, None), flux.lib)  # refused by name (FMI_ERR_UNSUPPORTED)
                raise ValueError(f"{gguf.path}: {src}: unsupported ggml type {tname}")
            be, bb = GGML_BLOCKS[ggml_type]
            flux.set_linear_gguf(dname[:-len(".weight")], ggml_type, _gguf_rows(gguf.data(src), shape[1] // be * bb, ranges), shape[0], shape[1])
            stats["gguf"] += 1
        stats["types"][tname] = stats["types"].get(tname, 0) + 1
    flux.assert_complete()
    return stats


# ---------------------------------------------------------------------------------------------------------------------------------------
# Single-file FLUX checkpoints: one .safetensors file in BFL's tensor naming (flux1-dev.safetensors, community fine-tunes) or diffusers',
# with or without `model.diffusion_model.`, in F32 / F16 / BF16 or as 8-bit floats (flux1-dev-fp8.safetensors, *_fp8_e4m3fn, *_fp8_e5m2: the safetensors
# dtypes F8_E4M3 / F8_E5M2).  An fp8 Linear stays resident as codes and is expanded on the device (csrc/f8_dequant.hip).
_ST_F8 = {torch.float8_e4m3fn: "e4m3", torch.float8_e5m2: "e5m2"}
# what an all-in-one file carries next to the transformer: the VAE and the text encoders keep coming from the base directory
SINGLE_FILE_OTHER_COMPONENTS = ("vae.", "first_stage_model.", "text_encoders.", "cond_stage_model.")


class SingleFile:
    """mmap view of one .safetensors file: `tensors` {name: zero-copy torch tensor} (float8 dtypes included), `path`."""

    def __init__(self, path: str):
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: not a file (a single-file checkpoint is one .safetensors file)")
        self.path = path
        with open(path, "rb") as f:
            self._mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        self.tensors = dict(_safetensors_from_buffer(memoryview(self._mm)))


def single_file_flux_entries(sf: "SingleFile"):
    """The transformer's tensors of a single-file checkpoint under their diffusers names: ([(diffusers name, shape, source tensor, row ranges)], {source weight
    name: scale_weight tensor name}, skipped source names).  Skipped: the other components of an all-in-one file (SINGLE_FILE_OTHER_COMPONENTS), the
    `scaled_fp8` marker and every `<linear>.scale_input` of a "scaled fp8" file (activation scales belong to another runtime's fp8 matmul), and whatever else
    is no transformer tensor.  `<linear>.scale_weight` is the scale of `<linear>.weight`."""
    shapes, scales, skipped = {}, {}, []
    for name, t in sf.tensors.items():
        if name.startswith(SINGLE_FILE_OTHER_COMPONENTS):
            skipped.append(name)
        elif name.endswith(".scale_input") or name == "scaled_fp8" or name.endswith(".scaled_fp8"):
            skipped.append(name)
        elif name.endswith(".scale_weight"):
            scales[name[:-len(".scale_weight")] + ".weight"] = name
        else:
            shapes[name] = tuple(t.shape)
    entries, more = flux_entries_from_shapes(shapes, sf.path)
    for wname, sname in scales.items():
        if wname not in shapes:
            more.append(sname)
    return entries, scales, skipped + more


def flux_config_from_single_file(path, base_config: Optional[dict] = None) -> dict:
    """flux_config_from_shapes of a single-file checkpoint (a path or a SingleFile)."""
    sf = path if isinstance(path, SingleFile) else SingleFile(path)
    entries, _, _ = single_file_flux_entries(sf)
    return flux_config_from_shapes({n: s for n, s, _, _ in entries}, sf.path, base_config)


def _single_file_scale(sf: "SingleFile", sname: str) -> float:
    t = sf.tensors[sname]
    if t.dtype != torch.float32 or tuple(t.shape) not in ((), (1,)):
        raise ValueError(f"{sf.path}: {sname} is {str(t.dtype).replace('torch.', '')} {tuple(t.shape)}: a scale_weight must be one F32 element, of shape () or (1,) "
                         f"(per-row and block scales are not supported)")
    v = float(t.reshape(-1)[0])
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"{sf.path}: {sname} = {v}: a scale_weight must be finite and > 0")
    return v


def load_flux_single_file(flux, path, expand: bool = False) -> dict:
    """Feed a FluxModel from a single-file checkpoint (a path or a SingleFile).  F32 / F16 / BF16 tensors go through set_tensor; fp8 2-D `.weight` tensors through
    set_linear_f8 with their `scale_weight` (1 without one) — the row splits of the BFL naming and the exchange of the final layer's halves are done on the rows
    of the stored bytes —; fp8 tensors of any other rank (biases, norm scales) are widened on the host, exactly, and go through set_tensor.  expand=True: every
    fp8 Linear is dequantised at load by the same kernel into its plain bf16 slot, and the model is an ordinary bf16 model (LoRA, get_tensor, the 8-bit modes and
    state_export work).  Returns load_flux's stats plus "f8" (Linears fed as codes or expanded from them) and "formats" ({"e4m3" | "e5m2": Linears})."""
    from . import flux as F
    sf = path if isinstance(path, SingleFile) else SingleFile(path)
    want = synth.flux_tensor_shapes(flux.cfg)
    entries, scales, skipped = single_file_flux_entries(sf)
    stats = {"dense": 0, "bnb4": 0, "int8": 0, "f8": 0, "formats": {}, "skipped": list(skipped)}
    for dname, shape, src, ranges in entries:
        if dname not in want:
            stats["skipped"].append(src)
            continue
        if tuple(shape) != tuple(want[dname]):
            raise ValueError(f"{sf.path}: {src} -> {dname} is {tuple(shape)}, the configuration says {tuple(want[dname])}")
        t = sf.tensors[src]
        fmt = _ST_F8.get(t.dtype)
        if src in scales and not (fmt and len(shape) == 2 and dname.endswith(".weight")):
            raise ValueError(f"{sf.path}: {scales[src]} belongs to {src}, which is no 2-D fp8 weight ({str(t.dtype).replace('torch.', '')} {tuple(t.shape)})")
        if fmt and len(shape) == 2 and dname.endswith(".weight"):
            scale = _single_file_scale(sf, scales[src]) if src in scales else 1.0
            codes = _gguf_rows(t.view(torch.uint8).numpy().reshape(-1), shape[1], ranges)
            if expand:
                dev = torch.from_numpy(np.ascontiguousarray(codes)).to(flux.device)
                flux.set_tensor(dname, F.f8_dequantize(dev, fmt, scale).reshape(shape))
            else:
                flux.set_linear_f8(dname[:-len(".weight")], fmt, codes, scale, shape[0], shape[1])
            stats["f8"] += 1
            stats["formats"][fmt] = stats["formats"].get(fmt, 0) + 1
            continue
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16) and not fmt:
            raise ValueError(f"{sf.path}: {src}: dtype {str(t.dtype).replace('torch.', '')} is not a transformer tensor's (F32, F16, BF16, F8_E4M3, F8_E5M2)")
        if fmt:
            t = t.to(torch.float32)  # (exact: every code is an f32 value)
        if len(ranges) != 1 or ranges[0] != (0, t.shape[0]):
            t = torch.cat([t[r0:r1] for r0, r1 in ranges])
        flux.set_tensor(dname, t)
        stats["dense"] += 1
    flux.assert_complete()
    return stats
