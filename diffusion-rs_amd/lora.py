"""LoRA adapter files for the FLUX DiT -> {linear prefix: (A, B, scale)} in this library's (diffusers) Linear names, ready for
FluxModel.lora_add (include/flux_mi355x.h: fmi_flux_lora_add).  Two key layouts are read:

  diffusers / PEFT   [transformer.]<linear>.lora_A.weight (r, in), <linear>.lora_B.weight (out, r), optional <linear>.alpha
  kohya / BFL        lora_unet_{double,single}_blocks_<i>_<part>.lora_down.weight / .lora_up.weight / .alpha, <part> in the
                     original FLUX module names; fused projections are split by rows of lora_up (the same lora_down for each):
                     img_attn_qkv / txt_attn_qkv into thirds, single-block linear1 into D, D, D, M rows (D = hidden_size when the caller
                     gives it, else the FLUX ratio M = 4 D is assumed)

scale = alpha / r, or 1 without an alpha.  Keys this library does not merge — text-encoder adapters, and the kohya final-layer and embedder
modules (the diffusers final modulation stores its halves in the other order; that is not guessed at) — raise a ValueError that lists
them, unless skip_unsupported=True drops them.
"""
import mmap
import os
import re
from typing import Dict, Tuple

_KOHYA_DOUBLE = {
    "img_attn_qkv": ("attn.to_q", "attn.to_k", "attn.to_v"),
    "txt_attn_qkv": ("attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj"),
    "img_attn_proj": ("attn.to_out.0",),
    "txt_attn_proj": ("attn.to_add_out",),
    "img_mlp_0": ("ff.net.0.proj",),
    "img_mlp_2": ("ff.net.2",),
    "txt_mlp_0": ("ff_context.net.0.proj",),
    "txt_mlp_2": ("ff_context.net.2",),
    "img_mod_lin": ("norm1.linear",),
    "txt_mod_lin": ("norm1_context.linear",),
}
_KOHYA_SINGLE = {
    "linear1": ("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp"),
    "linear2": ("proj_out",),
    "modulation_lin": ("norm.linear",),
}
# the same block-level map keyed by the BFL module path (img_attn.qkv, modulation.lin, ...): what loader.load_flux_gguf reads a BFL-named checkpoint with
BFL_DOUBLE = {k.replace("_attn_", "_attn.").replace("_mlp_", "_mlp.").replace("_mod_", "_mod."): v for k, v in _KOHYA_DOUBLE.items()}
BFL_SINGLE = {k.replace("modulation_", "modulation."): v for k, v in _KOHYA_SINGLE.items()}
_KOHYA_BLOCK = re.compile(r"^lora_unet_(double|single)_blocks_(\d+)_(.+)$")
_KOHYA_SUFFIXES = (".lora_down.weight", ".lora_up.weight", ".alpha")
_PEFT_SUFFIXES = (".lora_A.weight", ".lora_B.weight", ".alpha")


def read_safetensors(path: str) -> Dict[str, "object"]:
    """Every tensor of one .safetensors file (the repository's own reader: loader._safetensors_from_buffer), as torch tensors."""
    from .loader import _safetensors_from_buffer
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    return {k: t.clone() for k, t in _safetensors_from_buffer(memoryview(mm))}


def _split_key(key: str, suffixes):
    for s in suffixes:
        if key.endswith(s):
            return key[:-len(s)], s
    return None, None


def _is_unsupported(key: str) -> bool:
    return key.startswith(("text_encoder", "lora_te")) or (key.startswith("lora_unet_") and not _KOHYA_BLOCK.match(key.split(".", 1)[0]))


def _scale(alpha, r: int) -> float:
    return 1.0 if alpha is None else float(alpha) / r


def read_lora(path_or_dict, skip_unsupported: bool = False, hidden_size: int = None) -> Dict[str, Tuple[object, object, float]]:
    """{prefix: (A (r, in), B (out, r), scale)} from a .safetensors path or a {key: tensor} dict (torch tensors or numpy arrays; the factors keep
    their type and dtype, rows of a fused lora_up are views).  hidden_size: the model's D, for the row split of a kohya single-block linear1
    (D, D, D, the rest); without it the rows are split 1 : 1 : 1 : 4."""
    tensors = read_safetensors(os.fspath(path_or_dict)) if isinstance(path_or_dict, (str, os.PathLike)) else dict(path_or_dict)
    groups: Dict[str, dict] = {}  # module -> {"down", "up", "alpha"}, module = diffusers prefix or kohya base
    kohya: Dict[str, bool] = {}
    unsupported = []
    for key, t in tensors.items():
        if _is_unsupported(key):
            unsupported.append(key)
            continue
        base, suf = _split_key(key, _KOHYA_SUFFIXES) if key.startswith("lora_unet_") else (None, None)
        if base is not None:
            m = _KOHYA_BLOCK.match(base)
            if m.group(3) not in (_KOHYA_DOUBLE if m.group(1) == "double" else _KOHYA_SINGLE):
                unsupported.append(key)
                continue
            kohya[base] = True
            groups.setdefault(base, {})[{".lora_down.weight": "down", ".lora_up.weight": "up", ".alpha": "alpha"}[suf]] = t
            continue
        base, suf = _split_key(key, _PEFT_SUFFIXES)
        if base is None or key.startswith("lora_unet_"):
            unsupported.append(key)
            continue
        if base.startswith("transformer."):
            base = base[len("transformer."):]
        groups.setdefault(base, {})[{".lora_A.weight": "down", ".lora_B.weight": "up", ".alpha": "alpha"}[suf]] = t
    if unsupported and not skip_unsupported:
        raise ValueError(f"{len(unsupported)} LoRA keys are not supported (text-encoder, final-layer / embedder or unknown modules; "
                         f"skip_unsupported=True drops them): {sorted(unsupported)}")
    out: Dict[str, Tuple[object, object, float]] = {}
    for base, g in groups.items():
        if "down" not in g or "up" not in g:
            raise ValueError(f"LoRA module {base}: incomplete pair, have {sorted(g)}")
        down, up = g["down"], g["up"]
        if len(down.shape) != 2 or len(up.shape) != 2 or down.shape[0] != up.shape[1] or down.shape[0] < 1:
            raise ValueError(f"LoRA module {base}: down {tuple(down.shape)} and up {tuple(up.shape)} are not (r, in) and (out, r)")
        scale = _scale(g.get("alpha"), int(down.shape[0]))
        if base not in kohya:
            targets, rows = [base], [int(up.shape[0])]
        else:
            m = _KOHYA_BLOCK.match(base)
            double = m.group(1) == "double"
            block = ("transformer_blocks." if double else "single_transformer_blocks.") + m.group(2) + "."
            parts = (_KOHYA_DOUBLE if double else _KOHYA_SINGLE)[m.group(3)]
            targets = [block + p for p in parts]
            n = int(up.shape[0])
            if len(parts) == 1:
                rows = [n]
            elif len(parts) == 3:  # q | k | v
                if n % 3:
                    raise ValueError(f"LoRA module {base}: {n} rows of lora_up do not split into q, k, v")
                rows = [n // 3] * 3
            elif hidden_size is not None:  # q | k | v | proj_mlp = D, D, D, M
                if n <= 3 * hidden_size:
                    raise ValueError(f"LoRA module {base}: {n} rows of lora_up do not split into D, D, D, M at D = {hidden_size}")
                rows = [hidden_size] * 3 + [n - 3 * hidden_size]
            else:  # the FLUX ratio: D, D, D, 4 D
                if n % 7:
                    raise ValueError(f"LoRA module {base}: {n} rows of lora_up do not split into D, D, D, 4 D")
                rows = [n // 7] * 3 + [4 * (n // 7)]
        r0 = 0
        for tgt, nr in zip(targets, rows):
            if tgt in out:
                raise ValueError(f"LoRA: two modules of the file map to {tgt}")
            out[tgt] = (down, up[r0:r0 + nr], scale)
            r0 += nr
    return out
