"""Adapter files for the FLUX DiT -> {linear prefix: AdapterTerm} (read_adapter: LoRA, LoHa, LoKr, full differences, DoRA) or, for files of plain
pairs, {linear prefix: (A, B, scale)} (read_lora), in this library's (diffusers) Linear names, ready for FluxModel.lora_add_term / lora_add
(include/flux_mi355x.h: fmi_flux_lora_add_term).  Two key layouts are read:

  diffusers / PEFT   [transformer.]<linear>.lora_A.weight (r, in), <linear>.lora_B.weight (out, r), optional <linear>.alpha
  kohya / BFL        lora_unet_{double,single}_blocks_<i>_<part>.lora_down.weight / .lora_up.weight / .alpha, <part> in the
                     original FLUX module names; fused projections are split by rows of lora_up (the same lora_down for each):
                     img_attn_qkv / txt_attn_qkv into thirds, single-block linear1 into D, D, D, M rows (D = hidden_size when the caller
                     gives it, else the FLUX ratio M = 4 D is assumed)

Next to the plain pairs, a module may instead hold (the same suffixes in both layouts, after the kohya module name or the diffusers Linear name):
  LoHa    .hada_w1_a (out, r), .hada_w1_b (r, in), .hada_w2_a (out, r), .hada_w2_b (r, in)          Delta = scale (w1_a w1_b) * (w2_a w2_b), element-wise
  LoKr    .lokr_w1 (a, b) or .lokr_w1_a (a, r1) + .lokr_w1_b (r1, b); .lokr_w2 (c, d) or .lokr_w2_a + .lokr_w2_b     Delta = scale kron(w1, w2)
  diff    .diff (out, in): a full difference, read as the LoKr term w1 = [[1]], w2 = diff, scale 1
  DoRA    a plain pair plus .dora_scale (out, 1) (kohya / LyCORIS) or .lora_magnitude_vector[.weight] (out,) (PEFT)
scale = alpha / r with r the rank of the pair / of hada_w1_b / of the decomposed lokr_w2, else of the decomposed lokr_w1; a LoKr with both factors
full has scale 1 and its alpha is ignored.  Fused kohya modules split by rows: row slices of lora_up, hada_w1_a / hada_w2_a, dora_scale and diff;
a LoKr keeps its shared factors and gets the part's first row as row_offset.  These rules and the formulas behind them are written down from memory of
PEFT, LyCORIS and ComfyUI's loader; no file written by them was at hand.

Refused by name: the Tucker forms .hada_t1 / .hada_t2 / .lokr_t2 (convolutions), a .dora_scale of shape (1, in) (decomposition along the input axis) and
.diff_b (a bias difference: biases are never touched).  With skip_unsupported=True a .diff_b is dropped alone; a Tucker key or an input-axis dora_scale
drops its whole module (what is left of it would merge as something else).

scale = alpha / r, or 1 without an alpha.  Keys this library does not merge — text-encoder adapters, and the kohya final-layer and embedder
modules (the diffusers final modulation stores its halves in the other order; that is not guessed at) — raise a ValueError that lists
them, unless skip_unsupported=True drops them.
"""
import mmap
import os
import re
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

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


@dataclass(frozen=True)
class AdapterTerm:
    """One adapter term of one Linear.  kind and tensors (the factor slots of fmi_adapter_term, None for an absent one):
      "lora"  (A (r, in), B (out, r))
      "loha"  (w1_a (out, r), w1_b (r, in), w2_a (out, r), w2_b (r, in))
      "lokr"  (w1 (a, b) | w1_a (a, r1), None | w1_b (r1, b), w2 (c, d) | w2_a (c, r2), None | w2_b (r2, d)), row_offset into the a * c rows
      "dora"  (A, B, m (out,))"""
    kind: str
    tensors: tuple
    scale: float = 1.0
    row_offset: int = 0


# suffix -> slot of the module's group, the same in both layouts; the plain pair has its own suffixes per layout (_KOHYA_SUFFIXES / _PEFT_SUFFIXES)
_LYCORIS_SUFFIXES = {".hada_w1_a": "hada_w1_a", ".hada_w1_b": "hada_w1_b", ".hada_w2_a": "hada_w2_a", ".hada_w2_b": "hada_w2_b",
                     ".lokr_w1_a": "lokr_w1_a", ".lokr_w1_b": "lokr_w1_b", ".lokr_w2_a": "lokr_w2_a", ".lokr_w2_b": "lokr_w2_b",
                     ".lokr_w1": "lokr_w1", ".lokr_w2": "lokr_w2", ".diff": "diff", ".dora_scale": "mag",
                     ".lora_magnitude_vector.weight": "mag", ".lora_magnitude_vector": "mag"}
_REFUSED_MODULE = (".hada_t1", ".hada_t2", ".lokr_t2")  # Tucker forms: the module cannot be merged without them
_REFUSED_KEY = (".diff_b",)                              # a bias difference: dropped alone
_PAIR_SLOTS = {".lora_down.weight": "down", ".lora_up.weight": "up", ".lora_A.weight": "down", ".lora_B.weight": "up", ".alpha": "alpha"}


def _rank2(base, name, t):
    if len(t.shape) != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"adapter module {base}: {name} has shape {tuple(t.shape)}, not a matrix")
    return int(t.shape[0]), int(t.shape[1])


def _group_term(base: str, g: dict):
    """(kind, tensors, scale, rows of the module, row-sliced slots) of one module's keys; ValueError for an incomplete or mixed group."""
    have = sorted(k for k in g if k != "alpha")
    alpha = g.get("alpha")
    hada = [k for k in have if k.startswith("hada_")]
    lokr = [k for k in have if k.startswith("lokr_")]
    families = [f for f in (hada, lokr, ["diff"] if "diff" in g else [], [k for k in have if k in ("down", "up", "mag")]) if f]
    if len(families) != 1:
        raise ValueError(f"adapter module {base}: keys of more than one parametrisation (or none), have {sorted(g)}")
    if hada:
        names = ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")
        if any(n not in g for n in names):
            raise ValueError(f"LoHa module {base}: incomplete group, have {sorted(g)}")
        t = tuple(g[n] for n in names)
        (o1, r1), (r1b, i1), (o2, r2), (r2b, i2) = (_rank2(base, n, x) for n, x in zip(names, t))
        if r1 != r1b or r2 != r2b or r1 != r2 or o1 != o2 or i1 != i2:
            raise ValueError(f"LoHa module {base}: factor shapes {[tuple(x.shape) for x in t]} are not (out, r), (r, in), (out, r), (r, in)")
        return "loha", t, _scale(alpha, r1), o1, (0, 2)
    if lokr:
        halves, rank = [], None
        for h in ("lokr_w1", "lokr_w2"):
            full, fa, fb = g.get(h), g.get(h + "_a"), g.get(h + "_b")
            if (full is None) == (fa is None and fb is None) or (fa is None) != (fb is None):
                raise ValueError(f"LoKr module {base}: needs {h} or {h}_a with {h}_b, have {sorted(g)}")
            if full is not None:
                _rank2(base, h, full)
                halves.append((full, None))
            else:
                (_, ra), (rb, _) = _rank2(base, h + "_a", fa), _rank2(base, h + "_b", fb)
                if ra != rb:
                    raise ValueError(f"LoKr module {base}: {h}_a {tuple(fa.shape)} and {h}_b {tuple(fb.shape)} do not multiply")
                halves.append((fa, fb))
                if h == "lokr_w2" or rank is None:
                    rank = ra  # the rank of the decomposed w2, else of the decomposed w1
        t = halves[0] + halves[1]
        return "lokr", t, (1.0 if rank is None else _scale(alpha, rank)), int(t[0].shape[0]) * int(t[2].shape[0]), ()
    if "diff" in g:
        return "diff", (g["diff"],), 1.0, _rank2(base, "diff", g["diff"])[0], (0,)
    if "down" not in g or "up" not in g:
        raise ValueError(f"LoRA module {base}: incomplete pair, have {sorted(g)}")
    down, up = g["down"], g["up"]
    if len(down.shape) != 2 or len(up.shape) != 2 or down.shape[0] != up.shape[1] or down.shape[0] < 1:
        raise ValueError(f"LoRA module {base}: down {tuple(down.shape)} and up {tuple(up.shape)} are not (r, in) and (out, r)")
    scale = _scale(alpha, int(down.shape[0]))
    if "mag" not in g:
        return "lora", (down, up), scale, int(up.shape[0]), (1,)
    mag = g["mag"]
    if tuple(mag.shape) not in ((int(up.shape[0]),), (int(up.shape[0]), 1)):
        raise ValueError(f"DoRA module {base}: the magnitude has shape {tuple(mag.shape)}, lora_up has {int(up.shape[0])} rows")
    return "dora", (down, up, mag.reshape(-1)), scale, int(up.shape[0]), (1, 2)


def read_adapter(path_or_dict, skip_unsupported: bool = False, hidden_size: int = None) -> Dict[str, AdapterTerm]:
    """{prefix: AdapterTerm} from a .safetensors path or a {key: tensor} dict (torch tensors or numpy arrays; the factors keep their type and dtype,
    row slices of a fused module are views): plain pairs, LoHa, LoKr, full differences and DoRA (module docstring).  hidden_size: the model's D, for the
    row split of a kohya single-block linear1 (D, D, D, the rest); without it the rows are split 1 : 1 : 1 : 4."""
    import numpy as np
    tensors = read_safetensors(os.fspath(path_or_dict)) if isinstance(path_or_dict, (str, os.PathLike)) else dict(path_or_dict)
    groups: Dict[str, dict] = {}  # module -> {slot: tensor}, module = diffusers prefix or kohya base
    kohya: Dict[str, bool] = {}
    unsupported = []
    dropped_modules = set()
    keys_of: Dict[str, list] = {}
    for key, t in tensors.items():
        if _is_unsupported(key):
            unsupported.append(key)
            continue
        is_kohya = key.startswith("lora_unet_")
        base, suf = _split_key(key, _REFUSED_KEY)
        if base is not None:
            unsupported.append(key)
            continue
        base, suf = _split_key(key, _REFUSED_MODULE)
        refused = base is not None
        if base is None:
            base, suf = _split_key(key, tuple(_LYCORIS_SUFFIXES))
        if base is None:
            base, suf = _split_key(key, _KOHYA_SUFFIXES if is_kohya else _PEFT_SUFFIXES)
        if base is None:
            unsupported.append(key)
            continue
        if is_kohya:
            m = _KOHYA_BLOCK.match(base)
            if m is None or m.group(3) not in (_KOHYA_DOUBLE if m.group(1) == "double" else _KOHYA_SINGLE):
                unsupported.append(key)
                continue
            kohya[base] = True
        elif base.startswith("transformer."):
            base = base[len("transformer."):]
        keys_of.setdefault(base, []).append(key)
        slot = _PAIR_SLOTS.get(suf) or _LYCORIS_SUFFIXES.get(suf)
        if slot == "mag" and len(t.shape) == 2 and t.shape[0] == 1 and t.shape[1] > 1:
            refused = True  # (1, in): DoRA decomposed along the input axis
        if refused:
            unsupported.append(key)
            dropped_modules.add(base)
            continue
        groups.setdefault(base, {})[slot] = t
    if unsupported and not skip_unsupported:
        raise ValueError(f"{len(unsupported)} LoRA keys are not supported (text-encoder, final-layer / embedder or unknown modules, Tucker forms hada_t1 / "
                         f"hada_t2 / lokr_t2, an input-axis dora_scale of shape (1, in), bias differences diff_b; skip_unsupported=True drops them, "
                         f"a Tucker or input-axis DoRA key together with its module): {sorted(unsupported)}")
    out: Dict[str, AdapterTerm] = {}
    for base, g in groups.items():
        if base in dropped_modules:
            continue
        kind, t, scale, n, sliced = _group_term(base, g)
        if base not in kohya:
            targets, rows = [base], [n]
        else:
            m = _KOHYA_BLOCK.match(base)
            double = m.group(1) == "double"
            block = ("transformer_blocks." if double else "single_transformer_blocks.") + m.group(2) + "."
            parts = (_KOHYA_DOUBLE if double else _KOHYA_SINGLE)[m.group(3)]
            targets = [block + p for p in parts]
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
            part = tuple(x[r0:r0 + nr] if i in sliced else x for i, x in enumerate(t))
            if kind == "diff":  # the LoKr term with w1 = [[1]]
                out[tgt] = AdapterTerm("lokr", (np.ones((1, 1), np.float32), None, part[0], None), 1.0, 0)
            else:
                out[tgt] = AdapterTerm(kind, part, scale, r0 if kind == "lokr" else 0)
            r0 += nr
    return out


def read_lora(path_or_dict, skip_unsupported: bool = False, hidden_size: int = None) -> Dict[str, Tuple[object, object, float]]:
    """{prefix: (A (r, in), B (out, r), scale)} from a .safetensors path or a {key: tensor} dict (torch tensors or numpy arrays; the factors keep
    their type and dtype, rows of a fused lora_up are views).  hidden_size: the model's D, for the row split of a kohya single-block linear1
    (D, D, D, the rest); without it the rows are split 1 : 1 : 1 : 4.  A file of plain pairs only: one that holds a LoHa, LoKr, full-difference or
    DoRA module raises a ValueError that names the kind (read_adapter reads those)."""
    terms = read_adapter(path_or_dict, skip_unsupported=skip_unsupported, hidden_size=hidden_size)
    other = sorted({t.kind for t in terms.values()} - {"lora"})
    if other:
        raise ValueError(f"the file holds {', '.join(other)} modules, which are no (A, B, scale) pairs: read it with read_adapter")
    return {k: (t.tensors[0], t.tensors[1], t.scale) for k, t in terms.items()}
