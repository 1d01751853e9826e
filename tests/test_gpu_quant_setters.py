"""The four quantised-Linear setters of the FLUX transformer (fmi_flux_set_linear_bnb4 / _int8 / _gguf / _f8) pinned against
tests/golden/quant_setters.json, which tests/golden/gen_quant_setters.py wrote with THIS file's walks on the library of the commit before the setters were
given one shared frame: every refusal's (code, message), and for every ordered pair (A, B) of {dense, nf4, int8, gguf Q8_0, f8 e4m3} what loading a part
as B over a matrix loaded as A does — refused (code, message), or the model of the final contents bit for bit — with size_in_bytes() after the second
load and after one forward.  And one nf4 and one int8 Linear of a 2-layer T5 through fmi_t5_set_linear_*: the values of the stand-alone dequant entries.

The walk of a transition: load the whole model dense, the matrix's parts as A, evaluate once (finalize() has decided how the matrix is multiplied and, in
dense-cache mode 1, its expansion is cached: the state the second load has to undo), load the part(s) again as B with other values, then forward and a
3-step denoise next to a fresh model that was only ever given the final contents.  384 image rows: above both fused row thresholds of densify(), so mode 0
takes the per-call expansion."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import f8_ref as F8
from tests import gguf_ref as G
from tests.util import SMALL_FLUX, dev, flux_inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quant_setters.json")
KINDS = ("dense", "nf4", "int8", "q8_0", "f8")
SETTERS = ("bnb4", "int8", "gguf", "f8")
QKV = ["transformer_blocks.0.attn.to_q", "transformer_blocks.0.attn.to_k", "transformer_blocks.0.attn.to_v"]
LINEAR1 = ["single_transformer_blocks.0.attn.to_q", "single_transformer_blocks.0.attn.to_k", "single_transformer_blocks.0.attn.to_v",
           "single_transformer_blocks.0.proj_mlp"]
# matrix -> (its parts, the parts loaded a second time)
TARGETS = {"qkv": (QKV, QKV[:1]), "linear1": (LINEAR1, LINEAR1)}
CASES = [f"{t} {a}->{b}" for t in TARGETS for a in KINDS for b in KINDS]
PACKED = QKV[0]
T3 = [1.0, 0.75, 0.4, 0.0]


@functools.lru_cache(maxsize=None)
def _sd(version):
    import diffusion_rs_amd as d
    return d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=(0, 7)[version])


@functools.lru_cache(maxsize=None)
def _payload(prefix, kind, version):
    """the arguments of `prefix`'s setter for `kind`, from the weight of state dict `version`; computed once"""
    import torch
    import diffusion_rs_amd as d
    w = np.asarray(_sd(version)[prefix + ".weight"], np.float32)
    if kind == "nf4":
        packed, absmax = d.synth.quantize_nf4_device(dev(w, torch.bfloat16), 64)
        return packed.cpu().numpy(), absmax.cpu().numpy()
    if kind == "int8":
        scb = np.abs(w).max(1).astype(np.float32)
        return np.clip(np.rint(w / scb[:, None] * 127.0), -127, 127).astype(np.int8), scb
    if kind == "q8_0":
        return (G.encode(G.Q8_0, w.ravel()),)
    if kind == "f8":
        return F8.quantize(w, "e4m3", scaled=True)
    return (w,)


def load(m, prefix, kind, version):
    out_f, in_f = _sd(version)[prefix + ".weight"].shape
    p = _payload(prefix, kind, version)
    if kind == "dense":
        m.set_tensor(prefix + ".weight", p[0])
    elif kind == "nf4":
        m.set_linear_bnb4(prefix, p[0], p[1], 64, "nf4", out_f, in_f)
    elif kind == "int8":
        m.set_linear_int8(prefix, p[0], p[1], out_f, in_f)
    elif kind == "q8_0":
        m.set_linear_gguf(prefix, G.Q8_0, p[0], out_f, in_f)
    else:
        m.set_linear_f8(prefix, "e4m3", p[0], p[1], out_f, in_f)


@functools.lru_cache(maxsize=None)
def _args():
    import torch
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, 1, (16, 24), 32)
    return dev(img), dev(ids), dev(txt, torch.bfloat16), dev(txt_ids), dev(np.array([0.75], np.float32)), dev(y), dev(np.array([3.5], np.float32))


def evaluate(m):
    import torch
    img, ids, txt, txt_ids, t, y, g = _args()
    fwd = m.forward(img, ids, txt, txt_ids, t, y, g)
    torch.cuda.synchronize()
    size = m.size_in_bytes()
    den = m.denoise(img, ids, txt, txt_ids, y, g, T3)
    torch.cuda.synchronize()
    return fwd, den, size


def transition(case):
    """{"outcome": "refused", "code", "message"} | {"outcome": "equal" | "differs", "sizes": {mode: [after the second load, after one forward]}}"""
    import diffusion_rs_amd as d
    target, pair = case.split(" ")
    a, b = pair.split("->")
    parts, again = TARGETS[target]
    sizes, equal = {}, True
    for mode in (0, 1):
        m = d.FluxModel(SMALL_FLUX)
        try:
            m.set_quant_dense_cache(mode)
            m.load_state_dict(_sd(0))
            for p in parts:
                load(m, p, a, 0)
            evaluate(m)
            try:
                for p in again:
                    load(m, p, b, 1)
            except d.FmiError as e:
                return {"outcome": "refused", "code": e.code, "message": str(e)}
            after_load = m.size_in_bytes()
            fwd, den, after_forward = evaluate(m)
            sizes[str(mode)] = [after_load, after_forward]
            fresh = d.FluxModel(SMALL_FLUX)
            try:
                fresh.set_quant_dense_cache(mode)
                fresh.load_state_dict(_sd(0))
                for p in parts:
                    load(fresh, p, b if p in again else a, 1 if p in again else 0)
                ffwd, fden, _ = evaluate(fresh)
            finally:
                fresh.close()
            import torch
            equal = equal and torch.equal(fwd, ffwd) and torch.equal(den, fden)
        finally:
            m.close()
    return {"outcome": "equal" if equal else "differs", "sizes": sizes}


def _call(m, setter, prefix=PACKED, shape=(256, 256), data=True, **own):
    """one raw call of a setter with valid arguments but those named; (code, message)"""
    buf = np.full(1 << 20, 0x38, np.uint8)  # larger than any Linear of SMALL_FLUX in any kind: a call that should have been refused reads no further
    sc = np.ones(1 << 16, np.float32)
    bp, sp = (C.c_void_p(buf.ctypes.data) if data else None), C.c_void_p(sc.ctypes.data)
    px = prefix.encode()
    if setter == "bnb4":
        rc = m.lib.fmi_flux_set_linear_bnb4(m.h, px, bp, sp, own.get("blocksize", 64), own.get("quant_type", 2), *shape)
    elif setter == "int8":
        rc = m.lib.fmi_flux_set_linear_int8(m.h, px, bp, sp, *shape)
    elif setter == "gguf":
        rc = m.lib.fmi_flux_set_linear_gguf(m.h, px, own.get("ggml_type", G.Q8_0), bp, *shape)
    else:
        rc = m.lib.fmi_flux_set_linear_f8(m.h, px, own.get("format", 1), bp, own.get("scale", 1.0), *shape)
    return [int(rc), m.lib.fmi_last_error().decode() if rc else ""]


OWN = {
    "bnb4": {"quant_type 3": dict(quant_type=3), "blocksize 48": dict(blocksize=48), "blocksize 192 does not divide 256": dict(blocksize=192)},
    "int8": {},
    "gguf": {"ggml type 10 (Q2_K)": dict(ggml_type=10), "in_features 250 is no multiple of 32": dict(shape=(256, 250))},
    "f8": {"format 3": dict(format=3), "scale 0": dict(scale=0.0), "scale inf": dict(scale=float("inf"))},
}
# two violations in one call: today's order of checks decides which message comes.  (handle, arguments)
COMBINED = {
    "bnb4": {"ControlNet + quant_type 3": ("cn", dict(quant_type=3)), "blocksize 48 + unknown prefix": ("plain", dict(blocksize=48, prefix="nope")),
             "LoRA merged + wrong shape": ("lora", dict(shape=(256, 512)))},
    "int8": {"ControlNet + unknown prefix": ("cn", dict(prefix="nope")), "LoRA merged + wrong shape": ("lora", dict(shape=(256, 512)))},
    "gguf": {"8-bit model + ggml type 10": ("q8", dict(ggml_type=10)), "in_features 250 + unknown prefix": ("plain", dict(shape=(256, 250), prefix="nope")),
             "LoRA merged + wrong shape": ("lora", dict(shape=(256, 512)))},
    "f8": {"ControlNet + format 3": ("cn", dict(format=3)), "scale 0 + unknown prefix": ("plain", dict(scale=0.0, prefix="nope")),
           "LoRA merged + wrong shape": ("lora", dict(shape=(256, 512)))},
}


def make_handles():
    """plain: a loaded bf16 model; cn: a ControlNet; q8: a model after quantize_fp8; lora: one with an adapter merged into PACKED; i8 / q4: models whose
    [q|k|v] matrix of block 0 holds an int8 / an nf4 to_k"""
    import diffusion_rs_amd as d
    from tests import controlnet_ref as CR
    h = {k: d.FluxModel(SMALL_FLUX) for k in ("plain", "q8", "lora", "i8", "q4")}
    h["cn"] = d.FluxControlNetModel(CR.net_cfg("2+0"))
    for k in ("plain", "q8", "lora", "i8", "q4"):
        h[k].load_state_dict(_sd(0))
    h["q8"].quantize_fp8()
    h["lora"].lora_add("a", PACKED, np.ones((2, 256), np.float32), np.ones((256, 2), np.float32))
    load(h["i8"], QKV[1], "int8", 0)
    load(h["q4"], QKV[1], "nf4", 0)
    return h


@pytest.fixture(scope="module")
def handles():
    h = make_handles()
    yield h
    for m in h.values():
        m.close()


def refusals(h, setter):
    """{case: [code, message]} of one setter"""
    out = {
        "null data": _call(h["plain"], setter, data=False),
        "unknown prefix": _call(h["plain"], setter, prefix="transformer_blocks.0.attn.nope"),
        "not a Linear (QkNorm weight)": _call(h["plain"], setter, prefix="transformer_blocks.0.attn.norm_q"),
        "wrong shape": _call(h["plain"], setter, shape=(256, 512)),
        "ControlNet handle": _call(h["cn"], setter),
        "model after quantize_fp8": _call(h["q8"], setter),
        "LoRA adapter merged": _call(h["lora"], setter),
    }
    for name, own in OWN[setter].items():
        out[name] = _call(h["plain"], setter, **own)
    if setter == "bnb4":
        out["onto a matrix holding int8 parts"] = _call(h["i8"], setter)
    if setter == "int8":
        out["onto a matrix holding 4-bit parts"] = _call(h["q4"], setter)
    for name, (handle, args) in COMBINED[setter].items():
        out[name] = _call(h[handle], setter, **args)
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("setter", SETTERS)
def test_refusals_are_what_they_were(handles, setter):
    got = refusals(handles, setter)
    print(json.dumps(got, indent=1))
    assert all(rc != 0 for rc, _ in got.values())
    assert got == golden()["refusals"][setter]


@pytest.mark.parametrize("case", CASES)
def test_transition_is_what_it_was(case):
    got = transition(case)
    print(case, json.dumps(got))
    assert got == golden()["transitions"][case]


def test_t5_setters_expand_to_the_stand_alone_dequant_values():
    """One nf4 and one int8 Linear of a 2-layer T5 through fmi_t5_set_linear_bnb4 / _int8, next to the same encoder given the bf16 values that
    dequantize_blockwise_bf16_nf4 / dequantize_8bit_kernel_bf16 write for those codes: the forward reads the slots, and is the same bit for bit.
    (tests/test_gpu_text.py compares with the oracle's restatement of the dequantisation; this one with the library's own stand-alone entries.)"""
    import torch
    import diffusion_rs_amd as d
    from diffusion_rs_amd import text
    cfg = dict(vocab_size=96, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=2, relative_attention_num_buckets=32,
               relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
    sd = d.synth.text_state_dict_numpy(d.synth.t5_tensor_shapes(cfg), seed=21)
    q4, q8 = "encoder.block.0.layer.0.SelfAttention.q", "encoder.block.1.layer.1.DenseReluDense.wo"
    lib = d._lib.load()
    gq, gd = text.T5EncoderModel(cfg), text.T5EncoderModel(cfg)
    for name, w in sd.items():
        if name[:-len(".weight")] not in (q4, q8):
            gq.set_tensor(name, w), gd.set_tensor(name, w)
    w = np.asarray(sd[q4 + ".weight"], np.float32)
    packed, absmax = d.synth.quantize_nf4_device(dev(w, torch.bfloat16), 64)
    out = torch.empty(w.shape, dtype=torch.bfloat16, device="cuda")
    lib.dequantize_blockwise_bf16_nf4(None, C.c_void_p(packed.data_ptr()), C.c_void_p(absmax.data_ptr()), C.c_void_p(out.data_ptr()), 64, w.size, None)
    torch.cuda.synchronize()
    gq.set_linear_bnb4(q4, packed, absmax, 64, "nf4", *w.shape)
    gd.set_tensor(q4 + ".weight", out)
    w = np.asarray(sd[q8 + ".weight"], np.float32)
    scb = np.abs(w).max(1).astype(np.float32)
    codes, scb = dev(np.clip(np.rint(w / scb[:, None] * 127.0), -127, 127).astype(np.int8)), dev(scb)
    out = torch.empty(w.shape, dtype=torch.bfloat16, device="cuda")
    lib.dequantize_8bit_kernel_bf16(C.c_void_p(codes.data_ptr()), C.c_void_p(scb.data_ptr()), C.c_void_p(out.data_ptr()), w.shape[0], w.shape[1], w.size)
    torch.cuda.synchronize()
    gq.set_linear_int8(q8, codes, scb, *w.shape)
    gd.set_tensor(q8 + ".weight", out)
    assert gq.missing() == [] and gd.missing() == []
    ids = np.random.default_rng(3).integers(0, 96, (2, 40)).astype(np.int32)
    a, b = gq.forward(ids, dtype=torch.float32), gd.forward(ids, dtype=torch.float32)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    gq.close(), gd.close()
