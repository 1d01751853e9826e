"""8-bit float weights, the test side: the torch restatement of fmi_f8_dequantize, a quantiser for test weights (plain cast, or "scaled
fp8": one f32 scale per tensor), and a writer of .safetensors files whose tensors carry the dtypes F8_E4M3 / F8_E5M2.  torch's CPU float8 types decode both
formats (e4m3fn 0x7e = 448, 0x7f = NaN; e5m2 0x7b = 57344, 0x7c = inf)."""
import numpy as np
import torch

FORMATS = ("e4m3", "e5m2")
FORMAT_ID = {"e4m3": 1, "e5m2": 2}  # fmi_f8_dequantize's `format`
TORCH = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
ST_NAME = {"e4m3": "F8_E4M3", "e5m2": "F8_E5M2"}
MAX_FINITE = {"e4m3": 448.0, "e5m2": 57344.0}


def _codes(fmt, codes) -> torch.Tensor:
    c = np.ascontiguousarray(codes, np.uint8)
    return torch.from_numpy(c).view(TORCH[fmt])


def dequantize_f32(fmt, codes, scale=1.0) -> np.ndarray:
    """f32(code) * f32(scale), one rounded f32 multiply; codes: a uint8 array of any shape."""
    return (_codes(fmt, codes).float() * torch.tensor(float(scale), dtype=torch.float32)).numpy()


def dequantize_bf16_bits(fmt, codes, scale=1.0) -> np.ndarray:
    """the bf16 result's bits (uint16): dequantize_f32 rounded once, to nearest even"""
    y = (_codes(fmt, codes).float() * torch.tensor(float(scale), dtype=torch.float32)).to(torch.bfloat16)
    return y.view(torch.int16).numpy().view(np.uint16)


def dequantize_bf16_values(fmt, codes, scale=1.0) -> np.ndarray:
    """the bf16 result as f32 values: the dense twin's weights"""
    return (_codes(fmt, codes).float() * torch.tensor(float(scale), dtype=torch.float32)).to(torch.bfloat16).float().numpy()


def is_nan_code(fmt, codes) -> np.ndarray:
    c = np.asarray(codes, np.uint8) & 0x7F
    return c == 0x7F if fmt == "e4m3" else c > 0x7C


def quantize(a, fmt, scaled=False):
    """(codes uint8 of a's shape, scale): plain — the cast of a itself, scale 1 —, or scaled — scale = absmax / max_finite as f32, a / scale clamped to
    +- max_finite before the cast (torch's cast does not saturate: it yields NaN)."""
    x = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    scale = 1.0
    if scaled:
        s = (x.abs().max() / MAX_FINITE[fmt]).to(torch.float32)
        assert float(s) > 0
        x = (x / s).clamp(-MAX_FINITE[fmt], MAX_FINITE[fmt])
        scale = float(s)
    q = x.to(TORCH[fmt])
    codes = q.view(torch.uint8).numpy()
    assert not is_nan_code(fmt, codes).any()
    return codes, scale


def quantize_state_dict(sd: dict, spec, scale_suffix=".scale_weight"):
    """sd: {name: f32 array}; spec(name, shape) -> None (the tensor stays bf16) | (fmt, scaled).  Returns ({name: torch tensor} as a file holds them — fp8
    tensors as torch float8, the others bf16, `<linear>.scale_weight` f32 () next to a scaled weight — and {name: f32 array of the values the file states,
    rounded to bf16: the dense twin's weights})."""
    tensors, values = {}, {}
    for name, a in sd.items():
        a = np.asarray(a, np.float32)
        how = spec(name, a.shape)
        if how is None:
            t = torch.from_numpy(a).to(torch.bfloat16)
            tensors[name], values[name] = t, t.float().numpy()
            continue
        fmt, scaled = how
        codes, scale = quantize(a, fmt, scaled)
        tensors[name] = torch.from_numpy(codes).view(TORCH[fmt])
        if scaled:
            assert name.endswith(".weight")
            tensors[name[:-len(".weight")] + scale_suffix] = torch.tensor(scale, dtype=torch.float32)
        values[name] = dequantize_bf16_values(fmt, codes, scale)
    return tensors, values


def write_safetensors(path, tensors: dict, metadata=None):
    """{name: torch tensor} -> a .safetensors file; float8 tensors are written as F8_E4M3 / F8_E5M2 entries."""
    from safetensors.torch import save_file
    save_file({k: v.contiguous().clone() for k, v in tensors.items()}, str(path), metadata=metadata)  # (clones: the inputs may share memory)
