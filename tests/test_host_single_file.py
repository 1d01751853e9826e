"""Single-file FLUX checkpoints, host side: the new symbols, the safetensors reader on the 8-bit float dtypes, the BFL / diffusers name
maps on such a file (with and without `model.diffusion_model.`, with an all-in-one file's extras), the configuration inferred from shapes, "scaled fp8"
files, the refusals that come before any launch, and the front door's source.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import diffusion_rs_amd as d  # noqa: E402
from diffusion_rs_amd import _lib as L  # noqa: E402
from diffusion_rs_amd import loader  # noqa: E402
from tests import f8_ref as F8  # noqa: E402
from tests.gguf_ref import diffusers_to_bfl  # noqa: E402
from tests.util import SMALL_FLUX  # noqa: E402

C = L.C


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    assert "int fmi_f8_dequantize(int format, const void* codes, int64_t n_elems, float scale, void* out, fmi_dtype out_dtype, void* stream);" in header
    assert ("int fmi_flux_set_linear_f8(fmi_flux*, const char* prefix, int format, const void* codes, float scale, int out_features, int in_features);"
            in header)
    lib = L.load()
    for sym in ("fmi_f8_dequantize", "fmi_flux_set_linear_f8"):
        assert sym in L.EXPORTED and getattr(lib, sym).argtypes is not None
    assert lib.fmi_f8_dequantize.argtypes[3] is C.c_float and lib.fmi_flux_set_linear_f8.argtypes[4] is C.c_float
    assert callable(d.FluxModel.set_linear_f8) and callable(d.f8_dequantize)
    # additions only: the ABI number stays 6
    assert int(re.search(r"#define FMI_ABI_VERSION (\d+)", header).group(1)) == 6 and lib.fmi_abi_version() == 6
    assert loader._ST_DTYPES["F8_E4M3"] == (torch.float8_e4m3fn, 1) and loader._ST_DTYPES["F8_E5M2"] == (torch.float8_e5m2, 1)


def test_restatement_known_answers():
    """the values the issue states for torch's CPU decode, through f8_ref: e4m3fn 0x7e = 448, 0x7f = NaN; e5m2 0x7b = 57344, 0x7c = inf; one multiply, one
    rounding"""
    e4 = F8.dequantize_f32("e4m3", np.array([0x7E, 0x7F, 0x00, 0x80, 0x01, 0x38, 0xB8], np.uint8))
    assert e4[0] == 448 and np.isnan(e4[1]) and e4[2] == 0 and e4[3] == 0 and np.signbit(e4[3]) and e4[4] == 2.0 ** -9 and e4[5] == 1 and e4[6] == -1
    e5 = F8.dequantize_f32("e5m2", np.array([0x7B, 0x7C, 0xFC, 0x7D, 0x01, 0x3C], np.uint8))
    assert e5[0] == 57344 and e5[1] == np.inf and e5[2] == -np.inf and np.isnan(e5[3]) and e5[4] == 2.0 ** -16 and e5[5] == 1
    assert list(F8.is_nan_code("e4m3", np.array([0x7E, 0x7F, 0xFF], np.uint8))) == [False, True, True]
    assert list(F8.is_nan_code("e5m2", np.array([0x7C, 0x7D, 0xFE, 0xFC], np.uint8))) == [False, True, True, False]
    # 1.125 (e4m3 0x39) * 0.0123f, rounded once to f32, then once to bf16
    y = np.float32(1.125) * np.float32(0.0123)
    assert F8.dequantize_f32("e4m3", np.array([0x39], np.uint8), 0.0123)[0] == y
    assert F8.dequantize_bf16_bits("e4m3", np.array([0x39], np.uint8), 0.0123)[0] == torch.tensor(y).to(torch.bfloat16).view(torch.int16).item() & 0xFFFF


def test_reader_yields_both_fp8_dtypes_as_zero_copy_views(tmp_path):
    all_codes = np.arange(256, dtype=np.uint8).reshape(4, 64)
    p = tmp_path / "f8.safetensors"
    F8.write_safetensors(p, {"a.weight": torch.from_numpy(all_codes).view(torch.float8_e4m3fn), "b.weight": torch.from_numpy(all_codes).view(torch.float8_e5m2),
                             "c.bias": torch.arange(5, dtype=torch.bfloat16), "a.scale_weight": torch.tensor(0.5)})
    sf = loader.SingleFile(str(p))
    a, b = sf.tensors["a.weight"], sf.tensors["b.weight"]
    assert a.dtype == torch.float8_e4m3fn and b.dtype == torch.float8_e5m2 and tuple(a.shape) == tuple(b.shape) == (4, 64)
    np.testing.assert_array_equal(a.view(torch.uint8).numpy(), all_codes)
    np.testing.assert_array_equal(b.view(torch.uint8).numpy(), all_codes)
    assert tuple(sf.tensors["a.scale_weight"].shape) == () and float(sf.tensors["a.scale_weight"]) == 0.5
    base = np.frombuffer(sf._mm, np.uint8).ctypes.data  # zero-copy: the tensors point into the mapping
    for t in (a, b, sf.tensors["c.bias"]):
        assert base <= t.data_ptr() < base + len(sf._mm)
    with pytest.raises(FileNotFoundError):
        loader.SingleFile(str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- names
def host_spec(name, shape):
    """an all-fp8 file: 2-D weights e4m3 (the single blocks' e5m2), the biases fp8 as well; the QkNorm scales stay bf16"""
    if len(shape) == 2:
        return ("e5m2" if name.startswith(("single_transformer_blocks.", "single_blocks.")) else "e4m3", False)
    return ("e4m3", False) if name.endswith(".bias") else None


class RecordingModel:
    """Stands in for FluxModel: records what load_flux_single_file feeds."""

    def __init__(self, cfg):
        self.cfg, self.lib, self.dense, self.codes = dict(cfg), L.load(), {}, {}

    def set_tensor(self, name, t):
        assert name not in self.dense and name not in self.codes
        self.dense[name] = (t.dtype, t.float().numpy())

    def set_linear_f8(self, prefix, fmt, codes, scale, out_features, in_features):
        assert prefix + ".weight" not in self.dense and prefix + ".weight" not in self.codes
        self.codes[prefix + ".weight"] = (fmt, bytes(codes), scale, out_features, in_features)

    def assert_complete(self):
        want = d.synth.flux_tensor_shapes(self.cfg)
        missing = sorted(set(want) - set(self.dense) - set(self.codes))
        if missing:
            raise ValueError(f"{len(missing)} tensors missing, e.g. {missing[:3]}")


@pytest.fixture(scope="module")
def small_sd():
    return {k: np.asarray(v, np.float32) for k, v in d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=3).items()}


EXTRAS = {"vae.decoder.conv_in.weight": torch.zeros(2, 2, 3, 3, dtype=torch.bfloat16), "first_stage_model.encoder.conv_in.bias": torch.zeros(2),
          "text_encoders.clip_l.transformer.text_model.final_layer_norm.weight": torch.zeros(4, dtype=torch.float16),
          "cond_stage_model.t5xxl.shared.weight": torch.zeros(3, 4, dtype=torch.float8_e4m3fn), "unrelated.scalar": torch.tensor(1.0)}


def check_loaded(m, sd):
    """every diffusers tensor arrived once, holding what casting THAT tensor on its own gives (a plain cast is element-wise: cutting rows commutes with it)"""
    for name, a in sd.items():
        how = host_spec(name, a.shape)
        if how is None:
            dt, v = m.dense[name]
            assert dt == torch.bfloat16
            np.testing.assert_array_equal(v, torch.from_numpy(a).to(torch.bfloat16).float().numpy())
        elif len(a.shape) == 2:
            codes, _ = F8.quantize(a, how[0])
            assert m.codes[name] == (how[0], codes.tobytes(), 1.0, a.shape[0], a.shape[1]), name
        else:  # an fp8 bias: widened on the host, exactly
            dt, v = m.dense[name]
            assert dt == torch.float32
            np.testing.assert_array_equal(v, F8.dequantize_f32(how[0], F8.quantize(a, how[0])[0]))


@pytest.mark.parametrize("prefix", ["", "model.diffusion_model."])
@pytest.mark.parametrize("naming", ["bfl", "diffusers"])
def test_both_namings_map_onto_the_same_entries(tmp_path, small_sd, naming, prefix):
    src = diffusers_to_bfl(small_sd, SMALL_FLUX) if naming == "bfl" else small_sd
    tensors, _ = F8.quantize_state_dict(src, host_spec)
    p = str(tmp_path / "flux.safetensors")
    F8.write_safetensors(p, dict({prefix + n: t for n, t in tensors.items()}, **EXTRAS))
    sf = loader.SingleFile(p)
    entries, scales, skipped = loader.single_file_flux_entries(sf)
    want = d.synth.flux_tensor_shapes(SMALL_FLUX)
    assert sorted(e[0] for e in entries) == sorted(want) and scales == {}
    assert {e[0]: tuple(e[1]) for e in entries} == {k: tuple(v) for k, v in want.items()}
    assert sorted(skipped) == sorted(EXTRAS)
    if naming == "bfl":
        by = {e[0]: e for e in entries}
        D = 256
        assert by["transformer_blocks.1.attn.to_k.weight"][2:] == (prefix + "double_blocks.1.img_attn.qkv.weight", [(D, 2 * D)])
        assert by["single_transformer_blocks.1.proj_mlp.weight"][2:] == (prefix + "single_blocks.1.linear1.weight", [(3 * D, 7 * D)])
        assert by["norm_out.linear.weight"][2:] == (prefix + "final_layer.adaLN_modulation.1.weight", [(D, 2 * D), (0, D)])
    m = RecordingModel(SMALL_FLUX)
    stats = loader.load_flux_single_file(m, sf)
    check_loaded(m, small_sd)
    n2d = sum(1 for s in want.values() if len(s) == 2)
    assert stats["f8"] == n2d == len(m.codes) and stats["dense"] == len(want) - n2d and sorted(stats["skipped"]) == sorted(EXTRAS)
    assert set(stats["formats"]) == {"e4m3", "e5m2"} and sum(stats["formats"].values()) == n2d
    # the configuration comes from the shapes; a transformer/config.json that disagrees is named by field
    cfg = loader.flux_config_from_single_file(sf, dict(SMALL_FLUX, out_channels=None))
    assert all(cfg[k] == v for k, v in SMALL_FLUX.items()) and cfg["out_channels"] == 64
    assert loader.flux_config_from_single_file(p) == cfg
    for field, bad in (("num_layers", 3), ("joint_attention_dim", 4096), ("guidance_embeds", False), ("num_attention_heads", 24), ("num_single_layers", 5)):
        with pytest.raises(ValueError, match=field):
            loader.flux_config_from_single_file(sf, dict(SMALL_FLUX, **{field: bad}))
    with pytest.raises(ValueError, match="configuration says"):
        loader.load_flux_single_file(RecordingModel(dict(SMALL_FLUX, joint_attention_dim=256)), sf)


def test_a_missing_transformer_tensor_raises(tmp_path, small_sd):
    tensors, _ = F8.quantize_state_dict(diffusers_to_bfl(small_sd, SMALL_FLUX), host_spec)
    del tensors["double_blocks.1.txt_mlp.2.weight"]
    p = str(tmp_path / "short.safetensors")
    F8.write_safetensors(p, tensors)
    with pytest.raises(ValueError, match="ff_context.net.2.weight"):
        loader.load_flux_single_file(RecordingModel(SMALL_FLUX), p)
    F8.write_safetensors(p, {"foo.weight": torch.zeros(2, 2)})
    with pytest.raises(ValueError, match="neither BFL"):
        loader.load_flux_single_file(RecordingModel(SMALL_FLUX), p)


def scaled_spec(name, shape):
    return ("e4m3", True) if len(shape) == 2 else None


def test_scaled_fp8_files(tmp_path, small_sd):
    """`<linear>.scale_weight` is the scale of `<linear>.weight` — of every part cut out of a fused BFL matrix —; `scaled_fp8` and `<linear>.scale_input` are
    listed as skipped; a scale_weight that is not one F32 element raises, naming the tensor."""
    bfl = diffusers_to_bfl(small_sd, SMALL_FLUX)
    tensors, values = F8.quantize_state_dict(bfl, scaled_spec)
    extras = {"scaled_fp8": torch.zeros(2, dtype=torch.float8_e4m3fn), "double_blocks.0.img_attn.qkv.scale_input": torch.tensor(0.25),
              "stray.scale_weight": torch.tensor(1.0)}
    p = str(tmp_path / "scaled.safetensors")
    F8.write_safetensors(p, dict(tensors, **extras))
    m = RecordingModel(SMALL_FLUX)
    stats = loader.load_flux_single_file(m, p)
    assert sorted(stats["skipped"]) == sorted(extras)
    qkv = tensors["double_blocks.0.img_attn.qkv.weight"].view(torch.uint8).numpy()
    s = float(tensors["double_blocks.0.img_attn.qkv.scale_weight"])
    assert 0 < s < 1 and s != 1.0
    for i, part in enumerate(("to_q", "to_k", "to_v")):
        assert m.codes[f"transformer_blocks.0.attn.{part}.weight"] == ("e4m3", qkv[256 * i:256 * (i + 1)].tobytes(), s, 256, 256)
    # the final modulation's halves are exchanged on the stored bytes, under the tensor's one scale
    fin = tensors["final_layer.adaLN_modulation.1.weight"].view(torch.uint8).numpy()
    assert m.codes["norm_out.linear.weight"] == ("e4m3", np.concatenate([fin[256:], fin[:256]]).tobytes(), float(tensors["final_layer.adaLN_modulation.1.scale_weight"]), 512, 256)
    # the largest weight of a scaled tensor is max_finite * scale
    assert np.abs(F8.dequantize_f32("e4m3", qkv, s)).max() == np.float32(448) * np.float32(s)
    for bad in (torch.tensor([0.5, 0.5]), torch.full((768, 1), 0.5), torch.tensor(0.5, dtype=torch.float16), torch.tensor(0.0), torch.tensor(float("inf"))):
        F8.write_safetensors(p, dict(tensors, **{"double_blocks.0.img_attn.qkv.scale_weight": bad}))
        with pytest.raises(ValueError, match=r"double_blocks\.0\.img_attn\.qkv\.scale_weight"):
            loader.load_flux_single_file(RecordingModel(SMALL_FLUX), p)
    F8.write_safetensors(p, dict(tensors, **{"double_blocks.0.img_attn.qkv.scale_weight": torch.tensor([0.5])}))  # shape (1,) is accepted
    m = RecordingModel(SMALL_FLUX)
    loader.load_flux_single_file(m, p)
    assert m.codes["transformer_blocks.0.attn.to_k.weight"][2] == 0.5
    # a scale_weight next to a weight that is not fp8 is refused, not ignored
    F8.write_safetensors(p, dict(tensors, **{"double_blocks.0.img_attn.qkv.weight": torch.zeros(768, 256, dtype=torch.bfloat16)}))
    with pytest.raises(ValueError, match="scale_weight"):
        loader.load_flux_single_file(RecordingModel(SMALL_FLUX), p)


def test_refused_dequantize_calls_return_before_any_launch():
    lib = L.load()
    p, o = 4096, 8192  # never dereferenced: every call below is refused (or has nothing to do) on the host
    assert lib.fmi_f8_dequantize(0, p, 16, 1.0, o, L.BF16, None) == L.ERR_INVALID and b"format" in lib.fmi_last_error()
    assert lib.fmi_f8_dequantize(3, p, 16, 1.0, o, L.BF16, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(1, p, 16, 1.0, o, L.F16, None) == L.ERR_INVALID
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.fmi_f8_dequantize(1, p, 16, scale, o, L.BF16, None) == L.ERR_INVALID and b"scale" in lib.fmi_last_error()
    assert lib.fmi_f8_dequantize(2, p, -1, 1.0, o, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(2, None, 16, 1.0, o, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(2, p, 16, 1.0, None, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(1, p, 16, 1.0, o + 1, L.BF16, None) == L.ERR_INVALID  # out aligned to its element size
    assert lib.fmi_f8_dequantize(1, p, 16, 1.0, o + 2, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(1, None, 0, 1.0, None, L.BF16, None) == 0
    assert lib.fmi_flux_set_linear_f8(None, b"x", 1, p, 1.0, 2, 2) == L.ERR_INVALID
    assert d.flux.f8_format("e4m3") == 1 and d.flux.f8_format("e5m2") == 2 and d.flux.f8_format(torch.float8_e5m2) == 2 and d.flux.f8_format(7) == 7


def test_front_door_source():
    a = d.ModelSource.ModelId("base").override_transformer_file("x.safetensors")
    b = d.ModelSource.ModelId("base").override_transformer_model_id("x.safetensors")
    assert a.__dict__ == b.__dict__ and (a.kind, a.model_id, a.transformer_model_id) == ("model_id", "base", "x.safetensors")
    e = d.ModelSource.ModelId("base").override_transformer_file("x.safetensors", expand=True)
    assert e.transformer_expand is True and e.transformer_model_id == "x.safetensors"
    with pytest.raises(ValueError):
        d.ModelSource.DdufFile("f.dduf").override_transformer_file("x.safetensors")
