"""GGUF transformers, host side: the NumPy restatement of ggml's dequantisation against known answers written as literal bytes, the
GGUF reader against the test writer, the BFL -> diffusers name map, the configuration inferred from shapes, and the refusals.  No GPU."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import diffusion_rs_amd as d  # noqa: E402
from diffusion_rs_amd import _lib as L  # noqa: E402
from diffusion_rs_amd import loader  # noqa: E402
from tests import gguf_ref as G  # noqa: E402
from tests.util import SMALL_FLUX  # noqa: E402

K4_SCALES = bytes.fromhex("010203040002040685A6C7E8")  # sc_j = j + 1, m_j = 2 j (utils.rs:49)


def kat_blocks():
    """{ggml type: (block bytes, expected f32 values)} — one literal block per format, expected values in closed form (see the tests' docstrings)."""
    nib = bytes(j | ((15 - j) << 4) for j in range(16))
    ev = lambda j: 1 if j % 2 == 0 else 0  # noqa: E731
    out = {}
    out[G.Q4_0] = (bytes.fromhex("0038") + nib, [(j - 8) * 0.5 for j in range(16)] + [(7 - j) * 0.5 for j in range(16)])
    out[G.Q4_1] = (bytes.fromhex("003800C0") + nib, [j * 0.5 - 2 for j in range(16)] + [(15 - j) * 0.5 - 2 for j in range(16)])
    qh5 = bytes.fromhex("5555AAAA")
    out[G.Q5_0] = (bytes.fromhex("0038") + qh5 + nib,
                   [(j + 16 * ev(j) - 16) * 0.5 for j in range(16)] + [(15 - j + 16 * (1 - ev(j)) - 16) * 0.5 for j in range(16)])
    out[G.Q5_1] = (bytes.fromhex("003800C0") + qh5 + nib,
                   [(j + 16 * ev(j)) * 0.5 - 2 for j in range(16)] + [(15 - j + 16 * (1 - ev(j))) * 0.5 - 2 for j in range(16)])
    out[G.Q8_0] = (bytes.fromhex("0034") + bytes((j - 16) & 0xFF for j in range(32)), [(j - 16) * 0.25 for j in range(32)])
    out[G.Q4_K] = (bytes.fromhex("003C003C") + K4_SCALES + b"\x21" * 128, [v for run in (1, 2, -1, 2, -3, 2, -5, 2) for v in [run] * 32])
    qh = bytes(0xA5 if l % 2 == 0 else 0x5A for l in range(32))
    exp = []
    for s in range(8):
        for l in range(32):
            hb = (qh[l] >> s) & 1
            exp.append((s + 1) * ((1 if s % 2 == 0 else 2) + 16 * hb) - 2 * s)
    out[G.Q5_K] = (bytes.fromhex("003C003C") + K4_SCALES + qh + b"\x21" * 128, exp)
    sc = [(i + 1) * (-1 if i % 2 else 1) for i in range(16)]
    qh6 = bytes(0xE4 if l % 2 == 0 else 0x1B for l in range(32)) * 2
    qv = {0: (-31, -15, 2, 18), 1: (17, 1, -14, -30)}  # (q1, q2, q3, q4) for even / odd l
    exp = [0.0] * 256
    for idx in range(2):
        for l in range(32):
            for k in range(4):
                exp[128 * idx + 32 * k + l] = sc[8 * idx + l // 16 + 2 * k] * qv[l % 2][k]
    out[G.Q6_K] = (b"\x21" * 128 + qh6 + bytes(v & 0xFF for v in sc) + bytes.fromhex("003C"), exp)
    for t, (raw, _) in out.items():
        assert len(raw) == G.BLOCK[t][1]
    return out


def test_kat_q4_0():
    """d = f16 0x3800 = 0.5, qs[j] = j | ((15 - j) << 4): y[j] = (j - 8) * 0.5, y[16 + j] = (7 - j) * 0.5 (k_quants.rs:175)."""
    raw, exp = kat_blocks()[G.Q4_0]
    assert raw[:2] == b"\x00\x38"
    np.testing.assert_array_equal(G.dequantize_f32(G.Q4_0, raw), np.array(exp, np.float32))


def test_kat_q8_0():
    """d = f16 0x3400 = 0.25, qs[j] = int8(j - 16): y[j] = (j - 16) * 0.25 (:580)."""
    raw, exp = kat_blocks()[G.Q8_0]
    np.testing.assert_array_equal(G.dequantize_f32(G.Q8_0, raw), np.array(exp, np.float32))


def test_kat_q4_k():
    """d = dmin = 1, scales 01 02 03 04 00 02 04 06 85 A6 C7 E8 (sc_j = j + 1, m_j = 2 j), every qs byte 0x21 (low nibble 1: even sub-blocks,
    high nibble 2: odd ones): sub-block j is (j + 1) * q - 2 j = 1, 2, -1, 2, -3, 2, -5, 2 (:1568)."""
    raw, exp = kat_blocks()[G.Q4_K]
    got = G.dequantize_f32(G.Q4_K, raw)
    np.testing.assert_array_equal(got, np.array(exp, np.float32))
    assert [int(got[32 * j]) for j in range(8)] == [1, 2, -1, 2, -3, 2, -5, 2]


@pytest.mark.parametrize("t", [G.Q4_1, G.Q5_0, G.Q5_1, G.Q5_K, G.Q6_K], ids=lambda t: G.NAMES[t])
def test_kat_other_formats(t):
    """One literal block each (kat_blocks):
    Q4_1  d 0.5, m -2, Q4_0's nibbles: y[j] = j / 2 - 2, y[16 + j] = (15 - j) / 2 - 2 (:341).
    Q5_0  d 0.5, Q4_0's nibbles, qh = 55 55 AA AA (u32 0xAAAA5555: bit j set for even j < 16, bit 16 + j for odd j): the fifth bit adds 16 to the even
          elements of the first half and the odd ones of the second; y = (q5 - 16) / 2 (:440).   Q5_1: the same q5, y = q5 / 2 - 2 (:547).
    Q5_K  d = dmin = 1, Q4_K's scales (sc_s = s + 1, m_s = 2 s: all distinct), qs 0x21, qh[l] = A5 (l even) / 5A (l odd): bit s of qh[l] is the
          fifth bit of element l of sub-block s; y = (s + 1) * (q + 16 * bit) - 2 s with q = 1 (s even) / 2 (s odd) (:1872).
    Q6_K  d = 1, scales[i] = (i + 1) * (-1)^i (all distinct), ql 0x21, qh[l] = E4 (l even: two-bit fields 0, 1, 2, 3) / 1B (l odd: 3, 2, 1, 0):
          (q1, q2, q3, q4) = (1 | 0, 1 | 16, 2 | 32, 2 | 48) - 32 = (-31, -15, 2, 18) for even l and (17, 1, -14, -30) for odd l;
          y[128 idx + 32 k + l] = scales[8 idx + l / 16 + 2 k] * q_(k+1) (:2147)."""
    raw, exp = kat_blocks()[t]
    np.testing.assert_array_equal(G.dequantize_f32(t, raw), np.array(exp, np.float32))
    if t in (G.Q5_K, G.Q6_K):
        assert len(set(exp)) > 8


@pytest.mark.parametrize("t", G.TYPES, ids=lambda t: G.NAMES[t])
def test_encoder_sanity(t):
    """Guards the test inputs, not the product: |x - dequant(encode(x))| stays within the format's step (gguf_ref.step_bound derives it per format)."""
    rng = np.random.default_rng(t)
    x = (rng.standard_normal(16 * 256) * rng.uniform(0.01, 2.0, 16 * 256 // 32).repeat(32)).astype(np.float32)
    raw = G.encode(t, x)
    assert raw.size == x.size // G.BLOCK[t][0] * G.BLOCK[t][1]
    err = np.abs(G.dequantize_f32(t, raw).astype(np.float64) - x)
    bound = G.step_bound(t, x)
    assert np.all(err <= bound), (G.NAMES[t], float((err / bound).max()))
    assert np.abs(x).max() / 4 > bound.mean()  # (the bound says something)


@pytest.mark.parametrize("alignment", [32, 64])
def test_writer_reader_round_trip(tmp_path, alignment):
    rng = np.random.default_rng(0)
    q = G.encode(G.Q8_0, rng.standard_normal(6 * 64))
    a = rng.standard_normal((3, 5)).astype(np.float32)
    k = G.encode(G.Q6_K, rng.standard_normal(2 * 256))
    tensors = [("lin.weight", G.Q8_0, (6, 64), q.tobytes()), ("odd.weight", G.F32, (3, 5), a.tobytes()), ("k.weight", G.Q6_K, (2, 256), k.tobytes()),
               ("b.bias", G.F16, (7,), np.arange(7, dtype="<f2").tobytes())]
    meta = [("general.architecture", "str", "flux"), ("some.u8", "u8", 7), ("some.f64", "f64", 2.5), ("some.bool", "bool", True), ("some.i64", "i64", -3),
            ("names", ("array", "str"), ["a", "bcd", ""]), ("nums", ("array", "u16"), [1, 2, 3]), ("after.arrays", "u32", 99)]
    p = str(tmp_path / "t.gguf")
    where = G.write_gguf(p, tensors, meta, alignment=alignment)
    g = loader.GgufFile(p)
    assert g.version == 3 and g.alignment == alignment and g.data_offset % alignment == 0
    assert g.metadata["names"] == ["a", "bcd", ""] and g.metadata["nums"] == [1, 2, 3] and g.metadata["after.arrays"] == 99
    assert g.metadata["some.f64"] == 2.5 and g.metadata["some.bool"] is True and g.metadata["some.i64"] == -3 and g.metadata["general.architecture"] == "flux"
    got = list(g)
    assert [n for n, _, _, _ in got] == [t[0] for t in tensors]
    for (name, t, shape, raw), (gn, gt, gs, view) in zip(tensors, got):
        assert (gt, tuple(gs)) == (t, tuple(shape)) and isinstance(view, memoryview) and bytes(view) == raw
        assert g.tensors[name][2] == where[name] and where[name] % alignment == 0
    # the dims are stored innermost-first: (6, 64) is written as [64, 6]
    blob = open(p, "rb").read()
    i = blob.index(b"lin.weight") + len(b"lin.weight")
    assert struct.unpack_from("<IQQ", blob, i) == (2, 64, 6)
    # version 2 has the same layout
    p2 = str(tmp_path / "v2.gguf")
    G.write_gguf(p2, tensors, meta, alignment=alignment, version=2)
    assert loader.GgufFile(p2).version == 2 and bytes(loader.GgufFile(p2).data("k.weight")) == k.tobytes()


def test_reader_refusals(tmp_path):
    t = [("a.weight", G.Q8_0, (2, 32), bytes(68))]
    p = str(tmp_path / "x.gguf")
    G.write_gguf(p, t, magic=b"GGML")
    with pytest.raises(ValueError, match="magic"):
        loader.GgufFile(p)
    G.write_gguf(p, t, version=1)
    with pytest.raises(ValueError, match="version 1"):
        loader.GgufFile(p)
    G.write_gguf(p, t + t)
    with pytest.raises(ValueError, match="duplicate"):
        loader.GgufFile(p)
    G.write_gguf(p, t)
    blob = open(p, "rb").read()
    open(p, "wb").write(blob[:-1])
    with pytest.raises(ValueError, match="past the end"):
        loader.GgufFile(p)
    open(p, "wb").write(blob)
    assert loader.GgufFile(p).names() == ["a.weight"]


def test_unsupported_types_are_refused_by_name():
    lib = L.load()
    e, b = L.C.c_int(), L.C.c_int()
    for t in G.TYPES:
        assert lib.fmi_gguf_block_info(t, L.C.byref(e), L.C.byref(b)) == 0 and (e.value, b.value) == G.BLOCK[t] == loader.GGML_BLOCKS[t]
    for t, name in ((10, b"Q2_K"), (11, b"Q3_K"), (9, b"Q8_1"), (15, b"Q8_K"), (16, b"IQ2_XXS"), (20, b"IQ4_NL"), (23, b"IQ4_XS")):
        assert lib.fmi_gguf_block_info(t, None, None) == L.ERR_UNSUPPORTED and name in lib.fmi_last_error()
        assert lib.fmi_gguf_dequantize(t, None, 256, None, L.BF16, None) == L.ERR_UNSUPPORTED
    for t in (0, 1, 30, 99, -1):  # the plain types are not block formats either: they go through set_tensor
        assert lib.fmi_gguf_block_info(t, None, None) == L.ERR_UNSUPPORTED
    # argument checks come before any launch
    assert lib.fmi_gguf_dequantize(G.Q4_K, 16, 128, 16, L.BF16, None) == L.ERR_INVALID  # not a multiple of 256
    assert lib.fmi_gguf_dequantize(G.Q8_0, 16, 32, 16, L.F16, None) == L.ERR_INVALID   # BF16 | F32 only
    assert lib.fmi_gguf_dequantize(G.Q8_0, 17, 32, 16, L.BF16, None) == L.ERR_INVALID  # blocks are 2-byte aligned
    assert lib.fmi_gguf_dequantize(G.Q8_0, None, 32, 16, L.BF16, None) == L.ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- names
def small_type_of(name, shape):
    """What a real file does at SMALL_FLUX's widths: 2-D weights whose rows are whole 256-blocks get a K format, the 64- / 128-wide embedders a
    32-element format, everything 1-D stays plain."""
    if len(shape) != 2:
        return G.F32 if shape == (128,) else G.F16  # (the QkNorm scales in f32, the biases in f16)
    return G.Q4_K if shape[1] % 256 == 0 else G.Q5_0 if shape[1] % 32 == 0 else G.F16


class RecordingModel:
    """Stands in for FluxModel: records what load_flux_gguf feeds."""

    def __init__(self, cfg):
        self.cfg, self.lib, self.dense, self.packed = dict(cfg), L.load(), {}, {}

    def set_tensor(self, name, t):
        assert name not in self.dense and name not in self.packed
        self.dense[name] = t.numpy().astype(np.float32)  # (exact for f16 / f32)

    def set_linear_gguf(self, prefix, ggml_type, data, out_features, in_features):
        assert prefix + ".weight" not in self.dense and prefix + ".weight" not in self.packed
        self.packed[prefix + ".weight"] = (ggml_type, bytes(data), out_features, in_features)

    def assert_complete(self):
        want = d.synth.flux_tensor_shapes(self.cfg)
        assert set(self.dense) | set(self.packed) == set(want)


@pytest.fixture(scope="module")
def small_sd():
    return {k: np.asarray(v, np.float32) for k, v in d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=3).items()}


def check_loaded(m, sd):
    """every diffusers tensor arrived once, holding what quantising THAT tensor on its own gives"""
    for name, a in sd.items():
        t = small_type_of(name, a.shape)
        if t in (G.F32, G.F16):
            np.testing.assert_array_equal(m.dense[name], G.plain_values(a, t))
        else:
            assert m.packed[name] == (t, G.encode(t, a.reshape(-1)).tobytes(), a.shape[0], a.shape[1]), name


@pytest.mark.parametrize("prefix", ["", "model.diffusion_model."])
def test_bfl_names_map_to_diffusers(tmp_path, small_sd, prefix):
    """The full map on a SMALL_FLUX-shaped BFL file: every diffusers name once; qkv thirds, linear1's D, D, D, M rows and the exchanged halves of the
    final modulation, cut out of the PACKED bytes, equal the encoding of the diffusers tensor itself (a row is a whole number of blocks)."""
    bfl = G.diffusers_to_bfl(small_sd, SMALL_FLUX)
    tensors, _ = G.quantize_state_dict(bfl, small_type_of)
    p = str(tmp_path / "bfl.gguf")
    G.write_gguf(p, [(prefix + n, t, s, raw) for n, t, s, raw in tensors] + [("unrelated.scalar", G.F32, (), bytes(4))], [("general.architecture", "str", "flux")])
    g = loader.GgufFile(p)
    entries, skipped = loader.gguf_flux_entries(g)
    want = d.synth.flux_tensor_shapes(SMALL_FLUX)
    assert sorted(e[0] for e in entries) == sorted(want) and skipped == ["unrelated.scalar"]
    by = {e[0]: e for e in entries}
    D = 256
    assert by["transformer_blocks.1.attn.to_k.weight"][3:] == (prefix + "double_blocks.1.img_attn.qkv.weight", [(D, 2 * D)])
    assert by["transformer_blocks.0.attn.add_v_proj.bias"][3:] == (prefix + "double_blocks.0.txt_attn.qkv.bias", [(2 * D, 3 * D)])
    assert by["single_transformer_blocks.1.proj_mlp.weight"][3:] == (prefix + "single_blocks.1.linear1.weight", [(3 * D, 7 * D)])
    assert by["single_transformer_blocks.0.attn.to_v.weight"][4] == [(2 * D, 3 * D)]
    assert by["norm_out.linear.weight"][3:] == (prefix + "final_layer.adaLN_modulation.1.weight", [(D, 2 * D), (0, D)])
    assert by["norm_out.linear.bias"][4] == [(D, 2 * D), (0, D)]
    assert by["transformer_blocks.0.attn.norm_added_k.weight"][3] == prefix + "double_blocks.0.txt_attn.norm.key_norm.scale"
    m = RecordingModel(SMALL_FLUX)
    stats = loader.load_flux_gguf(m, g)
    check_loaded(m, small_sd)
    n2d = sum(1 for s in want.values() if len(s) == 2)
    assert stats["gguf"] == n2d and stats["dense"] == len(want) - n2d and stats["skipped"] == ["unrelated.scalar"]
    assert set(stats["types"]) == {"Q4_K", "Q5_0", "F16", "F32"} and sum(stats["types"].values()) == len(want)
    cfg = loader.flux_config_from_gguf(g)
    assert all(cfg[k] == v for k, v in SMALL_FLUX.items()) and cfg["out_channels"] == 64


def test_diffusers_names_are_taken_as_is(tmp_path, small_sd):
    tensors, _ = G.quantize_state_dict(small_sd, small_type_of)
    p = str(tmp_path / "diffusers.gguf")
    G.write_gguf(p, tensors)
    g = loader.GgufFile(p)
    m = RecordingModel(SMALL_FLUX)
    loader.load_flux_gguf(m, g)
    check_loaded(m, small_sd)
    cfg = loader.flux_config_from_gguf(g, dict(SMALL_FLUX, out_channels=None))
    assert all(cfg[k] == v for k, v in SMALL_FLUX.items())
    for field, bad in (("num_layers", 3), ("joint_attention_dim", 4096), ("guidance_embeds", False), ("num_attention_heads", 24)):
        with pytest.raises(ValueError, match=field):
            loader.flux_config_from_gguf(g, dict(SMALL_FLUX, **{field: bad}))
    # a model of another configuration refuses the file by shape
    with pytest.raises(ValueError, match="configuration says"):
        loader.load_flux_gguf(RecordingModel(dict(SMALL_FLUX, joint_attention_dim=256)), g)


def test_loader_refusals(tmp_path, small_sd):
    p = str(tmp_path / "bad.gguf")
    G.write_gguf(p, [("foo.weight", G.F16, (2, 2), bytes(8))])
    with pytest.raises(ValueError, match="neither BFL"):
        loader.load_flux_gguf(RecordingModel(SMALL_FLUX), p)
    # a supported file with one Q3_K tensor: refused by the type's name
    tensors, _ = G.quantize_state_dict(small_sd, small_type_of)
    name = "transformer_blocks.0.ff.net.2.weight"
    tensors = [(n, 11, s, bytes(s[0] * s[1] // 256 * 110)) if n == name else (n, t, s, raw) for n, t, s, raw in tensors]
    G.write_gguf(p, tensors)
    with pytest.raises(L.FmiError, match="Q3_K") as ei:
        loader.load_flux_gguf(RecordingModel(SMALL_FLUX), p)
    assert ei.value.code == L.ERR_UNSUPPORTED
    # the front door takes the file either way
    src = d.ModelSource.ModelId("base").override_transformer_gguf("x.gguf")
    assert (src.kind, src.model_id, src.transformer_model_id) == ("model_id", "base", "x.gguf")
