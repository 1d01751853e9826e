"""Host logic of the LyCORIS / DoRA adapter reader (diffusion_rs_amd.lora.read_adapter; CPU only, no HIP calls) and the declarations of the new C entries:
both key layouts of every kind give the same terms, fused kohya modules split (row slices for LoHa / DoRA / full differences, row_offset for LoKr), the
scale rules, what is refused by name, and a file round trip through the repository's own safetensors reader."""
import os
import re

import numpy as np
import pytest

from tests.adapter_ref import LOKR_C, MODULES, adapter_files, term_delta
from tests.lora_util import D, M, write_safetensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_tensor(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def assert_same_terms(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        assert g.kind == w.kind and g.scale == w.scale and g.row_offset == w.row_offset, (k, g.kind, g.scale, g.row_offset, w.kind, w.scale, w.row_offset)
        assert len(g.tensors) == len(w.tensors), k
        for x, y in zip(g.tensors, w.tensors):
            assert same_tensor(x, y), k


def test_new_symbols_are_declared_exported_and_bound():
    from diffusion_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    assert re.search(r"FMI_ABI_VERSION\s+6\b", header)  # additive: the number stays
    for sym in ("fmi_flux_lora_add_term", "fmi_adapter_merge"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTED
    for word in ("FMI_ADAPTER_LORA", "FMI_ADAPTER_LOHA", "FMI_ADAPTER_LOKR", "FMI_ADAPTER_DORA", "fmi_adapter_kind", "struct fmi_adapter_term"):
        assert word in header, word
    assert (_lib.ADAPTER_LORA, _lib.ADAPTER_LOHA, _lib.ADAPTER_LOKR, _lib.ADAPTER_DORA) == (0, 1, 2, 3)
    lib = _lib.load()  # (dlopen only: no GPU call)
    for sym in ("fmi_flux_lora_add_term", "fmi_adapter_merge"):
        assert getattr(lib, sym).argtypes is not None
    import diffusion_rs_amd as d
    assert callable(d.read_adapter) and callable(d.FluxModel.lora_add_term) and d.AdapterTerm("lora", (1, 2)).scale == 1.0
    with pytest.raises(Exception):  # frozen
        d.AdapterTerm("lora", (1, 2)).scale = 2.0


@pytest.mark.parametrize("kind", ["lora", "loha", "dora", "diff"])
def test_both_layouts_give_the_same_terms(kind):
    from diffusion_rs_amd.lora import read_adapter
    peft, kohya, want = adapter_files(kind, seed=1)
    assert len(want) == 20
    assert_same_terms(read_adapter(kohya), want)
    assert_same_terms(read_adapter(peft), want)
    assert_same_terms(read_adapter(kohya, hidden_size=D), want)


def test_lokr_layouts_and_row_offsets():
    from diffusion_rs_amd.lora import read_adapter
    peft, kohya, want = adapter_files("lokr", seed=2)
    got = read_adapter(kohya, hidden_size=D)
    assert_same_terms(got, want)
    # a fused module: every part shares the factors (the same objects) and carries its first row
    s1 = "single_transformer_blocks.1."
    parts = [got[s1 + p] for p in ("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp")]
    assert [p.row_offset for p in parts] == [0, D, 2 * D, 3 * D]
    assert all(x is y for p in parts[1:] for x, y in zip(p.tensors, parts[0].tensors))
    assert [got["transformer_blocks.0.attn." + p].row_offset for p in ("to_q", "to_k", "to_v")] == [0, D, 2 * D]
    assert got["transformer_blocks.0.ff.net.2"].row_offset == 0
    # the diffusers file states each part by its own rows of w1: the same terms on the unfused Linears, the same Delta on the parts of the fused ones
    gp = read_adapter(peft)
    assert set(gp) == set(want)
    for kname, rows, kin, alpha, targets, split in MODULES:
        for tgt, n in zip(targets, split):
            if len(targets) == 1:
                assert_same_terms({tgt: gp[tgt]}, {tgt: want[tgt]})
            else:
                assert gp[tgt].row_offset == 0 and gp[tgt].scale == want[tgt].scale
                w0 = np.zeros((n, kin))
                np.testing.assert_array_equal(term_delta(gp[tgt], w0), term_delta(want[tgt], w0))


def test_scale_rules():
    from diffusion_rs_amd.lora import read_adapter
    z = lambda *s: np.ones(s, np.float32)  # noqa: E731
    p = "transformer_blocks.0.attn.to_q"
    loha = {p + ".hada_w1_a": z(D, 4), p + ".hada_w1_b": z(4, D), p + ".hada_w2_a": z(D, 4), p + ".hada_w2_b": z(4, D)}
    assert read_adapter(loha)[p].scale == 1.0  # no alpha
    assert read_adapter(dict(loha, **{p + ".alpha": np.float32(2.0)}))[p].scale == 2.0 / 4
    full = {p + ".lokr_w1": z(4, 16), p + ".lokr_w2": z(64, 16), p + ".alpha": np.float32(8.0)}
    t = read_adapter(full)[p]
    assert t.kind == "lokr" and t.scale == 1.0 and t.tensors[1] is None and t.tensors[3] is None  # both factors full: the alpha is ignored
    w2dec = {p + ".lokr_w1_a": z(4, 2), p + ".lokr_w1_b": z(2, 16), p + ".lokr_w2_a": z(64, 3), p + ".lokr_w2_b": z(3, 16), p + ".alpha": np.float32(6.0)}
    assert read_adapter(w2dec)[p].scale == 6.0 / 3  # the rank of the decomposed w2
    w1dec = {p + ".lokr_w1_a": z(4, 2), p + ".lokr_w1_b": z(2, 16), p + ".lokr_w2": z(64, 16), p + ".alpha": np.float32(6.0)}
    assert read_adapter(w1dec)[p].scale == 6.0 / 2  # else of the decomposed w1
    assert read_adapter({k: v for k, v in w1dec.items() if "alpha" not in k})[p].scale == 1.0
    dora = {p + ".lora_A.weight": z(4, D), p + ".lora_B.weight": z(D, 4), p + ".lora_magnitude_vector": z(D), p + ".alpha": np.float32(2.0)}
    t = read_adapter(dora)[p]
    assert t.kind == "dora" and t.scale == 0.5 and t.tensors[2].shape == (D,)
    t = read_adapter({"lora_unet_double_blocks_0_img_attn_proj.lora_down.weight": z(4, D), "lora_unet_double_blocks_0_img_attn_proj.lora_up.weight": z(D, 4),
                      "lora_unet_double_blocks_0_img_attn_proj.dora_scale": z(D, 1)})["transformer_blocks.0.attn.to_out.0"]
    assert t.kind == "dora" and t.scale == 1.0 and t.tensors[2].shape == (D,)


def test_diff_becomes_the_lokr_term():
    from diffusion_rs_amd.lora import read_adapter
    diff = np.arange(3 * D * D, dtype=np.float32).reshape(3 * D, D)
    got = read_adapter({"lora_unet_double_blocks_0_img_attn_qkv.diff": diff, "transformer.transformer_blocks.1.attn.to_q.diff": diff[:D]})
    for i, p in enumerate(("to_q", "to_k", "to_v")):
        t = got["transformer_blocks.0.attn." + p]
        assert t.kind == "lokr" and t.scale == 1.0 and t.row_offset == 0 and t.tensors[1] is None and t.tensors[3] is None
        assert np.array_equal(np.asarray(t.tensors[0]), [[1.0]]) and np.array_equal(t.tensors[2], diff[i * D:(i + 1) * D])
        np.testing.assert_array_equal(term_delta(t, np.zeros((D, D))), diff[i * D:(i + 1) * D].astype(np.float64))
    assert np.array_equal(got["transformer_blocks.1.attn.to_q"].tensors[2], diff[:D])


def test_refused_keys_are_named_or_dropped():
    from diffusion_rs_amd.lora import read_adapter
    peft, kohya, want = adapter_files("loha", seed=3)
    z = np.zeros((2, 2), np.float32)
    q = "lora_unet_double_blocks_0_img_attn_proj"
    # a bias difference is dropped alone; a Tucker key or an input-axis dora_scale drops its module (the rest of it would merge as something else)
    cases = [({q + ".diff_b": z}, None), ({"transformer_blocks.0.attn.to_out.0.diff_b": z}, None),
             ({q + ".hada_t1": z, q + ".hada_t2": z}, "transformer_blocks.0.attn.to_out.0"),
             ({"lora_unet_double_blocks_0_txt_attn_proj.lokr_t2": z}, "transformer_blocks.0.attn.to_add_out")]
    for bad, dropped in cases:
        d = dict(kohya)
        d.update(bad)
        with pytest.raises(ValueError) as ei:
            read_adapter(d)
        for k in bad:
            assert k in str(ei.value)
        for k in kohya:
            assert k not in str(ei.value)
        assert_same_terms(read_adapter(d, skip_unsupported=True), {k: v for k, v in want.items() if k != dropped})
    # DoRA along the input axis: dora_scale (1, in)
    _, kd, wd = adapter_files("dora", seed=3)
    bad = dict(kd)
    bad[q + ".dora_scale"] = np.ones((1, D), np.float32)
    with pytest.raises(ValueError, match=re.escape(q + ".dora_scale")):
        read_adapter(bad)
    assert_same_terms(read_adapter(bad, skip_unsupported=True), {k: v for k, v in wd.items() if k != "transformer_blocks.0.attn.to_out.0"})
    # text-encoder and final-layer modules stay unsupported
    with pytest.raises(ValueError, match="lora_te1"):
        read_adapter(dict(kohya, **{"lora_te1_text_model_encoder_layers_0_mlp_fc1.hada_w1_a": z}))
    with pytest.raises(ValueError, match="final_layer"):
        read_adapter(dict(kohya, **{"lora_unet_final_layer_linear.lokr_w1": z}))
    # an incomplete group raises in either mode
    for skip in (False, True):
        with pytest.raises(ValueError, match="incomplete"):
            read_adapter({k: v for k, v in kohya.items() if k != q + ".hada_w2_b"}, skip_unsupported=skip)
        with pytest.raises(ValueError):
            read_adapter({"transformer_blocks.0.attn.to_q.lokr_w1": z, "transformer_blocks.0.attn.to_q.lokr_w2_a": z}, skip_unsupported=skip)
        with pytest.raises(ValueError):  # a magnitude without its pair
            read_adapter({"transformer_blocks.0.attn.to_q.lora_magnitude_vector": np.zeros(D, np.float32)}, skip_unsupported=skip)
        with pytest.raises(ValueError):  # two parametrisations on one module
            read_adapter(dict(kohya, **{q + ".lora_down.weight": z, q + ".lora_up.weight": z}), skip_unsupported=skip)


def test_read_lora_points_to_read_adapter():
    from diffusion_rs_amd.lora import read_lora
    for kind in ("loha", "lokr", "dora"):
        with pytest.raises(ValueError, match="read_adapter") as ei:
            read_lora(adapter_files(kind, seed=4)[1])
        assert kind in str(ei.value)
    peft, kohya, want = adapter_files("lora", seed=4)
    got = read_lora(kohya)  # files of plain pairs: (A, B, scale) as ever
    assert set(got) == set(want)
    for k, w in want.items():
        assert same_tensor(got[k][0], w.tensors[0]) and same_tensor(got[k][1], w.tensors[1]) and got[k][2] == w.scale


def test_adapter_file_round_trips_through_the_repository_reader(tmp_path):
    import torch
    from diffusion_rs_amd.lora import read_adapter
    for kind in ("loha", "lokr", "dora"):
        peft, kohya, want = adapter_files(kind, seed=5)
        mixed = {k: (v.astype(np.float16) if "img_mlp" in k and v.ndim == 2 else v) for k, v in kohya.items()}  # two dtypes in one file
        path = tmp_path / f"{kind}.safetensors"
        write_safetensors(path, mixed)
        got = read_adapter(path, hidden_size=D)
        assert set(got) == set(want)
        halves = 0
        for k, w in want.items():
            g = got[k]
            assert g.kind == w.kind and g.scale == w.scale and g.row_offset == w.row_offset
            for x, y in zip(g.tensors, w.tensors):
                if y is None:
                    assert x is None
                    continue
                assert isinstance(x, torch.Tensor)
                f16 = "ff.net" in k
                halves += x.dtype == torch.float16
                assert x.dtype == (torch.float16 if f16 else torch.float32), k
                np.testing.assert_array_equal(x.float().numpy(), y.astype(np.float16).astype(np.float32) if f16 else y)
        assert halves > 0
