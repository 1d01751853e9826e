"""Single-file FLUX checkpoints on the GPU: fmi_f8_dequantize bit for bit against the torch restatement (tests/f8_ref.py),
fmi_flux_set_linear_f8 against a dense model loaded with the dequantised weights, and the front door."""
import ctypes as C

import numpy as np
import pytest

from tests import f8_ref as F8
from tests.gguf_ref import diffusers_to_bfl
from tests.util import SMALL_FLUX, SMALL_VAE, bf16_round, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu

SCALES = (1.0, 2.0 ** -7, 0.0123, 3.0e-4, 2.0 ** 20)  # all inside [2^-40, 2^40]: no result is a bf16 subnormal (outside the contract)
LENGTHS = (1, 15, 16, 17, 255, 4097, 66560)            # scalar-only, one vector, tails, more than one workgroup, a partial last one; 66560 = 130 x 512
OFFSETS = (0, 1, 3)                                     # bytes between a 16-byte boundary and the first code
GUARD = 24                                              # output elements after the last one, which no launch may write


@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    from diffusion_rs_amd import _lib as L
    return dict(torch=torch, d=d, L=L, lib=L.load())


def gpu_dequant(env, fmt, codes, scale, out_dtype, offset=0):
    """codes (uint8 array) on the device, `offset` filler bytes in front of them, through fmi_f8_dequantize; returns the output's bits (uint16 for bf16, uint32
    for f32) after checking that the GUARD elements behind the output kept their fill."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    n = codes.size
    buf = torch.from_numpy(np.concatenate([np.full(offset, 0x7F, np.uint8), codes])).cuda()
    assert buf.data_ptr() % 16 == 0
    bf = out_dtype == "bf16"
    out = torch.full((n + GUARD,), -2.0, dtype=torch.bfloat16 if bf else torch.float32, device="cuda")
    L.check(lib.fmi_f8_dequantize(F8.FORMAT_ID[fmt], C.c_void_p(buf.data_ptr() + offset), n, scale, C.c_void_p(out.data_ptr()), L.BF16 if bf else L.F32,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    torch.cuda.synchronize()
    assert bool((out[n:] == -2.0).all())
    return out[:n].view(torch.int16).cpu().numpy().view(np.uint16) if bf else out[:n].cpu().numpy().view(np.uint32)


def check_bits(fmt, codes, got, want, what):
    """bit equality for every non-NaN code, NaN-ness for the NaN codes"""
    nan = F8.is_nan_code(fmt, codes)
    np.testing.assert_array_equal(got[~nan], want[~nan], err_msg=what)
    if nan.any():
        as_f = (got[nan].astype(np.uint32) << 16).view(np.float32) if got.dtype == np.uint16 else got[nan].view(np.float32)
        assert np.isnan(as_f).all(), what


@pytest.fixture(scope="module")
def random_codes():
    """130 x 512 random codes — every code value, NaNs and e5m2's infinities included — and a copy of them for the tails"""
    return np.random.default_rng(8).integers(0, 256, 130 * 512, dtype=np.uint8)


@pytest.mark.parametrize("out_dtype", ["bf16", "f32"])
@pytest.mark.parametrize("fmt", F8.FORMATS)
def test_dequantize_bit_equal(env, random_codes, fmt, out_dtype):
    every = np.arange(256, dtype=np.uint8)
    ref = F8.dequantize_bf16_bits if out_dtype == "bf16" else (lambda f, c, s: F8.dequantize_f32(f, c, s).view(np.uint32))
    for scale in SCALES:
        want_every, want_random = ref(fmt, every, scale), ref(fmt, random_codes, scale)  # (the reference of a prefix is the prefix of the reference)
        for off in OFFSETS:
            check_bits(fmt, every, gpu_dequant(env, fmt, every, scale, out_dtype, off), want_every, f"all codes, scale {scale}, offset {off}")
            for n in LENGTHS:
                check_bits(fmt, random_codes[:n], gpu_dequant(env, fmt, random_codes[:n], scale, out_dtype, off), want_random[:n],
                           f"{n} codes, scale {scale}, offset {off}")
    # scale 1 gives the code's value itself; e5m2's infinities stay infinities
    one = gpu_dequant(env, fmt, every, 1.0, "f32").view(np.float32)
    val = F8.dequantize_f32(fmt, every)
    finite = np.isfinite(val)
    np.testing.assert_array_equal(one[finite], val[finite])
    if fmt == "e5m2":
        assert one[0x7C] == np.inf and one[0xFC] == -np.inf
        assert gpu_dequant(env, fmt, every, 3.0e-4, "f32").view(np.float32)[0x7C] == np.inf
    else:
        assert one[0x7E] == 448.0 and np.isnan(one[0x7F]) and one[0x80] == 0 and np.signbit(one[0x80])


def test_dequantize_past_2_to_31_codes(env):
    """Indexes are 64-bit: 2^31 + 48 e4m3 codes (2.1 GB in, 4.3 GB out) whose bytes repeat with a period of 16 x 4057 random non-NaN codes (2^27 + 3 =
    4057 x 33083), so the expected output is the reference of one period repeated — compared on the device."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    n, period = (1 << 31) + 48, 16 * 4057
    assert n % period == 0
    pat = np.random.default_rng(9).integers(0, 256, period, dtype=np.uint8)
    pat[F8.is_nan_code("e4m3", pat)] = 0x35
    want = torch.from_numpy(F8.dequantize_bf16_bits("e4m3", pat, 0.0123).view(np.int16)).cuda()
    buf = torch.from_numpy(pat).cuda().repeat(n // period)
    out = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    L.check(lib.fmi_f8_dequantize(1, C.c_void_p(buf.data_ptr()), n, 0.0123, C.c_void_p(out.data_ptr()), L.BF16, C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16).view(-1, period) == want).all())


def test_refused_calls_write_nothing(env):
    L, lib, torch = env["L"], env["lib"], env["torch"]
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1024, dtype=torch.float32, device="cuda")
    p, o = C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr())
    buf.fill_(0x38)  # (1.0 in e4m3: any launch would leave non-zero values)
    for fmt in (0, 3, -1, 8):
        assert lib.fmi_f8_dequantize(fmt, p, 256, 1.0, o, L.F32, None) == L.ERR_INVALID
    for dt in (L.F16, L.U8):
        assert lib.fmi_f8_dequantize(1, p, 256, 1.0, o, dt, None) == L.ERR_INVALID
    for scale in (0.0, -2.0, float("inf"), float("nan")):
        assert lib.fmi_f8_dequantize(1, p, 256, scale, o, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(1, p, -256, 1.0, o, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(1, None, 256, 1.0, o, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(1, p, 256, 1.0, None, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(1, p, 256, 1.0, C.c_void_p(out.data_ptr() + 2), L.F32, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(1, p, 256, 1.0, C.c_void_p(out.data_ptr() + 1), L.BF16, None) == L.ERR_INVALID
    assert lib.fmi_f8_dequantize(1, p, 0, 1.0, o, L.F32, None) == 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0
    y = env["d"].f8_dequantize(buf[3:259], "e4m3", 0.5, torch.float32)  # the Python form, from an odd byte offset
    assert tuple(y.shape) == (256,) and bool((y == 0.5).all())


# ---------------------------------------------------------------------------------------------------------------- the model
def spec_e4m3(name, shape):
    return ("e4m3", False) if len(shape) == 2 else None


def spec_e5m2_scaled(name, shape):
    return ("e5m2", True) if len(shape) == 2 else None


EMBEDDERS = ("x_embedder.", "context_embedder.", "time_text_embed.", "proj_out.")


def spec_mixed(name, shape):
    """to_q e4m3 next to bf16 to_k / to_v inside one fused [q|k|v] matrix — which the mixed rule expands into the dense arena at finalize() — and bf16 embedders"""
    if len(shape) != 2 or name.startswith(EMBEDDERS) or name.endswith(("attn.to_k.weight", "attn.to_v.weight")):
        return None
    return ("e4m3", False)


SPECS = {"e4m3": spec_e4m3, "e5m2_scaled": spec_e5m2_scaled, "mixed": spec_mixed}
T3 = [1.0, 0.75, 0.4, 0.0]
PACKED = "transformer_blocks.0.attn.to_q"


def feed(gm, tensors):
    """{name: torch tensor} of f8_ref.quantize_state_dict under diffusers names, straight into the model"""
    import torch
    for name, t in tensors.items():
        if name.endswith(".scale_weight"):
            continue
        if t.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
            scale = float(tensors.get(name[:-len(".weight")] + ".scale_weight", 1.0))
            gm.set_linear_f8(name[:-len(".weight")], t.dtype, t, scale, t.shape[0], t.shape[1])
        else:
            gm.set_tensor(name, t)
    gm.assert_complete()


def run(env, gm, inputs):
    torch = env["torch"]
    img, ids, txt, txt_ids, y = inputs
    t, g = np.array([0.75], np.float32), np.array([3.5], np.float32)
    fwd = gm.forward(dev(img), dev(ids), dev(txt, torch.bfloat16), dev(txt_ids), dev(t), dev(y), dev(g))
    den = gm.denoise(dev(img), dev(ids), dev(txt, torch.bfloat16), dev(txt_ids), dev(y), dev(g), T3)
    torch.cuda.synchronize()
    return host(fwd), host(den)


@pytest.fixture(scope="module")
def twins(env):
    """per spec: the file's tensors, the dense twin's weights (f8_ref's bf16 values), the twin's forward / 3-step denoise, and the oracle's on the same
    weights — computed once"""
    d = env["d"]
    from oracle import oracle as orc
    sd = {k: np.asarray(v, np.float32) for k, v in d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=11).items()}
    inputs = flux_inputs(SMALL_FLUX, 1, (4, 4), 8)
    out = {"inputs": inputs}
    for key, spec in SPECS.items():
        tensors, values = F8.quantize_state_dict(sd, spec)
        dense = d.FluxModel(SMALL_FLUX)
        dense.load_state_dict(values)
        fwd, den = run(env, dense, inputs)
        dense_bytes = dense.size_in_bytes()
        dense.close()
        om = orc.Flux(SMALL_FLUX)
        om.load(values)
        img, ids, txt, txt_ids, y = inputs
        g = np.array([3.5], np.float32)
        out[key] = dict(tensors=tensors, values=values, fwd=fwd, den=den, dense_bytes=dense_bytes,
                        ofwd=om.forward(img, ids, txt, txt_ids, np.array([0.75], np.float32), y, g), oden=om.denoise(img, ids, txt, txt_ids, y, g, T3))
    return out


@pytest.mark.parametrize("key", list(SPECS))
def test_set_linear_f8_is_the_dense_model_of_the_dequantised_weights(env, twins, key):
    """forward and a 3-step denoise, bit-identical to the dense twin in dense-cache modes 0, 3, 1 and 2 (2 runs as 0): same operands, same kernels — and the twin
    within test_gpu_gguf.py's bars of the oracle on those weights (1e-2 one evaluation, 3e-2 the loop)."""
    d, L, tw = env["d"], env["L"], twins[key]
    gm = d.FluxModel(SMALL_FLUX)
    feed(gm, tw["tensors"])
    assert sum(1 for t in tw["tensors"].values() if t.element_size() == 1) >= 30
    for mode in (0, 3, 1, 2):
        gm.set_quant_dense_cache(mode)
        fwd, den = run(env, gm, twins["inputs"])
        np.testing.assert_array_equal(fwd.view(np.uint32), tw["fwd"].view(np.uint32), err_msg=f"forward, mode {mode}")
        np.testing.assert_array_equal(den.view(np.uint32), tw["den"].view(np.uint32), err_msg=f"denoise, mode {mode}")
    e1, e3 = rel_l2(tw["fwd"], tw["ofwd"]), rel_l2(tw["den"], tw["oden"])
    print(f"{key}: forward rel-L2 vs oracle {e1:.3e}, 3-step denoise {e3:.3e}")
    assert e1 <= 1e-2 and e3 <= 3e-2
    if key == "mixed":  # the mixture ends dense: the fused [q|k|v] matrix reads back, the fp8 part as its dequantised values
        for part in ("to_q", "to_k"):
            name = f"transformer_blocks.0.attn.{part}.weight"
            np.testing.assert_array_equal(host(gm.get_tensor(name)), tw["values"][name])
        with pytest.raises(L.FmiError) as ei:  # (a matrix whose parts are all e4m3 stays codes)
            gm.get_tensor("transformer_blocks.0.ff.net.0.proj.weight")
        assert ei.value.code == L.ERR_UNSUPPORTED
    if key == "e5m2_scaled":  # the parts of one fused matrix carry different scales
        s = {float(tw["tensors"][f"transformer_blocks.0.attn.{p}.scale_weight"]) for p in ("to_q", "to_k", "to_v")}
        assert len(s) == 3
    gm.close()


def test_size_in_bytes_counts_the_codes(env, twins):
    d, tw = env["d"], twins["e4m3"]
    want = d.synth.flux_tensor_shapes(SMALL_FLUX)
    gm = d.FluxModel(SMALL_FLUX)
    gm.set_quant_dense_cache(0)
    feed(gm, tw["tensors"])
    # a model holding everything BUT the block linears: the BASE and modulation arenas, which an fp8 model holds dense too
    part = d.FluxModel(SMALL_FLUX)
    for name in want:
        if not d.synth.is_block_linear(name):
            part.set_tensor(name, tw["values"][name])
    code_bytes = sum(s[0] * s[1] for n, s in want.items() if d.synth.is_block_linear(n))
    assert code_bytes > 0 and gm.size_in_bytes() - part.size_in_bytes() == code_bytes
    run(env, gm, twins["inputs"])
    packed_only = gm.size_in_bytes()
    assert packed_only < tw["dense_bytes"]  # (the same evaluations: the same workspace; the scratch included)
    gm.set_quant_dense_cache(1)
    run(env, gm, twins["inputs"])
    assert gm.size_in_bytes() > packed_only
    gm.close(), part.close()


def test_expand_gives_an_ordinary_bf16_model(env, twins, tmp_path):
    d, tw = env["d"], twins["e5m2_scaled"]
    from diffusion_rs_amd import loader
    p = str(tmp_path / "scaled.safetensors")
    F8.write_safetensors(p, tw["tensors"])
    gm = d.FluxModel(SMALL_FLUX)
    stats = loader.load_flux_single_file(gm, p, expand=True)
    assert stats["f8"] == sum(1 for s in d.synth.flux_tensor_shapes(SMALL_FLUX).values() if len(s) == 2) and stats["formats"] == {"e5m2": stats["f8"]}
    for name in (PACKED + ".weight", "single_transformer_blocks.1.proj_mlp.weight", "context_embedder.weight", "norm_out.linear.weight"):
        np.testing.assert_array_equal(host(gm.get_tensor(name)), tw["values"][name])
    fwd, den = run(env, gm, twins["inputs"])
    np.testing.assert_array_equal(fwd.view(np.uint32), tw["fwd"].view(np.uint32))
    assert gm.size_in_bytes() == tw["dense_bytes"]
    gm.lora_add("a", PACKED, np.ones((2, 256), np.float32), np.ones((256, 2), np.float32))
    assert gm.loras() == ["a"]
    gm.lora_remove()
    blob = gm.state_export()
    assert len(blob) > 0
    gm.quantize_fp8()
    gm.close()


def test_refusals_leave_the_state_untouched(env, twins, monkeypatch):
    d, L, torch = env["d"], env["L"], env["torch"]
    tw = twins["e4m3"]
    gm = d.FluxModel(SMALL_FLUX)
    feed(gm, tw["tensors"])
    run(env, gm, twins["inputs"])
    with pytest.raises(L.FmiError) as ei:
        gm.get_tensor(PACKED + ".weight")
    assert ei.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.FmiError) as ei:
        gm.lora_add("a", PACKED, np.zeros((2, 256), np.float32), np.zeros((256, 2), np.float32))
    assert ei.value.code == L.ERR_UNSUPPORTED
    # embedders and modulation linears were expanded at load: they read back as the dequantised values
    for name in ("context_embedder.weight", "transformer_blocks.1.norm1.linear.weight", "norm_out.linear.weight"):
        np.testing.assert_array_equal(host(gm.get_tensor(name)), tw["values"][name])
    for call in (gm.quantize_fp8, gm.quantize_int8, gm.calibrate_int8):
        with pytest.raises(L.FmiError) as ei:
            call()
        assert ei.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.FmiError) as ei:
        gm.state_export()
    assert ei.value.code == L.ERR_UNSUPPORTED
    from diffusion_rs_amd import dist as D
    monkeypatch.setattr(D, "world", lambda: (0, 2))
    monkeypatch.setattr(D.dist, "broadcast_object_list", lambda head, src=0: None)
    with pytest.raises(D.StateExportUnsupported):
        D.broadcast_state(gm, gm.device)
    # the setter's own refusals
    raw = np.full(256 * 256, 0x38, np.uint8)
    rp = C.c_void_p(raw.ctypes.data)
    for args, code in (((b"transformer_blocks.0.attn.nope", 1, 1.0, 256, 256), L.ERR_INVALID), ((PACKED.encode(), 1, 1.0, 256, 512), L.ERR_INVALID),
                       ((PACKED.encode(), 3, 1.0, 256, 256), L.ERR_INVALID), ((PACKED.encode(), 1, 0.0, 256, 256), L.ERR_INVALID),
                       ((PACKED.encode(), 2, float("nan"), 256, 256), L.ERR_INVALID), ((PACKED.encode(), 1, 1.0, 0, 256), L.ERR_INVALID)):
        rc = gm.lib.fmi_flux_set_linear_f8(gm.h, args[0], args[1], rp, args[2], args[3], args[4])
        assert rc == code, (args, rc)
    assert gm.lib.fmi_flux_set_linear_f8(gm.h, PACKED.encode(), 1, None, 1.0, 256, 256) == L.ERR_INVALID
    with pytest.raises(L.FmiError) as ei:
        gm.set_linear_f8("context_embedder", "e4m3", raw[:100], 1.0, 256, 128)  # too few codes for the shape
    assert ei.value.code == L.ERR_INVALID
    # every refusal above left the model as it was
    fwd, den = run(env, gm, twins["inputs"])
    np.testing.assert_array_equal(fwd.view(np.uint32), tw["fwd"].view(np.uint32))
    np.testing.assert_array_equal(den.view(np.uint32), tw["den"].view(np.uint32))
    from tests import controlnet_ref as CR
    cn = d.FluxControlNetModel(CR.net_cfg("2+0"))
    assert cn.lib.fmi_flux_set_linear_f8(cn.h, PACKED.encode(), 1, rp, 1.0, 256, 256) == L.ERR_UNSUPPORTED
    # a weight with LoRA adapters merged, and a model in an 8-bit mode, as fmi_flux_set_linear_gguf
    dense = d.FluxModel(SMALL_FLUX)
    dense.load_state_dict(tw["values"])
    dense.lora_add("a", PACKED, np.ones((2, 256), np.float32), np.ones((256, 2), np.float32))
    assert dense.lib.fmi_flux_set_linear_f8(dense.h, PACKED.encode(), 1, rp, 1.0, 256, 256) == L.ERR_STATE
    dense.lora_remove()
    dense.quantize_fp8()
    assert dense.lib.fmi_flux_set_linear_f8(dense.h, PACKED.encode(), 1, rp, 1.0, 256, 256) == L.ERR_STATE
    torch.cuda.synchronize()
    gm.close(), dense.close(), cn.close()


def test_plain_bf16_model_is_untouched(env, twins):
    """A model with no fp8 part: its flat state says that no matrix is quantised (so densify() has nothing to expand), and the dense-cache mode changes neither
    its bits nor its allocations (no scratch, no codes)."""
    d, tw = env["d"], twins["e4m3"]
    gm = d.FluxModel(SMALL_FLUX)
    gm.load_state_dict(tw["values"])
    blob = gm.state_export()
    nf = int.from_bytes(blob[4:8], "little")
    assert nf > 0 and all(blob[12 + 5 * i] == 0 for i in range(nf))  # (8 header bytes, 4 arena flags, then q_type + blocksize per fused matrix)
    sizes = []
    for mode in (-1, 0, 1):
        gm.set_quant_dense_cache(mode)
        fwd, den = run(env, gm, twins["inputs"])
        np.testing.assert_array_equal(fwd.view(np.uint32), tw["fwd"].view(np.uint32))
        np.testing.assert_array_equal(den.view(np.uint32), tw["den"].view(np.uint32))
        sizes.append(gm.size_in_bytes())
    assert sizes[0] == sizes[1] == sizes[2] == tw["dense_bytes"]
    gm.close()


# ---------------------------------------------------------------------------------------------------------------- front door
def spec_all_in_one(name, shape):
    """an all-fp8 BFL file: e4m3 2-D weights (linear2 scaled), e4m3 biases; the QkNorm scales stay bf16"""
    if len(shape) == 2:
        return ("e4m3", name.endswith("linear2.weight"))
    return ("e4m3", False) if name.endswith(".bias") else None


def test_pipeline_with_a_bfl_named_all_in_one_fp8_file(env, tmp_path):
    """ModelSource.ModelId(dir).override_transformer_file(file): the directory gives model_index.json, scheduler and VAE, the BFL-named all-in-one fp8 file the
    transformer alone; the image equals, value for value, the image of the same pipeline with the dequantised dense transformer."""
    torch, d = env["torch"], env["d"]
    from diffusion_rs_amd import loader
    from tests.test_gpu_pipeline import _write_diffusers_dir
    sd = {k: np.asarray(v, np.float32) for k, v in d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=5).items()}
    vsd = d.synth.vae_state_dict_numpy(SMALL_VAE, seed=5)
    tensors, bfl_values = F8.quantize_state_dict(diffusers_to_bfl(sd, SMALL_FLUX), spec_all_in_one)
    assert sum(1 for n in tensors if n.endswith(".scale_weight")) == SMALL_FLUX["num_single_layers"]
    back = {}  # the dense twin under diffusers names: the dequantised BFL tensors, split the way the writer fused them
    for name, a in bfl_values.items():
        for dname, ranges in loader.bfl_to_diffusers(name, a.shape[0], 256):
            back[dname] = np.concatenate([a[r0:r1] for r0, r1 in ranges])
    assert set(back) == set(sd)
    root = str(tmp_path / "base")
    _write_diffusers_dir(root, back, vsd)  # (its transformer/ holds the dense twin: bf16 values, exactly representable)
    extras = {"vae.decoder.conv_in.weight": torch.ones(2, 2, 3, 3, dtype=torch.bfloat16), "text_encoders.clip_l.logit_scale": torch.tensor(4.6),
              "text_encoders.t5xxl.transformer.shared.weight": torch.zeros(4, 8, dtype=torch.float8_e4m3fn)}
    f = str(tmp_path / "flux-small-fp8-all-in-one.safetensors")
    F8.write_safetensors(f, dict({"model.diffusion_model." + n: t for n, t in tensors.items()}, **extras))
    params = d.DiffusionGenerationParams(height=64, width=64, num_steps=3, guidance_scale=3.5)
    rng = np.random.default_rng(3)
    t5 = bf16_round(rng.standard_normal((1, 8, 128)).astype(np.float32))
    clip = rng.standard_normal((1, 64)).astype(np.float32)
    lat = rng.standard_normal((1, 16, 8, 8)).astype(np.float32)
    images, stats = [], []
    for src in (d.ModelSource.ModelId(root).override_transformer_file(f), d.ModelSource.ModelId(root),
                d.ModelSource.ModelId(root).override_transformer_model_id(f), d.ModelSource.ModelId(root).override_transformer_file(f, expand=True)):
        pipe = d.Pipeline(src)
        images.append(pipe.forward(["a"], params, embeddings=(dev(t5, torch.bfloat16), dev(clip)), latents=dev(lat), output="tensor").cpu().numpy())
        stats.append(pipe.load_stats)
        del pipe
    for other in images[1:]:
        np.testing.assert_array_equal(images[0], other)
    assert images[0].shape == (1, 3, 64, 64) and images[0].std() > 0
    n2d = sum(1 for s in d.synth.flux_tensor_shapes(SMALL_FLUX).values() if len(s) == 2)
    for st in (stats[0], stats[2], stats[3]):
        assert st["f8"] == n2d and st["formats"] == {"e4m3": n2d} and st["dense"] > 0 and sorted(st["skipped"]) == sorted(extras)
