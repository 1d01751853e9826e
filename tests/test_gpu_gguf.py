"""GGUF transformers on the GPU: the block dequantisation kernels bit for bit against the NumPy restatement of the reference's
to_float (tests/gguf_ref.py), fmi_flux_set_linear_gguf against a dense model loaded with the dequantised weights, and the front door."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import gguf_ref as G
from tests.test_host_gguf import kat_blocks
from tests.util import SMALL_FLUX, SMALL_VAE, bf16_round, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    from diffusion_rs_amd import _lib as L
    return dict(torch=torch, d=d, L=L, lib=L.load())


def gpu_dequant(env, t, raw, out_dtype, offset_blocks=0):
    """raw (uint8 array) on the device — `offset_blocks` filler blocks in front, so the first block's address is only as aligned as the block size — through
    fmi_gguf_dequantize; returns the output's bits (uint16 for bf16, uint32 for f32).  The tensor ends with the allocation's last byte."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    be, bb = G.BLOCK[t]
    n = raw.size // bb * be
    buf = torch.from_numpy(np.concatenate([np.full(offset_blocks * bb, 0xFF, np.uint8), raw])).cuda()
    out = torch.empty(n, dtype=torch.bfloat16 if out_dtype == "bf16" else torch.float32, device="cuda")
    L.check(lib.fmi_gguf_dequantize(t, C.c_void_p(buf.data_ptr() + offset_blocks * bb), n, C.c_void_p(out.data_ptr()), L.BF16 if out_dtype == "bf16" else L.F32,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.view(torch.int16).cpu().numpy().view(np.uint16) if out_dtype == "bf16" else out.cpu().numpy().view(np.uint32)


def ref_bits(t, raw, out_dtype):
    y = G.dequantize_f32(t, raw)
    return G.bf16_bits(y) if out_dtype == "bf16" else y.view(np.uint32)


@pytest.fixture(scope="module")
def random_blocks():
    """130 x 512 weights of RANDOM block bytes per format (the reference computed once): every bit is free — the K formats' high scale bits, negative
    Q6_K scales, subnormal f16 scales — except that an f16 scale with an all-ones exponent is made finite."""
    out = {}
    for t in G.TYPES:
        be, bb = G.BLOCK[t]
        raw = G.sanitize(t, np.random.default_rng(100 + t).integers(0, 256, 130 * 512 // be * bb, dtype=np.uint8))
        out[t] = (raw, G.dequantize_f32(t, raw))
    return out


@pytest.mark.parametrize("out_dtype", ["bf16", "f32"])
@pytest.mark.parametrize("t", G.TYPES, ids=lambda t: G.NAMES[t])
def test_dequantize_bit_equal(env, random_blocks, t, out_dtype):
    be, bb = G.BLOCK[t]
    kat = np.frombuffer(kat_blocks()[t][0], np.uint8)
    np.testing.assert_array_equal(gpu_dequant(env, t, kat, out_dtype), ref_bits(t, kat, out_dtype))  # the literal known answer
    if out_dtype == "f32":
        np.testing.assert_array_equal(gpu_dequant(env, t, kat, "f32").view(np.float32), np.array(kat_blocks()[t][1], np.float32))
    raw, y = random_blocks[t]
    want = G.bf16_bits(y) if out_dtype == "bf16" else y.view(np.uint32)
    assert np.isfinite(y).all()
    for nblk in (1, 3):
        np.testing.assert_array_equal(gpu_dequant(env, t, raw[:nblk * bb], out_dtype), want[:nblk * be])
    np.testing.assert_array_equal(gpu_dequant(env, t, raw, out_dtype), want)                   # 130 x 512: 9 workgroups, the last one partial
    np.testing.assert_array_equal(gpu_dequant(env, t, raw, out_dtype, offset_blocks=1), want)  # first block at base + one block: 2-byte alignment


def test_dequantize_past_2_to_31_weights(env):
    """Element and byte offsets are 64-bit: 2^26 + 3 Q4_0 blocks (2^31 + 96 weights, 1.2 GB in, 4.3 GB out; the last workgroup holds 3 blocks) whose bytes
    repeat with a period of 7 random blocks, so the expected output is the reference of those 7 blocks repeated — compared on the device."""
    torch, L, lib = env["torch"], env["L"], env["lib"]
    t, (be, bb) = G.Q4_0, G.BLOCK[G.Q4_0]
    nblk, period = (1 << 26) + 3, 7
    pat = G.sanitize(t, np.random.default_rng(7).integers(0, 256, period * bb, dtype=np.uint8))
    want = torch.from_numpy(G.bf16_bits(G.dequantize_f32(t, pat)).view(np.int16)).cuda()
    buf = torch.from_numpy(pat).cuda().repeat(nblk // period)
    n = nblk * be
    assert n > (1 << 31)
    out = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    L.check(lib.fmi_gguf_dequantize(t, C.c_void_p(buf.data_ptr()), n, C.c_void_p(out.data_ptr()), L.BF16, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = out.view(torch.int16)
    assert nblk % period == 0  # (2^26 + 3 = 7 * 9586981)
    assert bool((got.view(-1, period * be) == want).all())


def test_block_info_and_refusals(env):
    L, lib, torch = env["L"], env["lib"], env["torch"]
    e, b = C.c_int(), C.c_int()
    for t in G.TYPES:
        assert lib.fmi_gguf_block_info(t, C.byref(e), C.byref(b)) == 0 and (e.value, b.value) == G.BLOCK[t]
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    out = torch.zeros(1024, dtype=torch.float32, device="cuda")
    p, o = C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr())
    for t, name in ((10, b"Q2_K"), (11, b"Q3_K"), (9, b"Q8_1"), (15, b"Q8_K"), (19, b"IQ1_S")):
        assert lib.fmi_gguf_block_info(t, None, None) == L.ERR_UNSUPPORTED and name in lib.fmi_last_error()
        assert lib.fmi_gguf_dequantize(t, p, 256, o, L.F32, None) == L.ERR_UNSUPPORTED
    assert lib.fmi_gguf_dequantize(G.Q4_K, p, 128, o, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_gguf_dequantize(G.Q8_0, p, 48, o, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_gguf_dequantize(G.Q8_0, p, 32, o, L.F16, None) == L.ERR_INVALID
    assert lib.fmi_gguf_dequantize(G.Q8_0, C.c_void_p(buf.data_ptr() + 1), 32, o, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_gguf_dequantize(G.Q8_0, None, 32, o, L.F32, None) == L.ERR_INVALID
    assert lib.fmi_gguf_dequantize(G.Q8_0, p, 0, o, L.F32, None) == 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # no refused call wrote anything


# ---------------------------------------------------------------------------------------------------------------- the model
def _small(shape):
    """the narrow embedders (K = 64 / 128 / 256-wide rows that are no multiple of 256) take a 32-element format, as in real files"""
    return shape[1] % 256 != 0


def spec_q8_0(name, shape):
    return G.Q8_0 if len(shape) == 2 else G.F32


def spec_q4k_q6k(name, shape):
    if len(shape) != 2:
        return G.F32
    if _small(shape):
        return G.Q5_1 if shape[1] == 128 else G.Q4_0
    return G.Q6_K if name.endswith("single_transformer_blocks.0.proj_out.weight") or name.endswith("single_transformer_blocks.1.proj_out.weight") else G.Q4_K


def spec_mixed(name, shape):
    """to_q Q4_K, to_k / to_v Q5_K: two types inside one fused [q|k|v] matrix, which the mixed rule expands into the dense arena at finalize()"""
    if len(shape) != 2:
        return G.F32
    if name.endswith("attn.to_q.weight"):
        return G.Q4_K
    if name.endswith("attn.to_k.weight") or name.endswith("attn.to_v.weight"):
        return G.Q5_K
    return G.F16 if _small(shape) else G.Q5_0


SPECS = {"q8_0": spec_q8_0, "q4k_q6k": spec_q4k_q6k, "mixed": spec_mixed}
T3 = [1.0, 0.75, 0.4, 0.0]


def feed(gm, tensors):
    for name, t, shape, raw in tensors:
        if t in (G.F32, G.F16, G.BF16):
            a = np.frombuffer(raw, {G.F32: np.float32, G.F16: np.float16}[t]).reshape(shape)
            gm.set_tensor(name, a)
        else:
            gm.set_linear_gguf(name[:-len(".weight")], t, np.frombuffer(raw, np.uint8), shape[0], shape[1])
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
    """per spec: the file's tensors, the dense twin's weights (gguf_ref's bf16 values), the twin's forward / 3-step denoise, and the oracle's on the same
    weights — computed once"""
    d = env["d"]
    from oracle import oracle as orc
    sd = {k: np.asarray(v, np.float32) for k, v in d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=11).items()}
    inputs = flux_inputs(SMALL_FLUX, 1, (4, 4), 8)
    out = {"inputs": inputs}
    for key, spec in SPECS.items():
        tensors, values = G.quantize_state_dict(sd, spec)
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
def test_set_linear_gguf_is_the_dense_model_of_the_dequantised_weights(env, twins, key):
    """forward and a 3-step denoise, bit-identical to the dense twin in dense-cache modes 0, 3 and 1 (2 runs as 0): same operands, same kernels — and
    within test_gpu_flux.py's tolerances of the oracle on those weights (1e-2 one evaluation, 3e-2 the loop)."""
    d, tw = env["d"], twins[key]
    gm = d.FluxModel(SMALL_FLUX)
    feed(gm, tw["tensors"])
    assert sum(1 for _, t, _, _ in tw["tensors"] if t in G.TYPES) >= 30
    for mode in (0, 3, 1, 2):
        gm.set_quant_dense_cache(mode)
        fwd, den = run(env, gm, twins["inputs"])
        np.testing.assert_array_equal(fwd.view(np.uint32), tw["fwd"].view(np.uint32), err_msg=f"forward, mode {mode}")
        np.testing.assert_array_equal(den.view(np.uint32), tw["den"].view(np.uint32), err_msg=f"denoise, mode {mode}")
    e1, e3 = rel_l2(tw["fwd"], tw["ofwd"]), rel_l2(tw["den"], tw["oden"])
    print(f"{key}: forward rel-L2 vs oracle {e1:.3e}, 3-step denoise {e3:.3e}")
    assert e1 <= 1e-2 and e3 <= 3e-2
    gm.close()


def test_size_in_bytes_counts_the_blocks(env, twins):
    d, tw = env["d"], twins["q8_0"]
    want = d.synth.flux_tensor_shapes(SMALL_FLUX)
    gm = d.FluxModel(SMALL_FLUX)
    gm.set_quant_dense_cache(0)
    feed(gm, tw["tensors"])
    # a model holding everything BUT the block linears: the BASE and modulation arenas, which a GGUF model holds dense too
    part = d.FluxModel(SMALL_FLUX)
    for name in want:
        if not d.synth.is_block_linear(name):
            part.set_tensor(name, tw["values"][name])
    file_bytes = sum(len(raw) for name, t, _, raw in tw["tensors"] if d.synth.is_block_linear(name))
    assert file_bytes == sum(s[0] * s[1] // 32 * 34 for n, s in want.items() if d.synth.is_block_linear(n))
    assert gm.size_in_bytes() - part.size_in_bytes() == file_bytes
    run(env, gm, twins["inputs"])
    packed_only = gm.size_in_bytes()
    assert packed_only < tw["dense_bytes"]  # (the same evaluations: the same workspace; the scratch included)
    gm.set_quant_dense_cache(1)
    run(env, gm, twins["inputs"])
    assert gm.size_in_bytes() > packed_only
    gm.close(), part.close()


def test_refusals_and_fallbacks(env, twins, monkeypatch):
    d, L, torch = env["d"], env["L"], env["torch"]
    tw = twins["q8_0"]
    gm = d.FluxModel(SMALL_FLUX)
    feed(gm, tw["tensors"])
    run(env, gm, twins["inputs"])
    packed = "transformer_blocks.0.attn.to_q"
    with pytest.raises(L.FmiError) as ei:
        gm.get_tensor(packed + ".weight")
    assert ei.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.FmiError) as ei:
        gm.lora_add("a", packed, np.zeros((2, 256), np.float32), np.zeros((256, 2), np.float32))
    assert ei.value.code == L.ERR_UNSUPPORTED
    # embedders and modulation linears were expanded at load: they read back as the dequantised values
    for name in ("context_embedder.weight", "transformer_blocks.1.norm1.linear.weight", "norm_out.linear.weight"):
        np.testing.assert_array_equal(host(gm.get_tensor(name)), tw["values"][name])
    for call in (gm.quantize_fp8, gm.quantize_int8, gm.calibrate_int8):  # as on an nf4 model
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
    raw = np.zeros(256 * 256 // 32 * 34, np.uint8)
    for args, code in (((b"transformer_blocks.0.attn.nope", G.Q8_0, 256, 256), L.ERR_INVALID), ((packed.encode(), G.Q8_0, 256, 512), L.ERR_INVALID),
                       ((packed.encode(), G.Q4_K, 256, 256 + 32), L.ERR_INVALID), ((packed.encode(), 10, 256, 256), L.ERR_UNSUPPORTED)):
        rc = gm.lib.fmi_flux_set_linear_gguf(gm.h, args[0], args[1], C.c_void_p(raw.ctypes.data), args[2], args[3])
        assert rc == code, (args, rc)
    with pytest.raises(L.FmiError) as ei:
        gm.set_linear_gguf("context_embedder", G.Q8_0, raw[:100], 256, 128)  # too few bytes for the shape
    assert ei.value.code == L.ERR_INVALID
    from tests import controlnet_ref as CR
    cn = d.FluxControlNetModel(CR.net_cfg("2+0"))
    assert cn.lib.fmi_flux_set_linear_gguf(cn.h, packed.encode(), G.Q8_0, C.c_void_p(raw.ctypes.data), 256, 256) == L.ERR_UNSUPPORTED
    # a weight with LoRA adapters merged, and a model in an 8-bit mode, as fmi_flux_set_linear_bnb4
    dense = d.FluxModel(SMALL_FLUX)
    dense.load_state_dict(tw["values"])
    dense.lora_add("a", packed, np.ones((2, 256), np.float32), np.ones((256, 2), np.float32))
    assert dense.lib.fmi_flux_set_linear_gguf(dense.h, packed.encode(), G.Q8_0, C.c_void_p(raw.ctypes.data), 256, 256) == L.ERR_STATE
    dense.lora_remove()
    dense.quantize_fp8()
    assert dense.lib.fmi_flux_set_linear_gguf(dense.h, packed.encode(), G.Q8_0, C.c_void_p(raw.ctypes.data), 256, 256) == L.ERR_STATE
    torch.cuda.synchronize()
    gm.close(), dense.close()


def test_plain_bf16_model_is_untouched(env, twins):
    """A model with no GGUF part: its flat state says that no matrix is quantised (so densify() has nothing to expand), the dense-cache mode changes
    neither its bits nor its allocations (no scratch, no blocks), and it computes what it did for the twins fixture."""
    d, tw = env["d"], twins["q8_0"]
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
def test_pipeline_with_a_bfl_named_gguf_transformer(env, tmp_path):
    """ModelSource.ModelId(dir).override_transformer_gguf(file): the directory gives model_index.json, scheduler and VAE, the BFL-named .gguf the
    transformer; the u8 image equals, value for value, the image of the same pipeline with the dequantised dense transformer."""
    torch, d = env["torch"], env["d"]
    from tests.test_gpu_pipeline import _write_diffusers_dir
    sd = {k: np.asarray(v, np.float32) for k, v in d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=5).items()}
    vsd = d.synth.vae_state_dict_numpy(SMALL_VAE, seed=5)
    bfl = G.diffusers_to_bfl(sd, SMALL_FLUX)
    tensors, bfl_values = G.quantize_state_dict(bfl, spec_q4k_q6k_bfl)
    # the dense twin under diffusers names: the dequantised BFL tensors, split the way the writer fused them
    _, values = G.quantize_state_dict(sd, lambda n, s: G.F32)
    back = {}
    from diffusion_rs_amd import loader
    for name, a in bfl_values.items():
        for dname, ranges in loader.bfl_to_diffusers(name, a.shape[0], 256):
            back[dname] = np.concatenate([a[r0:r1] for r0, r1 in ranges])
    assert set(back) == set(sd)
    root = str(tmp_path / "base")
    _write_diffusers_dir(root, back, vsd)  # (its transformer/ holds the dense twin: bf16 values, exactly representable)
    f = str(tmp_path / "flux-small-Q4_K.gguf")
    G.write_gguf(f, [("model.diffusion_model." + n, t, s, raw) for n, t, s, raw in tensors], [("general.architecture", "str", "flux")])
    params = d.DiffusionGenerationParams(height=64, width=64, num_steps=3, guidance_scale=3.5)
    rng = np.random.default_rng(3)
    t5 = bf16_round(rng.standard_normal((1, 8, 128)).astype(np.float32))
    clip = rng.standard_normal((1, 64)).astype(np.float32)
    lat = rng.standard_normal((1, 16, 8, 8)).astype(np.float32)
    images = []
    for src in (d.ModelSource.ModelId(root).override_transformer_gguf(f), d.ModelSource.ModelId(root)):
        pipe = d.Pipeline(src)
        images.append(pipe.forward(["a"], params, embeddings=(dev(t5, torch.bfloat16), dev(clip)), latents=dev(lat), output="tensor").cpu().numpy())
        stats = pipe.load_stats
        del pipe
    np.testing.assert_array_equal(images[0], images[1])
    assert images[0].shape == (1, 3, 64, 64) and images[0].std() > 0
    gpipe = d.Pipeline(d.ModelSource.ModelId(root).override_transformer_model_id(f))  # a transformer id ending in .gguf is the same
    assert gpipe.load_stats["gguf"] > 0 and set(gpipe.load_stats["types"]) >= {"Q4_K", "Q6_K"} and stats["dense"] > 0
    # a base directory whose transformer/config.json disagrees with the file names the field
    cfgp = os.path.join(root, "transformer", "config.json")
    json.dump(dict(json.load(open(cfgp)), num_single_layers=5), open(cfgp, "w"))
    with pytest.raises(ValueError, match="num_single_layers"):
        d.Pipeline(d.ModelSource.ModelId(root).override_transformer_gguf(f))


def spec_q4k_q6k_bfl(name, shape):
    if len(shape) != 2:
        return G.F32 if name.endswith(".scale") else G.F16
    if shape[1] % 256:
        return G.Q5_1 if shape[1] == 128 else G.Q4_0
    return G.Q6_K if name.endswith("linear2.weight") else G.Q4_K
