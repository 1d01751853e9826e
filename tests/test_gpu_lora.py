"""LoRA adapters merged into the resident bf16 weights (fmi_flux_lora_* / fmi_flux_get_tensor, csrc/lora.hip) on tests.util.SMALL_FLUX
(D = 256, M = 1024).  The contract (include/flux_mi355x.h): W = bf16_rne(W0 + sum_a weight_a scale_a (B_a A_a)), adapters in name order, exact f32
operands, f64 products and sums, one rounding — always recomputed from a pristine copy of W0, so unloading is exact and nothing depends on the history of calls.

Tolerances.  Merge: against target = W0 + sum w s B A in float64, every element within 2^-7 |target| (bf16 keeps 8 significant bits: that is one of the
two neighbouring bf16 values) and at least 99.9 % equal to bf16_rne(target) (an f32-accumulated sum rounds differently from the float64 one only when
target sits within ~1e-7 relative of a rounding boundary: measured with numpy at <= 8e-5 of the elements at these magnitudes and ranks; the kernel
accumulates in f64 and rounds once, so it measures 0 — and it needs f64 for the first bound: an f32 emulation leaves 5 elements, where W0 and the update
cancel, outside it — a figure from that numpy emulation, not from a run of an f32 kernel).  Model parity:
the bars of tests/test_gpu_flux.py (1e-2 one evaluation, 3e-2 after 4 Euler steps) and of tests/test_gpu_int8.py (1e-2 against the int8 oracle)."""
import ctypes as C

import numpy as np
import pytest

from tests.lora_util import peft_and_kohya, write_safetensors
from tests.util import SMALL_FLUX, SMALL_VAE, bf16_round, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu

D = 256
INVALID, STATE, UNSUPPORTED = -1, -3, -4


@pytest.fixture(scope="module")
def env():
    import torch
    import diffusion_rs_amd as d
    from oracle import oracle as orc
    sd = d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, 1, (8, 8), 32, seed=11)
    t, g = np.array([0.8], np.float32), np.array([3.5], np.float32)
    fwd = (dev(img), dev(ids), dev(txt, torch.bfloat16), dev(txt_ids), dev(t), dev(y), dev(g))
    e = dict(torch=torch, d=d, orc=orc, sd=sd, inputs=(img, ids, txt, txt_ids, y, t, g), fwd=fwd)
    base = fresh(e)
    e["base_bits"] = snapshot(base)
    e["base_out"] = host(base.forward(*fwd))
    e["base_size"] = base.size_in_bytes()
    return e


def fresh(env):
    m = env["d"].FluxModel(SMALL_FLUX)
    m.load_state_dict(env["sd"])
    return m


def snapshot(m, skip=()):
    """{name: the resident bf16 bits} of every tensor of the model."""
    torch = __import__("torch")
    return {n: m.get_tensor(n).view(torch.int16).cpu().numpy() for n in m._shapes() if n not in skip}


def assert_bits(got, want, names=None):
    for n in (names if names is not None else want):
        np.testing.assert_array_equal(got[n], want[n], err_msg=n)


def bf16_rne64(x):
    """float64 -> the nearest bf16 value (ties to even), in ONE rounding (tests.util.bf16_round would round to f32 first); as float64."""
    x = np.asarray(x, np.float64)
    q = np.ldexp(1.0, np.frexp(x)[1] - 8)  # |x| = m 2^e, m in [0.5, 1): 8 significant bits -> a grid of 2^(e - 8)
    return np.rint(x / q) * q


def make_adapter(seed, shapes, ranks, std, scale=1.0, f16=False):
    """{prefix: (A, B, scale)}: A (r, in), B (out, r) ~ N(0, std^2), bf16-rounded: exact as F32 and BF16; f16: also rounded through float16 (whose
    subnormal range the smallest values fall into), so exact as F16 as well."""
    rng = np.random.default_rng(seed)

    def values(shape):
        v = bf16_round(std * rng.standard_normal(shape))
        return v.astype(np.float16).astype(np.float32) if f16 else v

    out = {}
    for prefix, r in ranks.items():
        o, i = shapes[prefix + ".weight"]
        out[prefix] = (values((r, i)), values((o, r)), scale)
    return out


def add_adapter(m, name, pairs, to=None):
    torch = __import__("torch")
    for prefix, (A, B, s) in pairs.items():
        if to is None:
            m.lora_add(name, prefix, A, B, s)
        else:  # as device tensors of another dtype (make_adapter: the values are exact in it)
            assert np.array_equal(torch.from_numpy(A).to(to).float().numpy(), A) and np.array_equal(torch.from_numpy(B).to(to).float().numpy(), B)
            m.lora_add(name, prefix, torch.from_numpy(A).to(to).cuda(), torch.from_numpy(B).to(to).cuda(), s)


def target64(env, prefix, terms):
    """f32(W0) + sum w s B A in float64; terms = [(weight, pairs)] in adapter-name order (w and s as the f32 values that cross the C-ABI)."""
    w = bf16_round(env["sd"][prefix + ".weight"]).astype(np.float64)
    for weight, pairs in terms:
        if prefix in pairs:
            A, B, s = pairs[prefix]
            w = w + np.float64(np.float32(weight)) * np.float64(np.float32(s)) * (B.astype(np.float64) @ A.astype(np.float64))
    return w


TARGETS = ["x_embedder", "context_embedder", "transformer_blocks.0.attn.to_k", "transformer_blocks.1.norm1.linear", "transformer_blocks.0.ff.net.2",
           "single_transformer_blocks.1.proj_mlp", "single_transformer_blocks.0.proj_out", "proj_out"]
RANKS_A = dict(zip(TARGETS, [1, 3, 16, 17, 64, 64, 17, 3]))
RANKS_B = dict(zip(TARGETS, [3, 1, 17, 16, 64, 1, 64, 16]))


@pytest.fixture(scope="module")
def stacked(env):
    """Two stacked adapters, weights 0.7 and 1.2, on the eight target Linears (one model shared by the merge and the unload tests)."""
    torch = env["torch"]
    m = fresh(env)
    shapes = m._shapes()
    a = make_adapter(1, shapes, RANKS_A, 0.05, scale=1.0)
    b = make_adapter(2, shapes, RANKS_B, 0.05, scale=0.5, f16=True)
    add_adapter(m, "a", a, to=torch.bfloat16)
    add_adapter(m, "b", b, to=torch.float16)
    m.lora_set_weight("a", 0.7)
    m.lora_set_weight("b", 1.2)
    return dict(m=m, a=a, b=b)


def test_get_tensor_reads_back_what_was_loaded(env):
    """Every tensor, de-fused from its row range: the bf16 rounding of the loaded values, as bf16 bits and as f32."""
    torch = env["torch"]
    m = fresh(env)
    for n, w in env["sd"].items():
        want = bf16_round(w)
        np.testing.assert_array_equal(env["base_bits"][n].view(np.uint16), (want.view(np.uint32) >> 16).astype(np.uint16), err_msg=n)
    for n in ("transformer_blocks.1.attn.to_v.weight", "single_transformer_blocks.1.proj_mlp.bias", "transformer_blocks.0.attn.norm_k.weight"):
        np.testing.assert_array_equal(host(m.get_tensor(n, torch.float32)), bf16_round(env["sd"][n]))
    with pytest.raises(env["d"].FmiError) as ei:
        m.get_tensor("x_embedder.weight", torch.float16)
    assert ei.value.code == INVALID


def test_merge_is_exact(env, stacked):
    torch = env["torch"]
    m, a, b = stacked["m"], stacked["a"], stacked["b"]
    assert m.loras() == ["a", "b"]
    bits = snapshot(m)
    worst_off, worst_far = 0.0, 0.0
    for prefix in TARGETS:
        tgt = target64(env, prefix, [(0.7, a), (1.2, b)])
        got = host(m.get_tensor(prefix + ".weight", torch.float32)).astype(np.float64)
        far = float(np.max(np.abs(got - tgt) / np.maximum(np.abs(tgt), 1e-30)))
        off = float(np.mean(got != bf16_rne64(tgt)))
        print(f"merge {prefix}: ranks {RANKS_A[prefix]} + {RANKS_B[prefix]}, max |got - target| / |target| = {far:.3e}, not bf16_rne(target): {off:.2e} of the elements")
        worst_far, worst_off = max(worst_far, far), max(worst_off, off)
        assert not np.array_equal(bits[prefix + ".weight"], env["base_bits"][prefix + ".weight"])
        assert far <= 2.0 ** -7, prefix
        assert off <= 1e-3, prefix
    # every tensor that was not targeted — to_q and to_v next to to_k, the other rows of the modulation matrix, every bias — holds the loaded bits
    untouched = [n for n in bits if n not in {p + ".weight" for p in TARGETS}]
    assert "transformer_blocks.0.attn.to_q.weight" in untouched and "transformer_blocks.0.attn.to_v.weight" in untouched
    assert "transformer_blocks.1.norm1_context.linear.weight" in untouched and "transformer_blocks.0.attn.to_k.bias" in untouched
    assert_bits(bits, env["base_bits"], untouched)


def test_unload_is_exact(env, stacked):
    m = stacked["m"]
    merged = snapshot(m)
    out = host(m.forward(*env["fwd"]))
    assert not np.array_equal(out, env["base_out"])
    # weight 0 on every adapter: the loaded weights, bit for bit (the adapters stay listed)
    m.lora_set_weight("a", 0.0)
    m.lora_set_weight("b", 0.0)
    assert m.loras() == ["a", "b"]
    assert_bits(snapshot(m), env["base_bits"])
    np.testing.assert_array_equal(host(m.forward(*env["fwd"])), env["base_out"])
    # back on: the same merged bits as before (nothing depends on the detour)
    m.lora_set_weight("b", 1.2)
    m.lora_set_weight("a", 0.7)
    assert_bits(snapshot(m), merged)
    np.testing.assert_array_equal(host(m.forward(*env["fwd"])), out)
    # one adapter removed by name: its Linears follow the other adapter alone
    m.lora_remove("a")
    assert m.loras() == ["b"]
    only_b = fresh(env)
    add_adapter(only_b, "b", stacked["b"])
    only_b.lora_set_weight("b", 1.2)
    assert_bits(snapshot(m), snapshot(only_b))
    # all removed
    m.lora_remove(None)
    assert m.loras() == []
    assert_bits(snapshot(m), env["base_bits"])
    np.testing.assert_array_equal(host(m.forward(*env["fwd"])), env["base_out"])
    assert m.size_in_bytes() == env["base_size"]  # factors and pristine copies are released
    m.lora_remove(None)  # nothing loaded: a no-op
    # and the model is as usable as before: the adapters go in again and give the merged bits again
    add_adapter(m, "b", stacked["b"])
    add_adapter(m, "a", stacked["a"])
    m.lora_set_weight("a", 0.7)
    m.lora_set_weight("b", 1.2)
    assert_bits(snapshot(m), merged)


def test_history_independence(env):
    shapes = fresh(env)._shapes()
    names = ["transformer_blocks.0.attn.to_k", "transformer_blocks.1.ff.net.0.proj", "single_transformer_blocks.0.attn.to_q",
             "single_transformer_blocks.0.proj_mlp", "transformer_blocks.0.norm1.linear", "context_embedder"]
    a = make_adapter(3, shapes, dict(zip(names[:5], [16, 3, 17, 1, 4])), 0.05, scale=2.0)
    b = make_adapter(4, shapes, dict(zip(names[1:], [5, 16, 2, 17, 3])), 0.05, scale=0.25)
    results = []
    for order in ("ab", "ba", "ab-a+a", "fresh"):
        m = fresh(env)
        if order == "ba":
            add_adapter(m, "b", b)
            m.lora_set_weight("b", 1.3)
            add_adapter(m, "a", a)
        else:
            add_adapter(m, "a", a)
            add_adapter(m, "b", b)
            m.lora_set_weight("b", 1.3)
        if order == "ab-a+a":
            m.lora_remove("a")
            add_adapter(m, "a", a)
        if order == "fresh":  # (pairs arriving in another order, too)
            m = fresh(env)
            add_adapter(m, "b", dict(reversed(list(b.items()))))
            add_adapter(m, "a", dict(reversed(list(a.items()))))
            m.lora_set_weight("b", 1.3)
        assert m.loras() == ["a", "b"]
        results.append((snapshot(m), host(m.forward(*env["fwd"]))))
    assert not np.array_equal(results[0][1], env["base_out"])
    for bits, out in results[1:]:
        assert_bits(bits, results[0][0])
        np.testing.assert_array_equal(out, results[0][1])
    # the summation order is the NAME order, not the call order: the same factors under swapped names are another sum only where both meet — and
    # re-adding a pair replaces it
    m = fresh(env)
    add_adapter(m, "a", a)
    add_adapter(m, "a", {names[1]: b[names[1]]})  # replaces a's pair on names[1]
    only = fresh(env)
    add_adapter(only, "a", dict(a, **{names[1]: b[names[1]]}))
    assert_bits(snapshot(m), snapshot(only))
    # switching a -> b equals a fresh model with b only
    sw = fresh(env)
    add_adapter(sw, "a", a)
    sw.lora_remove("a")
    add_adapter(sw, "b", b)
    fb = fresh(env)
    add_adapter(fb, "b", b)
    assert_bits(snapshot(sw), snapshot(fb))
    np.testing.assert_array_equal(host(sw.forward(*env["fwd"])), host(fb.forward(*env["fwd"])))


@pytest.fixture(scope="module")
def block_adapter(env):
    """One adapter on all 34 block Linears (rank 16, scale 1, N(0, 0.1^2) bf16-rounded, seed 5) and the oracle loaded with bf16_rne(target)."""
    sd = env["sd"]
    names = [n[:-len(".weight")] for n, w in sd.items() if "transformer_blocks." in n and n.endswith(".weight") and w.ndim == 2 and "norm" not in n]
    assert len(names) == 34
    shapes = {n: tuple(w.shape) for n, w in sd.items()}
    pairs = make_adapter(5, shapes, {n: 16 for n in names}, 0.1, scale=1.0)
    merged = dict(sd)
    for n in names:
        merged[n + ".weight"] = bf16_rne64(target64(env, n, [(1.0, pairs)])).astype(np.float32)
    om = env["orc"].Flux(SMALL_FLUX)
    om.load(merged)
    return dict(pairs=pairs, om=om, names=names)


def test_parity_through_the_model(env, block_adapter):
    torch, d = env["torch"], env["d"]
    img, ids, txt, txt_ids, y, t, g = env["inputs"]
    om = block_adapter["om"]
    ob = env["orc"].Flux(SMALL_FLUX)
    ob.load(env["sd"])
    ref = om.forward(img, ids, txt, txt_ids, t, y, g)
    moved = rel_l2(ref, ob.forward(img, ids, txt, txt_ids, t, y, g))
    m = fresh(env)
    add_adapter(m, "style", block_adapter["pairs"])
    got = host(m.forward(*env["fwd"]))
    err = rel_l2(got, ref)
    print(f"LoRA on 34 block linears: the oracle's output moves by {moved:.3e}; GPU forward vs adapted oracle rel-L2 {err:.3e}")
    assert moved >= 1e-1  # otherwise the comparison below shows nothing
    assert np.isfinite(got).all() and err <= 1e-2
    sched = d.SchedulerConfig()
    ts = sched.get_timesteps(4, sched.calculate_shift(64))
    ref4 = om.denoise(img, ids, txt, txt_ids, y, g, ts)
    got4 = host(m.denoise(dev(img), dev(ids), dev(txt, torch.bfloat16), dev(txt_ids), dev(y), dev(g), ts))
    err4 = rel_l2(got4, ref4)
    print(f"LoRA 4-step denoise: rel-L2 {err4:.3e}")
    assert err4 <= 3e-2


def test_quantize_int8_after_lora_quantises_the_merged_weights(env, block_adapter):
    img, ids, txt, txt_ids, y, t, g = env["inputs"]
    m = fresh(env)
    add_adapter(m, "style", block_adapter["pairs"])
    m.quantize_int8()
    got = host(m.forward(*env["fwd"]))
    om = block_adapter["om"]
    om.set_int8(True, 0x33, attention=True)  # (8, 8) / 32 tokens: aligned, so q and k of the attention are e4m3 as in the library
    try:
        ref8 = om.forward(img, ids, txt, txt_ids, t, y, g)
    finally:
        om.set_int8(False)
    e8 = rel_l2(got, ref8)
    print(f"int8 after LoRA: vs the int8 oracle on the merged weights {e8:.3e}")
    assert e8 <= 1e-2
    # the codes were taken from the merged weights: the adapter can no longer be changed
    for call in (lambda: m.lora_set_weight("style", 0.5), lambda: m.lora_remove("style"), lambda: m.lora_remove(None)):
        with pytest.raises(env["d"].FmiError) as ei:
            call()
        assert ei.value.code == STATE
    assert m.loras() == ["style"]
    plain = fresh(env)
    plain.quantize_int8()
    plain.forward(*env["fwd"])
    assert m.size_in_bytes() == plain.size_in_bytes()  # the factors and the pristine copies were released when the adapters froze


def expect_error(env, m, code, call, before, skip=(), from_library=True):
    lib = m.lib
    lib.fmi_flux_get_tensor(m.h, b"no such tensor", None, 0, None, 0)  # leaves ITS message: a stale one cannot pass for the call's own below
    stale = lib.fmi_last_error()
    with pytest.raises(env["d"].FmiError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    if from_library:  # (an error the Python layer raises before any C call has no fmi_last_error of its own)
        assert len(lib.fmi_last_error()) > 0 and lib.fmi_last_error() != stale
    assert_bits(snapshot(m, skip), before)


def test_errors_leave_the_model_untouched(env):
    torch, d, orc = env["torch"], env["d"], env["orc"]
    m = fresh(env)
    shapes = m._shapes()
    good = make_adapter(6, shapes, {"transformer_blocks.0.attn.to_k": 4, "x_embedder": 2}, 0.05)
    add_adapter(m, "a", good)
    before = snapshot(m)
    A, B, _ = good["transformer_blocks.0.attn.to_k"]
    Ad, Bd = dev(A), dev(B)

    def raw_add(adapter, prefix, rank, scale):
        rc = m.lib.fmi_flux_lora_add(m.h, adapter, prefix, C.c_void_p(Ad.data_ptr()), C.c_void_p(Bd.data_ptr()), 0, rank, scale)
        d._lib.check(rc, m.lib)

    expect_error(env, m, INVALID, lambda: raw_add(b"b", b"transformer_blocks.0.attn.to_x", 4, 1.0), before)             # unknown prefix
    expect_error(env, m, INVALID, lambda: raw_add(b"b", b"transformer_blocks.0.attn.to_k.bias", 4, 1.0), before)        # a bias name
    expect_error(env, m, INVALID, lambda: raw_add(b"b", b"transformer_blocks.0.attn.norm_k", 4, 1.0), before)           # a 1-D weight
    expect_error(env, m, INVALID, lambda: raw_add(b"b", b"transformer_blocks.0.attn.to_k", 0, 1.0), before)             # rank 0
    expect_error(env, m, INVALID, lambda: raw_add(b"b", b"transformer_blocks.0.attn.to_k", 4, float("nan")), before)    # NaN scale
    expect_error(env, m, INVALID, lambda: raw_add(b"b", b"transformer_blocks.0.attn.to_k", 4, float("inf")), before)
    expect_error(env, m, INVALID, lambda: d._lib.check(m.lib.fmi_flux_lora_add(m.h, b"b", b"x_embedder", None, C.c_void_p(Bd.data_ptr()), 0, 4, 1.0), m.lib), before)
    expect_error(env, m, INVALID, lambda: m.lora_add("b", "x_embedder", A, B), before, from_library=False)                                   # factors of another Linear
    expect_error(env, m, INVALID, lambda: m.lora_set_weight("nope", 1.0), before)                                       # unknown adapter
    expect_error(env, m, INVALID, lambda: m.lora_set_weight("a", float("nan")), before)
    expect_error(env, m, INVALID, lambda: m.lora_remove("nope"), before)
    assert m.loras() == ["a"]  # no failed call left an adapter "b" behind
    # set_tensor on an adapted weight: first remove the adapters
    w = env["sd"]["transformer_blocks.0.attn.to_k.weight"]
    with pytest.raises(d.FmiError, match="remove the adapters first") as ei:
        m.set_tensor("transformer_blocks.0.attn.to_k.weight", w)
    assert ei.value.code == STATE
    assert_bits(snapshot(m), before)
    packed, absmax = orc.quantize_blockwise_4bit(w.ravel(), 64, "nf4")
    expect_error(env, m, STATE, lambda: m.set_linear_bnb4("transformer_blocks.0.attn.to_k", packed, absmax, 64, "nf4", w.shape[0], w.shape[1]), before)
    wx = env["sd"]["x_embedder.weight"]
    expect_error(env, m, STATE, lambda: m.set_linear_int8("x_embedder", np.zeros(wx.shape, np.int8), np.ones(wx.shape[0], np.float32), wx.shape[0], wx.shape[1]), before)
    m.set_tensor("transformer_blocks.0.attn.to_q.weight", env["sd"]["transformer_blocks.0.attn.to_q.weight"])  # its neighbour has none: as ever
    m.set_tensor("transformer_blocks.0.attn.to_k.bias", env["sd"]["transformer_blocks.0.attn.to_k.bias"])      # biases are not adapted
    assert_bits(snapshot(m), before)
    m.lora_remove("a")
    m.set_tensor("transformer_blocks.0.attn.to_k.weight", w)
    assert_bits(snapshot(m), env["base_bits"])

    # tensors missing
    part = d.FluxModel(SMALL_FLUX)
    part.set_tensor("x_embedder.weight", env["sd"]["x_embedder.weight"])
    with pytest.raises(d.FmiError) as ei:
        part.lora_add("a", "x_embedder", *good["x_embedder"][:2])
    assert ei.value.code == STATE and part.loras() == []
    with pytest.raises(d.FmiError) as ei:
        part.get_tensor("x_embedder.bias")
    assert ei.value.code == STATE

    # add after quantize_int8
    q = fresh(env)
    q.quantize_int8()
    expect_error(env, q, STATE, lambda: q.lora_add("a", "transformer_blocks.0.attn.to_k", A, B), env["base_bits"])
    assert q.loras() == []

    # a Linear that is resident as nf4 codes (q | k | v of one stream all set through set_linear_bnb4: the fused matrix stays packed)
    n4 = d.FluxModel(SMALL_FLUX)
    packed_names = ["transformer_blocks.0.attn.to_q.weight", "transformer_blocks.0.attn.to_k.weight", "transformer_blocks.0.attn.to_v.weight"]
    for n, w in env["sd"].items():
        if n in packed_names:
            packed, absmax = orc.quantize_blockwise_4bit(w.ravel(), 64, "nf4")
            n4.set_linear_bnb4(n[:-len(".weight")], packed, absmax, 64, "nf4", w.shape[0], w.shape[1])
        else:
            n4.set_tensor(n, w)
    n4.assert_complete()
    rest = {n: v for n, v in env["base_bits"].items() if n not in packed_names}
    assert_bits(snapshot(n4, skip=packed_names), rest)
    expect_error(env, n4, UNSUPPORTED, lambda: n4.lora_add("a", "transformer_blocks.0.attn.to_k", A, B), rest, skip=packed_names)
    expect_error(env, n4, UNSUPPORTED, lambda: n4.get_tensor("transformer_blocks.0.attn.to_k.weight"), rest, skip=packed_names)
    assert n4.loras() == []
    n4.lora_add("a", "transformer_blocks.0.attn.add_k_proj", A, B)  # the dense Linears of the same model take adapters
    assert n4.loras() == ["a"]


@pytest.fixture(scope="module")
def adapter_files(tmp_path_factory):
    root = tmp_path_factory.mktemp("lora")
    peft, kohya, _ = peft_and_kohya(seed=9, std=0.1, rank=16)
    write_safetensors(root / "style_peft.safetensors", peft)
    write_safetensors(root / "style_kohya.safetensors", kohya)
    return str(root / "style_peft.safetensors"), str(root / "style_kohya.safetensors")


def test_pipeline_load_and_unload(env, adapter_files):
    torch, d = env["torch"], env["d"]
    peft_path, kohya_path = adapter_files
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=SMALL_FLUX, vae_cfg=SMALL_VAE))
    params = d.DiffusionGenerationParams(height=64, width=64, num_steps=2, guidance_scale=3.5)

    def image():
        return pipe.forward(["a lighthouse at dusk"], params, seed=3, output="tensor").cpu().numpy()

    base = image()
    assert pipe.load_lora(peft_path) == "style_peft" and pipe.loras() == ["style_peft"]
    with_peft = image()
    assert not np.array_equal(with_peft, base)
    with pytest.raises(ValueError):
        pipe.load_lora(peft_path)  # the name is taken
    pipe.unload_lora()
    assert pipe.loras() == []
    np.testing.assert_array_equal(image(), base)
    # the kohya / BFL file of the same adapter gives the same image
    assert pipe.load_lora(kohya_path, name="style") == "style"
    np.testing.assert_array_equal(image(), with_peft)
    pipe.set_lora_weight("style", 0.0)
    np.testing.assert_array_equal(image(), base)
    pipe.set_lora_weight("style", 0.5)
    half = image()
    assert not np.array_equal(half, base) and not np.array_equal(half, with_peft)
    pipe.unload_lora("style")
    # loaded at a weight == loaded, then reweighted
    pipe.load_lora(peft_path, name="style", weight=0.5)
    np.testing.assert_array_equal(image(), half)
    pipe.unload_lora("style")
    # a file with keys the library does not merge: refused as a whole, nothing is loaded; or loaded without them
    bad = dict(peft_and_kohya(seed=9, std=0.1, rank=16)[1])
    bad["lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_down.weight"] = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="lora_te1"):
        pipe.load_lora(bad, name="style")
    assert pipe.loras() == []
    pipe.load_lora(bad, name="style", skip_unsupported=True)
    np.testing.assert_array_equal(image(), with_peft)
    pipe.unload_lora()
    np.testing.assert_array_equal(image(), base)
