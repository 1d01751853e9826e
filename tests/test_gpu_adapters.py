"""LoHa, LoKr, full-difference and DoRA adapters merged into the resident bf16 weights (fmi_flux_lora_add_term / fmi_adapter_merge, csrc/adapter.hip) on
tests.util.SMALL_FLUX (D = 256, M = 1024).  The contract (include/flux_mi355x.h): W = bf16_rne(W0 + sum_a weight_a Delta_a), adapters in name order,
exact f32 operands, every product / sum / sqrt / division in f64, one rounding, always from a pristine copy of W0.

THE BOUND (tests/adapter_ref.assert_within_bound, used by every exactness test): with t the float64 target of tests/adapter_ref.merge_ref,
mag = |W0| + sum |weight Delta| and err = 2^-40 mag, an element is DECIDED if bf16_rne(t - err) == bf16_rne(t + err).  Every decided element must equal
bf16_rne(t) bit for bit, an undecided one must be one of the two bf16 neighbours of t, and at most 4 elements per test may be undecided — a condition on
the inputs (it depends on the reference alone; the seeds below were checked against it on the CPU).  2^-40 covers the f64 evaluation order and DoRA's
K <= 1280 row sums (K 2^-53 < 2^-42).  Model parity: the one-evaluation bar of tests/test_gpu_flux.py (1e-2)."""
import ctypes as C

import numpy as np
import pytest

from tests.adapter_ref import KINDS, MODULES, Term, adapter_files, assert_within_bound, bf16_rne64, merge_ref, random_term, undecided
from tests.lora_util import write_safetensors
from tests.util import SMALL_FLUX, SMALL_VAE, bf16_round, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu

D = 256
INVALID, STATE, UNSUPPORTED = -1, -3, -4
GUARD = 0x7BCD  # the pattern around the op-level destination


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
    torch = __import__("torch")
    return {n: m.get_tensor(n).view(torch.int16).cpu().numpy() for n in m._shapes() if n not in skip}


def assert_bits(got, want, names=None):
    for n in (names if names is not None else want):
        np.testing.assert_array_equal(got[n], want[n], err_msg=n)


def w0_of(env, prefix):
    return bf16_round(env["sd"][prefix + ".weight"]).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. op level: the tile edges through fmi_adapter_merge
def c_terms(env, terms):
    """[(weight, Term)] -> (fmi_adapter_term array, weights array, keepalive) with every tensor an f32 device tensor."""
    L = env["d"]._lib
    kinds = {"lora": L.ADAPTER_LORA, "loha": L.ADAPTER_LOHA, "lokr": L.ADAPTER_LOKR, "dora": L.ADAPTER_DORA}
    arr = (L.AdapterTermC * len(terms))()
    keep = []
    for ct, (_, t) in zip(arr, terms):
        ct.kind, ct.dtype, ct.scale, ct.row_offset = kinds[t.kind], L.F32, t.scale, t.row_offset
        tensors = list(t.tensors)
        mag = tensors.pop() if t.kind == "dora" else None
        for i, x in enumerate(tensors):
            if x is not None:
                dx = dev(np.ascontiguousarray(x, np.float32))
                keep.append(dx)
                ct.factor[i], ct.factor_rows[i], ct.factor_cols[i] = dx.data_ptr(), x.shape[0], x.shape[1]
        if mag is not None:
            dm = dev(np.ascontiguousarray(mag, np.float32))
            keep.append(dm)
            ct.magnitude = dm.data_ptr()
    return arr, (C.c_float * len(terms))(*[w for w, _ in terms]), keep


def op_merge(env, w0, terms):
    """fmi_adapter_merge of [(weight, Term)] on the bf16 values w0 (rows, K), into a destination surrounded by guard rows; run twice: the same bits.
    Returns the merged values as float64."""
    torch, lib = env["torch"], env["d"]._lib.load()
    rows, K = w0.shape
    w0d = dev(w0.astype(np.float32), torch.bfloat16)
    arr, weights, keep = c_terms(env, terms)
    runs = []
    for _ in range(2):
        buf = torch.full((rows + 16, K), GUARD, dtype=torch.int16, device="cuda")
        rc = lib.fmi_adapter_merge(C.c_void_p(w0d.data_ptr()), C.c_void_p(buf[8:].data_ptr()), rows, K, arr, weights, len(terms), None)
        env["d"]._lib.check(rc, lib)
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:8] == GUARD).all() and (out[8 + rows:] == GUARD).all(), "rows outside the matrix were written"
        runs.append(out[8:8 + rows])
    np.testing.assert_array_equal(runs[0], runs[1])  # the same bits from two runs
    return (runs[0].astype(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


CANCEL_STRIDE = 97
LOKR_SHAPES = {(72, 136): (8, 17, 9, 8), (64, 128): (4, 8, 16, 16), (200, 1280): (8, 16, 25, 80)}


def op_cases(rows, K, seed):
    """{name: (w0, [(weight, Term)])}: each kind alone at ranks 1, 16, 17 (below, at and one past the rank chunk), the LoKr forms, a full difference that
    cancels W0 on some elements, and all four kinds stacked at weights (1, -0.5, 0.75, 2)."""
    rng = np.random.default_rng(seed)
    w0 = bf16_round(0.02 * rng.standard_normal((rows, K))).astype(np.float64)
    a, b, c, d = LOKR_SHAPES[(rows, K)]
    cases = {}
    for r in (1, 16, 17):
        for kind in ("lora", "loha", "dora"):
            cases[f"{kind} r{r}"] = (w0, [(1.0, random_term(kind, rng, rows, K, r, scale=0.5 if r == 16 else 1.0, w0=w0))])
    cases["lokr full"] = (w0, [(1.0, random_term("lokr", rng, rows, K, 0, lokr=dict(a=a, b=b, c=c, d=d)))])
    cases["lokr w2 rank 3"] = (w0, [(1.0, random_term("lokr", rng, rows, K, 0, scale=2.0 / 3, lokr=dict(a=a, b=b, c=c, d=d, r2=3)))])
    cases["lokr w1 decomposed"] = (w0, [(1.0, random_term("lokr", rng, rows, K, 0, scale=0.5, lokr=dict(a=a, b=b, c=c, d=d, r1=2)))])
    cases["lokr both decomposed"] = (w0, [(-1.0, random_term("lokr", rng, rows, K, 0, lokr=dict(a=a, b=b, c=c, d=d, r1=2, r2=17)))])
    # row_offset: the last two thirds of the rows of the product (24 with 48 rows of the 72-row product at (72, 136)), as a part of a fused module
    off = rows // 3
    cases[f"lokr row_offset {off}"] = (w0[:rows - off], [(1.0, random_term("lokr", rng, rows - off, K, 0, lokr=dict(a=a, b=b, c=c, d=d, r2=3, row_offset=off)))])
    # the full-difference form w1 = [[1]] at weight f32(0.7), cancelling W0 on every 97th element up to a residue of the order of 3e-6 (1e-4 of |W0|).
    # The residue must not sit on a coarse binary grid (a difference of two f32 values near W0 would: 8 % of such elements are exact bf16 ties, which the
    # bound calls undecided), hence the 24-bit weight: weight * diff has 48 significant bits.
    diff = (0.01 * rng.standard_normal((rows, K))).astype(np.float32)
    sel = np.zeros(rows * K, bool)
    sel[::CANCEL_STRIDE] = True
    sel = sel.reshape(rows, K)
    diff[sel] = ((-w0[sel] + 3e-6 * rng.standard_normal(int(sel.sum()))) / np.float64(np.float32(0.7))).astype(np.float32)
    cases["diff cancels W0"] = (w0, [(0.7, Term("lokr", (np.ones((1, 1), np.float32), None, diff, None), 1.0))])
    stack = [(1.0, random_term("lora", rng, rows, K, 17, w0=w0)), (-0.5, random_term("loha", rng, rows, K, 16)),
             (0.75, random_term("lokr", rng, rows, K, 0, lokr=dict(a=a, b=b, c=c, d=d, r2=3))), (2.0, random_term("dora", rng, rows, K, 1, w0=w0))]
    cases["stacked"] = (w0, stack)
    cases["stacked, one off"] = (w0, [stack[0], (0.0, stack[1][1]), stack[2], stack[3]])
    return cases


@pytest.mark.parametrize("rows,K,seed", [(72, 136, 1), (64, 128, 2), (200, 1280, 3)])
def test_op_level_tile_edges(env, rows, K, seed):
    und = 0
    for name, (w0, terms) in op_cases(rows, K, seed).items():
        t, mag = merge_ref(w0, terms)
        got = op_merge(env, w0, terms)
        und += assert_within_bound(got, t, mag, what=f"({rows}, {K}) {name}")
        if name == "diff cancels W0":
            assert np.abs(t.ravel()[::CANCEL_STRIDE]).max() < 2e-5 < 1e-2 < np.abs(w0.ravel()[::CANCEL_STRIDE]).max()  # (W0 and the update cancel there)
        assert not np.array_equal(got, w0)
    assert und <= 4, und


# ------------------------------------------------------------------------------------------------ 2. plain LoRA is untouched
def test_plain_lora_is_untouched(env):
    torch = env["torch"]
    rng = np.random.default_rng(7)
    names = ["transformer_blocks.0.attn.to_k", "transformer_blocks.1.norm1.linear", "single_transformer_blocks.0.proj_out", "x_embedder"]
    pairs = {}
    for a_name, ranks in (("a", (16, 17, 3, 1)), ("b", (1, 64, 16, 5))):
        for n, r in zip(names, ranks):
            o, i = env["sd"][n + ".weight"].shape
            pairs[(a_name, n)] = random_term("lora", rng, o, i, r, scale=0.5 if a_name == "b" else 1.0)
    m1, m2 = fresh(env), fresh(env)
    for (a_name, n), t in pairs.items():
        m1.lora_add(a_name, n, t.tensors[0], t.tensors[1], t.scale)
        m2.lora_add_term(a_name, n, t)  # kind LORA through the new entry
    for m in (m1, m2):
        m.lora_set_weight("b", 1.2)
    b1 = snapshot(m1)
    assert_bits(snapshot(m2), b1)  # identical bits on every tensor of the model
    # ... and they are the bits of test_gpu_lora's own target: the one rounding of W0 + sum w s B A in float64
    und = 0
    for n in names:
        w0 = w0_of(env, n)
        t, mag = merge_ref(w0, [(1.0, pairs[("a", n)]), (1.2, pairs[("b", n)])])
        got = host(m1.get_tensor(n + ".weight", torch.float32))
        und += assert_within_bound(got, t, mag, what="plain " + n)
        assert float(np.mean(got != bf16_rne64(t))) <= 1e-3 and float(np.max(np.abs(got - t) / np.maximum(np.abs(t), 1e-30))) <= 2.0 ** -7  # test_gpu_lora's bars
    assert und <= 4
    # a LoHa term that is switched off does not move a Linear off the plain path: the same bits again
    m2.lora_add_term("c", names[0], random_term("loha", rng, D, D, 4))
    m2.lora_set_weight("c", 0.0)
    assert_bits(snapshot(m2), b1)


# ------------------------------------------------------------------------------------------------ 3. model level
def two_adapters(env, seed=11):
    """Adapters "a" and "b" over every module of MODULES (qkv thirds, linear1, linear2 with K = 1280, the modulation Linears, the MLPs), read from kohya
    files: module i holds kind i % 4 in "a" and kind (i + 1) % 4 in "b", so that all four kinds meet each other.  {name: {prefix: AdapterTerm}}."""
    from diffusion_rs_amd.lora import read_adapter
    out = {}
    for which, shift in (("a", 0), ("b", 1)):
        files = {}
        for k, kind in enumerate(KINDS):
            mods = [mod for i, mod in enumerate(MODULES) if (i + shift) % 4 == k]
            files.update(adapter_files(kind, seed=seed + 10 * shift + k, rank=16, sd=env["sd"], modules=mods)[1])
        out[which] = read_adapter(files, hidden_size=D)
        assert len(out[which]) == 20
    return out


WEIGHTS = {"a": 0.75, "b": -0.5}


def model_targets(env, adapters, weights):
    """{prefix: (target, mag)} of every adapted Linear, adapters in name order."""
    prefixes = sorted({p for terms in adapters.values() for p in terms})
    return {p: merge_ref(w0_of(env, p), [(weights[a], adapters[a][p]) for a in sorted(adapters) if p in adapters[a]]) for p in prefixes}


@pytest.fixture(scope="module")
def adapted(env):
    adapters = two_adapters(env)
    m = fresh(env)
    for name in ("b", "a"):
        for prefix, term in adapters[name].items():
            m.lora_add_term(name, prefix, term)
        m.lora_set_weight(name, WEIGHTS[name])
    return dict(m=m, adapters=adapters, targets=model_targets(env, adapters, WEIGHTS))


def test_model_level_exactness(env, adapted):
    torch = env["torch"]
    m = adapted["m"]
    assert m.loras() == ["a", "b"]
    kinds = {(adapted["adapters"]["a"][p].kind, adapted["adapters"]["b"][p].kind) for p in adapted["targets"]}
    assert {k for pair in kinds for k in pair} == set(KINDS)
    und = 0
    for prefix, (t, mag) in adapted["targets"].items():
        und += assert_within_bound(host(m.get_tensor(prefix + ".weight", torch.float32)), t, mag, what=prefix)
    assert und <= 4, und
    bits = snapshot(m)
    untouched = [n for n in bits if n[:-len(".weight")] not in adapted["targets"] or not n.endswith(".weight")]
    assert "transformer_blocks.1.attn.to_q.weight" in untouched and "single_transformer_blocks.0.proj_mlp.weight" in untouched
    assert "transformer_blocks.0.attn.to_k.bias" in untouched and len(untouched) == len(bits) - 20
    assert_bits(bits, env["base_bits"], untouched)


# ------------------------------------------------------------------------------------------------ 4. unload is exact, history does not matter
def test_unload_is_exact_and_history_does_not_matter(env, adapted):
    adapters = adapted["adapters"]
    want = snapshot(adapted["m"])

    def add(m, name, reverse=False):
        items = list(adapters[name].items())
        for prefix, term in (reversed(items) if reverse else items):
            m.lora_add_term(name, prefix, term)

    results = []
    # order 1: a, b, reweight; order 2: b at another weight, a, switch b off and on, reweight; order 3: a, b, remove a, add a again (its terms reversed)
    m = fresh(env)
    add(m, "a"), add(m, "b")
    m.lora_set_weight("a", WEIGHTS["a"]), m.lora_set_weight("b", WEIGHTS["b"])
    results.append(m)
    m = fresh(env)
    add(m, "b", reverse=True)
    m.lora_set_weight("b", 3.0)
    add(m, "a")
    m.lora_set_weight("b", 0.0)
    m.lora_set_weight("a", WEIGHTS["a"])
    m.lora_set_weight("b", WEIGHTS["b"])
    results.append(m)
    m = fresh(env)
    add(m, "a"), add(m, "b")
    m.lora_set_weight("b", WEIGHTS["b"])
    m.lora_remove("a")
    add(m, "a", reverse=True)
    m.lora_set_weight("a", WEIGHTS["a"])
    results.append(m)
    out0 = host(adapted["m"].forward(*env["fwd"]))
    assert not np.array_equal(out0, env["base_out"])
    for m in results:
        assert m.loras() == ["a", "b"]
        assert_bits(snapshot(m), want)
        np.testing.assert_array_equal(host(m.forward(*env["fwd"])), out0)
    # weight 0 on both: the loaded bits while the adapters stay listed; removal: the loaded bits, the base output, the base size
    m = results[0]
    m.lora_set_weight("a", 0.0), m.lora_set_weight("b", 0.0)
    assert_bits(snapshot(m), env["base_bits"])
    m.lora_set_weight("b", WEIGHTS["b"])
    m.lora_remove("a")
    only_b = fresh(env)
    add(only_b, "b")
    only_b.lora_set_weight("b", WEIGHTS["b"])
    assert_bits(snapshot(m), snapshot(only_b))
    for m in results:
        assert m.size_in_bytes() > env["base_size"]
        m.lora_remove(None)
        assert m.loras() == []
        assert_bits(snapshot(m), env["base_bits"])
        np.testing.assert_array_equal(host(m.forward(*env["fwd"])), env["base_out"])
        assert m.size_in_bytes() == env["base_size"]


# ------------------------------------------------------------------------------------------------ 5. through the model
def test_through_the_model(env, adapted):
    torch = env["torch"]
    img, ids, txt, txt_ids, y, t, g = env["inputs"]
    m = adapted["m"]
    got = host(m.forward(*env["fwd"]))
    twin = env["d"].FluxModel(SMALL_FLUX)
    for n in m._shapes():
        twin.set_tensor(n, m.get_tensor(n))
    twin.assert_complete()
    np.testing.assert_array_equal(host(twin.forward(*env["fwd"])), got)
    merged = dict(env["sd"])
    for prefix, (tgt, _) in adapted["targets"].items():
        merged[prefix + ".weight"] = bf16_rne64(tgt).astype(np.float32)
    om = env["orc"].Flux(SMALL_FLUX)
    om.load(merged)
    ref = om.forward(img, ids, txt, txt_ids, t, y, g)
    ob = env["orc"].Flux(SMALL_FLUX)
    ob.load(env["sd"])
    moved = rel_l2(ref, ob.forward(img, ids, txt, txt_ids, t, y, g))
    err = rel_l2(got, ref)
    print(f"two adapters of four kinds on 20 linears: the oracle's output moves by {moved:.3e}; GPU forward vs adapted oracle rel-L2 {err:.3e}")
    assert moved >= 1e-2  # otherwise the comparison below shows nothing
    assert np.isfinite(got).all() and err <= 1e-2


# ------------------------------------------------------------------------------------------------ 6. errors leave the model untouched
def expect_error(env, m, code, call, before, skip=(), match=None):
    lib = m.lib
    lib.fmi_flux_get_tensor(m.h, b"no such tensor", None, 0, None, 0)  # leaves ITS message: a stale one cannot pass for the call's own below
    stale = lib.fmi_last_error()
    with pytest.raises(env["d"].FmiError, match=match) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    assert len(lib.fmi_last_error()) > 0 and lib.fmi_last_error() != stale
    assert_bits(snapshot(m, skip), before)


def test_errors_leave_the_model_untouched(env):
    d, orc = env["d"], env["orc"]
    rng = np.random.default_rng(8)
    m = fresh(env)
    p = "transformer_blocks.0.attn.to_k"  # (256, 256), the middle part of a fused matrix
    m.lora_add_term("a", p, random_term("loha", rng, D, D, 4))
    m.lora_add_term("a", "x_embedder", random_term("lora", rng, D, 64, 2))
    before = snapshot(m)
    f = lambda *s: (0.05 * rng.standard_normal(s)).astype(np.float32)  # noqa: E731
    lokr = lambda a, b, c, dd, off=0: Term("lokr", (f(a, b), None, f(c, dd), None), 1.0, off)  # noqa: E731
    bad = {
        "lokr b * d != in": lokr(4, 16, 64, 15),
        "lokr row_offset + out > a * c": lokr(4, 16, 64, 16, off=8),
        "lokr negative row_offset": lokr(8, 16, 64, 16, off=-64),
        "lokr a * c < out": lokr(3, 16, 64, 16),
        "lokr decomposed w2 does not multiply": Term("lokr", (f(4, 16), None, f(64, 3), f(2, 16))),
        "loha unequal ranks": Term("loha", (f(D, 4), f(4, D), f(D, 3), f(3, D))),
        "loha rows of another Linear": Term("loha", (f(D + 8, 4), f(4, D), f(D + 8, 4), f(4, D))),
        "loha columns of another Linear": Term("loha", (f(D, 4), f(4, D + 8), f(D, 4), f(4, D + 8))),
        "loha missing factor": Term("loha", (f(D, 4), f(4, D), f(D, 4), None)),
        "lora factors of another Linear": Term("lora", (f(4, D + 8), f(D, 4))),
        "dora without a magnitude": Term("dora", (f(4, D), f(D, 4))),
        "nan scale": Term("loha", (f(D, 4), f(4, D), f(D, 4), f(4, D)), float("nan")),
        "unknown kind": Term(7, (f(4, D), f(D, 4))),
        "negative kind": Term(-1, (f(4, D), f(D, 4))),
    }
    for what, term in bad.items():
        print(what)
        expect_error(env, m, INVALID, lambda: m.lora_add_term("b", p, term), before)
    # a zero-norm DoRA row: rank 1, B = -e_5, A = row 5 of W0, scale 1 -> row 5 of V = W0 + B A is exactly zero
    w0 = w0_of(env, p)
    B = np.zeros((D, 1), np.float32)
    B[5] = -1.0
    zero = Term("dora", (w0[5:6].astype(np.float32), B, np.ones(D, np.float32)), 1.0)
    expect_error(env, m, INVALID, lambda: m.lora_add_term("b", p, zero), before, match="to_k")
    # ... also while the Linear holds merged adapters (the norm reads the pristine copy, not the resident rows) and on a Linear without any
    expect_error(env, m, INVALID, lambda: m.lora_add_term("a", p, zero), before, match="to_k")
    q = "transformer_blocks.1.attn.to_out.0"
    wq = w0_of(env, q)
    zq = Term("dora", (wq[5:6].astype(np.float32), B, np.ones(D, np.float32)), 1.0)
    expect_error(env, m, INVALID, lambda: m.lora_add_term("b", q, zq), before, match="to_out")
    expect_error(env, m, INVALID, lambda: m.lora_add_term("b", "transformer_blocks.0.attn.to_x", random_term("loha", rng, D, D, 4)), before)  # unknown Linear
    expect_error(env, m, INVALID, lambda: d._lib.check(m.lib.fmi_flux_lora_add_term(m.h, b"b", p.encode(), None), m.lib), before)             # null term
    assert m.loras() == ["a"]  # no failed call left an adapter "b" behind
    # an adapted weight answers as it does for LoRA: set_tensor and the quantised setters are STATE until the adapters are removed
    w = env["sd"][p + ".weight"]
    expect_error(env, m, STATE, lambda: m.set_tensor(p + ".weight", w), before, match="remove the adapters first")
    packed, absmax = orc.quantize_blockwise_4bit(w.ravel(), 64, "nf4")
    expect_error(env, m, STATE, lambda: m.set_linear_bnb4(p, packed, absmax, 64, "nf4", w.shape[0], w.shape[1]), before)
    m.lora_remove("a")
    assert_bits(snapshot(m), env["base_bits"])

    # an 8-bit model
    q8 = fresh(env)
    q8.quantize_int8()
    expect_error(env, q8, STATE, lambda: q8.lora_add_term("a", p, random_term("loha", rng, D, D, 4)), env["base_bits"])
    assert q8.loras() == []

    # a Linear that is resident as nf4 codes
    n4 = d.FluxModel(SMALL_FLUX)
    packed_names = ["transformer_blocks.0.attn.to_q.weight", "transformer_blocks.0.attn.to_k.weight", "transformer_blocks.0.attn.to_v.weight"]
    for n, wt in env["sd"].items():
        if n in packed_names:
            pk, am = orc.quantize_blockwise_4bit(wt.ravel(), 64, "nf4")
            n4.set_linear_bnb4(n[:-len(".weight")], pk, am, 64, "nf4", wt.shape[0], wt.shape[1])
        else:
            n4.set_tensor(n, wt)
    n4.assert_complete()
    rest = {n: v for n, v in env["base_bits"].items() if n not in packed_names}
    for kind in ("loha", "dora"):
        expect_error(env, n4, UNSUPPORTED, lambda: n4.lora_add_term("a", p, random_term(kind, rng, D, D, 4, w0=w0)), rest, skip=packed_names)
    assert n4.loras() == []
    n4.lora_add_term("a", "transformer_blocks.0.attn.add_k_proj", random_term("loha", rng, D, D, 4))  # the dense Linears of the same model take adapters
    assert n4.loras() == ["a"]


# ------------------------------------------------------------------------------------------------ 7. pipeline
@pytest.fixture(scope="module")
def files(env, tmp_path_factory):
    root = tmp_path_factory.mktemp("adapters")
    paths = {}
    for i, kind in enumerate(("lora", "loha", "lokr", "dora")):
        peft, kohya, _ = adapter_files(kind, seed=20 + i, rank=16, sd=env["sd"])
        paths[kind] = str(root / f"{kind}.safetensors")
        write_safetensors(paths[kind], peft if kind == "dora" else kohya)  # (DoRA in PEFT's layout, the LyCORIS kinds in kohya's)
    return paths


def test_pipeline_loads_every_kind(env, files):
    d = env["d"]
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=SMALL_FLUX, vae_cfg=SMALL_VAE))
    params = d.DiffusionGenerationParams(height=64, width=64, num_steps=2, guidance_scale=3.5)

    def image():
        return pipe.forward(["a lighthouse at dusk"], params, seed=3, output="tensor").cpu().numpy()

    base = image()
    seen = [base]
    for kind in ("lora", "loha", "lokr", "dora"):  # stacked on a plain one
        assert pipe.load_lora(files[kind], weight=0.5 if kind == "lokr" else 1.0) == kind
        seen.append(image())
        assert np.isfinite(seen[-1]).all() and not any(np.array_equal(seen[-1], s) for s in seen[:-1]), kind
    assert pipe.loras() == ["dora", "loha", "lokr", "lora"]
    stacked = seen[-1]
    for kind in ("loha", "lokr", "dora", "lora"):
        pipe.set_lora_weight(kind, 0.0)
    np.testing.assert_array_equal(image(), base)
    for kind, w in (("lora", 1.0), ("dora", 1.0), ("lokr", 0.5), ("loha", 1.0)):
        pipe.set_lora_weight(kind, w)
    np.testing.assert_array_equal(image(), stacked)  # nothing depends on the detour
    pipe.unload_lora("dora")
    np.testing.assert_array_equal(image(), seen[3])
    pipe.unload_lora()
    assert pipe.loras() == []
    np.testing.assert_array_equal(image(), base)
    with pytest.raises(ValueError, match="read_adapter"):
        d.read_lora(files["loha"])


def test_quantize_int8_after_loading_quantises_the_merged_weights(env, adapted):
    img, ids, txt, txt_ids, y, t, g = env["inputs"]
    m = fresh(env)
    for name in ("a", "b"):
        for prefix, term in adapted["adapters"][name].items():
            m.lora_add_term(name, prefix, term)
        m.lora_set_weight(name, WEIGHTS[name])
    m.quantize_int8()
    got = host(m.forward(*env["fwd"]))
    merged = dict(env["sd"])
    for prefix, (tgt, _) in adapted["targets"].items():
        merged[prefix + ".weight"] = bf16_rne64(tgt).astype(np.float32)
    om = env["orc"].Flux(SMALL_FLUX)
    om.load(merged)
    om.set_int8(True, 0x33, attention=True)
    ref8 = om.forward(img, ids, txt, txt_ids, t, y, g)
    e8 = rel_l2(got, ref8)
    print(f"int8 after LoHa / LoKr / DoRA: vs the int8 oracle on the merged weights {e8:.3e}")
    assert e8 <= 1e-2  # the bar of tests/test_gpu_int8.py, as in tests/test_gpu_lora.py
    rng = np.random.default_rng(9)
    for call in (lambda: m.lora_add_term("c", "transformer_blocks.0.attn.to_k", random_term("loha", rng, D, D, 4)), lambda: m.lora_set_weight("a", 0.5),
                 lambda: m.lora_remove("a")):
        with pytest.raises(env["d"].FmiError) as ei:
            call()
        assert ei.value.code == STATE
    assert m.loras() == ["a", "b"]
    plain = fresh(env)
    plain.quantize_int8()
    plain.forward(*env["fwd"])
    assert m.size_in_bytes() == plain.size_in_bytes()  # factors, per-row vectors, pristine copies and scratch were released when the adapters froze
