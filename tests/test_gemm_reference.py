"""The checker of tests/test_gpu_gemm_epilogues.py, and its own test on the CPU: the f64 reference of one GEMM problem with each of the launcher's
epilogues, the element-wise tolerance the GPU result is held to, the table of cases, and a self-check — an f32 emulation of every epilogue with two
accumulation orders must stay inside the tolerance on every case, and each planted error (the mistakes an epilogue can make without a whole-model
rel-L2 noticing) must fall outside it.

Tolerance (derived, not fitted).  The operands are bf16, e4m3 or int8 values, so every product x * w is exact in f32; what an f32 accumulation of K
products loses, in any order, is at most K * 2^-24 * A with A = sum_k |x * w| (the classical bound, first order).  With c = 2 (C_ACC: doubled because
the rounding inside the MFMA accumulator is not documented):
  e_acc = c * K * 2^-24 * A * |alpha|                                      (0 for int8: the integer sum is exact)
  tol32 = |g| * e_acc + 4 * 2^-24 * (|r| + |g| * (|alpha| * A + |bias|))   f32 results; g = gate (1 without), r = incoming residual (0 without)
  tol   = tol32 + 2^-8 * (|ref| + tol32)                                   bf16 results: one rounding to 8 significant bits on top
  tol   = max(2^-7 * |ref|, 1e-6) + 1.13 * tol32                           GELU / SiLU outputs: the activation bar of
          test_gpu_ops.py::test_activation_epilogues_over_the_whole_range, plus the input error through a slope of at most 1.13
The bf16 term is the format's unit roundoff: round-to-nearest to p = 8 significant bits errs by up to half an ulp = 2^-8 of the value at the bottom of
a binade (2^-9 only at its top), so 2^-9 — the figure the issue for this file first named — rejects correctly rounded results: the f32 emulation below
(exact rounding) reached 1.94 x that bound on the first bf16 case it met.  2^-8 is the smallest bound a correct kernel can meet; a two-ulp error stays outside.
e4m3 operands take c = 8 (C_ACC_E4M3).  Measured on the MI355X: the bf16 and int8 paths stay below 0.08 of the classical bound, the e4m3 MFMA
(v_mfma_scale_f32_32x32x64_f8f6f4) reaches 4.7 of it at K = 256 on operands that span the format's range, with a mean of 0.6 — and the excess is spread
evenly: 176 .. 252 elements above 2 in each of the nine 32-row blocks, 226 .. 271 in each 64-column block, 43 .. 77 per row position inside a block,
219 .. 289 per column position (probe: 300 x 512 x 256, unit scales, plain f32 store).  That is the instruction's accumulation (products aligned and
truncated inside the matrix unit), not an indexing error of the kernel, which would sit in rows, columns or tiles; so the bound is raised for this
operand type alone, to the next power of two above the measurement.  Every planted error still falls outside.
For 8-bit operands A is taken in dequantised units: sum_k |x * w| * a_scale * w_scale + |a_off * w_sum|.
"""
import numpy as np
import pytest

from tests.util import bf16_round

STORE_BF16, GELU_BF16, RESID_GATE_F32, GELU_FROM_COL, STORE_F32, SCALE_BF16, RESID_ADD_BF16, SILU_BF16 = range(8)
U32 = 2.0 ** -24  # unit roundoff of f32
U16 = 2.0 ** -8   # unit roundoff of bf16 (8 significant bits; see the docstring)
C_ACC = 2.0
C_ACC_E4M3 = 8.0  # e4m3 operands: see the docstring
F32_OUT = (RESID_GATE_F32, STORE_F32)


def spec(M, N, K, epi, **kw):
    """One GEMM problem of a case.  rpb = rows_per_batch (0: one gate row); a_col0 / lda, ldw, ldo: strided views (defaults: dense);
    out_off / bias_off: elements the out / bias pointer is moved past its (aligned) buffer; q8: 0 bf16, 1 e4m3, 2 int8; off: the int8 offset term."""
    s = dict(M=M, N=N, K=K, epi=epi, bias=True, alpha=1.0, gelu_from=0, rpb=0, gate_bstride=None, lda=None, a_col0=0, ldw=None, ldo=None, q8=0,
             off=False, out_off=0, bias_off=0, seed=0)
    assert not set(kw) - set(s), kw
    s.update(kw)
    s["lda"] = s["lda"] or K
    s["ldw"] = s["ldw"] or K
    s["ldo"] = s["ldo"] or N
    s["nb"] = -(-M // s["rpb"]) if s["rpb"] else 1
    if s["gate_bstride"] is None:
        s["gate_bstride"] = 2 * N if s["rpb"] else 0
    return s


def _cases():
    RG, GFC = RESID_GATE_F32, GELU_FROM_COL
    c = {}
    # gated f32 residual read-modify-write: staged with a ragged last tile row; per-batch gate rows (boundaries at rows 100, 200: inside a 64-row pass and
    # inside a group of 8 rows); N = 260: first N tile staged, second direct; ldo = N + 4: the whole launch direct; N = 64 / 128: the narrow kernel
    c["gate_one_row"] = [spec(300, 512, 128, RG)]
    c["gate_per_batch"] = [spec(300, 512, 128, RG, rpb=100)]
    c["gate_per_batch_n260"] = [spec(300, 260, 128, RG, rpb=100)]
    c["gate_per_batch_ldo_n_plus_4"] = [spec(300, 512, 128, RG, rpb=100, ldo=516)]
    c["gate_per_batch_n64"] = [spec(300, 64, 128, RG, rpb=100)]
    c["gate_per_batch_n128"] = [spec(300, 128, 128, RG, rpb=100)]
    # GELU from a column on: whole tiles on either side (768), a tile that straddles the boundary (384: tile 1 of 4)
    c["gelu_from_768"] = [spec(300, 1024, 128, GFC, gelu_from=768)]
    c["gelu_from_384"] = [spec(300, 1024, 128, GFC, gelu_from=384)]
    for epi, name in ((STORE_F32, "store_f32"), (SCALE_BF16, "scale_bf16")):
        for n in (64, 512, 260):
            for bias in (True, False):
                c[f"{name}_n{n}_{'bias' if bias else 'nobias'}"] = [spec(300, n, 128, epi, alpha=0.125, bias=bias)]
    # unaligned views: out + 4 elements (8 bytes: no 16-byte stores), bias + 1 element (no 8-byte bias loads: the per-element path)
    c["unaligned_out"] = [spec(300, 512, 128, STORE_BF16, out_off=4)]
    c["unaligned_bias"] = [spec(300, 512, 128, GELU_BF16, bias_off=1)]
    c["unaligned_out_and_bias"] = [spec(300, 512, 128, SCALE_BF16, alpha=0.125, out_off=4, bias_off=1)]
    # strided operands: A = columns [256, 512) of a (300, 768) buffer, W rows 2 K apart, out rows N + 256 apart
    c["strided_store"] = [spec(300, 512, 256, STORE_BF16, lda=768, a_col0=256, ldw=512, ldo=768)]
    c["strided_gate"] = [spec(300, 512, 256, RG, rpb=100, lda=768, a_col0=256, ldw=512, ldo=768)]
    c["resid_add_bf16"] = [spec(300, 260, 128, RESID_ADD_BF16)]
    # grouped launches
    c["group_2"] = [spec(192, 512, 128, STORE_BF16), spec(80, 512, 128, RG, seed=1)]
    c["group_3_kind3"] = [spec(300, 512, 64, STORE_F32, alpha=0.125), spec(200, 260, 128, SCALE_BF16, alpha=0.125, seed=1), spec(100, 512, 192, SILU_BF16, seed=2)]
    c["group_8"] = [spec(40 + 37 * i, (256, 512, 260, 512)[i % 4], 64 + 64 * (i % 2), RG if i % 3 == 0 else STORE_BF16, rpb=50 if i == 3 else 0, seed=i)
                    for i in range(8)]
    c["group_n64_in_wide"] = [spec(300, 512, 128, STORE_BF16), spec(100, 64, 128, STORE_BF16, seed=1)]
    c["group_13_tiles"] = [spec(600, 768, 64, STORE_BF16), spec(300, 512, 64, STORE_BF16, seed=1)]  # 9 + 4 tiles: the XCD remap with a remainder
    # 8-bit operands
    for q8, name in ((1, "e4m3"), (2, "i8")):
        c[f"{name}_gate_per_batch"] = [spec(300, 512, 256, RG, rpb=100, q8=q8)]
        c[f"{name}_gelu_from_768"] = [spec(300, 1024, 256, GFC, gelu_from=768, q8=q8)]
        c[f"{name}_gelu_from_384"] = [spec(300, 1024, 256, GFC, gelu_from=384, q8=q8)]
        c[f"{name}_store_f32"] = [spec(300, 260, 256, STORE_F32, alpha=0.125, q8=q8)]
    c["i8_offset_gate_per_batch"] = [spec(300, 512, 256, RG, rpb=100, q8=2, off=True)]
    c["i8_offset_store_f32"] = [spec(300, 260, 256, STORE_F32, alpha=0.125, q8=2, off=True)]
    return c


CASES = _cases()
# split-K: name -> (the unsplit problems, the split factors); every part is a STORE_F32 problem of ONE grouped launch, then the reduce kernel per problem
SPLITK_CASES = {
    "splitk_one": ([spec(300, 512, 2048, RESID_GATE_F32, rpb=100, ldo=520)], (2, 4, 8)),
    "splitk_group_2": ([spec(300, 512, 2048, RESID_GATE_F32, rpb=100), spec(120, 260, 1024, RESID_GATE_F32, seed=1)], (2, 4)),
}


def e4m3_values():
    """The 256 OCP e4m3 values as f64 (NaN at 0x7f / 0xff) — the same table as oracle.e4m3_table(), restated so that this file needs numpy only."""
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    v = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    v = np.where((c & 0x7f) == 0x7f, np.nan, v)
    return np.where(c & 0x80, -v, v)


def make(s):
    """The arrays of a problem, deterministic in the spec.  x / w: the operand VALUES as f32 (bf16-exact; for q8 the decoded codes xq / wq)."""
    rng = np.random.default_rng([s["seed"], s["M"], s["N"], s["K"], s["epi"], s["q8"]])
    M, N, K = s["M"], s["N"], s["K"]
    a = {}
    if s["q8"] == 0:
        a["x"] = bf16_round(rng.standard_normal((M, K)).astype(np.float32))
        a["w"] = bf16_round((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
    else:
        if s["q8"] == 1:  # codes below 0x58 (|value| < 16), either sign: no NaN code
            a["xq"] = (rng.integers(0, 0x58, (M, K)) | (rng.integers(0, 2, (M, K)) << 7)).astype(np.uint8)
            a["wq"] = (rng.integers(0, 0x58, (N, K)) | (rng.integers(0, 2, (N, K)) << 7)).astype(np.uint8)
            tab = e4m3_values().astype(np.float32)
            a["x"], a["w"] = tab[a["xq"]], tab[a["wq"]]
            unit = 4.0
        else:
            a["xq"] = rng.integers(-127, 128, (M, K)).astype(np.int8)
            a["wq"] = rng.integers(-127, 128, (N, K)).astype(np.int8)
            a["x"], a["w"] = a["xq"].astype(np.float32), a["wq"].astype(np.float32)
            unit = 73.0
        # per-row / per-channel scales that bring the products back to x ~ 1, w ~ 1 / sqrt(K)
        a["a_scale"] = ((0.5 + rng.random(M)) / unit).astype(np.float32)
        a["w_scale"] = ((0.5 + rng.random(N)) / (unit * np.sqrt(K))).astype(np.float32)
        if s["off"]:
            a["a_off"] = rng.standard_normal(M).astype(np.float32)
            a["w_sum"] = (rng.standard_normal(N) * 0.5).astype(np.float32)
    a["bias"] = bf16_round(rng.standard_normal(N).astype(np.float32)) if s["bias"] else None
    if s["epi"] == RESID_GATE_F32:
        g = rng.standard_normal((s["nb"], N))
        a["gate"] = (np.sign(g) * (0.5 + np.abs(g))).astype(np.float32)  # |gate| >= 0.5: the error figure err / (|g| K 2^-24 A) stays meaningful
        a["r0"] = rng.standard_normal((M, N)).astype(np.float32)
    elif s["epi"] == RESID_ADD_BF16:
        a["r0"] = bf16_round(rng.standard_normal((M, N)).astype(np.float32))
    return a


def gelu64(v):
    return 0.5 * v * (1.0 + np.tanh(0.7978845608028654 * v * (1.0 + 0.044715 * v * v)))


def silu64(v):
    with np.errstate(over="ignore"):
        return v / (1.0 + np.exp(-v))


def gate_rows(s, a):
    """(M, N) gate of every output row (1 without a gate)."""
    if s["epi"] != RESID_GATE_F32:
        return np.ones((1, 1))
    b = np.arange(s["M"]) // s["rpb"] if s["rpb"] else np.zeros(s["M"], int)
    return a["gate"].astype(np.float64)[b]


def ref(s, a):
    """f64 reference of one problem: dict(out, A, g, r, bias) — out (M, N), A = sum_k |x w| (dequantised units), g gate, r incoming residual."""
    x, w = a["x"].astype(np.float64), a["w"].astype(np.float64)
    acc, A = x @ w.T, np.abs(x) @ np.abs(w).T
    if s["q8"]:
        sc = a["a_scale"].astype(np.float64)[:, None] * a["w_scale"].astype(np.float64)[None, :]
        acc, A = acc * sc, A * sc
        if s["off"]:
            o = a["a_off"].astype(np.float64)[:, None] * a["w_sum"].astype(np.float64)[None, :]
            acc, A = acc + o, A + np.abs(o)
    bias = np.zeros(s["N"]) if a["bias"] is None else a["bias"].astype(np.float64)
    pre = s["alpha"] * acc + bias[None, :]
    g = gate_rows(s, a)
    r = a["r0"].astype(np.float64) if "r0" in a else np.zeros((1, 1))
    epi = s["epi"]
    if epi == GELU_BF16:
        out = gelu64(pre)
    elif epi == SILU_BF16:
        out = silu64(pre)
    elif epi == GELU_FROM_COL:
        out = np.where(np.arange(s["N"])[None, :] >= s["gelu_from"], gelu64(pre), pre)
    elif epi in (RESID_GATE_F32, RESID_ADD_BF16):
        out = r + g * pre
    else:
        out = pre
    return dict(out=out, A=A, g=g, r=r, bias=bias)


def tol(s, R, c=None):
    """Element-wise tolerance (M, N) of a result against ref(); affine in c: tol(c) = tol(0) + c * (tol(1) - tol(0)).  c: C_ACC, C_ACC_E4M3 for e4m3 operands."""
    if c is None:
        c = C_ACC_E4M3 if s["q8"] == 1 else C_ACC
    al, g = abs(s["alpha"]), np.abs(R["g"])
    e_acc = 0.0 if s["q8"] == 2 else c * s["K"] * U32 * R["A"] * al
    tol32 = g * e_acc + 4 * U32 * (np.abs(R["r"]) + g * (al * R["A"] + np.abs(R["bias"])[None, :]))
    epi = s["epi"]
    if epi in F32_OUT:
        return tol32
    plain = tol32 + U16 * (np.abs(R["out"]) + tol32)
    act = np.maximum(2.0 ** -7 * np.abs(R["out"]), 1e-6) + 1.13 * tol32
    if epi in (GELU_BF16, SILU_BF16):
        return act
    if epi == GELU_FROM_COL:
        return np.where(np.arange(s["N"])[None, :] >= s["gelu_from"], act, plain)
    return plain


def acc_ratio(s, R, err):
    """err / (K 2^-24 A |alpha| |g|): the error in units of the classical accumulation bound (c = 1), element-wise."""
    return err / (s["K"] * U32 * R["A"] * abs(s["alpha"]) * np.abs(R["g"]) + 1e-300)


# ---------------------------------------------------------------------------------------------------- f32 emulation (self-check)
def _accumulate(x, w, order):
    M, K = x.shape
    N = w.shape[0]
    if order == "seq":
        acc = np.zeros((M, N), np.float32)
        for k in range(K):
            acc += x[:, k, None] * w[None, :, k]
        return acc
    parts = []  # sequential inside blocks of 16, then a pairwise tree over the blocks
    for k0 in range(0, K, 16):
        p = np.zeros((M, N), np.float32)
        for k in range(k0, min(k0 + 16, K)):
            p += x[:, k, None] * w[None, :, k]
        parts.append(p)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def _gelu32(v):
    v = v.astype(np.float32)
    u = np.float32(0.7978845608028654) * v * (np.float32(1) + np.float32(0.044715) * v * v)
    return np.float32(0.5) * v * (np.float32(1) + np.tanh(u))


def emulate(s, a, order, splits=1, plant=None, acc=None):
    """The launcher's arithmetic in numpy f32 (every step rounded to f32, the result to bf16 where the kernel stores bf16), with a planted error on request."""
    f = np.float32
    M, N, K = s["M"], s["N"], s["K"]
    if acc is None:
        kc = K // splits
        acc = _accumulate(a["x"][:, :kc], a["w"][:, :kc], order)
        for i in range(1, splits):  # the split-K reduce adds the parts in index order
            acc = acc + _accumulate(a["x"][:, i * kc:(i + 1) * kc], a["w"][:, i * kc:(i + 1) * kc], order)
    v = acc.copy()
    if s["q8"]:
        v = v * (a["a_scale"][:, None] * a["w_scale"][None, :])
        if s["off"]:
            v = v + a["a_off"][:, None] * a["w_sum"][None, :]
    epi = s["epi"]
    if epi in (STORE_F32, SCALE_BF16):
        v = v * f(s["alpha"])
    if a["bias"] is not None:
        b = np.roll(a["bias"], -1) if plant == "bias_shift" else a["bias"]
        v = v + b[None, :]
    gf = s["gelu_from"] + (4 if plant == "gelu_shift4" else 0)
    if epi == GELU_BF16:
        v = _gelu32(v)
    elif epi == SILU_BF16:
        v = silu64(v.astype(np.float64)).astype(f)
    elif epi == GELU_FROM_COL:
        v = np.where(np.arange(N)[None, :] >= gf, _gelu32(v), v)
    if epi == RESID_GATE_F32:
        b = np.arange(M) // s["rpb"] if s["rpb"] else np.zeros(M, int)
        if plant == "gate_neighbour":  # the last row of a batch takes the next batch's gate, the first row the previous one's
            pos = np.arange(M) % s["rpb"]
            b = np.clip(b + (pos == s["rpb"] - 1) - (pos == 0), 0, s["nb"] - 1)
        out = a["r0"] + a["gate"][b] * v
    elif epi == RESID_ADD_BF16:
        out = bf16_round(v + a["r0"])
    elif epi == STORE_F32:
        out = v
    else:
        out = bf16_round(v)
    out = out.astype(np.float64)
    if plant == "tile_swap":  # the rows of tile row 0 and of tile row 1 change places (as many as the ragged second tile has)
        n = min(256, M - 256)
        out[:n], out[256:256 + n] = out[256:256 + n].copy(), out[:n].copy()
    return out


def plant_two_ulps(s, R, out):
    """`out` with ONE element moved by two bf16 ulps: the element the result determines best (largest |ref| / A) among those in the lower half of
    their binade — there two ulps are 2^-6 .. 2^-6 / 1.5 of the value, above every bar of tol() including the one-ulp activation bar."""
    ref_ = np.abs(R["out"])
    mant = ref_ / 2.0 ** np.floor(np.log2(np.maximum(ref_, 1e-300)))
    score = np.where((mant < 1.5) & (ref_ > 2.0 ** -20), ref_ / (np.abs(R["g"]) * R["A"] + np.abs(R["r"]) + 1e-300), -1.0)
    i = np.unravel_index(np.argmax(score), score.shape)
    bad = out.copy()
    bad[i] += 2 * 2.0 ** (np.floor(np.log2(ref_[i])) - 7)
    return bad, i


def all_specs():
    seen, out = set(), []
    for name, specs in list(CASES.items()) + [(n, v[0]) for n, v in SPLITK_CASES.items()]:
        for i, s in enumerate(specs):
            key = tuple(sorted((k, v) for k, v in s.items() if k not in ("lda", "a_col0", "ldw", "ldo", "out_off", "bias_off", "gate_bstride")))
            if key not in seen:  # (strides and pointer offsets do not change the arithmetic)
                seen.add(key)
                out.append((f"{name}[{i}]", s, SPLITK_CASES[name][1] if name in SPLITK_CASES else (1,)))
    return out


SPECS = all_specs()


@pytest.mark.parametrize("name,s,splits", SPECS, ids=[n for n, _, _ in SPECS])
def test_emulation_inside_and_planted_errors_outside(name, s, splits):
    a = make(s)
    R = ref(s, a)
    t = tol(s, R)
    assert np.isfinite(R["out"]).all() and (t > 0).all()
    worst, outs = 0.0, {}
    for order in ("seq", "pair16"):
        for S in splits:
            out = emulate(s, a, order, S)
            err = np.abs(out - R["out"])
            worst = max(worst, float((err / t).max()))
            assert (err <= t).all(), (order, S, float((err / t).max()), np.unravel_index(np.argmax(err / t), err.shape))
            outs.setdefault(order, out)
    print(f"{name}: emulation max err / tol = {worst:.3f}")
    # the accumulators once more for the planted runs (first split factor), so that a plant changes the epilogue only
    kc = s["K"] // splits[0]
    acc = None
    for i in range(splits[0]):
        p = _accumulate(a["x"][:, i * kc:(i + 1) * kc], a["w"][:, i * kc:(i + 1) * kc], "seq")
        acc = p if acc is None else acc + p
    plants = []
    if s["rpb"]:
        plants.append("gate_neighbour")
    if s["epi"] == GELU_FROM_COL:
        plants.append("gelu_shift4")
    if s["bias"]:
        plants.append("bias_shift")
    if s["M"] > 256:
        plants.append("tile_swap")
    for plant in plants:
        err = np.abs(emulate(s, a, "seq", acc=acc, plant=plant) - R["out"])
        n_out = int((err > t).sum())
        print(f"{name}: planted {plant}: {n_out} elements outside")
        assert n_out > 0, plant
        if plant == "gate_neighbour":  # every row next to a boundary shows it, and no other row does
            rows = np.unique(np.nonzero(err > t)[0])
            pos = rows % s["rpb"]
            assert ((pos == 0) | (pos == s["rpb"] - 1)).all()
            inner = [m for m in range(s["M"]) if (m % s["rpb"] == 0 and m > 0) or (m % s["rpb"] == s["rpb"] - 1 and m // s["rpb"] < s["nb"] - 1)]
            assert set(inner) <= set(rows.tolist())
        if plant == "gelu_shift4":
            cols = np.unique(np.nonzero(err > t)[1])
            assert cols.min() >= s["gelu_from"] and cols.max() < s["gelu_from"] + 4
    bad, i = plant_two_ulps(s, R, outs["seq"])
    assert abs(bad[i] - R["out"][i]) > t[i], ("two bf16 ulps", i, float(abs(bad[i] - R["out"][i])), float(t[i]))


def test_e4m3_values_match_the_oracle_table():
    from oracle import oracle as orc
    mine, theirs = e4m3_values().astype(np.float32), orc.e4m3_table()
    assert np.array_equal(np.isnan(mine), np.isnan(theirs)) and np.array_equal(mine[~np.isnan(mine)], theirs[~np.isnan(theirs)])


def test_tolerance_is_affine_in_c_and_reference_matches_the_oracle_linear():
    """tol(c) = tol(0) + c (tol(1) - tol(0)) (what the GPU test's error figure relies on), and the f64 reference agrees with the oracle's linear + GELU."""
    from oracle import oracle as orc
    s = CASES["gelu_from_384"][0]
    a = make(s)
    R = ref(s, a)
    t0, t1, t2 = tol(s, R, 0.0), tol(s, R, 1.0), tol(s, R, 2.0)
    assert np.allclose(t2, t0 + 2 * (t1 - t0), rtol=1e-12, atol=0)
    y = orc.linear(a["x"], a["w"], a["bias"])
    want = np.where(np.arange(s["N"])[None, :] >= s["gelu_from"], orc.gelu(y), y)
    assert np.abs(want - R["out"]).max() <= 1e-5
