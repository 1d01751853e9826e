"""The GEMM launcher's epilogues, grouped launches and split-K reduce, element by element against the f64 reference of tests/test_gemm_reference.py
(reference, derived tolerance and case table live there, with their own CPU self-check), through the test seams fmi_gemm_group /
fmi_splitk_resid_gate / fmi_set_gemm_kernel.

Every case: bf16-exact inputs (x ~ N(0,1), w ~ N(0,1) / sqrt(K); 8-bit codes drawn in numpy), every output buffer with 3 guard rows and ldo - N guard
columns, bf16 outputs and plain f32 stores pre-filled with NaN, residual buffers with known finite values, unused parts of strided operands poisoned
with NaN.  After the launch every result element is inside tol(), everything outside [0, M) x [0, N) is bit-for-bit unchanged, and a second run
from the same state gives the same bits.  Each case prints the largest err / (|g| |alpha| K 2^-24 A) it saw (DESIGN.md 5 records the maximum over the
f32 results, bf16 and e4m3 operands apart; a bf16 result's figure is its output rounding)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import test_gemm_reference as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from diffusion_rs_amd import _lib as L
    lib = L.load()
    L.check(lib.fmi_init(0))
    alt = L.load_alt() if os.path.exists(L.ALT_LIB_PATH) else None
    e = dict(torch=torch, L=L, product=lib, alt=alt, worst_f32=(0.0, None), worst_bf16=(0.0, None), worst_e4m3=(0.0, None))
    yield e
    print(f"\n[gemm epilogues] largest err / (|g| |alpha| K 2^-24 A): f32 results of bf16 operands {e['worst_f32'][0]:.4f} ({e['worst_f32'][1]}), "
          f"of e4m3 operands {e['worst_e4m3'][0]:.3f} ({e['worst_e4m3'][1]}), "
          f"bf16 results {e['worst_bf16'][0]:.3f} ({e['worst_bf16'][1]}; output rounding)")


def _need_alt(env):
    if env["alt"] is None:
        pytest.skip("libflux_mi355x_alt.so not built (make alt)")
    return env["alt"]


# ---------------------------------------------------------------------------------------------------- device buffers of one problem
def _bits(t):
    torch_int = {2: "int16", 4: "int32", 1: "uint8"}[t.element_size()]
    import torch
    return t.view(getattr(torch, torch_int)).cpu().numpy().copy()


def _dev(torch, arr, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def build(torch, L, s, a):
    """Device buffers + descriptor of one problem.  Returns (desc, keep): keep holds the tensors (alive as long as the descriptor is used), the output tensor,
    its initial image and where the (M, N) result sits inside it."""
    M, N, K, q8, epi = s["M"], s["N"], s["K"], s["q8"], s["epi"]
    keep = {}
    if q8 == 0:
        xa = np.full((M, s["lda"]), np.nan, np.float32)
        xa[:, s["a_col0"]:s["a_col0"] + K] = a["x"]
        wa = np.full((N, s["ldw"]), np.nan, np.float32)
        wa[:, :K] = a["w"]
        keep["a"], keep["w"] = _dev(torch, xa, True), _dev(torch, wa, True)
        es = 2
    else:
        poison = 0x7f  # e4m3: NaN; int8: 127
        xa = np.full((M, s["lda"]), poison, np.uint8)
        xa[:, s["a_col0"]:s["a_col0"] + K] = a["xq"].view(np.uint8)
        wa = np.full((N, s["ldw"]), poison, np.uint8)
        wa[:, :K] = a["wq"].view(np.uint8)
        keep["a"], keep["w"] = _dev(torch, xa), _dev(torch, wa)
        es = 1
        for k in ("a_scale", "w_scale", "a_off", "w_sum"):
            if k in a:
                keep[k] = _dev(torch, a[k])
    if a["bias"] is not None:
        keep["bias"] = _dev(torch, np.concatenate([np.full(s["bias_off"], np.nan, np.float32), a["bias"], np.full(8, np.nan, np.float32)]), True)
    f32_out = epi in G.F32_OUT
    rows, ldo, off = M + 3, s["ldo"], s["out_off"]
    rng = np.random.default_rng(s["seed"] + 99)
    if epi == G.RESID_GATE_F32:
        img = rng.standard_normal(off + rows * ldo).astype(np.float32)  # known finite values, the guards included
        img[off:].reshape(rows, ldo)[:M, :N] = a["r0"]
        gb = np.full(max(s["nb"] - 1, 0) * s["gate_bstride"] + N + 4, np.nan, np.float32)
        for b in range(s["nb"]):
            gb[b * s["gate_bstride"]:b * s["gate_bstride"] + N] = a["gate"][b]
        keep["gate"] = _dev(torch, gb)
    else:
        img = np.full(off + rows * ldo, np.nan, np.float32)
    if epi == G.RESID_ADD_BF16:
        rb = np.full((rows, ldo), np.nan, np.float32)
        rb[:M, :N] = a["r0"]
        keep["resid"] = _dev(torch, rb, True)
    keep["init"] = _dev(torch, img, not f32_out)
    keep["out"] = keep["init"].clone()
    keep["f32_out"], keep["view"] = f32_out, (off, rows, ldo)
    p = lambda k, o=0: C.c_void_p(keep[k].data_ptr() + o) if k in keep else None  # noqa: E731
    d = L.GemmDesc(a=p("a", s["a_col0"] * es), w=p("w"), bias=p("bias", s["bias_off"] * 2), out=p("out", off * (4 if f32_out else 2)), gate=p("gate"),
                   resid=p("resid"), M=M, N=N, K=K, lda=s["lda"], ldw=s["ldw"], ldo=ldo, epi=epi, gelu_from=s["gelu_from"], alpha=s["alpha"],
                   rows_per_batch=s["rpb"], gate_bstride=s["gate_bstride"], q8=q8, a_scale=p("a_scale"), w_scale=p("w_scale"), a_off=p("a_off"),
                   w_sum=p("w_sum"))
    return d, keep


def launch(lib, L, descs):
    arr = (L.GemmDesc * len(descs))(*descs)
    return lib.fmi_gemm_group(arr, len(descs), None)


def region(keep, s, flat):
    off, rows, ldo = keep["view"]
    return flat[off:off + rows * ldo].reshape(rows, ldo)[:s["M"], :s["N"]]


def outside_mask(keep, s, n):
    off, rows, ldo = keep["view"]
    m = np.ones(n, bool)
    m[off:off + rows * ldo].reshape(rows, ldo)[:s["M"], :s["N"]] = False
    return m


_REF = {}


def reference(name, specs):
    """f64 reference and tolerance of a case's problems: computed once, shared by every test of the case, never modified."""
    if name not in _REF:
        out = []
        for s in specs:
            a = G.make(s)
            R = G.ref(s, a)
            t = G.tol(s, R)
            for arr in list(R.values()) + [t]:
                arr.setflags(write=False)
            out.append((a, R, t))
        _REF[name] = out
    return _REF[name]


_RUN = {}


def run_case(env, libname, mode, name):
    """One grouped launch of CASES[name] on a library with a kernel choice (pingpong, w4), twice from the same state.  Cached: the kernel twins compare
    with what the plain run left."""
    key = (libname, mode, name)
    if key in _RUN:
        return _RUN[key]
    torch, L, lib = env["torch"], env["L"], env[libname]
    specs = G.CASES[name]
    refs = reference(name, specs)
    built = [build(torch, L, s, a) for s, (a, _, _) in zip(specs, refs)]
    descs = [d for d, _ in built]
    runs = []
    try:
        if mode != (1, 0):
            L.check(lib.fmi_set_gemm_kernel(*mode), lib)
        for _ in range(2):
            for _, keep in built:
                keep["out"].copy_(keep["init"])
            torch.cuda.synchronize()
            L.check(launch(lib, L, descs), lib)
            torch.cuda.synchronize()
            runs.append([_bits(keep["out"]) for _, keep in built])
    finally:
        if mode != (1, 0):
            lib.fmi_set_gemm_kernel(1, 0)
    res = dict(specs=specs, refs=refs, keeps=[k for _, k in built], first=runs[0], second=runs[1],
               vals=[keep["out"].float().cpu().numpy().astype(np.float64) for _, keep in built], init=[_bits(keep["init"]) for _, keep in built])
    for _, keep in built:  # the device buffers are not needed again
        for k in [k for k in keep if hasattr(keep[k], "data_ptr")]:
            del keep[k]
    _RUN[key] = res
    return res


def check_problem(env, label, s, R, t, keep, vals, init_bits, first_bits, second_bits):
    got = region(keep, s, vals)
    assert np.isfinite(got).all(), f"{label}: non-finite result"
    err = np.abs(got - R["out"])
    ratio = float(G.acc_ratio(s, R, err).max())
    which = ("worst_e4m3" if s["q8"] == 1 else "worst_f32") if keep["f32_out"] else "worst_bf16"
    if s["q8"] != 2 and ratio > env[which][0]:
        env[which] = (ratio, label)
    print(f"{label}: max err / tol = {float((err / t).max()):.3f}, max err / (|g| |alpha| K 2^-24 A) = {ratio:.4f}")
    bad = err > t
    assert not bad.any(), (label, int(bad.sum()), "first at", tuple(int(i) for i in np.argwhere(bad)[0]), "rows", np.unique(np.nonzero(bad)[0])[:8],
                           "cols", np.unique(np.nonzero(bad)[1])[:8], float((err / t).max()))
    out = outside_mask(keep, s, first_bits.size)
    assert np.array_equal(first_bits[out], init_bits[out]), f"{label}: wrote outside [0, M) x [0, N)"
    assert np.array_equal(first_bits, second_bits), f"{label}: second run differs"


# ---------------------------------------------------------------------------------------------------- the case table, on both builds
@pytest.mark.parametrize("name", list(G.CASES))
@pytest.mark.parametrize("libname", ["product", "alt"])
def test_case_inside_tolerance_guards_untouched_deterministic(env, libname, name):
    if libname == "alt":
        _need_alt(env)
    r = run_case(env, libname, (1, 0), name)
    for i, s in enumerate(r["specs"]):
        _, R, t = r["refs"][i]
        check_problem(env, f"{libname}:{name}[{i}]", s, R, t, r["keeps"][i], r["vals"][i], r["init"][i], r["first"][i], r["second"][i])


def _dense_wide(name):
    return all(s["q8"] == 0 for s in G.CASES[name]) and max(s["N"] for s in G.CASES[name]) > 128


@pytest.mark.parametrize("name", [n for n in G.CASES if _dense_wide(n)])
def test_double_buffered_kernel_is_bit_identical(env, name):
    """GK_DB256 (test build, fmi_set_gemm_kernel(0, 0)) against the product library's ping-pong kernel."""
    _need_alt(env)
    a, b = run_case(env, "product", (1, 0), name), run_case(env, "alt", (0, 0), name)
    for i in range(len(a["specs"])):
        assert np.array_equal(a["first"][i], b["first"][i]) and np.array_equal(b["first"][i], b["second"][i]), (name, i)


@pytest.mark.parametrize("name", [n for n in G.CASES if _dense_wide(n) and all(s["epi"] == G.RESID_GATE_F32 for s in G.CASES[n])])
def test_four_wave_kernel_is_bit_identical(env, name):
    """GK_W4 (test build, fmi_set_gemm_kernel(1, 1): the residual-update launches) against the product library's ping-pong kernel."""
    _need_alt(env)
    a, b = run_case(env, "product", (1, 0), name), run_case(env, "alt", (1, 1), name)
    for i in range(len(a["specs"])):
        assert np.array_equal(a["first"][i], b["first"][i]) and np.array_equal(b["first"][i], b["second"][i]), (name, i)


# ---------------------------------------------------------------------------------------------------- split-K: grouped strided parts, then the reduce
@pytest.mark.parametrize("name,S", [(n, S) for n, (_, Ss) in G.SPLITK_CASES.items() for S in Ss])
@pytest.mark.parametrize("libname", ["product", "alt"])
def test_split_k_parts_and_reduce(env, libname, name, S):
    if libname == "alt":
        _need_alt(env)
    torch, L, lib = env["torch"], env["L"], env[libname]
    specs = G.SPLITK_CASES[name][0]
    refs = reference(name, specs)
    built = [build(torch, L, s, a) for s, (a, _, _) in zip(specs, refs)]
    parts, descs = [], []
    for s, (d, keep) in zip(specs, built):
        kc = s["K"] // S
        pt = torch.full((S * s["M"] * s["N"],), float("nan"), dtype=torch.float32, device="cuda")
        parts.append(pt)
        for k in range(S):  # as gemm_split_k builds them: A and W advanced by k K / S columns, f32 parts, no bias, no gate
            descs.append(L.GemmDesc(a=C.c_void_p(keep["a"].data_ptr() + 2 * k * kc), w=C.c_void_p(keep["w"].data_ptr() + 2 * k * kc),
                                    out=C.c_void_p(pt.data_ptr() + 4 * k * s["M"] * s["N"]), M=s["M"], N=s["N"], K=kc, lda=s["lda"], ldw=s["ldw"],
                                    ldo=s["N"], epi=G.STORE_F32, alpha=1.0))
    runs = []
    for _ in range(2):
        for _, keep in built:
            keep["out"].copy_(keep["init"])
        torch.cuda.synchronize()
        L.check(launch(lib, L, descs), lib)
        for s, (d, keep), pt in zip(specs, built, parts):
            L.check(lib.fmi_splitk_resid_gate(C.c_void_p(pt.data_ptr()), S, d.bias, d.gate, s["rpb"], s["gate_bstride"], d.out, s["ldo"], s["M"], s["N"], None), lib)
        torch.cuda.synchronize()
        runs.append([_bits(keep["out"]) for _, keep in built])
    for i, (s, (d, keep)) in enumerate(zip(specs, built)):
        assert torch.isfinite(parts[i]).all()
        _, R, t = refs[i]
        check_problem(env, f"{libname}:{name}[{i}] S={S}", s, R, t, keep, keep["out"].cpu().numpy().astype(np.float64), _bits(keep["init"]), runs[0][i], runs[1][i])


# ---------------------------------------------------------------------------------------------------- rejections: host-side only, nothing launched
def _copy(L, d, **over):
    n = L.GemmDesc()
    C.memmove(C.byref(n), C.byref(d), C.sizeof(d))
    for k, v in over.items():
        setattr(n, k, v)
    return n


@pytest.mark.parametrize("libname", ["product", "alt"])
def test_rejections_before_any_launch(env, libname):
    if libname == "alt":
        _need_alt(env)
    torch, L, lib = env["torch"], env["L"], env[libname]
    sg, sb, sc, sr = (G.CASES[n][0] for n in ("gate_per_batch", "unaligned_out", "gelu_from_768", "resid_add_bf16"))
    (dg, kg), (db, kb), (dc, kc), (dr, kr) = (build(torch, L, s, G.make(s)) for s in (sg, sb, sc, sr))
    keeps = (kg, kb, kc, kr)
    bad = {
        "nine problems": [_copy(L, db)] * 9,
        "mixed activation kinds": [_copy(L, db), _copy(L, db, epi=G.GELU_BF16)],
        "gated residual without gate": [_copy(L, dg, gate=None)],
        "gate pointer off by one float": [_copy(L, dg, gate=dg.gate + 4)],
        "gate batch stride not a multiple of 4": [_copy(L, dg, gate_bstride=sg["gate_bstride"] + 2)],
        "residual add without resid": [_copy(L, dr, resid=None)],
        "gelu_from not a multiple of 4": [_copy(L, dc, gelu_from=770)],
        "negative rows_per_batch": [_copy(L, dg, rows_per_batch=-1)],
        "null operand": [_copy(L, db, a=None)],
        "lda below K": [_copy(L, db, lda=sb["K"] - 8)],
        "alpha where it is not read": [_copy(L, db, alpha=0.5)],
        "mixed 8-bit and bf16": [_copy(L, db), _copy(L, db, q8=1)],
    }
    for what, descs in bad.items():
        rc = launch(lib, L, descs)
        msg = lib.fmi_last_error()
        print(f"{what}: {rc} {msg.decode(errors='replace')}")
        assert rc == L.ERR_INVALID and len(msg) > 8, (what, rc, msg)
    rc = lib.fmi_splitk_resid_gate(dg.out, 2, None, None, 0, 0, dg.out, sg["ldo"], sg["M"], sg["N"], None)
    assert rc == L.ERR_INVALID and b"gate" in lib.fmi_last_error()
    if libname == "product":  # a kernel choice that needs the test build fails per launch, and the default works again afterwards
        try:
            for mode in ((0, 0), (1, 1)):
                assert lib.fmi_set_gemm_kernel(*mode) == 0
                rc = launch(lib, L, [dg])
                assert rc == L.ERR_UNSUPPORTED and b"test build" in lib.fmi_last_error(), (mode, rc)
        finally:
            lib.fmi_set_gemm_kernel(1, 0)
    torch.cuda.synchronize()
    for keep in keeps:
        assert np.array_equal(_bits(keep["out"]), _bits(keep["init"]))
    L.check(launch(lib, L, [dg]), lib)  # the untouched descriptor is accepted
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(kg["out"]), _bits(kg["init"]))
