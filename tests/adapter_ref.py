"""Shared by the adapter tests (tests/test_host_adapters.py, tests/test_gpu_adapters.py): a numpy float64 restatement of the four Delta formulas of
include/flux_mi355x.h (LoRA, LoHa, LoKr / full difference, DoRA) and of W = W0 + sum weight * Delta, the bound the exactness tests hold the GPU to, and
one adapter of every kind in the kohya and the diffusers key layouts (in the style of tests/lora_util.py).  The formulas are the issue's, written from
memory of PEFT / LyCORIS / ComfyUI: this file restates them independently of the kernels, it does not compare with those libraries."""
import numpy as np

from tests.lora_util import D, M

KINDS = ("lora", "loha", "lokr", "dora")
ERR_REL = 2.0 ** -40  # of mag: covers the f64 evaluation order and DoRA's K <= 1280 row sums (K * 2^-53 < 2^-42)


def f64(x):
    """A factor as float64 (numpy array or torch tensor of F32 / F16 / BF16: exact)."""
    if isinstance(x, np.ndarray):
        return x.astype(np.float64)
    return x.double().cpu().numpy()


def bf16_rne64(x):
    """float64 -> the nearest bf16 value (ties to even), in ONE rounding; as float64."""
    x = np.asarray(x, np.float64)
    q = np.ldexp(1.0, np.frexp(x)[1] - 8)  # |x| = m 2^e, m in [0.5, 1): 8 significant bits -> a grid of 2^(e - 8)
    return np.rint(x / q) * q


def term_delta(term, w0):
    """Delta (out, in) in float64 of one term (kind, tensors, scale, row_offset: diffusion_rs_amd.lora.AdapterTerm or anything shaped like it) on the
    Linear with pristine weight w0 (float64, the bf16 values).  scale is the f32 value that crosses the C ABI."""
    s = np.float64(np.float32(term.scale))
    t = term.tensors
    out, kin = w0.shape
    if term.kind == "lora":
        return s * (f64(t[1]) @ f64(t[0]))
    if term.kind == "loha":
        return s * ((f64(t[0]) @ f64(t[1])) * (f64(t[2]) @ f64(t[3])))
    if term.kind == "lokr":
        w1 = f64(t[0]) if t[1] is None else f64(t[0]) @ f64(t[1])
        w2 = f64(t[2]) if t[3] is None else f64(t[2]) @ f64(t[3])
        assert w1.shape[1] * w2.shape[1] == kin and term.row_offset + out <= w1.shape[0] * w2.shape[0]
        return s * np.kron(w1, w2)[term.row_offset:term.row_offset + out]
    if term.kind == "dora":
        v = w0 + s * (f64(t[1]) @ f64(t[0]))
        n = np.sqrt(np.sum(v * v, axis=1))
        return f64(t[2]).reshape(-1)[:, None] * v / n[:, None] - w0
    raise ValueError(term.kind)


def merge_ref(w0, terms):
    """(target, mag): target = W0 + sum weight * Delta and mag = |W0| + sum |weight * Delta| in float64; terms = [(weight, term)] in summation order
    (weight as the f32 value that crosses the C ABI; weight 0 terms are skipped, as the library skips them)."""
    w0 = np.asarray(w0, np.float64)
    t, mag = w0.copy(), np.abs(w0)
    for weight, term in terms:
        if weight == 0:
            continue
        d = np.float64(np.float32(weight)) * term_delta(term, w0)
        t, mag = t + d, mag + np.abs(d)
    return t, mag


def undecided(t, mag):
    """The elements whose bf16 rounding the bound leaves open: bf16_rne(t - err) != bf16_rne(t + err), err = 2^-40 mag.  Depends on the reference only."""
    err = ERR_REL * mag
    return bf16_rne64(t - err) != bf16_rne64(t + err)


def assert_within_bound(got, t, mag, what="", cap=4):
    """THE bound of the exactness tests: every decided element equals bf16_rne(t) bit for bit (as values: bf16 -> float64 is exact), an undecided one is
    one of the two bf16 neighbours of t, and at most `cap` are undecided (a condition on the inputs).  Returns the undecided count."""
    got = np.asarray(got, np.float64)
    err = ERR_REL * mag
    lo, hi = bf16_rne64(t - err), bf16_rne64(t + err)
    und = lo != hi
    n_und = int(und.sum())
    off = (got != bf16_rne64(t)) & ~und
    far = und & (got != lo) & (got != hi)
    print(f"{what}: {got.size} elements, {n_und} undecided, {int(off.sum())} decided elements off, {int(far.sum())} undecided elements not a neighbour")
    assert n_und <= cap, (what, n_und)
    assert not off.any(), (what, int(off.sum()), np.argwhere(off)[:4].tolist())
    assert not far.any(), (what, int(far.sum()))
    return n_und


class Term:
    """A stand-in for diffusion_rs_amd.lora.AdapterTerm (so that this file imports without the feature)."""

    def __init__(self, kind, tensors, scale=1.0, row_offset=0):
        self.kind, self.tensors, self.scale, self.row_offset = kind, tuple(tensors), float(scale), int(row_offset)


def random_term(kind, rng, out, kin, rank, scale=1.0, w0=None, std=None, lokr=None):
    """One term of `kind` for an (out, kin) Linear at the operand magnitudes of the LoRA tests (|Delta| of the order of |W0| ~ 0.02), float32 values.
    lokr = dict(a, b, c, d, r1=None, r2=None, row_offset=0): w1 (a, b) / w2 (c, d), decomposed at rank r1 / r2 when given."""
    def nrm(shape, s):
        return (s * rng.standard_normal(shape)).astype(np.float32)

    if kind == "lora":
        s = std or 0.05
        return Term("lora", (nrm((rank, kin), s), nrm((out, rank), s)), scale)
    if kind == "loha":
        s = std or 0.15  # each rank sum ~ s^2 sqrt(r), their product of the order of 1e-2
        return Term("loha", (nrm((out, rank), s), nrm((rank, kin), s), nrm((out, rank), s), nrm((rank, kin), s)), scale)
    if kind == "dora":
        s = std or 0.05
        A, B = nrm((rank, kin), s), nrm((out, rank), s)
        base = np.sqrt(np.sum(np.asarray(w0, np.float64) ** 2, axis=1)) if w0 is not None else np.full(out, 0.3)
        m = (base * (1.0 + 0.1 * rng.standard_normal(out))).astype(np.float32)  # near the row norms of W0: the update stays of the order of W0
        return Term("dora", (A, B, m), scale)
    if kind == "lokr":
        k = lokr
        r1, r2 = k.get("r1"), k.get("r2")
        w1 = (nrm((k["a"], k["b"]), 0.2), None) if r1 is None else (nrm((k["a"], r1), 0.4), nrm((r1, k["b"]), 0.4))
        w2 = (nrm((k["c"], k["d"]), 0.1), None) if r2 is None else (nrm((k["c"], r2), 0.3), nrm((r2, k["d"]), 0.3))
        return Term("lokr", w1 + w2, scale, k.get("row_offset", 0))
    raise ValueError(kind)


# every kohya module kind of tests/lora_util.peft_and_kohya on double block 0 and single block 1: (kohya name, rows, in, alpha, targets, row split)
_B0, _S1 = "transformer_blocks.0.", "single_transformer_blocks.1."
MODULES = [
    ("lora_unet_double_blocks_0_img_attn_qkv", 3 * D, D, 8.0, [_B0 + "attn.to_q", _B0 + "attn.to_k", _B0 + "attn.to_v"], [D, D, D]),
    ("lora_unet_double_blocks_0_txt_attn_qkv", 3 * D, D, 1.5, [_B0 + "attn.add_q_proj", _B0 + "attn.add_k_proj", _B0 + "attn.add_v_proj"], [D, D, D]),
    ("lora_unet_double_blocks_0_img_attn_proj", D, D, None, [_B0 + "attn.to_out.0"], [D]),
    ("lora_unet_double_blocks_0_txt_attn_proj", D, D, 4.0, [_B0 + "attn.to_add_out"], [D]),
    ("lora_unet_double_blocks_0_img_mlp_0", M, D, 2.0, [_B0 + "ff.net.0.proj"], [M]),
    ("lora_unet_double_blocks_0_img_mlp_2", D, M, 2.0, [_B0 + "ff.net.2"], [D]),
    ("lora_unet_double_blocks_0_txt_mlp_0", M, D, 2.0, [_B0 + "ff_context.net.0.proj"], [M]),
    ("lora_unet_double_blocks_0_txt_mlp_2", D, M, 2.0, [_B0 + "ff_context.net.2"], [D]),
    ("lora_unet_double_blocks_0_img_mod_lin", 6 * D, D, 6.0, [_B0 + "norm1.linear"], [6 * D]),
    ("lora_unet_double_blocks_0_txt_mod_lin", 6 * D, D, 6.0, [_B0 + "norm1_context.linear"], [6 * D]),
    ("lora_unet_single_blocks_1_linear1", 3 * D + M, D, 16.0, [_S1 + "attn.to_q", _S1 + "attn.to_k", _S1 + "attn.to_v", _S1 + "proj_mlp"], [D, D, D, M]),
    ("lora_unet_single_blocks_1_linear2", D, D + M, 1.0, [_S1 + "proj_out"], [D]),
    ("lora_unet_single_blocks_1_modulation_lin", 3 * D, D, None, [_S1 + "norm.linear"], [3 * D]),
]
LOKR_C = 64  # rows of w2 in adapter_files' LoKr modules: every part of a fused module starts on a multiple of it, so the diffusers layout can state the part


def adapter_files(kind, seed=0, rank=4, sd=None, modules=None):
    """One adapter of `kind` ("lora", "loha", "lokr", "dora" or "diff") on every module of MODULES, in both layouts:
    (diffusers dict, kohya dict, {prefix: Term}) with float32 numpy values.  want holds the terms the KOHYA file reads as; the diffusers file reads as the
    same terms except for the parts of a fused LoKr module, where it holds the part's own rows of w1 (row_offset 0): the same Delta, another term.
    sd: the model's state dict, for DoRA magnitudes near the row norms of the loaded weights."""
    rng = np.random.default_rng(seed)
    peft, kohya, want = {}, {}, {}
    for mi, (kname, rows, kin, alpha, targets, split) in enumerate(MODULES if modules is None else modules):
        r = rank if mi % 3 else 3
        if kind == "lokr":
            r = min(r, 3)
        scale = 1.0 if alpha is None else alpha / r
        w0 = None
        if sd is not None:
            w0 = np.concatenate([np.asarray(sd[t + ".weight"], np.float32) for t in targets]).astype(np.float64)

        def put(suffixes, tensors, sliced, peft_suffixes=None):
            """tensors under kohya `suffixes`; the diffusers file gets them per target, rows [r0, r0 + n) of the ones in `sliced`"""
            for s, t in zip(suffixes, tensors):
                if t is not None:
                    kohya[kname + s] = t
            r0 = 0
            for tgt, n in zip(targets, split):
                key = "transformer." + tgt if (len(peft) // 2) % 2 else tgt  # the optional "transformer." prefix on about every other Linear
                for i, (s, t) in enumerate(zip(peft_suffixes or suffixes, tensors)):
                    if t is not None:
                        peft[key + s] = t[r0:r0 + n] if i in sliced else t
                r0 += n

        if alpha is not None and kind != "diff":
            put([".alpha"], [np.float32(alpha)], ())
        if kind in ("lora", "dora"):
            t = random_term(kind, rng, rows, kin, r, scale, w0=w0)
            A, B = t.tensors[:2]
            put([".lora_down.weight", ".lora_up.weight"], [A, B], (1,), [".lora_A.weight", ".lora_B.weight"])
            if kind == "dora":
                m = t.tensors[2]
                put([".dora_scale"], [m.reshape(-1, 1)], (0,), [".lora_magnitude_vector" + (".weight" if mi % 2 else "")])
                # (the diffusers file stores (n,) vectors: PEFT's shape)
                for k in [k for k in peft if ".lora_magnitude_vector" in k]:
                    peft[k] = peft[k].reshape(-1)
            r0 = 0
            for tgt, n in zip(targets, split):
                want[tgt] = Term(kind, (A, B[r0:r0 + n]) + ((t.tensors[2][r0:r0 + n],) if kind == "dora" else ()), scale)
                r0 += n
        elif kind == "loha":
            t = random_term("loha", rng, rows, kin, r, scale)
            put([".hada_w1_a", ".hada_w1_b", ".hada_w2_a", ".hada_w2_b"], list(t.tensors), (0, 2))
            r0 = 0
            for tgt, n in zip(targets, split):
                x = t.tensors
                want[tgt] = Term("loha", (x[0][r0:r0 + n], x[1], x[2][r0:r0 + n], x[3]), scale)
                r0 += n
        elif kind == "diff":
            diff = (0.01 * rng.standard_normal((rows, kin))).astype(np.float32)
            put([".diff"], [diff], (0,))
            r0 = 0
            for tgt, n in zip(targets, split):
                want[tgt] = Term("lokr", (np.ones((1, 1), np.float32), None, diff[r0:r0 + n], None), 1.0)
                r0 += n
        elif kind == "lokr":
            # w1 (rows / 64, 16), w2 (64, in / 16); the variants rotate over the modules: both full (scale 1, alpha ignored), w2 decomposed, w1 decomposed
            variant = mi % 3
            shape = dict(a=rows // LOKR_C, b=16, c=LOKR_C, d=kin // 16, r1=r if variant == 2 else None, r2=r if variant == 1 else None)
            lscale = 1.0 if variant == 0 else scale
            t = random_term("lokr", rng, rows, kin, r, lscale, lokr=shape)
            w1a, w1b, w2a, w2b = t.tensors
            names = [".lokr_w1" if w1b is None else ".lokr_w1_a", ".lokr_w1_b", ".lokr_w2" if w2b is None else ".lokr_w2_a", ".lokr_w2_b"]
            for s, x in zip(names, t.tensors):
                if x is not None:
                    kohya[kname + s] = x
            r0 = 0
            for tgt, n in zip(targets, split):
                key = "transformer." + tgt if (len(peft) // 2) % 2 else tgt
                for s, x in zip(names, (w1a[r0 // LOKR_C:(r0 + n) // LOKR_C], w1b, w2a, w2b)):  # the part's own rows of w1 (or of w1_a)
                    if x is not None:
                        peft[key + s] = x
                want[tgt] = Term("lokr", t.tensors, lscale, r0)
                r0 += n
        else:
            raise ValueError(kind)
    return peft, kohya, want
