"""The d = 64 MFMA attention: ops.sdpa_d64 against a float64 softmax attention on the same bf16 inputs, and the T5 / CLIP text / CLIP vision
encoders under fmi_set_encoder_attention(1) against their oracles at the bars their own tests state.

The op's bound is 1.5 x what the encoders' lane-per-key kernel (enc_attention_kernel) measures against the same float64 reference on the same kind of inputs
(B, H = 2, 3, randn bf16, scale 1 / 8, no bias, not causal, Tq = Tk), by key count — OLD_KERNEL below, profiles/encoder_attention.txt.  Measured on an MI355X,
the MFMA kernel on the same inputs: rel-L2 1.25 .. 1.31 x the old kernel's (it rounds P to bf16 once, the old kernel sums f32 P; both round the output to
bf16), max-abs 1.0 .. 1.25 x.

rel-L2: every case, bias and causal ones included, is held to 1.5 x the old kernel's figure at its key count.
max-abs: the cases that ARE the old kernel's measured inputs (square, no bias, not causal) are held to 1.5 x its figure.  For the others an absolute figure taken
on other inputs says nothing: the max-abs of a bf16 output is half an ulp of its largest values, and those differ from case to case — a causal row's first
outputs are single V rows (|o| up to ~4, half an ulp 7.8e-3) where a 512-key average stays below 0.6 (the old kernel's 9.7e-4); the float64 result ROUNDED TO
BF16 would miss 1.5 x 9.7e-4 by a factor of five.  Those cases are held to 1.5 x the max-abs of exactly that best possible bf16 answer, computed in the test:
the format's own precision, with the same factor."""
import numpy as np
import pytest

from tests.util import host, rel_l2

pytestmark = pytest.mark.gpu

# Tk: (rel-L2, max-abs) of enc_attention_kernel against float64 at Tq = Tk, the inputs of _qkv(Tk, Tk, 1001 Tk), measured on an MI355X (profiles/encoder_attention.txt)
OLD_KERNEL = {1: (0.0, 0.0), 64: (1.6542e-03, 3.6616e-03), 65: (1.6649e-03, 1.9514e-03), 77: (1.6532e-03, 3.6146e-03), 257: (1.6554e-03, 1.9366e-03),
              512: (1.6669e-03, 9.6509e-04)}
SHAPES = [(1, 1), (16, 64), (77, 77), (64, 65), (130, 257), (512, 512)]
CASES = [(Tq, Tk, with_bias, causal) for Tq, Tk in SHAPES for with_bias in (False, True) for causal in (False, True) if Tq == Tk or not causal]
B, H = 2, 3


def _qkv(Tq, Tk, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn((B, T, H, 64), generator=g).to(torch.bfloat16).cuda() for T in (Tq, Tk, Tk))
    return q, k, v


def _bias(Tq, Tk, seed):
    """An f32 bias with a relative-position slope, and in row 0 of every head a key of the LAST tile that beats everything before it by far more than
    2^6 ln 2 = 44.4: that row's maximum moves in a later tile and everything accumulated before it is rescaled by ~0."""
    import torch
    g = torch.Generator().manual_seed(seed)
    bias = torch.randn((H, Tq, Tk), generator=g) * 2.0 - 0.01 * (torch.arange(Tq)[:, None] - torch.arange(Tk)[None, :]).abs()
    bias[:, 0, Tk - 1] += 100.0
    return bias.float().cuda()


def _reference(q, k, v, bias, causal, scale):
    import torch
    q, k, v = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias.double()[None]
    if causal:
        s = s.masked_fill(torch.ones(s.shape[-2:], dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).cpu().numpy()


def _check(got, want, Tk, what, old_inputs=False, any_tk=False):
    """any_tk: a key count the old kernel was not measured at is held to the largest rel-L2 figure of OLD_KERNEL (the table is flat in Tk, 1.653e-3 ..
    1.667e-3: the bf16 rounding of the output dominates), and to the max-abs rule of inputs the old kernel was not measured on."""
    import torch
    got = host(got.float()).astype(np.float64)
    err, mx = rel_l2(got, want), float(np.abs(got - want).max())
    if any_tk and Tk not in OLD_KERNEL:
        assert not old_inputs
        old_err, old_mx = max(e for e, _ in OLD_KERNEL.values()), float("nan")
    else:
        old_err, old_mx = OLD_KERNEL[Tk]
    best = float(np.abs(torch.from_numpy(want).to(torch.bfloat16).double().numpy() - want).max())  # the float64 result rounded to bf16
    mx_bound = 1.5 * (old_mx if old_inputs else best)
    print(f"sdpa_d64 {what}: rel-L2 {err:.3e} (bound {1.5 * old_err:.3e}), max-abs {mx:.3e} (bound {mx_bound:.3e}; the old kernel {old_mx:.3e}, the best bf16 answer {best:.3e})")
    assert np.isfinite(got).all() and err <= 1.5 * old_err and mx <= mx_bound


@pytest.mark.parametrize("Tq,Tk,with_bias,causal", CASES)
def test_op_against_float64(Tq, Tk, with_bias, causal):
    import diffusion_rs_amd as d
    q, k, v = _qkv(Tq, Tk, seed=Tq * 1000 + Tk)
    bias = _bias(Tq, Tk, seed=7) if with_bias else None
    got = d.ops.sdpa_d64(q, k, v, bias=bias, causal=causal)
    _check(got, _reference(q, k, v, bias, causal, 0.125), Tk, f"Tq={Tq} Tk={Tk} bias={with_bias} causal={causal}", old_inputs=Tq == Tk and not with_bias and not causal)


@pytest.mark.parametrize("layout", ["fused", "odd_offset"])
def test_op_reads_strided_and_unaligned_operands(layout):
    """fused: q, k, v are the thirds of a (B, T, 3 H 64) projection, read where they lie (the LDS-DMA form); odd_offset: the same views one element into a
    buffer, so nothing is 16-byte aligned (the 2-byte-load form).  T5's convention: scale 1, with a bias."""
    import torch
    import diffusion_rs_amd as d
    T = 257
    g = torch.Generator().manual_seed(11)
    flat = (torch.randn(B * T * 3 * H * 64 + 1, generator=g) * 0.35).to(torch.bfloat16).cuda()
    qkv = flat[1:] if layout == "odd_offset" else flat[:-1]
    q, k, v = qkv.view(B, T, 3, H, 64).unbind(2)
    bias = _bias(T, T, seed=5)
    got = d.ops.sdpa_d64(q, k, v, bias=bias, scale=1.0)
    _check(got, _reference(q, k, v, bias, False, 1.0), 257, layout)


def test_op_refuses_bad_arguments():
    import torch
    import diffusion_rs_amd as d
    from diffusion_rs_amd import _lib as L
    q, k, v = _qkv(4, 4, 0)
    with pytest.raises(TypeError, match="bias must be a float32"):
        d.ops.sdpa_d64(q, k, v, bias=torch.zeros((H, 4, 5), device="cuda"))
    with pytest.raises(ValueError, match="do not fit"):
        d.ops.sdpa_d64(q, k[:, :, :2], v)
    lib = L.load()
    p = lambda t: t.data_ptr()
    assert lib.fmi_sdpa_d64_bf16(p(q), p(k), p(v), p(q), B, H, 0, 4, None, 1.0, None, 0, None) == L.ERR_INVALID
    assert lib.fmi_sdpa_d64_bf16(p(q), None, p(v), p(q), B, H, 4, 4, None, 1.0, None, 0, None) == L.ERR_INVALID
    assert lib.fmi_sdpa_bf16(p(q), p(q), p(q), p(q), 1, 1, 4, 4, 64, 1.0, 0, None) == L.ERR_UNSUPPORTED  # the d = 128 seam keeps refusing d = 64


@pytest.fixture
def mfma_encoders():
    import diffusion_rs_amd as d
    d.set_encoder_attention("mfma")
    yield d
    d.set_encoder_attention("default")


@pytest.mark.parametrize("T", [300, 1030])
def test_t5_under_the_switch(T):
    """T5's small tower against the oracle (rel-L2 <= 1e-2, tests/test_gpu_text.py); 1030 tokens are past the lane-per-key kernel's 1024: refused under
    "default", the oracle's output under "mfma"."""
    import torch
    import diffusion_rs_amd as d
    from tests.test_gpu_text import SMALL_T5, _pair
    _, gm, om, _ = _pair("t5", dict(SMALL_T5, num_layers=2))
    ids = np.random.default_rng(T).integers(0, SMALL_T5["vocab_size"], (1, T)).astype(np.int32)
    try:
        if T > 1024:
            with pytest.raises(d.FmiError, match="sequence longer than 1024"):
                gm.forward(ids, dtype=torch.float32)
        d.set_encoder_attention("mfma")
        err = rel_l2(host(gm.forward(ids, dtype=torch.float32)), om.forward(ids))
    finally:
        d.set_encoder_attention("default")
    print(f"T5 under mfma, T={T}: rel-L2 {err:.3e}")
    assert err <= 1e-2


def test_clip_text_under_the_switch(mfma_encoders):
    from tests.test_gpu_text import SMALL_CLIP, _pair
    _, gm, om, _ = _pair("clip", SMALL_CLIP)
    ids = np.random.default_rng(0).integers(1, SMALL_CLIP["vocab_size"] - 1, (3, 77)).astype(np.int32)
    ids[:, 60] = SMALL_CLIP["vocab_size"] - 1
    (rp, rh), (gp, gh) = om.forward(ids, return_hidden=True), gm.forward(ids, return_hidden=True)
    print(f"CLIP text under mfma: pooled rel-L2 {rel_l2(host(gp), rp):.3e}, hidden {rel_l2(host(gh), rh):.3e}")
    assert rel_l2(host(gh), rh) <= 1e-2 and rel_l2(host(gp), rp) <= 1e-2


def test_clip_vision_under_the_switch(mfma_encoders):
    from tests import clip_vision_ref as R
    name = list(R.CONFIGS)[0]
    cfg = dict(R.CONFIGS[name])
    m = mfma_encoders.ClipVisionModel(cfg)
    m.load_state_dict(R.state_dict(cfg))
    want_e, want_h = R.reference(name, 3)
    got_e, got_h = m.forward(R.pixel_values(cfg, 3), return_hidden=True)
    print(f"CLIP vision {name} under mfma: image_embeds rel-L2 {rel_l2(host(got_e), want_e):.3e}, hidden {rel_l2(host(got_h), want_h):.3e}")
    assert rel_l2(host(got_e), want_e) <= 1e-2 and rel_l2(host(got_h), want_h) <= 1e-2
    big = dict(cfg, image_size=cfg["patch_size"] * 32)  # 1025 tokens: refused at creation under "default" only
    mfma_encoders.ClipVisionModel(big).close()
