"""The d = 64 MFMA attention (csrc/attention_d64.hip) without tolerances, next to tests/test_gpu_sdpa_d64.py's float64 comparison.

1. Routing.  Inputs whose softmax is exactly one-hot in the kernel's f32 arithmetic (tests/sdpa_d64_inputs.py, proved on the CPU by
   tests/test_host_sdpa_d64_inputs.py): out[b, i, h, :] must be v[b, pi[h, i], h, :] as 16-bit patterns.  A key that reaches the wrong query, lane, g group,
   key block or k-step, or a bias value read from the wrong place, delivers another V row.
2. Launch pairs that run the same arithmetic in the same order and differ in the loads or the trip count only: identical bits.
3. Stores: the output is a strided view into a buffer of sentinels; nothing outside the view changes.
4. The float64 comparison of the neighbouring file at the inputs it leaves out (its _reference and _check).
5. T5 under the "mfma" switch at the tile boundaries."""
import ctypes as C

import numpy as np
import pytest

from tests import sdpa_d64_inputs as I
from tests.test_gpu_sdpa_d64 import B, H, _bias, _check, _qkv, _reference
from tests.util import host, rel_l2

pytestmark = pytest.mark.gpu

assert (B, H) == (I.B, I.H)
SENTINEL = 0x7FC1  # a bf16 NaN pattern no arithmetic result carries


# ---------------------------------------------------------------- helpers

def _odd(t):
    """The same values one element into a fresh buffer: a bf16 tensor is then 2-byte aligned only, an f32 one 4-byte aligned only."""
    import torch
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


def _aligned(*ts):
    assert all(t.data_ptr() % 16 == 0 for t in ts if t is not None)
    return ts


def _launch(q, k, v, out, bias=None, causal=False, scale=0.125, strides=True):
    """fmi_sdpa_d64_bf16 itself, into a caller's `out` (any view); strides=False passes NULL (four contiguous tensors)."""
    import torch
    from diffusion_rs_amd import _lib as L
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = (C.c_int64 * 12)(*(int(t.stride(i)) for t in (q, k, v, out) for i in (0, 1, 2))) if strides else None
    L.check(L.load().fmi_sdpa_d64_bf16(p(q), p(k), p(v), p(out), q.shape[0], q.shape[2], q.shape[1], k.shape[1], st, float(scale), p(bias),
                                       1 if causal else 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu()


def _same_bits(a, b, what):
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype == torch.bfloat16
    ba, bb = _bits(a), _bits(b)
    if not torch.equal(ba, bb):
        bad = (ba != bb).nonzero()
        diff = (a.float().cpu() - b.float().cpu()).abs()
        pytest.fail(f"{what}: {len(bad)} of {ba.numel()} elements differ, first at (b, i, h, c) = {tuple(bad[0].tolist())}: {a[tuple(bad[0])].item()!r} against "
                    f"{b[tuple(bad[0])].item()!r}; largest difference {float(diff.nan_to_num(nan=float('inf')).max()):.3e}")


def _plain_bias(Tq, Tk, seed):
    """The neighbouring file's kind of bias (random, with a relative-position slope) without its +100 spike."""
    import torch
    g = torch.Generator().manual_seed(seed)
    bias = torch.randn((H, Tq, Tk), generator=g) * 2.0 - 0.01 * (torch.arange(Tq)[:, None] - torch.arange(Tk)[None, :]).abs()
    return bias.float().cuda()


def _future(Tq, Tk):
    import torch
    return torch.ones((Tq, Tk), dtype=torch.bool, device="cuda").triu(1)


# ---------------------------------------------------------------- 1. routing

def _expect_rows(out, v, pi, what):
    """out (B, Tq, H, 64) must be v[b, pi[h, i], h, :] bit for bit; the message names the first wrong row and where its bits came from."""
    import torch
    out_bits, v_bits = _bits(out), _bits(v)
    want = v_bits.permute(0, 2, 1, 3).gather(2, pi[None, :, :, None].expand(B, H, pi.shape[1], 64)).permute(0, 2, 1, 3)
    if torch.equal(out_bits, want):
        return
    wrong = (out_bits != want).any(-1).nonzero()
    b, i, h = wrong[0].tolist()
    row = out_bits[b, i, h]
    hit = (v_bits == row).all(-1).nonzero()
    if len(hit):
        b2, j2, h2 = hit[0].tolist()
        came = f"it holds V row (b, key, h) = ({b2}, {j2}, {h2})"
    else:
        ch = (row != want[b, i, h]).nonzero().flatten().tolist()
        came = f"no V row matches; channels {ch} differ: {out[b, i, h].float().cpu()[ch].tolist()} against {v[b, int(pi[h, i]), h].float().cpu()[ch].tolist()}"
    pytest.fail(f"{what}: {len(wrong)} of {B * pi.shape[1] * H} rows wrong, first (b, i, h) = ({b}, {i}, {h}), expected key {int(pi[h, i])}; {came}")


def _run_layout(layout, q, k, v, bias, causal, scale):
    """aligned: ops.sdpa_d64 on fresh tensors (the LDS-DMA kernel, the float4 bias reads where Tk % 4 == 0); odd: q, k, v, the bias and the output one
    element into their buffers (the 2-byte kernel, scalar bias reads)."""
    import torch
    import diffusion_rs_amd as d
    q, k, v, bias = (t.cuda() if t is not None else None for t in (q, k, v, bias))
    if layout == "aligned":
        _aligned(q, k, v, bias)
        return d.ops.sdpa_d64(q, k, v, bias=bias, causal=causal, scale=scale), v
    q, k, v = _odd(q), _odd(k), _odd(v)
    out = _odd(torch.zeros((B, q.shape[1], H, 64), dtype=torch.bfloat16, device="cuda"))
    return _launch(q, k, v, out, _odd(bias) if bias is not None else None, causal, scale), v


ROUTING = [c + ("aligned",) for c in I.ROUTING_CASES] + [c + ("odd",) for c in I.ROUTING_CASES if c[:2] in I.ODD_OFFSET_SHAPES]


def _routing_id(case):
    Tq, Tk, name, causal, layout = case
    return f"{Tq}x{Tk}-{name}-{'causal' if causal else 'full'}-{layout}"


@pytest.mark.parametrize("case", ROUTING, ids=_routing_id)
def test_routing_through_qk(case):
    """Builder (a): the query carries the code of its key; pins K staging (the swizzle on the fetch side and on the read side), the Q fragments and the
    key order inside the MFMA result, then the V transpose and the P V operand order."""
    Tq, Tk, name, causal, layout = case
    pi = I.key_map(name, Tq, Tk, causal)
    q, k, scale = I.select_by_qk(Tq, Tk, pi)
    out, v = _run_layout(layout, q, k, I.values(Tk, seed=Tk), None, causal, scale)
    _expect_rows(out, v, pi, f"selection through Q K, {_routing_id(case)}")


@pytest.mark.parametrize("case", ROUTING, ids=_routing_id)
def test_routing_through_the_bias(case):
    """Builder (b): bias[h, i, pi[h, i]] = 1000 selects; pins the bias indexing on the float4 path (aligned, Tk % 4 == 0) and on the scalar one."""
    Tq, Tk, name, causal, layout = case
    pi = I.key_map(name, Tq, Tk, causal)
    q, k, scale, bias = I.select_by_bias(Tq, Tk, pi, seed=Tq + Tk)
    out, v = _run_layout(layout, q, k, I.values(Tk, seed=Tk), bias, causal, scale)
    _expect_rows(out, v, pi, f"selection through the bias, {_routing_id(case)}")


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("Tq,Tk", I.LADDER_SHAPES)
def test_routing_with_a_maximum_that_moves_in_every_tile(Tq, Tk, layout):
    """Each of the four tiles holds a key 300 above the best of the tile before: every row rescales what it has by exactly 0 three times over, and the
    output is still one V row, the last tile's."""
    bias, pi = I.ladder_bias(Tq, Tk)
    q, k, scale, _ = I.select_by_bias(Tq, Tk, pi, seed=3)
    out, v = _run_layout(layout, q, k, I.values(Tk, seed=Tk), bias, False, scale)
    _expect_rows(out, v, pi, f"ladder bias {Tq}x{Tk} {layout}")


# ---------------------------------------------------------------- 2. launch pairs that must agree bit for bit

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("T", [257, 68])
def test_pair_aligned_and_unaligned_operands(T, causal):
    """attention_d64_kernel<true> (LDS-DMA K, 16-byte loads and stores) against <false> (2-byte): the same LDS image, the same arithmetic."""
    import diffusion_rs_amd as d
    q, k, v = _aligned(*_qkv(T, T, seed=T))
    bias = _plain_bias(T, T, seed=1)
    _same_bits(d.ops.sdpa_d64(q, k, v, bias=bias, causal=causal), d.ops.sdpa_d64(_odd(q), _odd(k), _odd(v), bias=bias, causal=causal), f"T={T} causal={causal}")


@pytest.mark.parametrize("Tk", [68, 128])
def test_pair_bias_read_paths(Tk):
    """The same bias 16-byte aligned (bias_vec: float4 reads, at Tk = 68 with the key < Tk guard firing inside the last tile) and offset by one float (scalar)."""
    import diffusion_rs_amd as d
    q, k, v = _qkv(70, Tk, seed=Tk)
    bias, = _aligned(_plain_bias(70, Tk, seed=2))
    assert Tk % 4 == 0
    _same_bits(d.ops.sdpa_d64(q, k, v, bias=bias), d.ops.sdpa_d64(q, k, v, bias=_odd(bias)), f"Tk={Tk}")


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("Tq,Tk", [(77, 77), (130, 257), (257, 130)])
def test_pair_causal_and_explicit_mask(Tq, Tk, with_bias):
    """causal=True against causal=False with -inf above the diagonal: the second launch visits the future tiles, and they contribute exactly nothing."""
    import torch
    import diffusion_rs_amd as d
    q, k, v = _qkv(Tq, Tk, seed=Tq + Tk)
    r = _plain_bias(Tq, Tk, seed=3) if with_bias else None
    masked = (r if with_bias else torch.zeros((H, Tq, Tk), device="cuda")).masked_fill(_future(Tq, Tk), float("-inf"))
    _same_bits(d.ops.sdpa_d64(q, k, v, bias=r, causal=True), d.ops.sdpa_d64(q, k, v, bias=masked, causal=False), f"Tq={Tq} Tk={Tk} bias={with_bias}")


@pytest.mark.parametrize("Tk,Tpad", [(65, 128), (130, 192), (130, 256)])
def test_pair_ragged_tail_and_padded_keys(Tk, Tpad):
    """Tk keys against Tpad keys of which those past Tk hold random finite K and V under a -inf bias: the index mask of the ragged tile against the bias's.
    130 -> 256 adds a tile that is masked as a whole."""
    import torch
    import diffusion_rs_amd as d
    Tq = 70
    q, k, v = _qkv(Tq, Tk, seed=Tk)
    _, k_pad, v_pad = _qkv(Tq, Tpad - Tk, seed=Tpad)
    r = _plain_bias(Tq, Tk, seed=4)
    r_pad = torch.cat([r, torch.full((H, Tq, Tpad - Tk), float("-inf"), device="cuda")], 2)
    _same_bits(d.ops.sdpa_d64(q, k, v, bias=r), d.ops.sdpa_d64(q, torch.cat([k, k_pad], 1), torch.cat([v, v_pad], 1), bias=r_pad), f"Tk={Tk} against {Tpad}")


def test_pair_query_slices():
    """A row keeps its wave and its lane when the queries before a multiple of 64 or behind any point are cut away, and no row depends on another."""
    import diffusion_rs_amd as d
    q, k, v = _qkv(130, 130, seed=5)
    bias = _plain_bias(130, 130, seed=5)
    full = d.ops.sdpa_d64(q, k, v, bias=bias)
    _same_bits(d.ops.sdpa_d64(q[:, :70], k, v, bias=bias[:, :70]), full[:, :70], "queries 0 .. 69")
    _same_bits(d.ops.sdpa_d64(q[:, 64:], k, v, bias=bias[:, 64:]), full[:, 64:], "queries 64 .. 129")


def test_pair_batch_and_head_slices():
    import diffusion_rs_amd as d
    q, k, v = _qkv(70, 130, seed=6)
    bias = _plain_bias(70, 130, seed=6)
    full = d.ops.sdpa_d64(q, k, v, bias=bias)
    _same_bits(d.ops.sdpa_d64(q[1:], k[1:], v[1:], bias=bias), full[1:], "sample 1 alone")
    _same_bits(d.ops.sdpa_d64(q[:, :, 2:], k[:, :, 2:], v[:, :, 2:], bias=bias[2:]), full[:, :, 2:], "head 2 alone")


@pytest.mark.parametrize("perm", ["seeded", "reversal"])
def test_pair_v_channel_permutation(perm):
    """Every output channel is its own sum over the keys, in the same order whatever its place in the V^T tile."""
    import torch
    import diffusion_rs_amd as d
    q, k, v = _qkv(70, 130, seed=7)
    bias = _plain_bias(70, 130, seed=7)
    p = (torch.randperm(64, generator=torch.Generator().manual_seed(8)) if perm == "seeded" else torch.arange(63, -1, -1)).cuda()
    _same_bits(d.ops.sdpa_d64(q, k, v[..., p].contiguous(), bias=bias), d.ops.sdpa_d64(q, k, v, bias=bias)[..., p].contiguous(), f"{perm} permutation")


def test_pair_batch_stride_0():
    import diffusion_rs_amd as d
    q, k, v = _qkv(70, 130, seed=9)
    bias = _plain_bias(70, 130, seed=9)
    k1, v1 = k[:1].expand(B, -1, -1, -1), v[:1].expand(B, -1, -1, -1)
    assert k1.stride(0) == 0 and v1.stride(0) == 0
    _same_bits(d.ops.sdpa_d64(q, k1, v1, bias=bias), d.ops.sdpa_d64(q, k1.contiguous(), v1.contiguous(), bias=bias), "k, v expanded from one sample")


@pytest.mark.parametrize("causal", [False, True])
def test_pair_c_abi_default_strides(causal):
    """strides = NULL: four contiguous (B, T, H, 64) tensors."""
    import torch
    import diffusion_rs_amd as d
    q, k, v = _qkv(70, 130, seed=10)
    bias = _plain_bias(70, 130, seed=10)
    out = torch.zeros((B, 70, H, 64), dtype=torch.bfloat16, device="cuda")
    _same_bits(_launch(q, k, v, out, bias, causal, strides=False), d.ops.sdpa_d64(q, k, v, bias=bias, causal=causal), f"causal={causal}")


def test_pair_aligned_pointers_with_an_odd_stride():
    """16-byte aligned pointers whose token stride is 3 H 64 + 4 elements: every other row is 8-byte aligned only, so the launch must take the 2-byte kernel
    (which kernel ran cannot be seen from here; a 16-byte LDS-DMA fetch of such a row is what this guards against).  Equal to the dense layout's output."""
    import torch
    import diffusion_rs_amd as d
    T = 130
    q, k, v = _qkv(T, T, seed=11)
    bias = _plain_bias(T, T, seed=11)
    buf = torch.zeros((B, T, 3 * H * 64 + 4), dtype=torch.bfloat16, device="cuda")
    q2, k2, v2 = buf[..., :3 * H * 64].view(B, T, 3, H, 64).unbind(2)
    for dst, src in ((q2, q), (k2, k), (v2, v)):
        dst.copy_(src)
    _aligned(q2, k2, v2)
    assert q2.stride(1) == 3 * H * 64 + 4 and q2.stride(1) % 8 == 4
    _same_bits(d.ops.sdpa_d64(q2, k2, v2, bias=bias), d.ops.sdpa_d64(q, k, v, bias=bias), "token stride 3 H 64 + 4")


def test_pair_repeated_launches():
    """The same launch three times on one stream: 8 key tiles through the two buffers, one barrier a tile.  A tile read before it has landed, or overwritten
    while a slower wave still reads it, would not repeat."""
    import diffusion_rs_amd as d
    q, k, v = _qkv(512, 512, seed=12)
    bias = _plain_bias(512, 512, seed=12)
    first = d.ops.sdpa_d64(q, k, v, bias=bias)
    for n in (2, 3):
        _same_bits(d.ops.sdpa_d64(q, k, v, bias=bias), first, f"launch {n} against launch 1")


# ---------------------------------------------------------------- 3. stores stay inside the output view

@pytest.mark.parametrize("start", [64, 65], ids=["aligned", "odd"])
def test_stores_stay_inside_the_output_view(start):
    """out is a view with a head stride of 128 (64 used), a token stride of H 128 + 64 and gaps before, between and behind the samples, in a buffer full
    of SENTINEL.  Tq = 70: wave 0 of the second workgroup holds rows 70 .. 79, which must not be stored."""
    import torch
    import diffusion_rs_amd as d
    Tq, Tk = 70, 65
    q, k, v = _aligned(*_qkv(Tq, Tk, seed=13))
    bias = _plain_bias(Tq, Tk, seed=13)
    strides = (Tq * (H * 128 + 64) + 192, H * 128 + 64, 128, 1)
    size = start + B * strides[0] + 256
    buf = torch.full((size,), SENTINEL, dtype=torch.int16, device="cuda")
    inside = torch.zeros(size, dtype=torch.bool, device="cuda")
    torch.as_strided(inside, (B, Tq, H, 64), strides, start).fill_(True)
    assert int(inside.sum()) == B * Tq * H * 64
    out = torch.as_strided(buf.view(torch.bfloat16), (B, Tq, H, 64), strides, start)
    assert out.data_ptr() % 16 == (0 if start == 64 else 2)
    _launch(q, k, v, out, bias)
    torch.cuda.synchronize()
    touched = ((buf != SENTINEL) & ~inside).nonzero().flatten()
    assert len(touched) == 0, f"{len(touched)} elements outside the view were written, first at buffer offsets {touched[:8].tolist()} (the view starts at {start})"
    assert bool(torch.isfinite(out.float()).all()), "an element inside the view was not written (or is not finite)"
    _same_bits(out, d.ops.sdpa_d64(q, k, v, bias=bias), "the strided view against the dense launch")


# ---------------------------------------------------------------- 4. float64 comparison where exactness does not reach

TOLERANCE_CASES = [(Tq, Tk, with_bias, True, None) for Tq, Tk in [(16, 64), (64, 65), (130, 257), (257, 130)] for with_bias in (False, True)] + \
                  [(70, 68, True, False, None), (100, 100, True, False, None), (130, 257, False, False, 1.0)]


@pytest.mark.parametrize("Tq,Tk,with_bias,causal,scale", TOLERANCE_CASES)
def test_op_against_float64_at_the_inputs_left_out(Tq, Tk, with_bias, causal, scale):
    """Causal launches with Tq != Tk, Tk = 68 and 100 with a bias (the float4 bias path with a ragged tile), and scale 1.0 on randn q, k (scores of +- 30).
    Bounds: _check's, from the old kernel's measured figures (tests/test_gpu_sdpa_d64.py: OLD_KERNEL); at a key count that table lacks, 1.5 x its largest
    rel-L2 figure and 1.5 x the max-abs of the float64 result rounded to bf16 — nothing here is taken from the kernel under test."""
    import diffusion_rs_amd as d
    q, k, v = _qkv(Tq, Tk, seed=Tq * 1000 + Tk)
    bias = _bias(Tq, Tk, seed=7) if with_bias else None
    got = d.ops.sdpa_d64(q, k, v, bias=bias, causal=causal, scale=scale)
    _check(got, _reference(q, k, v, bias, causal, 0.125 if scale is None else scale), Tk, f"Tq={Tq} Tk={Tk} bias={with_bias} causal={causal} scale={scale}", any_tk=True)


# ---------------------------------------------------------------- 5. encoders at the tile boundaries

@pytest.mark.parametrize("T", [1, 64, 65, 128])
def test_t5_under_the_switch_at_tile_boundaries(T):
    """T5's small tower against the oracle at one token, a full tile, a tile and one key, two full tiles (rel-L2 <= 1e-2, tests/test_gpu_text.py)."""
    import torch
    import diffusion_rs_amd as d
    from tests.test_gpu_text import SMALL_T5, _pair
    _, gm, om, _ = _pair("t5", dict(SMALL_T5, num_layers=2))
    ids = np.random.default_rng(T).integers(0, SMALL_T5["vocab_size"], (1, T)).astype(np.int32)
    try:
        d.set_encoder_attention("mfma")
        err = rel_l2(host(gm.forward(ids, dtype=torch.float32)), om.forward(ids))
    finally:
        d.set_encoder_attention("default")
    print(f"T5 under mfma, T={T}: rel-L2 {err:.3e}")
    assert err <= 1e-2
