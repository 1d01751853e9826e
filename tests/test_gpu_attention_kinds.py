"""Every attention kernel kind through both output layouts.  The kernels share one frame (csrc/attention_frame.h: workgroup decode, output
row pointer, LDS-DMA offsets with the last tile's clamp, epilogues) and one dispatcher; the fuzz tests drive the token-major layout only.
Here: kinds 0..5 of the test build and the product build's 5 and 1, head-major and token-major output, on four small shapes that are
ragged in both directions, put one row into a second query block, put one key into a second KV tile, and have a single KV tile (which
every kind must hand to an 8-wave kernel).  Tolerance: the op-level one of DESIGN.md §5 against torch f32."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

SHAPES = [  # (B, H, Lq, Lk)
    (2, 2, 65, 129),    # ragged both ways, batch and head strides
    (1, 3, 257, 193),   # a second q-block holding one row
    (1, 1, 64, 65),     # two tiles, the second with one key: the clamped DMA offsets of the last tile
    (1, 2, 300, 64),    # single tile: every kind lands on an 8-wave kernel
]
SCALE = 1.0 / 128 ** 0.5


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def env():
    import torch
    from diffusion_rs_amd import _lib as L
    return torch, L, L.load(), L.load_alt()


@pytest.fixture(scope="module")
def problems(env):
    """Inputs and the torch f32 reference (head-major) of every shape, made once."""
    torch = env[0]
    g = torch.Generator(device="cuda").manual_seed(5)
    out = {}
    for (B, H, Lq, Lk) in SHAPES:
        q = torch.randn(B, H, Lq, 128, device="cuda", generator=g).to(torch.bfloat16)
        k = torch.randn(B, H, Lk, 128, device="cuda", generator=g).to(torch.bfloat16)
        v = torch.randn(B, H, Lk, 128, device="cuda", generator=g).to(torch.bfloat16)
        ref = torch.softmax((q.float() @ k.float().transpose(-1, -2)) * SCALE, -1) @ v.float()
        out[(B, H, Lq, Lk)] = (q, k, v, ref)
    return out


def _run(torch, L, lib, q, k, v, token_major):
    B, H, Lq, _ = q.shape
    o = torch.full((B, Lq, H * 128) if token_major else (B, H, Lq, 128), float("nan"), device="cuda", dtype=torch.bfloat16)
    L.check(lib.fmi_sdpa_bf16(_p(q), _p(k), _p(v), _p(o), B, H, Lq, k.shape[2], 128, SCALE, token_major, None))
    torch.cuda.synchronize()
    return o


def _check_kinds(torch, L, lib, kinds, shape, problem):
    """-> {kind: head-major output}; checks finiteness, the tolerance, the two layouts against each other and kind 5's reproducibility."""
    q, k, v, ref = problem
    B, H, Lq, _ = shape
    outs = {}
    try:
        for kind in kinds:
            L.check(lib.fmi_set_attention_kernel(kind))
            hm = _run(torch, L, lib, q, k, v, 0)
            tm = _run(torch, L, lib, q, k, v, 1)
            assert torch.isfinite(hm.float()).all() and torch.isfinite(tm.float()).all(), (shape, kind)
            err = float((hm.float() - ref).norm() / ref.norm())
            assert err <= 6e-3, (shape, kind, err)
            assert torch.equal(tm.view(B, Lq, H, 128).transpose(1, 2).contiguous().view(torch.int16), hm.view(torch.int16)), (shape, kind, "token-major vs head-major")
            outs[kind] = hm.view(torch.int16)
        L.check(lib.fmi_set_attention_kernel(5))
        assert torch.equal(_run(torch, L, lib, q, k, v, 0).view(torch.int16), outs[5]), (shape, "kind 5 rerun")
    finally:
        L.check(lib.fmi_set_attention_kernel(5))
    return outs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_kind_in_both_output_layouts(env, problems, shape):
    torch, L, product, alt = env
    outs = _check_kinds(torch, L, alt, range(6), shape, problems[shape])
    for family in ((0, 1, 2), (3, 4)):  # one arithmetic each: bit-identical inside
        for kind in family[1:]:
            assert torch.equal(outs[kind], outs[family[0]]), (shape, kind, "differs from kind", family[0])
    if shape[3] <= 64:  # a single KV tile: whatever the kind, an 8-wave kernel runs
        for kind in range(1, 6):
            assert torch.equal(outs[kind], outs[1]), (shape, kind, "single tile: differs from kind 1")
    _check_kinds(torch, L, product, (5, 1), shape, problems[shape])
