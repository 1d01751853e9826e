"""The input builders of tests/test_gpu_sdpa_d64_exact.py (tests/sdpa_d64_inputs.py), checked in float64 on the CPU for every case the GPU file runs: the
selected key wins by at least 200 in the log2 domain (an f32 exp2 of the difference is exactly 0), it is visible under the causal mask, the V rows of a
(batch, head) all differ, and builder (a)'s operands are exact in bf16.  With these a mismatch on the GPU is the kernel's, not the inputs'."""
import pytest
import torch

from tests import sdpa_d64_inputs as I

VALUE_TKS = sorted({Tk for _, Tk in I.SHAPES + I.LADDER_SHAPES})


def _ids(case):
    Tq, Tk, name, causal = case
    return f"{Tq}x{Tk}-{name}-{'causal' if causal else 'full'}"


@pytest.mark.parametrize("case", I.ROUTING_CASES, ids=_ids)
def test_maps_select_a_visible_key(case):
    Tq, Tk, name, causal = case
    pi = I.key_map(name, Tq, Tk, causal)
    assert pi.shape == (I.H, Tq) and pi.dtype == torch.int64 and int(pi.min()) >= 0 and int(pi.max()) < Tk
    if causal:
        assert bool((pi <= torch.arange(Tq)[None]).all())
    else:  # the named maps are what they say where nothing folds them
        i = torch.arange(Tq)
        want = {"identity": i % Tk, "reversal": (Tk - 1 - i) % Tk, "first": i * 0, "last": i * 0 + Tk - 1, "tile_edges": (64 * i + 63) % Tk}.get(name)
        assert want is None or torch.equal(pi, want[None].expand(I.H, Tq))


@pytest.mark.parametrize("case", I.ROUTING_CASES, ids=_ids)
def test_selection_through_qk_wins_by_the_margin(case):
    Tq, Tk, name, causal = case
    pi = I.key_map(name, Tq, Tk, causal)
    q, k, scale = I.select_by_qk(Tq, Tk, pi)
    assert q.dtype == k.dtype == torch.bfloat16 and q.shape == (I.B, Tq, I.H, 64) and k.shape == (I.B, Tk, I.H, 64) and scale == 1.0
    # exact in bf16: every value is 0 or 16, two 16s a row, and the rows are the codes they should be
    for t, codes in ((q, I.key_code(pi).permute(1, 0, 2)), (k, I.key_code(torch.arange(Tk))[:, None, :].expand(Tk, I.H, 64))):
        assert torch.equal(t.float(), codes[None].expand_as(t).float()) and bool(((t == 0) | (t == 16)).all()) and bool(((t == 16).sum(-1) == 2).all())
    s = I.log2_scores(q, k, scale, None, False)
    assert set(torch.unique(s / I.LOG2E).round().tolist()) <= {0.0, 256.0, 512.0}
    margin = I.selection_margin(q, k, scale, None, causal, pi)
    print(f"builder (a) {_ids(case)}: margin {margin:.1f}")
    assert margin >= I.MARGIN and (margin >= 369.0 or margin == float("inf"))


@pytest.mark.parametrize("case", I.ROUTING_CASES, ids=_ids)
def test_selection_through_the_bias_wins_by_the_margin(case):
    Tq, Tk, name, causal = case
    pi = I.key_map(name, Tq, Tk, causal)
    q, k, scale, bias = I.select_by_bias(Tq, Tk, pi, seed=Tq + Tk)
    assert bias.dtype == torch.float32 and bias.shape == (I.H, Tq, Tk) and bool((bias.sum(-1) == 1000.0).all()) and bool(((bias == 0) | (bias == 1000.0)).all())
    margin = I.selection_margin(q, k, scale, bias, causal, pi)
    print(f"builder (b) {_ids(case)}: margin {margin:.1f}")
    assert margin >= I.MARGIN


@pytest.mark.parametrize("Tq,Tk", I.LADDER_SHAPES)
def test_ladder_bias_moves_the_maximum_in_every_tile(Tq, Tk):
    bias, pi = I.ladder_bias(Tq, Tk)
    q, k, scale, _ = I.select_by_bias(Tq, Tk, pi, seed=3)
    s = I.log2_scores(q, k, scale, bias, False)
    nt = (Tk + 63) // 64
    assert nt == 4
    best = torch.stack([s[..., 64 * t:64 * t + 64].amax(-1) for t in range(nt)])  # (nt, B, H, Tq): each tile's best score
    steps = best[1:] - best[:-1]
    print(f"ladder {Tq}x{Tk}: the tile maxima rise by {float(steps.min()):.1f} .. {float(steps.max()):.1f}")
    assert float(steps.min()) >= I.MARGIN  # the maximum moves in every tile, and what was accumulated before is rescaled by exactly 0
    assert bool((pi >= 64 * (nt - 1)).all()) and I.selection_margin(q, k, scale, bias, False, pi) >= I.MARGIN


@pytest.mark.parametrize("Tk", VALUE_TKS)
def test_value_rows_differ_pairwise(Tk):
    v = I.values(Tk, seed=Tk)
    assert v.dtype == torch.bfloat16 and v.shape == (I.B, Tk, I.H, 64) and not bool((v == 0).any()) and bool(torch.isfinite(v.float()).all())
    bits = v.view(torch.int16)
    for b in range(I.B):
        for h in range(I.H):
            assert len(torch.unique(bits[b, :, h], dim=0)) == Tk, f"two keys of (b, h) = ({b}, {h}) hold the same V row"
            # a wrong channel shows as well: no row is constant
            assert bool((bits[b, :, h] != bits[b, :, h, :1]).any(-1).all())
