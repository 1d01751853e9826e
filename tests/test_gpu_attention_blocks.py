"""Block-sparse joint attention at d = 128.  The op is held to 1.5 x the rel-L2 that fmi_sdpa_bf16 shows against float64 on the same q, k, v
unmasked (tests/test_gpu_attention_groups.py's bar and operands) and to fmi_sdpa_groups_bf16's BITS on the same mask; the model and the pipeline to bits as well."""
import numpy as np
import pytest

from tests.test_gpu_attention_groups import B, H, SCALE, _problem
from tests.util import SMALL_FLUX, SMALL_VAE, dev, flux_inputs, host, rel_l2

pytestmark = pytest.mark.gpu


def lists(pattern, Lq, Lk):
    """(row_ptr, cols): the key tiles of every query block, ascending."""
    nqb, nt = -(-Lq // 128), -(-Lk // 64)
    own = lambda b: {min(2 * b, nt - 1), min(2 * b + 1, nt - 1)}
    rows = {"full": lambda b: range(nt),
            "band": lambda b: {t for o in own(b) for t in (o - 1, o, o + 1) if 0 <= t < nt},
            "first+own": lambda b: {0} | own(b),
            "single": lambda b: {(2 * b + 3) % nt},
            "uneven": lambda b: (range(1, 2), range(nt), range(nt - 2, nt))[b % 3]}[pattern]
    rows = [sorted(rows(b)) for b in range(nqb)]
    return np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), np.concatenate(rows).astype(np.int32)


def reference(q, k, v, row_ptr, cols):
    """float64 masked softmax on the bf16-rounded inputs (B, H, L, 128)."""
    Lq, Lk = q.shape[2], k.shape[2]
    seen = np.zeros((Lq, Lk), bool)
    for b in range(len(row_ptr) - 1):
        for t in cols[row_ptr[b]:row_ptr[b + 1]]:
            seen[128 * b:128 * b + 128, 64 * t:64 * t + 64] = True
    s = np.where(seen, np.einsum("bhqd,bhkd->bhqk", q.astype(np.float64), k.astype(np.float64)) * SCALE, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    return np.einsum("bhqk,bhkd->bhqd", p / p.sum(-1, keepdims=True), v.astype(np.float64))


def groups_output(q, k, v, row_ptr, cols, token_major):
    """fmi_sdpa_groups_bf16 on the same mask: query block b carries bit b, key tile t the bits of the blocks that list it.  (The entry itself: ops.sdpa_groups
    insists that a token sees itself, which `single` and `uneven` do not grant.)"""
    import torch
    from diffusion_rs_amd import _lib as L
    Lq, Lk = q.shape[2], k.shape[2]
    kt = np.zeros(-(-Lk // 64), np.int32)
    for b in range(len(row_ptr) - 1):
        kt[cols[row_ptr[b]:row_ptr[b + 1]]] |= 1 << b
    qg, kg = dev((1 << (np.arange(Lq) // 128)).astype(np.int32)), dev(kt[np.arange(Lk) // 64])
    out = torch.empty((B, Lq, H * 128) if token_major else (B, H, Lq, 128), dtype=torch.bfloat16, device=q.device)
    L.check(L.load().fmi_sdpa_groups_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, Lq, Lk, 128, SCALE, int(token_major), qg.data_ptr(), kg.data_ptr(), 1, None))
    return out


@pytest.mark.parametrize("pattern", ["full", "band", "first+own", "single", "uneven"])
@pytest.mark.parametrize("Lq,Lk", [(320, 320), (300, 300), (128, 700)])  # a partial last query block, a ragged last key tile, cross shapes
def test_op_against_float64_and_the_groups_kernel_bit_for_bit(Lq, Lk, pattern):
    import torch
    import diffusion_rs_amd as d
    q, k, v, f, base = _problem(Lq, Lk)
    rp, cl = lists(pattern, Lq, Lk)
    want, nqb = reference(*f, rp, cl), len(rp) - 1
    for token_major in (False, True):
        out = d.ops.sdpa_blocks(q, k, v, rp, cl, out_token_major=token_major)
        got = host(out.float())
        got = got.reshape(B, Lq, H, 128).transpose(0, 2, 1, 3) if token_major else got
        err = rel_l2(got, want)
        print(f"sdpa_blocks Lq={Lq} Lk={Lk} {pattern} token_major={token_major}: rel-L2 {err:.3e} (fmi_sdpa_bf16 unmasked {base:.3e}, bound {1.5 * base:.3e})")
        assert np.isfinite(got).all() and err <= 1.5 * base
        assert torch.equal(out, groups_output(q, k, v, rp, cl, token_major))
        for order in (np.arange(nqb)[::-1].copy(), np.arange(nqb)):  # the launch order changes no bit
            assert torch.equal(out, d.ops.sdpa_blocks(q, k, v, rp, cl, order=order, out_token_major=token_major))


T, GRID = 128, (4, 128)  # one query block of text, then one per image row: at radius 1 the lists are the chain block b <-> b +- 1, which group words can say


@pytest.fixture(scope="module")
def model():
    import torch
    import diffusion_rs_amd as d
    sd = d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    gm = d.FluxModel(SMALL_FLUX)
    gm.load_state_dict(sd)
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, B, GRID, T)
    t, g = np.linspace(0.9, 0.4, B).astype(np.float32), np.full(B, 3.5, np.float32)

    def run(rows=T):
        out = gm.forward(dev(img), dev(ids), dev(txt[:, :rows], torch.bfloat16), dev(txt_ids[:, :rows]), dev(t), dev(y), dev(g))
        torch.cuda.synchronize()
        return host(out)
    return dict(d=d, gm=gm, run=run, sd=sd, plain=run(), lists=d.flux.local_attention_tiles(T, *GRID, 1))


def test_model_equals_the_groups_forward_and_clearing_restores_the_plain_one(model):
    gm, run, (rp, cl) = model["gm"], model["run"], model["lists"]
    # image row y shares bit y with the row above and bit y + 1 with the row below; the text shares one with every row
    txt_w, img_w = np.full(T, 0b11111, np.uint32), np.repeat([0b00011, 0b00110, 0b01100, 0b11000], GRID[1]).astype(np.uint32)
    words = np.concatenate([txt_w, img_w])
    for b in range(len(rp) - 1):  # the words say the lists
        assert sorted(cl[rp[b]:rp[b + 1]]) == [t for t in range(len(words) // 64) if words[128 * b] & words[64 * t]]
    try:
        gm.set_attention_groups(txt_w, img_w)
        want = run()
    finally:
        gm.clear_attention_groups()
    try:
        gm.set_attention_blocks(rp, cl)
        got = run()
    finally:
        gm.clear_attention_blocks()
    np.testing.assert_array_equal(got, want)
    assert np.isfinite(got).all() and np.abs(got - model["plain"]).max() > 0  # the mask is applied
    np.testing.assert_array_equal(run(), model["plain"])


def test_pipeline_window_is_the_lists_installed_by_hand_and_leaves_the_handle_clear():
    import torch
    import diffusion_rs_amd as d
    pipe = d.Pipeline(d.ModelSource.Synthetic(flux_cfg=SMALL_FLUX, vae_cfg=SMALL_VAE))
    pipe.flux.load_state_dict(d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0))
    pipe.vae.load_state_dict(d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0))
    rng = np.random.default_rng(7)
    emb = (dev(rng.standard_normal((1, T, SMALL_FLUX["joint_attention_dim"])).astype(np.float32), torch.bfloat16),
           dev(rng.standard_normal((1, SMALL_FLUX["pooled_projection_dim"])).astype(np.float32)))
    params = d.DiffusionGenerationParams(height=16 * GRID[0], width=16 * GRID[1], num_steps=2, guidance_scale=3.5)
    request = lambda **kw: pipe.forward(["a"], params, output="tensor", seed=3, embeddings=emb, **kw)
    got, plain = request(attention_window=1), request()
    try:
        pipe.flux.set_attention_blocks(*d.flux.local_attention_tiles(T, *GRID, 1))
        want = request()
    finally:
        pipe.flux.clear_attention_blocks()
    assert torch.equal(got, want) and not torch.equal(got, plain) and torch.equal(request(), plain)


def test_refusals_leave_the_state_untouched(model):
    d, gm, run, (rp, cl) = model["d"], model["gm"], model["run"], model["lists"]
    from diffusion_rs_amd import _lib as L

    def refused(code, call):
        with pytest.raises(d.FmiError) as e:
            call()
        assert e.value.code == code, e.value
    q8 = d.FluxModel(SMALL_FLUX)
    q8.load_state_dict(model["sd"])
    q8.quantize_int8()
    refused(L.ERR_UNSUPPORTED, lambda: q8.set_attention_blocks(rp, cl))
    q8.close()
    try:
        gm.set_attention_groups(np.ones(T, np.uint32), np.ones(GRID[0] * GRID[1], np.uint32))
        refused(L.ERR_UNSUPPORTED, lambda: gm.set_attention_blocks(rp, cl))
    finally:
        gm.clear_attention_groups()
    descending, out_of_range, empty = cl.copy(), cl.copy(), rp.copy()
    descending[[0, 1]] = descending[[1, 0]]
    out_of_range[-1], empty[1] = 2 * (len(rp) - 1), 0  # (empty: row 0 lists nothing)
    for bad in ((rp, descending), (rp, out_of_range), (empty, cl)):
        refused(L.ERR_INVALID, lambda: gm.set_attention_blocks(*bad))
    np.testing.assert_array_equal(run(), model["plain"])  # nothing of the above installed anything
    try:
        gm.set_attention_blocks(rp, cl)
        refused(L.ERR_INVALID, lambda: run(rows=T - 65))  # another L: a key tile fewer
        refused(L.ERR_UNSUPPORTED, lambda: gm.set_attention_groups(np.ones(T, np.uint32), np.ones(GRID[0] * GRID[1], np.uint32)))
    finally:
        gm.clear_attention_blocks()
    np.testing.assert_array_equal(run(), model["plain"])
