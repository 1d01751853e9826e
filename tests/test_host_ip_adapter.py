"""FLUX IP-Adapter, the parts that need no GPU: the composed CPU reference of tests/ip_adapter_ref.py is the oracle's own forward when the
adapter's scale is 0, every wrong variant lies at least 10 x the GPU loop bar (3e-2) from the correct loop, the recipe of the kernel agrees with the composed
attention, both checkpoint namings map to the same tensors, and every refusal of the Python layer."""
import numpy as np
import pytest

import diffusion_rs_amd as d
from diffusion_rs_amd import _lib as L
from diffusion_rs_amd import flux as F
from diffusion_rs_amd import loader
from diffusion_rs_amd import pipeline as P
from tests import ip_adapter_ref as IR
from tests.util import bf16_round, rel_l2

GPU_LOOP_BAR = 3e-2  # tests/test_gpu_ip_adapter.py, as tests/test_gpu_controlnet.py


def test_symbols_are_exported_and_bound():
    for s in ("fmi_ip_adapter_create", "fmi_ip_adapter_destroy", "fmi_ip_adapter_set_tensor", "fmi_ip_adapter_missing_count", "fmi_ip_adapter_missing_name",
              "fmi_ip_adapter_size_in_bytes", "fmi_flux_forward_ip", "fmi_flux_denoise_ip", "fmi_ip_attention"):
        assert s in L.EXPORTED and hasattr(L.load(), s), s
    assert [f[0] for f in L.FluxIp._fields_] == ["adapter", "embeds", "embeds_dtype", "neg_embeds", "scale", "step_scales"]
    assert len(L.FluxDenoiseOptions._fields_) == 7  # (the adapter is an argument of its own)


@pytest.mark.parametrize("grid", list(IR.GRIDS))
def test_scale_zero_is_the_oracle_forward(grid):
    s = IR.inputs(grid)
    om, sd = IR.main_oracle(), IR.main_state_dict()
    Ks, Vs = IR.project(IR.adapter_state_dict(), IR.MAIN_CFG, s["emb"])
    t = np.full(IR.B, 0.8, np.float32)
    want = om.forward(s["img"], s["ids"], s["txt"], s["txt_ids"], t, s["y"], s["g"])
    got = IR.forward(om, sd, IR.MAIN_CFG, s["img"], s["ids"], s["txt"], s["txt_ids"], t, s["y"], s["g"], Ks, Vs, 0.0)
    assert rel_l2(got, want) <= 1e-5
    loop = IR.ip_loop(om, sd, IR.MAIN_CFG, IR.adapter_state_dict(), s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], IR.TS4, s["emb"], c=0.0)
    assert rel_l2(loop, om.denoise(s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], IR.TS4)) <= 1e-5
    # and a step scale of 0 is a plain step: [0, 0, 0, 0] at any scale
    loop0 = IR.ip_loop(om, sd, IR.MAIN_CFG, IR.adapter_state_dict(), s["img"], s["ids"], s["txt"], s["txt_ids"], s["y"], s["g"], IR.TS4, s["emb"], c=IR.IP_SCALE,
                       step_scales=[0, 0, 0, 0])
    assert (loop0 == loop).all()


@pytest.mark.parametrize("mode", list(IR.MODES))
@pytest.mark.parametrize("grid", list(IR.GRIDS))
def test_every_variant_is_far_from_the_correct_loop(grid, mode):
    """Measured with the stds of tests/ip_adapter_ref.py (PROJ_STD 0.2, K_STD 0.25, V_STD 0.006, IP_SCALE 4, IMG_MULT 0.15), rel-L2 of the final latents to the
    correct loop, aligned / ragged grid, mode "plain": rotated_q 0.47 / 0.49, unnormed_q 0.41 / 0.43, norm_k_on_ip_keys 0.37 / 0.38, through_out_proj 1.27 / 1.27,
    into_txt_rows 1.17 / 1.17, scale_dropped 0.42 / 0.42, next_block_kv 0.84 / 0.84, k_viewed_hn 0.86 / 0.91, singles_too 0.45 / 0.46; "cfg": 0.55, 0.48, 0.43,
    1.27, 1.02, 0.43, 1.03, 1.06, neg_uses_pos_embeds 0.83, 0.63 (aligned); the smallest over all modes and grids is norm_k_on_ip_keys in "steps", 0.32."""
    ok = IR.loop_reference(grid, mode)
    assert np.isfinite(ok).all()
    for v in IR.VARIANTS:
        if v == "neg_uses_pos_embeds" and mode not in ("cfg", "cfg_neg"):
            assert (IR.loop_reference(grid, mode, v) == ok).all()  # (without a negative the variant IS the correct loop)
            continue
        dist = rel_l2(IR.loop_reference(grid, mode, v), ok)
        print(f"{grid} {mode}: {v} {dist:.3f}")
        assert dist >= 10 * GPU_LOOP_BAR, (v, dist)


def test_the_kernel_recipe_is_the_composed_attention():
    """ip_attention_recipe (what the kernel is held to) against the composition the model reference uses (oracle rms_norm_slow + softmax_last_dim)"""
    from oracle import oracle as orc
    rng = np.random.default_rng(7)
    B, S, H, N = 2, 9, 2, 5
    q = bf16_round(rng.standard_normal((B, S, H, 128)))
    wq = bf16_round(1.0 + 0.1 * rng.standard_normal(128))
    K, V = bf16_round(rng.standard_normal((B, H, N, 128))), bf16_round(rng.standard_normal((B, H, N, 128)))
    x = rng.standard_normal((B, S, H * 128)).astype(np.float32)
    want = x + np.float32(0.7) * IR.ip_attention(orc.rms_norm_slow(q, wq, 1e-6), K, V)
    assert rel_l2(IR.ip_attention_recipe(q, wq, K, V, x, 0.7, np.float32), want) <= 1e-6
    assert rel_l2(IR.ip_attention_recipe(q, wq, K, V, x, 0.7, np.float64), want) <= 1e-6
    one = IR.ip_attention_recipe(q, wq, K[:, :, :1], V[:, :, :1], np.zeros_like(x), 1.0, np.float32)  # one token: the softmax is 1 and ip is its value row
    np.testing.assert_allclose(one.reshape(B, S, H, 128), np.broadcast_to(V[:, None, :, 0], (B, S, H, 128)), rtol=0, atol=1e-6)


def _xlabs(sd, drop_bias=False):
    out = {}
    for k, v in sd.items():
        p = k.split(".")
        if p[0] == "image_proj":
            out[f"ip_adapter_proj_model.{'proj' if p[1] == 'image_embeds' else 'norm'}.{p[2]}"] = v
        elif not (drop_bias and p[3] == "bias"):
            out[f"double_blocks.{p[1]}.processor.ip_adapter_double_stream_{p[2][3]}_proj.{p[3]}"] = v
    return out


def test_key_mapping_of_both_namings(tmp_path):
    sd = IR.adapter_state_dict()
    assert list(sd) == list(d.synth.ip_adapter_tensor_shapes(IR.MAIN_CFG, IR.E, IR.N))
    for k in sd:
        assert loader.ip_adapter_key_map(k) == k
    xl = _xlabs(sd)
    assert len(xl) == len(sd) and "double_blocks.2.processor.ip_adapter_double_stream_v_proj.bias" in xl and "ip_adapter_proj_model.proj.weight" in xl
    for src in (sd, xl):
        E, N, conv = loader.ip_adapter_from_tensors(IR.MAIN_CFG, src)
        assert (E, N) == (IR.E, IR.N) and set(conv) == set(sd) and all(conv[k] is sd[k] for k in sd)
    E, N, conv = loader.ip_adapter_from_tensors(IR.MAIN_CFG, _xlabs(sd, drop_bias=True))  # the k / v biases are optional
    assert (E, N) == (IR.E, IR.N) and set(conv) == {k for k in sd if not (k.startswith("ip_adapter.") and k.endswith(".bias"))}
    for name in ("ip_adapter_proj_model.proj.scale", "double_blocks.0.processor.qkv.weight", "ip_adapter.0.to_q_ip.weight", "image_proj.other.weight", "x.weight"):
        assert loader.ip_adapter_key_map(name) is None
    with pytest.raises(ValueError, match="unexpected tensors.*single_blocks.0.foo.weight"):
        loader.ip_adapter_from_tensors(IR.MAIN_CFG, dict(xl, **{"single_blocks.0.foo.weight": sd["image_proj.norm.weight"]}))
    with pytest.raises(ValueError, match=r"unexpected tensors.*ip_adapter\.3\.to_k_ip\.weight"):  # a block the transformer does not have
        loader.ip_adapter_from_tensors(IR.MAIN_CFG, dict(sd, **{"ip_adapter.3.to_k_ip.weight": sd["ip_adapter.0.to_k_ip.weight"]}))
    with pytest.raises(ValueError, match=r"1 IP-Adapter tensors missing.*ip_adapter\.1\.to_v_ip\.weight"):
        loader.ip_adapter_from_tensors(IR.MAIN_CFG, {k: v for k, v in sd.items() if k != "ip_adapter.1.to_v_ip.weight"})
    with pytest.raises(ValueError, match="image_proj.image_embeds.weight"):
        loader.ip_adapter_from_tensors(IR.MAIN_CFG, {k: v for k, v in sd.items() if k != "image_proj.image_embeds.weight"})
    with pytest.raises(ValueError, match="no multiple of joint_attention_dim"):
        loader.ip_adapter_from_tensors(IR.MAIN_CFG, dict(sd, **{"image_proj.image_embeds.weight": sd["image_proj.image_embeds.weight"][:-1]}))
    with pytest.raises(ValueError, match=r"ip_adapter\.0\.to_k_ip\.weight is"):
        loader.ip_adapter_from_tensors(IR.MAIN_CFG, dict(sd, **{"ip_adapter.0.to_k_ip.weight": sd["ip_adapter.0.to_k_ip.weight"][:, :64]}))
    # a file: N and E from the shapes (N = 3 here)
    import torch
    from safetensors.torch import save_file
    sd3 = d.synth.ip_adapter_state_dict_numpy(IR.MAIN_CFG, 32, 3, seed=1)
    path = str(tmp_path / "ip_adapter.safetensors")
    save_file({k: torch.from_numpy(v).to(torch.bfloat16) for k, v in _xlabs(sd3).items()}, path)
    E, N, conv = loader.load_ip_adapter(path, IR.MAIN_CFG)
    assert (E, N) == (32, 3) and set(conv) == set(sd3)
    np.testing.assert_array_equal(conv["ip_adapter.2.to_k_ip.weight"].float().numpy(), sd3["ip_adapter.2.to_k_ip.weight"])
    with pytest.raises(FileNotFoundError):
        loader.load_ip_adapter(str(tmp_path / "none.safetensors"), IR.MAIN_CFG)


ADA = dict(num_heads=2, joint_attention_dim=128, num_layers=3, embed_dim=IR.E, num_tokens=IR.N)
IMG = (2, 24, 64)


def test_flux_layer_refusals_without_a_device():
    ok = dict(cfg=IR.MAIN_CFG, adapter=ADA, img_shape=IMG, embeds_shape=(2, IR.E))
    assert F.check_ip_adapter_args(**ok) is None
    assert F.check_ip_adapter_args(IR.MAIN_CFG) is None  # no adapter, nothing given
    ss = F.check_ip_adapter_args(**ok, step_scales=[1, 0, 0.5, 1], n_steps=4)
    assert ss.dtype == np.float32 and ss.tolist() == [1, 0, 0.5, 1]
    assert F.check_ip_adapter_args(**ok, negative_embeds_shape=(2, IR.E), has_negative=True) is None
    for kw, msg in ((dict(embeds_shape=(2, IR.E)), "needs ip_adapter="), (dict(negative_embeds_shape=(2, IR.E)), "needs ip_adapter="),
                    (dict(step_scales=[1.0]), "needs ip_adapter=")):
        with pytest.raises(ValueError, match=msg):
            F.check_ip_adapter_args(IR.MAIN_CFG, None, IMG, **kw)
    bad = [(dict(embeds_shape=None), "needs ip_adapter_image_embeds="), (dict(embeds_shape=(2, IR.E + 8)), "expected"), (dict(embeds_shape=(1, IR.E)), "expected"),
           (dict(adapter=dict(ADA, num_heads=4)), "num_heads"), (dict(adapter=dict(ADA, joint_attention_dim=256)), "joint_attention_dim"),
           (dict(adapter=dict(ADA, num_layers=2)), "num_layers"), (dict(adapter=dict(ADA, num_tokens=33)), "1 <= N <= 32"), (dict(adapter=dict(ADA, num_tokens=0)), "1 <= N <= 32"),
           (dict(negative_embeds_shape=(2, IR.E)), "needs a negative prompt"), (dict(negative_embeds_shape=(2, 8), has_negative=True), "expected"),
           (dict(scale=float("nan")), "finite"), (dict(scale=float("inf")), "finite"), (dict(step_scales=[1, 2, 3], n_steps=4), "one entry per step"),
           (dict(step_scales=[1, float("nan"), 1, 1], n_steps=4), "finite")]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            F.check_ip_adapter_args(**dict(ok, **kw))
    for other, msg in (("context", "context="), ("cache", "step cache"), ("sequence_parallel", "sequence parallelism"), ("fp8", "fp8 mode"), ("int8", "int8 mode")):
        with pytest.raises(ValueError, match=msg):
            F.check_combination({"ip_adapter", other})


def test_pipeline_layer_refusals_without_a_device():
    E = IR.E
    P.check_ip_adapter_request(False)  # nothing given, nothing loaded
    P.check_ip_adapter_request(True, E)  # loaded, not given: not conditioned
    P.check_ip_adapter_request(True, E, (E,))
    P.check_ip_adapter_request(True, E, (1, E), (E,), 0.5, 0.25, 0.75, has_negative=True)
    bad = [(dict(loaded=False, embeds_shape=(E,)), "load_ip_adapter"), (dict(negative_embeds_shape=(E,)), "needs ip_adapter_image_embeds="),
           (dict(embeds_shape=(2, E)), "one embedding per request"), (dict(embeds_shape=(E + 1,)), "one embedding per request"),
           (dict(embeds_shape=(E,), negative_embeds_shape=(2, E), has_negative=True), "one embedding per request"),
           (dict(embeds_shape=(E,), negative_embeds_shape=(E,)), "negative prompt"), (dict(embeds_shape=(E,), scale=float("nan")), "finite"),
           (dict(embeds_shape=(E,), start=0.6, end=0.5), "0 <= start <= end <= 1"), (dict(embeds_shape=(E,), end=1.5), "0 <= start <= end <= 1"),
           (dict(embeds_shape=(E,), start=-0.1), "0 <= start <= end <= 1")]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            P.check_ip_adapter_request(**dict(dict(loaded=True, embed_dim=E), **kw))
    for other, msg in (("context", "reference="), ("cache", "step cache"), ("sequence_parallel", "sequence parallelism"), ("int8", "int8 mode"), ("fp8", "fp8 mode")):
        with pytest.raises(ValueError, match=msg):
            F.check_combination({"ip_adapter", other}, P.REQUEST_NAMES)
    assert IR.keep(4, 0.25, 0.75) == F.controlnet_step_scales(4, 0.25, 0.75) == [0.0, 1.0, 1.0, 0.0]


def test_synthetic_weights_are_bf16_and_seeded():
    a, b = IR.adapter_state_dict(), d.synth.ip_adapter_state_dict_numpy(IR.MAIN_CFG, IR.E, IR.N, seed=5, proj_std=IR.PROJ_STD, k_std=IR.K_STD, v_std=IR.V_STD)
    assert all((a[k] == b[k]).all() and (bf16_round(a[k]) == a[k]).all() for k in a)
    c = d.synth.ip_adapter_state_dict_numpy(IR.MAIN_CFG, IR.E, IR.N, seed=6)
    assert not (a["ip_adapter.0.to_k_ip.weight"] == c["ip_adapter.0.to_k_ip.weight"]).all()
    nb = d.synth.ip_adapter_tensor_shapes(IR.MAIN_CFG, IR.E, IR.N, kv_bias=False)
    assert "ip_adapter.0.to_k_ip.bias" not in nb and "image_proj.image_embeds.bias" in nb
    assert a["image_proj.image_embeds.weight"].shape == (IR.N * 128, IR.E) and a["ip_adapter.2.to_v_ip.weight"].shape == (256, 128)
