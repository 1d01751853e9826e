"""Host logic of the LoRA file reader (diffusion_rs_amd.lora.read_lora; CPU only, no HIP calls): the diffusers / PEFT and the kohya / BFL key
layouts give the same {prefix: (A, B, scale)}, fused kohya modules are split by rows, unsupported keys are listed or dropped, and an adapter
file written by hand (safetensors: 8-byte header length, JSON header, raw data) goes through the repository's own reader."""
import numpy as np
import pytest

from tests.lora_util import D, M, peft_and_kohya, write_safetensors


def assert_same(got, want):
    assert set(got) == set(want)
    for k, (A, B, s) in want.items():
        gA, gB, gs = got[k]
        np.testing.assert_array_equal(np.asarray(gA), A)
        np.testing.assert_array_equal(np.asarray(gB), B)
        assert gs == s, (k, gs, s)


def test_peft_and_kohya_layouts_read_the_same():
    from diffusion_rs_amd.lora import read_lora
    peft, kohya, want = peft_and_kohya()
    assert len(want) == 20
    assert_same(read_lora(peft), want)
    assert_same(read_lora(kohya), want)
    # the row split of the fused modules: thirds of q|k|v, and D, D, D, M of the single block's linear1, each with the SAME down projection
    got = read_lora(kohya)
    up = kohya["lora_unet_single_blocks_1_linear1.lora_up.weight"]
    for name, r0, n in (("attn.to_q", 0, D), ("attn.to_k", D, D), ("attn.to_v", 2 * D, D), ("proj_mlp", 3 * D, M)):
        A, B, s = got["single_transformer_blocks.1." + name]
        assert B.shape == (n, 4) and np.array_equal(B, up[r0:r0 + n]) and s == 16.0 / 4
        assert A is got["single_transformer_blocks.1.attn.to_q"][0]
    assert_same(read_lora(kohya, hidden_size=D), want)  # the model's D given: D, D, D, the rest
    wide = {"lora_unet_single_blocks_0_linear1.lora_down.weight": np.zeros((2, 8), np.float32), "lora_unet_single_blocks_0_linear1.lora_up.weight": np.zeros((3 * 8 + 16, 2), np.float32)}
    assert [read_lora(wide, hidden_size=8)["single_transformer_blocks.0." + p][1].shape[0] for p in ("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp")] == [8, 8, 8, 16]
    assert got["transformer_blocks.0.attn.to_k"][2] == 8.0 / 4 and got["transformer_blocks.0.attn.add_k_proj"][2] == 1.5 / 3
    assert got["transformer_blocks.0.attn.to_out.0"][2] == 1.0  # no alpha: scale 1


def test_unsupported_keys_raise_and_list_themselves_or_are_dropped():
    from diffusion_rs_amd.lora import read_lora
    peft, kohya, want = peft_and_kohya()
    z = np.zeros((2, 2), np.float32)
    bad_kohya = ["lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_down.weight", "lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_up.weight",
                 "lora_unet_final_layer_linear.lora_down.weight", "lora_unet_final_layer_adaLN_modulation_1.lora_up.weight",
                 "lora_unet_img_in.lora_down.weight", "lora_unet_txt_in.alpha", "lora_unet_time_in_in_layer.lora_up.weight",
                 "lora_unet_vector_in_out_layer.lora_down.weight", "lora_unet_guidance_in_in_layer.lora_down.weight"]
    bad_peft = ["text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight", "text_encoder_2.encoder.block.0.layer.0.SelfAttention.q.lora_B.weight"]
    for base, bad in ((kohya, bad_kohya), (peft, bad_peft)):
        d = dict(base)
        d.update({k: z for k in bad})
        with pytest.raises(ValueError) as ei:
            read_lora(d)
        for k in bad:
            assert k in str(ei.value)
        for k in base:
            assert k not in str(ei.value)
        assert_same(read_lora(d, skip_unsupported=True), want)  # exactly those keys are dropped
    with pytest.raises(ValueError):  # half a pair is an error in either mode
        read_lora({"transformer_blocks.0.attn.to_q.lora_A.weight": z}, skip_unsupported=True)
    with pytest.raises(ValueError):  # fused rows that do not split
        read_lora({"lora_unet_single_blocks_0_linear1.lora_down.weight": np.zeros((2, 8), np.float32),
                   "lora_unet_single_blocks_0_linear1.lora_up.weight": np.zeros((15, 2), np.float32)})


def test_adapter_file_round_trips_through_the_repository_reader(tmp_path):
    import torch
    from diffusion_rs_amd.lora import read_lora, read_safetensors
    peft, kohya, want = peft_and_kohya(seed=3)
    kohya = {k: (v.astype(np.float16) if "img_mlp" in k else v) for k, v in kohya.items()}  # two dtypes in one file
    path = tmp_path / "adapter.safetensors"
    write_safetensors(path, kohya)
    raw = read_safetensors(str(path))
    assert set(raw) == set(kohya)
    for k, v in kohya.items():
        assert isinstance(raw[k], torch.Tensor) and tuple(raw[k].shape) == v.shape
        np.testing.assert_array_equal(raw[k].numpy(), v)
    got = read_lora(path)
    assert set(got) == set(want)
    for k, (A, B, s) in want.items():
        gA, gB, gs = got[k]
        f16 = "ff.net" in k
        assert gA.dtype == (torch.float16 if f16 else torch.float32)
        np.testing.assert_array_equal(gA.float().numpy(), A.astype(np.float16).astype(np.float32) if f16 else A)
        np.testing.assert_array_equal(gB.float().numpy(), B.astype(np.float16).astype(np.float32) if f16 else B)
        assert gs == s
