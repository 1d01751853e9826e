"""Shared by the LoRA tests (tests/test_host_lora.py, tests/test_gpu_lora.py): a hand-written safetensors writer and one adapter in both key layouts."""
import json
import struct

import numpy as np

D, M = 256, 1024  # tests.util.SMALL_FLUX: hidden size and MLP width


def write_safetensors(path, tensors):
    """{name: float32 / float16 numpy array} -> a .safetensors file, written by hand (no dependency on the safetensors package)."""
    header, blobs, off = {}, [], 0
    for name, a in tensors.items():
        a = np.asarray(a)
        raw = a.tobytes()
        header[name] = {"dtype": {"float32": "F32", "float16": "F16"}[a.dtype.name], "shape": list(a.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    hj = json.dumps(header).encode()
    hj += b" " * (-len(hj) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(hj)) + hj + b"".join(blobs))


def peft_and_kohya(seed=0, std=1.0, rank=4):
    """The same adapter in both layouts: every kohya module kind on double block 0 and single block 1, ranks `rank` / 3, alphas on most pairs.
    Returns (peft dict, kohya dict, {prefix: (A, B, scale)})."""
    rng = np.random.default_rng(seed)
    peft, kohya, want = {}, {}, {}

    def module(kname, rows_out, k_in, r, alpha, targets, split):
        r = rank if r == 4 else r
        down = (std * rng.standard_normal((r, k_in))).astype(np.float32)
        up = (std * rng.standard_normal((rows_out, r))).astype(np.float32)
        kohya[kname + ".lora_down.weight"], kohya[kname + ".lora_up.weight"] = down, up
        if alpha is not None:
            kohya[kname + ".alpha"] = np.float32(alpha)
        r0 = 0
        for tgt, n in zip(targets, split):
            key = "transformer." + tgt if len(peft) % 2 else tgt  # the optional "transformer." prefix on every other key
            peft[key + ".lora_A.weight"], peft[key + ".lora_B.weight"] = down, up[r0:r0 + n]
            if alpha is not None:
                peft[key + ".alpha"] = np.float32(alpha)
            want[tgt] = (down, up[r0:r0 + n], 1.0 if alpha is None else alpha / r)
            r0 += n
        assert r0 == rows_out

    b0, s1 = "transformer_blocks.0.", "single_transformer_blocks.1."
    module("lora_unet_double_blocks_0_img_attn_qkv", 3 * D, D, 4, 8.0, [b0 + "attn.to_q", b0 + "attn.to_k", b0 + "attn.to_v"], [D, D, D])
    module("lora_unet_double_blocks_0_txt_attn_qkv", 3 * D, D, 3, 1.5, [b0 + "attn.add_q_proj", b0 + "attn.add_k_proj", b0 + "attn.add_v_proj"], [D, D, D])
    module("lora_unet_double_blocks_0_img_attn_proj", D, D, 4, None, [b0 + "attn.to_out.0"], [D])
    module("lora_unet_double_blocks_0_txt_attn_proj", D, D, 4, 4.0, [b0 + "attn.to_add_out"], [D])
    module("lora_unet_double_blocks_0_img_mlp_0", M, D, 4, 2.0, [b0 + "ff.net.0.proj"], [M])
    module("lora_unet_double_blocks_0_img_mlp_2", D, M, 4, 2.0, [b0 + "ff.net.2"], [D])
    module("lora_unet_double_blocks_0_txt_mlp_0", M, D, 4, 2.0, [b0 + "ff_context.net.0.proj"], [M])
    module("lora_unet_double_blocks_0_txt_mlp_2", D, M, 4, 2.0, [b0 + "ff_context.net.2"], [D])
    module("lora_unet_double_blocks_0_img_mod_lin", 6 * D, D, 3, 6.0, [b0 + "norm1.linear"], [6 * D])
    module("lora_unet_double_blocks_0_txt_mod_lin", 6 * D, D, 3, 6.0, [b0 + "norm1_context.linear"], [6 * D])
    module("lora_unet_single_blocks_1_linear1", 3 * D + M, D, 4, 16.0, [s1 + "attn.to_q", s1 + "attn.to_k", s1 + "attn.to_v", s1 + "proj_mlp"], [D, D, D, M])
    module("lora_unet_single_blocks_1_linear2", D, D + M, 4, 1.0, [s1 + "proj_out"], [D])
    module("lora_unet_single_blocks_1_modulation_lin", 3 * D, D, 3, None, [s1 + "norm.linear"], [3 * D])
    return peft, kohya, want
