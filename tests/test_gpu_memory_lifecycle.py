"""Device memory of the model handles over their whole life: every path on which a handle allocates, regrows or retires a block is walked once
(`lifecycle()`), every handle is closed, and two things are asserted.

  * `size_in_bytes()` after each numbered step equals tests/golden/size_in_bytes_small.json, integer for integer.  That file was written by
    tests/golden/gen_size_in_bytes_small.py from this same walk on the commit BEFORE the handles' blocks became DeviceBuffer members: the accounting
    did not move.  The steps of the vision towers and the Redux embedder (8, 9) were written the same way on the commit before the five encoder handles
    came to share one frame (arena creation, workspace carving, encoder layer); steps 1 - 6 came out of that run as they were.
  * Five passes of the walk leave the device's free memory where one pass left it (no growth with the number of passes = no leaked block).

Which branch each step takes at these shapes (SMALL_FLUX: D = 256, MLP width 1024, 2 heads; read off flux_model.hip):
  1.3  set_split_k: gemm_split_k() does split here.  The double blocks' MLP-out pair (K = 1024, two problems in one launch: n * S <= 8 and K / S >= 256
       give S = 4) and the single blocks' linear2 (K = 1280 = 5 * 256: S = 4) are cut by 4 into splitk_scratch; the K = 256 projections are not (K / S < 256).
  3.1  set_quant_dense_cache(0) at 384 image rows: above Q4_FUSED_MAX_ROWS = 383, so the block launches take densify()'s per-call branch (both
       wscratch blocks are allocated, counted by size_in_bytes); the 1-row modulation GEMMs stay on the fused kernels.
  3.2  set_quant_dense_cache(1): densify()'s expand-once branch for every quantised matrix: ensure_arena() allocates the MOD and BLOCKS arenas.
The walk provokes no allocation failure, fault or hang; it only uses what the public API offers.

What the free-memory assertion can see: profiles/device_buffer_ab.txt records the step of hipMemGetInfo on this part.  Free memory moves in steps of
2 MiB: the runtime carves small blocks out of 2 MiB chunks, so one 256-byte block moved it by 2 MiB when it opened a chunk and 64 of them held at once
moved it by the same 2 MiB.  A leak of 2 MiB or more per pass is seen for certain; a 256-byte leak per pass shows only if it happens to open or pin a
chunk — below what this test can promise.  What covers those is that no hipMalloc / hipFree call is left outside DeviceBuffer and capi.hip."""
import functools
import json
import os

import numpy as np
import pytest

from tests import clip_vision_ref as CVR
from tests import redux_ref as RR
from tests.test_gpu_text import SMALL_CLIP, SMALL_T5
from tests.util import SMALL_FLUX, SMALL_VAE, dev, flux_inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "size_in_bytes_small.json")
# F1 - F5 of test_no_growth_across_passes measured three times on the commit before this test existed (raw pointers, hand-written frees): 0, 0, 0 bytes.
# The bar is the largest of the three, no margin (profiles/device_buffer_ab.txt).
DRIFT_BYTES = 0
LINEAR = "transformer_blocks.0.attn.to_q"


@functools.lru_cache(maxsize=None)
def _weights(kind):
    import diffusion_rs_amd as d
    if kind == "flux":
        return d.synth.flux_state_dict_numpy(SMALL_FLUX, seed=0)
    if kind == "vae":
        return d.synth.vae_state_dict_numpy(SMALL_VAE, seed=0, encoder=True)
    if kind == "clip_vision":
        return CVR.state_dict(CVR.CONFIGS["s56p14"])
    if kind == "siglip_vision":
        return RR.state_dict(RR.CONFIGS["h72_t16"])
    if kind == "redux":
        return RR.redux_state_dict(128, 64)
    return d.synth.text_state_dict_numpy(d.synth.t5_tensor_shapes(SMALL_T5) if kind == "t5" else d.synth.clip_tensor_shapes(SMALL_CLIP), seed=0)


def _args(S_hw, T, seed=1):
    import torch
    img, ids, txt, txt_ids, y = flux_inputs(SMALL_FLUX, 1, S_hw, T, seed=seed)
    t, g = np.array([0.75], np.float32), np.array([3.5], np.float32)
    return dev(img), dev(ids), dev(txt, torch.bfloat16), dev(txt_ids), dev(t), dev(y), dev(g)


def _forward(m, S_hw, T):
    return m.forward(*_args(S_hw, T))


def _denoise(m, S_hw, T, steps):
    img, ids, txt, txt_ids, _, y, g = _args(S_hw, T)
    return m.denoise(img, ids, txt, txt_ids, y, g, list(np.linspace(1.0, 0.0, steps + 1)))


def lifecycle():
    """One walk over every growth path of every handle; returns {step: size_in_bytes()} in step order."""
    import torch
    import diffusion_rs_amd as d
    from diffusion_rs_amd.dist import _DeviceBytes
    sizes = {}
    sd = _weights("flux")

    # ---- 1. Flux, bf16 checkpoint
    m = d.FluxModel(SMALL_FLUX)
    m.load_state_dict(sd)
    _forward(m, (8, 8), 32)
    _forward(m, (8, 16), 64)  # the workspace regrows
    sizes["1.1 forward, forward larger"] = m.size_in_bytes()
    _denoise(m, (8, 8), 32, 2)
    _denoise(m, (8, 8), 32, 3)  # the *_steps buffers regrow
    sizes["1.2 denoise 2 steps, 3 steps"] = m.size_in_bytes()
    m.set_split_k(True)
    _forward(m, (8, 8), 32)
    sizes["1.3 split-k forward"] = m.size_in_bytes()
    m.set_split_k(False)
    m.calibrate_int8(True)
    _forward(m, (8, 8), 32)
    sizes["1.4a calibrate_int8, forward"] = m.size_in_bytes()
    m.quantize_int8()
    sizes["1.4b quantize_int8"] = m.size_in_bytes()
    _forward(m, (8, 8), 32)
    sizes["1.4c forward in int8 mode"] = m.size_in_bytes()
    torch.cuda.synchronize()
    m.close()

    # ---- 2. Flux, LoRA on one Linear
    m = d.FluxModel(SMALL_FLUX)
    m.load_state_dict(sd)
    base = m.size_in_bytes()
    sizes["2.0 loaded"] = base
    rng = np.random.default_rng(5)
    out_f, in_f = sd[LINEAR + ".weight"].shape
    for name, r in (("a", 4), ("b", 16)):  # the second adapter makes the factor scratch grow: the old block is retired, not freed in place
        m.lora_add(name, LINEAR, (0.1 * rng.standard_normal((r, in_f))).astype(np.float32), (0.1 * rng.standard_normal((out_f, r))).astype(np.float32))
        sizes[f"2.1 adapter {name} of rank {r}"] = m.size_in_bytes()
    m.lora_set_weight("a", 0.0)
    sizes["2.2 weight of a = 0"] = m.size_in_bytes()
    m.lora_remove("a")
    m.lora_remove("b")
    sizes["2.3 both removed"] = m.size_in_bytes()
    assert m.size_in_bytes() == base
    m.close()

    # ---- 3. Flux, nf4 block and modulation linears
    m = d.FluxModel(SMALL_FLUX)
    for name, w in sd.items():
        if name.endswith(".weight") and (d.synth.is_block_linear(name) or ("norm" in name and "linear" in name)):
            packed, absmax = d.synth.quantize_nf4_device(dev(w, torch.bfloat16), 64)
            m.set_linear_bnb4(name[:-len(".weight")], packed, absmax, 64, "nf4", w.shape[0], w.shape[1])
        else:
            m.set_tensor(name, w)
    m.assert_complete()
    sizes["3.0 nf4 loaded"] = m.size_in_bytes()
    m.set_quant_dense_cache(0)
    _forward(m, (16, 24), 32)  # 384 image rows
    sizes["3.1 packed only: per-call expansion"] = m.size_in_bytes()
    m.set_quant_dense_cache(1)
    _forward(m, (16, 24), 32)
    sizes["3.2 dense cache: expanded once"] = m.size_in_bytes()
    torch.cuda.synchronize()
    m2 = d.FluxModel(SMALL_FLUX)  # an LLM.int8 part of a fused projection: the matrix owns its storage
    w = sd[LINEAR + ".weight"]
    scb = np.abs(w).max(1).astype(np.float32)
    m2.set_linear_int8(LINEAR, np.clip(np.rint(w / scb[:, None] * 127.0), -127, 127).astype(np.int8), scb, w.shape[0], w.shape[1])
    sizes["3.4 one int8 part of a fused projection"] = m2.size_in_bytes()
    m2.close()
    m.close()

    # ---- 4. Flux, sequence parallel: world 2 on one device, the exchange a loop-back (this rank's send block copied into every receive block)
    m = d.FluxModel(SMALL_FLUX)
    m.load_state_dict(sd)
    device = torch.device("cuda", 0)

    def loopback(send, recv, nbytes, stream):
        src = torch.as_tensor(_DeviceBytes(send, nbytes), device=device).expand(2, nbytes)
        torch.as_tensor(_DeviceBytes(recv, nbytes * 2), device=device).view(2, nbytes).copy_(src)

    m.set_sequence_parallel(0, 2, loopback)
    _forward(m, (4, 8), 16)  # this rank's half of S = 64, T = 32: sp_base is allocated
    sizes["4.2 shard of S=64, T=32"] = m.size_in_bytes()
    _forward(m, (8, 8), 32)  # another shard shape: it regrows
    sizes["4.3 shard of S=128, T=64"] = m.size_in_bytes()
    torch.cuda.synchronize()
    m.close()

    # ---- 5. T5 with one nf4 and one LLM.int8 linear
    t5 = d.T5EncoderModel(SMALL_T5)
    tsd = _weights("t5")
    q4, q8 = "encoder.block.0.layer.0.SelfAttention.q", "encoder.block.0.layer.1.DenseReluDense.wo"
    for name, w in tsd.items():
        if name == q4 + ".weight":
            packed, absmax = d.synth.quantize_nf4_device(dev(w, torch.bfloat16), 64)
            t5.set_linear_bnb4(q4, packed, absmax, 64, "nf4", w.shape[0], w.shape[1])
        elif name == q8 + ".weight":
            scb = np.abs(w).max(1).astype(np.float32)
            t5.set_linear_int8(q8, torch.from_numpy(np.clip(np.rint(w / scb[:, None] * 127.0), -127, 127).astype(np.int8)), torch.from_numpy(scb), w.shape[0], w.shape[1])
        else:
            t5.set_tensor(name, w)
    assert t5.missing() == []
    sizes["5.1 t5 loaded"] = t5.size_in_bytes()
    ids = np.random.default_rng(2).integers(0, SMALL_T5["vocab_size"], (1, 40)).astype(np.int32)
    for T in (17, 40):
        t5.forward(ids[:, :T])
        sizes[f"5.2 t5 forward T={T}"] = t5.size_in_bytes()
    torch.cuda.synchronize()
    t5.close()

    # ---- 6. CLIP
    clip = d.ClipTextTransformer(SMALL_CLIP)
    clip.load_state_dict(_weights("clip"))
    ids = np.random.default_rng(3).integers(1, SMALL_CLIP["vocab_size"], (1, 33)).astype(np.int32)
    for T in (9, 33):
        clip.forward(ids[:, :T])
        sizes[f"6.1 clip forward T={T}"] = clip.size_in_bytes()
    torch.cuda.synchronize()
    clip.close()

    # ---- 7. VAE (no size_in_bytes: it only takes part in the free-memory assertion)
    vae = d.AutoEncoderKl(SMALL_VAE)
    vae.load_state_dict(_weights("vae"))
    z = np.random.default_rng(4).standard_normal((1, 16, 4, 6)).astype(np.float32)
    vae.decode(dev(z[:, :, :3, :5]))
    vae.decode(dev(z))  # the workspace regrows
    vae.encode(dev(np.random.default_rng(6).uniform(-1, 1, (1, 3, 32, 48)).astype(np.float32)))
    torch.cuda.synchronize()
    vae.close()

    # ---- 8. CLIP vision tower (s56p14: 17 tokens)
    cv = d.ClipVisionModel(CVR.CONFIGS["s56p14"])
    cv.load_state_dict(_weights("clip_vision"))
    sizes["8.0 clip vision loaded"] = cv.size_in_bytes()
    pix = CVR.pixel_values(CVR.CONFIGS["s56p14"], 2)
    for B in (1, 2):  # the workspace regrows
        cv.forward(pix[:B])
        sizes[f"8.1 clip vision forward B={B}"] = cv.size_in_bytes()
    torch.cuda.synchronize()
    cv.close()

    # ---- 9. SigLIP vision tower (h72_t16: heads and MLP padded in the weights) and the Redux embedder
    sv = d.SiglipVisionModel(RR.CONFIGS["h72_t16"])
    sv.load_state_dict(_weights("siglip_vision"))
    sizes["9.0 siglip vision loaded"] = sv.size_in_bytes()
    sv.poison_workspace(1)  # the test seam allocates the workspace of a batch of 1
    sizes["9.1 siglip vision poison_workspace(1)"] = sv.size_in_bytes()
    pix = RR.pixel_values(RR.CONFIGS["h72_t16"], 2)
    for B in (1, 2):
        sv.forward(pix[:B])
        sizes[f"9.2 siglip vision forward B={B}"] = sv.size_in_bytes()
    torch.cuda.synchronize()
    sv.close()
    rx = d.ReduxImageEmbedder(128, 64)
    rx.load_state_dict(_weights("redux"))
    sizes["9.3 redux loaded"] = rx.size_in_bytes()
    hidden = np.random.default_rng(7).standard_normal((81, 128)).astype(np.float32)
    for rows in (16, 81):
        rx.forward(hidden[:rows])
        sizes[f"9.4 redux forward rows={rows}"] = rx.size_in_bytes()
    torch.cuda.synchronize()
    rx.close()
    return sizes


def _settle():
    import ctypes as C
    import torch
    from diffusion_rs_amd import _lib
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    _lib.check(_lib.load().fmi_release_scratch(C.POINTER(C.c_size_t)()))


@pytest.fixture(scope="module")
def first_pass():
    """The first walk: the sizes test reads it, and it is the warm-up (every code object loaded) of the free-memory test."""
    import torch
    sizes = lifecycle()
    _settle()
    return sizes, torch.cuda.mem_get_info()[0]


def test_size_in_bytes_at_every_step_is_what_it_was(first_pass):
    sizes, _ = first_pass
    with open(GOLDEN) as f:
        want = json.load(f)
    for k, v in sizes.items():
        print(f"{k}: {v}")
    assert sizes == want


def test_no_growth_across_passes(first_pass):
    import torch
    _, f1 = first_pass
    for _ in range(4):
        lifecycle()
        _settle()
    f5 = torch.cuda.mem_get_info()[0]
    print(f"free after pass 1: {f1}, after pass 5: {f5}, F1 - F5 = {f1 - f5} bytes (bar {DRIFT_BYTES})")
    assert f1 - f5 <= DRIFT_BYTES
