#!/usr/bin/env python
"""Generate tests/golden/c2_trajectory.npz (committed as the pieces .npz.00, .01, ...: tests/util.py save_split_npz) — the HEADLINE config pinned at full size and full length (VERDICT r5 "next" 2).

BASELINE configs[1]: FLUX.1-dev, D = 3072, 19 + 38 blocks, 1024 x 1024 (S = 4096 image tokens) + T = 512 text tokens, guidance 3.5,
the real 50-step dynamic-shift schedule: `Sampler::sample` (pipelines/sampling.rs:25-48) around the step closure
(pipelines/flux/mod.rs:305-318), then unpack + latent affine + `AutoEncoderKl::decode` + the u8 cast (pipelines/flux/mod.rs:320-332) —
executed by the f32 CPU ORACLE (oracle/flux_oracle.cpp; no reference code runs: the reference is Rust and cannot be built here).
3.7e15 FLOP: about two hours on the 8 cores of the build container, which is why the result is a committed fixture rather than a live
oracle call in the GPU suite.

What makes a committed fixture possible without shipping 24 GB of weights: every tensor of the synthetic checkpoint, the latent noise and
the text embeddings are "exact synthetic tensors" (diffusion-rs_amd/synth.py: Philox4x32-10 words seeded by the tensor's name -> byte sums
-> one f32 multiply -> bf16), bit-identical on this CPU (oracle Philox) and on the GPU box (fmi_philox_u32) — the GPU test regenerates them.

The fixture holds: the 51 timesteps, the oracle's f32 latents after 10 / 25 / 50 steps (1 MB each), the oracle's u8 image (3 MB) and its
CRC-32, CRC-32s of three weight tensors and the inputs (so the GPU side can prove it regenerated the same bits), and the per-step wall times.

Run:   OMP_WAIT_POLICY=passive python tests/golden/gen_c2_trajectory_fixture.py [--threads 7] [--scratch /tmp/c2_traj]
Resumable: the latents after every step are kept under --scratch; a rerun continues from the last finished step.
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import diffusion_rs_amd as d  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests.util import save_split_npz  # noqa: E402

S_ = d.synth
MARKS = (10, 25, 50)
# --config: c2 = BASELINE configs[1] (1024 x 1024: latent 128 x 128, S = 4096), c5 = the shape of configs[4] (1280 x 720: latent 90 x 160, S = 3600: every ragged path)
CONFIGS = {"c2": (128, 128, "FLUX.1-dev 1024x1024 50-step, S=4096 + T=512, guidance 3.5 (BASELINE configs[1])"),
           "c5": (90, 160, "FLUX.1-dev 1280x720 50-step, S=3600 + T=512, guidance 3.5 (the shape of BASELINE configs[4], one sample, f32 semantics)"),
           # o2 = the headline shape on the OUTLIER-CHANNEL checkpoint (synth.apply_outlier_profile on the exact synthetic tensors: AdaLN (1 + scale) of 30-100 on 12 hidden
           # channels in every block, massive residual channels, x 3 QkNorm dimensions): what the int8 mode's calibrated smoothing is held to over a whole trajectory
           "o2": (128, 128, "FLUX.1-dev 1024x1024 50-step, S=4096 + T=512, guidance 3.5, OUTLIER-CHANNEL checkpoint (synth.apply_outlier_profile)")}
H_LAT = W_LAT = 128
D_MODEL = 3072
TAG = "c2"
T_TXT = 512
GUIDANCE = 3.5
N_STEPS = 50
CRC_TENSORS = ("transformer_blocks.0.attn.to_q.weight", "single_transformer_blocks.37.proj_out.weight", "transformer_blocks.7.attn.norm_q.weight",
               "transformer_blocks.11.norm1.linear.bias", "single_transformer_blocks.20.norm.linear.bias", "x_embedder.bias")


def raw(n, seed):
    return orc.philox_u32_c(n, 1, seed)[0]


def inputs():
    """(latent (1,16,128,128), t5 (1,512,4096), clip (1,768)): f32 arrays of bf16-representable values; the GPU test builds the same"""
    cfg = d.FLUX_DEV
    lat = S_.exact_tensor_np(f"input.{TAG}.latent", (1, 16, H_LAT, W_LAT), raw, "input")
    t5 = S_.exact_tensor_np(f"input.{TAG}.t5", (1, T_TXT, cfg["joint_attention_dim"]), raw, "input")
    clip = S_.exact_tensor_np(f"input.{TAG}.clip", (1, cfg["pooled_projection_dim"]), raw, "input")
    return lat, t5, clip


def bits_crc(a_f32):
    return zlib.crc32((np.ascontiguousarray(a_f32, np.float32).view(np.uint32) >> 16).astype(np.uint16).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=max(1, orc.usable_cpus() - 1))
    ap.add_argument("--config", choices=sorted(CONFIGS), default="c2")
    ap.add_argument("--scratch", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=N_STEPS, help="(debug) stop after this many steps; the fixture is only written at 50")
    a = ap.parse_args()
    global H_LAT, W_LAT, TAG
    TAG = a.config
    H_LAT, W_LAT, desc = CONFIGS[TAG]
    a.scratch = a.scratch or f"/tmp/{TAG}_traj"
    a.out = a.out or os.path.join(ROOT, "tests", "golden", f"{TAG}_trajectory.npz")
    os.makedirs(a.scratch, exist_ok=True)
    orc.set_threads(a.threads)
    cfg = dict(d.FLUX_DEV)
    global D_MODEL
    D_MODEL = cfg["num_attention_heads"] * sum(cfg["axes_dim"])
    t0 = time.time()
    om = orc.Flux(cfg)
    shapes = S_.flux_tensor_shapes(cfg)
    buf = np.empty(max(int(np.prod(s)) for s in shapes.values()), np.uint16)
    crcs = {}
    n_w = 0
    for name, shape in shapes.items():
        n = int(np.prod(shape))
        off, sc = S_.exact_rule(name, shape, "flux")
        b = orc.exact_bf16(n, S_.exact_seed(name), off, S_.exact_coeff(sc), buf)
        if TAG == "o2" and S_.outlier_profile_touches(name):
            # the profile edits a few rows / columns / entries: in f32 on the bf16 values, re-rounded to bf16 — the arithmetic of the same in-place edit on a torch bf16 tensor
            f = (b.astype(np.uint32) << 16).view(np.float32).reshape(shape)
            g2 = S_.apply_outlier_profile(name, f.copy(), D_MODEL)
            if not np.array_equal(g2, f):
                b = (S_.to_bf16_f32(g2).view(np.uint32) >> 16).astype(np.uint16).reshape(-1)
        om.set_tensor_bf16(name, b)
        if name in CRC_TENSORS:
            crcs[name] = zlib.crc32(b.tobytes())
        n_w += n
    print(f"[gen] {n_w / 1e9:.2f}e9 exact synthetic weights in the oracle (bf16 bits, widened per block) in {time.time() - t0:.0f} s", flush=True)
    lat, t5, clip = inputs()
    crcs[f"input.{TAG}.latent"], crcs[f"input.{TAG}.t5"], crcs[f"input.{TAG}.clip"] = bits_crc(lat), bits_crc(t5), bits_crc(clip)
    img, ids = orc.pack_latents(lat)
    assert img.shape == (1, (H_LAT // 2) * (W_LAT // 2), 64)
    txt_ids = np.zeros((1, T_TXT, 3), np.float32)
    g = np.array([GUIDANCE], np.float32)
    ts = np.array(orc.get_timesteps(N_STEPS, True, orc.calculate_shift(img.shape[1]), 1.0), np.float64)
    assert len(ts) == N_STEPS + 1
    # resume
    cur, done, step_s = img.copy(), 0, []
    state = os.path.join(a.scratch, "state.npz")
    if os.path.exists(state):
        z = np.load(state)
        if np.array_equal(z["ts"], ts) and int(z["crc_img0"]) == zlib.crc32(img.tobytes()):
            cur, done, step_s = z["cur"].copy(), int(z["done"]), list(z["step_s"])
            print(f"[gen] resuming after step {done}", flush=True)
    for s in range(done, min(a.steps, N_STEPS)):
        t1 = time.time()
        cur = om.denoise(cur, ids, t5, txt_ids, clip, g, ts[s:s + 2])
        step_s.append(time.time() - t1)
        assert np.isfinite(cur).all()
        if (s + 1) in MARKS:
            np.save(os.path.join(a.scratch, f"lat_{s + 1}.npy"), cur)
        np.savez(state + ".tmp.npz", cur=cur, done=s + 1, ts=ts, step_s=np.array(step_s), crc_img0=zlib.crc32(img.tobytes()))
        os.replace(state + ".tmp.npz", state)
        print(f"[gen] step {s + 1}/{N_STEPS}: {step_s[-1]:.0f} s, latents moved {np.linalg.norm(cur - img) / np.linalg.norm(img):.4f}", flush=True)
    if min(a.steps, N_STEPS) < N_STEPS:
        return
    marks = {n: np.load(os.path.join(a.scratch, f"lat_{n}.npy")) for n in MARKS}
    del om
    # the image: unpack + affine + the real-config decoder + u8 (pipelines/flux/mod.rs:320-332)
    vcfg = d.VAE_FLUX
    ov = orc.Vae(vcfg)
    ov.load({name: S_.exact_tensor_np(name, shape, raw, "vae") for name, shape in S_.vae_tensor_shapes(vcfg).items()})
    z = orc.unpack_latents(marks[50], 16, H_LAT, W_LAT) * np.float32(1.0 / vcfg["scaling_factor"]) + np.float32(vcfg["shift_factor"])
    t1 = time.time()
    u8 = orc.postprocess_u8(ov.decode(z.astype(np.float32)))
    print(f"[gen] VAE decode + u8 in {time.time() - t1:.0f} s; image CRC-32 {zlib.crc32(u8.tobytes()):08x}, saturated {float(((u8 == 0) | (u8 == 255)).mean()):.3f}", flush=True)
    meta = dict(config=desc, tag=TAG, latent_hw=[H_LAT, W_LAT], marks=list(MARKS), crcs=crcs,
                image_crc32=zlib.crc32(u8.tobytes()), oracle_threads=a.threads, total_oracle_s=float(np.sum(step_s)), exact_salt=S_.EXACT_SALT,
                generator="tests/golden/gen_c2_trajectory_fixture.py")
    size = save_split_npz(a.out, ts=ts, u8=u8, step_s=np.array(step_s, np.float32), meta=np.frombuffer(json.dumps(meta).encode(), np.uint8),
                          **{f"lat_{n}": marks[n].astype(np.float32) for n in MARKS})
    print(f"[gen] wrote {a.out}.00, .01, ... ({size / 2**20:.1f} MiB); oracle time {np.sum(step_s) / 3600:.2f} h", flush=True)


if __name__ == "__main__":
    main()
