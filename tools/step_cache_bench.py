#!/usr/bin/env python
"""First-block step cache: what the bookkeeping costs and what a reused step costs.  Prints part (a) of profiles/step_cache.txt:

    python tools/step_cache_bench.py [runs]

Full-size synthetic FLUX.1-dev, bf16, B = 1, T = 512, 1024 x 1024 (S = 4096), 50 steps: fmi_flux_denoise against fmi_flux_denoise_cached with FORCED masks
of 0 %, 50 %, 80 % reuse and with every step but the first reused, `runs` (default 3) runs of each alternating in one process after a warm-up of all, host
clock around a synchronised call.  The 0 % mask is the price of the bookkeeping (the X0 copy, the residual / distance pass with its device-to-host copy and
stream synchronisation per step, the delta pass).  The masks are forced on purpose: random weights move block 0's residual by about 0.14 per step, which says
nothing about a real checkpoint, so a speed-up driven by a threshold on synthetic weights would be meaningless.

Part (b) of the profile is bench.py itself, run alternately on this commit's library and on its parent's."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffusion_rs_amd as d  # noqa: E402
from diffusion_rs_amd import synth  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
dev = torch.device("cuda", 0)
S, T, NS = 4096, 512, 50

cfg = d.FLUX_DEV
flux = d.FluxModel(cfg)
synth.fill_flux_random_device(flux, seed=0, device=dev)
g = torch.Generator(device=dev)
g.manual_seed(1234)
txt = torch.randn((1, T, cfg["joint_attention_dim"]), generator=g, device=dev).to(torch.bfloat16)
y = torch.randn((1, cfg["pooled_projection_dim"]), generator=g, device=dev)
guid = torch.full((1,), 3.5, device=dev)
txt_ids = torch.zeros((1, T, 3), device=dev)
noise, ids = d.pack_latents(d.randn_latents(1, 16, 128, 128, seed=1, device=dev))
sched = d.SchedulerConfig()
ts = sched.get_timesteps(NS, sched.calculate_shift(S))

MASKS = {
    "plain fmi_flux_denoise            ": None,
    "cached, forced  0 % reuse (0 / 50)": [0] * NS,
    "cached, forced 50 % reuse (25 / 50)": [i % 2 for i in range(NS)],
    "cached, forced 80 % reuse (40 / 50)": [int(i % 5 != 0) for i in range(NS)],
    "cached, all but step 0   (49 / 50)": [0] + [1] * (NS - 1),
}


def run(mask):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if mask is None:
        out = flux.denoise(noise, ids, txt, txt_ids, y, guid, ts)
    else:
        out, st = flux.denoise(noise, ids, txt, txt_ids, y, guid, ts, cache_force=mask, return_cache_stats=True)
        assert st["decisions"].tolist() == mask
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


for m in MASKS.values():  # warm-up of all
    run(m)
print(f"step-cache buffers at this shape: {flux.step_cache_bytes() / 2**20:.1f} MiB")
res = {k: [] for k in MASKS}
outs = {}
for rep in range(RUNS):  # alternating, same process
    for k, m in MASKS.items():
        ms, out = run(m)
        assert torch.isfinite(out).all()
        res[k].append(ms)
        outs[k] = out
keys = list(MASKS)
for k in keys:
    v = res[k]
    print(f"B=1, S=4096, T=512, 50 steps, bf16, {k}: ms/image {' '.join(f'{x:.1f}' for x in v)}  median {np.median(v):.1f}  spread {max(v) - min(v):.1f}"
          f"  ({np.median(v) / NS:.3f} ms per step on average)")
med = {k: float(np.median(res[k])) for k in keys}
plain, zero = med[keys[0]], med[keys[1]]
print(f"bookkeeping on a computed step (0 % mask - plain, medians): {(zero - plain) / NS:+.3f} ms per step ({(zero / plain - 1) * 100:+.2f} %); "
      f"0 % mask == plain bit for bit: {torch.equal(outs[keys[0]], outs[keys[1]])}")
computed = zero / NS
for k, n_reused in ((keys[2], 25), (keys[3], 40), (keys[4], 49)):
    reused = (med[k] - (NS - n_reused) * computed) / n_reused
    print(f"{k.strip()}: {med[k] / plain:.3f} x the plain image time (speed-up {plain / med[k]:.2f} x); one reused step {reused:.3f} ms "
          f"(a computed step with the bookkeeping: {computed:.3f} ms)")
