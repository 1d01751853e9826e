#!/usr/bin/env python
"""Second-order solvers: what a step of each loop costs.  Prints the lines of profiles/solvers.txt:

    python tools/solver_bench.py [--solver none|euler|heun|dpmpp_2m] [--runs N] [--steps K] [--tree DIR]

Full-size synthetic FLUX.1-dev, bf16, S = 4096 (1024 x 1024), T = 512, B = 1, `--steps` (default 50) steps of FluxModel.denoise with the given solver; "none"
passes no solver keyword at all, which is also what a tree from before the solvers understands.  `--tree DIR` imports the package from another checkout
(with its own built library), so that the parent commit's loop and this one's run from the same script in the same session.  `--runs` (default 3) timed runs
after one warm-up, host clock around a synchronised call; ms per STEP (not per model evaluation: Heun evaluates twice per step but the last)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--solver", default="none", choices=["none", "euler", "heun", "dpmpp_2m"])
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.tree))
import diffusion_rs_amd as d  # noqa: E402
from diffusion_rs_amd import synth  # noqa: E402

dev = torch.device("cuda", 0)
S, T = 4096, 512
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
ts = sched.get_timesteps(args.steps, sched.calculate_shift(S))
kw = {} if args.solver == "none" else dict(solver=args.solver)


def run():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = flux.denoise(noise, ids, txt, txt_ids, y, guid, ts, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.steps, out


run()  # warm-up
ms = []
for _ in range(args.runs):
    v, out = run()
    assert torch.isfinite(out).all()
    ms.append(v)
print(f"tree {os.path.abspath(args.tree)} build {flux.lib.fmi_build_id().decode()[:12]}")
print(f"S=4096, T=512, B=1, {args.steps} steps, bf16, solver={args.solver}: ms/step {' '.join(f'{x:.3f}' for x in ms)}  median {np.median(ms):.3f}  spread {max(ms) - min(ms):.3f}"
      f"  (model + workspace {flux.lib.fmi_flux_size_in_bytes(flux.h) / 2**30:.2f} GiB)")
