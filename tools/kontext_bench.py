#!/usr/bin/env python
"""Reference-image (FLUX.1 Kontext) conditioning: what the context loop costs.  Prints part (a) of profiles/kontext.txt:

    python tools/kontext_bench.py [runs]

Full-size synthetic FLUX.1-dev, bf16, B = 1, T = 512, a 1024 x 1024 output (S = 4096) and a 1024 x 1024 reference (R = 4096): fmi_flux_denoise_context
against fmi_flux_denoise on the 8192-row concatenation — the same evaluation length L = 8704, the second with the final layer and the update on all
8192 rows — 50 steps each, `runs` (default 3) runs of each alternating in one process after a warm-up of both, host clock around a synchronised call.
Also one evaluation of each form compared bit for bit at this size (the tests do that at small shapes only).

Part (b) of the profile is bench.py itself, run alternately from this commit's tree and from its parent's."""
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
S, R, T, NS = 4096, 4096, 512, 50

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
ctx, _ = d.pack_latents(d.randn_latents(1, 16, 128, 128, seed=2, device=dev))
rids = d.latent_ids(1, 64, 64, id0=1.0, device=dev)
cat, cat_ids = torch.cat([noise, ctx], 1), torch.cat([ids, rids], 1)
sched = d.SchedulerConfig()
ts = sched.get_timesteps(NS, sched.calculate_shift(S))

# one evaluation of each form at L = 8704: the first at this length
t1 = torch.full((1,), 0.7, device=dev)
p_ctx = flux.forward(noise, ids, txt, txt_ids, t1, y, guid, context=ctx, context_ids=rids)
p_cat = flux.forward(cat, cat_ids, txt, txt_ids, t1, y, guid)[:, :S]
p_plain = flux.forward(noise, ids, txt, txt_ids, t1, y, guid)
torch.cuda.synchronize()
print(f"one evaluation at L = T + S + R = {T + S + R}: finite {bool(torch.isfinite(p_ctx).all())}, forward(context=) == forward(cat)[:, :S] bit for bit: "
      f"{torch.equal(p_ctx, p_cat)}; rel-L2 to the evaluation without the context {float((p_ctx - p_plain).norm() / p_plain.norm()):.3e}")
print(f"model + workspace at this shape: {flux.lib.fmi_flux_size_in_bytes(flux.h) / 2**30:.2f} GiB")


def run(context):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if context:
        out = flux.denoise(noise, ids, txt, txt_ids, y, guid, ts, context=ctx, context_ids=rids)
    else:
        out = flux.denoise(cat, cat_ids, txt, txt_ids, y, guid, ts)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / NS, out


run(True), run(False)  # warm-up of both
res = {True: [], False: []}
for rep in range(RUNS):  # alternating, same process
    for context in (True, False):
        ms, out = run(context)
        assert torch.isfinite(out).all()
        res[context].append(ms)
for context in (True, False):
    v = res[context]
    name = "fmi_flux_denoise_context (S=4096 state + R=4096 context)" if context else "fmi_flux_denoise on the 8192-row concatenation      "
    print(f"B=1, T=512, 50 steps, bf16, {name}: ms/step {' '.join(f'{x:.3f}' for x in v)}  median {np.median(v):.3f}  spread {max(v) - min(v):.3f}")
mc, mp = np.median(res[True]), np.median(res[False])
print(f"context - concatenation, medians: {mc - mp:+.3f} ms/step ({(mc / mp - 1) * 100:+.2f} %)")
