#!/usr/bin/env python
"""Channel-concatenated conditioning (FLUX.1 Fill): what the wider embedder costs.  Prints part (a) of profiles/control.txt:

    python tools/control_bench.py [runs] [steps]

Two full-size synthetic FLUX.1-dev models in one process, bf16, S = 4096 (1024 x 1024), T = 512, B = 1, `steps` (default 50) steps: the 384-channel model
(in_channels 384, out_channels 64: fmi_flux_denoise_control with a (1, 4096, 320) conditioning) against the plain 64-channel model (fmi_flux_denoise).  Per step
the conditioned loop differs in the state cast (fmi_cast_cols_bf16 into columns [0, 64) of the (4096, 384) operand instead of a contiguous cast) and in the
x_embedder GEMM (K = 384 instead of 64); the conditioning columns are written once per call.  `runs` (default 3) runs of each, alternating after a warm-up of
both, host clock around a synchronised call.  Also times the glue once: fmi_mask_image and fmi_fill_condition at 1024 x 1024 (hipEvents, 20 launches).

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
NS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
dev = torch.device("cuda", 0)
S, T = 4096, 512

models = {}
for name, cfg in (("fill", dict(d.FLUX_DEV, in_channels=384, out_channels=64)), ("plain", d.FLUX_DEV)):
    m = d.FluxModel(cfg)
    synth.fill_flux_random_device(m, seed=0, device=dev)
    models[name] = m
cfg = d.FLUX_DEV
g = torch.Generator(device=dev)
g.manual_seed(1234)
txt = torch.randn((1, T, cfg["joint_attention_dim"]), generator=g, device=dev).to(torch.bfloat16)
y = torch.randn((1, cfg["pooled_projection_dim"]), generator=g, device=dev)
guid = torch.full((1,), 3.5, device=dev)
txt_ids = torch.zeros((1, T, 3), device=dev)
noise, ids = d.pack_latents(d.randn_latents(1, 16, 128, 128, seed=1, device=dev))
image = torch.rand((1, 3, 1024, 1024), generator=g, device=dev) * 2 - 1
mask = (torch.rand((1, 1024, 1024), generator=g, device=dev) > 0.5).float()
lat = torch.randn((1, S, 64), generator=g, device=dev)
cond = d.fill_condition(lat, mask)
sched = d.SchedulerConfig()
ts = sched.get_timesteps(NS, sched.calculate_shift(S))

FORMS = {
    "fill": ("fmi_flux_denoise_control, in_channels 384 (Fill)", lambda: models["fill"].denoise(noise, ids, txt, txt_ids, y, guid, ts, control=cond)),
    "plain": ("fmi_flux_denoise,         in_channels  64        ", lambda: models["plain"].denoise(noise, ids, txt, txt_ids, y, guid, ts)),
}


def run(form):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = FORMS[form][1]()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / NS, out


res = {form: [] for form in FORMS}
for form in FORMS:  # warm-up
    run(form)
for rep in range(RUNS):  # alternating, same process
    for form in FORMS:
        ms, out = run(form)
        assert torch.isfinite(out).all()
        res[form].append(ms)
for name, m in models.items():
    print(f"{name}: model + workspace {m.size_in_bytes() / 2**30:.3f} GiB")
for form, (name, _) in FORMS.items():
    v = res[form]
    print(f"S=4096, T=512, B=1, {NS} steps, bf16, {name}: ms/step {' '.join(f'{x:.3f}' for x in v)}  median {np.median(v):.3f}  spread {max(v) - min(v):.3f}")
mf, mp = (float(np.median(res[f])) for f in ("fill", "plain"))
print(f"fill - plain, medians: {mf - mp:+.3f} ms/step ({(mf / mp - 1) * 100:+.2f} %); the larger spread of the two: {max(max(v) - min(v) for v in res.values()):.3f} ms/step")


def events(fn, n=20):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


op = torch.empty((S, 384), dtype=torch.bfloat16, device=dev)
print(f"fmi_mask_image 1 x 3 x 1024 x 1024 (12.6 MB in, 4.2 MB mask, 12.6 MB out): {events(lambda: d.mask_image(image, mask)):.1f} us (with the output's allocation)")
print(f"fmi_fill_condition 1024 x 1024 (1 MB latents + 4.2 MB mask in, 5.2 MB out)  : {events(lambda: d.fill_condition(lat, mask)):.1f} us (with the output's allocation)")
print(f"fmi_cast_cols_bf16 state (4096, 64) f32 -> columns [0, 64) of (4096, 384)    : {events(lambda: d.cast_cols_bf16(noise[0], op, 0)):.1f} us")
print(f"fmi_cast_cols_bf16 conditioning (4096, 320) f32 -> columns [64, 384)         : {events(lambda: d.cast_cols_bf16(cond[0], op, 64)):.1f} us")
