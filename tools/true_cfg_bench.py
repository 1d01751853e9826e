#!/usr/bin/env python
"""True classifier-free guidance: what the CFG loop costs.  Prints part (a) of profiles/true_cfg.txt:

    python tools/true_cfg_bench.py [runs] [steps]

Full-size synthetic FLUX.1-dev, bf16, S = 4096 (1024 x 1024), T = 512, `steps` (default 50) steps: fmi_flux_denoise_cfg at B = 1 — every step evaluates the
prompt and the negative as ONE batch of two — against fmi_flux_denoise at B = 2 (the same model rows per step; only the input cast and the update kernel
differ) and against fmi_flux_denoise at B = 1 (text to image: CFG is expected near twice its step).  `runs` (default 3) runs of each, alternating in one
process after a warm-up of both (then the B = 1 loop, whose workspace has another shape, on its own), host clock around a synchronised call.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/true_cfg_bench.py 1 4

gives the kernel time of the guided update, step_kernel<4, true, false, EulerOp> (4096 x 64 elements per step, whatever the step count).

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
S, T, SCALE = 4096, 512, 4.0

cfg = d.FLUX_DEV
flux = d.FluxModel(cfg)
synth.fill_flux_random_device(flux, seed=0, device=dev)
g = torch.Generator(device=dev)
g.manual_seed(1234)
txt = torch.randn((2, T, cfg["joint_attention_dim"]), generator=g, device=dev).to(torch.bfloat16)  # row 0: the prompt, row 1: the negative (or a second prompt)
y = torch.randn((2, cfg["pooled_projection_dim"]), generator=g, device=dev)
guid = torch.full((2,), 3.5, device=dev)
txt_ids = torch.zeros((2, T, 3), device=dev)
noise, ids = d.pack_latents(d.randn_latents(2, 16, 128, 128, seed=1, device=dev))
sched = d.SchedulerConfig()
ts = sched.get_timesteps(NS, sched.calculate_shift(S))

FORMS = {
    "cfg": ("fmi_flux_denoise_cfg B=1 (prompt + negative, one batch of 2)", lambda: flux.denoise(noise[:1], ids[:1], txt[:1], txt_ids[:1], y[:1], guid[:1], ts,
                                                                                                 negative_txt=txt[1:], negative_y=y[1:], true_cfg_scale=SCALE)),
    "b2": ("fmi_flux_denoise     B=2 (two prompts)                     ", lambda: flux.denoise(noise, ids, txt, txt_ids, y, guid, ts)),
    "b1": ("fmi_flux_denoise     B=1 (text to image)                   ", lambda: flux.denoise(noise[:1], ids[:1], txt[:1], txt_ids[:1], y[:1], guid[:1], ts)),
}


def run(form):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = FORMS[form][1]()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / NS, out


res = {form: [] for form in FORMS}
# the B = 1 loop has a workspace of its own shape, and a change of shape reallocates it: CFG and the B = 2 loop (one shape) alternate first, text to image follows
for forms in (("cfg", "b2"), ("b1",)):
    for form in forms:  # warm-up
        run(form)
    for rep in range(RUNS):  # alternating, same process
        for form in forms:
            ms, out = run(form)
            assert torch.isfinite(out).all()
            res[form].append(ms)
print(f"model + workspace: {flux.lib.fmi_flux_size_in_bytes(flux.h) / 2**30:.2f} GiB")
for form, (name, _) in FORMS.items():
    v = res[form]
    print(f"S=4096, T=512, {NS} steps, bf16, {name}: ms/step {' '.join(f'{x:.3f}' for x in v)}  median {np.median(v):.3f}  spread {max(v) - min(v):.3f}")
mc, m2, m1 = (float(np.median(res[f])) for f in ("cfg", "b2", "b1"))
print(f"cfg - B=2 loop, medians: {mc - m2:+.3f} ms/step ({(mc / m2 - 1) * 100:+.2f} %); the larger spread of the two: {max(max(res[f]) - min(res[f]) for f in ('cfg', 'b2')):.3f} ms/step")
print(f"cfg / B=1 text to image, medians: {mc / m1:.3f} x per step")
