#!/usr/bin/env python
"""FLUX IP-Adapter: what the image prompt costs.  Prints the body of profiles/ip_adapter.txt:

    python tools/ip_adapter_bench.py [runs] [steps] [--plain-only]

One full-size synthetic FLUX.1-dev model and an XLabs-sized adapter (E = 768, N = 4) in one process, bf16, S = 4096 (1024 x 1024), T = 512, B = 1.
  (a) the kernel alone: fmi_ip_attention on (1, 4096, 24 heads) for N = 4 and N = 32, hipEvents over 50 launches; GB/s from the bytes the algorithm needs
      (q once, x read and written once, K / V once);
  (b) the denoise loop with the adapter against the plain loop, `steps` (default 50) and 10 steps, `runs` (default 3) runs of each, alternating after a warm-up of
      both, host clock around a synchronised call.  extra(n) = a + b * n over the two lengths gives the per-step cost b (the once-per-call part a is below the
      loops' spread and is measured in (c));
  (c) the projection: FluxModel.forward projects at every call, so forward with the adapter minus forward without it, minus b, is the projection (hipEvents over 20
      calls of each, alternating three times).
--plain-only: the plain loop alone, with the sha256 of its latents — the same script runs on this commit's library and on its parent's (FMI_LIB=...) for the A/B."""
import hashlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffusion_rs_amd as d  # noqa: E402
from diffusion_rs_amd import synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
PLAIN_ONLY = "--plain-only" in sys.argv
RUNS = int(args[0]) if len(args) > 0 else 3
NS = int(args[1]) if len(args) > 1 else 50
dev = torch.device("cuda", 0)
S, T, H, D = 4096, 512, 24, 3072
cfg = d.FLUX_DEV

model = d.FluxModel(cfg)
synth.fill_flux_random_device(model, seed=0, device=dev)
g = torch.Generator(device=dev)
g.manual_seed(1234)
txt = torch.randn((1, T, cfg["joint_attention_dim"]), generator=g, device=dev).to(torch.bfloat16)
y = torch.randn((1, cfg["pooled_projection_dim"]), generator=g, device=dev)
guid = torch.full((1,), 3.5, device=dev)
txt_ids = torch.zeros((1, T, 3), device=dev)
noise, ids = d.pack_latents(d.randn_latents(1, 16, 128, 128, seed=1, device=dev))
sched = d.SchedulerConfig()
schedule = lambda n: sched.get_timesteps(n, sched.calculate_shift(S))


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n, out


if PLAIN_ONLY:
    ts = schedule(NS)
    plain = lambda: model.denoise(noise, ids, txt, txt_ids, y, guid, ts)
    timed(plain, NS)
    v = []
    for _ in range(RUNS):
        ms, out = timed(plain, NS)
        v.append(ms)
    sha = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
    print(f"plain loop, {NS} steps, library {os.environ.get('FMI_LIB', 'of this tree')}: ms/step {' '.join(f'{x:.3f}' for x in v)}   latents sha256 {sha}")
    sys.exit(0)

E, N = 768, 4
ada = d.FluxIPAdapter(cfg, E, N)
synth.fill_ip_adapter_random_device(ada, seed=2, device=dev)
emb = torch.randn((1, E), generator=g, device=dev)


def events(fn, n=50):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


# (a) the kernel alone, on the q third of a (1, S, 3 D) projection as the model lays it out
qkv = torch.randn((1, S, 3, H, 128), generator=g, device=dev).to(torch.bfloat16)
wq = torch.ones(128, dtype=torch.bfloat16, device=dev)
x = torch.randn((1, S, D), generator=g, device=dev)
for n in (4, 32):
    k = torch.randn((1, H, n, 128), generator=g, device=dev).to(torch.bfloat16)
    v = torch.randn((1, H, n, 128), generator=g, device=dev).to(torch.bfloat16)
    us = events(lambda: d.ip_attention(qkv[:, :, 0], wq, k, v, x, 0.001))
    nbytes = S * D * 2 + 2 * S * D * 4 + 2 * H * n * 128 * 2
    print(f"fmi_ip_attention B=1 S=4096 H=24 N={n}: {us:.1f} us a launch over 50 back-to-back launches, {nbytes / 1e6:.1f} MB needed -> {nbytes / us / 1e3:.0f} GB/s "
          f"(x, 50 MB, stays in the 256 MB Infinity Cache between launches of this loop)")

# (b) the loop
forms = {}
for n in (NS, 10):
    ts = schedule(n)
    forms[("plain", n)] = (lambda ts=ts: model.denoise(noise, ids, txt, txt_ids, y, guid, ts))
    forms[("adapter", n)] = (lambda ts=ts: model.denoise(noise, ids, txt, txt_ids, y, guid, ts, ip_adapter=ada, ip_adapter_image_embeds=emb, ip_adapter_scale=0.7))
res = {k: [] for k in forms}
for k, fn in forms.items():
    timed(fn, k[1])
for rep in range(RUNS):
    for k, fn in forms.items():
        ms, out = timed(fn, k[1])
        assert torch.isfinite(out).all()
        res[k].append(ms)
for k, v in res.items():
    print(f"{k[0]:8s} loop, {k[1]:3d} steps: ms/step {' '.join(f'{x:.3f}' for x in v)}   median {np.median(v):.3f}   spread {max(v) - min(v):.3f}")
med = {k: float(np.median(v)) for k, v in res.items()}
extra_long, extra_short = (med[("adapter", NS)] - med[("plain", NS)]) * NS, (med[("adapter", 10)] - med[("plain", 10)]) * 10
b = (extra_long - extra_short) / (NS - 10)
a = extra_short - 10 * b
print(f"extra over the plain loop: {extra_long:.2f} ms in {NS} steps, {extra_short:.2f} ms in 10 steps -> per step {b:.3f} ms ({b / med[('plain', NS)] * 100:+.2f} % of the plain step), "
      f"once-per-call remainder of the fit {a:.2f} ms (below the spread of the loops: see the single evaluations)")
# (c) the projection, from single evaluations
tvec = torch.full((1,), 0.5, device=dev)
fplain = lambda: model.forward(noise, ids, txt, txt_ids, tvec, y, guid)
fada = lambda: model.forward(noise, ids, txt, txt_ids, tvec, y, guid, ip_adapter=ada, ip_adapter_image_embeds=emb, ip_adapter_scale=0.7)
fp, fa = [], []
for rep in range(3):
    fp.append(events(fplain, 20) / 1e3)
    fa.append(events(fada, 20) / 1e3)
print(f"single evaluation (no hoisting), ms: plain {' '.join(f'{v:.3f}' for v in fp)}   adapter {' '.join(f'{v:.3f}' for v in fa)}")
print(f"adapter - plain, medians: {np.median(fa) - np.median(fp):.3f} ms = the projection + the per-step cost -> projection {np.median(fa) - np.median(fp) - b:.3f} ms once per call")
print(f"adapter: weights + projection buffers {ada.size_in_bytes() / 2**30:.3f} GiB")
