#!/usr/bin/env python
"""Image to image / inpainting: what the masked loop and its glue cost.  Prints the measurements of profiles/img2img.txt, one part per process:

    python tools/img2img_bench.py loop     # fmi_flux_denoise_inpaint against fmi_flux_denoise, full-size synthetic FLUX.1-dev at the headline shape
                                           # (B = 1, S = 4096 + T = 512, 50 steps), alternating in one process, host clock around a synchronised call
    python tools/img2img_bench.py glue     # fmi_vae_encode at 1024 x 1024 and the glue entries through their Python wrappers (device events)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/img2img_bench.py trace
                                           # kernel times by name: the glue kernels at 1024 x 1024 and the blend at 4096 x 64 elements
                                           # (small model: the blend only sees the element count)
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffusion_rs_amd as d  # noqa: E402
from diffusion_rs_amd import synth  # noqa: E402

part = sys.argv[1]
dev = torch.device("cuda", 0)
H = W = 1024
S, T, NS = 4096, 512, 50


def events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def loop_inputs(cfg, B=1, T=T):
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    txt = torch.randn((B, T, cfg["joint_attention_dim"]), generator=g, device=dev).to(torch.bfloat16)
    y = torch.randn((B, cfg["pooled_projection_dim"]), generator=g, device=dev)
    guid = torch.full((B,), 3.5, device=dev)
    txt_ids = torch.zeros((B, T, 3), device=dev)
    noise, ids = d.pack_latents(d.randn_latents(B, 16, 128, 128, seed=1, device=dev))
    x0, _ = d.pack_latents(d.randn_latents(B, 16, 128, 128, seed=2, device=dev))
    mask = d.latent_mask((torch.rand((B, H, W), generator=g, device=dev) < 0.5).float(), 16)
    return txt, y, guid, txt_ids, noise, ids, x0, mask


if part == "loop":
    flux = d.FluxModel(d.FLUX_DEV)
    synth.fill_flux_random_device(flux, seed=0, device=dev)
    txt, y, guid, txt_ids, noise, ids, x0, mask = loop_inputs(d.FLUX_DEV)
    sched = d.SchedulerConfig()
    ts = sched.get_timesteps(NS, sched.calculate_shift(S))

    def run(masked):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = flux.denoise(noise, ids, txt, txt_ids, y, guid, ts, **(dict(x0=x0, noise=noise, mask=mask) if masked else {}))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / NS, out

    run(False), run(True)  # warm-up of both
    res = {False: [], True: []}
    for rep in range(4):  # alternating, same process
        for masked in (False, True):
            ms, out = run(masked)
            res[masked].append(ms)
    assert torch.isfinite(out).all()
    for masked in (False, True):
        v = res[masked]
        print(f"C2 shape (B=1, S=4096, T=512, 50 steps, bf16) {'fmi_flux_denoise_inpaint' if masked else 'fmi_flux_denoise        '}: "
              f"ms/step {' '.join(f'{x:.3f}' for x in v)}  median {np.median(v):.3f}")
    print(f"masked - plain, medians: {np.median(res[True]) - np.median(res[False]):+.3f} ms/step ({(np.median(res[True]) / np.median(res[False]) - 1) * 100:+.2f} %)")

elif part == "glue":
    vae = d.AutoEncoderKl(d.VAE_FLUX)
    synth.fill_vae_random_device(vae, seed=1, device=dev, encoder=True)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    u8 = torch.randint(0, 256, (1, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    img = d.preprocess_u8(u8, interleaved=True)
    print(f"fmi_vae_encode 1 x 3 x 1024 x 1024 (posterior mean): {events(lambda: vae.encode(img), 5, warm=2):.2f} ms")
    z = vae.encode(img)
    pm = (torch.rand((1, H, W), generator=g, device=dev) < 0.5).float()
    x0, _ = d.encode_latents(z, vae.scale_factor(), vae.shift_factor())
    noise = torch.randn_like(x0)
    R = 200
    print("glue at 1024 x 1024, B = 1, mean of 200 back-to-back calls through the Python wrapper (device events; includes the output allocation and launch gaps):")
    print(f"  fmi_preprocess_u8 NHWC (3 MB in, 12.6 MB out): {events(lambda: d.preprocess_u8(u8, interleaved=True), R) * 1e3:.1f} us")
    print(f"  fmi_preprocess_u8 NCHW                       : {events(lambda: d.preprocess_u8(u8.permute(0, 3, 1, 2).contiguous()), R) * 1e3:.1f} us (with the permute copy)")
    print(f"  fmi_latent_mask (4.2 MB in, 1 MB out)        : {events(lambda: d.latent_mask(pm, 16), R) * 1e3:.1f} us")
    print(f"  fmi_encode_latents (1 MB in, 1 MB out)       : {events(lambda: d.encode_latents(z, 0.3611, 0.1159), R) * 1e3:.1f} us")
    print(f"  fmi_scale_noise (2 MB in, 1 MB out)          : {events(lambda: d.scale_noise(x0, noise, 0.6), R) * 1e3:.1f} us")
    print(f"  (an empty launch pair for scale: torch.empty_like) : {events(lambda: torch.empty_like(x0), R) * 1e3:.1f} us")

elif part == "trace":  # under rocprofv3 --kernel-trace --stats: kernel times by name; the small model at the C2 token count (the blend sees the same 4096 x 64 elements)
    from tests.util import SMALL_FLUX
    flux = d.FluxModel(SMALL_FLUX)
    flux.load_state_dict(synth.flux_state_dict_numpy(SMALL_FLUX, seed=0))
    txt, y, guid, txt_ids, noise, ids, x0, mask = loop_inputs(SMALL_FLUX, T=32)
    sched = d.SchedulerConfig()
    ts = sched.get_timesteps(10, sched.calculate_shift(S))
    flux.denoise(noise, ids, txt, txt_ids, y, guid, ts, x0=x0, noise=noise, mask=mask)
    flux.denoise(noise, ids, txt, txt_ids, y, guid, ts)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    u8 = torch.randint(0, 256, (1, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    pm = (torch.rand((1, H, W), generator=g, device=dev) < 0.5).float()
    z = torch.randn((1, 16, 128, 128), device=dev)
    for _ in range(10):
        d.preprocess_u8(u8, interleaved=True)
        d.latent_mask(pm, 16)
        d.encode_latents(z, 0.3611, 0.1159)
        d.scale_noise(x0, noise, 0.6)
    torch.cuda.synchronize()
    print("trace part done")
