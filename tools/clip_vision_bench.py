#!/usr/bin/env python
"""CLIP vision encoder: how far the GPU lies from its CPU reference and what one image prompt costs.  Prints the body of profiles/clip_vision.txt:

    python tools/clip_vision_bench.py [runs]

  (a) the small towers of tests/clip_vision_ref.py (B = 3): rel-L2 of image_embeds and of the hidden output to the float32 reference;
  (b) the resize: the largest difference and the share of differing values against the CPU recipe and, on the committed pictures, against PIL;
  (c) openai/clip-vit-large-patch14's tower on random weights, B = 1, a 301 x 517 u8 picture already on the device: `runs` (default 30) encodes after 3 warm-up
      calls, each timed by a host clock around a call that ends in a stream synchronise (fmi_clip_vision_forward synchronises itself); the median, the spread, and
      the same for the resize + preprocess and the tower alone; the encoder's resident bytes."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diffusion_rs_amd as d  # noqa: E402
from tests import clip_vision_ref as R  # noqa: E402
from tests.util import rel_l2  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
host = lambda t: t.detach().float().cpu().numpy()

print("(a) small towers (D = 128, 2 heads, F = 256, 3 layers, projection 64), B = 3, rel-L2 to tests/clip_vision_ref.py in float32:")
for name, cfg in R.CONFIGS.items():
    m = d.ClipVisionModel(cfg)
    m.load_state_dict(R.state_dict(cfg))
    e, h = m.forward(R.pixel_values(cfg, 3), return_hidden=True)
    we, wh = R.reference(name, 3)
    T = 1 + (cfg["image_size"] // cfg["patch_size"]) ** 2
    print(f"      image {cfg['image_size']:3d} / patch {cfg['patch_size']}  T = {T:2d}   image_embeds {rel_l2(host(e), we):.3e}   hidden {rel_l2(host(h), wh):.3e}")
    m.close()


def distance(got, want):
    diff = np.abs(got.astype(int) - want.astype(int))
    return int(diff.max()), float((diff > 0).mean())


print("(b) fmi_resize_bicubic_u8: largest difference / share of differing values")
m = d.ClipVisionModel(dict(R.CONFIGS["s56p14"], num_hidden_layers=1))
z = np.load(R.GOLDEN)
cases = list(R.RESIZE_CASES.items()) + [("real", ((301, 517), (224, 384), "noise"))]
for i, (name, ((h, w), (nh, nw), kind)) in enumerate(cases):
    src = R.picture((h, w), kind, seed=100 + i)
    got = m.resize(src, nh, nw).cpu().numpy()
    a = distance(got, R.resize_bicubic_u8(src, nh, nw))
    b = distance(got, z[f"resize_out/{name}"]) if name != "real" else None
    print(f"      {name:9s} {h:3d} x {w:3d} -> {nh:3d} x {nw:3d}   recipe {a[0]} / {a[1]:.2e}   PIL " + (f"{b[0]} / {b[1]:.2e}" if b else "(no fixture)"))
m.close()

print(f"(c) CLIP ViT-L/14 vision tower (24 x 1024, 257 tokens, projection 768), random weights, B = 1, a 301 x 517 picture on the device, {RUNS} runs after 3 warm-up calls:")
m = d.ClipVisionModel()
d.synth.fill_text_random_device(m, seed=4)
pic = torch.from_numpy(R.picture((301, 517), seed=9)).cuda()


def timed(fn):
    for _ in range(3):
        fn()
    v = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(v)), min(v), max(v)


pv = m.preprocess(pic)
for what, fn in (("encode (resize + preprocess + tower)", lambda: m.encode(pic)), ("resize + preprocess", lambda: m.preprocess(pic)), ("tower", lambda: m.forward(pv))):
    med, lo, hi = timed(fn)
    print(f"      {what:38s} median {med:7.3f} ms   min {lo:7.3f}   max {hi:7.3f}")
print(f"      resident: {m.size_in_bytes()} bytes ({m.size_in_bytes() / 2**20:.1f} MiB: bf16 weights + the B = 1 workspace)")
