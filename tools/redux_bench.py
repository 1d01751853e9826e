#!/usr/bin/env python
"""FLUX.1 Redux: how far the GPU lies from its CPU reference and what image variation costs.  Prints the body of profiles/redux.txt:

    python tools/redux_bench.py [runs] [steps]

  (a) the small towers of tests/redux_ref.py (B = 2 and B = 1): rel-L2 of last_hidden_state to the float32 reference; the embedder on the reference's hidden states;
  (b) the direct-to-square resize: the largest difference and the share of differing values against the CPU recipe and against PIL's committed outputs;
  (c) google/siglip-so400m-patch14-384's tower and the FLUX.1-dev embedder (1152 -> 12288 -> 4096) on random weights, B = 1, a 301 x 517 u8 picture already on the
      device: `runs` (default 20) calls after 3 warm-up calls, each timed by a host clock around a call that ends in a stream synchronise (the forwards synchronise
      themselves); the median and the spread of the whole encode, of resize + preprocess, of the tower and of the embedder.  The attention's share: the tower's
      27 attention calls are the op-level fmi_sdpa_bf16 at B = 1, H = 16, L = 729, d = 128 (V transpose + attention, the launches siglip_attention makes), timed by
      device events over 27 x `runs` calls on the same stream;
  (d) the denoise loop of the FLUX.1-dev shape (random weights) at 1024 x 1024, B = 1: `steps` (default 20) steps at T = 512 + 729 text rows beside T = 512, the
      plain step of the same build, ms per step, 3 timed loops each after a warm-up loop."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diffusion_rs_amd as d  # noqa: E402
from diffusion_rs_amd import _lib as L  # noqa: E402
from diffusion_rs_amd import synth  # noqa: E402
from diffusion_rs_amd.flux import _ptr, _stream  # noqa: E402
from tests import redux_ref as R  # noqa: E402
from tests.util import rel_l2  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
host = lambda t: t.detach().float().cpu().numpy()

print("(a) small towers, rel-L2 of last_hidden_state to tests/redux_ref.py in float32 (bar 1e-2):")
for name, cfg in R.CONFIGS.items():
    m = d.SiglipVisionModel(cfg)
    m.load_state_dict(R.state_dict(cfg))
    pix = R.pixel_values(cfg, 2)
    e2, e1 = rel_l2(host(m.forward(pix)), R.reference(name, 2)), rel_l2(host(m.forward(pix[:1])), R.reference(name, 2)[:1])
    print(f"      {name}  D {cfg['hidden_size']:4d}  hd {cfg['hidden_size'] // cfg['num_attention_heads']:3d}  F {cfg['intermediate_size']:4d}  Np {R.num_patches(cfg):2d}"
          f"   B = 2 {e2:.3e}   B = 1 {e1:.3e}")
    m.close()
for name in ("h72_t81", "h64_t16"):
    cfg = R.CONFIGS[name]
    e = d.ReduxImageEmbedder(cfg["hidden_size"], R.REDUX_J)
    e.load_state_dict(R.redux_state_dict(cfg["hidden_size"]))
    hid = np.array(R.reference(name, 1))
    errs = [rel_l2(host(e.forward(hid, s)), R.redux_forward(R.redux_state_dict(cfg["hidden_size"]), hid, s)) for s in (1.0, 0.5)]
    print(f"      embedder {cfg['hidden_size']} -> {3 * R.REDUX_J} -> {R.REDUX_J} on {name}'s hidden states: scale 1 {errs[0]:.3e}   scale 0.5 {errs[1]:.3e}")
    e.close()

print(f"(b) fmi_resize_bicubic_u8 straight to {R.RESIZE_S} x {R.RESIZE_S}: largest difference / share of differing values")
m = d.SiglipVisionModel(dict(R.CONFIGS["h64_t16"], num_hidden_layers=1))
z = np.load(R.GOLDEN)
for name, (shape, kind, seed) in R.RESIZE_CASES.items():
    src = R.picture(shape, kind, seed=seed)
    got = m.resize(src, R.RESIZE_S, R.RESIZE_S).cpu().numpy().astype(int)
    a, b = np.abs(got - R.resize_bicubic_u8(src, R.RESIZE_S, R.RESIZE_S).astype(int)), np.abs(got - z[f"resize_out/{name}"].astype(int))
    print(f"      {name:7s} {shape[0]:3d} x {shape[1]:3d}   recipe {int(a.max())} / {float((a > 0).mean()):.2e}   PIL {int(b.max())} / {float((b > 0).mean()):.2e}")
m.close()


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


print(f"(c) SigLIP so400m-patch14-384 tower (27 x 1152, 729 tokens, head dim 72, F 4304) + Redux embedder (1152 -> 12288 -> 4096), random weights, B = 1, a 301 x 517 "
      f"picture on the device, {RUNS} runs after 3 warm-up calls:")
m = d.SiglipVisionModel()
synth.fill_text_random_device(m, seed=4)
e = d.ReduxImageEmbedder(1152, 4096)
synth.fill_text_random_device(e, seed=5)
pic = torch.from_numpy(R.picture((301, 517), seed=9)).cuda()
pv = m.preprocess(pic)
hid = m.forward(pv)
rows = []
for what, fn in (("encode (resize + preprocess + tower + embedder)", lambda: e.forward(m.encode(pic))), ("resize + preprocess", lambda: m.preprocess(pic)),
                 ("tower", lambda: m.forward(pv)), ("embedder", lambda: e.forward(hid))):
    med, lo, hi = timed(fn)
    rows.append(med)
    print(f"      {what:48s} median {med:7.3f} ms   min {lo:7.3f}   max {hi:7.3f}")
lib = L.load()
q, k, v = (torch.randn((1, 16, 729, 128), device="cuda").to(torch.bfloat16) for _ in range(3))
o = torch.empty((1, 729, 16 * 128), dtype=torch.bfloat16, device="cuda")
scale = 72 ** -0.5
sdpa = lambda: L.check(lib.fmi_sdpa_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(o), 1, 16, 729, 729, 128, scale, 1, _stream()), lib)
for _ in range(27):
    sdpa()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
a.record()
for _ in range(27 * RUNS):
    sdpa()
b.record()
torch.cuda.synchronize()
att = a.elapsed_time(b) / RUNS
print(f"      attention (27 x V transpose + MFMA attention at H = 16, L = 729, d = 128; device events)   {att:7.3f} ms = {100 * att / rows[2]:.1f} % of the tower, "
      f"{100 * att / rows[0]:.1f} % of the encode")
print(f"      resident: tower {m.size_in_bytes()} bytes ({m.size_in_bytes() / 2**20:.1f} MiB), embedder {e.size_in_bytes()} bytes ({e.size_in_bytes() / 2**20:.1f} MiB): bf16 "
      f"weights (heads padded to 128, F to 4352) + the B = 1 workspaces")
m.close()
e.close()

print(f"(d) FLUX.1-dev shape, random weights, 1024 x 1024, B = 1, {STEPS} steps per loop, one warm-up loop then 3 timed loops, ms per step:")
dev = torch.device("cuda", 0)
cfg = d.FLUX_DEV
model = d.FluxModel(cfg)
synth.fill_flux_random_device(model, seed=0, device=dev)
g = torch.Generator(device=dev)
g.manual_seed(1234)
y = torch.randn((1, cfg["pooled_projection_dim"]), generator=g, device=dev)
guid = torch.full((1,), 3.5, device=dev)
noise, ids = d.pack_latents(d.randn_latents(1, 16, 128, 128, seed=1, device=dev))
sched = d.SchedulerConfig()
ts = sched.get_timesteps(STEPS, sched.calculate_shift(4096))
for T in (512, 512 + 729):
    txt = torch.randn((1, T, cfg["joint_attention_dim"]), generator=g, device=dev).to(torch.bfloat16)
    txt_ids = torch.zeros((1, T, 3), device=dev)
    loop = lambda: model.denoise(noise, ids, txt, txt_ids, y, guid, ts)
    loop()
    v = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3 / STEPS)
    print(f"      T = {T:4d} text rows ({'plain' if T == 512 else 'prompt + 729 Redux tokens'}):   {' '.join(f'{x:.3f}' for x in v)}")
