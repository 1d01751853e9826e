#!/usr/bin/env python3
"""GGUF measurements -> profiles/gguf.txt.

  table 1  stand-alone fmi_gguf_dequantize of a 21504 x 3072 matrix (a single block's linear1) per block format, bf16 out, next to
           dequantize_blockwise_bf16_nf4 on the same shape in the same process: microseconds and achieved (bytes in + bytes out) / time
  table 2  FLUX.1-dev shape, 1024 x 1024, B = 1, synthetic Q8_0 and Q4_K transformers: ms per denoise step with the dense cache in mode 3 (expanded
           once) and mode 0 (per call), against the bf16 model in the same run, and the resident bytes of each

Every number is an event-timed median after a warm-up.  Each part runs in a child process of its own under its own time limit; a part that does not
end with status 0 stops the run (nothing more is started on the device).  Usage: python tools/gguf_bench.py [--out profiles/gguf.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K = 21504, 3072
GGML = {"Q4_0": 2, "Q4_1": 3, "Q5_0": 6, "Q5_1": 7, "Q8_0": 8, "Q4_K": 12, "Q5_K": 13, "Q6_K": 14}


def event_median_us(torch, fn, warm=5, reps=15, inner=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(ts), min(ts), max(ts)


def part_dequant():
    import torch
    from diffusion_rs_amd import _lib as L, synth
    lib = L.load()
    dev = torch.device("cuda", 0)
    n = N * K
    out = torch.empty(n, dtype=torch.bfloat16, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    w = torch.randn((N, K), device=dev, dtype=torch.bfloat16) * 0.02
    packed, absmax = synth.quantize_nf4_device(w, 64)
    fn = lambda: lib.dequantize_blockwise_bf16_nf4(None, C.c_void_p(packed.data_ptr()), C.c_void_p(absmax.data_ptr()), C.c_void_p(out.data_ptr()), 64, n, stream)  # noqa: E731
    rows.append(("nf4 (bnb, blocksize 64)", packed.numel() + absmax.numel() * 4, event_median_us(torch, fn)))
    del w, packed, absmax
    for name, t in GGML.items():
        be, bb = C.c_int(), C.c_int()
        L.check(lib.fmi_gguf_block_info(t, C.byref(be), C.byref(bb)))
        nbytes = n // be.value * bb.value
        raw = torch.randint(0, 256, (n // be.value, bb.value), dtype=torch.uint8, device=dev)
        for off in {2: (0,), 3: (0, 2), 6: (0,), 7: (0, 2), 8: (0,), 12: (0, 2), 13: (0, 2), 14: (208,)}[t]:
            raw[:, off + 1] &= 0x3F  # finite f16 scales of small magnitude
        fn = lambda: L.check(lib.fmi_gguf_dequantize(t, C.c_void_p(raw.data_ptr()), n, C.c_void_p(out.data_ptr()), L.BF16, stream))  # noqa: E731
        rows.append((name, nbytes, event_median_us(torch, fn)))
        del raw
    print(f"# stand-alone dequantisation, {N} x {K} -> bf16 ({n * 2 / 1e6:.1f} MB out); median of 15 event-timed windows of 20 launches (min .. max)")
    print("# (bytes in + bytes out are 169 .. 202 MB and every launch reads and writes the same buffers: part of that stays in the 256 MiB last-level cache, so these are")
    print("#  rates of the kernels next to each other under equal conditions, not HBM rates; the nf4 kernel is the yardstick)")
    print(f"{'format':<26}{'bytes in':>12}{'us':>10}{'min':>9}{'max':>9}{'GB/s (in + out)':>18}{'vs nf4':>9}")
    base = None
    for name, nb, (med, lo, hi) in rows:
        bw = (nb + n * 2) / med / 1e3
        base = base or bw
        print(f"{name:<26}{nb:>12}{med:>10.1f}{lo:>9.1f}{hi:>9.1f}{bw:>18.0f}{bw / base:>9.2f}")


def part_model(quant, feed=None):
    """feed(model, name, w) -> bool: another way to load a weight (tools/single_file_bench.py); True = it took the tensor"""
    import torch
    import diffusion_rs_amd as d
    from diffusion_rs_amd import synth
    dev = torch.device("cuda", 0)
    model = d.FluxModel(d.FLUX_DEV, 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    t = GGML.get(quant)
    for name, shape in synth.flux_tensor_shapes(d.FLUX_DEV).items():
        if "norm_q" in name or "norm_k" in name or "norm_added" in name:
            w = torch.ones(shape, dtype=torch.bfloat16, device=dev)
        elif name.endswith(".bias"):
            w = torch.zeros(shape, dtype=torch.bfloat16, device=dev)
        else:
            w = torch.randn(shape, generator=g, device=dev, dtype=torch.bfloat16)
            w.mul_(synth._std_for(name, 0.02, 0.01))
        if feed is not None and feed(model, name, w):
            pass
        elif t is not None and len(shape) == 2 and shape[1] % 256 == 0:  # what a GGUF file quantises: every 2-D weight whose rows are whole blocks
            model.set_linear_gguf(name[:-len(".weight")], t, synth.quantize_gguf_device(w, t), shape[0], shape[1])
        else:
            model.set_tensor(name, w)
        del w
    model.assert_complete()
    H = W = 1024
    h, w_ = H // 16 * 2, W // 16 * 2
    S, T, NS = (h // 2) * (w_ // 2), 512, 4
    sched = d.SchedulerConfig()
    ts = sched.get_timesteps(NS, sched.calculate_shift(S))
    gi = torch.Generator(device=dev)
    gi.manual_seed(1234)
    txt = torch.randn((1, T, 4096), generator=gi, device=dev, dtype=torch.float32).to(torch.bfloat16)
    y = torch.randn((1, 768), generator=gi, device=dev, dtype=torch.float32)
    guidance = torch.full((1,), 3.5, dtype=torch.float32, device=dev)
    txt_ids = torch.zeros((1, T, 3), dtype=torch.float32, device=dev)
    img, img_ids = d.pack_latents(d.randn_latents(1, 16, h, w_, seed=1234, device=dev))
    loaded = model.size_in_bytes()
    for mode in ((0, 3) if t is not None or feed is not None else (-1,)):  # (0 first: its resident bytes are then the packed-only figure)
        model.set_quant_dense_cache(mode)
        run = lambda: model.denoise(img.clone(), img_ids, txt, txt_ids, y, guidance, ts)  # noqa: E731
        med, lo, hi = event_median_us(torch, run, warm=2, reps=7, inner=1)
        torch.cuda.synchronize()
        print(f"{quant:<8}{mode:>6}{med / NS / 1e3:>14.2f}{lo / NS / 1e3:>10.2f}{hi / NS / 1e3:>10.2f}{loaded / 2**30:>16.2f}{model.size_in_bytes() / 2**30:>16.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["dequant", "model"])
    ap.add_argument("--quant", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gguf.txt"))
    args = ap.parse_args()
    if args.part == "dequant":
        return part_dequant()
    if args.part == "model":
        return part_model(args.quant)
    parts = [(["--part", "dequant"], 240)] + [(["--part", "model", "--quant", q], 300) for q in ("bf16", "Q8_0", "Q4_K")]
    text = ["# tools/gguf_bench.py — GGUF transformers on one MI355X (DESIGN.md 4.16); every figure measured in this run", ""]
    for i, (argv, limit) in enumerate(parts):
        if i == 1:
            text += ["", "# FLUX.1-dev shape, 1024 x 1024, B = 1, T = 512, 4-step denoise; ms per step = median of 7 event-timed loops / 4 (min, max); GiB = fmi_flux_size_in_bytes",
                     "# mode 3: block matrices expanded once (the bf16 kernels on bf16 operands); mode 0: expanded per call into the scratch; bf16: the dense model, same process layout",
                     f"{'model':<8}{'mode':>6}{'ms / step':>14}{'min':>10}{'max':>10}{'GiB loaded':>16}{'GiB after run':>16}"]
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
        text += [ln for ln in r.stdout.splitlines() if ln.strip()]
        print("\n".join(r.stdout.splitlines()), flush=True)
        if r.returncode != 0:
            print(r.stderr[-2000:], file=sys.stderr)
            raise SystemExit(f"part {argv} ended with status {r.returncode}: nothing more is started")
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
