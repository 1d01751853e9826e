#!/usr/bin/env python3
"""Single-file fp8 checkpoint measurements -> profiles/single_file.txt.

  table 1  stand-alone fmi_f8_dequantize of a 21504 x 3072 matrix (a single block's linear1), e4m3 and e5m2, bf16 out, next to fmi_gguf_dequantize Q8_0
           and dequantize_blockwise_bf16_nf4 on the same shape in the same process: microseconds and achieved (bytes in + bytes out) / time
  table 2  FLUX.1-dev shape, 1024 x 1024, B = 1, generated e4m3 codes for every 2-D weight: ms per denoise step with the dense cache in mode 3 (expanded
           once) and mode 0 (per call), against the bf16 model and a generated GGUF Q8_0 model of the same build, and the resident bytes of each

The timing and the model set-up are tools/gguf_bench.py's.  Each part runs in a child process of its own under its own time limit; a part that does not end
with status 0 stops the run (nothing more is started on the device).  Usage: python tools/single_file_bench.py [--out profiles/single_file.txt]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gguf_bench as GB  # noqa: E402

N, K = GB.N, GB.K


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
    rows.append(("nf4 (bnb, blocksize 64)", packed.numel() + absmax.numel() * 4, GB.event_median_us(torch, fn)))
    q8 = synth.quantize_gguf_device(w, 8)
    fn = lambda: L.check(lib.fmi_gguf_dequantize(8, C.c_void_p(q8.data_ptr()), n, C.c_void_p(out.data_ptr()), L.BF16, stream))  # noqa: E731
    rows.append(("GGUF Q8_0", q8.numel(), GB.event_median_us(torch, fn)))
    del packed, absmax, q8
    for name, fmt, dt in (("fp8 e4m3", 1, torch.float8_e4m3fn), ("fp8 e5m2", 2, torch.float8_e5m2)):
        codes = w.to(dt).view(torch.uint8).contiguous()
        fn = lambda: L.check(lib.fmi_f8_dequantize(fmt, C.c_void_p(codes.data_ptr()), n, 0.0123, C.c_void_p(out.data_ptr()), L.BF16, stream))  # noqa: E731
        rows.append((name, codes.numel(), GB.event_median_us(torch, fn)))
        del codes
    print(f"# stand-alone dequantisation, {N} x {K} -> bf16 ({n * 2 / 1e6:.1f} MB out); median of 15 event-timed windows of 20 launches (min .. max)")
    print("# (bytes in + bytes out are 169 .. 202 MB and every launch reads and writes the same buffers: part of that stays in the 256 MiB last-level cache, so these are")
    print("#  rates of the kernels next to each other under equal conditions, not HBM rates; the nf4 kernel is the yardstick)")
    print(f"{'format':<26}{'bytes in':>12}{'us':>10}{'min':>9}{'max':>9}{'GB/s (in + out)':>18}{'vs nf4':>9}")
    base = None
    for name, nb, (med, lo, hi) in rows:
        bw = (nb + n * 2) / med / 1e3
        base = base or bw
        print(f"{name:<26}{nb:>12}{med:>10.1f}{lo:>9.1f}{hi:>9.1f}{bw:>18.0f}{bw / base:>9.2f}")


def part_model(quant):
    """gguf_bench.part_model with one more kind of weights: "e4m3" = every 2-D weight whose rows are a multiple of 256 wide (what its Q8_0 model quantises) as
    generated e4m3 codes: a plain cast, scale 1"""
    if quant != "e4m3":
        return GB.part_model(quant)
    import torch

    def feed(model, name, w):
        if w.dim() != 2 or w.shape[1] % 256:
            return False
        model.set_linear_f8(name[:-len(".weight")], "e4m3", w.to(torch.float8_e4m3fn), 1.0, w.shape[0], w.shape[1])
        return True

    return GB.part_model("e4m3", feed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["dequant", "model"])
    ap.add_argument("--quant", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "single_file.txt"))
    args = ap.parse_args()
    if args.part == "dequant":
        return part_dequant()
    if args.part == "model":
        return part_model(args.quant)
    parts = [(["--part", "dequant"], 240)] + [(["--part", "model", "--quant", q], 300) for q in ("bf16", "e4m3", "Q8_0")]
    text = ["# tools/single_file_bench.py — single-file fp8 checkpoints on one MI355X (DESIGN.md 4.20); every figure measured in this run", ""]
    for i, (argv, limit) in enumerate(parts):
        if i == 1:
            text += ["", "# FLUX.1-dev shape, 1024 x 1024, B = 1, T = 512, 4-step denoise; ms per step = median of 7 event-timed loops / 4 (min, max); GiB = fmi_flux_size_in_bytes",
                     "# mode 3: block matrices expanded once (the bf16 kernels on bf16 operands); mode 0: expanded per call into the scratch; bf16: the dense model, same process layout",
                     "# e4m3: every 2-D weight whose rows are a multiple of 256 wide as generated e4m3 codes, scale 1; Q8_0: the GGUF model of tools/gguf_bench.py, same build",
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
