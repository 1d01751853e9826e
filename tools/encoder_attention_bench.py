"""Encode times of T5-XXL (T = 512), CLIP-L text (T = 77) and the CLIP-L vision tower (T = 257) under fmi_set_encoder_attention 0 and 1, and the d = 64 attention
op alone at T5's shape (needs an MI355X; DESIGN.md 4.22, profiles/encoder_attention.txt).  Random weights; both switch values in ONE process, alternating, after a
warm-up of each; an encode ends in the library's own stream synchronise, so the host clock around it is the encode's time.

    python tools/encoder_attention_bench.py [--out profiles/encoder_attention_timings.txt] [--rounds 5] [--calls 4]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import diffusion_rs_amd as d
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encoder_attention_bench needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def encoder(name, model, run):
        times, outs = {0: [], 1: []}, {}
        for kind in (0, 1):  # warm-up of both paths
            d.set_encoder_attention(("default", "mfma")[kind])
            outs[kind] = run().float()
        for _ in range(a.rounds):
            for kind in (0, 1):
                d.set_encoder_attention(("default", "mfma")[kind])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    run()
                torch.cuda.synchronize()
                times[kind].append((time.perf_counter() - t0) / a.calls * 1e3)
        d.set_encoder_attention("default")
        diff = float((outs[1] - outs[0]).norm() / outs[0].norm())
        med = {k: statistics.median(v) for k, v in times.items()}
        say(f"{name}: default {med[0]:8.3f} ms (min {min(times[0]):.3f}, max {max(times[0]):.3f})   mfma {med[1]:8.3f} ms (min {min(times[1]):.3f}, max {max(times[1]):.3f})"
            f"   mfma - default {med[1] - med[0]:+.3f} ms   outputs differ by rel-L2 {diff:.2e}")
        model.close()

    say(f"{a.rounds} rounds x {a.calls} encodes per switch value, alternating; median of the rounds' means")
    t5 = d.T5EncoderModel()
    d.synth.fill_text_random_device(t5, seed=0)
    ids = torch.randint(0, 32128, (1, 512), generator=torch.Generator().manual_seed(0)).int().cuda()
    encoder("T5-XXL encode, B = 1, T = 512 (24 layers, H = 64)  ", t5, lambda: t5.forward(ids))
    clip = d.ClipTextTransformer()
    d.synth.fill_text_random_device(clip, seed=1)
    cid = torch.randint(1, 49407, (1, 77), generator=torch.Generator().manual_seed(1)).int()
    cid[:, 40] = 49407
    cid = cid.cuda()
    encoder("CLIP-L text encode, B = 1, T = 77 (12 layers, H = 12)", clip, lambda: clip.forward(cid))
    vis = d.ClipVisionModel()
    d.synth.fill_text_random_device(vis, seed=2)
    pix = torch.randn((1, 3, 224, 224), generator=torch.Generator().manual_seed(2)).cuda()
    encoder("CLIP-L vision encode, B = 1, T = 257 (24 layers, H = 16)", vis, lambda: vis.forward(pix))

    # the op alone at T5's shape: q, k, v views of a fused projection, the (H, T, T) bias
    H, T = 64, 512
    qkv = (torch.randn((1, T, 3, H, 64), generator=torch.Generator().manual_seed(3)) * 0.5).to(torch.bfloat16).cuda()
    q, k, v = qkv.unbind(2)
    bias = torch.randn((H, T, T), generator=torch.Generator().manual_seed(4)).cuda()
    for _ in range(10):
        d.ops.sdpa_d64(q, k, v, bias=bias, scale=1.0)
    n = 200
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        d.ops.sdpa_d64(q, k, v, bias=bias, scale=1.0)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / n * 1e3
    flops, byts = 4.0 * H * T * T * 64, 4.0 * H * T * 64 * 2 + 4.0 * H * T * T
    say(f"sdpa_d64 alone, B = 1, H = 64, T = 512, f32 bias: {us:.1f} us a call over {n} back-to-back calls (device events; includes the launch gaps of a Python loop) = "
        f"{flops / us * 1e-6:.1f} TFLOP/s of {flops * 1e-9:.2f} GFLOP, {byts / us * 1e-3:.0f} GB/s of {byts * 1e-6:.1f} MB")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
