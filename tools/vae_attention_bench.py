"""Times and workspace sizes of the VAE mid-block attention under both kinds of fmi_vae_set_mid_attention, and the d = 512 flash kernel alone (needs an
MI355X; DESIGN.md 4.25, profiles/vae_attention.txt).  Random weights at the FLUX VAE config; warm, device events on the launch stream, median of 21 calls.

    python tools/vae_attention_bench.py [--out profiles/vae_attention_timings.txt] [--sides 64 128 256]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sides", type=int, nargs="*", default=[64, 128, 256], help="latent sides: L = side^2")
    ap.add_argument("--calls", type=int, default=21)
    args = ap.parse_args()
    import torch
    import diffusion_rs_amd as d
    if not torch.cuda.is_available():
        raise SystemExit("vae_attention_bench needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def median_ms(fn, calls=args.calls):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    say(d._lib.load().fmi_device_info().decode())
    gv = d.AutoEncoderKl(d.VAE_FLUX)
    d.synth.fill_vae_random_device(gv, seed=1, device=torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(0)
    for side in args.sides:
        L = side * side
        q, k, v = (torch.randn((1, L, 512), generator=g, device="cuda").to(torch.bfloat16) for _ in range(3))
        out = torch.empty_like(q)
        ms = median_ms(lambda: d.ops.sdpa_d512(q, k, v, out=out))
        say(f"L = {L}: sdpa_d512 alone {ms:.3f} ms = {4.0 * L * L * 512 / ms / 1e9:.0f} TFLOP/s")
        del q, k, v, out
        x = (1.5 * torch.randn((1, side, side, 512), generator=g, device="cuda")).to(torch.bfloat16)
        for kind in ("default", "flash"):
            gv.set_mid_attention(kind)
            base = used()
            try:
                ms = median_ms(lambda: gv.mid_attention(x), calls=args.calls if side <= 128 else 5)
                say(f"L = {L}: fmi_vae_mid_attention under {kind!r} {ms:.3f} ms, device memory in use grew by {(used() - base) / 2 ** 20:.0f} MiB")
            except d._lib.FmiError as e:
                say(f"L = {L}: fmi_vae_mid_attention under {kind!r} failed: {e}")
        del x
    for B in (1, 4):
        z = torch.randn((B, 16, 128, 128), generator=g, device="cuda")
        for kind in ("default", "flash"):
            gv.set_mid_attention(kind)
            ms = median_ms(lambda: gv.decode(z))
            say(f"decode 1024^2, B = {B}, under {kind!r}: {ms:.2f} ms")
    gv.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
