#!/usr/bin/env python
"""LoRA merge on a full-size synthetic FLUX.1-dev: how long do Pipeline.load_lora / set_lora_weight / unload_lora take for an adapter on every
block Linear (418 of them, 17.2 GB of bf16 weights), next to a device-to-device hipMemcpyAsync of the same matrices — the yardstick: it moves the
bytes a merge must read and write and is no code of this library.  Prints the table of profiles/lora_merge.txt.

    python tools/lora_bench.py [--ranks 16 64] [--repeat 3]

load        = read_lora on a {key: device tensor} dict + one fmi_flux_lora_add per Linear (factor upload, pristine copy, merge)
reweight    = fmi_flux_lora_set_weight: every adapted Linear merged again from its pristine copy — the merge pass alone (per Linear: one
              launch that packs the factors, one merge kernel)
unload      = fmi_flux_lora_remove: the pristine copies go back
copy        = one hipMemcpyAsync per matrix (same sizes, out of the block arena into a scratch buffer), one synchronisation at the end
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import diffusion_rs_amd as d  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    pipe = d.Pipeline(d.ModelSource.Synthetic())
    flux, lib = pipe.flux, pipe.flux.lib
    shapes = {n[:-len(".weight")]: s for n, s in flux._shapes().items() if "transformer_blocks." in n and n.endswith(".weight") and len(s) == 2 and "norm" not in n}
    total = sum(o * i for o, i in shapes.values())
    print(f"{len(shapes)} block Linears, {total * 2 / 1e9:.2f} GB of bf16 weights; {lib.fmi_device_info().decode()}")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # the yardstick
    arena, arena_bytes = flux.state_buffers()[2]  # the block arena
    scratch = torch.empty(max(o * i for o, i in shapes.values()) * 2, dtype=torch.uint8, device="cuda")

    def copy_all():
        off = 0
        for o, i in shapes.values():
            n = o * i * 2
            d._lib.check(lib.fmi_memcpy(C.c_void_p(scratch.data_ptr()), C.c_void_p(arena + off), n, None))
            off += (n + 255) // 256 * 256
        assert off <= arena_bytes

    copy_all()
    t_copy = min(wall(copy_all) for _ in range(args.repeat))
    print(f"copy      {t_copy:9.2f} ms   ({2 * total * 2 / t_copy / 1e9:.2f} TB/s read + written)")

    for r in args.ranks:
        g = torch.Generator(device="cuda")
        g.manual_seed(r)
        adapter = {}
        for p, (o, i) in shapes.items():
            adapter[p + ".lora_A.weight"] = torch.randn((r, i), generator=g, device="cuda") * 0.02
            adapter[p + ".lora_B.weight"] = torch.randn((o, r), generator=g, device="cuda") * 0.02
        t_load, t_rew, t_unload = [], [], []
        for _ in range(args.repeat):
            t_load.append(wall(lambda: pipe.load_lora(adapter, name="bench")))
            t_rew.append(wall(lambda: pipe.set_lora_weight("bench", 0.75)))
            t_unload.append(wall(lambda: pipe.unload_lora("bench")))
        for name, ts in (("load", t_load), ("reweight", t_rew), ("unload", t_unload)):
            t = min(ts)
            print(f"rank {r:3d} {name:9s} {t:9.2f} ms   {t / t_copy:6.2f} x copy   (runs: {', '.join(f'{x:.1f}' for x in ts)})", flush=True)


if __name__ == "__main__":
    main()
