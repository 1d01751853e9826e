#!/usr/bin/env python
"""LoHa / LoKr / DoRA merge on a full-size synthetic FLUX.1-dev: how long does a re-merge of every block Linear (418 of them, 17.2 GB of bf16 weights)
take with one adapter of each kind at rank 16, next to plain LoRA at rank 16 and a device-to-device copy of the same matrices, all in one run on one
box (the method of tools/lora_bench.py).  Prints the table of profiles/lycoris_merge.txt.

    python tools/lycoris_bench.py [--repeat 3] [--kinds lora loha lokr dora]

load        = one fmi_flux_lora_add_term per Linear (factor upload, the kind's pre-pass — DoRA's row norms, LoKr's expanded w2 — pristine copy, merge)
reweight    = fmi_flux_lora_set_weight: every adapted Linear merged again from its pristine copy — the merge pass alone (plain LoRA: lora_pack_kernel +
              lora_merge_kernel per Linear; the other kinds: one adapter_merge_kernel per Linear)
unload      = fmi_flux_lora_remove: the pristine copies go back
copy        = one hipMemcpyAsync per matrix (same sizes, out of the block arena into a scratch buffer), one synchronisation at the end
LoKr: factor 16 — w1 (16, 16) full, w2 = w2_a (out / 16, 16) w2_b (16, in / 16) decomposed at rank 16.
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import diffusion_rs_amd as d  # noqa: E402

RANK = 16


def make_term(kind, o, i, g):
    def rn(*shape, s=0.02):
        return torch.randn(shape, generator=g, device="cuda") * s

    if kind == "lora":
        return d.AdapterTerm("lora", (rn(RANK, i), rn(o, RANK)), 1.0)
    if kind == "loha":
        return d.AdapterTerm("loha", (rn(o, RANK, s=0.1), rn(RANK, i, s=0.1), rn(o, RANK, s=0.1), rn(RANK, i, s=0.1)), 1.0)
    if kind == "lokr":
        return d.AdapterTerm("lokr", (rn(16, 16, s=0.2), None, rn(o // 16, RANK, s=0.1), rn(RANK, i // 16, s=0.1)), 1.0)
    if kind == "dora":
        return d.AdapterTerm("dora", (rn(RANK, i), rn(o, RANK), 1.0 + 0.1 * torch.rand((o,), generator=g, device="cuda")), 1.0)
    raise ValueError(kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--kinds", nargs="+", default=["lora", "loha", "lokr", "dora"])
    args = ap.parse_args()
    pipe = d.Pipeline(d.ModelSource.Synthetic())
    flux, lib = pipe.flux, pipe.flux.lib
    shapes = {n[:-len(".weight")]: s for n, s in flux._shapes().items() if "transformer_blocks." in n and n.endswith(".weight") and len(s) == 2 and "norm" not in n}
    total = sum(o * i for o, i in shapes.values())
    print(f"{len(shapes)} block Linears, {total * 2 / 1e9:.2f} GB of bf16 weights; {lib.fmi_device_info().decode()}; build {lib.fmi_build_id().decode()}")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

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
    print(f"copy           {t_copy:9.2f} ms   ({2 * total * 2 / t_copy / 1e9:.2f} TB/s read + written)")

    for kind in args.kinds:
        g = torch.Generator(device="cuda")
        g.manual_seed(16)
        terms = {p: make_term(kind, o, i, g) for p, (o, i) in shapes.items()}

        def load():
            for p, t in terms.items():
                flux.lora_add_term("bench", p, t)

        t_load, t_rew, t_unload = [], [], []
        for _ in range(args.repeat):
            t_load.append(wall(load))
            t_rew.append(wall(lambda: flux.lora_set_weight("bench", 0.75)))
            t_unload.append(wall(lambda: flux.lora_remove("bench")))
        for name, ts in (("load", t_load), ("reweight", t_rew), ("unload", t_unload)):
            t = min(ts)
            print(f"{kind:4s} r{RANK} {name:9s} {t:9.2f} ms   {t / t_copy:6.2f} x copy   (runs: {', '.join(f'{x:.1f}' for x in ts)})", flush=True)
        del terms


if __name__ == "__main__":
    main()
