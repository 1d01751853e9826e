"""Block-sparse joint attention next to the group-mask kernel with everything visible and the unmasked stream: profiles/attention_blocks.txt.
Needs an MI355X.  Op level, B = 1, H = 24: device events around one call (each entry builds its V^T image per call), the entries alternated inside every
round; a figure is the median over a round's calls, reported as the median (min .. max) over the rounds — the spread is that of the round medians."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffusion_rs_amd as d  # noqa: E402
from diffusion_rs_amd import _lib as L  # noqa: E402

H, SCALE = 24, 128 ** -0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/attention_blocks.txt")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    lib, lines = L.load(), []
    for T, h, w, radii in ((512, 64, 64, ()), (512, 128, 128, (8, 16, 32))):
        n = T + h * w
        nqb, nt = -(-n // 128), -(-n // 64)
        g = torch.Generator().manual_seed(n)
        q, k, v = (torch.randn((1, H, n, 128), generator=g).to(torch.bfloat16).cuda() for _ in range(3))
        o, ones = torch.empty_like(q), torch.ones(n, dtype=torch.int32, device="cuda")
        ptr = lambda t: t.data_ptr()
        entries = {"fmi_sdpa_bf16": lambda: lib.fmi_sdpa_bf16(ptr(q), ptr(k), ptr(v), ptr(o), 1, H, n, n, 128, SCALE, 0, None),
                   "fmi_sdpa_groups_bf16 all visible": lambda: lib.fmi_sdpa_groups_bf16(ptr(q), ptr(k), ptr(v), ptr(o), 1, H, n, n, 128, SCALE, 0, ptr(ones), ptr(ones), 1, None)}
        share = {}
        for name, r in [("all tiles listed", max(h, w))] + [(f"radius {r}", r) for r in radii]:
            rp, cl = d.flux.local_attention_tiles(T, h, w, r)
            dl = [torch.from_numpy(a).cuda() for a in (rp, cl, d.flux.attention_blocks_order(rp))]
            name = f"fmi_sdpa_blocks_bf16 {name}"
            share[name] = cl.size / (nqb * nt)
            entries[name] = lambda dl=dl, nc=int(cl.size): lib.fmi_sdpa_blocks_bf16(ptr(q), ptr(k), ptr(v), ptr(o), 1, H, n, n, 128, SCALE, 0, ptr(dl[0]), ptr(dl[1]), ptr(dl[2]), nqb, nc, None)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        med = {name: [] for name in entries}
        for rnd in range(args.rounds + 1):  # round 0 warms every entry up and is dropped
            us = {name: [] for name in entries}
            for _ in range(args.calls):
                for name, call in entries.items():
                    ev[0].record()
                    L.check(call())
                    ev[1].record()
                    ev[1].synchronize()
                    us[name].append(ev[0].elapsed_time(ev[1]) * 1e3)
            if rnd:
                for name in entries:
                    med[name].append(statistics.median(us[name]))
        lines.append(f"L = {n} ({T} text rows + {h} x {w} image tokens), {nqb} query blocks x {nt} key tiles, {args.rounds} rounds of {args.calls} calls")
        for name, m in med.items():
            tiles = share.get(name, 1.0) * nqb * nt * H
            lines.append(f"  {name}: {statistics.median(m):.0f} us ({min(m):.0f} .. {max(m):.0f})" +
                         (f"; {100 * share[name]:.1f} % of the tiles listed, {1e3 * statistics.median(m) / tiles:.1f} ns per listed tile and head" if name in share else ""))
        grp, blk = med["fmi_sdpa_groups_bf16 all visible"], med["fmi_sdpa_blocks_bf16 all tiles listed"]
        lines.append(f"  all tiles listed against groups all visible: {statistics.median(blk):.0f} vs {statistics.median(grp):.0f} us, the groups call's spread {max(grp) - min(grp):.0f} us")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
