"""Time of an all-192-row launch against an all-256-row and an automatically cut launch of the same problem (equal FLOPs) through fmi_gemm_group,
alternating the three settings of fmi_set_gemm_rows, CUDA events: profiles/tile_rows_ratio.txt.  Needs an MI355X; run from the repository root."""
import ctypes as C
import sys

import torch

sys.path.insert(0, ".")
from diffusion_rs_amd import _lib as L  # noqa: E402

lib = L.load()
L.check(lib.fmi_init(0))


def run(M, N, K, epi, reps=12):
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, device="cuda").to(torch.bfloat16)
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    d = L.GemmDesc(a=C.c_void_p(x.data_ptr()), w=C.c_void_p(w.data_ptr()), bias=C.c_void_p(b.data_ptr()), out=C.c_void_p(out.data_ptr()), M=M, N=N, K=K,
                   lda=K, ldw=K, ldo=N, epi=epi, alpha=1.0)
    arr = (L.GemmDesc * 1)(d)
    times = {256: [], 192: [], 0: []}
    ref = None
    for it in range(reps + 2):
        for mode in (256, 192, 0):
            L.check(lib.fmi_set_gemm_rows(mode), lib)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.check(lib.fmi_gemm_group(arr, 1, None), lib)
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:
                times[mode].append(e0.elapsed_time(e1) * 1e3)
            if it == 0:
                bits = out.view(torch.int16).clone()
                if ref is None:
                    ref = bits
                assert torch.equal(bits, ref), mode
    lib.fmi_set_gemm_rows(0)
    m = {k: sum(v) / len(v) for k, v in times.items()}
    mn = {k: min(v) for k, v in times.items()}
    print(f"{M} x {N} x {K} epi {epi}: all-256 mean {m[256]:.1f} us (min {mn[256]:.1f}), all-192 mean {m[192]:.1f} us (min {mn[192]:.1f}), automatic mean {m[0]:.1f} us "
          f"(min {mn[0]:.1f}); all-192 / all-256 = {m[192] / m[256]:.3f} (min / min {mn[192] / mn[256]:.3f}); automatic / all-256 = {m[0] / m[256]:.3f}", flush=True)


run(4608, 32768, 3072, 0)   # 2304 tall tiles = 9 whole rounds of 256 CUs, 3072 short tiles = 12 whole rounds: per-tile ratio = launch ratio * 9 / 12
run(4608, 12288, 3072, 1)   # MLP-in: 864 tall (3.375 rounds) / 1152 short (4.5 rounds)
run(4608, 21504, 3072, 3)   # linear1's shape
