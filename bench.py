#!/usr/bin/env python
"""bench.py — images/sec + ms/denoise-step, FLUX.1-dev 1024x1024 50-step (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    ... bench.py --gpus N --sequence-parallel [--split-k]      (opt-in: ONE image on all N ranks, strong scaling)

A plain run does only what the headline figure needs: set-up, W warm-up steps, K timed steps, the outputs of the last timed step
(--dump-outputs DIR: DIR/image.npy, the u8 image(s) as float32, and DIR/latents.npy, the denoised f32 latents), one JSON line.
Everything else described below — the profiled pass (roofline, phases, VAE timing), the live PMC traffic passes, the energy
counters, the image CRC-32s, the secondary legs and the CPU baseline — runs only with --full (the --no-* flags then switch parts off).

A "step" is ONE IMAGE: the full hot path over one batch of synthetic input — 50 denoise
steps (Flux::forward + Euler update), unpack, VAE decode, u8 post-process — with inputs
(embeddings, latents) already resident in HBM.  Weights are random-init FLUX.1-dev / FLUX VAE
of the real architecture (no checkpoints offline), data is synthetic.  Batch sharding: every
rank generates its own image (weak scaling, no data-path collective); weights are generated on
rank 0 and broadcast over RCCL/xGMI, the decoded u8 images are gathered to rank 0 after the
timed region.

With N = 1 a --full run appends short legs under "secondary" (2 images each, own roofline): BASELINE config C3
(nf4 weights: only the packed codes resident), the headline workload in fp8 mode, the C5 shape (fp8 e4m3 block linears,
1280x720, batch 2), plus the per-rank compute of single-image sequence parallelism at 8 ranks (loopback exchange, 10 denoise
steps) — `--no-secondary` skips them.  `python bench.py --gpus N` with N > 1 and no launcher starts its N ranks itself.

One JSON line is printed by rank 0; with --full it holds two extra objects:
  roofline     — the dominant kernel (bf16 MFMA GEMM): algorithmic FLOPs / device time from
                 hipEvents on the launch stream, measured in a profiled pass of the same step
                 right after the timed region (the per-phase event pairs serialise phases, so
                 they are kept out of the timed region itself);
  cpu_baseline — the CPU oracle ("port" of the reference CPU semantics, f32) timed on this
                 host's cores: a bounded sample of C2 (one double + one single block at the full shape)
                 extrapolated to images/s by algorithmic FLOPs, and config C1 (schnell 256x256, 4 steps)
                 executed in full (`c1_full`).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

D_HID, N_HEADS, MLP = 3072, 24, 12288
N_DOUBLE, N_SINGLE = 19, 38


def step_flops(S, T, B=1, cfg=None):
    """Algorithmic FLOPs of one denoise step, split by kernel class."""
    D, M = D_HID, MLP
    L = S + T
    nd, ns = N_DOUBLE, N_SINGLE
    if cfg is not None:
        D = cfg["num_attention_heads"] * 128
        M = 4 * D
        nd, ns = cfg["num_layers"], cfg["num_single_layers"]
    gemm = 0
    # double blocks: per stream qkv (3D), proj (D), mlp1 (M), mlp2 (M) : tokens * 2 * D * (3D + D + M + M)
    gemm += nd * 2 * L * D * (3 * D + D + 2 * M)
    # single blocks: fused (3D+M) and proj_out (D+M -> D)
    gemm += ns * 2 * L * (D * (3 * D + M) + (D + M) * D)
    # img_in, txt_in, final proj
    gemm += 2 * S * 64 * D + 2 * T * 4096 * D + 2 * S * D * 64
    attn = (nd + ns) * 4 * L * L * D
    mod = 2 * (nd * 12 + ns * 3 + 2) * D * D + 2 * (3 * D * D + 2 * 256 * D + 768 * D)
    return dict(gemm=B * gemm, attn=B * attn, gemv=B * mod, total=B * (gemm + attn + mod))


def vae_flops(h8, w8):
    """Algorithmic conv+attention FLOPs of one VAE decode at latent (h8,w8) (public FLUX VAE config)."""
    boc = [128, 256, 512, 512]
    px = h8 * w8
    f = 2 * px * 9 * 16 * 512
    res = lambda cin, cout, p: 2 * p * 9 * (cin * cout + cout * cout) + (2 * p * cin * cout if cin != cout else 0)
    f += 2 * res(512, 512, px) + 2 * px * 512 * 512 * 4 + 4 * px * px * 512
    cin = 512
    for lvl, cout in enumerate(reversed(boc)):
        for _ in range(3):
            f += res(cin, cout, px)
            cin = cout
        if lvl != 3:
            px *= 4
            f += 2 * px * 9 * cin * cin
    f += 2 * px * 9 * 128 * 3
    return f


def self_launch_command(n_gpus, argv, port):
    """The command `bench.py --gpus N` re-executes itself under when it was started plainly (no WORLD_SIZE in the environment):
    one rank per GPU on this node, rendezvous on 127.0.0.1 — the same launch line the driver uses."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def maybe_self_launch(args, argv):
    """`python bench.py --gpus N` with N > 1 and no launcher: spawn the N ranks ourselves.  Fails loudly if the node has fewer
    than N devices (unless FMI_BENCH_BACKEND=gloo, the debugging mode in which ranks share devices)."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    import subprocess
    import torch
    n_dev = torch.cuda.device_count()
    if os.environ.get("FMI_BENCH_BACKEND", "nccl") == "nccl" and n_dev < args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus}: only {n_dev} GPU(s) visible on this node — one rank per GPU is required "
                         "(FMI_BENCH_BACKEND=gloo lets ranks share a device for debugging)")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = self_launch_command(args.gpus, argv, port)
    print(f"[bench] --gpus {args.gpus} without a launcher: starting {args.gpus} ranks: {' '.join(cmd)}", file=sys.stderr)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.call(cmd, env=env))


def measure_traffic_live(quant_args, denoise_steps=4, timeout=300):
    """roofline.traffic measured by THIS run: two short rocprofv3 counter passes (--pmc FETCH_SIZE, then --pmc WRITE_SIZE: the TCC
    cannot hold both, and counters are never combined with traces) over a child `bench.py` that runs `denoise_steps` steps of the
    same workload, summed over the block-linear GEMM kernels and divided by their dispatch count.  FETCH_SIZE x 2 is the gfx950
    correction of MI355X_MICROARCH.md (HBM section).  Returns (bytes per launch | None, note)."""
    import glob
    import re
    import shutil
    import signal
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not found"
    if any(k.startswith(("ROCPROF", "ROCP_TOOL", "ROCPROFILER")) for k in os.environ):
        return None, "this run is itself under a profiler: no nested counter passes"
    rx = re.compile(r"fmi::gemm_(pp|w4|w4q)_kernel<")
    kib, disp = {}, 0
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["TMPDIR"] = "/tmp"
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="fmi_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--pmc", counter, "-d", d, "-o", "pmc", "--", sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--no-secondary",
                   "--no-profile-pass", "--no-live-traffic", "--denoise-steps", str(denoise_steps), "--steps", "1", "--warmup", "0"] + list(quant_args)
            pr = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                rc = pr.wait(timeout=timeout)
            except subprocess.TimeoutExpired:
                os.killpg(pr.pid, signal.SIGKILL)  # exactly the process group started above
                pr.wait()
                return None, f"rocprofv3 --pmc {counter} pass timed out after {timeout} s"
            dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
            if rc != 0 or not dbs:
                return None, f"rocprofv3 --pmc {counter} pass failed (exit code {rc})"
            con = sqlite3.connect(dbs[0])
            rows = [r for r in con.execute("select kernel_name, count(*), sum(value) from counters_collection where counter_name=? group by kernel_name",
                                           (counter,)) if rx.search(r[0])]
            con.close()
            n = sum(r[1] for r in rows)
            if not n:
                return None, f"no block-linear GEMM dispatch in the --pmc {counter} pass"
            kib[counter], disp = sum(r[2] for r in rows) / n, n
        except Exception as e:  # a missing table, an unreadable database ...
            return None, f"--pmc {counter} pass: {type(e).__name__}: {e}"
        finally:
            shutil.rmtree(d, ignore_errors=True)
    note = (f"measured by this run: HBM-side (L2-miss) bytes per block-linear launch = FETCH_SIZE*2 + WRITE_SIZE, two separate rocprofv3 --pmc passes "
            f"(FETCH_SIZE {kib['FETCH_SIZE']:.0f} KiB, WRITE_SIZE {kib['WRITE_SIZE']:.0f} KiB per launch as reported; x2 = the gfx950 FETCH_SIZE correction) over a child "
            f"`bench.py --denoise-steps {denoise_steps} --steps 1 --warmup 0` of the same workload, {disp} GEMM dispatches; Infinity-Cache hits are included")
    return int((2 * kib["FETCH_SIZE"] + kib["WRITE_SIZE"]) * 1024), note


DUMP_LIMIT_BYTES = 64 * 2**20


def dump_outputs(dirname, arrays, limit=DUMP_LIMIT_BYTES):
    """Writes each array as dirname/<name>.npy in float32 (float64 stays float64).  Above `limit` bytes in all, every array takes a share of
    it in proportion to its size, as a fixed sample (seed 0, sorted flat indices, saved flat): two builds given the same arguments
    write the same elements, so their files compare element for element."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    host = {}
    for name, a in arrays.items():
        if hasattr(a, "detach"):  # a torch tensor (bf16 has no numpy type: widen on the way)
            a = a.detach().cpu()
            a = (a if a.is_floating_point() and a.element_size() == 8 else a.float()).numpy()
        a = np.asarray(a)
        host[name] = a if a.dtype == np.float64 else a.astype(np.float32)
    total = sum(a.nbytes for a in host.values())
    for name, a in host.items():
        if total > limit:
            keep = max(1, int(a.size * limit / total))
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=keep, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, f"{name}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2, help="images to time (one step = one 50-step image)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--txt-tokens", type=int, default=512)
    ap.add_argument("--quant", choices=["none", "nf4", "fp8", "int8"], default="none",
                    help="nf4: block linears stored bitsandbytes-nf4, fused dequant-GEMM (config C3); fp8: block linears on the e4m3 MFMA path (config C5); "
                         "int8: the int8 MFMA on the default linear mask (all but the double blocks' MLP); both 8-bit modes hand q and k to the attention as e4m3 (static scales), P.V stays bf16")
    ap.add_argument("--int8-mask", type=lambda v: int(v, 0), default=None, help="--quant int8: the FMI_Q8_* linear mask (default: the library's FMI_INT8_DEFAULT_MASK)")
    ap.add_argument("--int8-unsmoothed", action="store_true", help="int8 legs: round 5's recipe without the calibrated per-channel smoothing (fmi_flux_calibrate_int8)")
    ap.add_argument("--batch", type=int, default=1, help="samples per GPU per image step (C5: 2)")
    ap.add_argument("--sequence-parallel", action="store_true",
                    help="N > 1: all ranks denoise ONE image together (token shards, two all-to-alls per block; strong scaling) instead of one image each")
    ap.add_argument("--split-k", action="store_true", help="with --sequence-parallel: the opt-in latency mode (fmi_flux_set_split_k)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline figure: profiled pass, live PMC traffic, energy, image CRCs, secondary legs, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32; at most 64 MB, a seeded sample beyond)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the nf4 (C3) and fp8 (C5 shape) legs appended to the N = 1 line")
    ap.add_argument("--no-profile-pass", action="store_true")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="roofline.traffic from profiles/pmc_summary_latest.json instead of two rocprofv3 --pmc passes of a short child run (~1 min)")
    ap.add_argument("--cpu-baseline-tokens", type=int, default=0, help="override L of the CPU sample (debug)")
    ap.add_argument("--cpu-baseline-budget-s", type=float, default=300.0,
                    help="host seconds the default run may spend on the whole-step CPU sample (estimated from a probe GEMM); beyond it the two-block sample is used")
    ap.add_argument("--cpu-baseline-blocks", action="store_true",
                    help="cpu_baseline from one double + one single block (round 3's bounded sample) instead of one WHOLE C2 step on the full f32 model "
                         "(the default when the host has the memory for its 48 GB of weights)")
    ap.add_argument("--as-rank", type=int, default=None, help="N = 1 only: draw the prompts / latents that rank R of an --as-world job draws (test hook: "
                    "the images of an N-GPU run must equal the single-GPU images of the same global samples)")
    ap.add_argument("--as-world", type=int, default=None)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be at least 1 and --warmup at least 0")
    if not args.full:  # a plain run: the headline figure only
        args.no_cpu_baseline = args.no_secondary = args.no_profile_pass = args.no_live_traffic = True
    maybe_self_launch(args, sys.argv[1:])

    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: launched with WORLD_SIZE={world} but --gpus {args.gpus}; they must agree (n_gpus in the JSON line is the number of ranks)")
    if (args.as_rank is None) != (args.as_world is None) or (args.as_rank is not None and (world != 1 or not 0 <= args.as_rank < args.as_world)):
        raise SystemExit("bench.py: --as-rank R --as-world N go together, on one GPU, with 0 <= R < N")
    # which global samples / prompt seed this process draws: its own rank's, or (test hook) those of rank R in a job of N
    srank, sworld = (rank, world) if args.as_rank is None else (args.as_rank, args.as_world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    # debugging aid for boxes with fewer GPUs than ranks: FMI_BENCH_BACKEND=gloo lets several ranks share device 0
    backend = os.environ.get("FMI_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = local_rank % torch.cuda.device_count()
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} has no GPU (LOCAL_RANK {local_rank}, {torch.cuda.device_count()} visible): one rank per GPU is required")
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend, rank=rank, world_size=world)

    import diffusion_rs_amd as d
    from diffusion_rs_amd import _lib as L
    from diffusion_rs_amd import synth
    lib = L.load()
    dev = torch.device("cuda", local_rank)

    # ---------------- model: random-init FLUX.1-dev + FLUX VAE.  N > 1: rank 0 generates the DiT and its flat weight arenas
    # go out over RCCL (dist.broadcast_state: a ~1 KB layout blob, then a few dozen 1-GiB messages); the 168 MB VAE is
    # generated by every rank from the same seed.
    from diffusion_rs_amd import dist as fdist

    def is_quant_linear(name):  # what a bitsandbytes checkpoint quantises: every nn.Linear of the blocks + norm_out.linear
        return name.endswith(".weight") and ((("transformer_blocks." in name) and ("attn.norm" not in name)) or name == "norm_out.linear.weight")

    def fill_flux(model, quant):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        for name, shape in synth.flux_tensor_shapes(d.FLUX_DEV).items():
            if "norm_q" in name or "norm_k" in name or "norm_added" in name:
                t = torch.ones(shape, dtype=torch.bfloat16, device=dev)
            elif name.endswith(".bias"):
                t = torch.zeros(shape, dtype=torch.bfloat16, device=dev)
            else:
                t = torch.randn(shape, generator=g, device=dev, dtype=torch.bfloat16)
                t.mul_(synth._std_for(name, 0.02, 0.01))
            if quant == "nf4" and is_quant_linear(name):
                packed, absmax = synth.quantize_nf4_device(t, 64)
                model.set_linear_bnb4(name[:-len(".weight")], packed, absmax, 64, "nf4", shape[0], shape[1])
                del packed, absmax
            else:
                model.set_tensor(name, t)
            del t
        model.assert_complete()

    t_load = time.time()
    flux = d.FluxModel(d.FLUX_DEV, local_rank)
    vae = d.AutoEncoderKl(d.VAE_FLUX, local_rank)
    gen_err = None
    try:
        if rank == 0:
            fill_flux(flux, "nf4" if args.quant == "nf4" else "none")
    except Exception as e:  # the other ranks must hear about it instead of waiting in the broadcast
        gen_err = e
    fdist.agree_or_raise(gen_err, "weight generation on rank 0")
    torch.cuda.synchronize()
    gen_s = time.time() - t_load
    bcast = fdist.broadcast_state(flux, dev) if world > 1 else None
    if args.quant == "fp8":
        flux.quantize_fp8()
    int8_main_pending = args.quant == "int8"  # (calibrated below, once the workload's inputs exist)
    synth.fill_vae_random_device(vae, seed=1, device=dev)
    torch.cuda.synchronize()
    load_s = time.time() - t_load
    # single-image sequence parallelism: the ranks work on the SAME image, each on 1/N of its tokens
    spg = None
    if args.sequence_parallel and world > 1:
        if args.quant in ("fp8", "int8") or args.batch != 1:
            raise SystemExit("--sequence-parallel runs one bf16 / nf4 image at a time (batch 1)")
        spg = fdist.SequenceParallel(dev)
        spg.attach(flux)
        flux.set_split_k(args.split_k)

    # ---------------- synthetic inputs resident in HBM (per rank: its own prompt / seed)
    NS, T = args.denoise_steps, args.txt_tokens
    sched = d.SchedulerConfig()

    class Workload:
        """One (resolution, batch) configuration: inputs in HBM, the per-image hot path, and the profiled pass."""

        def __init__(self, H, W, B):
            self.H, self.W, self.B = H, W, B
            self.h, self.w = (H + 15) // 16 * 2, (W + 15) // 16 * 2
            self.S = (self.h // 2) * (self.w // 2)
            gi = torch.Generator(device=dev)
            gi.manual_seed(1234 + (0 if spg is not None else srank))  # sequence parallel: every rank holds the same prompt
            self.txt = torch.randn((B, T, 4096), generator=gi, device=dev, dtype=torch.float32).to(torch.bfloat16)
            self.y = torch.randn((B, 768), generator=gi, device=dev, dtype=torch.float32)
            self.guidance = torch.full((B,), 3.5, dtype=torch.float32, device=dev)
            self.txt_ids = torch.zeros((B, T, 3), dtype=torch.float32, device=dev)
            self.timesteps = sched.get_timesteps(NS, sched.calculate_shift(self.S))

        def calibrate_int8(self, model):
            """The int8 mode's calibration (round 6, fmi_flux_calibrate_int8; what Pipeline(dtype=I8) does at its first request): four bf16 evaluations of
            one sample across the schedule record the per-channel absmax of every block linear's input; quantize_int8 then folds the smoothing factors
            in.  Outside every timed region."""
            lat = d.randn_latents(1, 16, self.h, self.w, seed=4321, device=dev)
            img, img_ids = d.pack_latents(lat)
            model.calibrate_int8(True)
            n = len(self.timesteps) - 1
            for i in sorted({0, n // 3, 2 * n // 3, n - 1}):
                t = torch.full((1,), float(self.timesteps[i]), dtype=torch.float32, device=dev)
                model.forward(img, img_ids, self.txt[:1], self.txt_ids[:1], t, self.y[:1], self.guidance[:1])

        def one_image(self, model, i):
            if spg is not None and model is flux:  # same latents everywhere; each rank denoises its token shard, all get the result
                lat = d.randn_latents(self.B, 16, self.h, self.w, seed=1234, first_sample=i * self.B, device=dev)
                img, img_ids = d.pack_latents(lat)
                img = spg.gather(model.denoise(spg.shard(img), spg.shard(img_ids), spg.shard(self.txt), spg.shard(self.txt_ids), self.y, self.guidance,
                                               self.timesteps))
                self.last_latents = img
                z = d.unpack_latents(img, 16, self.h, self.w, vae.scale_factor(), vae.shift_factor())
                return d.postprocess_u8(vae.decode(z))
            lat = d.randn_latents(self.B, 16, self.h, self.w, seed=1234, first_sample=(srank + sworld * i) * self.B, device=dev)
            img, img_ids = d.pack_latents(lat)
            img = model.denoise(img, img_ids, self.txt, self.txt_ids, self.y, self.guidance, self.timesteps)
            self.last_latents = img  # (a reference: what --dump-outputs writes besides the image)
            z = d.unpack_latents(img, 16, self.h, self.w, vae.scale_factor(), vae.shift_factor())
            return d.postprocess_u8(vae.decode(z))

        def profile(self, model, kernel_desc, peak, traffic=None, traffic_note=None):
            """Per-phase hipEvent timing on the launch stream over the whole 50-step loop (the modulation precompute
            is per image, so a shorter pass would misprice it) -> (roofline object, extras, final latents)."""
            fl = step_flops(self.S, T, self.B)
            lat = d.randn_latents(self.B, 16, self.h, self.w, seed=99, device=dev)
            img, img_ids = d.pack_latents(lat)
            model.set_profiling(True)
            img = model.denoise(img, img_ids, self.txt, self.txt_ids, self.y, self.guidance, self.timesteps)
            torch.cuda.synchronize()
            ph = {k: v / NS for k, v in model.phase_ms().items()}
            model.set_profiling(False)
            gemm_ms = ph["gemm_qkv"] + ph["gemm_proj"] + ph["gemm_mlp"]
            gemm_launches = N_DOUBLE * 4 + N_SINGLE * 2
            gemm_fl = fl["gemm"] - self.B * (2 * self.S * 64 * D_HID + 2 * T * 4096 * D_HID + 2 * self.S * D_HID * 64)
            ach = gemm_fl / (gemm_ms * 1e-3) / 1e12
            roof = {"bound": "mfma", "kernel": kernel_desc, "achieved": round(ach, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                    "traffic": traffic, "launches_per_step": gemm_launches, "avg_launch_ms": round(gemm_ms / gemm_launches, 4),
                    "flop_per_launch_avg": gemm_fl / gemm_launches,
                    "measured_on": f"profiled pass, {NS} denoise steps, hipEvents on the launch stream"}
            if traffic_note:
                roof["traffic_note"] = traffic_note
            ex = {"phase_ms_per_denoise_step": {k: round(v, 3) for k, v in ph.items()},
                  "attention_tflops": round(fl["attn"] / (ph["attention"] * 1e-3) / 1e12, 1), "step_flops": fl}
            return roof, ex, img

    wl = Workload(args.height, args.width, args.batch)
    if int8_main_pending:
        if not args.int8_unsmoothed:
            wl.calibrate_int8(flux)
        flux.quantize_int8(args.int8_mask)
    H, W, B, S, h, w = wl.H, wl.W, wl.B, wl.S, wl.h, wl.w

    def one_image(i):
        return wl.one_image(flux, i)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def energy_uj():
        # socket energy counter of this rank's GPU (rocm-smi, ~0.3 s per call: read outside the timed region)
        try:
            import re
            import subprocess
            o = subprocess.run(["rocm-smi", "--showenergycounter"], capture_output=True, text=True, timeout=20).stdout
            m = re.findall(r"GPU\[(\d+)\]\s*:\s*Accumulated Energy \(uJ\):\s*([\d.]+)", o)
            d_ = {int(k): float(v) for k, v in m}
            return d_.get(local_rank)
        except Exception:
            return None

    for i in range(args.warmup):
        u8 = one_image(i)
    barrier()
    e_start = energy_uj() if rank == 0 and args.full else None
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        u8 = one_image(args.warmup + i)
    barrier()
    elapsed = time.perf_counter() - t0
    e_end = energy_uj() if rank == 0 and args.full else None
    per_rank_ms = [elapsed / args.steps * 1e3]
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        allt = [torch.zeros_like(tt) for _ in range(world)]
        dist.all_gather(allt, tt)
        per_rank_ms = [float(t.item()) / args.steps * 1e3 for t in allt]
        elapsed = max(float(t.item()) for t in allt)  # the job is as slow as its slowest rank
    finite = bool(torch.isfinite(u8.float()).all().item()) and int(u8.max()) > int(u8.min())

    # gather the decoded images to rank 0 (outside the timed region; 3 MB/sample over xGMI)
    gather_ms = None
    if world > 1 and spg is None:
        torch.cuda.synchronize()
        tg = time.perf_counter()
        gathered = fdist.gather_to_rank0(u8, world * B)
        torch.cuda.synchronize()
        gather_ms = (time.perf_counter() - tg) * 1e3
        if rank == 0:
            assert gathered.shape[0] == world * B
    if rank == 0 and args.dump_outputs:  # what the last timed step computed: the image(s) rank 0 holds, and its denoised latents
        dump_outputs(args.dump_outputs, {"image": gathered if world > 1 and spg is None else u8, "latents": wl.last_latents})
    # CRC-32 of the last image of every rank (rank order; after the gather for N > 1): lets a test check that an image does not depend
    # on how many GPUs the job ran on (tests/test_gpu_multi_device.py)
    image_crc = None
    if rank == 0 and spg is None and args.full:
        import zlib
        imgs = gathered if world > 1 else u8
        image_crc = [zlib.crc32(imgs[j].contiguous().cpu().numpy().tobytes()) for j in range(imgs.shape[0])]

    # ---------------- profiled pass: per-phase hipEvent timing on the launch stream
    roof = None
    extra = {}
    if e_start is not None and e_end is not None and e_end > e_start:
        # includes ~0.3 s of idle (two rocm-smi calls) around the timed region: a <= 1 % overestimate per image
        extra["energy_j_per_image_rank0"] = round((e_end - e_start) / 1e6 / (args.steps * B), 1)
        extra["avg_power_w_rank0"] = round((e_end - e_start) / 1e6 / elapsed, 1)
    KDESC = {"none": "gemm_pp_kernel (bf16 MFMA GEMM: the 152 block-linear launches of a step)",
             "nf4": "gemm_w4q_kernel (fused nf4 dequant-GEMM on the packed weights: the 152 block-linear launches of a step; dense-equivalent FLOPs)",
             "fp8": "gemm_pp_kernel<fp8> (e4m3 MFMA GEMM, all block linears)",
             "int8": "gemm_pp_kernel<int8> (v_mfma_i32_32x32x32_i8: double q|k|v + attention out, single linear1 + linear2) + gemm_pp_kernel<bf16> (the double "
                     "blocks' MLP); one average over both kinds of launch, priced against the int8 peak"}
    PEAK_NOTE = "2500 = dense bf16 MFMA peak at 2.4 GHz; a register-only MFMA loop (tools/mfma_peak.hip) sustains 2020-2160 on this part (power cap, ~1.95 GHz)"
    if rank == 0 and not args.no_profile_pass and spg is None:  # (the profiled pass is a single-device pass)
        traffic = tnote = None
        if args.quant == "none":
            live_note = None
            if world == 1 and not args.no_live_traffic and (args.height, args.width, args.batch) == (1024, 1024, 1):
                torch.cuda.synchronize()
                traffic, live_note = measure_traffic_live([])
                if traffic is not None:
                    tnote = live_note
            if traffic is None:
                try:  # the committed summary of this round's separate rocprofv3 --pmc passes (tools/profile_round.sh)
                    with open(os.path.join(ROOT, "profiles", "pmc_summary_latest.json")) as f:
                        pm = json.load(f)
                    traffic = pm.get("traffic_bytes_per_launch")
                    tnote = ("HBM-side bytes per block-linear launch = FETCH_SIZE*2 + WRITE_SIZE from separate rocprofv3 --pmc passes of the same command "
                             f"({pm.get('source', 'profiles/')}); read from profiles/pmc_summary_latest.json, not re-measured inside this run"
                             + (f" ({live_note})" if live_note else ""))
                except Exception:
                    pass
        roof, ex, img = wl.profile(flux, KDESC[args.quant], 5000.0 if args.quant in ("fp8", "int8") else 2500.0, traffic, tnote)
        roof["peak_note"] = PEAK_NOTE
        extra.update(ex)
        # VAE decode timing
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        z = d.unpack_latents(img, 16, h, w, vae.scale_factor(), vae.shift_factor())
        torch.cuda.synchronize()
        e0.record()
        vae.decode(z)
        e1.record()
        torch.cuda.synchronize()
        extra["vae_decode_ms"] = round(e0.elapsed_time(e1), 2)
        extra["vae_tflops"] = round(vae_flops(h, w) / (e0.elapsed_time(e1) * 1e-3) / 1e12, 1)
    extra["weights_resident_gib"] = round(flux.size_in_bytes() / 2**30, 2)

    # the GPU's answer for the one model evaluation the CPU baseline times below (taken now: the secondary legs switch `flux` to fp8)
    gpu_pred0 = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline and args.quant == "none" and (args.height, args.width, args.batch) == (1024, 1024, 1):
        lat0 = d.randn_latents(1, 16, h, w, seed=1234, first_sample=0, device=dev)
        img0, ids0 = d.pack_latents(lat0)
        t_first = float(wl.timesteps[0])
        # one Euler step with dt = -1 returns img - pred (fmi_flux_denoise keeps the latent f32)
        gpu_pred0 = (img0 - flux.denoise(img0.clone(), ids0, wl.txt, wl.txt_ids, wl.y, wl.guidance, [t_first, t_first - 1.0])).cpu().numpy()

    # ---------------- secondary legs (N = 1): config C3 (nf4) and the C5 shape (fp8, 1280x720, batch 2), 2 images each
    secondary = None
    if rank == 0 and world == 1 and args.quant == "none" and not args.no_secondary and (args.height, args.width, args.batch) == (1024, 1024, 1):
        secondary = {}

        ref_images = {}  # (H, W, B) -> the bf16 model's image of sample 0 at that shape: what a mode's image of the same sample is compared with

        def image_drift(a, b_):
            """u8 image of a mode against the bf16 model's for the same latents after all NS steps: the whole pipeline's drift, not a per-forward
            figure (random-init weights: the trajectories diverge faster than a trained model's; the per-forward distances are DESIGN 5's)"""
            df = (a.to(torch.int16) - b_.to(torch.int16)).abs().float()
            mse = float((df * df).mean())
            return {"mean_abs_du8": round(float(df.mean()), 3), "frac_within_2": round(float((df <= 2).float().mean()), 4), "frac_within_8": round(float((df <= 8).float().mean()), 4),
                    "psnr_db": round(10.0 * math.log10(255.0 ** 2 / mse), 2) if mse > 0 else None}

        def leg(model, wk, name, kdesc, peak, dtype):
            key = (wk.H, wk.W, wk.B)
            if key not in ref_images and model is not flux:  # (legs that convert `flux` itself run last: the reference of their shape is taken before)
                ref_images[key] = wk.one_image(flux, 0)
            first = wk.one_image(model, 0)  # warm-up (workspace allocation, first-use paths); also the image the drift is measured on
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(2):
                out = wk.one_image(model, 1 + i)
            torch.cuda.synchronize()
            el = time.perf_counter() - t1
            traffic = tnote = None
            mode = name.split("_")[0]  # nf4 / int8 / fp8: the legs that have PMC passes of their own under profiles/
            if (wk.H, wk.W, wk.B) == (1024, 1024, 1) and mode in ("nf4", "int8", "fp8"):  # the PMC passes are taken at the headline shape
                try:
                    with open(os.path.join(ROOT, "profiles", f"pmc_summary_{mode}.json")) as f:
                        pm = json.load(f)
                    traffic = pm.get("traffic_bytes_per_launch")
                    tnote = f"FETCH_SIZE*2 + WRITE_SIZE per block-linear launch from separate rocprofv3 --pmc passes ({pm.get('source', 'profiles/')}); not re-measured inside this run"
                except Exception:
                    pass
            r, ex, _ = wk.profile(model, kdesc, peak, traffic, tnote)
            secondary[name] = {"value": 2 * wk.B / el, "unit": "images/s", "images": 2 * wk.B, "ms_per_image": round(el / (2 * wk.B) * 1e3, 1),
                               "ms_per_denoise_step": round(el / 2 / NS * 1e3, 2), "dtype": dtype,
                               "config": {"workload": f"FLUX.1-dev {wk.W}x{wk.H} {NS}-step, batch={wk.B}, S={wk.S} img + T={T} txt tokens"},
                               "output_ok": bool(int(out.max()) > int(out.min())), "roofline": r, "weights_resident_gib": round(model.size_in_bytes() / 2**30, 2),
                               "phase_ms_per_denoise_step": ex["phase_ms_per_denoise_step"], "attention_tflops": ex["attention_tflops"]}
            if key in ref_images and first.shape == ref_images[key].shape:  # (every leg's model holds the same seeded weights, nf4: their nf4 codes)
                secondary[name]["image_vs_bf16_same_latents"] = image_drift(first, ref_images[key])

        # single-image sequence parallelism: what one of 8 ranks computes per denoise step, exchange as a loopback copy
        # of the right size (everything but the xGMI wire time) — bit-identical default and the opt-in split-K latency mode
        ts10 = sched.get_timesteps(10, sched.calculate_shift(4096))
        sp = {"note": "per-rank compute of ONE image on 8 ranks, measured on this one GPU with a loopback all-to-all "
                      "(dist.sequence_parallel_rank_time); one device runs the same step in ms_per_denoise_step above; wire time not included"}
        sp["default_bit_identical"] = fdist.sequence_parallel_rank_time(flux, 8, ts10, dev)
        flux.set_split_k(True)
        sp["split_k_latency_mode"] = fdist.sequence_parallel_rank_time(flux, 8, ts10, dev)
        flux.set_split_k(False)
        secondary["sequence_parallel_rank"] = sp
        # opt-in (fmi_flux_set_fp8_attention(m, 2)): the bf16 model with q and k handed to the attention as e4m3 (static scales), QK^T on the fp8 MFMA in the
        # lock-step stream — a reduced-precision attention operand, so never the headline; the leg says what it is worth
        ref_images[(wl.H, wl.W, wl.B)] = wl.one_image(flux, 0)
        wl_c5 = Workload(720, 1280, 2)
        ref_images[(720, 1280, 2)] = wl_c5.one_image(flux, 0)
        flux.set_fp8_attention(2)
        leg(flux, wl, "bf16_e4m3qk_1024", KDESC["none"], 2500.0, "bf16 block linears and P.V; q, k of the attention as e4m3 with static per-block scales (opt-in)")
        flux.set_fp8_attention(1)
        fq = d.FluxModel(d.FLUX_DEV, local_rank)
        fill_flux(fq, "nf4")
        # opt-in policy (fmi_flux_set_quant_dense_cache(0)): only the packed codes are resident; the block linears (launches above 383 rows) expand per call
        # into a 264 MB scratch (stand-alone dequant kernel) and run the dense GEMM, smaller launches multiply from the packed codes
        fq.set_quant_dense_cache(0)
        leg(fq, wl, "nf4_c3_packed", "dequant4_kernel + gemm_pp_kernel (nf4 block linears expanded per call into a scratch, then the dense bf16 MFMA GEMM; "
            "the expansions are inside the timed phases; dense-equivalent FLOPs)", 2500.0,
            "bf16 MFMA on nf4 weights (bitsandbytes blocksize 64; every block + modulation linear packed; no bf16 copy resident)")
        # default policy since round 5 (by memory, flux_model.hip: resolve_quant_mode): on a part with the room the block matrices of the large launches are
        # expanded ONCE (BnbLinear::forward's "dequantise, then matmul" without repeating the first half 228 times per step); the 6.5 GB modulation matrix and
        # every launch of up to 383 rows keep multiplying from the packed codes.  Same bits as the packed policy.
        fq.set_quant_dense_cache(-1)
        leg(fq, wl, "nf4_c3", "gemm_pp_kernel on nf4 block linears expanded once into the bf16 arena (+16 GB; the modulation matrix and small launches stay on the "
            "fused dequant-GEMM); dense-equivalent FLOPs", 2500.0,
            "bf16 MFMA on nf4 weights (bitsandbytes blocksize 64): packed codes + one expanded copy of the block matrices resident (the default when HBM allows)")
        fq.close()
        del fq
        # int8 mode (round 4): its own handle (bf16 weights + int8 codes of the masked linears), default mask = all but the double blocks' MLP
        fi = d.FluxModel(d.FLUX_DEV, local_rank)
        fill_flux(fi, "none")
        if not args.int8_unsmoothed:
            wl.calibrate_int8(fi)
        fi.quantize_int8()
        leg(fi, wl, "int8_1024", KDESC["int8"], 5000.0,
            "int8 block linears (per-channel weight / per-token activation scales on per-input-channel smoothed operands — s = sqrt(amax_x / amax_W) from a 4-evaluation calibration —, exact int32 accumulate) for double q|k|v + attention out and single "
            "linear1 + linear2; attention with e4m3 q / k operands (static per-block scales, QK^T on the fp8 MFMA) and bf16 P.V; the double blocks' MLP and everything else bf16; f32 residual stream")
        leg(fi, wl_c5, "int8_c5_shape", KDESC["int8"], 5000.0, "as int8_1024 (BASELINE configs[4]'s shape, 1280x720 batch 2, in the 8-bit mode that is within tolerance)")
        fi.close()
        del fi
        flux.quantize_fp8()  # last: the headline model itself switches to the fp8 path
        fp8_dtype = "fp8 e4m3 block linears (per-channel weight / per-token activation scales, f32 accumulate), fp8 QK^T, f32 residual stream"
        leg(flux, wl, "fp8_1024", KDESC["fp8"], 5000.0, fp8_dtype)  # the headline workload (1024x1024, batch 1) in fp8 mode
        leg(flux, wl_c5, "fp8_c5_shape", KDESC["fp8"], 5000.0, fp8_dtype)

    if rank == 0:
        ms_per_image = elapsed / args.steps * 1e3
        total_images = args.steps * B * (1 if spg is not None else world)
        out = {
            "metric": "images/sec, FLUX.1-dev 1024x1024 50-step" if (H, W, NS) == (1024, 1024, 50) else f"images/sec, FLUX.1-dev {W}x{H} {NS}-step",
            "value": total_images / elapsed, "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_image, "higher_is_better": True, "scaling": "strong" if spg is not None else "weak", "vs_baseline": None, "dtype": {"none": "bf16", "nf4": "bf16 MFMA on nf4 weights (default policy: block matrices expanded once when HBM allows, modulation / small launches fused dequant-GEMM on the packed codes)",
                                                                                                                 "fp8": "fp8 e4m3 block linears (per-channel weight / per-token activation scales, f32 accumulate); attention: e4m3 q / k operands with static per-block scales (QK^T on the fp8 MFMA), bf16 P.V; f32 residual stream",
                                                                                                                 "int8": "int8 block linears on the default mask (per-channel / per-token scales, exact int32 accumulate); attention: e4m3 q / k operands with static per-block scales (QK^T on the fp8 MFMA), bf16 P.V; the double blocks' MLP and everything else bf16, f32 residual stream"}[args.quant],
            "data": "synthetic (random-init FLUX.1-dev + FLUX VAE weights, N(0,1) embeddings, Philox latents)",
            "config": {"workload": f"FLUX.1-dev {args.quant if args.quant in ('fp8', 'int8') else 'bf16'} {W}x{H} {NS}-step, batch={B} per GPU, S={S} img + T={T} txt tokens, step = one image "
                                   "(50x Flux::forward + Euler, unpack, VAE decode, u8)",
                       "global_batch": B if spg is not None else world * B,
                       "parallelism": (f"sequence-parallel x{world} (one image on all ranks{', split-K latency mode' if args.split_k else ''})" if spg is not None
                                       else f"batch-sharded x{world}" if world > 1 else "single GPU")},
            "ms_per_denoise_step": round((ms_per_image - extra.get("vae_decode_ms", 0.0)) / NS, 2),
            "ms_per_image": round(ms_per_image, 1),
            "output_ok": finite, "load_s": round(load_s, 1), "weights_generated_s": round(gen_s, 1),
            "roofline": roof, "cpu_baseline": None,
        }
        out["ms_per_step_per_rank"] = [round(x, 1) for x in per_rank_ms]
        out["build_id"] = lib.fmi_build_id().decode()
        if image_crc is not None:
            out["image_crc32"] = image_crc
        if args.as_rank is not None:
            out["drawn_as"] = {"rank": args.as_rank, "world": args.as_world}
        if world > 1:
            out["rccl_ranks"] = world
            out["backend"] = backend
            out["broadcast_s"] = round(bcast["seconds"], 2)
            out["broadcast_gib"] = round(bcast["bytes"] / 2**30, 2)
            out["broadcast_messages"] = bcast["messages"]
            if gather_ms is not None:
                out["gather_ms"] = round(gather_ms, 2)
            if spg is not None:
                out["exchanges"] = spg.exchanges
                out["exchange_gb_sent_rank0"] = round(spg.bytes_sent / 1e9, 2)
        if secondary is not None:
            out["secondary"] = secondary
        out.update(extra)
        if world == 1 and not args.no_cpu_baseline:
            # The GPU figures are complete here.  They go to stderr BEFORE the CPU baseline starts — minutes of host work that can be
            # OOM-killed — and to stdout as THE one JSON line once the baseline has been added.
            sys.stderr.write("[bench] GPU line (cpu_baseline pending): " + json.dumps(out) + "\n")
            sys.stderr.flush()

    # ---------------- CPU baseline (rank 0, N=1 only): oracle = port of the reference CPU semantics
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
      try:  # (a host-side failure of the reported baseline must not take the measured GPU line with it: ADVICE r4)
        from oracle import oracle as orc

        orc.set_threads(orc.usable_cpus())  # affinity capped by the cgroup CPU quota (16 of the box's 256 logical CPUs)
        cpu_model, logical = "unknown", os.cpu_count()
        try:
            for line in open("/proc/cpuinfo"):
                if line.startswith("model name"):
                    cpu_model = line.split(":", 1)[1].strip()
                    break
        except OSError:
            pass

        def host_mem_gib():  # memory this process may still take: min(MemAvailable, cgroup limit)
            avail = 0.0
            try:
                for line in open("/proc/meminfo"):
                    if line.startswith("MemAvailable:"):
                        avail = int(line.split()[1]) / 2**20
            except OSError:
                pass
            for path in ("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory/memory.limit_in_bytes"):  # cgroup v2, v1
                try:
                    lim = open(path).read().strip()
                    if lim != "max":
                        avail = min(avail, int(lim) / 2**30)
                except (OSError, ValueError):
                    pass
            return avail

        Dh = D_HID
        rng = np.random.default_rng(0)
        whole = not args.cpu_baseline_blocks and not args.cpu_baseline_tokens and (H, W, B) == (1024, 1024, 1) and host_mem_gib() >= 100
        if whole:
            # bounded by a time budget: a probe GEMM at the step's dominant shape class prices the whole-step sample (model build + one
            # Flux::forward + the C1 run) before 48 GB are built for it; over budget -> the two-block sample below
            px, pw = rng.standard_normal((2048, Dh), dtype=np.float32), rng.standard_normal((Dh, Dh), dtype=np.float32)
            orc.linear(px, pw)
            tp = time.perf_counter()
            orc.linear(px, pw)
            rate = 2.0 * 2048 * Dh * Dh / (time.perf_counter() - tp)
            est_s = 30.0 + 1.2 * (step_flops(S, T)["total"] + 4 * step_flops(256, 256)["total"]) / rate
            if est_s > args.cpu_baseline_budget_s:
                sys.stderr.write(f"[bench] whole-step CPU sample estimated at {est_s:.0f} s > --cpu-baseline-budget-s {args.cpu_baseline_budget_s}: using the two-block sample\n")
                whole = False
            del px, pw
        if whole:
            # ONE WHOLE denoise step of the headline config on the oracle: the full FLUX.1-dev (19 + 38 blocks, every block its own
            # weights: the values rank 0 generated for the GPU, regenerated from the same seed and widened to f32 = 48 GB on the host),
            # S = 4096 + T = 512 tokens, Flux::forward end to end (embedders, modulation, blocks, final layer).  An image is 50 such
            # steps + one VAE decode: the steps are extrapolated x 50 (marked), the VAE by FLOPs from the 256 x 256 decode timed below.
            tb = time.perf_counter()
            om = orc.Flux(dict(d.FLUX_DEV))
            g = torch.Generator(device=dev)
            g.manual_seed(0)
            for name, shape in synth.flux_tensor_shapes(d.FLUX_DEV).items():  # the same stream of values as fill_flux(…, "none")
                if "norm_q" in name or "norm_k" in name or "norm_added" in name:
                    t = torch.ones(shape, dtype=torch.bfloat16, device=dev)
                elif name.endswith(".bias"):
                    t = torch.zeros(shape, dtype=torch.bfloat16, device=dev)
                else:
                    t = torch.randn(shape, generator=g, device=dev, dtype=torch.bfloat16)
                    t.mul_(synth._std_for(name, 0.02, 0.01))
                om.set_tensor(name, t.float().cpu().numpy())
                del t
            build_s = time.perf_counter() - tb
            lat = d.randn_latents(1, 16, h, w, seed=1234, first_sample=0, device=dev)
            img0, ids0 = d.pack_latents(lat)
            tvec = np.array([float(wl.timesteps[0])], np.float32)
            tc = time.perf_counter()
            ref = om.forward(img0.cpu().numpy(), ids0.cpu().numpy(), wl.txt.float().cpu().numpy(), wl.txt_ids.cpu().numpy(), tvec, wl.y.cpu().numpy(),
                             wl.guidance.cpu().numpy())
            step_s = time.perf_counter() - tc
            got = gpu_pred0  # the same evaluation on the GPU, for the record (the parity tests proper live in tests/)
            step_fl = step_flops(S, T)["total"]
            sample = (f"ONE whole denoise step of the headline config (FLUX.1-dev in full: 19 + 38 blocks with their own weights, 48 GB f32 on the host; "
                      f"S={S} + T={T} tokens; {step_fl / 1e12:.1f} TFLOP) timed in {step_s:.1f} s on {orc.get_threads()} host threads "
                      f"(model build {build_s:.0f} s, not counted); an image = that x {NS} (extrapolated) + the VAE decode scaled by FLOPs from the 256x256 decode timed under c1_full; "
                      "C++ restatement of the reference CPU semantics (oracle/, AVX2 register-blocked GEMM + OpenMP), not the reference binary")
            cpu = {"value": None, "unit": "images/s", "cores": orc.get_threads(), "kind": "port", "cpu_model": cpu_model, "logical_cpus_on_host": logical,
                   "gflops": round(step_fl / step_s / 1e9, 1), "step_seconds": round(step_s, 2), "sample": sample}
            if got is not None:
                num = float(np.linalg.norm(got.astype(np.float64) - ref.astype(np.float64)))
                cpu["gpu_vs_oracle_rel_l2_this_step"] = round(num / float(np.linalg.norm(ref.astype(np.float64))), 5)
        else:
            Sc, Tc = (S, T) if not args.cpu_baseline_tokens else (args.cpu_baseline_tokens * 3 // 4, args.cpu_baseline_tokens // 4)
            Lc = Sc + Tc
            cfg1 = dict(d.FLUX_DEV, num_layers=1, num_single_layers=1)
            om = orc.Flux(cfg1)
            for name, shape in synth.flux_tensor_shapes(cfg1).items():
                if "transformer_blocks.0." in name:  # double block 0 and single block 0
                    if "norm_q" in name or "norm_k" in name or "norm_added" in name:
                        a = np.ones(shape, np.float32)
                    else:
                        a = rng.standard_normal(shape, dtype=np.float32) * (0.01 if ("norm.linear" in name or "norm1" in name) else 0.02)
                    om.set_tensor(name, a)
            xi = rng.standard_normal((1, Sc, Dh), dtype=np.float32)
            xt = rng.standard_normal((1, Tc, Dh), dtype=np.float32)
            vec = rng.standard_normal((1, Dh), dtype=np.float32)
            ids = np.zeros((Lc, 3), np.float32)
            ids[Tc:, 1] = np.arange(Sc) // max(1, (w // 2))
            ids[Tc:, 2] = np.arange(Sc) % max(1, (w // 2))
            pe = orc.rope_table(ids, [16, 56, 56], 10000)[None]
            # one DoubleStreamBlock + one SingleStreamBlock at the full shape = 1/19 + 1/38 of a step's blocks
            blk_fl = 2 * (24 * Dh * Dh * Lc + 4 * Lc * Lc * Dh)
            reps, cpu_s = 0, 0.0
            while cpu_s < 10.0 and reps < 8:
                tc = time.perf_counter()
                a, b = om.double_block(0, xi, xt, vec, pe)
                om.single_block(0, np.concatenate([b, a], 1), vec, pe)
                cpu_s += time.perf_counter() - tc
                reps += 1
            img_fl = step_flops(S, T)["total"] * NS + vae_flops(h, w)
            cpu_ips = 1.0 / (cpu_s / reps * img_fl / blk_fl)
            cpu = {"value": cpu_ips, "unit": "images/s", "cores": orc.get_threads(), "kind": "port", "cpu_model": cpu_model, "logical_cpus_on_host": logical,
                   "gflops": round(blk_fl * reps / cpu_s / 1e9, 1),
                   "sample": f"{reps} x (one DoubleStreamBlock + one SingleStreamBlock at the full shape S={Sc}, T={Tc}, D=3072, f32, {blk_fl / 1e12:.2f} TFLOP) "
                             f"timed in {cpu_s:.1f} s on {orc.get_threads()} host threads, extrapolated to one image ({img_fl / 1e15:.2f} PFLOP) by "
                             "algorithmic FLOPs (the host lacks the memory for the whole-step sample, or it was switched off); C++ restatement of the reference "
                             "CPU semantics (oracle/, AVX2 register-blocked GEMM + OpenMP), not the reference binary"}
        # config C1 (BASELINE configs[0]: FLUX.1-schnell 256x256, 4 steps, S = T = 256 — the reference's own CPU-runnable case) executed IN FULL
        # on the oracle, VAE decode and u8 post-process included.  With the whole model on the host (above) every block runs its own weights
        # (the dev tensors without the guidance embedder = the schnell model); otherwise one double / one single block's weights serve every depth.
        if not args.cpu_baseline_tokens:
            S1 = T1 = 256
            vsd = synth.vae_state_dict_numpy(d.VAE_FLUX, seed=1)
            ov = orc.Vae(d.VAE_FLUX)
            ov.load(vsd)
            lat1 = rng.standard_normal((1, 16, 32, 32)).astype(np.float32)
            if whole:
                img1, ids1 = orc.pack_latents(lat1)
                t51 = rng.standard_normal((1, T1, 4096)).astype(np.float32)
                y1 = rng.standard_normal((1, 768)).astype(np.float32)
                ts1 = orc.get_timesteps(4, False, 0.0, 1.0)  # schnell: no dynamic shifting, shift = 1.0
                tc = time.perf_counter()
                out1 = om.denoise(img1, ids1, t51, np.zeros((1, T1, 3), np.float32), y1, None, ts1)
                dit_s = time.perf_counter() - tc
                z1 = orc.unpack_latents(out1, 16, 32, 32) / 0.3611 + 0.1159
            else:
                xi1 = rng.standard_normal((1, S1, Dh), dtype=np.float32)
                xt1 = rng.standard_normal((1, T1, Dh), dtype=np.float32)
                ids1 = np.zeros((S1 + T1, 3), np.float32)
                ids1[T1:, 1] = np.arange(S1) // 16
                ids1[T1:, 2] = np.arange(S1) % 16
                pe1 = orc.rope_table(ids1, [16, 56, 56], 10000)[None]
                tc = time.perf_counter()
                for _ in range(4):
                    a, b = xi1, xt1
                    for _ in range(N_DOUBLE):
                        a, b = om.double_block(0, a, b, vec, pe1)
                    x1 = np.concatenate([b, a], 1)
                    for _ in range(N_SINGLE):
                        x1 = om.single_block(0, x1, vec, pe1)
                dit_s = time.perf_counter() - tc
                z1 = lat1
            tc = time.perf_counter()
            u81 = orc.postprocess_u8(ov.decode(np.ascontiguousarray(z1, np.float32)))
            vae_s = time.perf_counter() - tc
            c1_s = dit_s + vae_s
            c1_fl = 4 * step_flops(S1, T1)["total"] + vae_flops(32, 32)
            cpu["c1_full"] = {"config": "FLUX.1-schnell 256x256 4-step, batch 1 (BASELINE configs[0]): 4 x Flux::forward + Euler, unpack, VAE decode, u8", "seconds": round(c1_s, 2),
                              "dit_seconds": round(dit_s, 2), "vae_decode_seconds": round(vae_s, 2),
                              "images_per_s": round(1.0 / c1_s, 4), "gflops": round(c1_fl / c1_s / 1e9, 1), "output_ok": bool(int(u81.max()) > int(u81.min())),
                              "note": ("executed in full on the oracle: the whole model at D=3072 (19 + 38 blocks, every block its own weights), S=T=256, real FLUX VAE config" if whole else
                                       "all 4 x 57 block evaluations executed at D=3072, S=T=256 with one double / one single block's weights reused for every depth (embedders and final "
                                       "layer, < 0.1 % of the FLOPs, left out) + the real-config VAE decode")}
            if whole:  # an image of the headline config: 50 measured-step equivalents + the VAE decode scaled by FLOPs from the one just timed
                vae_c2_s = vae_s * vae_flops(h, w) / vae_flops(32, 32)
                cpu["value"] = 1.0 / (cpu["step_seconds"] * NS + vae_c2_s)
                cpu["vae_decode_seconds_extrapolated"] = round(vae_c2_s, 1)
        if cpu.get("value") is None:  # (whole-step sample without the C1 leg: the VAE by FLOPs at the DiT's rate)
            cpu["value"] = 1.0 / (cpu["step_seconds"] * NS * (1.0 + vae_flops(h, w) / (step_flops(S, T)["total"] * NS)))

      except Exception as e:  # noqa: BLE001 — reported, not raised
        import traceback
        traceback.print_exc()
        cpu = {"value": None, "unit": "images/s", "cores": None, "kind": "port", "sample": f"the CPU baseline failed on this host: {type(e).__name__}: {e}"}

    if rank == 0:
        out["cpu_baseline"] = cpu
        print(json.dumps(out))
    if world > 1:
        dist.barrier()  # rank 0 ran the (untimed) profiled pass meanwhile: leave together
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
