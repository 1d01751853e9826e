"""CPU-only tests: host schedule math (library vs oracle vs closed form), API mirror objects,
the C-ABI library loads and exports every declared symbol, and the product fails loudly
without a GPU (no CPU fallback)."""
import ctypes as C
import json
import math
import os
import re
import struct
import zlib

import numpy as np
import pytest

import diffusion_rs_amd as d
from diffusion_rs_amd import _lib as L
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fmi_[a-z0-9_]+|dequantize_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 55
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert set(L.EXPORTED) == declared
    assert lib.fmi_abi_version() == 6


def test_product_and_test_build_of_the_library():
    """The shipped library carries what the product runs; the superseded kernels sit behind ONE build flag (-DFMI_ALT_KERNELS=1) that only the test
    build sets (libflux_mi355x_alt.so, `make alt`).  Both export the whole header, carry the same source id, and say which they
    are; the product library answers a request for a kernel it does not carry with an error, not with another kernel (no GPU needed: the
    switch is checked before any launch)."""
    lib = L.load()
    assert lib.fmi_has_alt_kernels() == 0
    assert lib.fmi_set_attention_kernel(3) == L.ERR_UNSUPPORTED and b"test build" in lib.fmi_last_error()
    assert lib.fmi_set_attention_kernel(5) == 0 and lib.fmi_set_attention_kernel(1) == 0 and lib.fmi_set_attention_kernel(5) == 0
    alt = L.load_alt()
    assert alt.fmi_has_alt_kernels() == 1 and L.load() is lib  # (loading the test build does not replace the product library)
    assert not [s for s in L.EXPORTED if not hasattr(alt, s)]
    assert alt.fmi_build_id() == lib.fmi_build_id() == L.tree_build_id(ROOT).encode()
    for kind in range(6):
        assert alt.fmi_set_attention_kernel(kind) == 0
    assert alt.fmi_set_attention_kernel(5) == 0
    with L.use_alt() as a:
        assert L.load() is a
    assert L.load() is lib
    so, so_alt = os.path.getsize(L.LIB_PATH), os.path.getsize(L.ALT_LIB_PATH)
    print(f"product library {so / 2**20:.1f} MiB, test build {so_alt / 2**20:.1f} MiB")
    assert so < so_alt


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = L.load()
    rc = lib.fmi_init(0)
    assert rc != 0
    assert len(lib.fmi_last_error()) > 0
    with pytest.raises(d.FmiError):
        d.FluxModel(d.FLUX_DEV)


def test_calculate_shift_and_timesteps_match_oracle_and_closed_form():
    s = d.SchedulerConfig()
    for seq in (256, 1024, 3600, 4096):
        mu = s.calculate_shift(seq)
        assert mu == orc.calculate_shift(seq)
        assert mu == pytest.approx(0.5 + (1.15 - 0.5) * (seq - 256) / (4096 - 256), abs=1e-12)
    assert s.calculate_shift(256) == pytest.approx(0.5)
    assert s.calculate_shift(4096) == pytest.approx(1.15)
    for n in (1, 4, 50):
        mu = s.calculate_shift(4096)
        ts = s.get_timesteps(n, mu)
        np.testing.assert_array_equal(np.array(ts), orc.get_timesteps(n, True, mu))
        assert ts[0] == 1.0 and ts[-1] == 0.0 and all(a > b for a, b in zip(ts, ts[1:]))
        for i, t in enumerate(ts[1:-1], 1):
            sig = (n - i) / n
            assert t == pytest.approx(math.exp(mu) / (math.exp(mu) + (1 / sig - 1)), rel=1e-14)
    sch = d.SchedulerConfig(shift=1.0, use_dynamic_shifting=False)  # schnell
    np.testing.assert_array_equal(np.array(sch.get_timesteps(4, None)), np.array([1.0, 0.75, 0.5, 0.25, 0.0]))
    np.testing.assert_array_equal(np.array(d.SchedulerConfig(shift=3.0, use_dynamic_shifting=False).get_timesteps(4, None)),
                                  orc.get_timesteps(4, False, 0.0, 3.0))
    with pytest.raises(ValueError):
        s.get_timesteps(4, None)  # `mu` is required for dynamic shifting (scheduler.rs:34)


def test_pack_unpack_roundtrip_oracle():
    rng = np.random.default_rng(0)
    lat = rng.standard_normal((2, 16, 6, 10)).astype(np.float32)
    img, ids = orc.pack_latents(lat)
    assert img.shape == (2, 15, 64) and ids.shape == (2, 15, 3)
    np.testing.assert_array_equal(orc.unpack_latents(img, 16, 6, 10), lat)
    # independent numpy restatement of State::new (reshape/permute chain of sampling.rs:131-133)
    ref = lat.reshape(2, 16, 3, 2, 5, 2).transpose(0, 2, 4, 1, 3, 5).reshape(2, 15, 64)
    np.testing.assert_array_equal(img, ref)
    assert ids[0, 7].tolist() == [0.0, 1.0, 2.0]  # token 7 = row 1, col 2


def test_postprocess_u8_truncates_and_saturates():
    x = np.array([-2.0, -1.0, -0.999, 0.0, 0.003, 0.999, 1.0, 3.0, np.nan], np.float32)
    np.testing.assert_array_equal(orc.postprocess_u8(x), np.array([0, 0, 0, 127, 127, 254, 255, 255, 0], np.uint8))


def test_api_mirror_objects():
    p = d.DiffusionGenerationParams(height=720, width=1280, num_steps=50, guidance_scale=3.5)
    assert repr(p) == "DiffusionGenerationParams(height = 720, width = 1280, num_steps = 50, guidance_scale = 3.5)"
    s = d.ModelSource.ModelId("black-forest-labs/FLUX.1-dev")
    assert repr(s) == "model id: black-forest-labs/FLUX.1-dev"
    s2 = s.override_transformer_model_id("x/y")
    assert s2.transformer_model_id == "x/y"
    with pytest.raises(ValueError):
        d.ModelSource.DdufFile("a.dduf").override_transformer_model_id("x")
    assert [m.name for m in d.ModelDType][:4] == ["Auto", "BF16", "F16", "F32"]  # the reference's four (lib.rs:37-44) ...
    assert [m.name for m in d.ModelDType][4:] == ["F8E4M3", "I8"]                # ... plus this build's two 8-bit extensions
    assert d.Offloading.Full.name == "Full"


def test_png_encoder_roundtrip():
    rgb = (np.arange(5 * 7 * 3) % 256).astype(np.uint8).reshape(5, 7, 3)
    png = d.encode_png(rgb)
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    off, idat = 8, b""
    while off < len(png):
        ln, tag = struct.unpack(">I4s", png[off:off + 8])
        body = png[off + 8:off + 8 + ln]
        assert zlib.crc32(tag + body) & 0xFFFFFFFF == struct.unpack(">I", png[off + 8 + ln:off + 12 + ln])[0]
        if tag == b"IHDR":
            assert struct.unpack(">IIBBBBB", body) == (7, 5, 8, 2, 0, 0, 0)
        if tag == b"IDAT":
            idat += body
        off += 12 + ln
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(5, 1 + 21)
    np.testing.assert_array_equal(raw[:, 1:].reshape(5, 7, 3), rgb)


def test_synthetic_shapes_cover_flux1():
    shapes = d.synth.flux_tensor_shapes(d.FLUX_DEV)
    n = sum(int(np.prod(s)) for s in shapes.values())
    assert 11.8e9 < n < 12.0e9  # FLUX.1's 12 B parameters (SURVEY §8d parameter check)
    assert shapes["single_transformer_blocks.37.proj_out.weight"] == (3072, 15360)
    assert shapes["transformer_blocks.18.norm1_context.linear.weight"] == (18432, 3072)
    assert "time_text_embed.guidance_embedder.linear_1.weight" not in d.synth.flux_tensor_shapes(d.FLUX_SCHNELL)
    v = d.synth.vae_tensor_shapes(d.VAE_FLUX)
    assert v["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)
    assert v["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"] == (128, 256, 1, 1)
    assert "decoder.up_blocks.3.upsamplers.0.conv.weight" not in v and "decoder.up_blocks.2.upsamplers.0.conv.weight" in v


def test_bnb_quantise_dequantise_consistency():
    rng = np.random.default_rng(1)
    w = rng.standard_normal(64 * 40).astype(np.float32)
    for qt in ("nf4", "fp4"):
        packed, absmax = orc.quantize_blockwise_4bit(w, 64, qt)
        dq = orc.dequantize_blockwise(None, packed, absmax, 64, w.size, qt)
        # every value is a code point times its block absmax, and the block max is reproduced exactly
        blocks = w.reshape(-1, 64)
        np.testing.assert_array_equal(np.abs(dq.reshape(-1, 64)).max(1), np.abs(blocks).max(1))
        assert np.abs(dq - w).max() <= 0.2 * np.abs(w).max()
        # bf16 / f16 outputs are the f32 outputs rounded once
        np.testing.assert_array_equal(orc.dequantize_blockwise(None, packed, absmax, 64, w.size, qt, "bf16"), orc.round_bf16(dq))


def test_bench_self_launch_command():
    """`python bench.py --gpus N` (N > 1) without a launcher re-executes itself under torch.distributed.run with one rank per
    GPU and a 127.0.0.1 rendezvous; under a launcher (WORLD_SIZE set) or with N = 1 it does nothing."""
    import argparse
    import os
    import sys
    import bench
    cmd = bench.self_launch_command(4, ["--gpus", "4", "--steps", "3"], 29517)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29517"
    assert cmd[-5] == os.path.abspath(bench.__file__) and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    bench.maybe_self_launch(argparse.Namespace(gpus=1), [])  # N = 1: returns
    old = os.environ.get("WORLD_SIZE")
    os.environ["WORLD_SIZE"] = "4"
    try:
        bench.maybe_self_launch(argparse.Namespace(gpus=4), [])  # already under a launcher: returns
    finally:
        if old is None:
            del os.environ["WORLD_SIZE"]
        else:
            os.environ["WORLD_SIZE"] = old
    # no launcher and too few GPUs: refuses loudly instead of silently measuring one device (here: 0 GPUs visible)
    import pytest
    import torch
    if torch.cuda.device_count() < 4 and "WORLD_SIZE" not in os.environ:
        with pytest.raises(SystemExit) as e:
            bench.maybe_self_launch(argparse.Namespace(gpus=4), ["--gpus", "4"])
        assert "GPU(s) visible" in str(e.value)


def test_bench_live_traffic_declines_cleanly(monkeypatch, tmp_path):
    """bench.measure_traffic_live (roofline.traffic from two rocprofv3 --pmc child passes) never raises: under a profiler it
    declines (no nested counter passes), and a counter pass that fails — here a stand-in `rocprofv3` that exits 1 without
    writing a database — is reported as a note, so bench.py falls back to the committed summary."""
    import os
    import stat
    import bench
    monkeypatch.setenv("ROCPROFILER_TEST_MARKER", "1")
    val, note = bench.measure_traffic_live([])
    assert val is None and "profiler" in note
    monkeypatch.delenv("ROCPROFILER_TEST_MARKER")
    for k in [k for k in os.environ if k.startswith(("ROCPROF", "ROCP_TOOL"))]:
        monkeypatch.delenv(k)
    fake = tmp_path / "rocprofv3"
    fake.write_text("#!/bin/sh\nexit 1\n")
    fake.chmod(fake.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", f"{tmp_path}:{os.environ['PATH']}")
    val, note = bench.measure_traffic_live([], timeout=30)
    assert val is None and "FETCH_SIZE" in note and "failed" in note


def test_build_id_ties_the_library_to_the_source_tree(tmp_path):
    """fmi_build_id() = sha256 of csrc/*, include/*.h, Makefile as compiled in; _lib.tree_build_id() recomputes it from the tree (what
    __graft_entry__.build() compares, so a stale prebuilt .so cannot pass the build check); `make print-build-id` is the third witness."""
    import shutil
    import subprocess
    lib = L.load()
    have = lib.fmi_build_id().decode()
    assert re.fullmatch(r"[0-9a-f]{16}", have)
    assert have == L.tree_build_id(ROOT), "libflux_mi355x.so was not built from the sources in this tree: run `make lib`"
    assert have == subprocess.check_output(["make", "-C", ROOT, "-s", "print-build-id"]).decode().strip()
    assert f'"build_id": "{have}"' in lib.fmi_device_info().decode() or "no device" in lib.fmi_device_info().decode()
    # any byte of any source moves it
    for sub in ("diffusion-rs_amd/csrc", "include"):
        shutil.copytree(os.path.join(ROOT, sub), tmp_path / sub)
    shutil.copy(os.path.join(ROOT, "Makefile"), tmp_path / "Makefile")
    assert L.tree_build_id(str(tmp_path)) == have
    with open(tmp_path / "diffusion-rs_amd" / "csrc" / "vae.hip", "a") as f:
        f.write("// edited\n")
    assert L.tree_build_id(str(tmp_path)) != have


def test_bench_as_rank_hook_is_validated():
    """bench.py --as-rank / --as-world (the hook that lets one GPU draw rank R's samples, tests/test_gpu_multi_device.py) only goes
    together, on one GPU, with R < N: anything else stops before touching a device."""
    import subprocess
    import sys
    for bad in (["--as-rank", "1"], ["--as-rank", "2", "--as-world", "2"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True, timeout=300,
                           env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
        assert r.returncode != 0 and "--as-rank" in r.stderr, r.stderr[-500:]


def test_bench_dump_outputs_writes_float32_within_the_limit(tmp_path):
    """bench.dump_outputs (--dump-outputs DIR): one DIR/<name>.npy per array, float32 (float64 kept), whole when the arrays fit the limit;
    above it a seeded sample of each array in proportion to its size — the same elements on every call, so two builds compare element for element."""
    import torch
    import bench
    img = torch.arange(2 * 3 * 8 * 8, dtype=torch.uint8).reshape(2, 3, 8, 8)
    lat = torch.linspace(-1, 1, 4 * 64, dtype=torch.bfloat16).reshape(1, 4, 64)
    f64 = np.linspace(0, 1, 10)
    bench.dump_outputs(str(tmp_path / "all"), {"image": img, "latents": lat, "x": f64})
    got = {n: np.load(tmp_path / "all" / f"{n}.npy") for n in ("image", "latents", "x")}
    assert got["image"].dtype == np.float32 and got["latents"].dtype == np.float32 and got["x"].dtype == np.float64
    np.testing.assert_array_equal(got["image"], img.numpy().astype(np.float32))
    np.testing.assert_array_equal(got["latents"], lat.float().numpy())
    np.testing.assert_array_equal(got["x"], f64)
    big = np.arange(100_000, dtype=np.float32)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"big": big, "small": big[:1000]}, limit=40_000)
    a, b = (np.load(tmp_path / r / "big.npy") for r in ("a", "b"))
    small = np.load(tmp_path / "a" / "small.npy")
    assert a.nbytes + small.nbytes <= 40_000 and a.size > 0 and small.size > 0
    np.testing.assert_array_equal(a, b)
    assert np.all(np.diff(a) > 0) and set(a.tolist()) <= set(big.tolist())  # sorted distinct elements of the array
    assert bench.DUMP_LIMIT_BYTES == 64 * 2**20


def test_golden_files_are_small_and_the_split_fixtures_load():
    """Every committed fixture stays under 1 MiB; the full-size trajectory fixtures are byte pieces (<tag>_trajectory.npz.00, .01, ...) that
    tests/util.load_split_npz joins into the .npz that tests/test_gpu_c2_fixture.py reads."""
    from tests.util import load_split_npz
    golden = os.path.join(ROOT, "tests", "golden")
    for name in os.listdir(golden):
        path = os.path.join(golden, name)
        assert not os.path.isfile(path) or os.path.getsize(path) < 2**20, name
    for tag, n_img in (("c2", 4096), ("c5", 3600), ("o2", 4096)):
        z = load_split_npz(os.path.join(golden, f"{tag}_trajectory.npz"))
        assert z is not None, tag
        assert sorted(z.files) == ["lat_10", "lat_25", "lat_50", "meta", "step_s", "ts", "u8"]
        assert z["lat_50"].shape == (1, n_img, 64) and z["ts"].shape == (51,)
        meta = json.loads(bytes(z["meta"]).decode())
        assert meta["marks"] == [10, 25, 50] and zlib.crc32(z["u8"].tobytes()) == meta["image_crc32"]


def test_committed_attention_streams_are_what_their_generators_emit(tmp_path):
    """The seven generated instruction streams under csrc/ (`*_loop.inc`: the hand-scheduled KV loops of the attention kernels) are committed
    files; each must be byte for byte what its generator in tools/ emits — a stream edited by hand, or a generator changed without
    regenerating, would otherwise ship unnoticed (the generators also assert their own invariants — rule 3, read order, wait counts — while
    they run).  The generators write relative to their own location, so they run from a scratch copy of tools/."""
    import shutil
    import subprocess
    import sys
    (tmp_path / "tools").mkdir()
    (tmp_path / "diffusion-rs_amd" / "csrc").mkdir(parents=True)
    jobs = [("gen_attention_w4_loop.py", {}, "attention_w4_loop.inc"), ("gen_attention_w16.py", {}, "attention_w16_loop.inc"),
            ("gen_attention_w16.py", {"AW16_MODE": "fp8qk"}, "attention_w16f8_loop.inc"), ("gen_attention_w32.py", {}, "attention_w32_loop.inc"),
            ("gen_attention_w16l.py", {}, "attention_w16l_loop.inc"), ("gen_attention_w16l.py", {"AW16L_MODE": "fp8qk"}, "attention_w16lf8_loop.inc"),
            ("gen_attention_w16l.py", {"AW16L_MODE": "fp8pv"}, "attention_w16lf8pv_loop.inc")]
    shutil.copy(os.path.join(ROOT, "tools", "attn_stream.py"), tmp_path / "tools" / "attn_stream.py")  # what the generators import
    for gen, env, out in jobs:
        shutil.copy(os.path.join(ROOT, "tools", gen), tmp_path / "tools" / gen)
        clean = {k: v for k, v in os.environ.items() if not k.startswith(("AW16", "AW32", "AW4"))}
        r = subprocess.run([sys.executable, str(tmp_path / "tools" / gen)], env=dict(clean, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (gen, r.stderr[-1000:])
        made = (tmp_path / "diffusion-rs_amd" / "csrc" / out).read_bytes()
        have = open(os.path.join(ROOT, "diffusion-rs_amd", "csrc", out), "rb").read()
        assert made == have, f"{out} differs from what tools/{gen} {env or ''} emits: regenerate it (make) or revert the edit"


def test_no_entry_point_of_the_op_seam_synchronises_or_allocates_in_source():
    """`grep -n hipStreamSynchronize capi.hip` shows only fmi_stream_synchronize (VERDICT r4 'Done' criterion); the bodies of the op-level entry
    points (everything from the workspace-size queries to the attention-kernel switch) call no allocator and no synchronisation at all —
    the one hipMalloc besides fmi_malloc sits in the grow-only scratch cache, reached only when a stream's block is outgrown."""
    import re
    src = open(os.path.join(ROOT, "diffusion-rs_amd", "csrc", "capi.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert len(re.findall(r"\bhipStreamSynchronize\s*\(", code)) == 1
    # the one hipDeviceSynchronize is fmi_release_scratch's (ABI 6: blocks go back to the driver only behind a drained device), in front of the op entries
    assert code.count("hipDeviceSynchronize") == 1 and code.index("hipDeviceSynchronize") < code.index('extern "C" size_t fmi_linear_q8_workspace_bytes')
    assert len(re.findall(r"\bhipMalloc\s*\(", code)) == 2
    ops = code[code.index('extern "C" size_t fmi_linear_q8_workspace_bytes'):code.index('extern "C" int fmi_set_attention_kernel')]
    for banned in ("hipMalloc", "hipFree", "Synchronize", "hipMemcpy("):
        assert banned not in ops, banned


def test_design_status_table_is_generated():
    """DESIGN.md section 0's status table is the output of tools/status_table.py on the round's committed bench line (generated, not typed)."""
    import subprocess
    import sys
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import status_table as st
    a, b = design.index(st.BEGIN), design.index(st.END) + len(st.END)
    block = design[a:b]
    src = block.split("Source: `")[1].split("`")[0]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "status_table.py"), os.path.join(ROOT, src)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stdout.strip() == block.strip(), "DESIGN.md's status block differs from tools/status_table.py's output: run `python tools/status_table.py --write <bench json>`"


def test_outlier_profile_is_deterministic_and_the_same_on_numpy_and_torch():
    """synth.apply_outlier_profile (the off-Gaussian stress checkpoint of tests/test_gpu_outlier_stats.py): fixed channels and amplitudes, the same edit whether
    the tensor is a numpy array (oracle side of the small-config test) or a torch tensor (device side), and untouched tensors stay untouched."""
    import torch
    S = d.synth
    D = 3072
    out, amp, res = S.outlier_channels(D)
    assert (out, res) == S.outlier_channels(D)[::2] and len(out) == 12 and len(set(out) | set(res)) == 14
    assert sorted(abs(a) for a in amp)[0] >= 30 and sorted(abs(a) for a in amp)[-1] <= 100 and any(a < 0 for a in amp) and any(a > 0 for a in amp)
    rng = np.random.default_rng(0)
    cases = {"transformer_blocks.3.norm1.linear.bias": (6 * D,), "single_transformer_blocks.9.norm.linear.bias": (3 * D,), "transformer_blocks.0.attn.to_q.weight": (64, D),
             "single_transformer_blocks.1.proj_mlp.weight": (32, D), "x_embedder.bias": (D,), "transformer_blocks.2.attn.norm_added_k.weight": (128,),
             "transformer_blocks.0.ff.net.2.weight": (16, 4 * D), "proj_out.weight": (64, D), "transformer_blocks.3.norm1.linear.weight": (12, D)}
    for name, shape in cases.items():
        a = rng.standard_normal(shape).astype(np.float32)
        n = S.apply_outlier_profile(name, a.copy(), D)
        t = S.apply_outlier_profile(name, torch.from_numpy(a.copy()), D).numpy()
        np.testing.assert_array_equal(n, t)
        touched = not np.array_equal(n, a)
        assert touched == (name not in ("transformer_blocks.0.ff.net.2.weight", "proj_out.weight", "transformer_blocks.3.norm1.linear.weight")), name
    b = S.apply_outlier_profile("transformer_blocks.3.norm1.linear.bias", np.zeros(6 * D, np.float32), D)
    assert sorted(np.nonzero(b)[0].tolist()) == sorted([D + c for c in out] + [4 * D + c for c in out])  # the SCALE rows of (shift, scale, gate) x 2
    q = S.apply_outlier_profile("transformer_blocks.0.attn.norm_q.weight", np.ones(128, np.float32), D)
    assert q[[5, 77, 100]].tolist() == [3.0, 3.0, 3.0] and q.sum() == 128 + 6
