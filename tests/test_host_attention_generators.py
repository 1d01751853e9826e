"""CPU-only: every ablation and tuning knob of the three attention stream generators (tools/gen_attention_w16.py, _w32.py, _w16l.py) emits
byte for byte what it emitted when tests/golden/attention_stream_variants.json was recorded, and the settings that violate a scheduler
invariant still die on the assertion that names it.  The seven default streams are pinned against the committed `.inc` files by
test_host_logic.py; this pins what `AW16_X`, `AW32_X`, `AW16L_X`, the `*_LOOKAHEAD`s and w16l's placement knobs produce — every number in
profiles/r03 .. r05_attention_*.txt was measured on such a variant.

`python tests/test_host_attention_generators.py --record [--tools DIR]` rewrites the fixture from the generators in DIR (default: this
tree's tools/).  A change to the generators that is meant to leave their output alone is checked against a fixture recorded BEFORE it."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "attention_stream_variants.json")
SHARED = "attn_stream.py"  # the module the three generators import (copied next to them when it exists)


def _cases():
    """[(generator, env, name of the env variable that takes a dump path | None)]"""
    out = []
    for mode in ("bf16", "fp8qk"):
        m = {"AW16_MODE": mode}
        for x in ("novalu", "noexp", "nodma", "nobarrier", "halfreads", "nomfma", "nowait", "halfpv", "nopv", "drop_v_exp+v_cvt"):
            out.append(("gen_attention_w16.py", dict(m, AW16_X=x), None))
        for la in (8, 10) + ((14, 16) if mode == "fp8qk" else ()):
            out.append(("gen_attention_w16.py", dict(m, AW16_X=f"la{la}", AW16_LOOKAHEAD=str(la)), None))
        out.append(("gen_attention_w16.py", m, "AW16_DUMP"))
    for x in ("novalu", "noexp", "nodma", "nobarrier", "halfreads", "nomfma", "nowait", "drop_v_exp"):
        out.append(("gen_attention_w32.py", {"AW32_X": x}, None))
    for la in (4, 5, 7):
        out.append(("gen_attention_w32.py", {"AW32_X": f"la{la}", "AW32_LOOKAHEAD": str(la)}, None))
    out.append(("gen_attention_w32.py", {}, "AW32_DUMP"))
    for mode in ("bf16", "fp8qk", "fp8pv"):
        m = {"AW16L_MODE": mode}
        for x in ("novalu", "noexp", "nodma", "nobarrier", "nomfma", "nowait", "nolds", "nosetup", "halftree", "drop:v_exp+v_cvt"):
            out.append(("gen_attention_w16l.py", dict(m, AW16L_X=x), None))
        out.append(("gen_attention_w16l.py", dict(m, AW16L_TAG="t", AW16L_LOOKAHEAD="12"), None))
        out.append(("gen_attention_w16l.py", dict(m, AW16L_TAG="t", AW16L_OOL="1"), None))
        out.append(("gen_attention_w16l.py", dict(m, AW16L_TAG="ool", AW16L_OOL="1", AW16L_X="novalu/nodma"), None))
        knobs = {"bf16": ("AW16L_EY=10", "AW16L_TREE_END=17", "AW16L_LOOKAHEAD=20"), "fp8qk": ("AW16L_F8_EX=5",),
                 "fp8pv": ("AW16L_F8_EX=5", "AW16L_CVT_GRP=2", "AW16L_PV8_TREE_END=2", "AW16L_LOOKAHEAD=20")}[mode]
        for kv in knobs:
            out.append(("gen_attention_w16l.py", dict(m, **dict([kv.split("=")])), None))
        out.append(("gen_attention_w16l.py", m, "AW16L_DUMP"))
    return out


# settings that break a scheduler invariant: the generator must exit non-zero on the AssertionError that names it
MUST_FAIL = [("gen_attention_w16.py", {"AW16_MODE": "bf16", "AW16_LOOKAHEAD": "14"}, "'rule 3'"),
             ("gen_attention_w16.py", {"AW16_MODE": "bf16", "AW16_LOOKAHEAD": "16"}, "'rule 3'"),
             ("gen_attention_w32.py", {"AW32_LOOKAHEAD": "8"}, "'rule 3'"),
             ("gen_attention_w16l.py", {"AW16L_MODE": "fp8qk", "AW16L_LOOKAHEAD": "20"}, "next phase's reads must follow the own ones")]

# first 16 hex digits of the sha256 of seven outputs of the generators the fixture was first recorded from: {file name: digest}
ANCHORS = {"attention_w16_loop_novalu.inc": "4d223dc6573fce0f", "attention_w16f8_loop_la16.inc": "b5184fb56e410fcb",
           "attention_w32_loop_la7.inc": "ca23bb21c717438c", "attention_w16l_loop_halftree.inc": "c24af418a1a34028",
           "attention_w16lf8_loop_nosetup.inc": "d633e78b10dd8dd3", "attention_w16lf8pv_loop_nolds.inc": "7844acae486fe073",
           "attention_w16lf8pv_loop_ool.inc": "c6917fba35e813a3"}


def _case_id(gen, env, dump):
    return " ".join([gen] + [f"{k}={v}" for k, v in sorted(env.items())] + ([dump] if dump else []))


def _run(tools, scratch, gen, env, dump=None):
    """run one generator from a scratch copy of tools/ (it writes relative to its own location); -> (CompletedProcess, scratch root)"""
    root = tempfile.mkdtemp(dir=scratch)
    os.makedirs(os.path.join(root, "tools"))
    os.makedirs(os.path.join(root, "diffusion-rs_amd", "csrc"))
    for name in (gen, SHARED):
        if os.path.exists(os.path.join(tools, name)):
            shutil.copy(os.path.join(tools, name), os.path.join(root, "tools", name))
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("AW16", "AW32", "AW4"))}
    if dump:
        env = dict(env, **{dump: os.path.join(root, "dump.txt")})
    return subprocess.run([sys.executable, os.path.join(root, "tools", gen)], env=dict(clean, **env), capture_output=True, text=True, timeout=300), root


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def _emit(tools, scratch, case):
    gen, env, dump = case
    r, root = _run(tools, scratch, gen, env, dump)
    assert r.returncode == 0, (_case_id(*case), r.stderr[-1000:])
    made = [os.path.join(d, f) for d in ("build", os.path.join("diffusion-rs_amd", "csrc")) if os.path.isdir(os.path.join(root, d))
            for f in sorted(os.listdir(os.path.join(root, d))) if f.endswith(".inc")]
    assert len(made) == 1, (_case_id(*case), made)
    rec = {"inc": os.path.basename(made[0]), "sha256": _sha(os.path.join(root, made[0]))}
    if dump:
        rec["dump_sha256"] = _sha(os.path.join(root, "dump.txt"))
    shutil.rmtree(root)
    return rec


def _emit_all(tools, scratch):
    cases = _cases()
    with ThreadPoolExecutor(4) as pool:
        recs = list(pool.map(lambda c: _emit(tools, scratch, c), cases))
    return {_case_id(*c): r for c, r in zip(cases, recs)}


def test_every_generator_variant_emits_what_the_fixture_records(tmp_path):
    want = json.load(open(FIXTURE))
    have = _emit_all(os.path.join(ROOT, "tools"), str(tmp_path))
    assert sorted(have) == sorted(want), "the case list and the fixture differ: " + str(sorted(set(have) ^ set(want)))
    differ = [cid for cid in sorted(want) if have[cid] != want[cid]]
    assert not differ, f"{len(differ)} of {len(want)} generator outputs differ from the recorded ones: {differ}"


def test_fixture_holds_the_anchor_digests():
    by_file = {}
    for rec in json.load(open(FIXTURE)).values():
        by_file.setdefault(rec["inc"], set()).add(rec["sha256"][:16])
    for name, digest in ANCHORS.items():
        assert digest in by_file.get(name, ()), (name, digest, by_file.get(name))


def test_settings_that_break_an_invariant_still_fail_on_it(tmp_path):
    for gen, env, invariant in MUST_FAIL:
        r, _ = _run(os.path.join(ROOT, "tools"), str(tmp_path), gen, env)
        assert r.returncode != 0, (gen, env)
        assert "AssertionError" in r.stderr and invariant in r.stderr, (gen, env, r.stderr[-600:])


if __name__ == "__main__":
    assert "--record" in sys.argv[1:], __doc__
    src = sys.argv[sys.argv.index("--tools") + 1] if "--tools" in sys.argv else os.path.join(ROOT, "tools")
    with tempfile.TemporaryDirectory() as tmp:
        recorded = _emit_all(os.path.abspath(src), tmp)
    with open(FIXTURE, "w") as out:
        json.dump(recorded, out, indent=1, sort_keys=True)
        out.write("\n")
    print(f"{FIXTURE}: {len(recorded)} cases from {src}")
