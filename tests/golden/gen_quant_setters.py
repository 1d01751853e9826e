#!/usr/bin/env python
"""Generates tests/golden/quant_setters.json: the (code, message) of every refusal of the four quantised-Linear setters and the outcome of every kind
transition, with tests/test_gpu_quant_setters.py's own walks (refusals(), transition()).  The committed file was written on the commit BEFORE the
setters were given one shared frame (that commit's library, this walk), which is what makes the test a before / after comparison: the commit that
reshaped them has to reproduce it.  Regenerate it only for a change that is meant to move a message or an outcome, or to add cases — then on the
commit BEFORE that change, with the extended walk copied in, and what is already there must come out as committed.
Needs the GPU: python tests/golden/gen_quant_setters.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_gpu_quant_setters as T  # noqa: E402

if __name__ == "__main__":
    h = T.make_handles()
    out = {"refusals": {s: T.refusals(h, s) for s in T.SETTERS}, "transitions": {}}
    for m in h.values():
        m.close()
    for case in T.CASES:
        out["transitions"][case] = T.transition(case)
        print(case, json.dumps(out["transitions"][case]), flush=True)
    with open(T.GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["refusals"], indent=1))
