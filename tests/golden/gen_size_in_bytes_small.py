#!/usr/bin/env python
"""Generates tests/golden/size_in_bytes_small.json: size_in_bytes() after every step of tests/test_gpu_memory_lifecycle.py's lifecycle().  The committed
file was written on the commit BEFORE the handles' device blocks became DeviceBuffer members (that commit's library, this walk), which is what makes the
test a before / after comparison; regenerate it only for a change that is meant to move the accounting, or to add steps to the walk — then on the commit
BEFORE the change the new steps are there to pin, with the extended walk copied in, and the integers of the existing steps must come out as committed (steps
8 and 9, the vision towers and the Redux embedder, were added that way).  Needs the GPU: python tests/golden/gen_size_in_bytes_small.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.test_gpu_memory_lifecycle import GOLDEN, lifecycle  # noqa: E402

if __name__ == "__main__":
    sizes = lifecycle()
    with open(GOLDEN, "w") as f:
        json.dump(sizes, f, indent=1)
        f.write("\n")
    print(json.dumps(sizes, indent=1))
