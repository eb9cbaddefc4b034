#!/usr/bin/env python3
"""Record tests/golden/tail_fused_parent_hashes.json: the sha256 of every result of tests/test_tail_fused_live_gpu.py, computed on
the GPU with the library that is in the tree.  Run it from a checkout of the commit whose bytes are to be pinned (build first), or
with that commit's libfcvsr_hip.so copied over fcvsr_amd/lib/ - never with the code under test.
usage: python scripts/record_tail_fused_hashes.py <recorded-from: commit id> [out.json]"""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (before the library: it must bind to torch's HIP runtime)
import test_tail_fused_live_gpu as T  # noqa: E402


def main(commit, out=T.GOLDEN):
    sha = {}
    for shape, dn, slope in T.GROUPS:
        sha.update(T.result_hashes(*shape, dn, slope))
    doc = {"what": "sha256 of the results of every entry point of tail_fused.hip on the problems of tests/test_tail_fused_live_gpu.py",
           "recorded_from": commit, "device": torch.cuda.get_device_name(0), "sha256": dict(sorted(sha.items()))}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(sha)} hashes ({len(set(sha.values()))} distinct) -> {out}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
