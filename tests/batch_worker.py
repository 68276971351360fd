"""Batch cases on the device in a process of their own: a batch reads
LPG_BATCH_TIER / LPG_BATCH_CHUNK when it is created, so the tests/test_gpu_batch*.py
run the other tier and the small chunks here.

    python batch_worker.py CASES SPECS.json OUT.npz

CASES: the module the specs belong to (batch_cases, batch2_cases,
batch3_cases, tie_cases, ...); SPECS.json: a list of its specs; OUT.npz: its run_batch's arrays
of case i under the prefix "i/".
"""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main(cases_name, specs_path, out_path):
    cases = importlib.import_module(cases_name)
    with open(specs_path) as f:
        specs = json.load(f)
    out = {}
    for i, s in enumerate(specs):
        for key, val in cases.run_batch(s).items():
            out[f"{i}/{key}"] = val
    np.savez(out_path, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3]))
