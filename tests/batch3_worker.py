"""Big-M batch cases on the device in a process of their own: the batch reads
LPG_BATCH_TIER / LPG_BATCH_CHUNK when it is created, so
tests/test_gpu_batch_big_m.py runs the other tier and the small chunks here.

    python batch3_worker.py SPECS.json OUT.npz

SPECS.json: a list of batch3_cases specs; OUT.npz: run_batch's arrays of case
i under the prefix "i/".
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import batch3_cases  # noqa: E402


def main(specs_path, out_path):
    with open(specs_path) as f:
        specs = json.load(f)
    out = {}
    for i, s in enumerate(specs):
        for key, val in batch3_cases.run_batch(s).items():
            out[f"{i}/{key}"] = val
    np.savez(out_path, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
