#!/usr/bin/env python
"""Tooling: the accuracy of dueling_dexp (csrc/irbpp_dueling.hip), measured on its numpy restatement (tests/test_dueling_cpu.py,
bit-equal to the kernel's) against numpy's float64 exp over EVERY float32 argument from the cut-off -80 to -0.0: 1.12e9
arguments, a few minutes on one CPU core, no GPU.  Prints one JSON line; profiles/dueling_head/dexp_sweep.json keeps it.

    python tools/dexp_sweep.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from test_dueling_cpu import DEXP_CUT, dexp_np, ulp_error  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--chunk", type=int, default=1 << 24)
    a = ap.parse_args()
    first = int(np.array([-0.0], dtype=np.float32).view(np.uint32)[0])
    last = int(np.array([DEXP_CUT], dtype=np.float32).view(np.uint32)[0])          # bit patterns ascend as the value descends
    worst, worst_t, count, above_one = 0.0, 0.0, 0, 0
    for lo in range(first, last + 1, a.chunk):
        t = np.arange(lo, min(lo + a.chunk, last + 1), dtype=np.int64).astype(np.uint32).view(np.float32)
        err = ulp_error(t)
        i = int(err.argmax())
        if err[i] > worst:
            worst, worst_t = float(err[i]), float(t[i])
        above_one += int((dexp_np(t) > 1.0).sum())
        count += len(t)
    below = np.nextafter(DEXP_CUT, np.float32(-np.inf))
    out = {"arguments": count, "from": float(DEXP_CUT), "to": -0.0, "max_ulp": worst, "max_ulp_at": worst_t,
           "results_above_one": above_one, "below_cut_off": float(dexp_np(below)), "reference": "numpy float64 exp"}
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
