#!/usr/bin/env python
"""Tooling: the accuracy of dueling_dlog (csrc/irbpp_dueling_loss.hip), measured on its numpy restatement
(tests/test_dueling_loss_cpu.py, bit-equal to the kernel's) against numpy's float64 log over EVERY float32 argument in
[1, 128]: 58,720,257 arguments, under a minute on one CPU core, no GPU.  Prints one JSON line;
profiles/dueling_loss/dlog_sweep.json keeps it.

    python tools/dlog_sweep.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from test_dueling_loss_cpu import dlog_errors, dlog_np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    a = ap.parse_args()
    first = int(np.array([1.0], dtype=np.float32).view(np.uint32)[0])
    last = int(np.array([128.0], dtype=np.float32).view(np.uint32)[0])
    worst_abs, abs_at, worst_ulp, ulp_at, count, low, not_finite = 0.0, 0.0, 0.0, 0.0, 0, np.inf, 0
    for lo in range(first, last + 1, a.chunk):
        d = np.arange(lo, min(lo + a.chunk, last + 1), dtype=np.int64).astype(np.uint32).view(np.float32)
        err, ulp = dlog_errors(d)
        i, j = int(err.argmax()), int(ulp.argmax())
        if err[i] > worst_abs:
            worst_abs, abs_at = float(err[i]), float(d[i])
        if ulp[j] > worst_ulp:
            worst_ulp, ulp_at = float(ulp[j]), float(d[j])
        out = dlog_np(d)
        low = min(low, float(out.min()))
        not_finite += int((~np.isfinite(out)).sum())
        count += len(d)
    res = {"arguments": count, "from": 1.0, "to": 128.0, "max_abs": worst_abs, "max_abs_at": abs_at, "max_ulp": worst_ulp,
           "max_ulp_at": ulp_at, "min_result": low, "not_finite": not_finite, "at_one": float(dlog_np(np.float32(1.0))),
           "reference": "numpy float64 log"}
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
