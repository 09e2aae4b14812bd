#!/usr/bin/env python
"""Tooling: what saving, loading and forking bins costs (irbpp_save_bins / irbpp_load_bins / irbpp_copy_bins).

    python tools/bin_state_rates.py [--bins 8192] [--repeats 3] [--out profiles/bin_state/bin_state_rates.json]

A BlockOut R = 4 environment of 2 * bins bins: the lower half is forked into the upper half, `bins` bins are saved and
loaded.  The three calls are timed in turn, `--repeats` times round (interleaved, so that a drift of the machine meets all
three alike), each timing HIP events around `--calls` calls; reported: median and spread (min .. max) of the time per call,
the bytes of a bin from the segment table (csrc/irbpp_binstate.h, asked of tests/host/binstate_host.cpp, which g++ compiles
here: a fork moves the segments marked in_fork), and the resulting bandwidth -- every byte is read once and written once --
against the MI355X's 8 TB/s HBM peak.  `save` is irbpp_save_bins into a blob allocated beforehand, the kernel alone like
`fork` and `load`; `save_wrapper` is GpuPackingEnv.save_bins, which allocates and zero-fills its blob tensor per call."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import irbpp_amd  # noqa: E402,F401
from irbpp_amd import _lib, build, synthetic  # noqa: E402
from irbpp_amd.vec_env import GpuPackingEnv, _ptr  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s


def segment_table(env):
    """[(name, row_bytes, bytes, offset, in_fork)] of the environment's geometry, from irbpp_binstate.h itself"""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "host")
    exe = os.path.join(root, "_build", "binstate_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "stub"), os.path.join(root, "binstate_host.cpp"), "-o", exe],
                   check=True)
    step = env.Hx // env.Ax
    wide = int(env.Ax > 16 or env.Ay > 16)
    out = subprocess.run([exe], input=f"table {env.Ax} {env.Ay} {step} {env.n_rot} {env.S} {env.K} {wide} 0\n", capture_output=True,
                         text=True, check=True).stdout.split("\n")
    n, total = (int(v) for v in out[0].split())
    segs = [(f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])) for f in (line.split() for line in out[1:1 + n])]
    assert total == env.bin_blob_info()["bytes_per_bin"], "the host build of the table and the library disagree"
    return segs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.bins
    sh = synthetic.blockout_shapes(n_shapes=64, n_rot=4, cube=0.06, seed=0)
    env = GpuPackingEnv(sh, synthetic.make_sequences(sh.n_shapes, 4096, 100, seed=5), 2 * n, device="cuda:0")
    obs = env.reset()
    for _ in range(5):
        obs, _, _ = env.step(env.policy_minz(obs))
    low = torch.arange(n, dtype=torch.int32, device=env.device)
    up = low + n
    segs = segment_table(env)
    whole, forked = sum(g[2] for g in segs), sum(g[2] for g in segs if g[4])
    per_bin = {"fork": forked, "save": whole, "load": whole, "save_wrapper": whole}
    blob = env.save_bins(low)
    into = torch.zeros_like(blob.data)

    def save_kernel():
        _lib.check(env.lib.irbpp_save_bins(env._h, _ptr(low), n, _ptr(into), env._stream()), "irbpp_save_bins")

    calls = {"fork": lambda: env.fork_bins(low, up, validate=False), "save": save_kernel, "load": lambda: env.load_bins(low, blob),
             "save_wrapper": lambda: env.save_bins(low)}
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.repeats):
        for name, f in calls.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                f()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.calls)
    env.check_device_error()
    res = {"bins": n, "repeats": a.repeats, "calls_per_timing": a.calls, "source_hash": build.source_hash(),
           "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "segments": [dict(zip(("array", "row_bytes", "bytes", "offset", "in_fork"), g)) for g in segs], "calls": {}}
    for name, ms in times.items():
        med = statistics.median(ms)
        moved = 2.0 * per_bin[name] * n
        res["calls"][name] = {"bytes_per_bin": per_bin[name], "ms_median": round(med, 5), "ms_min": round(min(ms), 5),
                              "ms_max": round(max(ms), 5), "bytes_moved": int(moved), "bytes_per_s": round(moved / (med * 1e-3)),
                              "fraction_of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 4)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    env.close()


if __name__ == "__main__":
    main()
