#!/usr/bin/env python
"""Tooling: what one pooled learning batch costs (VectorReplayMemory.sample_pooled / update_priorities_pooled).

    python tools/pooled_sample_rates.py [--envs 4096] [--capacity 64] [--obs-len 2500] [--repeats 3] [--out FILE.json]

`--envs` memories filled by appends, then for B = 64 and 256: sample_pooled (the sample launch, the read of the failure flag,
the gather launch) and update_priorities_pooled (one launch), timed in turn `--repeats` times round, each timing HIP events
around `--calls` calls; reported: median and spread (min .. max) of the time per call.  The sample's time includes its one
host round trip.  Nothing in the project rests on these numbers."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import irbpp_amd  # noqa: E402,F401
from irbpp_amd import build  # noqa: E402
from irbpp_amd.replay import VectorReplayMemory  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--obs-len", type=int, default=2500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.envs
    mem = VectorReplayMemory(n, a.capacity, a.obs_len, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for _ in range(a.capacity + 3):
        mem.append(torch.rand(n, a.obs_len, device=dev, generator=g), torch.zeros(n, dtype=torch.int64, device=dev),
                   torch.rand(n, device=dev, generator=g), torch.rand(n, device=dev, generator=g) < 0.05)
    draw = torch.Generator().manual_seed(1)
    res = {"envs": n, "capacity": a.capacity, "obs_len": a.obs_len, "repeats": a.repeats, "calls_per_timing": a.calls,
           "source_hash": build.source_hash(), "device": torch.cuda.get_device_name(0), "batches": {}}
    for b in (64, 256):
        batch = mem.sample_pooled(b, generator=draw)
        loss = torch.rand(b, device=dev, generator=g) + 0.1
        calls = {"sample_pooled": lambda: mem.sample_pooled(b, generator=draw),
                 "update_priorities_pooled": lambda: mem.update_priorities_pooled(batch[0], loss)}
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
        res["batches"][str(b)] = {name: {"ms_median": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5),
                                         "ms_max": round(max(ms), 5)} for name, ms in times.items()}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
