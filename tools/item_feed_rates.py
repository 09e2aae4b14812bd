#!/usr/bin/env python
"""Tooling: what the item supply costs the training-time stepping loop.  BlockOut (R = 4, k = 1) through
``make_vec_envs`` with the actions chosen on the device (``policy_minz`` on the observation tensor), fed three ways:

    host    args.item_feed absent: itemgen.StreamFeeder (cursor read-back, draws on one host core, upload)
    device  args.item_feed = "device": itemgen.DeviceStreamFeeder (irbpp_stream_refill, no host involvement)
    table   args.sequences: a plain sequence table, no feeder at all -- the ceiling

in one process, interleaved, ``--repeats`` times each per ring length; per feed the median and the spread (max - min) of
the step rate, and the construction time of the environments (make_vec_envs until the device is idle).

    python tools/item_feed_rates.py [--envs 4096] [--rings 4096 256] [--steps 3072] [--repeats 3] [--out FILE.json]
    python tools/item_feed_rates.py --feed device --rings 256 --steps 512 --repeats 1      (one loop: for a kernel trace)

The refill kernel's time comes from running the second form under ``rocprofv3 --kernel-trace --stats``.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench import make_workload  # noqa: E402
from irbpp_amd.vec_env import make_vec_envs  # noqa: E402


def run(feed, envs_n, ring, steps, warmup, dev=0):
    shapes, seqs, kw = make_workload("blockout")
    dic = {i: "family%02d_%d.obj" % (i % 16, i // 16) for i in range(shapes.n_shapes)}      # 16 names of 4 instances each
    args = types.SimpleNamespace(
        num_processes=envs_n, device=dev, seed=0, shapes=shapes, dicPath=dic, dataSample="instance",
        resolutionA=kw["resolutionA"], resolutionH=kw["resolutionH"], selectedAction=500, bufferSize=1,
        evaluate=False, item_ring=ring, obs_ring=3)
    if feed == "table":
        args.sequences = seqs
    elif feed == "device":
        args.item_feed = "device"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    envs, _, _ = make_vec_envs(args, None, True)
    torch.cuda.synchronize()
    construct = time.perf_counter() - t0
    obs = envs.reset()
    for _ in range(warmup):
        obs = envs.step(envs.env.policy_minz(obs))[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        obs = envs.step(envs.env.policy_minz(obs))[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    envs.env.check_device_error()
    refills = steps // envs.feeder.every if envs.feeder is not None else 0
    envs.close()
    return {"feed": feed, "envs": envs_n, "ring": ring, "steps": steps, "steps_per_s": envs_n * steps / dt,
            "us_per_step": 1e6 * dt / steps, "construct_s": construct, "refills_timed": refills}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rings", type=int, nargs="+", default=[4096, 256])
    ap.add_argument("--steps", type=int, default=3072)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--feed", default=None, choices=["host", "device", "table"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    feeds = [a.feed] if a.feed else ["host", "device", "table"]
    rows, summary = [], []
    for ring in a.rings:
        for rep in range(a.repeats):                       # interleaved repeats: drift hits every feed alike
            for feed in feeds:
                r = run(feed, a.envs, ring, a.steps, a.warmup)
                r["repeat"] = rep
                rows.append(r)
                print(json.dumps(r), flush=True)
        for feed in feeds:
            mine = [r for r in rows if r["ring"] == ring and r["feed"] == feed]
            rates = [r["steps_per_s"] for r in mine]
            s = {"summary": feed, "envs": a.envs, "ring": ring, "median_steps_per_s": statistics.median(rates),
                 "spread_steps_per_s": max(rates) - min(rates),
                 "median_construct_s": statistics.median(r["construct_s"] for r in mine)}
            summary.append(s)
            print(json.dumps(s), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"runs": rows, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
