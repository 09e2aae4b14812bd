#!/usr/bin/env python
"""Tooling: do the per-die lists of polygon rounds (State::w_round, Params::round_cap entries each) fill in practice?
Steps a bench.py workload as one environment under the scripted min-z policy and records, per step, the eight reservation
totals (GpuPackingEnv.debug_round_counts) against the cap: the largest per-die count, how many dies are over the cap, the sum.

    python tools/round_list_fill.py [--bins 4096] [--steps 30] [--workloads general blockout] [--out profiles/round_list/fill.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from irbpp_amd.vec_env import GpuPackingEnv  # noqa: E402


def measure(workload, bins, steps):
    shapes, seqs, kw = bench.make_workload(workload)
    env = GpuPackingEnv(shapes, seqs, bins, device="cuda:0", **kw)
    cap = (bins // 8 + 64) * 16
    env.debug_round_counts()                       # switches the recording on
    obs = env.reset()
    rows = []
    for t in range(steps + 1):
        c = env.debug_round_counts()
        rows.append(dict(step=t, max=int(c.max()), dies_over_cap=int((c > cap).sum()), sum=int(c.sum()), counts=c.tolist()))
        obs = env.step(env.policy_minz(obs))[0]
    env.check_device_error()
    env.close()
    return dict(workload=workload, bins=bins, round_cap=cap, steps=rows,
                largest=max(r["max"] for r in rows), observations_with_a_full_list=sum(r["dies_over_cap"] > 0 for r in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--workloads", nargs="+", default=["general", "blockout"])
    ap.add_argument("--out", default=os.path.join("profiles", "round_list", "fill.json"))
    a = ap.parse_args()
    res = [measure(w, a.bins, a.steps) for w in a.workloads]
    for r in res:
        print(f"{r['workload']}: cap {r['round_cap']}, largest per-die count {r['largest']}, "
              f"{r['observations_with_a_full_list']} of {len(r['steps'])} observations with a full list")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:                  # one line per step
        f.write("[\n" + ",\n".join(
            "{" + ", ".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in r.items() if k != "steps") + ', "steps": [\n  ' +
            ",\n  ".join(json.dumps(row) for row in r["steps"]) + "\n]}" for r in res) + "\n]\n")


if __name__ == "__main__":
    main()
