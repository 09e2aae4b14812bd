#!/usr/bin/env python
"""Tooling: placement-steps/s of a device-resident heuristic roll-out (``heuristic_step`` with MINZ; ``heuristic_action`` +
``step_cells`` beside it) and of the candidate-row roll-out bench.py times (the
scripted MINZ policy fused into the observation + ``step``), same build, same process, same shape of timed region: one
group, registered ping-pong observation buffers, prefill + warm-up, a block of steps between two synchronisations.

    python tools/heuristic_step_rates.py [--bins 1024 4096 8192] [--steps 200] [--out FILE.json]
    python tools/heuristic_step_rates.py --loop heuristic --bins 8192 --steps 50      (one loop only: for a kernel trace)

Kernel times come from running the second form under ``rocprofv3 --kernel-trace --stats``.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench import make_workload  # noqa: E402
from irbpp_amd import _lib  # noqa: E402
from irbpp_amd.vec_env import GpuPackingEnv  # noqa: E402


def rate(loop, bins, steps, prefill, warmup, dev="cuda:0"):
    shapes, seqs, kw = make_workload("blockout")[:3]
    tuning = _lib.TUNE_SPLIT_APPLY if loop == "candidates_split" else 0
    env = GpuPackingEnv(shapes, seqs, bins, device=dev, tuning=tuning, **kw)
    cur = env.reset()
    nxt = torch.empty_like(cur)
    act = torch.empty((bins,), dtype=torch.int32, device=dev)
    env.policy_minz(cur, actions_out=act)
    if loop.startswith("candidates"):
        env.set_auto_policy(act)
    env.register_obs_buffer(cur)
    env.register_obs_buffer(nxt)

    def one_step():
        nonlocal cur, nxt
        if loop.startswith("candidates"):
            env.step(act, obs_out=nxt)
        elif loop == "scorer_then_cells":       # the parent's scorer (irbpp_heuristic_kernel recomputes the overlap test), then the cell step
            env.step_cells(env.heuristic_action("MINZ", 0), obs_out=nxt)
        else:
            env.heuristic_step("MINZ", 0, obs_out=nxt)
        cur, nxt = nxt, cur

    for _ in range(prefill + warmup):
        one_step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        one_step()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    env.check_device_error()
    episodes = float(env.episode_totals()[0].item())
    env.close()
    return {"loop": loop, "bins": bins, "steps": steps, "steps_per_s": bins * steps / dt, "us_per_step": 1e6 * dt / steps,
            "episodes_finished": episodes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, nargs="+", default=[1024, 4096, 8192])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--prefill", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop", default=None, choices=["candidates", "candidates_split", "heuristic", "scorer_then_cells"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    loops = [a.loop] if a.loop else ["candidates", "candidates_split", "heuristic", "scorer_then_cells"]
    rows = []
    for bins in a.bins:
        for rep in range(1 if a.loop else a.repeats):          # interleaved repeats: drift hits every loop alike
            for loop in loops:
                r = rate(loop, bins, a.steps, a.prefill, a.warmup)
                r["repeat"] = rep
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
