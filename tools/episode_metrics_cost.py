"""What the device-side episode metrics cost the acting loop: bench.actor_loop_rate's loop (environment step + MINZ policy +
VectorReplayMemory append, all on the device) at 4096 and 8192 BlockOut bins, without and with an EpisodeMetrics window
(W = 10, read every 100 steps), alternated A/B/A/B.  Prints one JSON line.  The update kernel's own duration comes from a
kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/episode_metrics_cost.py --steps 300
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from irbpp_amd.metrics import EpisodeMetrics  # noqa: E402
from irbpp_amd.replay import VectorReplayMemory, actor_step  # noqa: E402
from irbpp_amd.vec_env import GpuPackingEnv  # noqa: E402


def loop_rate(bins, dev, steps, with_metrics, capacity=64, read_every=100):
    shapes, seqs, kw = bench.make_workload("blockout")
    env = GpuPackingEnv(shapes, seqs, bins, device=dev, **kw)
    mem = VectorReplayMemory(bins, capacity, env.obs_len, device=dev)
    policy = lambda s_, m_: env.policy_minz(s_).to(torch.int64)      # noqa: E731
    metrics = EpisodeMetrics(env, window=10, history=1024) if with_metrics else None
    state = env.reset()
    for _ in range(capacity + 8):
        state, _, _ = actor_step(env, policy, mem, state)
    if metrics is not None:
        metrics.read()
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    rows = 0
    for i in range(1, steps + 1):
        state, _, _ = actor_step(env, policy, mem, state)
        if metrics is not None and i % read_every == 0:
            rows += metrics.read().shape[0]
    if metrics is not None:
        rows += metrics.read().shape[0]
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t
    env.check_device_error()
    if metrics is not None:
        metrics.close()
    env.close()
    return bins * steps / dt, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bins", type=int, nargs="+", default=[4096, 8192])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"unit": "placement-steps/s", "steps": a.steps, "window": 10, "read_every": 100, "sizes": {}}
    for bins in a.bins:
        base, win = [], []
        for _ in range(a.rounds):
            base.append(loop_rate(bins, dev, a.steps, False)[0])
            r, rows = loop_rate(bins, dev, a.steps, True)
            win.append(r)
        b, w = sorted(base)[len(base) // 2], sorted(win)[len(win) // 2]
        out["sizes"][str(bins)] = {"without": b, "with_metrics": w, "loss_pct": 100.0 * (b - w) / b, "runs_without": base,
                                   "runs_with": win}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
