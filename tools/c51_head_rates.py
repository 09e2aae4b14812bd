#!/usr/bin/env python
"""Tooling: the distributional head around the network, the reference's torch lines against the HIP calls
(irbpp_categorical_act / irbpp_categorical_target through irbpp_amd.replay), in one process and interleaved.

    act     agent.py:54-58 on p [N, 500, 51] with the observation's mask, N in --envs (1024 4096)
    target  agent.py:91-115 on two [B, 500, 51] tensors, B in --batches (64 512)

Per shape and form: --repeats (3) timed windows of --iters calls between device events, taken in turns (torch, hip, torch,
hip, ...); the median and the spread (max - min) of the time per call, and for the act kernel the bytes per second of the
N x S x atoms x 4 bytes of p it must read (the call's time: launch included).  One GPU process; run it under a timeout.

    python tools/c51_head_rates.py [--out FILE.json]
    python tools/c51_head_rates.py --only hip --repeats 1      (for `rocprofv3 --kernel-trace --stats`: the kernels' own times)
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from irbpp_amd import replay  # noqa: E402

S, ATOMS, V_MIN, V_MAX, GAMMA_N = 500, 51, -1.0, 8.0, 0.99 ** 3


def act_torch(p, support, mask):
    sum_q_map = p * support
    sum_q_map = sum_q_map.sum(2)
    sum_q_map[(1 - mask).bool()] = -math.inf
    return sum_q_map.argmax(1)


def learn_torch(p_on, p_tg, returns, nonterminals, support):
    B, atoms = p_on.shape[0], p_on.shape[2]
    delta_z = (V_MAX - V_MIN) / (atoms - 1)
    a = (support.expand_as(p_on) * p_on).sum(2).argmax(1)
    pns_a = p_tg[range(B), a]
    Tz = returns.unsqueeze(1) + nonterminals * GAMMA_N * support.unsqueeze(0)
    Tz = Tz.clamp(min=V_MIN, max=V_MAX)
    b = (Tz - V_MIN) / delta_z
    l, u = b.floor().to(torch.int64), b.ceil().to(torch.int64)
    l[(u > 0) * (l == u)] -= 1
    u[(l < (atoms - 1)) * (l == u)] += 1
    m = p_tg.new_zeros(B, atoms)
    offset = torch.linspace(0, ((B - 1) * atoms), B).unsqueeze(1).expand(B, atoms).to(a)
    m.view(-1).index_add_(0, (l + offset).view(-1), (pns_a * (u.float() - b)).view(-1))
    m.view(-1).index_add_(0, (u + offset).view(-1), (pns_a * (b - l.float())).view(-1))
    return m, a


def window(fn, iters):
    """ms per call over `iters` calls between two device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def compare(forms, iters, repeats, warmup=3):
    times = {k: [] for k in forms}
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in forms.items():
            times[k].append(window(fn, iters))
    return {k: {"median_ms": statistics.median(v), "spread_ms": max(v) - min(v), "windows_ms": v} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--only", choices=["torch", "hip"], default=None)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("c51_head_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    support = torch.linspace(V_MIN, V_MAX, ATOMS, device=dev)
    pick = lambda d: {k: v for k, v in d.items() if a.only in (None, k)}        # noqa: E731
    out = {"S": S, "atoms": ATOMS, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "act": {}, "target": {}}
    for n in a.envs:
        p = torch.softmax(3 * torch.randn((n, S, ATOMS), device=dev, generator=gen), 2)
        state = torch.zeros((n, S * 5 + 7), device=dev)
        mask = (torch.rand((n, S), device=dev, generator=gen) < 0.7).float()
        state[:, :S * 5].view(n, S, 5)[:, :, 4] = mask
        r = compare(pick({"torch": lambda: act_torch(p, support, replay.mask_from_state(state, S)),
                          "hip": lambda: replay.distributional_greedy_action(p, support, state, S, use_hip=True)}), a.iters, a.repeats)
        nbytes = n * S * ATOMS * 4
        for v in r.values():
            v["p_bytes_per_s"] = nbytes / (v["median_ms"] * 1e-3)
        r["p_bytes"] = nbytes
        out["act"][str(n)] = r
        del p, state, mask
    for b in a.batches:
        p_on = torch.softmax(3 * torch.randn((b, S, ATOMS), device=dev, generator=gen), 2)
        p_tg = torch.softmax(3 * torch.randn((b, S, ATOMS), device=dev, generator=gen), 2)
        returns = torch.rand((b,), device=dev, generator=gen) * 11 - 2
        nonterm = (torch.rand((b, 1), device=dev, generator=gen) < 0.8).float()
        out["target"][str(b)] = compare(
            pick({"torch": lambda: learn_torch(p_on, p_tg, returns, nonterm, support),
                  "hip": lambda: replay.c51_target(p_on, p_tg, returns, nonterm, support, GAMMA_N, V_MIN, V_MAX, use_hip=True)}),
            a.iters * 5, a.repeats)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
