#!/usr/bin/env python
"""Tooling: the head from the network's logits, three forms in one process, interleaved (the manner of c51_head_rates.py):

    torch        model.py:395-400 (combine + softmax) followed by the reference's torch lines (agent.py:54-58 / 91-115)
    torch+c51    the same combine + softmax followed by the categorical kernels (replay.distributional_greedy_action /
                 replay.c51_target with use_hip=True)
    dueling      the fused kernels (replay.dueling_greedy_action / replay.dueling_c51_target with use_hip=True)

    act     v [N, 31], a [N, 500, 31] with the observation's mask, N in --envs (4096)
    target  online and target logits [B, 500, 31], B in --batches (64)

Per shape and form: --repeats (5) timed windows of --iters calls between device events after a warm-up, taken in turns; the
median and the spread (max - min) of the time per call.  One GPU process; run it under a timeout.

    python tools/dueling_head_rates.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from irbpp_amd import replay  # noqa: E402
from c51_head_rates import GAMMA_N, V_MAX, V_MIN, act_torch, compare, learn_torch  # noqa: E402

S, ATOMS = 500, 31


def head_torch(v, a):
    q = v.unsqueeze(1) + a - a.mean(1, keepdim=True)
    return torch.softmax(q, dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="*", default=[4096])
    ap.add_argument("--batches", type=int, nargs="*", default=[64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dueling_head_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    support = torch.linspace(V_MIN, V_MAX, ATOMS, device=dev)
    rand = lambda *shape: torch.randn(shape, device=dev, generator=gen)          # noqa: E731
    out = {"S": S, "atoms": ATOMS, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "act": {}, "target": {}}
    for n in a.envs:
        v, adv = rand(n, ATOMS), 3 * rand(n, S, ATOMS)
        state = torch.zeros((n, S * 5 + 7), device=dev)
        state[:, :S * 5].view(n, S, 5)[:, :, 4] = (torch.rand((n, S), device=dev, generator=gen) < 0.7).float()
        forms = {"torch": lambda: act_torch(head_torch(v, adv), support, replay.mask_from_state(state, S)),
                 "torch+c51": lambda: replay.distributional_greedy_action(head_torch(v, adv), support, state, S, use_hip=True),
                 "dueling": lambda: replay.dueling_greedy_action(v, adv, support, state, S, use_hip=True)}
        r = compare(forms, a.iters, a.repeats)
        r["a_bytes"] = n * S * ATOMS * 4
        out["act"][str(n)] = r
        del v, adv, state
    for b in a.batches:
        v_on, a_on, v_tg, a_tg = rand(b, ATOMS), 3 * rand(b, S, ATOMS), rand(b, ATOMS), 3 * rand(b, S, ATOMS)
        returns = torch.rand((b,), device=dev, generator=gen) * 11 - 2
        nonterm = (torch.rand((b, 1), device=dev, generator=gen) < 0.8).float()
        forms = {"torch": lambda: learn_torch(head_torch(v_on, a_on), head_torch(v_tg, a_tg), returns, nonterm, support),
                 "torch+c51": lambda: replay.c51_target(head_torch(v_on, a_on), head_torch(v_tg, a_tg), returns, nonterm, support,
                                                        GAMMA_N, V_MIN, V_MAX, use_hip=True),
                 "dueling": lambda: replay.dueling_c51_target(v_on, a_on, v_tg, a_tg, returns, nonterm, support, GAMMA_N, V_MIN,
                                                              V_MAX, use_hip=True)}
        out["target"][str(b)] = compare(forms, a.iters * 5, a.repeats)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
