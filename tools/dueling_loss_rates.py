#!/usr/bin/env python
"""Tooling: the loss that carries the gradient, from the online network's logits, two forms in one process, interleaved (the
manner of dueling_head_rates.py):

    torch      model.py:395-398 with log=True (combine + log_softmax), agent.py:86 and 117, and autograd back to v.grad and a.grad
    dueling    replay.dueling_c51_loss with use_hip=True (irbpp_dueling_loss + irbpp_dueling_loss_backward), likewise

    v [B, 31], a [B, 500, 31], B in --batches (64 512); one call = forward, (weights * loss).mean().backward(), both .grad set
    to None again

Per shape and form: --repeats (5) timed windows of --iters (20) calls between device events after a warm-up of --warmup (20)
calls of every form, taken in turns; the median and the spread (max - min) of the time per call.  One GPU process; run it
under a timeout.

    python tools/dueling_loss_rates.py [--out FILE.json]
    python tools/dueling_loss_rates.py --only dueling --repeats 1      (for `rocprofv3 --kernel-trace --stats`: the kernels' own times)
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from irbpp_amd import replay  # noqa: E402
from c51_head_rates import compare  # noqa: E402

S, ATOMS = 500, 31


def loss_torch(v, a, actions, m):
    q = v.unsqueeze(1) + a - a.mean(1, keepdim=True)
    log_ps = F.log_softmax(q, dim=2)
    log_ps_a = log_ps[range(a.shape[0]), actions]
    return -torch.sum(m * log_ps_a, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=["torch", "dueling"], default=None)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dueling_loss_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda *shape: torch.randn(shape, device=dev, generator=gen)          # noqa: E731
    out = {"S": S, "atoms": ATOMS, "iters": a.iters, "repeats": a.repeats, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "loss": {}}
    for b in a.batches:
        v, adv = rand(b, ATOMS).requires_grad_(), (3 * rand(b, S, ATOMS)).requires_grad_()
        actions = torch.randint(0, S, (b,), device=dev, generator=gen)
        m = torch.softmax(rand(b, ATOMS), 1)
        weights = torch.rand((b,), device=dev, generator=gen)

        def step(form):
            loss = form(v, adv, actions, m)
            (weights * loss).mean().backward()
            v.grad = adv.grad = None
        forms = {"torch": lambda: step(loss_torch),
                 "dueling": lambda: step(lambda *x: replay.dueling_c51_loss(*x, use_hip=True))}
        out["loss"][str(b)] = compare({k: f for k, f in forms.items() if a.only in (None, k)}, a.iters, a.repeats, a.warmup)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
