#!/usr/bin/env python
"""Tooling: the last stage of the network in front of the greedy action, three forms in one process, interleaved (the manner of
dueling_head_rates.py):

    torch    the parent's path: the four effective weight matrices materialised (mu + sigma * eps), four F.linear and two
             relu (model.py:393-394), then the dueling head kernel (replay.dueling_greedy_action with use_hip=True)
    fused    StreamWeights.refresh() + replay.streams_greedy_action with use_hip=True: irbpp_noisy_weights and one launch
    mfma     the same with form="mfma": the chains on the matrix cores (irbpp_streams_act_mfma), the same bits

    act      x [N, 500, 128], x_global [N, 128], 31 atoms, with the observation's mask, N in --envs (4096 1024)
    logits   the no-grad forward of a learn batch: torch's layers against replay.streams_logits, B in --batches (64)

Per shape and form: --repeats (5) timed windows of --iters calls between device events after a warm-up, taken in turns; the
median and the spread (max - min) of the time per call, and the bytes of x per second the median implies.  One GPU process;
run it under a timeout.

    python tools/streams_rates.py [--out FILE.json]
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
from c51_head_rates import V_MAX, V_MIN, compare  # noqa: E402

S, E, H, ATOMS = 500, 128, 128, 31


class Layer(object):
    def __init__(self, out, inp, dev, gen):
        r = lambda *s: torch.randn(s, device=dev, generator=gen)                 # noqa: E731
        self.weight_mu, self.weight_sigma, self.weight_epsilon = r(out, inp) / inp ** 0.5, r(out, inp) * 0.02, r(out, inp)
        self.bias_mu, self.bias_sigma, self.bias_epsilon = r(out) * 0.1, r(out) * 0.02, r(out)

    def linear(self, x):
        return F.linear(x, self.weight_mu + self.weight_sigma * self.weight_epsilon, self.bias_mu + self.bias_sigma * self.bias_epsilon)


def logits_torch(layers, x, xg):
    hv, zv, ha, za = layers
    return zv.linear(F.relu(hv.linear(xg))), za.linear(F.relu(ha.linear(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="*", default=[4096, 1024])
    ap.add_argument("--batches", type=int, nargs="*", default=[64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("streams_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    support = torch.linspace(V_MIN, V_MAX, ATOMS, device=dev)
    layers = [Layer(H, E, dev, gen), Layer(ATOMS, H, dev, gen), Layer(H, E, dev, gen), Layer(ATOMS, H, dev, gen)]
    w = replay.StreamWeights.from_layers(*layers)
    out = {"S": S, "embed": E, "hidden": H, "atoms": ATOMS, "iters": a.iters, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "act": {}, "logits": {}}

    def fused_act(x, xg, state, form="chain"):
        w.refresh()
        return replay.streams_greedy_action(x, xg, w, support, state, use_hip=True, form=form)

    def fused_logits(x, xg, form="chain"):
        w.refresh()
        return replay.streams_logits(x, xg, w, use_hip=True, form=form)

    with torch.no_grad():
        for kind, sizes in (("act", a.envs), ("logits", a.batches)):
            for n in sizes:
                x, xg = torch.randn((n, S, E), device=dev, generator=gen), torch.randn((n, E), device=dev, generator=gen)
                state = torch.zeros((n, S * 5 + 7), device=dev)
                state[:, :S * 5].view(n, S, 5)[:, :, 4] = (torch.rand((n, S), device=dev, generator=gen) < 0.7).float()
                if kind == "act":
                    forms = {"torch": lambda: replay.dueling_greedy_action(*logits_torch(layers, x, xg), support, state, S, use_hip=True),
                             "fused": lambda: fused_act(x, xg, state), "mfma": lambda: fused_act(x, xg, state, "mfma")}
                    same = (forms["torch"]() == forms["fused"]()).float().mean().item()
                    fused_same = bool(torch.equal(forms["fused"](), forms["mfma"]()))
                else:
                    forms = {"torch": lambda: logits_torch(layers, x, xg), "fused": lambda: fused_logits(x, xg),
                             "mfma": lambda: fused_logits(x, xg, "mfma")}
                    same = None
                    fused_same = all(torch.equal(c, m) for c, m in zip(forms["fused"](), forms["mfma"]()))
                r = compare(forms, a.iters, a.repeats)
                r["x_bytes"] = n * S * E * 4
                for f in forms:
                    r[f]["x_bytes_per_s"] = r["x_bytes"] / (r[f]["median_ms"] * 1e-3)
                if same is not None:
                    r["actions_equal_fraction"] = same      # torch's GEMM sums in another order: near-ties may differ
                r["fused_and_mfma_identical"] = fused_same  # act: every environment's action; logits: every bit of v and a
                out[kind][str(n)] = r
                del x, xg, state
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
