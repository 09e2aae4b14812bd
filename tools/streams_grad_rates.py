#!/usr/bin/env python
"""Tooling: the noisy streams of the forward that carries a gradient (Agent.learn's online forward, model.py:393-394), forward
plus backward, the forms in one process, interleaved (the manner of shape_grad_rates.py):

    parent   what the caller had before: torch's four noisy layers under autograd (F.linear / relu on mu + sigma * epsilon),
             from the embeddings to the logits and back (replay.streams_logits_grad(use_hip=False) is these lines)
    chain    replay.streams_logits_grad(use_hip=True, form="chain"): irbpp_noisy_weights, irbpp_streams_act, then
             irbpp_streams_backward
    mfma     the same with the forward on the matrix cores (irbpp_streams_act_mfma); the backward is the same launches

    B in --batch (64: the learn batch; 512), S = 500, E = H = 128, A = 31.

Per size and form: --repeats (5) timed windows of --iters calls (forward, backward into cleared .grad, x and x_global with a
gradient) between device events after a warm-up, taken in turns; the median and the spread (max - min) of the time per call.
The inputs and the upstream gradients are drawn once outside the windows.  One GPU process; run it under a timeout.

    python tools/streams_grad_rates.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from irbpp_amd import replay  # noqa: E402
from c51_head_rates import compare  # noqa: E402

S, E, H, A = 500, 128, 128, 31


class Noisy(torch.nn.Module):
    def __init__(self, fan_in, fan_out, gen, dev):
        super().__init__()
        r = lambda *s: torch.randn(s, device=dev, generator=gen)                                # noqa: E731
        self.weight_mu = torch.nn.Parameter(r(fan_out, fan_in) / fan_in ** 0.5)
        self.weight_sigma = torch.nn.Parameter(torch.full((fan_out, fan_in), 0.5 / fan_in ** 0.5, device=dev))
        self.bias_mu = torch.nn.Parameter(r(fan_out) / fan_in ** 0.5)
        self.bias_sigma = torch.nn.Parameter(torch.full((fan_out,), 0.5 / fan_in ** 0.5, device=dev))
        self.register_buffer("weight_epsilon", r(fan_out, fan_in))
        self.register_buffer("bias_epsilon", r(fan_out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("streams_grad_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    layers = [Noisy(E, H, gen, dev), Noisy(H, A, gen, dev), Noisy(E, H, gen, dev), Noisy(H, A, gen, dev)]
    params = [p for layer in layers for p in layer.parameters()]
    out = {"S": S, "embed": E, "hidden": H, "atoms": A, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "sizes": {}}
    for b in a.batch:
        x = torch.randn((b, S, E), device=dev, generator=gen).requires_grad_(True)
        xg = torch.randn((b, E), device=dev, generator=gen).requires_grad_(True)
        gv, ga = torch.randn((b, A), device=dev, generator=gen), torch.randn((b, S, A), device=dev, generator=gen)

        def step(kw):
            for p in params + [x, xg]:
                p.grad = None
            v, adv = replay.streams_logits_grad(x, xg, *layers, **kw)
            torch.autograd.backward([v, adv], [gv, ga])

        kws = {"parent": dict(use_hip=False), "chain": dict(use_hip=True, form="chain"), "mfma": dict(use_hip=True, form="mfma")}
        forms = {k: (lambda kw=kw: step(kw)) for k, kw in kws.items()}
        grads = {}
        for k, fn in forms.items():
            fn()
            grads[k] = [p.grad.detach().clone() for p in params + [x, xg]]
        r = compare(forms, a.iters, a.repeats)
        for k in ("chain", "mfma"):                          # beside the parent's, relative to the largest entry of each tensor
            r[k]["max_relative_difference_to_parent"] = max(((p - q).abs().max() / q.abs().max()).item() for p, q in zip(grads[k], grads["parent"]))
        r["mfma_bits_equal_chain"] = all(torch.equal(p, q) for p, q in zip(grads["mfma"], grads["chain"]))
        out["sizes"][f"B{b}"] = r
        del x, xg, gv, ga
    sizes = out["sizes"].values()
    out["chain_beats_parent_at_every_size"] = all(
        v["parent"]["median_ms"] - v["chain"]["median_ms"] > max(v["parent"]["spread_ms"], v["chain"]["spread_ms"]) for v in sizes)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
