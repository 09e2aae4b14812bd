#!/usr/bin/env python
"""Tooling: the optimiser step of Agent.learn over DQNBPP's parameter tensors, four forms in one process, interleaved (the
manner of dueling_loss_rates.py):

    reference    online_net.zero_grad(), clip_grad_norm_(params, 10), optim.Adam(lr 6.25e-5, eps 1.5e-4).step(): the reference's
                 lines with torch's default arguments (agent.py:44, 118-121)
    foreach      the same with clip_grad_norm_(foreach=True) and Adam(foreach=True)
    fused        the same with Adam(fused=True), where this build of torch offers it
    fused_step   optim.ClippedAdam(grads="zero", use_hip=True).step(): irbpp_clipped_adam_step, two launches

The parameter sets have DQNBPP's tensor shapes (model.py:258-299) for bufferSize 1 (34 tensors) and bufferSize 10 (47: the
attention layer and gat_project_layer on top), written out below.  Every form owns a copy of the set.  The gradients are not
produced by a backward here: after zero_grad() (which frees them) the torch forms get each p.grad set to a kept tensor again,
a host-side attribute write per tensor and no launch; the fused step leaves zeros behind in place and steps on those.  None of
the forms' work depends on the values.

Per size and form: --repeats (5) timed windows of --iters (50) calls between device events after a warm-up of --warmup (20)
calls of every form, taken in turns; the median and the spread (max - min) of the time per call.  One GPU process; run it
under a timeout.

    python tools/optimiser_step_rates.py [--out profiles/optimiser_step/optimiser_step_rates.json]
    python tools/optimiser_step_rates.py --only fused_step --repeats 1   (for `rocprofv3 --kernel-trace --stats`: the kernels' own times)
"""
import argparse
import json
import os
import sys

import torch
from torch.nn.utils import clip_grad_norm_

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from irbpp_amd.optim import ClippedAdam  # noqa: E402
from c51_head_rates import compare  # noqa: E402

LR, EPS, NORM_CLIP = 6.25e-5, 1.5e-4, 10.0
_NOISY = lambda o, i: [(o, i), (o, i), (o,), (o,)]                       # noqa: E731  weight_mu, weight_sigma, bias_mu, bias_sigma
SHAPES_1 = ([(16, 1, 4, 4), (16,), (32, 16, 4, 4), (32,), (4, 32, 3, 3), (4,)]                # heightEncoder
            + [(128, 3), (128,), (128, 128), (128,)]                                           # shapeEncoder
            + [(32, 4), (32,), (128, 32), (128,)]                                              # init_candidate_embed
            + [(256, 512), (256,), (128, 256), (128,)]                                         # project_layer
            + _NOISY(128, 128) + _NOISY(128, 128) + _NOISY(31, 128) + _NOISY(31, 128))         # fc_h_v, fc_h_a, fc_z_v, fc_z_a
SHAPES_10 = (SHAPES_1[:18]
             + [(128, 128), (128, 128), (128, 128), (128, 128), (128,)]                        # W_query, W_key, W_val, W_out
             + [(128, 128), (128,), (128, 128), (128,)]                                        # the attention layer's feed-forward
             + [(256, 384), (256,), (128, 256), (128,)]                                        # gat_project_layer
             + SHAPES_1[18:])
SIZES = {"1": SHAPES_1, "10": SHAPES_10}


def torch_form(shapes, dev, gen, **adam):
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen)) for s in shapes]
    gs = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    foreach = adam.get("foreach")
    opt = torch.optim.Adam(ps, lr=LR, eps=EPS, **adam)

    def step():
        opt.zero_grad()
        for p, g in zip(ps, gs):
            p.grad = g
        clip_grad_norm_(ps, NORM_CLIP, foreach=foreach)
        opt.step()
    return step


def fused_step_form(shapes, dev, gen):
    ps = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=gen)
    opt = ClippedAdam(ps, LR, (0.9, 0.999), EPS, NORM_CLIP, grads="zero", use_hip=True)
    return opt.step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["1", "10"], choices=sorted(SIZES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=["reference", "foreach", "fused", "fused_step"], default=None)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optimiser_step_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    out = {"lr": LR, "eps": EPS, "norm_clip": NORM_CLIP, "iters": a.iters, "repeats": a.repeats, "warmup": a.warmup,
           "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "step": {}}
    for size in a.sizes:
        shapes = SIZES[size]
        forms = {"reference": torch_form(shapes, dev, gen), "foreach": torch_form(shapes, dev, gen, foreach=True)}
        try:
            forms["fused"] = torch_form(shapes, dev, gen, fused=True)
            forms["fused"]()
        except (RuntimeError, TypeError, ValueError) as e:
            forms.pop("fused", None)
            out.setdefault("fused_unavailable", str(e).splitlines()[0])
        forms["fused_step"] = fused_step_form(shapes, dev, gen)
        res = compare({k: f for k, f in forms.items() if a.only in (None, k)}, a.iters, a.repeats, a.warmup)
        res["tensors"], res["elements"] = len(shapes), sum(int(torch.Size(s).numel()) for s in shapes)
        out["step"][size] = res
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
