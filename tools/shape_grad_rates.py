#!/usr/bin/env python
"""Tooling: the shape branch of the forward that carries a gradient (Agent.learn's online forward), forward plus backward,
three forms in one process, interleaved (the manner of streams_rates.py):

    parent   what the caller had before: ShapePoints.gather(ids, indices) [M, k, 3] into torch's layers per row, max over the
             points, backward (two [M, k, 128] activation blocks kept for autograd)
    torch    replay.shape_features_grad(use_hip=False): torch's layers on the unique ids, index back, backward
    fused    replay.shape_features_grad(use_hip=True): irbpp_shape_features_arg, then irbpp_shape_features_backward

    M in --rows (64: the item network's learn batch; 640: the order network's 64 states x 10 slots), k = 1024, 128 / 128 widths;
    tables: "blockout" (synthetic.blockout_voxels' 64 polycubes, P points drawn inside their cubes) and "synthetic200" (200
    shapes of normal points).

Per size and form: --repeats (5) timed windows of --iters calls (forward, backward into zeroed .grad) between device events
after a warm-up, taken in turns; the median and the spread (max - min) of the time per call.  The index set and the upstream
gradient are drawn once outside the windows.  One GPU process; run it under a timeout.

    python tools/shape_grad_rates.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from irbpp_amd import replay, synthetic  # noqa: E402
from c51_head_rates import compare  # noqa: E402

P, K, H1, FEAT, SLOPE = 10000, 1024, 128, 128, 0.01


def tables():
    rng = np.random.default_rng(0)
    block = []
    for occ in synthetic.blockout_voxels(64, 0):
        cells = np.argwhere(np.asarray(occ) > 0)
        block.append((cells[rng.integers(0, len(cells), P)] + rng.random((P, 3))) * 0.04)
    return {"blockout": np.asarray(block, dtype=np.float32), "synthetic200": (rng.standard_normal((200, P, 3)) * 0.2).astype(np.float32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[64, 640])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shape_grad_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    enc = torch.nn.Sequential(torch.nn.Linear(3, H1), torch.nn.LeakyReLU(SLOPE), torch.nn.Linear(H1, FEAT), torch.nn.LeakyReLU(SLOPE)).to(dev)
    params = list(enc.parameters())
    out = {"P": P, "k": K, "hidden": H1, "feat": FEAT, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "sizes": {}}

    def step(forward, g):
        for p in params:
            p.grad = None
        forward().backward(g)

    for name, table in tables().items():
        sp = replay.ShapePoints(table, dev)
        indices = sp.draw_indices(K, generator=gen)
        for m in a.rows:
            obs = torch.zeros((m, 37), device=dev)
            obs[:, 0] = torch.randint(0, sp.n_shapes, (m,), device=dev, generator=gen).float()
            g = torch.randn((m, FEAT), device=dev, generator=gen)
            forwards = {"parent": lambda: torch.max(enc(sp.gather(obs[:, 0], indices)), dim=1)[0],
                        "torch": lambda: replay.shape_features_grad(obs[:, 0], sp, indices, enc[0], enc[2], SLOPE, use_hip=False),
                        "fused": lambda: replay.shape_features_grad(obs[:, 0], sp, indices, enc[0], enc[2], SLOPE, use_hip=True)}
            forms = {k: (lambda f=f: step(f, g)) for k, f in forwards.items()}
            grads = {}
            for k, fn in forms.items():
                fn()
                grads[k] = [p.grad.detach().clone() for p in params]
            r = compare(forms, a.iters, a.repeats)
            for k in ("torch", "fused"):                     # beside the parent's, relative to the largest entry of each tensor
                r[k]["max_relative_difference_to_parent"] = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(grads[k], grads["parent"]))
            r["distinct_ids"] = int(torch.unique(obs[:, 0]).numel())
            out["sizes"][f"{name}_M{m}"] = r
            del obs, g
        del sp
    sizes = out["sizes"].values()
    out["fused_beats_torch_at_every_size"] = all(
        v["torch"]["median_ms"] - v["fused"]["median_ms"] > max(v["torch"]["spread_ms"], v["fused"]["spread_ms"]) for v in sizes)
    out["fused_beats_parent_at_every_size"] = all(
        v["parent"]["median_ms"] - v["fused"]["median_ms"] > max(v["parent"]["spread_ms"], v["fused"]["spread_ms"]) for v in sizes)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
