#!/usr/bin/env python
"""Tooling: the shape branch in front of the network (model.py:328-335), three forms in one process, interleaved (the manner
of streams_rates.py):

    parent   the reference's lines restated on torch tensors: the point table [n_shapes, P, 3] on the CPU, ids.cpu(), the
             host gather of the sampled points (one indexing with both index sets, N x k x 3 floats: kinder than the
             reference's two steps, whose first materialises N x P x 3), .to(device), the two Linear + LeakyReLU layers per
             row, max over the points
    torch    replay.shape_features(use_hip=False): the table on the device, torch.unique of the ids, the layers once per
             distinct id, max, index back
    fused    replay.shape_features(use_hip=True): the two launches of irbpp_shape_features

    N in --rows (4096 1024: acting; 64: the learn batch), n_shapes in --shapes (8 100), P = 100000, k = 1024, 128 / 128 widths.

Per shape and form: --repeats (5) timed windows of --iters calls between device events after a warm-up, taken in turns; the
median and the spread (max - min) of the time per call.  The index set is drawn once outside the windows in every form.  One
GPU process; run it under a timeout.

    python tools/shape_feature_rates.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from irbpp_amd import replay  # noqa: E402
from c51_head_rates import compare  # noqa: E402

P, K, H1, FEAT, SLOPE = 100000, 1024, 128, 128, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[4096, 1024, 64])
    ap.add_argument("--shapes", type=int, nargs="*", default=[8, 100])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shape_feature_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    l1, l2 = torch.nn.Linear(3, H1).to(dev), torch.nn.Linear(H1, FEAT).to(dev)
    w = replay.ShapeEncoderWeights.from_layers(l1, l2, SLOPE)
    out = {"P": P, "k": K, "hidden": H1, "feat": FEAT, "iters": a.iters, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "rows": {}}

    with torch.no_grad():
        for n_shapes in a.shapes:
            table = (np.random.default_rng(n_shapes).standard_normal((n_shapes, P, 3)) * 0.2).astype(np.float32)
            cpu_table = torch.from_numpy(table)
            sp = replay.ShapePoints(table, dev)
            indices = sp.draw_indices(K, generator=gen)
            host_indices = indices.cpu().long()
            for n in a.rows:
                obs = torch.zeros((n, 37), device=dev)
                obs[:, 0] = torch.randint(0, n_shapes, (n,), device=dev, generator=gen).float()

                def parent():
                    ids = obs[:, 0].long()
                    pts = cpu_table[ids.cpu()[:, None], host_indices[None, :]].to(dev)
                    h = F.leaky_relu(l2(F.leaky_relu(l1(pts), SLOPE)), SLOPE)
                    return torch.max(h, dim=1)[0]

                forms = {"parent": parent,
                         "torch": lambda: replay.shape_features(obs[:, 0], sp, indices, w, use_hip=False),
                         "fused": lambda: replay.shape_features(obs[:, 0], sp, indices, w, use_hip=True)}
                ref = forms["parent"]()
                r = compare(forms, a.iters, a.repeats)
                for f in ("torch", "fused"):
                    r[f]["max_abs_difference_to_parent"] = (forms[f]() - ref).abs().max().item()
                r["distinct_ids"] = int(torch.unique(obs[:, 0]).numel())
                out["rows"][f"N{n}_shapes{n_shapes}"] = r
                del obs, ref
            del sp, cpu_table, table
    acting = [v for k, v in out["rows"].items() if not k.startswith("N64_")]
    out["fused_beats_torch_at_every_acting_size"] = all(
        v["torch"]["median_ms"] - v["fused"]["median_ms"] > max(v["torch"]["spread_ms"], v["fused"]["spread_ms"]) for v in acting)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
