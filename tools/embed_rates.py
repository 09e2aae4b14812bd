#!/usr/bin/env python
"""Tooling: the embedding stage of the network's acting forward (model.py:318-326, :337-352), four forms in one process,
interleaved (the manner of shape_feature_rates.py):

    reference  the reference's lines restated on torch tensors: the heightmap CNN, init_candidate_embed, the
               [N * S, 512] concatenation, project_layer on every row, the boolean-mask zeroing, the mean
    torch      replay.embed(use_hip=False): torch's layers in the factored form (project_layer[0]'s shape / map part once
               per bin, added to the candidate part of every row)
    fused      replay.embed(use_hip=True): the two launches of irbpp_embed
    mfma       the same with form="mfma": the three per-row layers on the matrix cores (irbpp_embed_mfma), the same bits

    N in --bins (4096 1024: acting; 64: the no_grad forwards of learn), S = 500, L = 32, the reference's widths.

Per size and form: --repeats (5) timed windows of --iters calls between device events after a warm-up, taken in turns; the
median and the spread (max - min) of the time per call, and the multiply-adds of the factored form per millisecond of the
fused and of the mfma call.  Whether the two kernel forms wrote identical x and xg on the measured inputs is recorded per size
(as bits; a NaN, which these inputs do not produce, would count as a difference).  One GPU process; run it under a timeout.

    python tools/embed_rates.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from irbpp_amd import replay  # noqa: E402
from c51_head_rates import compare  # noqa: E402

S, L, FEAT, SLOPE = 500, 32, 128, 0.01


def multiply_adds(n, s, w):
    """(the factored form's, the reference's) multiply-adds of one call, from the shapes."""
    q = (w.map_len // 4) ** 2
    per_bin = w.c1 * 4 * q * 16 + w.c2 * q * w.c1 * 16 + w.c3 * q * w.c2 * 9
    row_rest = 4 * w.cand_hidden + w.cand_hidden * w.cand_embed + w.proj_hidden * w.embed
    shared = (w.feat + w.map_feat) * w.proj_hidden
    factored = n * (per_bin + shared + s * (row_rest + w.cand_embed * w.proj_hidden))
    reference = n * (per_bin + s * (row_rest + (w.feat + w.map_feat + w.cand_embed) * w.proj_hidden))
    return factored, reference


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, nargs="*", default=[4096, 1024, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("embed_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(1)
    height = nn.Sequential(nn.Conv2d(1, 16, 4, stride=2, padding=1), nn.LeakyReLU(), nn.Conv2d(16, 32, 4, stride=2, padding=1), nn.LeakyReLU(),
                           nn.Conv2d(32, 4, 3, stride=1, padding=1), nn.LeakyReLU()).to(dev)
    cand = nn.Sequential(nn.Linear(4, 32), nn.LeakyReLU(), nn.Linear(32, 128)).to(dev)
    proj = nn.Sequential(nn.Linear(512, 256), nn.LeakyReLU(), nn.Linear(256, 128)).to(dev)
    w = replay.EmbedWeights.from_layers(height, cand, proj, SLOPE, map_len=L)
    out = {"S": S, "L": L, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "bins": {}}

    with torch.no_grad():
        for n in a.bins:
            obs = torch.rand((n, 5 * S + 9 + L * L), device=dev, generator=gen)
            obs[:, 4:5 * S:5] = (torch.rand((n, S), device=dev, generator=gen) < 0.6).float()
            sf = torch.rand((n, FEAT), device=dev, generator=gen)
            x_out = torch.empty((n, S, w.embed), device=dev)
            xg_out = torch.empty((n, w.embed), device=dev)
            x_mfma = torch.empty((n, S, w.embed), device=dev)
            xg_mfma = torch.empty((n, w.embed), device=dev)

            def reference():
                rows = obs[:, :5 * S].reshape(n, S, 5)
                invalid = 1 - rows[:, :, 4]
                fmap = height(obs[:, 5 * S + 9:].reshape(n, 1, L, L)).reshape(n, -1)
                e2 = cand(rows[:, :, :4].contiguous().view(n, S, -1))
                cat = torch.cat((sf.repeat(1, S).reshape(n, S, -1), fmap.repeat((1, S)).reshape(n, S, -1), e2), dim=2).view(n * S, -1)
                emb = proj(cat).view(n, S, -1)
                emb[invalid.view(n, S, 1).expand(emb.shape).bool()] = 0
                return emb, emb.mean(1)

            forms = {"reference": reference,
                     "torch": lambda: replay.embed(obs, sf, w, use_hip=False),
                     "fused": lambda: replay.embed(obs, sf, w, use_hip=True, out=x_out, out_global=xg_out),
                     "mfma": lambda: replay.embed(obs, sf, w, use_hip=True, out=x_mfma, out_global=xg_mfma, form="mfma")}
            ref = [t.clone() for t in forms["reference"]()]
            r = compare(forms, a.iters, a.repeats, warmup=2)
            for f in ("torch", "fused", "mfma"):
                got = forms[f]()
                r[f]["max_abs_difference_to_reference"] = [(g - t).abs().max().item() for g, t in zip(got, ref)]
            fact, full = multiply_adds(n, S, w)
            r["multiply_adds_factored"], r["multiply_adds_reference"] = fact, full
            r["fused"]["multiply_adds_per_ms"] = fact / r["fused"]["median_ms"]
            r["mfma"]["multiply_adds_per_ms"] = fact / r["mfma"]["median_ms"]
            r["mfma"]["ratio_to_fused"] = r["mfma"]["median_ms"] / r["fused"]["median_ms"]
            r["mfma"]["ratio_to_torch"] = r["mfma"]["median_ms"] / r["torch"]["median_ms"]
            r["kernel_forms_identical"] = bool(torch.equal(x_out.view(torch.int32), x_mfma.view(torch.int32)) and
                                               torch.equal(xg_out.view(torch.int32), xg_mfma.view(torch.int32)))
            out["bins"][f"N{n}"] = r
            del obs, sf, x_out, xg_out, x_mfma, xg_mfma, ref
            torch.cuda.empty_cache()
    acting = [v for k, v in out["bins"].items() if k != "N64"]
    out["fused_beats_torch_at_every_acting_size"] = bool(acting) and all(
        v["torch"]["median_ms"] - v["fused"]["median_ms"] > max(v["torch"]["spread_ms"], v["fused"]["spread_ms"]) for v in acting)
    for name, other in (("mfma_beats_fused_at_every_acting_size", "fused"), ("mfma_beats_torch_at_every_acting_size", "torch")):
        out[name] = bool(acting) and all(
            v[other]["median_ms"] - v["mfma"]["median_ms"] > max(v[other]["spread_ms"], v["mfma"]["spread_ms"]) for v in acting)
    out["kernel_forms_identical"] = all(v["kernel_forms_identical"] for v in out["bins"].values())
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
