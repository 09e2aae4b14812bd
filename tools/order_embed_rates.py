#!/usr/bin/env python
"""Tooling: the order network's embedding stage (model.py:355-383, bufferSize > 1), four forms in one process, interleaved
(the manner of embed_rates.py):

    reference  the reference's lines restated on torch tensors: the heightmap CNN, shapeArray[ids.cpu()] on the host with the
               copy of the gathered points to the device, shapeEncoder and the max, the [N * k, 384] concatenation,
               gat_project_layer on every row, Q / K / V, the two batched k x k matmuls, softmax, clone and masked
               assignment, W_out, the feed-forward pair, the residual adds, the mean (it carries the shape branch: that is how
               the reference's stage comes)
    torch      replay.order_embed(use_hip=False): torch's layers in the factored form, from a given shape feature
    fused      replay.order_embed(use_hip=True): the two launches of irbpp_order_embed, from a given shape feature
    mfma       the same with form="mfma": the eight linear layers on the matrix cores (irbpp_order_embed_mfma), the same bits

and the first three for the whole acting forward (order_network_greedy_action with use_hip=True / None, and the reference's
lines followed by torch's streams, softmax and arg-max), as "chain_*".

    N in --bins (4096 1024), k = 10 (cfg 4), L = 32, the reference's widths, 100 shapes of 1000 points, 256 sampled.

Per size and form: --repeats (5) timed windows of --iters calls between device events after a warm-up, taken in turns; the
median and the spread (max - min) of the time per call.  Whether the two kernel forms wrote identical x and xg on the measured
inputs is recorded per size ("kernel_forms_identical").  One GPU process; run it under a timeout.

    python tools/order_embed_rates.py [--out FILE.json]
"""
import argparse
import json
import math
import os
import sys
import types

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from irbpp_amd import replay  # noqa: E402
from c51_head_rates import compare  # noqa: E402

K, L, E, SLOPE, N_SHAPES, TABLE_POINTS, SAMPLED, ATOMS, HIDDEN = 10, 32, 128, 0.01, 100, 1000, 256, 31, 128


class Noisy(nn.Module):
    """The parameters of the reference's NoisyLinear, which is all StreamWeights reads."""

    def __init__(self, i, o):
        super().__init__()
        for name, shape in (("weight_mu", (o, i)), ("weight_sigma", (o, i)), ("bias_mu", (o,)), ("bias_sigma", (o,))):
            self.register_parameter(name, nn.Parameter(torch.randn(shape) / math.sqrt(i)))
        self.register_buffer("weight_epsilon", torch.randn(o, i))
        self.register_buffer("bias_epsilon", torch.randn(o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, nargs="*", default=[4096, 1024])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("order_embed_rates.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(1)
    height = nn.Sequential(nn.Conv2d(1, 16, 4, stride=2, padding=1), nn.LeakyReLU(), nn.Conv2d(16, 32, 4, stride=2, padding=1), nn.LeakyReLU(),
                           nn.Conv2d(32, 4, 3, stride=1, padding=1), nn.LeakyReLU()).to(dev)
    shape_enc = nn.Sequential(nn.Linear(3, 128), nn.LeakyReLU(), nn.Linear(128, 128), nn.LeakyReLU()).to(dev)
    proj = nn.Sequential(nn.Linear(384, 256), nn.LeakyReLU(), nn.Linear(256, E)).to(dev)
    att = types.SimpleNamespace(n_heads=1, W_query=nn.Linear(E, E, bias=False).to(dev), W_key=nn.Linear(E, E, bias=False).to(dev),
                                W_val=nn.Linear(E, E, bias=False).to(dev), W_out=nn.Linear(E, E).to(dev))
    ff = nn.Sequential(nn.Linear(E, 128), nn.ReLU(), nn.Linear(128, E)).to(dev)
    embedder = types.SimpleNamespace(init_embed=None, layers=[[types.SimpleNamespace(module=att), types.SimpleNamespace(module=ff)]])
    w = replay.OrderEmbedWeights.from_layers(height, proj, embedder, SLOPE, map_len=L)
    sw = replay.ShapeEncoderWeights.from_layers(shape_enc[0], shape_enc[2], SLOPE)
    streams = [Noisy(E, HIDDEN).to(dev), Noisy(HIDDEN, ATOMS).to(dev), Noisy(E, HIDDEN).to(dev), Noisy(HIDDEN, ATOMS).to(dev)]
    tw = replay.StreamWeights(*streams)
    shape_array = torch.rand(N_SHAPES, TABLE_POINTS, 3) * 0.2                    # on the host, as the reference keeps it
    points = replay.ShapePoints(shape_array, dev)
    support = torch.linspace(-1.0, 8.0, ATOMS, device=dev)
    norm = 1 / math.sqrt(E)
    out = {"k": K, "L": L, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "bins": {}}

    with torch.no_grad():
        for n in a.bins:
            obs = torch.rand((n, K + L * L), device=dev, generator=gen)
            obs[:, :K] = torch.randint(0, N_SHAPES, (n, K), device=dev, generator=gen).float()
            indices = points.draw_indices(SAMPLED, generator=gen)
            idx_host = indices.cpu().long()
            sf = replay.shape_features(obs[:, :K].contiguous(), points, indices, sw, use_hip=True)
            x_out = torch.empty((n, K, E), device=dev)
            xg_out = torch.empty((n, E), device=dev)
            x_mfma = torch.empty((n, K, E), device=dev)
            xg_mfma = torch.empty((n, E), device=dev)

            def reference():
                fmap = height(obs[:, K:].reshape(n, 1, L, L)).reshape(n, -1)
                ids = obs[:, :K].detach().cpu().long().reshape(-1)
                pts = shape_array[ids][:, idx_host].to(dev)
                feat = torch.max(shape_enc(pts), dim=1)[0]
                cat = torch.cat((feat.reshape(n, K, -1), fmap.repeat((1, K)).reshape(n, K, -1)), dim=2).view(n * K, -1)
                h = proj(cat).view(n, K, E)
                mask = torch.zeros((n, K)).unsqueeze(1).repeat((1, K, 1)).bool().view(1, n, K, K).to(dev)
                hflat = h.contiguous().view(-1, E)
                q, key, v = (m(hflat).view(1, n, K, -1) for m in (att.W_query, att.W_key, att.W_val))
                compat = norm * torch.matmul(q, key.transpose(2, 3))
                compat[mask] = -30
                attn = torch.softmax(compat, dim=-1).clone()
                attn[mask] = 0
                heads = torch.matmul(attn, v)
                h = h + att.W_out(heads.permute(1, 2, 0, 3).contiguous().view(-1, E)).view(n, K, E)
                h = h + ff(h)
                return h, h.mean(1)

            def chain_reference():
                x, xg = reference()
                vv = F.linear(F.relu(F.linear(xg, tw.w_hv, tw.b_hv)), tw.w_zv, tw.b_zv).view(-1, 1, ATOMS)
                aa = F.linear(F.relu(F.linear(x, tw.w_ha, tw.b_ha)), tw.w_za, tw.b_za).view(-1, K, ATOMS)
                p = F.softmax(vv + aa - aa.mean(1, keepdim=True), dim=2)
                return ((p * support).sum(2).argmax(1),)

            forms = {"reference": reference,
                     "torch": lambda: replay.order_embed(obs, sf, w, use_hip=False),
                     "fused": lambda: replay.order_embed(obs, sf, w, use_hip=True, out=x_out, out_global=xg_out),
                     "mfma": lambda: replay.order_embed(obs, sf, w, use_hip=True, out=x_mfma, out_global=xg_mfma, form="mfma"),
                     "chain_reference": chain_reference,
                     "chain_default": lambda: (replay.order_network_greedy_action(obs, points, indices, sw, w, tw, support),),
                     "chain_fused": lambda: (replay.order_network_greedy_action(obs, points, indices, sw, w, tw, support, use_hip=True),)}
            ref = [t.clone() for t in forms["reference"]()]
            r = compare(forms, a.iters, a.repeats, warmup=2)
            for f in ("torch", "fused", "mfma"):
                got = forms[f]()
                r[f]["max_abs_difference_to_reference"] = [(g - t).abs().max().item() for g, t in zip(got, ref)]
            r["mfma"]["ratio_to_fused"] = r["mfma"]["median_ms"] / r["fused"]["median_ms"]
            r["mfma"]["ratio_to_torch"] = r["mfma"]["median_ms"] / r["torch"]["median_ms"]
            r["kernel_forms_identical"] = bool(torch.equal(x_out.view(torch.int32), x_mfma.view(torch.int32)) and
                                               torch.equal(xg_out.view(torch.int32), xg_mfma.view(torch.int32)))
            out["bins"][f"N{n}"] = r
            del obs, sf, x_out, xg_out, x_mfma, xg_mfma, ref
            torch.cuda.empty_cache()
    sizes = list(out["bins"].values())
    out["fused_beats_torch_at_every_size"] = bool(sizes) and all(
        v["torch"]["median_ms"] - v["fused"]["median_ms"] > max(v["torch"]["spread_ms"], v["fused"]["spread_ms"]) for v in sizes)
    for name, other in (("mfma_beats_fused_at_every_size", "fused"), ("mfma_beats_torch_at_every_size", "torch")):
        out[name] = bool(sizes) and all(
            v[other]["median_ms"] - v["mfma"]["median_ms"] > max(v[other]["spread_ms"], v["mfma"]["spread_ms"]) for v in sizes)
    out["kernel_forms_identical"] = all(v["kernel_forms_identical"] for v in sizes)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
