"""Writes tests/golden/order_embed_ref.npz: the reference's own DQNBPP.embed_k_buffer_shape_with_gat (model.py:355-383) run on
the CPU with bufferSize = 5 on a small seeded order observation block, with the weights it ran on.  Data only: the weights of
heightEncoder, shapeEncoder, gat_project_layer and embedder (256 820 floats), the observation, the [15, 128] shape_feature
the forward gathered and its two outputs.

    python tests/golden/make_order_embed_golden.py /path/to/the/reference

The reference's model.py is imported from where it lies.  Its `tools` module needs packages this project does not; model.py
takes one function from it, the usual three-line layer initialiser, which this script provides under that name.  That
initialiser zeroes every bias, so the biases of every layer that has one are redrawn (seeded) before the forward: they are
part of what is checked."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
K, BATCH, L, POINTS, N_SHAPES, TABLE_POINTS = 5, 3, 32, 64, 6, 200


def _init(module, weight_init, bias_init, gain=1):
    weight_init(module.weight.data, gain=gain)
    bias_init(module.bias.data)
    return module


def main(reference_dir):
    tools = types.ModuleType("tools")
    tools.init = _init
    sys.modules["tools"] = tools
    sys.path.insert(0, reference_dir)
    import model as reference_model

    torch.manual_seed(20240611)
    np.random.seed(20240611)
    args = types.SimpleNamespace(selectedAction=K, atoms=31, level="item", heightMap=True, ZRotNum=8, bin_dimension=[0.32, 0.32, 0.3],
                                 resolutionH=0.01, bufferSize=K, hidden_size=128, noisy_std=0.5, device="cpu", samplePointsNum=POINTS)
    shape_array = torch.rand(N_SHAPES, TABLE_POINTS, 3) * 0.2
    net = reference_model.DQNBPP(args, K, shape_array)
    assert net.MapLength == L
    att, ff = net.embedder.layers[0][0].module, net.embedder.layers[0][1].module
    assert att.n_heads == 1 and len(net.embedder.layers) == 1 and net.embedder.init_embed is None
    with torch.no_grad():
        for m in list(net.heightEncoder) + list(net.shapeEncoder) + list(net.gat_project_layer) + [att.W_out] + list(ff):
            if getattr(m, "bias", None) is not None:
                m.bias.uniform_(-0.1, 0.1)

    rng = np.random.default_rng(8)
    obs = np.zeros((BATCH, K + L * L), dtype=np.float32)
    obs[:, :K] = np.array([[4, 0, 2, 2, 5], [1, 1, 1, 1, 1], [3, 5, 0, 4, 2]], dtype=np.float32)     # one bin of five equal items
    obs[:, K:] = np.round(rng.uniform(0.0, 0.3, (BATCH, L * L)), 2)

    kept = {}
    handle = net.shapeEncoder.register_forward_hook(lambda mod, inp, out: kept.__setitem__("shape_feature", torch.max(out, dim=1)[0]))
    with torch.no_grad():
        embeddings, graph_embed = net.embed_k_buffer_shape_with_gat(torch.from_numpy(obs.copy()))
    handle.remove()
    assert tuple(kept["shape_feature"].shape) == (BATCH * K, 128) and tuple(embeddings.shape) == (BATCH, K, 128)

    data = {"obs": obs, "shape_feature": kept["shape_feature"].numpy(), "embeddings": embeddings.numpy(), "graph_embed": graph_embed.numpy(),
            "buffer_size": np.int32(K), "map_len": np.int32(L), "negative_slope": np.float32(0.01)}
    count = 0

    def keep(name, m):
        nonlocal count
        data[name + ".weight"] = m.weight.detach().numpy()
        count += m.weight.numel()
        if m.bias is not None:
            data[name + ".bias"] = m.bias.detach().numpy()
            count += m.bias.numel()

    for name, seq in (("height_encoder", net.heightEncoder), ("shape_encoder", net.shapeEncoder), ("gat_project_layer", net.gat_project_layer),
                      ("embedder.ff", ff)):
        for i, m in enumerate(m for m in seq if getattr(m, "weight", None) is not None):
            keep(f"{name}.{i}", m)
    for name in ("W_query", "W_key", "W_val", "W_out"):
        keep("embedder." + name, getattr(att, name))
    assert count == 256820
    out = os.path.join(HERE, "order_embed_ref.npz")
    np.savez_compressed(out, **data)                     # uncompressed it would pass the size limit of a committed file
    print("order_embed_ref.npz:", os.path.getsize(out), "bytes;", count, "weights")


if __name__ == "__main__":
    main(sys.argv[1])
