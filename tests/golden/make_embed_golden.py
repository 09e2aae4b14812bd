"""Writes tests/golden/embed_ref.npz: the reference's own DQNBPP.embed_heightmap_and_sampled_point_cloud (model.py:316-352) run
on the CPU on a small seeded observation block, with the weights it ran on.  Data only: the non-stream weights (195 284
floats), the observation, the shape_feature the forward gathered and its two outputs.

    python tests/golden/make_embed_golden.py /path/to/the/reference

The reference's model.py is imported from where it lies.  Its `tools` module needs packages this project does not; model.py
takes one function from it, the usual three-line layer initialiser, which this script provides under that name.  That
initialiser zeroes every bias, so the biases are redrawn (seeded) before the forward: they are part of what is checked."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
S, BATCH, L, POINTS, N_SHAPES, TABLE_POINTS = 5, 3, 32, 64, 6, 200


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

    torch.manual_seed(20240607)
    np.random.seed(20240607)
    args = types.SimpleNamespace(selectedAction=S, atoms=31, level="item", heightMap=True, ZRotNum=8, bin_dimension=[0.32, 0.32, 0.3],
                                 resolutionH=0.01, bufferSize=1, hidden_size=128, noisy_std=0.5, device="cpu", samplePointsNum=POINTS)
    shape_array = torch.rand(N_SHAPES, TABLE_POINTS, 3) * 0.2
    net = reference_model.DQNBPP(args, S, shape_array)
    assert net.MapLength == L
    stages = (net.heightEncoder, net.shapeEncoder, net.init_candidate_embed, net.project_layer)
    with torch.no_grad():
        for seq in stages:
            for m in seq:
                if getattr(m, "bias", None) is not None:
                    m.bias.uniform_(-0.1, 0.1)

    rng = np.random.default_rng(7)
    obs = np.zeros((BATCH, 5 * S + 9 + L * L), dtype=np.float32)
    rows = obs[:, :5 * S].reshape(BATCH, S, 5)
    rows[:, :, :4] = rng.uniform(0.0, 0.32, (BATCH, S, 4))
    rows[:, :, 4] = np.array([[1, 0, 1, 1, 0], [0, 0, 0, 0, 0], [1, 1, 0, 1, 1]], dtype=np.float32)    # one bin all invalid
    obs[:, 5 * S] = [4, 0, 2]
    obs[:, 5 * S + 1:5 * S + 9] = rng.uniform(0.0, 1.0, (BATCH, 8))
    obs[:, 5 * S + 9:] = np.round(rng.uniform(0.0, 0.3, (BATCH, L * L)), 2)

    kept = {}
    handle = net.shapeEncoder.register_forward_hook(lambda mod, inp, out: kept.__setitem__("shape_feature", torch.max(out, dim=1)[0]))
    with torch.no_grad():
        embeddings, graph_embed = net.embed_heightmap_and_sampled_point_cloud(torch.from_numpy(obs.copy()))
    handle.remove()

    data = {"obs": obs, "shape_feature": kept["shape_feature"].numpy(), "embeddings": embeddings.numpy(), "graph_embed": graph_embed.numpy(),
            "selected_action": np.int32(S), "map_len": np.int32(L), "negative_slope": np.float32(0.01)}
    count = 0
    for name, seq in zip(("height_encoder", "shape_encoder", "init_candidate_embed", "project_layer"), stages):
        i = 0
        for m in seq:
            if getattr(m, "weight", None) is not None:
                data[f"{name}.{i}.weight"] = m.weight.detach().numpy()
                data[f"{name}.{i}.bias"] = m.bias.detach().numpy()
                count += m.weight.numel() + m.bias.numel()
                i += 1
    assert count == 195284
    np.savez(os.path.join(HERE, "embed_ref.npz"), **data)
    print("embed_ref.npz:", os.path.getsize(os.path.join(HERE, "embed_ref.npz")), "bytes;", count, "weights")


if __name__ == "__main__":
    main(sys.argv[1])
