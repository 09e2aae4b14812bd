"""The learn step of tests/test_agent_golden_cpu.py with the shape branch of the online forward that carries the gradient
taken by replay.shape_features_grad: two Agent.learn calls with update_target_net() between them, held to the reference's own
Agent (tests/golden/agent_ref.npz) with that file's ``check_learn`` and its bounds, nothing loosened.

The forward is built here from the fixture net's own modules (``embeddings`` below is agent_fixture.Net.embeddings with one
line changed, the two-line change INTEGRATION.md shows) and put in the place of the fixture's for the duration of a test;
tests/agent_fixture.py itself is untouched.  On the CPU the numpy definition runs, forward and backward; the `gpu` variant
runs irbpp_shape_features_arg / irbpp_shape_features_backward (use_hip=True), the rest of the step as in
tests/test_gpu_agent_golden.py."""
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
import agent_fixture as fx
from test_agent_golden_cpu import check_learn, learn_two_steps


def embeddings_with(use_hip):
    def embeddings(self, x, points, indices):
        n, s, side = x.shape[0], self.rows, self.map_len
        rows = x[:, :5 * s].reshape(n, s, 5)
        fmap = self.heightEncoder(x[:, 5 * s + 9:].reshape(n, 1, side, side)).reshape(n, -1)
        shape_feature = replay.shape_features_grad(x[:, 5 * s], points, indices, self.shapeEncoder[0], self.shapeEncoder[2],
                                                   self.shapeEncoder[1].negative_slope, use_hip=use_hip)
        assert shape_feature.grad_fn is not None and tuple(shape_feature.shape) == (n, 128)
        cand = self.init_candidate_embed(rows[:, :, :4])
        joined = torch.cat((shape_feature[:, None, :].expand(n, s, -1), fmap[:, None, :].expand(n, s, -1), cand), dim=2)
        e = self.project_layer(joined)
        e = torch.where(rows[:, :, 4:5] == 1, e, torch.zeros((), dtype=e.dtype, device=e.device))
        return e, e.mean(1)
    return embeddings


def test_learn_two_steps_with_the_fused_shape_branch(monkeypatch):
    monkeypatch.setattr(fx.Net, "embeddings", embeddings_with(None))
    steps, skipped = learn_two_steps("cpu", False)
    check_learn(steps, skipped, "cpu, shape_features_grad")


@pytest.mark.gpu
def test_learn_two_steps_with_the_fused_shape_branch_on_the_device(monkeypatch):
    monkeypatch.setattr(fx.Net, "embeddings", embeddings_with(True))
    steps, skipped = learn_two_steps("cuda:0", True)
    check_learn(steps, skipped, "gpu, shape_features_grad")
