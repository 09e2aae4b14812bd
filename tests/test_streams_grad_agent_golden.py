"""The learn step of tests/test_agent_golden_cpu.py with the noisy streams of the online forward taken by
replay.streams_logits_grad: two Agent.learn calls with update_target_net() between them, held to the reference's own Agent
(tests/golden/agent_ref.npz) with that file's ``check_learn`` and its bounds, nothing loosened.

The forward is built here from the fixture net's own modules (``forward`` below is agent_fixture.Net.forward with its last line
changed, the two-line change INTEGRATION.md shows) and put in the place of the fixture's for the duration of a test;
tests/agent_fixture.py itself is untouched.  On the CPU the numpy definition runs, forward and backward; the `gpu` variant runs
irbpp_streams_act and irbpp_streams_backward (use_hip=True), the rest of the step as in tests/test_gpu_agent_golden.py."""
import pytest

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
import agent_fixture as fx
from test_agent_golden_cpu import check_learn, learn_two_steps


def forward_with(use_hip):
    def forward(self, x, points, indices):
        e, e_global = self.embeddings(x, points, indices)
        v, a = replay.streams_logits_grad(e, e_global, self.fc_h_v, self.fc_z_v, self.fc_h_a, self.fc_z_a, use_hip=use_hip)
        assert tuple(v.shape) == (x.shape[0], self.atoms) and tuple(a.shape) == (x.shape[0], self.rows, self.atoms)
        return v, a
    return forward


def test_learn_two_steps_with_the_defined_streams(monkeypatch):
    monkeypatch.setattr(fx.Net, "forward", forward_with(None))
    steps, skipped = learn_two_steps("cpu", False)
    check_learn(steps, skipped, "cpu, streams_logits_grad")


@pytest.mark.gpu
def test_learn_two_steps_with_the_defined_streams_on_the_device(monkeypatch):
    monkeypatch.setattr(fx.Net, "forward", forward_with(True))
    steps, skipped = learn_two_steps("cuda:0", True)
    check_learn(steps, skipped, "gpu, streams_logits_grad")
