"""The driver of tests/test_agent_golden_cpu.py on the device: Agent.act and two Agent.learn calls of the reference's own
Agent (tests/golden/agent_ref.npz) through the kernels, use_hip=True throughout.  Reads only the golden and
tests/agent_fixture.py.  Quantities, tolerances and the observed error / e_ref: that file's docstring.

Act runs every accepted combination of form="chain" | "mfma" for embed_form / order_form and streams_form; the forms must
agree bit for bit, the order network's also with the CPU form, which is the same defined arithmetic to the end.  Learn runs
with the chain forms and with the mfma forms in its no_grad forwards, whose logits must be the same bits (the forward with the
gradient and the backward are torch's, which promises no bits).  B = 6, S = 5."""
import itertools

import numpy as np
import pytest

from test_agent_golden_cpu import act_item, act_order, check, check_learn, gold, learn_two_steps, report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = list(itertools.product(("chain", "mfma"), ("chain", "mfma")))


def same_bits(a, b) -> bool:
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_item_act(mode, masked):
    g = gold()
    name = f"item/{mode}/{'masked' if masked else 'unmasked'}"
    first = None                                         # (the CPU form of the item head ends in torch's softmax: not these bits)
    for embed_form, streams_form in FORMS:
        q, action = act_item(DEV, True, mode, masked, embed_form, streams_form)
        check(f"act q, item {mode}", f"{name} ({embed_form}, {streams_form})", q, g[name + "/q"], g["e_ref/" + name + "/q"])
        assert np.array_equal(action, g[name + "/action"]), (embed_form, streams_form)
        first = q if first is None else first
        assert same_bits(q, first), f"embed_form {embed_form}, streams_form {streams_form}: other bits than (chain, chain)"
    report("gpu")


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_order_act(mode):
    g = gold()
    q_cpu, _ = act_order("cpu", False, mode)
    for order_form, streams_form in FORMS:
        q, action = act_order(DEV, True, mode, order_form, streams_form)
        check(f"act q, order {mode}", f"order/{mode} ({order_form}, {streams_form})", q, g[f"order/{mode}/q"], g[f"e_ref/order/{mode}/q"])
        assert np.array_equal(action, g[f"order/{mode}/action"]), (order_form, streams_form)
        assert same_bits(q, q_cpu), f"order_form {order_form}, streams_form {streams_form}: other bits than the definition"
    report("gpu")


def test_learn_two_steps():
    chain, skipped = learn_two_steps(DEV, True, "chain", "chain")
    check_learn(chain, skipped, "gpu")
    mfma, skipped = learn_two_steps(DEV, True, "mfma", "mfma")
    check_learn(mfma, skipped, "gpu")
    for a, b in zip(chain[:1], mfma[:1]):                # step 1 starts from the same parameters in both runs
        assert all(same_bits(x, y) for x, y in zip(a["next_logits"], b["next_logits"]))
