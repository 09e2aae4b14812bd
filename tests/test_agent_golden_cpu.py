"""The composed product against the reference's own Agent (tests/golden/agent_ref.npz, written by
tests/golden/make_agent_golden.py from agent.py and model.py): Agent.act through network_greedy_action and
order_network_greedy_action, and two Agent.learn calls with update_target_net() between them through learn_loss, backward and
ClippedAdam, wired as INTEGRATION.md tells a caller to.  This file holds the driver and runs it with the exact CPU emulations
(use_hip=False); tests/test_gpu_agent_golden.py runs the same driver on the device.

Nothing is read but the golden and tests/agent_fixture.py, which regenerates the weights, the noise and the inputs on both
sides.  Per quantity the tolerance is 4 * max(e_ref, 2^-24 * max|ref64|), e_ref the reference's own float32 - float64
difference from the golden: the product's fmaf chains and torch's blocked GEMM are two float32 evaluations of one function
with different summation orders.  Actions are compared for equality on every sample: the generator asserts that every
arg-max's gap in ref64 is more than 4 tolerances (the smallest is 105).

A parameter tensor's four quantities (the norm of its clipped gradient, of its update, and both at its sampled positions) are
held to the tensor's own scale: 4 * max(e_ref_i, 2^-24 * max|ref64_i|, r * |ref64_i|), r = e_ref(total norm) / total norm, the
reference's relative error of the gradient as a whole (3.3e-6).  The third term is there because one tensor's e_ref is a single
draw of a rounding error and can be far below the error every float32 evaluation of that gradient has: it ranges from 5.9e-8
to 3.4e-6 of the norm among tensors that share one upstream rounding, and with the first two terms alone the CPU form stood at
21 e_ref on heightEncoder.4's gradient norm (e_ref 5.2e-9 on a norm of 8.9e-2) and 7.0 on fc_h_v.weight_sigma's update norm.

`fc_z_a.bias_mu` and `fc_z_a.bias_sigma` have a gradient of zero in exact arithmetic (the advantage stream's bias is the same
in every row and leaves with `a - a.mean(1)`): ref64 holds 1e-17, every float32 side the rounding of terms that cancel, 1e-9.
Relative to their own value no scale exists, so the third term is r * the gradient norm of `fc_z_a.weight_mu` (the terms that
cancel are the ones that form it) for the gradient, and for the update one rounding of the parameter, 2^-24 * max|p| per
element (sqrt(numel) of it for the norm): Adam turns a gradient of rounding noise into zero or one ulp of the parameter.

The clipped gradient compared here is the gradient after backward times clip_grad_norm_'s coefficient, which the driver forms
from the norm `ClippedAdam.step` returns: with grads="zero" the step leaves no gradient to read.  The product's own clip is
pinned by the update norms: the active clip scales by 0.9936, 6e-3 of an update norm against a bound of at most 1e-4 of it.
One update element alone moves by 1e-7 at most and would not show it.

Observed error / scale, the largest per group (the bound is 4), with this file's CPU forms and on an MI355X (chain and mfma
forms give the same bits; the learn rows are the largest over both steps and, per tensor, over the 32 or the 2 tensors):

                                                   CPU     MI355X
    act q, item train                            0.714     1.702
    act q, item eval                             1.134     1.517
    act q, order train                           1.053     1.053
    act q, order eval                            3.243     3.243
    learn double-Q values                        1.155     2.451
    learn loss                                   1.012     1.012
    learn total norm                             0.617     0.617
    learn grad norm per tensor                   1.046     1.072
    learn grad positions per tensor              1.136     1.228
    learn update norm per tensor                 1.076     1.361
    learn update positions per tensor            1.601     2.348
    the same four, zero-gradient tensors         0.828     0.319

The learn step's backward on the device is torch's and is not the same from run to run: another run of the same code gave 3.7
for step 2's double-Q values when their e_ref was still taken from probabilities summed in float64 (4.8 in one more run: the
generator now forms sum_q_map in each run's own precision, as the reference does, which is what the figures above use).

Each of these faults in the driver fails a test (tried on a copy): refresh() left out after step 1 (step 2's double-Q values,
4400 e_ref); StreamWeights(training=False) in train mode (act q and step 1's double-Q values, 35000 e_ref); step 1's target
noise reused in step 2 (step 2's loss, 865 e_ref); `weights` dropped (step 1's total norm, 171000 e_ref); no target copy
between the steps (the target equality check; the loss of step 2 behind it); indices redrawn (every act q and step 1's
double-Q values, 1000 .. 15000 e_ref).
"""
import functools
import os

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from irbpp_amd.optim import ClippedAdam
import agent_fixture as fx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agent_ref.npz")
FILL_VALUES, INTEGER_VALUES = [0.5244981646537781, 0.832623302936554, -0.8859636187553406], [84161, 77317]
RATIOS = {}                                              # group -> the largest error / e_ref seen (printed by the tests)


@functools.lru_cache(maxsize=None)
def gold():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def check(group: str, what: str, got, ref64, e_ref, floor: float = 0.0) -> None:
    """|got - ref64| <= 4 scale, scale = max(e_ref, 2^-24 max|ref64|, floor); keeps error / scale per group.  `floor` is 0
    for every quantity but a parameter tensor's (module docstring)."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape, f"{what}: shape {got.shape} beside {ref64.shape}"
    err = float(np.max(np.abs(got - ref64)))
    scale = max(float(e_ref), 2.0 ** -24 * float(np.max(np.abs(ref64))), float(floor), 1e-300)
    tol, ratio = 4.0 * scale, err / scale
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)
    assert np.isfinite(err) and err <= tol, f"{what}: error {err:.3e} beside a tolerance of {tol:.3e} (error / e_ref {ratio:.2f})"


def report(prefix: str) -> None:
    for group in sorted(RATIOS):
        print(f"{prefix} error / e_ref  {group:32s} {RATIOS[group]:.3f}")


# ---- the wiring of INTEGRATION.md ------------------------------------------------------------------------------------------
class Snapshots(object):
    """What a caller keeps beside one network: the three weight snapshots of its no-gradient forward."""

    def __init__(self, net, training: bool):
        self.shape = replay.ShapeEncoderWeights.from_layers(net.shapeEncoder[0], net.shapeEncoder[2])
        if net.buffer_size > 1:
            self.front = replay.OrderEmbedWeights.from_layers(net.heightEncoder, net.gat_project_layer, net.embedder)
        else:
            self.front = replay.EmbedWeights.from_layers(net.heightEncoder, net.init_candidate_embed, net.project_layer)
        self.streams = replay.StreamWeights.from_layers(net.fc_h_v, net.fc_z_v, net.fc_h_a, net.fc_z_a, training=training)

    def refresh(self) -> None:
        self.shape.refresh(), self.front.refresh(), self.streams.refresh()

    def logits(self, x, points, indices, use_hip, embed_form, streams_form):
        """A no_grad forward of `learn`: shape_features -> embed -> streams_logits."""
        sf = replay.shape_features(x[:, 5 * fx.S], points, indices, self.shape, use_hip=use_hip)
        e, e_global = replay.embed(x, sf, self.front, use_hip=use_hip, form=embed_form)
        return replay.streams_logits(e, e_global, self.streams, use_hip=use_hip, form=streams_form)


def support_on(dev):
    return torch.linspace(fx.V_MIN, fx.V_MAX, fx.ATOMS).to(dev)


@functools.lru_cache(maxsize=None)
def acting(level: str, mode: str, dev: str):
    """-> (points, snapshots of the online network in `mode`): shared by the act tests, which change none of it."""
    g = gold()
    online, _ = fx.make_nets(fx.K_ORDER if level == "order" else 1, dev)
    getattr(online, mode)()
    if level == "order":                                 # updateShapeArray's resampled table, from its recorded draw
        table = fx.shape_table("order", fx.ORDER_TABLE_POINTS)[:, g["resample"].astype(np.int64)]
    else:
        table = fx.shape_table("item", fx.TABLE_POINTS)
    return replay.ShapePoints(table, dev), Snapshots(online, training=online.training)


def act_item(dev: str, use_hip: bool, mode: str, masked: bool, embed_form: str = "chain", streams_form: str = "chain"):
    """Agent.act(state, mask) / Agent.act(state, None) of the item network -> (q float32 [B, S] before masking, actions)."""
    points, w = acting("item", mode, dev)
    name = f"item/{mode}/{'masked' if masked else 'unmasked'}"
    state = torch.from_numpy(fx.item_observations("item/act", fx.ACT_MASKS)).to(dev)
    indices = torch.from_numpy(gold()[name + "/indices"]).to(dev)
    q = torch.full((fx.B, fx.S), float("nan"), dtype=torch.float32, device=dev)
    action = replay.network_greedy_action(state, points, indices, w.shape, w.front, w.streams, support_on(dev), q_out=q,
                                          use_hip=use_hip, streams_form=streams_form, embed_form=embed_form, mask=masked)
    return q.cpu().numpy(), action.cpu().numpy()


def act_order(dev: str, use_hip: bool, mode: str, order_form: str = "chain", streams_form: str = "chain"):
    """orderDQN.act(orderState, None) -> (q float32 [B, k], actions)."""
    points, w = acting("order", mode, dev)
    state = torch.from_numpy(fx.order_observations("order/act")).to(dev)
    indices = torch.from_numpy(gold()[f"order/{mode}/indices"]).to(dev)
    q = torch.full((fx.B, fx.K_ORDER), float("nan"), dtype=torch.float32, device=dev)
    action = replay.order_network_greedy_action(state, points, indices, w.shape, w.front, w.streams, support_on(dev), q_out=q,
                                                use_hip=use_hip, streams_form=streams_form, order_form=order_form)
    return q.cpu().numpy(), action.cpu().numpy()


def learn_two_steps(dev: str, use_hip: bool, embed_form: str = "chain", streams_form: str = "chain"):
    """Agent.learn, agent.update_target_net(), Agent.learn -> per step a dict of what the golden holds, and the optimiser's
    skipped-step count."""
    g = gold()
    online, target = fx.make_nets(1, dev)
    points = replay.ShapePoints(fx.shape_table("item", fx.TABLE_POINTS), dev)
    w_online, w_target = Snapshots(online, training=True), Snapshots(target, training=True)
    support = support_on(dev)
    optimiser = ClippedAdam(online.parameters(), fx.LEARNING_RATE, (0.9, 0.999), fx.ADAM_EPS, fx.NORM_CLIP, grads="zero",
                            target_params=target.parameters(), use_hip=use_hip)
    states, actions, returns, next_states, nonterminals, weights = (torch.from_numpy(a).to(dev) for a in fx.learn_batch())
    batch = (None, states, actions, returns, next_states, nonterminals, weights)
    named = fx.tensor_names(online)
    steps = []
    for s in (1, 2):
        indices = torch.from_numpy(g[f"learn{s}/indices"]).to(dev)             # the three forwards' draws, in the reference's order
        fx.fill_noise(target, f"target/{s}")                                   # target_net.reset_noise() (agent.py:94) ...
        w_target.streams.refresh()                                             # ... and the refresh that follows every reset_noise
        kept = {}

        def online_logits(x):
            if x is states:
                return online(x, points, indices[0])                           # the forward that carries the gradient: torch's
            kept["next"] = w_online.logits(x, points, indices[1], use_hip, embed_form, streams_form)
            return kept["next"]

        def target_logits(x):
            return w_target.logits(x, points, indices[2], use_hip, embed_form, streams_form)

        before = [p.detach().clone() for _, p in named]
        loss = replay.learn_loss(online_logits, target_logits, batch, support, fx.DISCOUNT ** fx.MULTI_STEP, fx.V_MIN, fx.V_MAX,
                                 use_hip=use_hip)
        (weights * loss).mean().backward()                                     # into the zeros the last step left
        grads = [p.grad.detach().double().cpu().numpy().reshape(-1).copy() for _, p in named]
        total = float(optimiser.step(sync_target=s == 1))                      # update_target_net() follows the first learn
        w_online.refresh()                                                     # after every optimiser step
        if s == 1:
            w_target.refresh()                                                 # the target's parameters were just written
        coef = min(1.0, fx.NORM_CLIP / (total + 1e-6))                         # clip_grad_norm_'s, from the norm the step returned
        next_q = torch.full((fx.B, fx.S), float("nan"), dtype=torch.float32, device=dev)    # the double-Q selection, from the logits learn_loss saw
        a_star = replay.dueling_greedy_action(*kept["next"], support, None, q_out=next_q, use_hip=use_hip)
        steps.append({
            "loss": loss.detach().cpu().numpy(), "total_norm": total, "a_star": a_star.cpu().numpy(),
            "next_logits": [t.cpu().numpy() for t in kept["next"]], "next_q": next_q.cpu().numpy(),
            "grads": [gr * coef for gr in grads],
            "updates": [(p.detach().double() - old.double()).cpu().numpy().reshape(-1) for (_, p), old in zip(named, before)],
            "param_max": [float(old.abs().max()) for old in before],
            "zeroed": all(not bool(p.grad.any()) for _, p in named),
            "target_equal": all(torch.equal(p, q) for (_, p), q in zip(named, target.parameters()))})
    return steps, optimiser.skipped()


def check_learn(steps, skipped, prefix: str) -> None:
    g = gold()
    names = [str(n) for n in g["tensors"]]
    assert skipped == 0
    assert steps[0]["target_equal"] and not steps[1]["target_equal"], "the target is copied after the first step only"
    for s, got in zip((1, 2), steps):
        key = f"learn{s}/"
        assert np.array_equal(got["a_star"], g[key + "a_star"]), f"step {s}: the double-Q arg-max"
        check("learn double-Q values", f"step {s} online values of next_states", got["next_q"], g[key + "next_q"], g["e_ref/" + key + "next_q"])
        check("learn loss", f"step {s} loss", got["loss"], g[key + "loss"], g["e_ref/" + key + "loss"])
        check("learn total norm", f"step {s} total norm", got["total_norm"], g[key + "total_norm"], g["e_ref/" + key + "total_norm"])
        assert (got["total_norm"] > fx.NORM_CLIP) == (float(g[key + "total_norm"]) > fx.NORM_CLIP)
        assert got["zeroed"], "grads='zero' leaves zeros for the next backward"
        at = [fx.positions(n, arr.size) for n, arr in zip(names, got["grads"])]
        offsets = np.concatenate(([0], np.cumsum([a.size for a in at])))
        relative = float(g["e_ref/" + key + "total_norm"]) / float(g[key + "total_norm"])      # of the gradient as a whole
        sibling = g[key + "grad_norm"][names.index("fc_z_a.weight_mu")]
        for kind, arrays in (("grad", got["grads"]), ("update", got["updates"])):
            for i, (n, arr) in enumerate(zip(names, arrays)):
                ref_norm, ref_at = g[f"{key}{kind}_norm"][i], g[f"{key}{kind}_at"][offsets[i]:offsets[i + 1]]
                floor_norm, floor_at, tag = relative * ref_norm, relative * float(np.max(np.abs(ref_at))), ""
                if n in fx.ZERO_GRADIENT:                # rounding of terms that cancel (module docstring)
                    tag = " (zero gradient)"
                    floor_at = relative * sibling if kind == "grad" else 2.0 ** -24 * got["param_max"][i]
                    floor_norm = floor_at * (1.0 if kind == "grad" else np.sqrt(arr.size))
                check(f"learn {kind} norm per tensor" + tag, f"step {s} {kind} norm of {n}", np.sqrt(np.sum(arr * arr)), ref_norm,
                      g[f"e_ref/{key}{kind}_norm"][i], floor_norm)
                check(f"learn {kind} positions per tensor" + tag, f"step {s} {kind} of {n} at its positions", arr[at[i]], ref_at,
                      g[f"e_ref/{key}{kind}_at"][i], floor_at)
    report(prefix)


# ---- the tests ----------------------------------------------------------------------------------------------------------------
def test_the_fill_is_the_same_on_every_machine():
    """Three values of `fill` and one of `integers` written out: a change of the hash would silently move both sides."""
    v = fx.fill("fc_h_v.weight_mu", (2, 3), 1.0)
    assert v.dtype == np.float32 and v.shape == (2, 3)
    assert [float(x) for x in v.reshape(-1)[:3]] == FILL_VALUES
    assert fx.integers("positions/project_layer.0", (2,), 131072).tolist() == INTEGER_VALUES


def test_golden_is_sane():
    """ref32 beside ref64: every e_ref is finite and below 1e-3 of its quantity (the float64 run computes the same function),
    the zero-gradient tensors' norms are rounding beside the total, the clip is active in exactly one step."""
    g = gold()
    names = [str(n) for n in g["tensors"]]
    assert names == [n for n, _ in fx.tensor_names(fx.Net())], "Net's parameter tensors are the reference's, in its order"
    for key in (k for k in g if k.startswith("e_ref/")):
        e, ref = g[key], g[key[6:]]
        assert np.all(np.isfinite(e)) and np.all(e >= 0)
        if e.ndim == 0:
            assert e <= 1e-3 * np.max(np.abs(ref)), key
        elif key.endswith("_norm"):
            for i, n in enumerate(names):
                if n in fx.ZERO_GRADIENT:
                    assert "update" in key or ref[i] <= 1e-9 * g[key[6:].split("/")[0] + "/total_norm"], (key, n)
                else:
                    assert e[i] <= 1e-3 * ref[i] and ref[i] > 0, (key, n)
        elif key.endswith("_at"):
            norms = g[key[6:-3] + "_norm"]
            for i, n in enumerate(names):
                assert n in fx.ZERO_GRADIENT or e[i] <= 1e-3 * norms[i], (key, n)
    active = [float(g[f"learn{s}/total_norm"]) > fx.NORM_CLIP for s in (1, 2)]
    assert sum(active) == 1 and float(g["norm_clip"]) == fx.NORM_CLIP


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_item_act(mode, masked):
    g = gold()
    name = f"item/{mode}/{'masked' if masked else 'unmasked'}"
    q, action = act_item("cpu", False, mode, masked)
    check(f"act q, item {mode}", name, q, g[name + "/q"], g["e_ref/" + name + "/q"])
    assert np.array_equal(action, g[name + "/action"])
    report("cpu")


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_order_act(mode):
    g = gold()
    q, action = act_order("cpu", False, mode)
    check(f"act q, order {mode}", f"order/{mode}", q, g[f"order/{mode}/q"], g[f"e_ref/order/{mode}/q"])
    assert np.array_equal(action, g[f"order/{mode}/action"])
    report("cpu")


def test_learn_two_steps():
    steps, skipped = learn_two_steps("cpu", False)
    check_learn(steps, skipped, "cpu")
