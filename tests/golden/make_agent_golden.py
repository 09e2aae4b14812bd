"""Writes tests/golden/agent_ref.npz: the reference's own Agent (agent.py, two DQNBPP of model.py) acting and learning on the
scenarios of tests/agent_fixture.py, run once as it is (float32) and once with both networks and the shape table in float64.

    python tests/golden/make_agent_golden.py /path/to/the/reference

The file holds no weights, no noise and no inputs: tests/agent_fixture.py regenerates them on both sides.  It holds, in
float64 from the float64 run: the expected values `sum_q_map` before masking and the actions of Agent.act (item network in
training and eval mode, each with the observation's mask and with mask=None; order network in both modes), and of two
Agent.learn calls with update_target_net() between them the per-sample loss, the gradient norm before the clip, and for every
parameter tensor the norms of its clipped gradient and of its update and both at up to 512 positions.  Beside every quantity
q stands `e_ref/q`, the largest difference between the two runs over the quantity: the reference's own float32 rounding
error.  The sample-point index draws of every forward (np.random.randint, recorded) and of the order network's
updateShapeArray are kept as integers.

The reference's modules are imported from where they lie; `tools` is replaced by the three-line layer initialiser model.py
takes from it.  The conditions at the end of `main` are asserted so that the tests need to leave no case out."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import agent_fixture as fx  # noqa: E402

SEED = 20240903


def _init(module, weight_init, bias_init, gain=1):
    weight_init(module.weight.data, gain=gain)
    bias_init(module.bias.data)
    return module


def tolerance(e_ref, ref64) -> float:
    """The tests' tolerance of a quantity (tests/test_agent_golden_cpu.py)."""
    return 4.0 * max(float(e_ref), 2.0 ** -24 * float(np.max(np.abs(ref64))))


class Memory(object):
    """What Agent.learn needs of a replay memory: the fixed batch, and a record of the priorities it hands back."""

    def __init__(self, dtype):
        states, actions, returns, next_states, nonterminals, weights = fx.learn_batch()
        t = lambda a: torch.from_numpy(a.copy()).to(dtype)  # noqa: E731
        self.batch = (np.arange(fx.B), t(states), torch.from_numpy(actions.copy()), t(returns), t(next_states), t(nonterminals), t(weights))
        self.priorities = []

    def sample(self, n):
        assert n == fx.B
        return self.batch

    def update_priorities(self, idxs, priorities):
        self.priorities.append(priorities.detach().double().numpy().copy())


def q_gaps(q, masks):
    """Per sample the gap between the best and the second-best admissible candidate of q [N, S] (inf with fewer than two).
    masks None: every row is admissible.  Rows given as one group (below) count as one candidate."""
    gaps = []
    for i in range(q.shape[0]):
        v = np.sort(q[i] if masks is None else q[i][np.asarray(masks[i]) == 1])[::-1]
        gaps.append(v[0] - v[1] if v.size >= 2 else np.inf)
    return np.array(gaps)


def unmasked_gaps(q, masks):
    """As q_gaps without a mask, the invalid rows of a sample counted as ONE candidate: their embeddings are all zero, so
    their values are the same number by construction (asserted), and the first of them wins on both sides."""
    gaps = []
    for i in range(q.shape[0]):
        m = np.asarray(masks[i]) == 1
        inv = q[i][~m]
        assert inv.size == 0 or np.all(inv == inv[0]), "rows with zero embeddings must have one value"
        v = np.sort(np.concatenate((q[i][m], inv[:1])))[::-1]
        gaps.append(v[0] - v[1] if v.size >= 2 else np.inf)
    return np.array(gaps)


def run(agent_module, dtype, level):
    """One run of the reference at `dtype` -> {name: array}."""
    draws = []
    real_randint = np.random.randint

    def randint(*a, **kw):
        out = real_randint(*a, **kw)
        draws.append(np.asarray(out).copy())
        return out

    order = level == "order"
    k = fx.K_ORDER if order else 1
    rows = k if order else fx.S
    table = fx.shape_table(level, fx.ORDER_TABLE_POINTS if order else fx.TABLE_POINTS)
    args = types.SimpleNamespace(
        action_space=rows, selectedAction=rows, atoms=fx.ATOMS, V_min=fx.V_MIN, V_max=fx.V_MAX, device="cpu", batch_size=fx.B,
        multi_step=fx.MULTI_STEP, discount=fx.DISCOUNT, norm_clip=fx.NORM_CLIP, shapeArray=table, model=None,
        learning_rate=fx.LEARNING_RATE, adam_eps=fx.ADAM_EPS, level=level, heightMap=True, ZRotNum=8, bin_dimension=[0.32, 0.32, 0.3],
        resolutionH=0.01, bufferSize=k, hidden_size=fx.HIDDEN, noisy_std=0.5, samplePointsNum=fx.POINTS)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    np.random.randint = randint
    norms = []
    real_clip = agent_module.clip_grad_norm_

    def clip(parameters, max_norm):
        total = real_clip(parameters, max_norm)
        norms.append(float(total))
        return total

    agent_module.clip_grad_norm_ = clip
    try:
        agent = agent_module.Agent(args)
        out = {}
        if order:
            out["resample"] = draws[0].astype(np.int16)          # the online network's updateShapeArray; the target's is draws[1]
            assert len(draws) == 2 and draws[0].shape == (10000,) and draws[0].max() < 2 ** 15
        del draws[:]
        fx.fill_parameters(agent.online_net)
        fx.fill_noise(agent.online_net, "online")
        agent.update_target_net()
        if dtype == torch.float64:
            for net in (agent.online_net, agent.target_net):
                net.double()
                net.shapeArray = net.shapeArray.double()
            agent.support = agent.support.double()
            agent.optimiser = torch.optim.Adam(agent.online_net.parameters(), lr=args.learning_rate, eps=args.adam_eps)
        step = [0]
        agent.target_net.reset_noise = lambda: fx.fill_noise(agent.target_net, f"target/{step[0]}")
        seen = []
        agent.online_net.register_forward_hook(lambda mod, inp, res: seen.append(res.detach().clone()))
        # sum_q_map as Agent.act and the double-Q selection of Agent.learn form it, in the run's own precision: the float32
        # run's products, its sum over the atoms and its rounded result are part of the reference's error
        expected = lambda p: (p * agent.support).sum(2).double().numpy()  # noqa: E731

        def act(name, state, masks):
            del seen[:], draws[:]
            mask = None if masks is None else torch.tensor(masks, dtype=dtype)
            action = agent.act(torch.from_numpy(state.copy()).to(dtype), mask)
            assert len(seen) == 1 and len(draws) == 1
            out[name + "/q"] = expected(seen[0])
            out[name + "/action"] = action.numpy().astype(np.int64)
            out[name + "/indices"] = draws[0].astype(np.int32)

        if order:
            state = fx.order_observations("order/act")
            agent.train()
            act("order/train", state, None)
            agent.eval()
            act("order/eval", state, None)
            return out
        state = fx.item_observations("item/act", fx.ACT_MASKS)
        for mode in ("train", "eval"):
            getattr(agent, mode)()
            act(f"item/{mode}/masked", state, fx.ACT_MASKS)
            act(f"item/{mode}/unmasked", state, None)
        agent.train()
        names = [n for n, _ in fx.tensor_names(agent.online_net)]
        out["tensors"] = np.array(names)
        for s in (1, 2):
            step[0] = s
            del seen[:], draws[:], norms[:]
            memory = Memory(dtype)
            before = [p.detach().double().clone() for _, p in fx.tensor_names(agent.online_net)]
            loss = agent.learn([memory])
            assert len(seen) == 2 and len(draws) == 3 and len(norms) == 1 and len(memory.priorities) == 1
            out[f"learn{s}/loss"] = loss.detach().double().numpy()
            assert np.array_equal(out[f"learn{s}/loss"], memory.priorities[0]), "update_priorities receives the loss"
            out[f"learn{s}/total_norm"] = np.float64(norms[0])
            out[f"learn{s}/indices"] = np.stack(draws).astype(np.int32)
            out[f"learn{s}/next_q"] = expected(seen[1])              # the double-Q selection's values
            out[f"learn{s}/a_star"] = out[f"learn{s}/next_q"].argmax(1).astype(np.int64)
            g_norm, u_norm, g_at, u_at = [], [], [], []
            for (name, p), old in zip(fx.tensor_names(agent.online_net), before):
                g, u = p.grad.detach().double().reshape(-1), (p.detach().double() - old).reshape(-1)
                at = torch.from_numpy(fx.positions(name, p.numel()))
                g_norm.append(float(g.norm())), u_norm.append(float(u.norm()))
                g_at.append(g[at].numpy()), u_at.append(u[at].numpy())
            out[f"learn{s}/grad_norm"], out[f"learn{s}/update_norm"] = np.array(g_norm), np.array(u_norm)
            out[f"learn{s}/grad_at"], out[f"learn{s}/update_at"] = np.concatenate(g_at), np.concatenate(u_at)
            if s == 1:
                agent.update_target_net()
        return out
    finally:
        np.random.randint = real_randint
        agent_module.clip_grad_norm_ = real_clip


PER_TENSOR = ("grad_norm", "update_norm")                # e_ref per tensor: every entry is a quantity of its own
SAMPLED = ("grad_at", "update_at")                       # e_ref per tensor: the largest over the tensor's positions


def main(reference_dir):
    tools = types.ModuleType("tools")
    tools.init = _init
    sys.modules["tools"] = tools
    sys.path.insert(0, reference_dir)
    import agent as agent_module

    torch.set_num_threads(1)                             # one summation order, whatever the machine
    data = {}
    for level in ("item", "order"):
        r32, r64 = run(agent_module, torch.float32, level), run(agent_module, torch.float64, level)
        assert r32.keys() == r64.keys()
        for key, ref in r64.items():
            if ref.dtype.kind in "iU":
                assert np.array_equal(ref, r32[key]), f"{key}: the two runs drew or chose differently"
                data[key] = ref
                continue
            diff = np.abs(r32[key].astype(np.float64) - ref)
            leaf = key.split("/")[-1]
            if leaf in SAMPLED:
                numel = {n: p.numel() for n, p in fx.tensor_names(fx.Net())}
                sizes = [fx.positions(str(n), numel[str(n)]).size for n in r64["tensors"]]
                e = np.array([d.max() for d in np.split(diff, np.cumsum(sizes)[:-1])])
            elif leaf in PER_TENSOR:
                e = diff
            else:
                e = np.float64(diff.max())
            data[key], data["e_ref/" + key] = ref, e

    # ---- the conditions the tests rely on -----------------------------------------------------------------------------------
    gap_over_tol = []

    def gaps_hold(key, gaps):
        tol = tolerance(data["e_ref/" + key], data[key])
        finite = gaps[np.isfinite(gaps)]
        assert finite.size and np.all(finite > 4 * tol), f"{key}: a gap of {finite.min():.3e} beside a tolerance of {tol:.3e}"
        gap_over_tol.append(finite.min() / tol)

    for mode in ("train", "eval"):
        gaps_hold(f"item/{mode}/masked/q", q_gaps(data[f"item/{mode}/masked/q"], fx.ACT_MASKS))
        gaps_hold(f"item/{mode}/unmasked/q", unmasked_gaps(data[f"item/{mode}/unmasked/q"], fx.ACT_MASKS))
        gaps_hold(f"order/{mode}/q", q_gaps(data[f"order/{mode}/q"], None))
    for s in (1, 2):
        gaps_hold(f"learn{s}/next_q", unmasked_gaps(data[f"learn{s}/next_q"], fx.NEXT_MASKS))
    assert any(sum(m) == 0 for m in fx.ACT_MASKS), "one bin has all candidates invalid"
    _, _, returns, _, nonterminals, _ = fx.learn_batch()
    assert (nonterminals == 0).any(), "one sample is terminal"
    support = np.linspace(fx.V_MIN, fx.V_MAX, fx.ATOMS).astype(np.float32).astype(np.float64)
    tz = returns.astype(np.float64)[:, None] + nonterminals.astype(np.float64) * fx.DISCOUNT ** fx.MULTI_STEP * support[None, :]
    assert (tz < fx.V_MIN).any() and (tz > fx.V_MAX).any(), "a Tz clamps at each end"
    b = (np.clip(tz, fx.V_MIN, fx.V_MAX) - fx.V_MIN) / ((fx.V_MAX - fx.V_MIN) / (fx.ATOMS - 1))
    inside = (tz > fx.V_MIN) & (tz < fx.V_MAX)
    assert (inside & (b == np.floor(b))).any(), "a Tz inside the support lands exactly on an atom"
    active = [bool(data[f"learn{s}/total_norm"] > fx.NORM_CLIP) for s in (1, 2)]
    assert sum(active) == 1, f"the clip is active in exactly one step: norms {data['learn1/total_norm']}, {data['learn2/total_norm']}"
    for s in (1, 2):                                     # and stays on its side of the clip within the tolerance
        assert abs(data[f"learn{s}/total_norm"] - fx.NORM_CLIP) > 4 * tolerance(data[f"e_ref/learn{s}/total_norm"], data[f"learn{s}/total_norm"])
        for name, norm in zip(data["tensors"], data[f"learn{s}/grad_norm"]):
            if str(name) in fx.ZERO_GRADIENT:            # zero in exact arithmetic: what is left is rounding
                assert norm <= 1e-9 * data[f"learn{s}/total_norm"], name
            else:
                assert norm > 1e-3 * data[f"learn{s}/total_norm"], f"{name}: every other parameter tensor has a gradient"
    data["norm_clip"] = np.float64(fx.NORM_CLIP)

    path = os.path.join(HERE, "agent_ref.npz")
    np.savez_compressed(path, **data)
    print("agent_ref.npz:", os.path.getsize(path), "bytes;", len(data), "arrays; total norms",
          float(data["learn1/total_norm"]), float(data["learn2/total_norm"]), "; smallest gap / tolerance", min(gap_over_tol))
    for key in sorted(k for k in data if k.startswith("e_ref/") and np.ndim(data[k]) == 0):
        print(f"  {key[6:]:28s} max|ref64| {np.max(np.abs(data[key[6:]])):.4e}  e_ref {float(data[key]):.3e}")


if __name__ == "__main__":
    main(sys.argv[1])
