"""replay.streams_logits_grad on CPU tensors: the four noisy layers of the value and advantage streams with the defined backward
("The noisy streams with a gradient"; csrc/irbpp_streams_grad.hip).

- replay's CPU backward (_streams_grad_backward_np, vectorised over everything but the chain) against the definition restated
  here with one explicit Python loop per chain and an fmaf of its own (exact rational arithmetic, rounded once), bit for bit.
- The definition against the reference's lines (NoisyLinear.forward, model.py:224-228; the streams, :393-394) restated with
  torch and run in float64 under autograd: each of the sixteen parameter gradients, dx and dxg within
  4 * max(e_ref, 2^-24 max|ref64|), e_ref the float32 torch run's own error against float64 (the rule of
  tests/test_shape_grad_cpu.py and tests/test_agent_golden_cpu.py).  The relu's side must not decide the comparison: every
  float64 pre-activation is asserted to satisfy |p| > 2^-18 max|p|; the seeds were picked so that no entry needs excluding.
- Training and eval mode, a detached x, grad sigma == fl(grad mu * eps), the forward's bits against streams_logits'."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay

f32, f64 = np.float32, np.float64
LAYERS = ("hv", "zv", "ha", "za")
PARAMS = ("weight_mu", "weight_sigma", "bias_mu", "bias_sigma")
NAMES = [f"{layer}_{p}" for layer in LAYERS for p in PARAMS]
SHAPES = [(1, 1, 1, 1, 2), (2, 3, 3, 5, 3), (3, 7, 12, 36, 31), (2, 65, 33, 17, 33)]         # (B, S, E, H, A)


class Noisy(torch.nn.Module):
    """the reference's NoisyLinear as far as the streams read it: four parameters, two buffers"""

    def __init__(self, rng, fan_in, fan_out, dtype=torch.float32):
        super().__init__()
        t = lambda *s: torch.from_numpy(rng.uniform(-1, 1, s).astype(f32)).to(dtype)          # noqa: E731
        bound = 1.0 / np.sqrt(fan_in)
        self.weight_mu = torch.nn.Parameter(t(fan_out, fan_in) * bound)
        self.weight_sigma = torch.nn.Parameter(t(fan_out, fan_in).abs() * 0.5 * bound + 0.01)
        self.bias_mu = torch.nn.Parameter(t(fan_out) * bound)
        self.bias_sigma = torch.nn.Parameter(t(fan_out).abs() * 0.5 * bound + 0.01)
        self.register_buffer("weight_epsilon", torch.from_numpy(rng.standard_normal((fan_out, fan_in)).astype(f32)).to(dtype))
        self.register_buffer("bias_epsilon", torch.from_numpy(rng.standard_normal(fan_out).astype(f32)).to(dtype))

    def forward(self, x):                                    # model.py:224-228
        if self.training:
            return torch.nn.functional.linear(x, self.weight_mu + self.weight_sigma * self.weight_epsilon,
                                              self.bias_mu + self.bias_sigma * self.bias_epsilon)
        return torch.nn.functional.linear(x, self.weight_mu, self.bias_mu)


def make_case(seed, B, S, E, H, A, device="cpu"):
    """-> (layers in fc_h_v, fc_z_v, fc_h_a, fc_z_a order, x, xg, gv, ga) as float32 torch tensors"""
    rng = np.random.default_rng(seed)
    layers = [Noisy(rng, E, H), Noisy(rng, H, A), Noisy(rng, E, H), Noisy(rng, H, A)]
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(f32))                       # noqa: E731
    x, xg, gv, ga = t(B, S, E), t(B, E), t(B, A), t(B, S, A)
    if device != "cpu":
        layers = [layer.to(device) for layer in layers]
        x, xg, gv, ga = (v.to(device) for v in (x, xg, gv, ga))
    return layers, x, xg, gv, ga


def effective(layers, training=True):
    """the eight effective arrays (StreamWeights' order) and the eight epsilons as float32 numpy arrays"""
    n = lambda v: v.detach().cpu().numpy().astype(f32)       # noqa: E731
    w, eps = [], []
    for layer in layers:
        if training:
            w += [n(layer.weight_mu) + n(layer.weight_sigma) * n(layer.weight_epsilon),
                  n(layer.bias_mu) + n(layer.bias_sigma) * n(layer.bias_epsilon)]
        else:
            w += [n(layer.weight_mu), n(layer.bias_mu)]
        eps += [n(layer.weight_epsilon), n(layer.bias_epsilon)]
    return w, (eps if training else None)


def run_wrapper(layers, x, xg, gv, ga, *, detach_x=False, training=None, **kw):
    """-> (v, a, {name: gradient as numpy or None}) through replay.streams_logits_grad and one backward"""
    for layer in layers:
        for p in layer.parameters():
            p.grad = None
    xr, xgr = x.clone().requires_grad_(not detach_x), xg.clone().requires_grad_(True)
    v, a = replay.streams_logits_grad(xr, xgr, *layers, training=training, **kw)
    assert v.grad_fn is not None and a.grad_fn is not None
    torch.autograd.backward([v, a], [gv, ga])
    n = lambda g: None if g is None else g.detach().cpu().numpy()                              # noqa: E731
    got = {"dx": n(xr.grad), "dxg": n(xgr.grad)}
    for lname, layer in zip(LAYERS, layers):
        for p in PARAMS:
            got[f"{lname}_{p}"] = n(getattr(layer, p).grad)
    return v.detach().cpu().numpy(), a.detach().cpu().numpy(), got


def same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == f32, what
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)


# ---- the definition with explicit loops -------------------------------------------------------------------------------------

def fma_exact(a, b, c):
    """fmaf on three float32 scalars in exact rational arithmetic, rounded once to the nearest float32, ties to even"""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:                                           # the sign of an exact zero: -0 only from (-0) + (-0)
        return f32(-0.0) if float(a) * float(b) == 0 and np.signbit(a) != np.signbit(b) and np.signbit(c) else f32(0.0)
    lo = f32(float(exact))                                   # a neighbour of the answer at worst
    cands = {lo, np.nextafter(lo, f32(np.inf)), np.nextafter(lo, f32(-np.inf))}
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.asarray(v, f32).view(np.uint32)) & 1))


def fma(a, b, c):
    """The same on Python floats, fast enough for the loops: the product of two float32 is exact in float64, the float64 sum
    is forced to round-to-odd by its exact error (TwoSum), and the rounding to float32 is then the only one."""
    a, b, c = float(a), float(b), float(c)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    if err != 0.0 and math.isfinite(s):
        bits = struct.unpack("<q", struct.pack("<d", s))[0]
        if bits & 1 == 0:
            s = struct.unpack("<d", struct.pack("<q", bits + (1 if (err > 0) == (s > 0) else -1)))[0]
    return f32(s)


def lin_loop(w, b, x):
    out = np.empty(w.shape[0], f32)
    for j in range(w.shape[0]):
        acc = f32(b[j])
        for k in range(w.shape[1]):
            acc = fma(x[k], w[j, k], acc)
        out[j] = acc
    return out


def stream_row_loop(x, w_h, b_h, w_z, g):
    H, E = w_h.shape
    p = lin_loop(w_h, b_h, x)
    h = np.array([v if v > 0 else f32(0) for v in p], f32)
    d, dx = np.empty(H, f32), np.empty(E, f32)
    for j in range(H):
        acc = f32(0)
        for t in range(w_z.shape[0]):
            acc = fma(g[t], w_z[t, j], acc)
        d[j] = acc if p[j] > 0 else f32(0)
    for k in range(E):
        acc = f32(0)
        for j in range(H):
            acc = fma(d[j], w_h[j, k], acc)
        dx[k] = acc
    return h, d, dx


def definition_loops(x, xg, w, eps, ga, gv):
    w_hv, b_hv, w_zv, b_zv, w_ha, b_ha, w_za, b_za = w
    B, S, E = x.shape
    H, A = w_ha.shape[0], w_za.shape[0]
    dx, dxg = np.zeros((B, S, E), f32), np.zeros((B, E), f32)
    ha, d = np.zeros((B, S, H), f32), np.zeros((B, S, H), f32)
    hv, dv = np.zeros((B, H), f32), np.zeros((B, H), f32)
    for b in range(B):
        hv[b], dv[b], dxg[b] = stream_row_loop(xg[b], w_hv, b_hv, w_zv, gv[b])
        for s in range(S):
            ha[b, s], d[b, s], dx[b, s] = stream_row_loop(x[b, s], w_ha, b_ha, w_za, ga[b, s])

    def two_level(left, right):                              # [B][S][R], [B][S][C] -> sum_b (chain over s)
        out = np.zeros((left.shape[2], right.shape[2]), f32)
        for r in range(left.shape[2]):
            for c in range(right.shape[2]):
                total = f32(0)
                for b in range(B):
                    acc = f32(0)
                    for s in range(S):
                        acc = fma(left[b, s, r], right[b, s, c], acc)
                    total = f32(total + acc)
                out[r, c] = total
        return out

    def two_level_bias(left):
        out = np.zeros(left.shape[2], f32)
        for r in range(left.shape[2]):
            total = f32(0)
            for b in range(B):
                acc = f32(0)
                for s in range(S):
                    acc = f32(acc + left[b, s, r])
                total = f32(total + acc)
            out[r] = total
        return out

    def chain_b(left, right):
        out = np.zeros((left.shape[1], right.shape[1]), f32)
        for r in range(left.shape[1]):
            for c in range(right.shape[1]):
                acc = f32(0)
                for b in range(B):
                    acc = fma(left[b, r], right[b, c], acc)
                out[r, c] = acc
        return out

    def sum_b(left):
        out = np.zeros(left.shape[1], f32)
        for b in range(B):
            out = (out + left[b]).astype(f32)
        return out

    dw = {"hv": (chain_b(dv, xg), sum_b(dv)), "zv": (chain_b(gv, hv), sum_b(gv)),
          "ha": (two_level(d, x), two_level_bias(d)), "za": (two_level(ga, ha), two_level_bias(ga))}
    grads = {}
    for i, layer in enumerate(LAYERS):
        grads[layer + "_weight_mu"], grads[layer + "_bias_mu"] = dw[layer]
        grads[layer + "_weight_sigma"] = None if eps is None else (dw[layer][0] * eps[2 * i]).astype(f32)
        grads[layer + "_bias_sigma"] = None if eps is None else (dw[layer][1] * eps[2 * i + 1]).astype(f32)
    return dx, dxg, grads


def test_fma_of_the_loops_is_replays():
    rng = np.random.default_rng(3)
    a, b, c = (rng.standard_normal(400).astype(f32) for _ in range(3))
    c[:50] = -(a[:50] * b[:50])                              # cancellation: the product's low bits decide
    a[50:60], c[50:60] = 0.0, -0.0
    got = np.array([fma(*t) for t in zip(a, b, c)], f32)
    same(got, np.array([fma_exact(*t) for t in zip(a, b, c)], f32), "the loops' fma against exact rational arithmetic")
    same(got, replay._fmaf_np(a, b, c), "replay's fma")


@pytest.mark.parametrize("B,S,E,H,A", SHAPES)
def test_cpu_backward_is_the_definition(B, S, E, H, A):
    layers, x, xg, gv, ga = make_case(100 + S, B, S, E, H, A)
    w, eps = effective(layers)
    n = lambda v: v.numpy()                                  # noqa: E731
    want = definition_loops(n(x), n(xg), w, eps, n(ga), n(gv))
    got = replay._streams_grad_backward_np(n(x), n(xg), w, eps, n(ga), n(gv))
    same(got[0], want[0], "dx")
    same(got[1], want[1], "dxg")
    for name in NAMES:
        same(got[2][name], want[2][name], name)
    # and through the wrapper
    _, _, through = run_wrapper(layers, x, xg, gv, ga)
    same(through["dx"], want[0], "dx")
    same(through["dxg"], want[1], "dxg")
    for name in NAMES:
        same(through[name], want[2][name], name)


def test_a_missing_gradient_counts_as_zeros():
    layers, x, xg, gv, ga = make_case(7, 2, 5, 6, 7, 4)
    w, eps = effective(layers)
    n = lambda v: v.numpy()                                  # noqa: E731
    full = replay._streams_grad_backward_np(n(x), n(xg), w, eps, n(ga), n(gv))
    only_a = replay._streams_grad_backward_np(n(x), n(xg), w, eps, n(ga), None)
    only_v = replay._streams_grad_backward_np(n(x), n(xg), w, eps, None, n(gv))
    same(only_a[0], full[0]), same(only_v[1], full[1])
    assert not only_a[1].any() and not only_v[0].any()
    for name in NAMES:
        if name.startswith(("ha", "za")):
            same(only_a[2][name], full[2][name], name)
            assert not only_v[2][name].any() and (name.endswith("sigma") or not np.signbit(only_v[2][name]).any())  # +0 * eps
        else:
            same(only_v[2][name], full[2][name], name)
            assert not only_a[2][name].any()


# ---- against the reference's lines in float64 -------------------------------------------------------------------------------

def reference(layers, x, xg, gv, ga, dtype):
    """NoisyLinear.forward and model.py:393-394 with torch in `dtype` under autograd -> ({name: gradient}, pre-activations)"""
    F = torch.nn.functional
    c = lambda v: v.detach().to(dtype)                       # noqa: E731
    P = [{p: c(getattr(layer, p)).requires_grad_(True) for p in PARAMS} for layer in layers]
    eff = [(q["weight_mu"] + q["weight_sigma"] * c(layer.weight_epsilon), q["bias_mu"] + q["bias_sigma"] * c(layer.bias_epsilon))
           for q, layer in zip(P, layers)]
    xr, xgr = c(x).requires_grad_(True), c(xg).requires_grad_(True)
    pv, pa = F.linear(xgr, *eff[0]), F.linear(xr, *eff[2])
    v, a = F.linear(F.relu(pv), *eff[1]), F.linear(F.relu(pa), *eff[3])
    torch.autograd.backward([v, a], [c(gv), c(ga)])
    out = {"dx": xr.grad, "dxg": xgr.grad}
    for lname, q in zip(LAYERS, P):
        for p in PARAMS:
            out[f"{lname}_{p}"] = q[p].grad
    return {k: t.cpu().numpy().astype(f64) for k, t in out.items()}, (pv.detach().cpu().numpy(), pa.detach().cpu().numpy())


def check_against_reference(got, layers, x, xg, gv, ga, label):
    ref64, pre = reference(layers, x, xg, gv, ga, torch.float64)
    ref32, _ = reference(layers, x, xg, gv, ga, torch.float32)
    for p in pre:                                            # the relu's side is the same in both precisions
        assert (np.abs(p) > 2.0 ** -18 * np.abs(p).max()).all(), "a pre-activation too close to the relu's corner: pick another seed"
    worst = {}
    for name in ["dx", "dxg"] + NAMES:
        e_ref = np.abs(ref32[name] - ref64[name]).max()
        scale = max(e_ref, 2.0 ** -24 * np.abs(ref64[name]).max())
        err = np.abs(got[name].astype(f64) - ref64[name]).max()
        worst[name] = err / scale
        print(f"{label} {name}: error {err:.3g}, e_ref {e_ref:.3g}, error / scale {err / scale:.3f}")
        assert err <= 4 * scale, f"{name}: error {err:.3g} beside 4 x {scale:.3g}"
    print(f"{label}: largest error / scale {max(worst.values()):.2f} ({max(worst, key=worst.get)})")
    return worst


@pytest.mark.parametrize("seed,B,S,E,H,A", [(11, 2, 3, 3, 5, 3), (12, 3, 7, 12, 36, 31), (11, 2, 65, 33, 17, 33), (11, 4, 50, 128, 128, 31)])
def test_definition_against_the_reference(seed, B, S, E, H, A):
    layers, x, xg, gv, ga = make_case(seed, B, S, E, H, A)
    _, _, got = run_wrapper(layers, x, xg, gv, ga)
    check_against_reference(got, layers, x, xg, gv, ga, f"({B},{S},{E},{H},{A})")


# ---- modes ------------------------------------------------------------------------------------------------------------------

def test_training_eval_and_a_detached_x():
    layers, x, xg, gv, ga = make_case(21, 2, 9, 12, 20, 5)
    v, a, got = run_wrapper(layers, x, xg, gv, ga)                             # training=None: no .training override -> module's True
    for lname, layer in zip(LAYERS, layers):
        n = lambda t: t.detach().numpy()                     # noqa: E731
        same(got[f"{lname}_weight_sigma"], got[f"{lname}_weight_mu"] * n(layer.weight_epsilon), lname)
        same(got[f"{lname}_bias_sigma"], got[f"{lname}_bias_mu"] * n(layer.bias_epsilon), lname)
    # forward bits: streams_logits' on the same effective weights
    sw = replay.StreamWeights(*layers, training=True)
    v0, a0 = replay.streams_logits(x, xg, sw)
    same(v, v0.numpy(), "v"), same(a, a0.numpy(), "a")
    # a detached x: no dx, everything else unchanged
    _, _, det = run_wrapper(layers, x, xg, gv, ga, detach_x=True)
    assert det["dx"] is None
    for name in ["dxg"] + NAMES:
        same(det[name], got[name], name)
    # eval mode: mu as the weights, no gradient for the sigmas; by the argument and by the modules' own flag
    for how in ("argument", "module"):
        if how == "module":
            for layer in layers:
                layer.eval()
        ve, ae, ev = run_wrapper(layers, x, xg, gv, ga, training=False if how == "argument" else None)
        sw = replay.StreamWeights(*layers, training=False)
        v0, a0 = replay.streams_logits(x, xg, sw)
        same(ve, v0.numpy(), "v eval"), same(ae, a0.numpy(), "a eval")
        w, _ = effective(layers, training=False)
        want = replay._streams_grad_backward_np(x.numpy(), xg.numpy(), w, None, ga.numpy(), gv.numpy())
        same(ev["dx"], want[0]), same(ev["dxg"], want[1])
        for name in NAMES:
            if name.endswith("sigma"):
                assert ev[name] is None and want[2][name] is None
            else:
                same(ev[name], want[2][name], name)


def test_only_one_output_used_and_the_limits():
    layers, x, xg, gv, ga = make_case(22, 2, 4, 6, 7, 3)
    _, _, full = run_wrapper(layers, x, xg, gv, ga)
    for layer in layers:
        for p in layer.parameters():
            p.grad = None
    xr = x.clone().requires_grad_(True)
    v, a = replay.streams_logits_grad(xr, xg, *layers)
    (a * ga).sum().backward()                                # v unused: its gradient arrives as None or zeros
    same(xr.grad.numpy(), full["dx"], "dx")
    same(layers[2].weight_mu.grad.numpy(), full["ha_weight_mu"])
    assert layers[0].weight_mu.grad is None or not layers[0].weight_mu.grad.any()
    with pytest.raises(ValueError):
        replay.streams_logits_grad(torch.zeros(1025, 1, 6), torch.zeros(1025, 6), *layers)
    with pytest.raises(ValueError):
        replay.streams_logits_grad(torch.zeros(2, 1025, 6), torch.zeros(2, 6), *layers)
    with pytest.raises(ValueError):
        replay.streams_logits_grad(x[:, :, :5], xg, *layers)
