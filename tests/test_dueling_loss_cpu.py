"""The dueling C51 loss (csrc/irbpp_dueling_loss.hip, replay.dueling_c51_loss / learn_loss) without a GPU.

The kernels' arithmetic is defined (the header of irbpp_dueling_loss.hip); this file carries that definition as numpy float32
code (``dlog_np``, ``dueling_loss_np``, ``dueling_loss_backward_np``: tests/test_gpu_dueling_loss.py and
tests/test_dueling_loss_kernel_on_host.py hold the kernels to it bit for bit; the mean and the exponential are those of
tests/test_dueling_cpu.py) and checks the definition itself:

* ``dlog_np`` against float64 log within the figures of the full sweep (tools/dlog_sweep.py,
  profiles/dueling_loss/dlog_sweep.json);
* the definition against the reference's torch lines (model.py:395-398 with log=True, agent.py:85-86, 117-119) evaluated in
  float64, loss and both gradients, within the bounds derived in ``loss_bounds`` below;
* identities of the definition that hold bit for bit;
* the wrappers' CPU form and the IRBPP_ERR_ARG limits of the two entry points (checked before any HIP call)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_c51_cpu import learn_torch
from test_dueling_cpu import DEXP_MAX_ULP, LN2_HI, LN2_LO, PARTS, U, dexp_np, f32, mean_np

SQRT2 = f32(1.4142135623730951)
DLOG_COEF = [f32(c) for c in (9.0909090909090912e-02, 1.1111111111111111e-01, 1.4285714285714285e-01, 2.0000000000000001e-01,
                              3.3333333333333331e-01)]
SWEEP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "dueling_loss", "dlog_sweep.json")
DLOG_MAX_ABS = 2.965e-07                                 # the full sweep: 2.96477e-07 at d = 90.2249 (profiles/dueling_loss/)
DLOG_MAX_ULP = 1.9684                                    # the full sweep: 1.96836 ulp at d = 1.00386


# ------------------------------------------------------------------ the definition, in numpy float32 ------------
def dlog_np(d):
    """dueling_dlog: float32 [...] in [1, 128] -> float32."""
    d = np.array(d, dtype=f32)                           # (a C-ordered copy: the bits are viewed)
    bits = d.view(np.uint32)
    n = (bits >> 23).astype(np.int32) - 127
    f = ((bits & np.uint32(0x007fffff)) | np.uint32(0x3f800000)).view(f32)
    big = f > SQRT2
    f = np.where(big, f * f32(0.5), f)
    nf = (n + big).astype(f32)
    s = (f - f32(1)) / (f + f32(1))
    z = s * s
    p = np.full(d.shape, DLOG_COEF[0], dtype=f32)
    for c in DLOG_COEF[1:]:
        p = p * z + c
    s2 = s + s
    lf = s2 + s2 * (z * p)
    out = nf * LN2_HI + (lf + nf * LN2_LO)
    assert out.dtype == f32
    return out


def wrap_actions(actions, s):
    """-> (row index with [-S, 0) counted from the end, valid [B])"""
    r = np.asarray(actions, dtype=np.int64)
    r = np.where(r < 0, r + s, r)
    return r, (r >= 0) & (r < s)


def dueling_loss_np(v, a, actions, m):
    """v [B, atoms], a [B, S, atoms], actions int64 [B], m [B, atoms] -> (loss float32 [B], g float32 [B, atoms])."""
    v, a, m = np.asarray(v, dtype=f32), np.asarray(a, dtype=f32), np.asarray(m, dtype=f32)
    b, s, atoms = a.shape
    r, ok = wrap_actions(actions, s)
    row = a[np.arange(b), np.where(ok, r, 0)]
    x = (v + row) - mean_np(a)
    t = x - x.max(-1, keepdims=True)
    e = dexp_np(t)
    den = e[:, 0]
    for k in range(1, atoms):
        den = den + e[:, k]
    lp = t - dlog_np(den)[:, None]
    loss, big_m = m[:, 0] * lp[:, 0], m[:, 0]
    for k in range(1, atoms):
        loss = loss + m[:, k] * lp[:, k]
        big_m = big_m + m[:, k]
    g = (e / den[:, None]) * big_m[:, None] - m
    loss, g = np.where(ok, -loss, f32(np.nan)), np.where(ok[:, None], g, f32(0))
    assert loss.dtype == f32 and g.dtype == f32
    return loss, g


def dueling_loss_backward_np(g, w, actions, s):
    """g [B, atoms], w [B], actions -> (grad_v float32 [B, atoms], grad_a float32 [B, S, atoms])."""
    g, w = np.asarray(g, dtype=f32), np.asarray(w, dtype=f32)
    b, atoms = g.shape
    r, ok = wrap_actions(actions, s)
    gw = w[:, None] * g
    c = gw / f32(s)
    grad_a = np.repeat((-c)[:, None, :], s, axis=1)
    hit = np.arange(b)[ok]
    grad_a[hit, r[ok]] = (gw - c)[hit]
    assert gw.dtype == f32 and grad_a.dtype == f32
    return gw, grad_a


# ------------------------------------------------------------------ the reference's lines, in torch ------------
def loss_torch(v, a, actions, m):
    """model.py:395-398 (log=True), agent.py:86 and 117."""
    atoms, action_space = v.shape[-1], a.shape[1]
    v, a = v.view(-1, 1, atoms), a.view(-1, action_space, atoms)
    q = v + a - a.mean(1, keepdim=True)
    log_ps = F.log_softmax(q, dim=2)
    log_ps_a = log_ps[range(a.shape[0]), actions]
    return -torch.sum(m * log_ps_a, 1)


def reference64(v, a, actions, m, w):
    """-> (loss, grad_v, grad_a) of the reference's lines in float64, the gradients from (w * loss).sum().backward()."""
    d = lambda x: torch.from_numpy(np.asarray(x)).double()          # noqa: E731
    v64, a64 = d(v).requires_grad_(), d(a).requires_grad_()
    loss = loss_torch(v64, a64, torch.from_numpy(np.asarray(actions)), d(m))
    (d(w) * loss).sum().backward()
    return loss.detach().numpy(), v64.grad.numpy(), a64.grad.numpy()


# ------------------------------------------------------------------ dlog ------------
def dlog_errors(d):
    """(absolute error, error in ulp of the float32 nearest the true value) of dlog_np against float64 log of the float32 d."""
    d = np.asarray(d, dtype=f32)
    want = np.log(d.astype(np.float64))
    err = np.abs(dlog_np(d).astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ulp = np.where(want > 0, err / np.spacing(want.astype(f32)).astype(np.float64), err * 0)
    return err, ulp


def test_dlog_special_arguments():
    assert dlog_np(f32(1.0)) == 0.0 and not np.signbit(dlog_np(f32(1.0)))
    pw = np.array([2.0 ** k for k in range(8)], dtype=f32)
    fold = np.concatenate([(np.arange(-8, 9).astype(np.int64) + int((SQRT2 * f32(2.0 ** k)).view(np.uint32))).astype(np.uint32).view(f32)
                           for k in range(7)])
    near = np.concatenate([np.nextafter(pw[1:], f32(0)), np.nextafter(pw[:-1], f32(200))])
    with open(SWEEP) as fh:
        sweep = json.load(fh)
    assert sweep["arguments"] == 58720257 and sweep["max_abs"] <= DLOG_MAX_ABS and sweep["max_ulp"] <= DLOG_MAX_ULP
    assert sweep["min_result"] == 0.0
    worst = np.array([sweep["max_abs_at"], sweep["max_ulp_at"]], dtype=f32)
    for d in (pw, fold, near, worst):
        assert d.min() >= 1 and d.max() <= 128
        err, ulp = dlog_errors(d)
        assert err.max() <= DLOG_MAX_ABS and ulp.max() <= DLOG_MAX_ULP
        assert np.isfinite(dlog_np(d)).all() and (dlog_np(d) >= 0).all()
    err, ulp = dlog_errors(worst)
    assert err[0] == pytest.approx(sweep["max_abs"], rel=1e-6) and ulp[1] == pytest.approx(sweep["max_ulp"], rel=1e-6)


def test_dlog_stratified_sample_stays_within_the_sweep():
    """2^20 + arguments: 8192 equal strata of the bit patterns of [1, 128] x 136 fixed offsets each, both ends included."""
    lo, hi = int(f32(1.0).view(np.uint32)), int(f32(128.0).view(np.uint32))
    strata, per = 8192, 136
    width = (hi - lo) // strata
    offs = (np.arange(per, dtype=np.int64) * 2654435761 + 12345) % width
    bits = np.concatenate([(lo + np.arange(strata, dtype=np.int64)[:, None] * width + offs[None, :]).ravel(), [lo, hi]])
    assert len(bits) >= 2 ** 20 and bits.max() <= hi
    d = bits.astype(np.uint32).view(f32)
    err, ulp = dlog_errors(d)
    assert err.max() <= DLOG_MAX_ABS, f"{err.max()} at d = {d[err.argmax()]!r}"
    assert ulp.max() <= DLOG_MAX_ULP, f"{ulp.max()} ulp at d = {d[ulp.argmax()]!r}"
    out = dlog_np(d)
    assert np.isfinite(out).all() and out.min() >= 0


# ------------------------------------------------------------------ the definition against the reference ------------
def loss_bounds(v, a, m, w):
    """Bounds on |definition - exact| for the loss, grad_v and grad_a (the float64 torch lines stand for exact; u = 2^-24,
    first-order terms times 1.02 for the higher orders, every term far below 1), continuing ``bounds`` of test_dueling_cpu.py:

    x:  dx <= (ceil(S/16) + 19) u (V + A) as there (V = max|v|, A = max|a|).
    t = x - mx: both operands carry dx, the subtraction rounds within u |t| and |t| <= T = 2 (V + 2A): dt <= 2 dx + u T.
    e:  where t >= -80 the subtraction rounds within 80 u, so ee = 2 dx + 80 u + 2 DEXP_MAX_ULP u relatively; below the
        cut-off e is 0 instead of at most exp(-80) < 2e-35 absolutely.
    den: atoms non-negative terms, atoms - 1 additions, den >= 1: relative ed = ee + (atoms - 1) u, + 2e-35 atoms.
    L = dlog(den): log(den (1 + ed)) = log(den) + ed to first order, and dlog is within DLOG_MAX_ABS of the logarithm of
        its float32 argument: dL <= 1.02 ed + 2e-35 atoms + DLOG_MAX_ABS.
    lp = t - L: rounds within u LP with |lp| <= LP = T + log(atoms): dlp <= dt + dL + u LP.
    loss: atoms products m lp, each within u m LP, and atoms - 1 additions of partial sums no larger than Ms LP with
        Ms = sum m: dloss <= Ms (dlp + 1.02 atoms u LP).
    p = e / den: relative ep = 2 ee + atoms u, p <= 1: |dp| <= 1.02 ep + 2e-35.
    g = p M - m: M = sum m in atoms - 1 additions (relative (atoms - 1) u), the product and the subtraction round within
        u Ms each: dg <= Ms (|dp| + 1.02 (atoms + 1) u).  The exact derivative of the reference's loss with respect to x[k]
        is p[k] sum(m) - m[k], so this is also the distance from autograd's.
    gw = w g rounds within u |w| Ms: dgw <= W (dg + u Ms), W = max|w|: the bound on grad_v (d x / d v = 1).
    c = gw / S: dc <= (dgw + u W Ms) / S.  grad_a is gw - c in the action's row (one more rounding, u W Ms) and -c elsewhere
        (d x[k] / d a[s][k] = [s == r] - 1 / S): dga <= dgw + dc + u W Ms."""
    s, atoms = a.shape[1], a.shape[2]
    V, A = float(np.abs(v).max()), float(np.abs(a).max())
    Ms, W = float(np.asarray(m, dtype=np.float64).sum(-1).max()), float(np.abs(w).max())
    T = 2 * (V + 2 * A)
    dx = (-(-s // PARTS) + 19) * U * (V + A)
    dt = 2 * dx + U * T
    ee = 2 * dx + 80 * U + 2 * DEXP_MAX_ULP * U
    ed = ee + (atoms - 1) * U
    dL = 1.02 * ed + 2e-35 * atoms + DLOG_MAX_ABS
    LP = T + float(np.log(atoms))
    dlp = dt + dL + U * LP
    dloss = Ms * (dlp + 1.02 * atoms * U * LP)
    dp = 1.02 * (2 * ee + atoms * U) + 2e-35
    dg = Ms * (dp + 1.02 * (atoms + 1) * U)
    dgw = W * (dg + U * Ms)
    dc = (dgw + U * W * Ms) / s
    return dloss, dgw, dgw + dc + U * W * Ms


def loss_inputs(rng, b, s, atoms, scale=1.0):
    """v, a standard normal times `scale`; actions over the rows, a few of them negative; m a random distribution with exact
    zeros, every third sample's scaled so that it does not sum to 1; w positive importance weights."""
    v = (scale * rng.standard_normal((b, atoms))).astype(f32)
    a = (scale * rng.standard_normal((b, s, atoms))).astype(f32)
    actions = rng.integers(0, s, b)
    actions[::3] -= s
    m = rng.random((b, atoms))
    m[rng.random((b, atoms)) < 0.3] = 0
    m[:, 0] += 0.1
    m = m / m.sum(-1, keepdims=True)
    m[::3] *= 0.5
    w = rng.uniform(0.1, 1.0, b).astype(f32)
    return v, a, actions.astype(np.int64), m.astype(f32), w


CONFIGS = [(16, 50, 31, 1.0), (5, 500, 31, 1.0), (7, 130, 51, 3.0), (16, 7, 2, 1.0), (4, 65, 128, 1.0), (6, 1, 31, 1.0), (6, 40, 31, 30.0)]


@pytest.mark.parametrize("b,s,atoms,scale", CONFIGS)
def test_definition_against_the_reference(b, s, atoms, scale):
    rng = np.random.default_rng(500 + s)
    v, a, actions, m, w = loss_inputs(rng, b, s, atoms, scale)
    dloss, dgv, dga = loss_bounds(v, a, m, w)
    want_loss, want_gv, want_ga = reference64(v, a, actions, m, w)
    loss, g = dueling_loss_np(v, a, actions, m)
    grad_v, grad_a = dueling_loss_backward_np(g, w, actions, s)
    assert np.isfinite(loss).all()
    assert np.abs(loss.astype(np.float64) - want_loss).max() <= dloss
    assert np.abs(grad_v.astype(np.float64) - want_gv).max() <= dgv
    assert np.abs(grad_a.astype(np.float64) - want_ga).max() <= dga
    if scale >= 30:
        x = (v + a[np.arange(b), actions]) - mean_np(a)
        assert (dexp_np(x - x.max(-1, keepdims=True)) == 0).mean() > 0.3, "the large logits are meant to drive many e to exactly 0"


# ------------------------------------------------------------------ identities of the definition ------------
def test_identities_hold_bit_for_bit():
    rng = np.random.default_rng(11)
    b, s, atoms = 5, 37, 31
    v, a, actions, m, w = loss_inputs(rng, b, s, atoms)
    loss, g = dueling_loss_np(v, a, actions, m)
    grad_v, grad_a = dueling_loss_backward_np(g, w, actions, s)
    c = (w[:, None] * g) / f32(s)
    r = np.where(actions < 0, actions + s, actions)
    for i in range(b):
        others = np.delete(grad_a[i], r[i], axis=0)
        np.testing.assert_array_equal(others, np.broadcast_to(-c[i], others.shape))
        np.testing.assert_array_equal(grad_a[i, r[i]], grad_v[i] - c[i])
    np.testing.assert_array_equal(grad_v, w[:, None] * g)
    zv, za = dueling_loss_backward_np(g, np.zeros(b, dtype=f32), actions, s)                 # w == 0
    assert (zv == 0).all() and (za == 0).all()
    one_loss, one_g = dueling_loss_np(v, a[:, :1], np.zeros(b, dtype=np.int64), m)           # S == 1
    _, one_a = dueling_loss_backward_np(one_g, w, np.zeros(b, dtype=np.int64), 1)
    assert (one_a == 0).all() and np.isfinite(one_loss).all()
    bad = np.array([s, -s - 1, 0, 2 ** 40, -1], dtype=np.int64)                              # out of range: NaN, g = 0
    loss, g = dueling_loss_np(v, a, bad, m)
    np.testing.assert_array_equal(np.isnan(loss), [True, True, False, True, False])
    assert (g[[0, 1, 3]] == 0).all() and (g[[2, 4]] != 0).any()
    gv, ga = dueling_loss_backward_np(g, w, bad, s)
    assert (gv[[0, 1, 3]] == 0).all() and (ga[[0, 1, 3]] == 0).all()
    np.testing.assert_array_equal(dueling_loss_np(v, a, np.full(b, -1), m)[0], dueling_loss_np(v, a, np.full(b, s - 1), m)[0])


# ------------------------------------------------------------------ the wrappers on the CPU ------------
def _leaves(v, a):
    return torch.from_numpy(v).clone().requires_grad_(), torch.from_numpy(a).clone().requires_grad_()


def test_loss_wrapper_takes_the_reference_lines_on_the_cpu():
    rng = np.random.default_rng(12)
    b, s, atoms = 6, 20, 31
    v, a, actions, m, w = loss_inputs(rng, b, s, atoms)
    t = torch.from_numpy
    for v_shape in ((b, atoms), (b, 1, atoms)):
        for reduce in (lambda loss: loss.sum(), lambda loss: (t(w) * loss).mean()):
            v0, a0 = _leaves(v, a)
            want = loss_torch(v0, a0, t(actions), t(m))
            reduce(want).backward()
            v1, a1 = _leaves(v.reshape(v_shape), a)
            got = replay.dueling_c51_loss(v1, a1, t(actions), t(m))
            assert got.dtype == torch.float32 and got.shape == (b,) and torch.equal(got, want)
            reduce(got).backward()
            assert v1.grad.shape == v_shape and torch.equal(v1.grad.reshape(b, atoms), v0.grad) and torch.equal(a1.grad, a0.grad)
    v0, a0 = _leaves(v, a)                                # only one side requires a gradient
    replay.dueling_c51_loss(v0, t(a), t(actions), t(m)).sum().backward()
    replay.dueling_c51_loss(t(v), a0, t(actions), t(m)).sum().backward()
    v1, a1 = _leaves(v, a)
    loss_torch(v1, a1, t(actions), t(m)).sum().backward()
    assert torch.equal(v0.grad, v1.grad) and torch.equal(a0.grad, a1.grad)
    m_leaf = t(m).clone().requires_grad_()               # m is a constant
    v0, a0 = _leaves(v, a)
    replay.dueling_c51_loss(v0, a0, t(actions), m_leaf).sum().backward()
    assert m_leaf.grad is None
    neg = t(np.where(actions < 0, actions, actions - s))  # negative indices count from the end
    assert torch.equal(replay.dueling_c51_loss(t(v), t(a), neg, t(m)), loss_torch(t(v), t(a), t(actions), t(m)))
    with pytest.raises(IndexError):                      # the reference's indexing refuses what the kernel answers with NaN
        replay.dueling_c51_loss(t(v), t(a), torch.full((b,), s), t(m))
    with pytest.raises(ValueError):
        replay.dueling_c51_loss(t(v)[:, :-1], t(a), t(actions), t(m))
    with pytest.raises(ValueError):
        replay.dueling_c51_loss(t(v), t(a), t(actions)[:-1], t(m))
    with pytest.raises(ValueError):
        replay.dueling_c51_loss(t(v), t(a), t(actions), t(m)[:, :-1])
    with pytest.raises(RuntimeError, match="HIP device"):
        replay.dueling_c51_loss(t(v), t(a), t(actions), t(m), use_hip=True)
    assert replay.DUELING_LOSS_HIP_DEFAULT in (False, True)


class ToyNet(torch.nn.Module):
    """two layers to (v, a) logits"""

    def __init__(self, obs_len, s, atoms, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.s, self.atoms = s, atoms
        self.fc = torch.nn.Linear(obs_len, 24)
        self.head = torch.nn.Linear(24, (s + 1) * atoms)

    def forward(self, x):
        y = self.head(torch.tanh(self.fc(x))).view(-1, self.s + 1, self.atoms)
        return y[:, :1], y[:, 1:]


def test_learn_loss_is_the_reference_learn_on_a_toy_network():
    """agent.py:84-119 with the network's forward written out (model.py:395-400), against replay.learn_loss."""
    b, s, atoms, obs_len, v_min, v_max, gamma_n = 8, 12, 31, 10, -1.0, 8.0, 0.99 ** 3
    rng = np.random.default_rng(13)
    online, target = ToyNet(obs_len, s, atoms, 1), ToyNet(obs_len, s, atoms, 2)
    support = torch.linspace(v_min, v_max, atoms)
    t = torch.from_numpy
    states, next_states = t(rng.standard_normal((b, obs_len)).astype(f32)), t(rng.standard_normal((b, obs_len)).astype(f32))
    actions = t(rng.integers(0, s, b))
    returns, nonterm = t(rng.uniform(-2, 9, b).astype(f32)), t((rng.random((b, 1)) < 0.6).astype(f32))
    weights = t(rng.uniform(0.1, 1, b).astype(f32))
    batch = (None, states, actions, returns, next_states, nonterm, weights)

    def net(model, x, log=False):
        v, a = model(x)
        q = v + a - a.mean(1, keepdim=True)
        return F.log_softmax(q, dim=2) if log else F.softmax(q, dim=2)
    log_ps_a = net(online, states, log=True)[range(b), actions]
    with torch.no_grad():
        m, _ = learn_torch(net(online, next_states), net(target, next_states), returns, nonterm, support, gamma_n, v_min, v_max, atoms)
    want = -torch.sum(m * log_ps_a, 1)
    online.zero_grad()
    (weights * want).mean().backward()
    want_grads = [p.grad.clone() for p in online.parameters()]
    got = replay.learn_loss(online, target, batch, support, gamma_n, v_min, v_max)
    assert got.shape == (b,) and torch.equal(got, want)
    online.zero_grad()
    (weights * got).mean().backward()
    for p, wg in zip(online.parameters(), want_grads):
        assert torch.equal(p.grad, wg)
    assert all(p.grad is None for p in target.parameters())


# ------------------------------------------------------------------ limits of the entry points ------------
@pytest.fixture(scope="module")
def lib():
    from irbpp_amd import _lib, build
    build.build()
    return _lib.load()


NULL = C.c_void_p(0)
ids = lambda d: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in d.items())      # noqa: E731


def _loss_args(**kw):
    buf = np.zeros(1024, dtype=f32)
    ptr = C.c_void_p(buf.ctypes.data)
    d = dict(v=ptr, v_stride=31, a=ptr, env_stride=31 * 4, row_stride=31, actions=ptr, m=ptr, atoms=31, s_rows=4, batch=1, loss=ptr,
             g=ptr, keep=buf)
    d.update(kw)
    return d


BAD_LOSS = [dict(atoms=1), dict(atoms=129, row_stride=129, env_stride=129 * 4, v_stride=129), dict(s_rows=0),
            dict(s_rows=1025, env_stride=1 << 20), dict(batch=0), dict(batch=-3), dict(row_stride=30), dict(env_stride=31 * 4 - 1),
            dict(v_stride=30), dict(v=NULL), dict(a=NULL), dict(actions=NULL), dict(m=NULL), dict(loss=NULL), dict(g=NULL)]


@pytest.mark.parametrize("bad", BAD_LOSS, ids=ids)
def test_loss_rejects_what_is_outside_its_limits(lib, bad):
    d = _loss_args(**bad)
    assert lib.irbpp_dueling_loss(d["v"], d["v_stride"], d["a"], d["env_stride"], d["row_stride"], d["actions"], d["m"], d["atoms"],
                                  d["s_rows"], d["batch"], d["loss"], d["g"], None) == -1        # IRBPP_ERR_ARG before any HIP call


BAD_BACKWARD = [dict(atoms=1), dict(atoms=129), dict(s_rows=0), dict(s_rows=1025), dict(batch=0), dict(g=NULL), dict(w=NULL),
                dict(actions=NULL)]


@pytest.mark.parametrize("bad", BAD_BACKWARD, ids=ids)
def test_backward_rejects_what_is_outside_its_limits(lib, bad):
    buf = np.zeros(1024, dtype=f32)
    ptr = C.c_void_p(buf.ctypes.data)
    d = dict(g=ptr, w=ptr, actions=ptr, atoms=31, s_rows=4, batch=1)
    d.update(bad)
    assert lib.irbpp_dueling_loss_backward(d["g"], d["w"], d["actions"], d["atoms"], d["s_rows"], d["batch"], ptr, ptr, None) == -1


def test_backward_with_no_output_launches_nothing(lib):
    buf = np.zeros(64, dtype=f32)
    ptr = C.c_void_p(buf.ctypes.data)
    assert lib.irbpp_dueling_loss_backward(ptr, ptr, ptr, 31, 4, 1, None, None, None) == 0       # IRBPP_OK without any HIP call
