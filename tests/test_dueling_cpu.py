"""The dueling head (csrc/irbpp_dueling.hip, replay.dueling_greedy_action / dueling_c51_target) without a GPU.

The kernels' arithmetic is defined (the header of irbpp_dueling.hip); this file carries that definition as numpy float32 code
(``dexp_np``, ``mean_np``, ``softmax_np``, ``dueling_act_np``, ``dueling_target_np``: tests/test_gpu_dueling.py and
tests/test_dueling_kernel_on_host.py hold the kernels to it bit for bit) and checks the definition itself:

* ``dexp_np`` against float64 exp within DEXP_MAX_ULP, the figure of the full sweep (tools/dexp_sweep.py,
  profiles/dueling_head/README.md);
* the definition against the reference's torch lines (model.py:395-400, agent.py:54-58, 90-115) evaluated in float64, within
  the bounds derived in ``bounds`` below;
* the wrappers' CPU form and the IRBPP_ERR_ARG limits of the two entry points (checked before any HIP call)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_c51_cpu import act_np, act_torch, learn_torch, project_np

f32 = np.float32
U = 2.0 ** -24                                           # unit roundoff of float32
PARTS = 16                                               # DUELING_PARTS
DEXP_CUT = f32(-80.0)
DEXP_MAX_ULP = 1.2123                                    # the full sweep: 1.21223 ulp at t = -71.0456 (profiles/dueling_head/)
LOG2E, LN2_HI, LN2_LO = f32(1.4426950408889634), f32(0.693145751953125), f32(1.4286068203094172e-06)
COEF = [f32(c) for c in (1.9841269841269841e-04, 1.3888888888888889e-03, 8.3333333333333332e-03, 4.1666666666666664e-02,
                         1.6666666666666666e-01, 0.5, 1.0, 1.0)]


# ------------------------------------------------------------------ the definition, in numpy float32 ------------
def dexp_np(t):
    """dueling_dexp: float32 [...] <= 0 -> float32, exactly 0 below the cut-off."""
    t = np.asarray(t, dtype=f32)
    tc = np.maximum(t, DEXP_CUT)                         # (the lanes below the cut-off are replaced at the end)
    n = np.floor(tc * LOG2E + f32(0.5))
    r = (tc - n * LN2_HI) - n * LN2_LO
    p = np.full(t.shape, COEF[0], dtype=f32)
    for c in COEF[1:]:
        p = p * r + c
    scale = ((n.astype(np.int32) + 127) << 23).astype(np.uint32).view(f32)
    out = np.where(t < DEXP_CUT, f32(0), p * scale)
    assert out.dtype == f32
    return out


def mean_np(a):
    """[N, S, atoms] -> [N, atoms]: 16 interleaved partial sums (rows ascending, from 0.0), added left to right, / (float)S."""
    a = np.asarray(a, dtype=f32)
    n, s, atoms = a.shape
    part = np.zeros((n, PARTS, atoms), dtype=f32)
    for i in range(s):
        part[:, i % PARTS] = part[:, i % PARTS] + a[:, i]
    tot = part[:, 0]
    for g in range(1, PARTS):
        tot = tot + part[:, g]
    return tot / f32(s)


def softmax_rows_np(v, a_rows, mean):
    """v, mean [N, atoms], a_rows [N, R, atoms] -> p [N, R, atoms]."""
    x = (v[:, None, :] + a_rows) - mean[:, None, :]
    e = dexp_np(x - x.max(-1, keepdims=True))
    den = e[..., 0]
    for k in range(1, e.shape[-1]):
        den = den + e[..., k]
    p = e / den[..., None]
    assert p.dtype == f32
    return p


def softmax_np(v, a):
    v, a = np.asarray(v, dtype=f32), np.asarray(a, dtype=f32)
    return softmax_rows_np(v, a, mean_np(a))


def dueling_act_np(v, a, z, flags=None):
    """-> (action int64 [N], q float32 [N, S], p float32 [N, S, atoms])."""
    p = softmax_np(v, a)
    act, q = act_np(p, z, flags)
    return act, q, p


def dueling_target_np(v_on, a_on, v_tg, a_tg, returns, nonterminals, z, gamma_n, v_min, v_max, delta_z):
    """-> (m, a_star): the target row is computed alone, from the target block's mean."""
    a_star = dueling_act_np(v_on, a_on, z)[0]
    v_tg, a_tg = np.asarray(v_tg, dtype=f32), np.asarray(a_tg, dtype=f32)
    row = a_tg[np.arange(len(a_star)), a_star][:, None, :]
    pns_a = softmax_rows_np(v_tg, row, mean_np(a_tg))[:, 0]
    return project_np(pns_a, returns, nonterminals, z, gamma_n, v_min, v_max, delta_z)[0], a_star


# ------------------------------------------------------------------ the reference's lines, in torch ------------
def head_torch(v, a):
    """model.py:395-400 (log=False)."""
    atoms, action_space = v.shape[-1], a.shape[1]
    v, a = v.view(-1, 1, atoms), a.view(-1, action_space, atoms)
    q = v + a - a.mean(1, keepdim=True)
    return F.softmax(q, dim=2)


# ------------------------------------------------------------------ dexp ------------
def ulp_error(t):
    """error of dexp_np(t) against float64 exp of the float32 argument, in ulp of the float32 nearest the true value."""
    t = np.asarray(t, dtype=f32)
    want = np.exp(t.astype(np.float64))
    ulp = np.spacing(want.astype(f32)).astype(np.float64)
    return np.abs(dexp_np(t).astype(np.float64) - want) / ulp


def reduction_boundaries():
    """the float32 arguments around every t at which n = floor(t log2(e) + 1/2) steps, 8 neighbours each side."""
    out = []
    for m in range(-116, 1):
        c = f32((m + 0.5) * np.log(2.0))
        if c > 0 or c < DEXP_CUT:
            continue
        bits = np.array([c], dtype=f32).view(np.uint32)[0]
        out.append((np.arange(-8, 9).astype(np.int64) + int(bits)).astype(np.uint32).view(f32))
    return np.concatenate(out)


def test_dexp_special_arguments():
    assert dexp_np(f32(0.0)) == f32(1.0) and dexp_np(f32(-0.0)) == f32(1.0)
    below = np.nextafter(DEXP_CUT, f32(-np.inf))
    assert dexp_np(below) == 0.0 and dexp_np(f32(-1e30)) == 0.0 and dexp_np(f32(-np.inf)) == 0.0
    at = dexp_np(np.array([DEXP_CUT, np.nextafter(DEXP_CUT, f32(0))], dtype=f32))
    assert (at > 0).all() and (at >= np.finfo(f32).tiny * 128).all()           # e / den stays normal for den <= 128
    assert ulp_error(np.array([DEXP_CUT, np.nextafter(DEXP_CUT, f32(0)), 0.0, -0.0], dtype=f32)).max() <= DEXP_MAX_ULP
    t = reduction_boundaries()
    t = t[(t <= 0) & (t >= DEXP_CUT)]
    assert len(t) > 1500
    assert ulp_error(t).max() <= DEXP_MAX_ULP
    tiny = -np.array([2.0 ** -k for k in range(1, 150)], dtype=f32)           # towards -0: subnormal arguments included
    assert ulp_error(tiny).max() <= DEXP_MAX_ULP


def test_dexp_stratified_sample_stays_within_the_sweep():
    """2^20 + arguments: 8192 equal strata of the bit patterns of [-80, -2^-126] x 136 fixed offsets each (the bit pattern is
    monotonic in the value, so every binade gets its share), and is monotone where it matters: dexp <= 1."""
    lo, hi = int(np.array([2.0 ** -126], dtype=f32).view(np.uint32)[0]), int(np.array([80.0], dtype=f32).view(np.uint32)[0])
    strata, per = 8192, 136
    width = (hi - lo) // strata
    offs = (np.arange(per, dtype=np.int64) * 2654435761 + 12345) % width
    bits = (lo + np.arange(strata, dtype=np.int64)[:, None] * width + offs[None, :]).ravel()
    assert len(bits) >= 2 ** 20 and bits.max() <= hi
    t = -bits.astype(np.uint32).view(f32)
    err = ulp_error(t)
    assert err.max() <= DEXP_MAX_ULP, f"{err.max()} ulp at t = {t[err.argmax()]!r}"
    assert dexp_np(t).max() <= 1.0


# ------------------------------------------------------------------ the definition against the reference ------------
def bounds(v, a, z, returns=None, delta_z=None):
    """Bounds on |definition - exact| (the float64 torch lines stand for exact; u = 2^-24, first-order terms times 1.02 for
    the higher orders, every term far below 1).

    x: the mean is a float32 sum of at most ceil(S / 16) + 15 additions per column and a division, relative error
       (ceil(S/16) + 16) u of sum|a| / S <= (ceil(S/16) + 16) u A with A = max|a|; v + a rounds within u (V + A), V = max|v|,
       and the subtraction within u (V + 2A).  dx <= (ceil(S/16) + 19) u (V + A).
    t = x - mx: both operands carry dx and the subtraction rounds within u |t|, |t| <= 80 above the cut-off:
       dt <= 2 dx + 80 u.
    e: exp(t + dt) = exp(t) (1 + dt) to first order, and dexp adds DEXP_MAX_ULP ulp = at most 2 DEXP_MAX_ULP u relative:
       ee = dt + 2 DEXP_MAX_ULP u relative.  Below the cut-off e is 0 instead of at most exp(-80) < 2e-35 (absolute; den >= 1).
    den: atoms non-negative terms, atoms - 1 additions: relative ee + (atoms - 1) u.
    p = e / den: relative ep = 2 ee + atoms u; p <= 1, so |dp| <= 1.02 ep + 2e-35 absolutely.
    q = sum p z in atoms products and atoms - 1 additions: |dq| <= (1.02 ep + 2e-35 atoms + atoms u) Z, Z = max|z|
       (sum p = 1 to within ep).
    m: every entry is a sum of at most 2 atoms terms pns_a[i] w with w in [0, 1] and sum pns_a <= 1 + ep: the p errors add up
       to at most atoms |dp| <= sum of relative errors on a unit mass = 1.02 ep + 2e-35 atoms, the products and sums round
       within (2 atoms + 1) u, and the weights move with b: Tz = R + g z rounds within 3 u (|R| + Z) before the clamp (the
       float32 gamma_n included), Tz - Vmin within u (Vmax - Vmin), and the division and the float32 delta_z within 2 u b,
       b <= atoms - 1: db <= (3 (|R| + Z) + (Vmax - Vmin)) u / delta_z + 2 (atoms - 1) u.  A b that crosses an integer moves
       l and u by one but the weights by no more than db: mass db moves between neighbours.  |dm| <= dp_sum + (2 atoms + 1) u
       + 2 db."""
    s, atoms = a.shape[1], a.shape[2]
    V, A, Z = float(np.abs(v).max()), float(np.abs(a).max()), float(np.abs(z).max())
    dx = (-(-s // PARTS) + 19) * U * (V + A)
    ee = 2 * dx + 80 * U + 2 * DEXP_MAX_ULP * U
    ep = 2 * ee + atoms * U
    dp = 1.02 * ep + 2e-35
    dq = (1.02 * ep + 2e-35 * atoms + atoms * U) * Z
    dm = None
    if returns is not None:
        span = float(z.max() - z.min())
        db = (3 * (float(np.abs(returns).max()) + Z) + span) * U / delta_z + 2 * (atoms - 1) * U
        dm = 1.02 * ep + 2e-35 * atoms + (2 * atoms + 1) * U + 2 * db
    return dp, dq, dm


def head_inputs(rng, n, s, atoms, z, lead=20.0):
    """v [n, atoms], a [n, s, atoms] standard normal, with a planted leader per env: one row whose last-atom logit is raised by
    `lead`, so its distribution sits on z[-1], the largest support value -> (v, a, leader row per env)."""
    v = rng.standard_normal((n, atoms)).astype(f32)
    a = rng.standard_normal((n, s, atoms)).astype(f32)
    leader = rng.integers(0, s, n)
    a[np.arange(n), leader, -1] += f32(lead)
    return v, a, leader


def gap64(q64, flags=None):
    """[N]: the float64 gap between the largest and the second largest (valid) value; inf with one candidate."""
    val = q64 if flags is None else np.where(flags == 0, -np.inf, q64)
    if val.shape[1] == 1:
        return np.full(val.shape[0], np.inf)
    top = np.sort(val, axis=1)[:, -2:]
    return top[:, 1] - top[:, 0]


CONFIGS = [(16, 50, 31, -1.0, 8.0), (5, 500, 31, -1.0, 8.0), (7, 130, 51, -10.0, 10.0), (16, 7, 2, 0.0, 1.0), (4, 65, 128, -1.0, 4.0),
           (6, 1, 31, -1.0, 8.0)]


@pytest.mark.parametrize("n,s,atoms,v_min,v_max", CONFIGS)
def test_definition_against_the_reference_act(n, s, atoms, v_min, v_max):
    rng = np.random.default_rng(300 + s)
    z = torch.linspace(v_min, v_max, atoms).numpy()
    v, a, leader = head_inputs(rng, n, s, atoms, z)
    flags = (rng.random((n, s)) < 0.7).astype(f32)
    flags[np.arange(n), leader] = 1
    dp, dq, _ = bounds(v, a, z)
    p64 = head_torch(torch.from_numpy(v).double(), torch.from_numpy(a).double())
    support64 = torch.from_numpy(z).double()
    for fl in (None, flags):
        want, q64 = act_torch(p64, support64, None if fl is None else torch.from_numpy(fl).double())
        got, q, p = dueling_act_np(v, a, z, fl)
        assert np.abs(p.astype(np.float64) - p64.numpy()).max() <= dp
        assert np.abs(q.astype(np.float64) - q64.numpy()).max() <= dq
        assert (gap64(q64.numpy(), fl) > 100 * dq).all(), "the planted leader does not lead by 100 bounds"
        np.testing.assert_array_equal(want.numpy(), leader)
        np.testing.assert_array_equal(got, want.numpy())


@pytest.mark.parametrize("n,s,atoms,v_min,v_max", CONFIGS)
@pytest.mark.parametrize("gamma_n", [0.99 ** 3, 0.0])
def test_definition_against_the_reference_learn(n, s, atoms, v_min, v_max, gamma_n):
    rng = np.random.default_rng(400 + s)
    support = torch.linspace(v_min, v_max, atoms)
    z = support.numpy()
    v_on, a_on, leader = head_inputs(rng, n, s, atoms, z)
    v_tg, a_tg, _ = head_inputs(rng, n, s, atoms, z, lead=0.0)
    returns = rng.uniform(v_min - 1.0, v_max + 1.0, n).astype(f32)
    nonterm = (rng.random(n) < 0.6).astype(f32)
    nonterm[::5] = 0.0
    delta_z = (v_max - v_min) / (atoms - 1)
    _, dq, _ = bounds(v_on, a_on, z)
    _, _, dm = bounds(v_tg, a_tg, z, returns, delta_z)
    d = lambda x: torch.from_numpy(x).double()           # noqa: E731
    p_on64, p_tg64 = head_torch(d(v_on), d(a_on)), head_torch(d(v_tg), d(a_tg))
    assert (gap64((p_on64 * support.double()).sum(2).numpy()) > 100 * dq).all(), "the planted leader does not lead by 100 bounds"
    want_m, want_a = learn_torch(p_on64, p_tg64, d(returns), d(nonterm).reshape(n, 1), support.double(), gamma_n, v_min, v_max,
                                 atoms)
    got_m, got_a = dueling_target_np(v_on, a_on, v_tg, a_tg, returns, nonterm, z, gamma_n, v_min, v_max, delta_z)
    np.testing.assert_array_equal(want_a.numpy(), leader)
    np.testing.assert_array_equal(got_a, want_a.numpy())
    assert np.abs(got_m.astype(np.float64) - want_m.numpy()).max() <= dm


def test_mean_order_is_the_sixteen_part_one():
    """The summation order is observable: a column of 1e8, 1, -1e8, ... sums differently in another order."""
    s, atoms = 40, 3
    a = np.zeros((1, s, atoms), dtype=f32)
    a[0, 0, 0], a[0, 16, 0], a[0, 32, 0], a[0, 1, 0] = 1e8, 1.0, -1e8, 1.0      # part 0: (1e8 + 1) - 1e8 = 0; part 1: 1
    assert mean_np(a)[0, 0] == f32(1.0) / f32(s)
    a[0, 15, 1], a[0, 0, 1], a[0, 16, 1] = 1.0, 1e8, -1e8                       # part 0 = 0 exactly, then + part 15
    assert mean_np(a)[0, 1] == f32(1.0) / f32(s)
    one = np.array([[[3.0, -0.0, 5.0]]], dtype=f32)
    np.testing.assert_array_equal(mean_np(one)[0], [3.0, 0.0, 5.0])


def test_row_alone_equals_row_of_the_block():
    rng = np.random.default_rng(8)
    v, a, _ = head_inputs(rng, 3, 37, 31, None)
    p = softmax_np(v, a)
    row = softmax_rows_np(v, a[:, 5:6], mean_np(a))[:, 0]
    np.testing.assert_array_equal(row, p[:, 5])
    den = p.astype(np.float64).sum(-1)
    assert np.abs(den - 1).max() <= 40 * U


# ------------------------------------------------------------------ the wrappers on the CPU ------------
def test_wrappers_take_the_reference_lines_on_the_cpu():
    rng = np.random.default_rng(9)
    n, s, atoms, v_min, v_max = 12, 20, 31, -1.0, 8.0
    support = torch.linspace(v_min, v_max, atoms)
    t = torch.from_numpy
    v, a = (t(x) for x in head_inputs(rng, n, s, atoms, None)[:2])
    v2, a2 = (t(x) for x in head_inputs(rng, n, s, atoms, None)[:2])
    state = torch.zeros((n, s * 5 + 11))
    mask = t((rng.random((n, s)) < 0.5).astype(f32))
    mask[3] = 0
    state[:, :s * 5].view(n, s, 5)[:, :, 4] = mask
    p = head_torch(v, a)
    want, q = act_torch(p, support, mask)
    q_out, p_out = torch.full((n, s), 7.0), torch.full((n, s, atoms), 7.0)
    got = replay.dueling_greedy_action(v, a, support, state, s, q_out, p_out)
    assert got.dtype == torch.int64 and got[3] == 0
    assert torch.equal(got, want) and torch.equal(q_out, q) and torch.equal(p_out, p)
    assert torch.equal(replay.dueling_greedy_action(v.view(n, 1, atoms), a, support), act_torch(p, support, None)[0])
    with pytest.raises(ValueError):
        replay.dueling_greedy_action(v, a, support, state, s + 1)
    with pytest.raises(ValueError):
        replay.dueling_greedy_action(v[:, :-1], a, support)
    with pytest.raises(RuntimeError, match="HIP device"):
        replay.dueling_greedy_action(v, a, support, use_hip=True)
    returns = t(rng.uniform(-2, 9, n).astype(f32))
    nonterm = t((rng.random((n, 1)) < 0.5).astype(f32))
    g = 0.99 ** 3
    want_m, want_a = learn_torch(p, head_torch(v2, a2), returns, nonterm, support, g, v_min, v_max, atoms)
    m, a_star = replay.dueling_c51_target(v, a, v2, a2, returns, nonterm, support, g, v_min, v_max)
    assert torch.equal(a_star, want_a) and torch.equal(m, want_m)
    with pytest.raises(ValueError):
        replay.dueling_c51_target(v, a, v2, a2[:, :-1], returns, nonterm, support, g, v_min, v_max)
    with pytest.raises(RuntimeError, match="HIP device"):
        replay.dueling_c51_target(v, a, v2, a2, returns, nonterm, support, g, v_min, v_max, use_hip=True)
    assert replay.DUELING_HIP_DEFAULT in (False, True)


# ------------------------------------------------------------------ limits of the entry points ------------
@pytest.fixture(scope="module")
def lib():
    from irbpp_amd import _lib, build
    build.build()
    return _lib.load()


NULL = C.c_void_p(0)


def _act_args(**kw):
    buf = np.zeros(1024, dtype=f32)
    ptr = C.c_void_p(buf.ctypes.data)
    d = dict(v=ptr, v_stride=31, a=ptr, env_stride=31 * 4, row_stride=31, support=ptr, atoms=31, obs=ptr, obs_stride=20, s_rows=4,
             n_env=1, action=ptr, q_out=ptr, q_stride=4, p_out=ptr, keep=buf)
    d.update(kw)
    return d


BAD_ACT = [dict(atoms=1), dict(atoms=129, row_stride=129, env_stride=129 * 4, v_stride=129), dict(s_rows=0),
           dict(s_rows=1025, env_stride=1 << 20, obs_stride=1 << 20, q_stride=1 << 20), dict(n_env=0), dict(n_env=-3),
           dict(row_stride=30), dict(env_stride=31 * 4 - 1), dict(v_stride=30), dict(obs_stride=19), dict(q_stride=3),
           dict(v=NULL), dict(a=NULL), dict(support=NULL), dict(action=NULL)]
ids = lambda d: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in d.items())      # noqa: E731


@pytest.mark.parametrize("bad", BAD_ACT, ids=ids)
def test_act_rejects_what_is_outside_its_limits(lib, bad):
    d = _act_args(**bad)
    assert lib.irbpp_dueling_act(d["v"], d["v_stride"], d["a"], d["env_stride"], d["row_stride"], d["support"], d["atoms"], d["obs"],
                                 d["obs_stride"], d["s_rows"], d["n_env"], d["action"], d["q_out"], d["q_stride"], d["p_out"],
                                 None) == -1                 # IRBPP_ERR_ARG before any HIP call


def _target_args(**kw):
    buf = np.zeros(1024, dtype=f32)
    ptr = C.c_void_p(buf.ctypes.data)
    d = dict(v_on=ptr, von_stride=31, a_on=ptr, on_env=31 * 4, on_row=31, v_tg=ptr, vtg_stride=31, a_tg=ptr, tg_env=31 * 4, tg_row=31,
             returns=ptr, nonterm=ptr, support=ptr, atoms=31, s_rows=4, batch=1, gamma_n=0.97, v_min=-1.0, v_max=8.0, delta_z=0.3,
             m=ptr, a_star=ptr, keep=buf)
    d.update(kw)
    return d


BAD_TARGET = [dict(atoms=1), dict(atoms=129, on_row=129, tg_row=129, on_env=129 * 4, tg_env=129 * 4, von_stride=129, vtg_stride=129),
              dict(s_rows=0), dict(s_rows=1025, on_env=1 << 20, tg_env=1 << 20), dict(batch=0), dict(on_row=30), dict(tg_row=30),
              dict(on_env=31 * 4 - 1), dict(tg_env=31 * 4 - 1), dict(von_stride=30), dict(vtg_stride=30), dict(v_max=-1.0),
              dict(delta_z=0.0), dict(delta_z=-0.3), dict(v_on=NULL), dict(a_on=NULL), dict(v_tg=NULL), dict(a_tg=NULL),
              dict(returns=NULL), dict(nonterm=NULL), dict(support=NULL), dict(m=NULL), dict(a_star=NULL)]


@pytest.mark.parametrize("bad", BAD_TARGET, ids=ids)
def test_target_rejects_what_is_outside_its_limits(lib, bad):
    d = _target_args(**bad)
    assert lib.irbpp_dueling_target(d["v_on"], d["von_stride"], d["a_on"], d["on_env"], d["on_row"], d["v_tg"], d["vtg_stride"],
                                    d["a_tg"], d["tg_env"], d["tg_row"], d["returns"], d["nonterm"], d["support"], d["atoms"],
                                    d["s_rows"], d["batch"], d["gamma_n"], d["v_min"], d["v_max"], d["delta_z"], d["m"], d["a_star"],
                                    None) == -1
