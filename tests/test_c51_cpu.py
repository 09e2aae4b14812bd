"""The distributional head (csrc/irbpp_c51.hip, replay.distributional_greedy_action / c51_target) without a GPU.

The kernels' arithmetic is defined, not left to the implementation: a row's expected value is the float32 sum, left to right
over the atoms, of fl32(p[a] * z[a]); the projection restates Agent.learn's float32 operations one by one and scatters in
the order of the reference's two sequential index_add_ calls.  This file carries that definition as numpy float32 code
(``act_np`` / ``target_np``; tests/test_gpu_c51.py holds the kernels to it bit for bit) and checks the definition itself
against the reference's torch lines (agent.py:51-58, 88-115, written out below, CPU tensors):

* actions / a_star equal wherever the gap between the top two expected values exceeds 2 * atoms * 2^-24 * sum|p z| (the bound
  for reordering a float32 sum of `atoms` terms, taken on both values); at most 2 % of the rows may fall inside it;
* m within an absolute 2 * atoms * 2^-24: an entry is at most 2 * atoms non-negative terms whose sum is at most 1.

Also here: the wrappers' CPU form and the IRBPP_ERR_ARG limits of the two entry points (checked before any HIP call)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay

f32 = np.float32
EPS = 2.0 ** -24


# ------------------------------------------------------------------ the definition, in numpy float32 ------------
def expected_np(p, z):
    """[..., atoms] float32 -> [...]: ((p0 z0 + p1 z1) + p2 z2) + ..., every product and every sum rounded to float32."""
    p, z = np.asarray(p, dtype=f32), np.asarray(z, dtype=f32)
    s = p[..., 0] * z[0]
    for a in range(1, p.shape[-1]):
        s = s + p[..., a] * z[a]
    assert s.dtype == f32
    return s


def act_np(p, z, flags=None):
    """-> (action int64 [N], q float32 [N, S]); flags [N, S]: 0 = masked.  np.argmax returns the first maximum, and 0 when
    every entry is -inf."""
    q = expected_np(p, z)
    v = q if flags is None else np.where(np.asarray(flags) == 0, f32(-np.inf), q)
    return v.argmax(1).astype(np.int64), q


def project_np(pns_a, returns, nonterminals, z, gamma_n, v_min, v_max, delta_z):
    """agent.py:100-115 in float32, one operation at a time -> (m [B, atoms], l, u, l == u before the fix-ups)."""
    pns_a, z = np.asarray(pns_a, dtype=f32), np.asarray(z, dtype=f32)
    B, atoms = pns_a.shape
    ret, nt = np.asarray(returns, dtype=f32).reshape(B, 1), np.asarray(nonterminals, dtype=f32).reshape(B, 1)
    gamma_n, v_min, v_max, delta_z = f32(gamma_n), f32(v_min), f32(v_max), f32(delta_z)
    tz = ret + (nt * gamma_n) * z[None, :]
    tz = np.minimum(np.maximum(tz, v_min), v_max)
    b = (tz - v_min) / delta_z
    assert b.dtype == f32
    fl, ce = np.floor(b), np.ceil(b)
    l, u = fl.astype(np.int64), ce.astype(np.int64)
    integral = l == u
    l = np.where((u > 0) & (l == u), l - 1, l)
    u = np.where((l < atoms - 1) & (l == u), u + 1, u)
    assert l.min() >= 0 and u.max() <= atoms - 1, "test inputs must keep the projection inside the support"
    wl = pns_a * (u.astype(f32) - b)
    wu = pns_a * (b - l.astype(f32))
    m = np.zeros((B, atoms), dtype=f32)
    rows = np.arange(B)
    for i in range(atoms):                               # first index_add_: ascending i (one entry per sample and step)
        m[rows, l[:, i]] = m[rows, l[:, i]] + wl[:, i]
    for i in range(atoms):                               # second index_add_
        m[rows, u[:, i]] = m[rows, u[:, i]] + wu[:, i]
    assert m.dtype == f32
    return m, l, u, integral


def target_np(p_online, p_target, returns, nonterminals, z, gamma_n, v_min, v_max, delta_z):
    """-> (m, a_star): the unmasked arg-max of the defined expected value of p_online, then the projection of its p_target row."""
    a_star, _ = act_np(p_online, z)
    pns_a = np.asarray(p_target, dtype=f32)[np.arange(len(a_star)), a_star]
    return project_np(pns_a, returns, nonterminals, z, gamma_n, v_min, v_max, delta_z)[0], a_star


# ------------------------------------------------------------------ the reference's lines, in torch ------------
def act_torch(q_map, support, mask):
    """agent.py:54-58."""
    sum_q_map = q_map * support
    sum_q_map = sum_q_map.sum(2)
    q = sum_q_map.clone()
    if mask is not None:
        sum_q_map[(1 - mask).bool()] = -math.inf
    return sum_q_map.argmax(1), q


def learn_torch(pns_online, pns_target, returns, nonterminals, support, discount_n, Vmin, Vmax, atoms):
    """agent.py:91-115 (returns [B], nonterminals [B, 1]); discount_n stands for self.discount ** self.n."""
    batch_size = pns_online.shape[0]
    delta_z = (Vmax - Vmin) / (atoms - 1)
    dns = support.expand_as(pns_online) * pns_online
    argmax_indices_ns = dns.sum(2).argmax(1)
    pns_a = pns_target[range(batch_size), argmax_indices_ns]
    Tz = returns.unsqueeze(1) + nonterminals * discount_n * support.unsqueeze(0)
    Tz = Tz.clamp(min=Vmin, max=Vmax)
    b = (Tz - Vmin) / delta_z
    l, u = b.floor().to(torch.int64), b.ceil().to(torch.int64)
    l[(u > 0) * (l == u)] -= 1
    u[(l < (atoms - 1)) * (l == u)] += 1
    m = pns_target.new_zeros(batch_size, atoms)
    offset = torch.linspace(0, ((batch_size - 1) * atoms), batch_size).unsqueeze(1).expand(batch_size, atoms).to(l)
    m.view(-1).index_add_(0, (l + offset).view(-1), (pns_a * (u.float() - b)).view(-1))
    m.view(-1).index_add_(0, (u + offset).view(-1), (pns_a * (b - l.float())).view(-1))
    return m, argmax_indices_ns


# ------------------------------------------------------------------ inputs ------------
def probabilities(rng, n, s, atoms, sharp=3.0):
    """softmax rows [n, s, atoms] float32."""
    x = rng.standard_normal((n, s, atoms)) * sharp
    x = np.exp(x - x.max(-1, keepdims=True))
    return (x / x.sum(-1, keepdims=True)).astype(f32)


def decided(q, absq, atoms, flags=None):
    """[N] bool: the gap between the top two (unmasked) values exceeds the reordering bound, taken with the largest
    sum|p z| of the env's rows.  One candidate only: decided."""
    v = np.asarray(q, dtype=np.float64)
    if flags is not None:
        v = np.where(np.asarray(flags) == 0, -np.inf, v)
    if v.shape[1] == 1:
        return np.ones(v.shape[0], dtype=bool)
    top = np.sort(v, axis=1)[:, -2:]
    bound = 2 * atoms * EPS * absq.max(1)
    with np.errstate(invalid="ignore"):
        gap = top[:, 1] - top[:, 0]
    return np.where(np.isnan(gap), False, gap > bound)          # (-inf) - (-inf): fewer than two valid rows, ties at index level


def abs_sum(p, z):
    return (np.abs(np.asarray(p, dtype=np.float64) * np.asarray(z, dtype=np.float64))).sum(-1)


CONFIGS = [(64, 50, 51, -1.0, 8.0), (33, 130, 51, -10.0, 10.0), (16, 7, 2, 0.0, 1.0), (8, 65, 128, -1.0, 4.0)]


@pytest.mark.parametrize("n,s,atoms,v_min,v_max", CONFIGS)
def test_definition_against_the_reference_act(n, s, atoms, v_min, v_max):
    rng = np.random.default_rng(100 + s)
    p = probabilities(rng, n, s, atoms)
    support = torch.linspace(v_min, v_max, atoms)
    z = support.numpy()
    flags = (rng.random((n, s)) < 0.7).astype(f32)
    absq = abs_sum(p, z)
    for fl in (None, flags):
        want, q_t = act_torch(torch.from_numpy(p), support, None if fl is None else torch.from_numpy(fl))
        got, q = act_np(p, z, fl)
        assert np.all(np.abs(q.astype(np.float64) - q_t.numpy()) <= 2 * atoms * EPS * absq)
        ok = decided(q, absq, atoms, fl)
        if fl is not None:
            ok |= (fl != 0).sum(1) == 0                      # nothing valid: index 0 on both sides
        assert (~ok).mean() <= 0.02, "too many rows inside the gap bound"
        np.testing.assert_array_equal(got[ok], want.numpy()[ok])


@pytest.mark.parametrize("n,s,atoms,v_min,v_max", CONFIGS)
@pytest.mark.parametrize("gamma_n", [0.99 ** 3, 0.0])
def test_definition_against_the_reference_learn(n, s, atoms, v_min, v_max, gamma_n):
    rng = np.random.default_rng(200 + s)
    p_on, p_tg = probabilities(rng, n, s, atoms), probabilities(rng, n, s, atoms)
    support = torch.linspace(v_min, v_max, atoms)
    z = support.numpy()
    returns = rng.uniform(v_min - 1.0, v_max + 1.0, n).astype(f32)
    returns[::5] = z[(np.arange(len(returns[::5])) * 7) % atoms]          # some returns exactly on an atom
    nonterm = (rng.random(n) < 0.6).astype(f32)
    nonterm[::5] = 0.0
    delta_z = (v_max - v_min) / (atoms - 1)
    want_m, want_a = learn_torch(torch.from_numpy(p_on), torch.from_numpy(p_tg), torch.from_numpy(returns),
                                 torch.from_numpy(nonterm).reshape(n, 1), support, gamma_n, v_min, v_max, atoms)
    got_m, got_a = target_np(p_on, p_tg, returns, nonterm, z, gamma_n, v_min, v_max, delta_z)
    ok = decided(expected_np(p_on, z), abs_sum(p_on, z), atoms)
    assert (~ok).mean() <= 0.02, "too many rows inside the gap bound"
    np.testing.assert_array_equal(got_a[ok], want_a.numpy()[ok])
    assert np.abs(got_m[ok].astype(np.float64) - want_m.numpy()[ok]).max() <= 2 * atoms * EPS
    pns_a = p_tg[np.arange(n), got_a].astype(np.float64)
    assert np.abs(got_m.astype(np.float64).sum(1) - pns_a.sum(1)).max() <= 2 * atoms * EPS


def test_fixups_at_the_support_ends_and_in_the_middle():
    """A terminal sample whose return lies exactly on atom 0, a middle atom, atom atoms-1: b is an integer, l == u, and the two
    fix-ups move l down (u > 0) or u up (atom 0) so that the whole mass lands on that atom.  delta_z = 0.25: b is exact."""
    atoms, v_min = 51, -2.0
    v_max = v_min + 0.25 * (atoms - 1)
    z = torch.linspace(v_min, v_max, atoms).numpy()
    np.testing.assert_array_equal(z, (v_min + 0.25 * np.arange(atoms)).astype(f32))
    rng = np.random.default_rng(5)
    pns_a = probabilities(rng, 1, 3, atoms)[0]
    on = [0, 17, atoms - 1]
    m, l, u, integral = project_np(pns_a, z[on], np.zeros(3), z, 0.99 ** 3, v_min, v_max, 0.25)
    assert integral.all()
    np.testing.assert_array_equal(l[:, 0], [0, 16, atoms - 2])
    np.testing.assert_array_equal(u[:, 0], [1, 17, atoms - 1])
    for r, j in enumerate(on):
        total = f32(0)
        for i in range(atoms):
            total = total + pns_a[r, i]
        want = np.zeros(atoms, dtype=f32)
        want[j] = total
        # (a terminal sample has one Tz for all atoms: atom 0 collects the l contributions p_i * 1, the others the u ones,
        # behind atoms-many contributions of exactly 0 to atom j-1)
        np.testing.assert_array_equal(m[r], want)


# ------------------------------------------------------------------ the wrappers on the CPU ------------
def test_wrappers_take_the_reference_lines_on_the_cpu():
    rng = np.random.default_rng(9)
    n, s, atoms, v_min, v_max = 12, 20, 51, -1.0, 8.0
    p = torch.from_numpy(probabilities(rng, n, s, atoms))
    p2 = torch.from_numpy(probabilities(rng, n, s, atoms))
    support = torch.linspace(v_min, v_max, atoms)
    state = torch.zeros((n, s * 5 + 11))
    mask = torch.from_numpy((rng.random((n, s)) < 0.5).astype(f32))
    mask[3] = 0
    state[:, :s * 5].view(n, s, 5)[:, :, 4] = mask
    want, q = act_torch(p, support, mask)
    q_out = torch.full((n, s), 7.0)
    got = replay.distributional_greedy_action(p, support, state, s, q_out)
    assert got.dtype == torch.int64 and got[3] == 0
    assert torch.equal(got, want) and torch.equal(q_out, q)
    assert torch.equal(replay.distributional_greedy_action(p, support), act_torch(p, support, None)[0])
    with pytest.raises(ValueError):
        replay.distributional_greedy_action(p, support, state, s + 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        replay.distributional_greedy_action(p, support, use_hip=True)
    returns = torch.from_numpy(rng.uniform(-2, 9, n).astype(f32))
    nonterm = torch.from_numpy((rng.random((n, 1)) < 0.5).astype(f32))
    g = 0.99 ** 3
    want_m, want_a = learn_torch(p, p2, returns, nonterm, support, g, v_min, v_max, atoms)
    m, a = replay.c51_target(p, p2, returns, nonterm, support, g, v_min, v_max)
    assert torch.equal(a, want_a) and torch.equal(m, want_m)
    with pytest.raises(RuntimeError, match="HIP device"):
        replay.c51_target(p, p2, returns, nonterm, support, g, v_min, v_max, use_hip=True)


# ------------------------------------------------------------------ limits of the entry points ------------
@pytest.fixture(scope="module")
def lib():
    from irbpp_amd import _lib, build
    build.build()
    return _lib.load()


def _act_args(**kw):
    buf = np.zeros(64, dtype=f32)
    ptr = C.c_void_p(buf.ctypes.data)
    a = dict(p=ptr, env_stride=51 * 4, row_stride=51, support=ptr, atoms=51, obs=ptr, obs_stride=20, s_rows=4, n_env=1,
             action=ptr, q_out=ptr, q_stride=4, keep=buf)
    a.update(kw)
    return a


def _call_act(lib, a):
    return lib.irbpp_categorical_act(a["p"], a["env_stride"], a["row_stride"], a["support"], a["atoms"], a["obs"], a["obs_stride"],
                                     a["s_rows"], a["n_env"], a["action"], a["q_out"], a["q_stride"], None)


NULL = C.c_void_p(0)
BAD_ACT = [dict(atoms=1), dict(atoms=129, row_stride=129, env_stride=129 * 4), dict(s_rows=0), dict(s_rows=1025, env_stride=1 << 20, obs_stride=1 << 20, q_stride=1 << 20),
           dict(n_env=0), dict(n_env=-3), dict(row_stride=50), dict(env_stride=51 * 4 - 1), dict(obs_stride=19), dict(q_stride=3),
           dict(p=NULL), dict(support=NULL), dict(action=NULL)]


@pytest.mark.parametrize("bad", BAD_ACT, ids=lambda d: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in d.items()))
def test_act_rejects_what_is_outside_its_limits(lib, bad):
    assert _call_act(lib, _act_args(**bad)) == -1                      # IRBPP_ERR_ARG before any HIP call


def _target_args(**kw):
    buf = np.zeros(64, dtype=f32)
    ptr = C.c_void_p(buf.ctypes.data)
    a = dict(p_on=ptr, on_env=51 * 4, on_row=51, p_tg=ptr, tg_env=51 * 4, tg_row=51, returns=ptr, nonterm=ptr, support=ptr,
             atoms=51, s_rows=4, batch=1, gamma_n=0.97, v_min=-1.0, v_max=8.0, delta_z=0.18, m=ptr, a_star=ptr, keep=buf)
    a.update(kw)
    return a


BAD_TARGET = [dict(atoms=1), dict(atoms=129, on_row=129, tg_row=129, on_env=129 * 4, tg_env=129 * 4), dict(s_rows=0),
              dict(s_rows=1025, on_env=1 << 20, tg_env=1 << 20), dict(batch=0), dict(on_row=50), dict(tg_row=50),
              dict(on_env=51 * 4 - 1), dict(tg_env=51 * 4 - 1), dict(v_max=-1.0), dict(delta_z=0.0), dict(delta_z=-0.18),
              dict(p_on=NULL), dict(p_tg=NULL), dict(returns=NULL), dict(nonterm=NULL), dict(support=NULL), dict(m=NULL),
              dict(a_star=NULL)]


@pytest.mark.parametrize("bad", BAD_TARGET, ids=lambda d: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in d.items()))
def test_target_rejects_what_is_outside_its_limits(lib, bad):
    a = _target_args(**bad)
    assert lib.irbpp_categorical_target(a["p_on"], a["on_env"], a["on_row"], a["p_tg"], a["tg_env"], a["tg_row"], a["returns"],
                                        a["nonterm"], a["support"], a["atoms"], a["s_rows"], a["batch"], a["gamma_n"], a["v_min"],
                                        a["v_max"], a["delta_z"], a["m"], a["a_star"], None) == -1
