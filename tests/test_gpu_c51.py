"""csrc/irbpp_c51.hip on the GPU, bit for bit against the numpy float32 definition of tests/test_c51_cpu.py (actions, q_out,
m, a_star: assert_array_equal), through the C ABI with strided arguments; then the two wrappers of irbpp_amd.replay end to end
on device tensors against the reference's torch lines under the gap rule of the CPU test.

Shapes: 64 rows are one trip of a wave's staging loop, so S in {1, 63, 64, 65, 500, 1024}; atoms in {2, 51, 64, 65, 128}
(below, at and above the 64 floats one load instruction covers; the two ends of the accepted range); n and B up to 257.
Every act case takes p as a slice of a wider tensor in the row and the env stride, with 1e30 around it; its envs cycle through
six scenarios (the maximum at row 0 / 63 / 64 / S-1, two identical rows, identical rows 64 apart = a tie across trips of the
lane loop, everything masked, the best row masked, plain)."""
import ctypes as C

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_c51_cpu import (EPS, abs_sum, act_np, act_torch, decided, expected_np, learn_torch, probabilities, project_np,
                          target_np)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
POISON = 1e30


def _lib():
    from irbpp_amd import _lib as L
    return L, L.load()


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _support(atoms, v_min=-1.0, v_max=8.0):
    return torch.linspace(v_min, v_max, atoms)


def act_inputs(s, atoms, n, shift):
    """-> p [n, s, atoms], flags [n, s], scenario per env.  The top row of an env is one-hot on the last atom (value
    z[atoms-1], above every softmax row)."""
    rng = np.random.default_rng(1000 * s + atoms)
    p = probabilities(rng, n, s, atoms)
    flags = (rng.random((n, s)) < 0.8).astype(f32)
    top = np.zeros(atoms, dtype=f32)
    top[-1] = 1.0
    scen = (np.arange(n) + shift) % 6
    spots = [0, 63, 64, s - 1]
    for e in range(n):
        r = min(spots[(e // 6 + shift) % 4], s - 1)
        if scen[e] == 0:                                 # the maximum at a chosen row, valid
            p[e, r], flags[e, r] = top, 1
        elif scen[e] == 1 and s >= 2:                    # two identical best rows: the first wins
            r = min(r, s - 2)
            p[e, r], p[e, s - 1] = top, top
            flags[e, r], flags[e, s - 1] = 1, 1
        elif scen[e] == 2 and s > 64:                    # identical best rows 64 apart: one lane, two trips
            r = min(r, s - 65)
            p[e, r], p[e, r + 64] = top, top
            flags[e, r], flags[e, r + 64] = 1, 1
        elif scen[e] == 3:                               # nothing valid
            flags[e] = 0
        elif scen[e] == 4:                               # the best row masked
            p[e, r], flags[e, r] = top, 0
    return p, flags, scen


def run_act(p, z, flags, with_q):
    """p through a wider tensor ([n][s+3][atoms+5], 1e30 outside), flags inside an observation of s*5+9 floats."""
    L, lib = _lib()
    n, s, atoms = p.shape
    wide = np.full((n, s + 3, atoms + 5), POISON, dtype=f32)
    wide[:, 1:1 + s, 2:2 + atoms] = p
    wide_d = torch.from_numpy(wide).to(DEV)
    p_d = wide_d[:, 1:1 + s, 2:2 + atoms]
    obs_d = None
    if flags is not None:
        obs = np.full((n, s * 5 + 9), 3.0, dtype=f32)
        obs[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
        obs_d = torch.from_numpy(obs).to(DEV)
    act_d = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    q_d = torch.full((n, s + 2), -5.0, dtype=torch.float32, device=DEV) if with_q else None
    z_d = torch.from_numpy(z).to(DEV)
    L.check(lib.irbpp_categorical_act(_ptr(p_d), p_d.stride(0), p_d.stride(1), _ptr(z_d), atoms, _ptr(obs_d),
                                      0 if obs_d is None else obs_d.stride(0), s, n, _ptr(act_d), _ptr(q_d), 0 if q_d is None else s + 2,
                                      _stream()), "irbpp_categorical_act")
    torch.cuda.synchronize()
    act = act_d.cpu().numpy()
    assert act[n] == -7, "the element after action[n] was written"
    q = None
    if with_q:
        q = q_d.cpu().numpy()
        assert (q[:, s:] == -5.0).all(), "q_out written beyond its s columns"
        q = q[:, :s]
    return act[:n], q


S_SET, ATOMS_SET, N_SET = [1, 63, 64, 65, 500, 1024], [2, 51, 64, 65, 128], [1, 3, 4, 5, 257]
ACT_CASES = [(s, a, N_SET[(i + j) % 5], (i + j) % 2 == 0, (i + 2 * j) % 3 != 0, i + j)
             for i, s in enumerate(S_SET) for j, a in enumerate(ATOMS_SET)]
# (257 envs x 1024 rows x 128 atoms would be 135 MB per tensor and a slow reference: that pair runs 257 envs at S = 65)
ACT_CASES = [(s, a, (5 if s * a > 40000 and n == 257 else n), o, q, k) for s, a, n, o, q, k in ACT_CASES] + \
            [(65, 128, 257, True, True, 3), (500, 51, 257, True, True, 0), (1024, 2, 257, False, False, 1)]


@pytest.mark.parametrize("s,atoms,n,with_obs,with_q,shift", ACT_CASES)
def test_act_bit_exact(s, atoms, n, with_obs, with_q, shift):
    z = _support(atoms).numpy()
    p, flags, _ = act_inputs(s, atoms, n, shift)
    want_a, want_q = act_np(p, z, flags if with_obs else None)
    got_a, got_q = run_act(p, z, flags if with_obs else None, with_q)
    if with_q:
        np.testing.assert_array_equal(got_q, want_q)
    np.testing.assert_array_equal(got_a, want_a)


def test_act_scenarios_choose_what_the_rules_say():
    """The scenarios' own expectations, independent of the numpy definition: first of two identical rows, the earlier trip of
    a tie, index 0 with everything masked, never a masked row."""
    s, atoms, n = 500, 51, 24
    z = _support(atoms).numpy()
    p, flags, scen = act_inputs(s, atoms, n, 0)
    got, _ = run_act(p, z, flags, False)
    spots = [0, 63, 64, s - 1]
    for e in range(n):
        r = spots[(e // 6) % 4]
        if scen[e] == 0:
            assert got[e] == r
        elif scen[e] == 1:
            assert got[e] == min(r, s - 2)
        elif scen[e] == 2:
            assert got[e] == min(r, s - 65)
        elif scen[e] == 3:
            assert got[e] == 0
        else:
            assert flags[e, got[e]] != 0 and (scen[e] != 4 or got[e] != r)
    free, _ = run_act(p, z, None, False)                 # obs = NULL: the masked best row of scenario 4 wins
    for e in np.nonzero(scen == 4)[0]:
        assert free[e] == spots[(e // 6) % 4]


# ------------------------------------------------------------------ target ------------
def target_inputs(b, s, atoms, z, v_min, v_max, shift):
    rng = np.random.default_rng(77 * b + s)
    p_on, p_tg = probabilities(rng, b, s, atoms), probabilities(rng, b, s, atoms)
    returns = rng.uniform(v_min, v_max, b).astype(f32)
    nonterm = np.ones(b, dtype=f32)
    top = np.zeros(atoms, dtype=f32)
    top[-1] = 1.0
    scen = (np.arange(b) + shift) % 8
    for k in range(b):
        c = scen[k]
        if c in (0, 1, 2):                               # terminal, the return exactly on atom 0 / a middle atom / atoms-1
            nonterm[k], returns[k] = 0, z[[0, atoms // 3, atoms - 1][c]]
        elif c == 3:
            returns[k] = v_min - 1.5
        elif c == 4:
            returns[k] = v_max + 2.25
        elif c == 5:                                     # the selected p_target row one-hot
            p_on[k, s // 2] = top
            p_tg[k, s // 2] = 0
            p_tg[k, s // 2, atoms // 2] = 1
        elif c == 6:                                     # a_star in the last row
            p_on[k, s - 1] = top
    return p_on, p_tg, returns, nonterm, scen


def run_target(p_on, p_tg, returns, nonterm, z, gamma_n, v_min, v_max, delta_z):
    L, lib = _lib()
    b, s, atoms = p_on.shape

    def widen(p, pad_r, pad_a):
        wide = np.full((b, s + pad_r, atoms + pad_a), POISON, dtype=f32)
        wide[:, :s, pad_a:] = p
        d = torch.from_numpy(wide).to(DEV)
        return d, d[:, :s, pad_a:]
    keep_on, on_d = widen(p_on, 2, 3)
    keep_tg, tg_d = widen(p_tg, 1, 6)
    m_d = torch.full((b + 1, atoms), -5.0, dtype=torch.float32, device=DEV)
    a_d = torch.full((b + 1,), -7, dtype=torch.int64, device=DEV)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)      # noqa: E731
    r_d, n_d, z_d = dev(returns), dev(nonterm), dev(z)
    L.check(lib.irbpp_categorical_target(_ptr(on_d), on_d.stride(0), on_d.stride(1), _ptr(tg_d), tg_d.stride(0), tg_d.stride(1),
                                         _ptr(r_d), _ptr(n_d), _ptr(z_d), atoms, s, b, float(gamma_n), float(v_min), float(v_max),
                                         float(delta_z), _ptr(m_d), _ptr(a_d), _stream()), "irbpp_categorical_target")
    torch.cuda.synchronize()
    m, a = m_d.cpu().numpy(), a_d.cpu().numpy()
    assert a[b] == -7 and (m[b] == -5.0).all(), "written beyond the batch"
    return m[:b], a[:b]


# delta_z = 0.25 (b exact: returns on an atom give l == u) and the reference-like (Vmax - Vmin) / (atoms - 1)
TARGET_CASES = [(1, 65, 51, True, 0), (1, 65, 51, True, 1), (1, 65, 51, True, 2), (4, 500, 51, False, 0), (4, 500, 51, True, 4),
                (64, 64, 128, True, 0), (64, 1024, 2, False, 0), (257, 63, 65, True, 0), (257, 1, 64, False, 0)]


@pytest.mark.parametrize("b,s,atoms,dyadic,shift", TARGET_CASES)
@pytest.mark.parametrize("gamma_n", [0.99 ** 3, 0.0])
def test_target_bit_exact(b, s, atoms, dyadic, shift, gamma_n):
    v_min = -2.0
    v_max = v_min + 0.25 * (atoms - 1) if dyadic else 7.0
    delta_z = (v_max - v_min) / (atoms - 1)
    z = _support(atoms, v_min, v_max).numpy()
    p_on, p_tg, returns, nonterm, scen = target_inputs(b, s, atoms, z, v_min, v_max, shift)
    want_m, want_a = target_np(p_on, p_tg, returns, nonterm, z, gamma_n, v_min, v_max, delta_z)
    got_m, got_a = run_target(p_on, p_tg, returns, nonterm, z, gamma_n, v_min, v_max, delta_z)
    np.testing.assert_array_equal(got_a, want_a)
    np.testing.assert_array_equal(got_m, want_m)
    if s > 1:
        assert (got_a[scen == 6] == s - 1).all() and (got_a[scen == 5] == s // 2).all()
    pns_a = p_tg[np.arange(b), got_a]
    if dyadic:                                           # the fix-ups were exercised: integral b at both ends and inside
        integral = project_np(pns_a, returns, nonterm, z, gamma_n, v_min, v_max, delta_z)[3]
        for c in (0, 1, 2):
            assert integral[scen == c].all()
    assert np.abs(got_m.astype(np.float64).sum(1) - pns_a.astype(np.float64).sum(1)).max() <= 2 * atoms * EPS


def test_target_is_the_same_from_run_to_run():
    atoms, v_min, v_max = 51, -1.0, 8.0
    z = _support(atoms, v_min, v_max).numpy()
    p_on, p_tg, returns, nonterm, _ = target_inputs(64, 130, atoms, z, v_min, v_max, 0)
    args = (p_on, p_tg, returns, nonterm, z, 0.99 ** 3, v_min, v_max, (v_max - v_min) / (atoms - 1))
    m0, a0 = run_target(*args)
    for _ in range(3):
        m1, a1 = run_target(*args)
        np.testing.assert_array_equal(m1, m0)
        np.testing.assert_array_equal(a1, a0)


# ------------------------------------------------------------------ wrappers, end to end ------------
def test_wrapper_act_against_the_torch_form():
    n, s, atoms = 37, 130, 51
    rng = np.random.default_rng(3)
    p = probabilities(rng, n, s, atoms)
    support = _support(atoms)
    z = support.numpy()
    flags = (rng.random((n, s)) < 0.7).astype(f32)
    flags[5] = 0
    state = np.zeros((n, s * 5 + 7), dtype=f32)
    state[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
    p_d, sup_d, st_d = torch.from_numpy(p).to(DEV), support.to(DEV), torch.from_numpy(state).to(DEV)
    absq = abs_sum(p, z)
    for st, fl in ((st_d, flags), (None, None)):
        want, want_q = act_torch(p_d, sup_d, None if fl is None else torch.from_numpy(fl).to(DEV))
        q_out = torch.empty((n, s), dtype=torch.float32, device=DEV)
        got = replay.distributional_greedy_action(p_d, sup_d, st, s if st is not None else None, q_out, use_hip=True)
        assert got.dtype == torch.int64 and got.shape == (n,)
        np.testing.assert_array_equal(q_out.cpu().numpy(), expected_np(p, z))
        assert np.all(np.abs(q_out.cpu().numpy().astype(np.float64) - want_q.cpu().numpy()) <= 2 * atoms * EPS * absq)
        ok = decided(expected_np(p, z), absq, atoms, fl)
        if fl is not None:
            ok |= (fl != 0).sum(1) == 0
        assert (~ok).mean() <= 0.02
        np.testing.assert_array_equal(got.cpu().numpy()[ok], want.cpu().numpy()[ok])
        assert torch.equal(got, replay.distributional_greedy_action(p_d, sup_d, st, use_hip=True))     # q_out absent
    # a column slice of a wider tensor goes to the kernel as it is
    wide = torch.full((n, s, atoms + 4), POISON, device=DEV)
    wide[:, :, 1:1 + atoms] = p_d
    np.testing.assert_array_equal(replay.distributional_greedy_action(wide[:, :, 1:1 + atoms], sup_d, st_d, use_hip=True).cpu().numpy(),
                                  act_np(p, z, flags)[0])


def test_wrapper_target_against_the_torch_form():
    """delta_z = 0.25 here: torch divides a device tensor by a Python scalar as a multiplication by its reciprocal, which is the
    IEEE division of the definition only where the reciprocal is exact; the bound on m does not cover that difference."""
    b, s, atoms, v_min = 64, 130, 51, -2.0
    v_max = v_min + 0.25 * (atoms - 1)
    support = _support(atoms, v_min, v_max)
    z = support.numpy()
    p_on, p_tg, returns, nonterm, _ = target_inputs(b, s, atoms, z, v_min, v_max, 0)
    g = 0.99 ** 3
    dev = lambda x: torch.from_numpy(x).to(DEV)          # noqa: E731
    want_m, want_a = learn_torch(dev(p_on), dev(p_tg), dev(returns), dev(nonterm).reshape(b, 1), support.to(DEV), g, v_min, v_max, atoms)
    m, a = replay.c51_target(dev(p_on), dev(p_tg), dev(returns), dev(nonterm).reshape(b, 1), support.to(DEV), g, v_min, v_max,
                             use_hip=True)
    assert m.dtype == torch.float32 and m.shape == (b, atoms) and a.dtype == torch.int64 and a.shape == (b,)
    ref_m, ref_a = target_np(p_on, p_tg, returns, nonterm, z, g, v_min, v_max, 0.25)
    np.testing.assert_array_equal(a.cpu().numpy(), ref_a)
    np.testing.assert_array_equal(m.cpu().numpy(), ref_m)
    ok = decided(expected_np(p_on, z), abs_sum(p_on, z), atoms)
    assert (~ok).mean() <= 0.02
    np.testing.assert_array_equal(a.cpu().numpy()[ok], want_a.cpu().numpy()[ok])
    assert np.abs(m.cpu().numpy()[ok].astype(np.float64) - want_m.cpu().numpy()[ok]).max() <= 2 * atoms * EPS
