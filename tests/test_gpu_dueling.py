"""csrc/irbpp_dueling.hip on the GPU, bit for bit against the numpy float32 definition of tests/test_dueling_cpu.py (action,
q_out, p_out, m, a_star: assert_array_equal), through the C ABI with strided arguments on the current stream; then the two
cross-checks that tie the new head to irbpp_c51.hip, and the status codes.

Shapes (S, atoms): (1, 2) and (3, 2) the smallest block and fewer rows than partial sums; (63 | 64 | 65, 31) around one wave of
row-per-thread work; (500, 31) the acting loop's block, 12 idle threads in its one trip; (600, 5) more rows than the 512
threads: a second, short trip of the row loop, with a row length that does not divide 512; (129, 128) the widest rows and a
tile above 64 KB; (1024, 128) the largest block.  The LDS threshold is DUELING_TILE_BYTES = 144 KB for S * (atoms | 1) * 4
bytes: RESIDENT shapes stay in LDS, STAGED ones (only (1024, 128): 528 KB) take their column sums from global memory and
are staged 256 rows at a time, four trips.  N and B are 1 and 3, and 257 once.  Every case slices `a` out of a wider tensor
(row and env stride, 1e30 around it) and `v` out of wider rows; its envs cycle through six scenarios (see head_case)."""
import ctypes as C

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_dueling_cpu import dueling_act_np, dueling_target_np, f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 1e30
TILE_BYTES = 144 * 1024
RESIDENT = [(1, 2), (3, 2), (63, 31), (64, 31), (65, 31), (500, 31), (600, 5), (129, 128)]
STAGED = [(1024, 128)]
SHAPES = RESIDENT + STAGED
assert all(s * (a | 1) * 4 <= TILE_BYTES for s, a in RESIDENT) and all(s * (a | 1) * 4 > TILE_BYTES for s, a in STAGED)
CASES = [(s, a, n) for s, a in SHAPES for n in (1, 3)] + [(65, 31, 257)]
V_MIN, V_MAX, GAMMA_N = -1.0, 8.0, 0.99 ** 3


def support_np(atoms, v_min=V_MIN, v_max=V_MAX):
    return torch.linspace(v_min, v_max, atoms).numpy()


def head_case(s, atoms, n, seed=0):
    """-> v [n, atoms], a [n, s, atoms], flags [n, s], scenario per env.  Scenarios (env index + seed mod 6):
    0 a planted best row (its last-atom logit + 30), valid;  1 two identical best rows, an exact tie: the first wins;
    2 every row masked: index 0;  3 the best row masked;  4 logits times 60: most e are exactly 0 (t < -80);  5 plain."""
    rng = np.random.default_rng(1000 * s + atoms + seed)
    v = rng.standard_normal((n, atoms)).astype(f32)
    a = rng.standard_normal((n, s, atoms)).astype(f32)
    flags = (rng.random((n, s)) < 0.8).astype(f32)
    scen = (np.arange(n) + seed) % 6
    spots = [0, 63, 64, s - 1, 255, 256, 511, 512]
    for e in range(n):
        r = min(spots[(e // 6 + seed) % 8], s - 1)
        if scen[e] == 0:
            a[e, r, -1] += 30
            flags[e, r] = 1
        elif scen[e] == 1 and s >= 2:
            r = min(r, s - 2)
            a[e, r, -1] += 30
            a[e, s - 1] = a[e, r]
            flags[e, r], flags[e, s - 1] = 1, 1
        elif scen[e] == 2:
            flags[e] = 0
        elif scen[e] == 3:
            a[e, r, -1] += 30
            flags[e, r] = 0
        elif scen[e] == 4:
            a[e] *= 60
    return v, a, flags, scen


def target_case(b, s, atoms, z, seed=0):
    """online and target logits, returns, nonterminals.  Samples cycle (index mod 5): terminal with the return exactly on an atom
    (nonterminal 0);  a return that clamps at Vmin;  one that clamps at Vmax;  two plain non-terminal ones."""
    v_on, a_on, _, _ = head_case(s, atoms, b, seed)
    v_tg, a_tg, _, _ = head_case(s, atoms, b, seed + 3)
    rng = np.random.default_rng(77 * b + s)
    returns = rng.uniform(V_MIN, V_MAX, b).astype(f32)
    nonterm = np.ones(b, dtype=f32)
    for k in range(b):
        c = (k + seed) % 5
        if c == 0:
            nonterm[k], returns[k] = 0, z[(3 * k) % atoms]
        elif c == 1:
            returns[k] = V_MIN - 20.5
        elif c == 2:
            returns[k] = V_MAX + 20.25
    return v_on, a_on, v_tg, a_tg, returns, nonterm


def _lib():
    from irbpp_amd import _lib as L
    return L, L.load()


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def widen(a, pad_rows, pad_front, pad_back):
    """[n, s, atoms] -> (the wider device tensor to keep alive, the slice holding a)"""
    n, s, atoms = a.shape
    wide = np.full((n, s + pad_rows, atoms + pad_front + pad_back), POISON, dtype=f32)
    wide[:, 1:1 + s, pad_front:pad_front + atoms] = a
    d = torch.from_numpy(wide).to(DEV)
    return d, d[:, 1:1 + s, pad_front:pad_front + atoms]


def widen_v(v):
    wide = np.full((v.shape[0], v.shape[1] + 7), POISON, dtype=f32)
    wide[:, 3:3 + v.shape[1]] = v
    d = torch.from_numpy(wide).to(DEV)
    return d, d[:, 3:3 + v.shape[1]]


def run_act(v, a, z, flags, with_q, with_p):
    L, lib = _lib()
    n, s, atoms = a.shape
    keep_a, a_d = widen(a, 3, 2, 3)
    keep_v, v_d = widen_v(v)
    obs_d = None
    if flags is not None:
        obs = np.full((n, s * 5 + 9), 3.0, dtype=f32)
        obs[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
        obs_d = torch.from_numpy(obs).to(DEV)
    act_d = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    q_d = torch.full((n, s + 2), -5.0, dtype=torch.float32, device=DEV) if with_q else None
    p_d = torch.full((n * s * atoms + 4,), -5.0, dtype=torch.float32, device=DEV) if with_p else None
    z_d = torch.from_numpy(z).to(DEV)
    L.check(lib.irbpp_dueling_act(_ptr(v_d), v_d.stride(0), _ptr(a_d), a_d.stride(0), a_d.stride(1), _ptr(z_d), atoms, _ptr(obs_d),
                                  0 if obs_d is None else obs_d.stride(0), s, n, _ptr(act_d), _ptr(q_d), 0 if q_d is None else s + 2,
                                  _ptr(p_d), _stream()), "irbpp_dueling_act")
    torch.cuda.synchronize()
    act = act_d.cpu().numpy()
    assert act[n] == -7, "the element after action[n] was written"
    q = p = None
    if with_q:
        q = q_d.cpu().numpy()
        assert (q[:, s:] == -5.0).all(), "q_out written beyond its s columns"
        q = q[:, :s]
    if with_p:
        p = p_d.cpu().numpy()
        assert (p[n * s * atoms:] == -5.0).all(), "p_out written beyond its end"
        p = p[:n * s * atoms].reshape(n, s, atoms)
    return act[:n], q, p


@pytest.mark.parametrize("s,atoms,n", CASES)
def test_act_bit_exact(s, atoms, n):
    z = support_np(atoms)
    v, a, flags, scen = head_case(s, atoms, n)
    want_a, want_q, want_p = dueling_act_np(v, a, z, flags)
    got_a, got_q, got_p = run_act(v, a, z, flags, True, True)
    np.testing.assert_array_equal(got_p, want_p)
    np.testing.assert_array_equal(got_q, want_q)
    np.testing.assert_array_equal(got_a, want_a)
    assert (got_a[scen == 2] == 0).all()
    if (scen == 4).any():
        assert (want_p[scen == 4] == 0).mean() > 0.5 or atoms == 2, "scenario 4 is meant to drive most e to exactly 0"
    free_a, _, _ = run_act(v, a, z, None, False, False)              # no mask, no q_out, no p_out
    np.testing.assert_array_equal(free_a, dueling_act_np(v, a, z)[0])


def test_act_scenarios_choose_what_the_rules_say():
    """The scenarios' own expectations, independent of the numpy definition."""
    s, atoms, n = 500, 31, 48
    z = support_np(atoms)
    v, a, flags, scen = head_case(s, atoms, n)
    got, _, _ = run_act(v, a, z, flags, False, False)
    free, _, _ = run_act(v, a, z, None, False, False)
    spots = [0, 63, 64, s - 1, 255, 256, 511, 512]
    for e in range(n):
        r = min(spots[(e // 6) % 8], s - 1)
        if scen[e] == 0:
            assert got[e] == r and free[e] == r
        elif scen[e] == 1:
            assert got[e] == min(r, s - 2) and free[e] == min(r, s - 2)
        elif scen[e] == 2:
            assert got[e] == 0
        elif scen[e] == 3:
            assert got[e] != r and flags[e, got[e]] != 0 and free[e] == r
        else:
            assert flags[e, got[e]] != 0


def run_target(v_on, a_on, v_tg, a_tg, returns, nonterm, z, gamma_n, delta_z):
    L, lib = _lib()
    b, s, atoms = a_on.shape
    keep1, on_d = widen(a_on, 2, 3, 0)
    keep2, tg_d = widen(a_tg, 1, 6, 1)
    keep3, von_d = widen_v(v_on)
    keep4, vtg_d = widen_v(v_tg)
    m_d = torch.full((b + 1, atoms), -5.0, dtype=torch.float32, device=DEV)
    s_d = torch.full((b + 1,), -7, dtype=torch.int64, device=DEV)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)      # noqa: E731
    r_d, n_d, z_d = dev(returns), dev(nonterm), dev(z)
    L.check(lib.irbpp_dueling_target(_ptr(von_d), von_d.stride(0), _ptr(on_d), on_d.stride(0), on_d.stride(1), _ptr(vtg_d),
                                     vtg_d.stride(0), _ptr(tg_d), tg_d.stride(0), tg_d.stride(1), _ptr(r_d), _ptr(n_d), _ptr(z_d),
                                     atoms, s, b, float(gamma_n), V_MIN, V_MAX, float(delta_z), _ptr(m_d), _ptr(s_d), _stream()),
            "irbpp_dueling_target")
    torch.cuda.synchronize()
    m, a_star = m_d.cpu().numpy(), s_d.cpu().numpy()
    assert a_star[b] == -7 and (m[b] == -5.0).all(), "written beyond the batch"
    return m[:b], a_star[:b]


@pytest.mark.parametrize("s,atoms,b", CASES)
def test_target_bit_exact(s, atoms, b):
    z = support_np(atoms)
    delta_z = (V_MAX - V_MIN) / (atoms - 1)
    args = target_case(b, s, atoms, z)
    for gamma_n in (GAMMA_N, 0.0):
        want_m, want_a = dueling_target_np(*args, z, gamma_n, V_MIN, V_MAX, delta_z)
        got_m, got_a = run_target(*args, z, gamma_n, delta_z)
        np.testing.assert_array_equal(got_a, want_a)
        np.testing.assert_array_equal(got_m, want_m)
    returns = args[4]
    for k in range(b):                                   # a clamped return (gamma_n = 0: Tz is the return) puts the mass on the end
        if k % 5 in (1, 2):                              # atom; its neighbour gets what b = (Vmax - Vmin) / delta_z rounds below atoms - 1
            end, nxt = (0, 1) if returns[k] < V_MIN else (atoms - 1, atoms - 2)
            assert got_m[k, end] > 0.999 and (np.delete(got_m[k], [end, nxt]) == 0).all()


# ------------------------------------------------------------------ the new head against the old one ------------
@pytest.mark.parametrize("s,atoms,n", [(65, 31, 3), (500, 31, 3), (1024, 128, 1)])
def test_wrappers_agree_with_the_categorical_kernels_on_p_out(s, atoms, n):
    """dueling_greedy_action's p_out fed to distributional_greedy_action gives the same action and the same Q; dueling_c51_target
    equals c51_target on the two p_out blocks: bit for bit, and equal to the definition."""
    support = torch.linspace(V_MIN, V_MAX, atoms)
    z = support.numpy()
    v_on, a_on, v_tg, a_tg, returns, nonterm = target_case(n, s, atoms, z)
    flags = head_case(s, atoms, n)[2]
    state = np.zeros((n, s * 5 + 7), dtype=f32)
    state[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
    d = lambda x: torch.from_numpy(x).to(DEV)            # noqa: E731
    sup_d, st_d = support.to(DEV), d(state)
    P, Q = {}, {}
    for name, (v, a) in (("on", (v_on, a_on)), ("tg", (v_tg, a_tg))):
        P[name] = torch.empty((n, s, atoms), dtype=torch.float32, device=DEV)
        Q[name] = torch.empty((n, s), dtype=torch.float32, device=DEV)
        act = replay.dueling_greedy_action(d(v), d(a), sup_d, st_d, s, Q[name], P[name], use_hip=True)
        assert act.dtype == torch.int64 and act.shape == (n,)
        want_a, want_q, want_p = dueling_act_np(v, a, z, flags)
        np.testing.assert_array_equal(P[name].cpu().numpy(), want_p)
        np.testing.assert_array_equal(act.cpu().numpy(), want_a)
        q_old = torch.empty((n, s), dtype=torch.float32, device=DEV)
        act_old = replay.distributional_greedy_action(P[name], sup_d, st_d, s, q_old, use_hip=True)
        assert torch.equal(act_old, act) and torch.equal(q_old, Q[name])
        assert torch.equal(replay.dueling_greedy_action(d(v).view(n, 1, atoms), d(a), sup_d, st_d, use_hip=True), act)
    m, a_star = replay.dueling_c51_target(d(v_on), d(a_on), d(v_tg), d(a_tg), d(returns), d(nonterm).reshape(n, 1), sup_d, GAMMA_N,
                                          V_MIN, V_MAX, use_hip=True)
    m_old, a_old = replay.c51_target(P["on"], P["tg"], d(returns), d(nonterm).reshape(n, 1), sup_d, GAMMA_N, V_MIN, V_MAX,
                                     use_hip=True)
    assert m.dtype == torch.float32 and m.shape == (n, atoms) and a_star.dtype == torch.int64 and a_star.shape == (n,)
    assert torch.equal(a_star, a_old) and torch.equal(m, m_old)
    want_m, want_s = dueling_target_np(v_on, a_on, v_tg, a_tg, returns, nonterm, z, GAMMA_N, V_MIN, V_MAX,
                                       (V_MAX - V_MIN) / (atoms - 1))
    np.testing.assert_array_equal(a_star.cpu().numpy(), want_s)
    np.testing.assert_array_equal(m.cpu().numpy(), want_m)


# ------------------------------------------------------------------ status codes ------------
def test_status_codes_on_device_pointers():
    """Arguments outside the limits answer IRBPP_ERR_ARG before anything is launched, and `check` turns that into an exception;
    the same call inside the limits answers IRBPP_OK."""
    L, lib = _lib()
    n, s, atoms = 2, 4, 31
    buf = torch.zeros((n * s * atoms,), dtype=torch.float32, device=DEV)
    act = torch.zeros((n,), dtype=torch.int64, device=DEV)

    def call(atoms=atoms, s=s, n=n, row=atoms, vs=atoms):
        return lib.irbpp_dueling_act(_ptr(buf), vs, _ptr(buf), s * row, row, _ptr(buf), atoms, None, 0, s, n, _ptr(act), None, 0, None,
                                     _stream())
    L.check(call(), "irbpp_dueling_act")
    torch.cuda.synchronize()
    for bad in (dict(atoms=1), dict(atoms=129), dict(s=0), dict(s=1025), dict(n=0), dict(row=atoms - 1), dict(vs=atoms - 1)):
        assert call(**bad) == -1
        with pytest.raises(L.IrbppError):
            L.check(call(**bad), "irbpp_dueling_act")
    m = torch.zeros((n, atoms), dtype=torch.float32, device=DEV)

    def call_t(batch=n, delta_z=0.3, v_max=8.0):
        return lib.irbpp_dueling_target(_ptr(buf), atoms, _ptr(buf), s * atoms, atoms, _ptr(buf), atoms, _ptr(buf), s * atoms, atoms,
                                        _ptr(buf), _ptr(buf), _ptr(buf), atoms, s, batch, 0.97, -1.0, v_max, delta_z, _ptr(m), _ptr(act),
                                        _stream())
    L.check(call_t(), "irbpp_dueling_target")
    torch.cuda.synchronize()
    for bad in (dict(batch=0), dict(delta_z=0.0), dict(v_max=-1.0)):
        with pytest.raises(L.IrbppError):
            L.check(call_t(**bad), "irbpp_dueling_target")
