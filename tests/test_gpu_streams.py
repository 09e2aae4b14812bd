"""csrc/irbpp_streams.hip on the GPU, bit for bit against the numpy definition of tests/test_streams_cpu.py (action, q_out,
v_out, a_out: assert_array_equal), through the C ABI with strided arguments on the current stream; then the cross-checks that
tie the new head to irbpp_dueling.hip and torch, and the status codes.

Shapes (S, E, H, atoms), N = 3: every S of {1, 2, 63, 64, 65, 500} (fewer rows than partial sums, around one wave of
row-per-thread work, the acting loop's block) and 600 (a second trip of the row loop) with the block resident in LDS, 500 and
1024 rows of 128 atoms on the workspace path (S * (atoms | 1) * 4 above 144 KB: two launches); every (E, H) of {(128, 128),
(5, 3), (130, 67), (256, 256)}: the vectorised x reads and the scalar ones, a last block of hidden units that is full, short
and a single short one; atoms {2, 31} on the 32-accumulator instantiation, {51, 128} on the 128 one.  Every case slices x and
xg out of wider tensors (1e30 around them); env 0 is plain with a random mask, env 1 has identical rows (an exact tie: the
first valid row wins), env 2 is masked throughout (index 0)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_streams_cpu import NAMES, effective_np, f32, make_layers, streams_act_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 1e30
TILE_BYTES = 144 * 1024
RESIDENT = [(1, 5, 3, 2), (2, 130, 67, 31), (63, 128, 128, 31), (64, 5, 3, 51), (65, 256, 256, 31), (500, 128, 128, 31), (600, 130, 67, 51),
            (65, 130, 67, 128), (64, 128, 128, 2)]
WORKSPACE = [(1024, 5, 3, 128), (500, 128, 128, 128)]
CASES = RESIDENT + WORKSPACE
assert all(s * (a | 1) * 4 <= TILE_BYTES for s, _, _, a in RESIDENT) and all(s * (a | 1) * 4 > TILE_BYTES for s, _, _, a in WORKSPACE)
V_MIN, V_MAX = -1.0, 8.0


def support_np(atoms):
    return torch.linspace(V_MIN, V_MAX, atoms).numpy()


@functools.lru_cache(maxsize=None)
def stream_case(s, E, H, atoms, n=3, seed=0):
    """-> layers, W (effective, numpy), xg [n, E], x [n, s, E], flags [n, s], and the definition's (action, q, v, a) with the
    flags and the action without them: computed once and shared (treat as read-only)."""
    rng = np.random.default_rng(7000 * s + 31 * E + H + atoms + seed)
    layers = make_layers(rng, E, H, atoms)
    W = effective_np(layers)
    xg = rng.standard_normal((n, E)).astype(f32)
    x = rng.standard_normal((n, s, E)).astype(f32)
    flags = (rng.random((n, s)) < 0.8).astype(f32)
    if n > 1:
        x[1] = x[1, 0]
        flags[1, 0] = 0
        if s > 1:
            flags[1, 1] = 1
    if n > 2:
        flags[2] = 0
    z = support_np(atoms)
    want = streams_act_np(W, xg, x, z, flags)
    free = streams_act_np(W, xg, x, z, None)[0]
    return layers, W, xg, x, flags, want, free


def _lib():
    from irbpp_amd import _lib as L
    return L, L.load()


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def dev_weights(W):
    """-> (tensors to keep alive, the C struct)"""
    keep = [torch.from_numpy(np.ascontiguousarray(W[n])).to(DEV) for n in NAMES]
    H, E = W["w_ha"].shape
    return keep, replay._IrbppStreamWeights(*(t.data_ptr() for t in keep), E, H, W["w_za"].shape[0])


def widen_x(x, pad_rows=3, front=4, back=4):
    n, s, E = x.shape
    wide = np.full((n, s + pad_rows, E + front + back), POISON, dtype=f32)
    wide[:, 1:1 + s, front:front + E] = x
    d = torch.from_numpy(wide).to(DEV)
    return d, d[:, 1:1 + s, front:front + E]


def widen_g(xg, front=3):
    wide = np.full((xg.shape[0], xg.shape[1] + 7), POISON, dtype=f32)
    wide[:, front:front + xg.shape[1]] = xg
    d = torch.from_numpy(wide).to(DEV)
    return d, d[:, front:front + xg.shape[1]]


def run_streams(W, xg, x, z, flags, with_action=True, with_q=True, with_v=True, with_a=True, front=4, expect=0):
    """One irbpp_streams_act call on slices of wider tensors -> (action, q, v, a), None where not asked for; `front`: floats in
    front of every x row (4: rows stay 16-byte aligned where E allows; 1: they do not)."""
    L, lib = _lib()
    n, s, E = x.shape
    atoms = W["w_za"].shape[0]
    keep_w, ws = dev_weights(W)
    keep_x, x_d = widen_x(x, front=front, back=8 - front)
    keep_g, g_d = widen_g(xg)
    obs_d = None
    if flags is not None:
        obs = np.full((n, s * 5 + 9), 3.0, dtype=f32)
        obs[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
        obs_d = torch.from_numpy(obs).to(DEV)
    act_d = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV) if with_action else None
    q_d = torch.full((n, s + 2), -5.0, dtype=torch.float32, device=DEV) if with_q else None
    v_d = torch.full((n * atoms + 4,), -5.0, dtype=torch.float32, device=DEV) if with_v else None
    a_d = torch.full((n * s * atoms + 4,), -5.0, dtype=torch.float32, device=DEV) if with_a else None
    z_d = torch.from_numpy(z).to(DEV)
    rc = lib.irbpp_streams_act(C.byref(ws), _ptr(g_d), g_d.stride(0), _ptr(x_d), x_d.stride(0), x_d.stride(1), _ptr(z_d), _ptr(obs_d),
                               0 if obs_d is None else obs_d.stride(0), s, n, _ptr(act_d), _ptr(q_d), 0 if q_d is None else s + 2,
                               _ptr(v_d), _ptr(a_d), _stream())
    assert rc == expect
    torch.cuda.synchronize()
    if rc != 0:
        return None
    act = q = v = a = None
    if with_action:
        act = act_d.cpu().numpy()
        assert act[n] == -7, "the element after action[n] was written"
        act = act[:n]
    if with_q:
        q = q_d.cpu().numpy()
        assert (q[:, s:] == -5.0).all(), "q_out written beyond its s columns"
        q = q[:, :s]
    if with_v:
        v = v_d.cpu().numpy()
        assert (v[n * atoms:] == -5.0).all(), "v_out written beyond its end"
        v = v[:n * atoms].reshape(n, atoms)
    if with_a:
        a = a_d.cpu().numpy()
        assert (a[n * s * atoms:] == -5.0).all(), "a_out written beyond its end"
        a = a[:n * s * atoms].reshape(n, s, atoms)
    return act, q, v, a


def first_valid(flags_row):
    nz = np.flatnonzero(flags_row)
    return int(nz[0]) if len(nz) else 0


@pytest.mark.parametrize("s,E,H,atoms", CASES)
def test_bit_exact(s, E, H, atoms):
    z = support_np(atoms)
    _, W, xg, x, flags, (want_act, want_q, want_v, want_a), want_free = stream_case(s, E, H, atoms)
    act, q, v, a = run_streams(W, xg, x, z, flags)
    np.testing.assert_array_equal(v, want_v)
    np.testing.assert_array_equal(a, want_a)
    np.testing.assert_array_equal(q, want_q)
    np.testing.assert_array_equal(act, want_act)
    assert act[1] == first_valid(flags[1]) and act[2] == 0          # the tie under a mask; every row masked
    fits = s * (atoms | 1) * 4 <= TILE_BYTES
    free = run_streams(W, xg, x, z, None, with_q=False, with_v=False, with_a=not fits, front=1)[0]   # unaligned rows, no mask
    np.testing.assert_array_equal(free, want_free)
    assert free[1] == 0                                              # the tie: the first maximum wins


@pytest.mark.parametrize("s,E,H,atoms", [(65, 256, 256, 31), (1024, 5, 3, 128)])
def test_logits_only_and_the_workspace_rule(s, E, H, atoms):
    z = support_np(atoms)
    _, W, xg, x, flags, (_, _, want_v, want_a), _ = stream_case(s, E, H, atoms)
    act, q, v, a = run_streams(W, xg, x, z, None, with_action=False, with_q=False)       # action_dev = NULL: logits only
    assert act is None and q is None
    np.testing.assert_array_equal(v, want_v)
    np.testing.assert_array_equal(a, want_a)
    fits = s * (atoms | 1) * 4 <= TILE_BYTES
    out = run_streams(W, xg, x, z, flags, with_v=False, with_a=False, expect=0 if fits else -1)   # no workspace: IRBPP_ERR_ARG
    assert (out is None) != fits


def test_a_hidden_layer_below_zero_gives_the_bias_rows():
    s, E, H, atoms = 65, 130, 67, 31
    _, W, xg, x, flags, _, _ = stream_case(s, E, H, atoms)
    W = dict(W)
    W["b_ha"] = np.full(H, -1e4, dtype=f32)
    z = support_np(atoms)
    act, q, v, a = run_streams(W, xg, x, z, flags)
    assert (a == W["b_za"][None, None, :]).all() and not np.signbit(a[a == 0]).any()
    assert [int(i) for i in act] == [first_valid(flags[0]), first_valid(flags[1]), 0]
    want = streams_act_np(W, xg, x, z, flags)
    np.testing.assert_array_equal(q, want[1])
    free = run_streams(W, xg, x, z, None, with_q=False, with_v=False, with_a=False)[0]
    assert (free == 0).all()


# ------------------------------------------------------------------ consistency with existing code ------------
@pytest.mark.parametrize("training", [True, False])
def test_noisy_weights_are_torchs_on_the_device(training):
    rng = np.random.default_rng(3)
    layers = [l.to(DEV) for l in make_layers(rng, 130, 67, 31)]
    w = replay.StreamWeights.from_layers(*layers, training=training)
    for (wn, bn), l in zip((("w_hv", "b_hv"), ("w_zv", "b_zv"), ("w_ha", "b_ha"), ("w_za", "b_za")), layers):
        tw = l.weight_mu + l.weight_sigma * l.weight_epsilon if training else l.weight_mu
        tb = l.bias_mu + l.bias_sigma * l.bias_epsilon if training else l.bias_mu
        assert getattr(w, wn).is_cuda and torch.equal(getattr(w, wn), tw) and torch.equal(getattr(w, bn), tb)
    want = effective_np(layers, training)
    np.testing.assert_array_equal(w.w_ha.cpu().numpy(), want["w_ha"])


@pytest.mark.parametrize("s,E,H,atoms", [(500, 128, 128, 31), (65, 130, 67, 128), (1024, 5, 3, 128)])
def test_wrappers_agree_with_the_dueling_head(s, E, H, atoms):
    """streams_logits followed by the existing dueling_greedy_action gives the actions and q_out bits of streams_greedy_action,
    and both equal the definition."""
    layers, W, xg, x, flags, (want_act, want_q, want_v, want_a), _ = stream_case(s, E, H, atoms)
    n = x.shape[0]
    w = replay.StreamWeights.from_layers(*[l.to(DEV) for l in layers])
    np.testing.assert_array_equal(w.w_za.cpu().numpy(), W["w_za"])
    support = torch.linspace(V_MIN, V_MAX, atoms, device=DEV)
    state = np.zeros((n, s * 5 + 7), dtype=f32)
    state[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
    st_d = torch.from_numpy(state).to(DEV)
    keep_x, x_d = widen_x(x)
    keep_g, g_d = widen_g(xg)
    q_new = torch.empty((n, s), dtype=torch.float32, device=DEV)
    act = replay.streams_greedy_action(x_d, g_d.unsqueeze(1), w, support, st_d, q_out=q_new, use_hip=True)
    assert act.dtype == torch.int64 and act.shape == (n,)
    v, a = replay.streams_logits(x_d, g_d, w, use_hip=True)
    assert v.shape == (n, atoms) and a.shape == (n, s, atoms) and not a.requires_grad
    q_old = torch.empty((n, s), dtype=torch.float32, device=DEV)
    act_old = replay.dueling_greedy_action(v, a, support, st_d, s, q_old, use_hip=True)
    assert torch.equal(act, act_old) and torch.equal(q_new, q_old)
    np.testing.assert_array_equal(act.cpu().numpy(), want_act)
    np.testing.assert_array_equal(q_new.cpu().numpy(), want_q)
    np.testing.assert_array_equal(v.cpu().numpy(), want_v)
    np.testing.assert_array_equal(a.cpu().numpy(), want_a)
    v_t, a_t = replay.streams_logits(x_d, g_d, w, use_hip=False)      # torch's layers: close to, not bit-equal with, the chains
    assert (a_t - a).abs().max() < 1e-3 and (v_t - v).abs().max() < 1e-3


def test_limits_are_rejected_before_any_launch():
    L, lib = _lib()
    _, W, xg, x, _, _, _ = stream_case(2, 130, 67, 31)
    n, s, E = x.shape
    keep, ws = dev_weights(W)
    buf = torch.zeros((n * s * E + 64,), dtype=torch.float32, device=DEV)
    act = torch.zeros((n,), dtype=torch.int64, device=DEV)

    def call(E=E, H=67, atoms=31, s=s, n=n, row=E, gs=E, action=act, a_out=None):
        w2 = replay._IrbppStreamWeights(*(t.data_ptr() for t in keep), E, H, atoms)
        return lib.irbpp_streams_act(C.byref(w2), _ptr(buf), gs, _ptr(buf), s * row, row, _ptr(buf), None, 0, s, n, _ptr(action), None, 0,
                                     None, _ptr(a_out), _stream())
    L.check(call(), "irbpp_streams_act")
    torch.cuda.synchronize()
    for bad in (dict(E=0), dict(E=257), dict(H=0), dict(H=257), dict(atoms=1), dict(atoms=129), dict(s=0), dict(s=1025), dict(n=0),
                dict(row=E - 1), dict(gs=E - 1), dict(action=None)):
        assert call(**bad) == -1
        with pytest.raises(L.IrbppError):
            L.check(call(**bad), "irbpp_streams_act")
    torch.cuda.synchronize()
