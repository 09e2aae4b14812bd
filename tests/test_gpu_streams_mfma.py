"""csrc/irbpp_streams_mfma.hip on the GPU: irbpp_streams_act_mfma gives, bit for bit, what the numpy definition of
tests/test_streams_cpu.py and irbpp_streams_act give on the same inputs (v_out, a_out, q_out, action: assert_array_equal).
This is the experiment behind csrc/irbpp_mfma_chain.h: the float32 matrix instruction as a k-ordered fmaf chain.

The inputs are drawn so that the order of a chain is visible in its bits: x, the weights and the biases are
+-2^u (1 + v), u uniform in -6 .. 6, v uniform in [0, 1).  tests/test_streams_mfma_kernel_on_host.py checks, on these very
inputs, that the definition with k descending differs from the definition in every layer: a kernel with another order fails.

Cases (n_env, S, E, H, atoms): the smallest shape; a second row tile, a second block of hidden units and padded atom columns
(also with rows of x that are not 16-byte aligned: the element-wise loads); a second block of atoms; the reference's shape;
208 KB of logits, the workspace path (two launches).  x and x_global are slices of wider tensors (1e30 around them) in
every case; the masked rows come from observations with invalid candidates; env 1 has identical rows (a tie), the last env
of three is masked throughout."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
import test_gpu_streams as G
from test_streams_cpu import NAMES, f32, streams_act_np

pytestmark = pytest.mark.gpu
DEV = G.DEV
CASES = [(1, 1, 4, 4, 2), (3, 33, 12, 36, 31), (2, 70, 128, 128, 33), (2, 500, 128, 128, 31), (1, 1024, 8, 8, 51)]
# per case, a seed at which the descending chains differ from the definition in every layer
# (test_streams_mfma_kernel_on_host.py::test_the_inputs_tell_the_order_of_a_chain holds them to it)
SEEDS = {(1, 1, 4, 4, 2): 2, (3, 33, 12, 36, 31): 0, (2, 70, 128, 128, 33): 0, (2, 500, 128, 128, 31): 0, (1, 1024, 8, 8, 51): 0}


def draw(rng, *shape):
    """+-2^u (1 + v): u in -6 .. 6, v in [0, 1)"""
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return (sign * 2.0 ** rng.integers(-6, 7, shape) * (1.0 + rng.random(shape))).astype(f32)


@functools.lru_cache(maxsize=None)
def mfma_case(n, s, E, H, atoms):
    """-> W (the eight effective arrays), xg [n, E], x [n, s, E], flags [n, s], the definition's (action, q, v, a) with the
    flags, and its action without them: computed once and shared (treat as read-only)."""
    rng = np.random.default_rng([SEEDS[(n, s, E, H, atoms)], n, s, E, H, atoms])
    shapes = {"w_hv": (H, E), "b_hv": (H,), "w_zv": (atoms, H), "b_zv": (atoms,), "w_ha": (H, E), "b_ha": (H,), "w_za": (atoms, H),
              "b_za": (atoms,)}
    W = {k: draw(rng, *shapes[k]) for k in NAMES}
    xg, x = draw(rng, n, E), draw(rng, n, s, E)
    flags = (rng.random((n, s)) < 0.8).astype(f32)
    if n > 1:
        x[1] = x[1, 0]
        flags[1, 0] = 0
        flags[1, 1] = 1
    if n > 2:
        flags[2] = 0
    z = G.support_np(atoms)
    return W, xg, x, flags, streams_act_np(W, xg, x, z, flags), streams_act_np(W, xg, x, z, None)[0]


def run(name, W, xg, x, z, flags, with_action=True, with_q=True, with_v=True, with_a=True, front=4, expect=0):
    """One call of the entry point `name` on slices of wider tensors -> (action, q, v, a), None where not asked for; poison
    behind every output."""
    L, lib = G._lib()
    n, s, E = x.shape
    atoms = W["w_za"].shape[0]
    keep_w, ws = G.dev_weights(W)
    keep_x, x_d = G.widen_x(x, front=front, back=8 - front)
    keep_g, g_d = G.widen_g(xg)
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
    rc = getattr(lib, name)(C.byref(ws), G._ptr(g_d), g_d.stride(0), G._ptr(x_d), x_d.stride(0), x_d.stride(1), G._ptr(z_d), G._ptr(obs_d),
                            0 if obs_d is None else obs_d.stride(0), s, n, G._ptr(act_d), G._ptr(q_d), 0 if q_d is None else s + 2,
                            G._ptr(v_d), G._ptr(a_d), G._stream())
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


def same_bits(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.parametrize("n,s,E,H,atoms", CASES)
def test_the_bits_are_the_chains(n, s, E, H, atoms):
    z = G.support_np(atoms)
    W, xg, x, flags, (want_act, want_q, want_v, want_a), want_free = mfma_case(n, s, E, H, atoms)
    act, q, v, a = run("irbpp_streams_act_mfma", W, xg, x, z, flags)
    print("a_out elements that differ from the definition:", int((a.view(np.uint32) != want_a.view(np.uint32)).sum()), "of", a.size)
    same_bits(v, want_v)
    same_bits(a, want_a)
    same_bits(q, want_q)
    np.testing.assert_array_equal(act, want_act)
    c_act, c_q, c_v, c_a = run("irbpp_streams_act", W, xg, x, z, flags)
    same_bits(v, c_v)
    same_bits(a, c_a)
    same_bits(q, c_q)
    np.testing.assert_array_equal(act, c_act)
    fits = s * (atoms | 1) * 4 <= G.TILE_BYTES
    assert fits == ((n, s, E, H, atoms) != CASES[-1])
    # only the logits: no action, no q_out
    l_act, l_q, l_v, l_a = run("irbpp_streams_act_mfma", W, xg, x, z, None, with_action=False, with_q=False)
    assert l_act is None and l_q is None
    same_bits(l_v, want_v)
    same_bits(l_a, want_a)
    # no mask, and no logits where the block fits
    free = run("irbpp_streams_act_mfma", W, xg, x, z, None, with_q=False, with_v=False, with_a=not fits)[0]
    np.testing.assert_array_equal(free, want_free)
    if not fits:                                         # the workspace rule
        assert run("irbpp_streams_act_mfma", W, xg, x, z, flags, with_v=False, with_a=False, expect=-1) is None


def test_rows_that_are_not_aligned():
    n, s, E, H, atoms = CASES[1]
    z = G.support_np(atoms)
    W, xg, x, flags, (want_act, want_q, want_v, want_a), _ = mfma_case(n, s, E, H, atoms)
    act, q, v, a = run("irbpp_streams_act_mfma", W, xg, x, z, flags, front=1)
    same_bits(v, want_v)
    same_bits(a, want_a)
    same_bits(q, want_q)
    np.testing.assert_array_equal(act, want_act)


@pytest.mark.parametrize("case,e", [(1, 1), (2, 1)])
def test_an_environment_alone_equals_itself_in_the_batch(case, e):
    n, s, E, H, atoms = CASES[case]
    z = G.support_np(atoms)
    W, xg, x, flags, (want_act, want_q, want_v, want_a), _ = mfma_case(n, s, E, H, atoms)
    act, q, v, a = run("irbpp_streams_act_mfma", W, xg[e:e + 1], x[e:e + 1], z, flags[e:e + 1])
    same_bits(v[0], want_v[e])
    same_bits(a[0], want_a[e])
    same_bits(q[0], want_q[e])
    assert act[0] == want_act[e]


class _EvalLayer(object):
    """A layer whose mu tensors are the effective ones (StreamWeights with training=False takes them as they are)."""

    def __init__(self, w, b):
        self.weight_mu = self.weight_sigma = self.weight_epsilon = torch.from_numpy(w).to(DEV)
        self.bias_mu = self.bias_sigma = self.bias_epsilon = torch.from_numpy(b).to(DEV)


def _stream_weights(W):
    return replay.StreamWeights.from_layers(*(_EvalLayer(W[NAMES[2 * i]], W[NAMES[2 * i + 1]]) for i in range(4)), training=False)


@pytest.mark.parametrize("case", [1, 4])
def test_the_wrappers_take_the_form(case):
    n, s, E, H, atoms = CASES[case]
    W, xg, x, flags, (want_act, want_q, want_v, want_a), _ = mfma_case(n, s, E, H, atoms)
    w = _stream_weights(W)
    support = torch.linspace(G.V_MIN, G.V_MAX, atoms, device=DEV)
    state = np.zeros((n, s * 5 + 7), dtype=f32)
    state[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
    st_d = torch.from_numpy(state).to(DEV)
    keep_x, x_d = G.widen_x(x)
    keep_g, g_d = G.widen_g(xg)
    got = {}
    for form in replay.STREAMS_FORMS:
        q = torch.empty((n, s), dtype=torch.float32, device=DEV)
        act = replay.streams_greedy_action(x_d, g_d, w, support, st_d, q_out=q, use_hip=True, form=form)
        v, a = replay.streams_logits(x_d, g_d, w, use_hip=True, form=form)
        got[form] = (act, q, v, a)
    for c, m in zip(got["chain"], got["mfma"]):
        assert torch.equal(c, m)
    act, q, v, a = got["mfma"]
    np.testing.assert_array_equal(act.cpu().numpy(), want_act)
    same_bits(q.cpu().numpy(), want_q)
    same_bits(v.cpu().numpy(), want_v)
    same_bits(a.cpu().numpy(), want_a)
    with pytest.raises(ValueError):
        replay.streams_logits(x_d, g_d, w, use_hip=True, form="matrix")


def test_widths_that_are_no_multiple_of_four_are_refused():
    L, lib = G._lib()
    rng = np.random.default_rng(9)
    n, s, atoms = 2, 5, 31
    z = G.support_np(atoms)
    for E, H in ((6, 8), (8, 6)):
        shapes = {"w_hv": (H, E), "b_hv": (H,), "w_zv": (atoms, H), "b_zv": (atoms,), "w_ha": (H, E), "b_ha": (H,), "w_za": (atoms, H),
                  "b_za": (atoms,)}
        W = {k: draw(rng, *shapes[k]) for k in NAMES}
        xg, x = draw(rng, n, E), draw(rng, n, s, E)
        assert run("irbpp_streams_act_mfma", W, xg, x, z, None, expect=-1) is None          # IRBPP_ERR_ARG through the ABI
        assert run("irbpp_streams_act", W, xg, x, z, None) is not None                        # the chain kernel takes them
        w = _stream_weights(W)
        x_d, g_d = torch.from_numpy(x).to(DEV), torch.from_numpy(xg).to(DEV)
        support = torch.from_numpy(z).to(DEV)
        with pytest.raises(ValueError, match="multiples of 4"):
            replay.streams_greedy_action(x_d, g_d, w, support, use_hip=True, form="mfma")
        with pytest.raises(ValueError, match="multiples of 4"):
            replay.streams_logits(x_d, g_d, w, use_hip=True, form="mfma")
        assert replay.streams_greedy_action(x_d, g_d, w, support, use_hip=True, form="chain").shape == (n,)
