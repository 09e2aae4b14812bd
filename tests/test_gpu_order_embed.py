"""csrc/irbpp_order_embed.hip on the GPU, bit for bit against the CPU definition of tests/test_order_embed_cpu.py, through the
C ABI on a stream of the test's own and through replay.order_embed(use_hip=True).

Every argument is a slice of a wider tensor with 1e30 around it, outputs and the workspace are filled with 1e30 before the
call, and the bytes between the strided rows are checked untouched.  Shapes: (N, k) of (1, 2), (3, 5), (14, 5), (7, 10),
(3, 33), (2, 64) -- the smallest call, less than one tile, 12 bins per tile with a short second tile, six bins and four idle
lanes then one bin, one bin per tile with 31 idle lanes, a bin that is the tile -- at L = 8 with (c1, c2, c3) = (3, 5, 2) and
widths that are no multiples of a block (feat 40, proj_hidden 48, embed 36, ff_hidden 21); L = 32 at the reference's sizes
with (7, 10).  Then the reference's own forward (the golden), the chained order_network_greedy_action, and the order
observation of a real buffered environment."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_order_embed_cpu import (REFERENCE, SMALL, check_golden_bound, golden_case, make_layers, make_obs, network_case, network_forms,
                                  order_embed_replay, same_bits, weights_of)
import test_shape_features_cpu as shp
import test_streams_cpu as stm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 1e30
CASES = [("small", 1, 2), ("small", 3, 5), ("small", 14, 5), ("small", 7, 10), ("small", 3, 33), ("small", 2, 64), ("reference", 7, 10)]


@functools.lru_cache(maxsize=None)
def case(name, N, k):
    """-> W, obs, sf and the definition's result: computed once and shared (treat as read-only)."""
    cfg = {"small": SMALL, "reference": REFERENCE}[name]
    rng = np.random.default_rng(70 + 100 * N + k)
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, N, k, cfg["L"], cfg["feat"])
    return W, obs, sf, order_embed_replay(obs, sf, W)


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


def wide_inputs(obs, sf):
    """obs and sf as slices of poisoned wider device tensors: -> (obs block, its slice, sf block, its slice)."""
    N = obs.shape[0]
    obs_w = torch.full((N, obs.shape[1] + 5), POISON, dtype=torch.float32, device=DEV)
    obs_w[:, 2:2 + obs.shape[1]] = torch.from_numpy(obs).to(DEV)
    sf_w = torch.full((sf.shape[0], sf.shape[1] + 3), POISON, dtype=torch.float32, device=DEV)
    sf_w[:, 1:1 + sf.shape[1]] = torch.from_numpy(sf).to(DEV)
    return obs_w, obs_w[:, 2:2 + obs.shape[1]], sf_w, sf_w[:, 1:1 + sf.shape[1]]


def untouched(t, before):
    return torch.equal(t.view(torch.int32), before.view(torch.int32))          # as bits: a NaN is itself


def abi_call(W, obs, sf, k):
    from irbpp_amd import _lib as L
    lib = L.load()
    N, E = obs.shape[0], W["w_g2"].shape[0]
    w = weights_of(W, DEV)
    obs_w, obs_s, sf_w, sf_s = wide_inputs(obs, sf)
    before = obs_w.clone(), sf_w.clone()
    x_w = torch.full((N, k + 1, E + 4), POISON, dtype=torch.float32, device=DEV)
    xg_w = torch.full((N, E + 5), POISON, dtype=torch.float32, device=DEV)
    base = torch.full((N, w.proj_hidden), POISON, dtype=torch.float32, device=DEV)
    ws = w._struct()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        L.check(lib.irbpp_order_embed(C.byref(ws), _ptr(obs_s), obs_w.stride(0), _ptr(sf_s), sf_w.stride(0), k, N, _ptr(base), _ptr(x_w, 1),
                                      x_w.stride(0), x_w.stride(1), _ptr(xg_w, 2), xg_w.stride(0), C.c_void_p(stream.cuda_stream)),
                "irbpp_order_embed")
    stream.synchronize()
    assert untouched(obs_w, before[0]) and untouched(sf_w, before[1])
    x, xg = x_w[:, :k, 1:1 + E].cpu().numpy(), xg_w[:, 2:2 + E].cpu().numpy()
    x_w[:, :k, 1:1 + E] = POISON
    xg_w[:, 2:2 + E] = POISON
    assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all()) and bool((base != POISON).all())
    return x, xg


def wrapper_call(W, obs, sf, k):
    N, E = obs.shape[0], W["w_g2"].shape[0]
    obs_w, obs_s, sf_w, sf_s = wide_inputs(obs, sf)
    before = obs_w.clone(), sf_w.clone()
    x_w = torch.full((N + 1, k + 2, E + 3), POISON, dtype=torch.float32, device=DEV)
    xg_w = torch.full((N, E + 1), POISON, dtype=torch.float32, device=DEV)
    x, xg = replay.order_embed(obs_s, sf_s, weights_of(W, DEV), use_hip=True, out=x_w[1:, 1:1 + k, :E], out_global=xg_w[:, 1:])
    torch.cuda.synchronize()
    assert x.data_ptr() == x_w[1:, 1:1 + k, :E].data_ptr() and xg.data_ptr() == xg_w[:, 1:].data_ptr()
    assert untouched(obs_w, before[0]) and untouched(sf_w, before[1])
    res = x.cpu().numpy(), xg.cpu().numpy()
    x_w[1:, 1:1 + k, :E] = POISON
    xg_w[:, 1:] = POISON
    assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all())
    return res


@pytest.mark.parametrize("name,N,k", CASES)
def test_kernels_are_the_definition(name, N, k):
    W, obs, sf, (want_x, want_xg) = case(name, N, k)
    x, xg = abi_call(W, obs, sf, k)
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    x, xg = wrapper_call(W, obs, sf, k)
    same_bits(x, want_x)
    same_bits(xg, want_xg)


def test_the_reference_forward_under_the_cpu_bound():
    g, W, k = golden_case()
    x, xg = replay.order_embed(torch.from_numpy(g["obs"]).to(DEV), torch.from_numpy(g["shape_feature"]).to(DEV), weights_of(W, DEV), use_hip=True)
    x, xg = x.cpu().numpy(), xg.cpu().numpy()
    check_golden_bound(x, xg, "the kernels")
    want_x, want_xg = order_embed_replay(g["obs"], g["shape_feature"], W)
    same_bits(x, want_x)
    same_bits(xg, want_xg)


def test_order_network_greedy_action_is_the_cpu_form():
    N, k = 7, 10
    cs = network_case(REFERENCE, N, k)
    act_hip, q_hip = network_forms(cs, k, DEV, True)
    act_cpu, q_cpu = network_forms(cs, k, "cpu", None)
    np.testing.assert_array_equal(act_hip, act_cpu)
    same_bits(q_hip, q_cpu)
    assert ((act_hip >= 0) & (act_hip < k)).all()


def test_on_the_order_observation_of_a_buffered_environment():
    from irbpp_amd import synthetic
    from irbpp_amd.vec_env import GpuPackingEnv
    n, k = 4, 3
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    seqs = synthetic.make_sequences(sh.n_shapes, 64, 150, seed=5)
    env = GpuPackingEnv(sh, seqs, n, device=DEV, bufferSize=k)
    assert env.obs_len == k + 32 * 32
    obs = env.reset()
    slot0 = torch.zeros((n,), dtype=torch.int32, device=DEV)
    for _ in range(4):
        loc = env.get_action_candidates(slot0)
        obs, _, _ = env.step(env.policy_minz(loc))
    env.check_device_error()
    rng = np.random.default_rng(21)
    cfg = dict(L=32, convs=(3, 5, 2), feat=40, proj_hidden=48, embed=36, ff_hidden=21)
    W = make_layers(rng, **cfg)
    points = shp.make_points(rng, sh.n_shapes, 50)
    enc = shp.make_encoder(rng, 20, cfg["feat"])
    indices = rng.integers(0, 50, 65).astype(np.int32)
    layers = stm.make_layers(rng, cfg["embed"], 24, 31)
    support = np.linspace(-1.0, 8.0, 31).astype(np.float32)

    def act_on(state, dev, use_hip):
        q = torch.zeros((n, k), dtype=torch.float32, device=dev)
        a = replay.order_network_greedy_action(state, replay.ShapePoints(points, dev), torch.from_numpy(indices).to(dev), shp.weights_of(enc, dev),
                                               weights_of(W, dev), replay.StreamWeights(*[l.to(dev) for l in layers]),
                                               torch.from_numpy(support).to(dev), q_out=q, use_hip=use_hip)
        return a, q

    host_obs = obs.cpu().clone()
    ids = host_obs[:, :k].numpy()
    assert (ids == np.floor(ids)).all() and (ids >= 0).all() and (ids < sh.n_shapes).all() and (host_obs[:, k:] != 0).any()
    act_hip, q_hip = act_on(obs, DEV, True)
    act_cpu, q_cpu = act_on(host_obs, "cpu", None)
    assert torch.equal(obs.cpu(), host_obs)                  # the observation is read, not written
    np.testing.assert_array_equal(act_hip.cpu().numpy(), act_cpu.numpy())
    same_bits(q_hip.cpu().numpy(), q_cpu.numpy())
    assert np.isfinite(q_cpu.numpy()).all()
    env.get_action_candidates(act_hip.to(torch.int32))
    env.check_device_error()
    env.close()


def test_status_codes_on_the_device():
    from irbpp_amd import _lib as L
    lib = L.load()
    buf = torch.zeros(4096, dtype=torch.float32, device=DEV)
    ptr = C.c_void_p(buf.data_ptr())
    ws = replay._IrbppOrderEmbedWeights(*([ptr.value] * 19), 8, 2, 2, 1, 4, 8, 8, 4, 0.01)
    args = lambda **kw: [kw.get("obs", ptr), kw.get("obs_stride", 67), ptr, 4, kw.get("k_slots", 3), 1, ptr, ptr, 24, kw.get("row_stride", 8), ptr, 8, None]  # noqa: E731
    assert lib.irbpp_order_embed(C.byref(ws), *args(obs_stride=66)) == -1
    assert lib.irbpp_order_embed(C.byref(ws), *args(obs=C.c_void_p(0))) == -1
    assert lib.irbpp_order_embed(C.byref(ws), *args(k_slots=1)) == -1
    assert lib.irbpp_order_embed(C.byref(ws), *args(row_stride=7)) == -1
    assert lib.irbpp_order_embed(C.byref(ws), *args()) == 0
    torch.cuda.synchronize()
    W, obs, sf, (want_x, _) = case("small", 1, 2)            # the device stays usable
    same_bits(abi_call(W, obs, sf, 2)[0], want_x)
