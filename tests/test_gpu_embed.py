"""csrc/irbpp_embed.hip on the GPU, bit for bit against the CPU definition of tests/test_embed_cpu.py, through the C ABI on a
stream of the test's own and through replay.embed(use_hip=True).

Every argument is a slice of a wider tensor with 1e30 around it, outputs and the workspace are filled with 1e30 before the
call, and the bytes between the strided rows are checked untouched.  Shapes: (N, S) of (1, 1), (3, 17), (2, 64), (2, 65),
(2, 130) -- below, at and above one tile of 64 rows, S not a multiple of the mean's 16 parts, the last-row recompute -- at
L = 8 with (c1, c2, c3) = (3, 5, 2) and widths that are no multiples of a block (feat 40, cand_hidden 7, cand_embed 33,
proj_hidden 48, embed 36); L = 32 at the reference's sizes with (3, 65).  make_obs puts in every case an all-valid bin, an
all-invalid bin (N > 1), mask values 0.5 and NaN, an invalid row with a NaN candidate and heightmaps of both signs."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
import test_shape_features_cpu as shp
import test_streams_cpu as stm
from test_embed_cpu import REFERENCE, SMALL, check_golden_bound, embed_cpu, f32, golden_case, make_layers, make_obs, same_bits, weights_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 1e30
CASES = [("small", 1, 1), ("small", 3, 17), ("small", 2, 64), ("small", 2, 65), ("small", 2, 130), ("reference", 3, 65)]


@functools.lru_cache(maxsize=None)
def case(name, N, S):
    """-> W, obs, sf and the definition's result: computed once and shared (treat as read-only)."""
    cfg = {"small": SMALL, "reference": REFERENCE}[name]
    rng = np.random.default_rng(70 + 100 * N + S)
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, N, S, cfg["L"], cfg["feat"])
    return W, obs, sf, embed_cpu(obs, sf, W)


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


def wide_inputs(obs, sf):
    """obs and sf as slices of poisoned wider device tensors: -> (obs block, its slice, sf block, its slice)."""
    N = obs.shape[0]
    obs_w = torch.full((N, obs.shape[1] + 5), POISON, dtype=torch.float32, device=DEV)
    obs_w[:, 2:2 + obs.shape[1]] = torch.from_numpy(obs).to(DEV)
    sf_w = torch.full((N, sf.shape[1] + 3), POISON, dtype=torch.float32, device=DEV)
    sf_w[:, 1:1 + sf.shape[1]] = torch.from_numpy(sf).to(DEV)
    return obs_w, obs_w[:, 2:2 + obs.shape[1]], sf_w, sf_w[:, 1:1 + sf.shape[1]]


def untouched(t, before):
    return torch.equal(t.view(torch.int32), before.view(torch.int32))          # as bits: a NaN is itself


def abi_call(W, obs, sf, S):
    from irbpp_amd import _lib as L
    lib = L.load()
    N, E = obs.shape[0], W["w_p2"].shape[0]
    w = weights_of(W, DEV)
    obs_w, obs_s, sf_w, sf_s = wide_inputs(obs, sf)
    before = obs_w.clone(), sf_w.clone()
    x_w = torch.full((N, S + 1, E + 4), POISON, dtype=torch.float32, device=DEV)
    xg_w = torch.full((N, E + 5), POISON, dtype=torch.float32, device=DEV)
    base = torch.full((N, w.proj_hidden), POISON, dtype=torch.float32, device=DEV)
    ws = w._struct()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        L.check(lib.irbpp_embed(C.byref(ws), _ptr(obs_s), obs_w.stride(0), _ptr(sf_s), sf_w.stride(0), S, N, _ptr(base), _ptr(x_w, 1),
                                x_w.stride(0), x_w.stride(1), _ptr(xg_w, 2), xg_w.stride(0), C.c_void_p(stream.cuda_stream)), "irbpp_embed")
    stream.synchronize()
    assert untouched(obs_w, before[0]) and untouched(sf_w, before[1])
    x, xg = x_w[:, :S, 1:1 + E].cpu().numpy(), xg_w[:, 2:2 + E].cpu().numpy()
    x_w[:, :S, 1:1 + E] = POISON
    xg_w[:, 2:2 + E] = POISON
    assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all()) and bool((base != POISON).all())
    return x, xg


def wrapper_call(W, obs, sf, S):
    N, E = obs.shape[0], W["w_p2"].shape[0]
    obs_w, obs_s, sf_w, sf_s = wide_inputs(obs, sf)
    before = obs_w.clone(), sf_w.clone()
    x_w = torch.full((N + 1, S + 2, E + 3), POISON, dtype=torch.float32, device=DEV)
    xg_w = torch.full((N, E + 1), POISON, dtype=torch.float32, device=DEV)
    x, xg = replay.embed(obs_s, sf_s, weights_of(W, DEV), use_hip=True, out=x_w[1:, 1:1 + S, :E], out_global=xg_w[:, 1:])
    torch.cuda.synchronize()
    assert x.data_ptr() == x_w[1:, 1:1 + S, :E].data_ptr() and xg.data_ptr() == xg_w[:, 1:].data_ptr()
    assert untouched(obs_w, before[0]) and untouched(sf_w, before[1])
    res = x.cpu().numpy(), xg.cpu().numpy()
    x_w[1:, 1:1 + S, :E] = POISON
    xg_w[:, 1:] = POISON
    assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all())
    return res


@pytest.mark.parametrize("name,N,S", CASES)
def test_kernels_are_the_definition(name, N, S):
    W, obs, sf, (want_x, want_xg) = case(name, N, S)
    x, xg = abi_call(W, obs, sf, S)
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    x, xg = wrapper_call(W, obs, sf, S)
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    if N > 1:
        assert (want_x[N - 1] == 0).all() and (want_x[0, 0] != 0).any()      # the all-invalid and the all-valid bin


def test_the_reference_forward_under_the_cpu_bound():
    g, W, S = golden_case()
    x, xg = replay.embed(torch.from_numpy(g["obs"]).to(DEV), torch.from_numpy(g["shape_feature"]).to(DEV), weights_of(W, DEV), use_hip=True)
    x, xg = x.cpu().numpy(), xg.cpu().numpy()
    check_golden_bound(x, xg, "the kernels")
    want_x, want_xg = embed_cpu(g["obs"], g["shape_feature"], W)
    same_bits(x, want_x)
    same_bits(xg, want_xg)


def test_torch_form_is_close_to_the_definition():
    """The fallback on a HIP device without the kernels: the same factored expression in the libraries' summation orders,
    under the golden's bound."""
    g, W, S = golden_case()
    x, xg = replay.embed(torch.from_numpy(g["obs"]).to(DEV), torch.from_numpy(g["shape_feature"]).to(DEV), weights_of(W, DEV), use_hip=False)
    check_golden_bound(x.cpu().numpy(), xg.cpu().numpy(), "torch's layers, factored")


def network_case():
    """A block with exact 0 / 1 masks and planted rows (a candidate far from the others') in which the best valid row of every
    bin leads the runner-up by more than 1e-3 in q (asserted by the test on the CPU form): far beyond what separates two
    float32 evaluations of the head."""
    rng = np.random.default_rng(11)
    N, S, atoms, n_shapes, P, k = 3, 17, 31, 5, 50, 65
    W = make_layers(rng, **SMALL)
    obs, _ = make_obs(rng, N, S, SMALL["L"], SMALL["feat"])
    rows = obs[:, :5 * S].reshape(N, S, 5)
    rows[:, :, :4] = rng.uniform(-1.0, 1.0, (N, S, 4))
    rows[:, :, 4] = (rng.random((N, S)) < 0.6).astype(f32)
    for n, r in enumerate([4, 9, 16]):
        rows[n, r, :4] = 6.0
        rows[n, r, 4] = 1.0
    points = shp.make_points(rng, n_shapes, P)
    enc = shp.make_encoder(rng, 20, SMALL["feat"])
    indices = rng.integers(0, P, k).astype(np.int32)
    layers = stm.make_layers(rng, SMALL["embed"], 24, atoms)
    return W, obs, points, enc, indices, layers, np.linspace(-1.0, 8.0, atoms).astype(f32)


def test_network_greedy_action_is_the_three_stages():
    W, obs, points, enc, indices, layers, support = network_case()
    S = 17

    def forms(dev, use_hip):
        sp, sw, ew = replay.ShapePoints(points, dev), shp.weights_of(enc, dev), weights_of(W, dev)
        tw = replay.StreamWeights(*[l.to(dev) for l in layers])
        state, idx, z = torch.from_numpy(obs).to(dev), torch.from_numpy(indices).to(dev), torch.from_numpy(support).to(dev)
        q = torch.zeros((obs.shape[0], S), dtype=torch.float32, device=dev)
        act = replay.network_greedy_action(state, sp, idx, sw, ew, tw, z, q_out=q, use_hip=use_hip)
        sf = replay.shape_features(state[:, 5 * S], sp, idx, sw, use_hip=use_hip)
        x, xg = replay.embed(state, sf, ew, use_hip=use_hip)
        q2 = torch.zeros_like(q)
        act2 = replay.streams_greedy_action(x, xg, tw, z, state, q_out=q2, use_hip=use_hip)
        assert torch.equal(act, act2) and torch.equal(q.view(torch.int32), q2.view(torch.int32))
        return act.cpu().numpy(), q.cpu().numpy()

    act_hip, q_hip = forms(DEV, True)
    act_cpu, q_cpu = forms("cpu", None)
    np.testing.assert_array_equal(act_hip, act_cpu)
    valid = obs[:, :5 * S].reshape(-1, S, 5)[:, :, 4] != 0
    masked = np.where(valid, q_cpu, -np.inf)
    top2 = np.sort(masked, axis=1)[:, -2:]
    print("lead of the chosen row over the runner-up per bin:", top2[:, 1] - top2[:, 0], "max |q_hip - q_cpu|", np.abs(q_hip - q_cpu).max())
    assert (act_cpu == masked.argmax(1)).all() and (top2[:, 1] - top2[:, 0] > 1e-3).all()


def test_status_codes_on_the_device():
    from irbpp_amd import _lib as L
    lib = L.load()
    buf = torch.zeros(4096, dtype=torch.float32, device=DEV)
    ptr = C.c_void_p(buf.data_ptr())
    ws = replay._IrbppEmbedWeights(*([ptr.value] * 14), 8, 2, 2, 1, 4, 4, 4, 8, 8, 0.01)
    args = lambda **kw: [kw.get("obs", ptr), kw.get("obs_stride", 88), ptr, 4, kw.get("s_rows", 3), 1, ptr, ptr, 24, kw.get("row_stride", 8), ptr, 8, None]  # noqa: E731
    assert lib.irbpp_embed(C.byref(ws), *args(obs_stride=87)) == -1
    assert lib.irbpp_embed(C.byref(ws), *args(obs=C.c_void_p(0))) == -1
    assert lib.irbpp_embed(C.byref(ws), *args(s_rows=1025)) == -1
    assert lib.irbpp_embed(C.byref(ws), *args(row_stride=7)) == -1
    assert lib.irbpp_embed(C.byref(ws), *args()) == 0
    torch.cuda.synchronize()
    W, obs, sf, (want_x, _) = case("small", 1, 1)            # the device stays usable
    same_bits(abi_call(W, obs, sf, 1)[0], want_x)
