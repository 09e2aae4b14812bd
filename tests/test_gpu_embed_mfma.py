"""csrc/irbpp_embed_mfma.hip on the GPU: irbpp_embed_mfma gives, bit for bit, what replay.embed on CPU tensors (the
definition, tests/test_embed_cpu.py) and irbpp_embed give on the same inputs, through the C ABI on a stream of the test's own
and through replay.embed(use_hip=True, form="mfma").  The hardware side of csrc/irbpp_mfma_chain.h's claim for its second
user: the float32 matrix instruction as a k-ordered fmaf chain started from the bias (e2, x) or from `base` (h).

Configurations, (N, S) and inputs are those of tests/test_embed_mfma_cpu.py, on which
tests/test_embed_mfma_kernel_on_host.py checks that each of the three layers summed in descending k differs from the
definition in a valid row.  Every argument is a slice of a wider tensor with 1e30 around it, outputs and the workspace are
filled with 1e30 before the call, and the bytes between the strided rows are checked untouched.  x starts one float into its
block, so its rows are never 16-byte aligned; the unaligned case adds weight rows that are not (feat + M = 49, every weight
array one float past a boundary: the element loads)."""
import ctypes as C

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
import test_gpu_embed as G
import test_shape_features_cpu as shp
from test_embed_cpu import same_bits, weights_of
from test_embed_mfma_cpu import CASES, CONFIGS, UNALIGNED, case

pytestmark = pytest.mark.gpu
DEV = G.DEV
POISON = G.POISON


def off_by_one_float(w):
    """The EmbedWeights' tensors moved to one float past a 16-byte boundary (torch's allocations are aligned)."""
    for n in replay._EMBED_FIELDS:
        t = getattr(w, n)
        buf = torch.zeros(t.numel() + 1, dtype=torch.float32, device=t.device)
        buf[1:] = t.reshape(-1)
        setattr(w, n, buf[1:].view(t.shape))
        assert getattr(w, n).data_ptr() % 16 == 4
    return w


def abi_call(name, W, obs, sf, S, unaligned=False, expect=0):
    """One call of the entry point `name` (irbpp_embed or irbpp_embed_mfma) on a stream of its own -> x, xg."""
    from irbpp_amd import _lib as L
    lib = L.load()
    N, E = obs.shape[0], W["w_p2"].shape[0]
    w = weights_of(W, DEV)
    if unaligned:
        w = off_by_one_float(w)
    obs_w, obs_s, sf_w, sf_s = G.wide_inputs(obs, sf)
    before = obs_w.clone(), sf_w.clone()
    x_w = torch.full((N, S + 1, E + 4), POISON, dtype=torch.float32, device=DEV)
    xg_w = torch.full((N, E + 5), POISON, dtype=torch.float32, device=DEV)
    base = torch.full((N, w.proj_hidden), POISON, dtype=torch.float32, device=DEV)
    ws = w._struct()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        rc = getattr(lib, name)(C.byref(ws), G._ptr(obs_s), obs_w.stride(0), G._ptr(sf_s), sf_w.stride(0), S, N, G._ptr(base), G._ptr(x_w, 1),
                                x_w.stride(0), x_w.stride(1), G._ptr(xg_w, 2), xg_w.stride(0), C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    assert rc == expect
    assert G.untouched(obs_w, before[0]) and G.untouched(sf_w, before[1])
    if rc != 0:
        assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all()) and bool((base == POISON).all())
        return None
    x, xg = x_w[:, :S, 1:1 + E].cpu().numpy(), xg_w[:, 2:2 + E].cpu().numpy()
    x_w[:, :S, 1:1 + E] = POISON
    xg_w[:, 2:2 + E] = POISON
    assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all()) and bool((base != POISON).all())
    return x, xg


def wrapper_call(W, obs, sf, S, form):
    N, E = obs.shape[0], W["w_p2"].shape[0]
    obs_w, obs_s, sf_w, sf_s = G.wide_inputs(obs, sf)
    before = obs_w.clone(), sf_w.clone()
    x_w = torch.full((N + 1, S + 2, E + 3), POISON, dtype=torch.float32, device=DEV)
    xg_w = torch.full((N, E + 1), POISON, dtype=torch.float32, device=DEV)
    x, xg = replay.embed(obs_s, sf_s, weights_of(W, DEV), use_hip=True, out=x_w[1:, 1:1 + S, :E], out_global=xg_w[:, 1:], form=form)
    torch.cuda.synchronize()
    assert x.data_ptr() == x_w[1:, 1:1 + S, :E].data_ptr() and xg.data_ptr() == xg_w[:, 1:].data_ptr()
    assert G.untouched(obs_w, before[0]) and G.untouched(sf_w, before[1])
    res = x.cpu().numpy(), xg.cpu().numpy()
    x_w[1:, 1:1 + S, :E] = POISON
    xg_w[:, 1:] = POISON
    assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all())
    return res


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("name,N,S", CASES)
def test_the_bits_are_the_chains(name, N, S):
    W, obs, sf, (want_x, want_xg) = case(name, N, S)
    x, xg = abi_call("irbpp_embed_mfma", W, obs, sf, S)
    print(f"elements that differ from the definition: x {differing(x, want_x)} of {x.size}, xg {differing(xg, want_xg)} of {xg.size}")
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    c_x, c_xg = abi_call("irbpp_embed", W, obs, sf, S)
    same_bits(x, c_x)
    same_bits(xg, c_xg)
    w_x, w_xg = wrapper_call(W, obs, sf, S, "mfma")
    same_bits(w_x, want_x)
    same_bits(w_xg, want_xg)
    if N > 1:
        assert (want_x[N - 1] == 0).all() and (want_x[0, 0] != 0).any()      # the all-invalid and the all-valid bin


def test_rows_that_are_not_aligned():
    name, N, S = UNALIGNED
    W, obs, sf, (want_x, want_xg) = case(name, N, S)
    x, xg = abi_call("irbpp_embed_mfma", W, obs, sf, S, unaligned=True)
    print(f"elements that differ from the definition: x {differing(x, want_x)} of {x.size}, xg {differing(xg, want_xg)} of {xg.size}")
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    c_x, c_xg = abi_call("irbpp_embed", W, obs, sf, S, unaligned=True)
    same_bits(x, c_x)
    same_bits(xg, c_xg)


@pytest.mark.parametrize("name,N,S,n", [("blocks", 3, 17, 1), ("small4", 2, 130, 0)])
def test_a_bin_alone_equals_itself_in_the_batch(name, N, S, n):
    W, obs, sf, (want_x, want_xg) = case(name, N, S)
    x, xg = abi_call("irbpp_embed_mfma", W, obs[n:n + 1], sf[n:n + 1], S)
    same_bits(x[0], want_x[n])
    same_bits(xg[0], want_xg[n])


def test_network_greedy_action_takes_the_forms():
    """The whole acting forward with both stages on the matrix cores: the CPU form's action, the all-chain call's q_out bit
    for bit.  test_gpu_embed.network_case with widths that are multiples of 4 (the best row of every bin leads by > 1e-3 on
    the CPU form, asserted here)."""
    import test_streams_cpu as stm
    from test_embed_cpu import make_layers, make_obs
    rng = np.random.default_rng(12)
    cfg = dict(CONFIGS["small4"], embed=36)                  # the streams' mfma form needs embed % 4 == 0
    N, S, atoms, n_shapes, P, k = 3, 17, 31, 5, 50, 65
    W = make_layers(rng, **cfg)
    obs, _ = make_obs(rng, N, S, cfg["L"], cfg["feat"])
    rows = obs[:, :5 * S].reshape(N, S, 5)
    rows[:, :, :4] = rng.uniform(-1.0, 1.0, (N, S, 4))
    rows[:, :, 4] = (rng.random((N, S)) < 0.6).astype(np.float32)
    for n, r in enumerate([4, 9, 16]):
        rows[n, r, :4] = 6.0
        rows[n, r, 4] = 1.0
    points = shp.make_points(rng, n_shapes, P)
    enc = shp.make_encoder(rng, 20, cfg["feat"])
    indices = rng.integers(0, P, k).astype(np.int32)
    layers = stm.make_layers(rng, cfg["embed"], 24, atoms)
    support = np.linspace(-1.0, 8.0, atoms).astype(np.float32)

    def act(dev, use_hip, **forms):
        sp, sw, ew = replay.ShapePoints(points, dev), shp.weights_of(enc, dev), weights_of(W, dev)
        tw = replay.StreamWeights(*[l.to(dev) for l in layers])
        state, idx, z = torch.from_numpy(obs).to(dev), torch.from_numpy(indices).to(dev), torch.from_numpy(support).to(dev)
        q = torch.zeros((N, S), dtype=torch.float32, device=dev)
        a = replay.network_greedy_action(state, sp, idx, sw, ew, tw, z, q_out=q, use_hip=use_hip, **forms)
        return a.cpu().numpy(), q.cpu().numpy()

    act_mfma, q_mfma = act(DEV, True, embed_form="mfma", streams_form="mfma")
    act_chain, q_chain = act(DEV, True)
    act_cpu, q_cpu = act("cpu", None, embed_form="mfma")
    np.testing.assert_array_equal(act_mfma, act_cpu)
    np.testing.assert_array_equal(act_mfma, act_chain)
    same_bits(q_mfma, q_chain)
    valid = rows[:, :, 4] != 0
    top2 = np.sort(np.where(valid, q_cpu, -np.inf), axis=1)[:, -2:]
    print("lead of the chosen row over the runner-up per bin:", top2[:, 1] - top2[:, 0], "q elements that differ from the CPU form's:",
          differing(q_mfma, q_cpu))
    assert (top2[:, 1] - top2[:, 0] > 1e-3).all()


@pytest.mark.parametrize("bad", [dict(cand_hidden=7), dict(cand_embed=34), dict(proj_hidden=45)], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_widths_that_are_no_multiple_of_four_are_refused(bad):
    from test_embed_cpu import embed_cpu, make_layers, make_obs
    rng = np.random.default_rng(13)
    cfg = dict(CONFIGS["small4"], **bad)
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, 2, 5, cfg["L"], cfg["feat"])
    assert abi_call("irbpp_embed_mfma", W, obs, sf, 5, expect=-1) is None     # IRBPP_ERR_ARG through the ABI, nothing written
    x, xg = abi_call("irbpp_embed", W, obs, sf, 5)                          # the chain form takes them
    want_x, want_xg = embed_cpu(obs, sf, W)
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    with pytest.raises(ValueError, match="multiples of 4"):
        replay.embed(torch.from_numpy(obs).to(DEV), torch.from_numpy(sf).to(DEV), weights_of(W, DEV), use_hip=True, form="mfma")
    with pytest.raises(ValueError, match="form"):
        replay.embed(torch.from_numpy(obs).to(DEV), torch.from_numpy(sf).to(DEV), weights_of(W, DEV), use_hip=True, form="matrix")
