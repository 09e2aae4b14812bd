"""csrc/irbpp_order_embed_mfma.hip on the GPU: irbpp_order_embed_mfma gives, bit for bit, what replay.order_embed on CPU
tensors (the definition, tests/test_order_embed_cpu.py) and irbpp_order_embed give on the same inputs, through the C ABI on a
stream of the test's own and through replay.order_embed(use_hip=True, form="mfma").  The hardware side of
csrc/irbpp_mfma_chain.h's claim for its third user: the float32 matrix instruction as a k-ordered fmaf chain started from a
`base` of its own per column (g), from a bias (h0, W_out, ff1, ff2) and from +0.0 (Q, K, V); the two earlier users started
theirs from a bias or from one `base` per workgroup.

Width sets, (N, k) and inputs are those of tests/test_order_embed_mfma_cpu.py, which checks that each of the eight layers
summed in descending k differs from the definition.  Every argument is a slice of a wider tensor with 1e30 around it, outputs
and the workspace are filled with 1e30 before the call, and the bytes between the strided rows are checked untouched.  x
starts one float into its block, so its rows are never 16-byte aligned; the unaligned case adds weight rows that are not
(feat + M = 21, every weight array one float past a boundary: the element loads)."""
import ctypes as C

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
import test_gpu_order_embed as G
from test_order_embed_cpu import make_layers, make_obs, network_case, order_embed_replay, same_bits, weights_of
from test_order_embed_mfma_cpu import CASES, CONFIGS, UNALIGNED, case

pytestmark = pytest.mark.gpu
DEV = G.DEV
POISON = G.POISON


def off_by_one_float(w):
    """The OrderEmbedWeights' tensors moved to one float past a 16-byte boundary (torch's allocations are aligned)."""
    for n in replay._ORDER_FIELDS:
        t = getattr(w, n)
        buf = torch.zeros(t.numel() + 1, dtype=torch.float32, device=t.device)
        buf[1:] = t.reshape(-1)
        setattr(w, n, buf[1:].view(t.shape))
        assert getattr(w, n).data_ptr() % 16 == 4
    return w


def abi_call(name, W, obs, sf, k, unaligned=False, expect=0):
    """One call of the entry point `name` (irbpp_order_embed or irbpp_order_embed_mfma) on a stream of its own -> x, xg."""
    from irbpp_amd import _lib as L
    lib = L.load()
    N, E = obs.shape[0], W["w_g2"].shape[0]
    w = weights_of(W, DEV)
    if unaligned:
        w = off_by_one_float(w)
    obs_w, obs_s, sf_w, sf_s = G.wide_inputs(obs, sf)
    before = obs_w.clone(), sf_w.clone()
    x_w = torch.full((N, k + 1, E + 4), POISON, dtype=torch.float32, device=DEV)
    xg_w = torch.full((N, E + 5), POISON, dtype=torch.float32, device=DEV)
    base = torch.full((N, w.proj_hidden), POISON, dtype=torch.float32, device=DEV)
    ws = w._struct()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        rc = getattr(lib, name)(C.byref(ws), G._ptr(obs_s), obs_w.stride(0), G._ptr(sf_s), sf_w.stride(0), k, N, G._ptr(base), G._ptr(x_w, 1),
                                x_w.stride(0), x_w.stride(1), G._ptr(xg_w, 2), xg_w.stride(0), C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    assert rc == expect
    assert G.untouched(obs_w, before[0]) and G.untouched(sf_w, before[1])
    if rc != 0:
        assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all()) and bool((base == POISON).all())
        return None
    x, xg = x_w[:, :k, 1:1 + E].cpu().numpy(), xg_w[:, 2:2 + E].cpu().numpy()
    x_w[:, :k, 1:1 + E] = POISON
    xg_w[:, 2:2 + E] = POISON
    assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all()) and bool((base != POISON).all())
    return x, xg


def wrapper_call(W, obs, sf, k, form):
    N, E = obs.shape[0], W["w_g2"].shape[0]
    obs_w, obs_s, sf_w, sf_s = G.wide_inputs(obs, sf)
    before = obs_w.clone(), sf_w.clone()
    x_w = torch.full((N + 1, k + 2, E + 3), POISON, dtype=torch.float32, device=DEV)
    xg_w = torch.full((N, E + 1), POISON, dtype=torch.float32, device=DEV)
    x, xg = replay.order_embed(obs_s, sf_s, weights_of(W, DEV), use_hip=True, out=x_w[1:, 1:1 + k, :E], out_global=xg_w[:, 1:], form=form)
    torch.cuda.synchronize()
    assert x.data_ptr() == x_w[1:, 1:1 + k, :E].data_ptr() and xg.data_ptr() == xg_w[:, 1:].data_ptr()
    assert G.untouched(obs_w, before[0]) and G.untouched(sf_w, before[1])
    res = x.cpu().numpy(), xg.cpu().numpy()
    x_w[1:, 1:1 + k, :E] = POISON
    xg_w[:, 1:] = POISON
    assert bool((x_w == POISON).all()) and bool((xg_w == POISON).all())
    return res


def differing(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("name,N,k", CASES)
def test_the_bits_are_the_chains(name, N, k):
    W, obs, sf, (want_x, want_xg) = case(name, N, k)
    x, xg = abi_call("irbpp_order_embed_mfma", W, obs, sf, k)
    print(f"elements that differ from the definition: x {differing(x, want_x)} of {x.size}, xg {differing(xg, want_xg)} of {xg.size}")
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    c_x, c_xg = abi_call("irbpp_order_embed", W, obs, sf, k)
    same_bits(x, c_x)
    same_bits(xg, c_xg)
    w_x, w_xg = wrapper_call(W, obs, sf, k, "mfma")
    same_bits(w_x, want_x)
    same_bits(w_xg, want_xg)


def test_rows_that_are_not_aligned():
    name, N, k = UNALIGNED
    W, obs, sf, (want_x, want_xg) = case(name, N, k)
    assert W["w_g1"].shape[1] % 4 != 0
    x, xg = abi_call("irbpp_order_embed_mfma", W, obs, sf, k, unaligned=True)
    print(f"elements that differ from the definition: x {differing(x, want_x)} of {x.size}, xg {differing(xg, want_xg)} of {xg.size}")
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    c_x, c_xg = abi_call("irbpp_order_embed", W, obs, sf, k, unaligned=True)
    same_bits(x, c_x)
    same_bits(xg, c_xg)


def test_a_bin_alone_equals_itself_in_the_batch():
    """Bin 6 of fourteen: rows 30 .. 34 of its tile, across the two row halves."""
    W, obs, sf, (want_x, want_xg) = case("odd32", 14, 5)
    x, xg = abi_call("irbpp_order_embed_mfma", W, obs[6:7], sf[30:35], 5)
    same_bits(x[0], want_x[6])
    same_bits(xg[0], want_xg[6])


def test_order_network_greedy_action_takes_the_forms():
    """The whole acting forward of the order network with both stages on the matrix cores: the CPU form's action, the
    all-chain call's q_out bit for bit."""
    N, k = 7, 10
    W, obs, points, enc, indices, layers, support = network_case(CONFIGS["odd32"], N, k)
    import test_shape_features_cpu as shp

    def act(dev, use_hip, **forms):
        sp, sw, ow = replay.ShapePoints(points, dev), shp.weights_of(enc, dev), weights_of(W, dev)
        tw = replay.StreamWeights(*[l.to(dev) for l in layers])
        state, idx, z = torch.from_numpy(obs).to(dev), torch.from_numpy(indices).to(dev), torch.from_numpy(support).to(dev)
        q = torch.zeros((N, k), dtype=torch.float32, device=dev)
        a = replay.order_network_greedy_action(state, sp, idx, sw, ow, tw, z, q_out=q, use_hip=use_hip, **forms)
        return a.cpu().numpy(), q.cpu().numpy()

    act_mfma, q_mfma = act(DEV, True, order_form="mfma", streams_form="mfma")
    act_chain, q_chain = act(DEV, True)
    act_cpu, q_cpu = act("cpu", None, order_form="mfma")
    print("q elements that differ from the CPU form's:", differing(q_mfma, q_cpu))
    np.testing.assert_array_equal(act_mfma, act_cpu)
    np.testing.assert_array_equal(act_mfma, act_chain)
    same_bits(q_mfma, q_chain)
    same_bits(q_mfma, q_cpu)


@pytest.mark.parametrize("bad", [dict(feat=13), dict(proj_hidden=38), dict(embed=45), dict(ff_hidden=21)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_widths_that_are_no_multiple_of_four_are_refused(bad):
    rng = np.random.default_rng(13)
    cfg = dict(CONFIGS["odd32"], **bad)
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, 2, 5, cfg["L"], cfg["feat"])
    assert abi_call("irbpp_order_embed_mfma", W, obs, sf, 5, expect=-1) is None     # IRBPP_ERR_ARG through the ABI, nothing written
    x, xg = abi_call("irbpp_order_embed", W, obs, sf, 5)                          # the chain entry takes the same arguments
    want_x, want_xg = order_embed_replay(obs, sf, W)
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    with pytest.raises(ValueError, match="multiples of 4"):
        replay.order_embed(torch.from_numpy(obs).to(DEV), torch.from_numpy(sf).to(DEV), weights_of(W, DEV), use_hip=True, form="mfma")
    with pytest.raises(ValueError, match="form"):
        replay.order_embed(torch.from_numpy(obs).to(DEV), torch.from_numpy(sf).to(DEV), weights_of(W, DEV), use_hip=True, form="matrix")
