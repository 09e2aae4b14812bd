"""The second form of the order network's row launch (csrc/irbpp_order_embed_mfma.hip, ``form="mfma"``) without a GPU: the
wrapper's argument rules -- an unknown form, widths that are no multiple of 4, the form ignored on CPU tensors,
``order_form=`` handed on by order_network_greedy_action -- and irbpp_order_embed_mfma's refusals through the C ABI, which are
answered before any device call: everything irbpp_order_embed refuses (the BAD list of tests/test_order_embed_cpu.py) with
the same status, and the four widths that are the K of its products.

Also the width sets, (N, k) pairs and inputs that tests/test_order_embed_mfma_kernel_on_host.py and
tests/test_gpu_order_embed_mfma.py share, and the eight linear layers of the definition one by one with the yardstick's own
check: on the shared inputs every layer's chain summed in descending k differs from the definition in at least one valid row,
so a kernel with another order cannot pass.

(N, k): (1, 2) the smallest call, 32 bins' room in a tile and one used; (3, 5) less than one tile; (14, 5) 12 bins per tile and a
short second tile, bin 6 crossing the row-32 boundary between the two row halves; (7, 10) six bins and four idle lanes, then one
bin; (3, 33) one bin per tile with 31 idle lanes; (2, 64) a bin that is the tile.  Widths (feat, proj_hidden, embed,
ff_hidden): every width 4 (one padded feature block of 28 thrown-away rows), (12, 36, 44, 20) (no multiple of 32), the
reference's, every width 256 with k = 64 (the LDS maximum; Q and K in two rounds).  The unaligned case: no width set with
L = 8 has (feat + M) % 4 != 0 (M = 4 c3 there and feat is a multiple of 4), so it takes L = 12 and c3 = 1: feat + M = 21."""
import ctypes as C
import functools
import inspect

import numpy as np
import pytest
import torch

from irbpp_amd import replay
from test_order_embed_cpu import BAD, NAMES, PTR, REFERENCE, SMALL, ids, lib, make_layers, make_obs, order_embed_replay, same_bits, weights_of  # noqa: F401

f32 = np.float32


def widths(base, feat, proj_hidden, embed, ff_hidden, **kw):
    return dict(base, feat=feat, proj_hidden=proj_hidden, embed=embed, ff_hidden=ff_hidden, **kw)


CONFIGS = {"fours": widths(SMALL, 4, 4, 4, 4), "odd32": widths(SMALL, 12, 36, 44, 20), "reference": dict(REFERENCE),
           "widest": widths(SMALL, 256, 256, 256, 256), "odd32u": widths(SMALL, 12, 36, 44, 20, L=12, convs=(3, 5, 1))}
PAIRS = [(1, 2), (3, 5), (14, 5), (7, 10), (3, 33), (2, 64)]
CASES = [(name, N, k) for name in ("fours", "odd32") for N, k in PAIRS] + [("reference", 7, 10), ("widest", 1, 64)]
UNALIGNED = ("odd32u", 3, 5)
# part of every case's seed.  With 0, the ("fours", 2, 64) draw left so few of ff2's four inputs above zero after the relu that
# no element of that layer told an ascending chain from a descending one: the inputs were changed, not the check.
SALT = 1


@functools.lru_cache(maxsize=None)
def case(name, N, k):
    """-> W, obs, sf and the CPU form's result: computed once and shared (treat as read-only)."""
    cfg = CONFIGS[name]
    rng = np.random.default_rng([sorted(CONFIGS).index(name), N, k, SALT])
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, N, k, cfg["L"], cfg["feat"])
    return W, obs, sf, order_embed_replay(obs, sf, W)


def layers_np(W, obs, sf):
    """The eight linear layers of the definition with their inputs, as replay._order_embed_cpu runs them:
    -> [(name, start [N, k, J], weights [J, K], input [N, k, K])], each before its activation and residual."""
    w = weights_of(W)
    N, L, F_, E = obs.shape[0], W["L"], w.feat, w.embed
    k = obs.shape[1] - L * L
    leaky = lambda s: np.where(s > 0, s, f32(W["slope"]) * s).astype(f32)  # noqa: E731
    relu = lambda s: np.where(s > 0, s, f32(0)).astype(f32)  # noqa: E731
    wide = lambda b, J: np.broadcast_to(b, (N, k, J)).astype(f32)  # noqa: E731
    with np.errstate(all="ignore"):
        sf3 = sf.reshape(N, k, F_)
        fmap = replay._height_map_np(obs[:, k:k + L * L].reshape(N, 1, L, L), w, leaky)
        base = replay._chain_np(np.broadcast_to(W["b_g1"], (N, w.proj_hidden)).astype(f32), W["w_g1"][:, F_:], fmap)
        start_g = wide(base[:, None, :], w.proj_hidden)
        g = leaky(replay._chain_np(start_g, W["w_g1"][:, :F_], sf3))
        h0 = replay._lin_np(W["w_g2"], W["b_g2"], g)
        zero = np.zeros((E,), dtype=f32)
        q, key, v = (replay._lin_np(W[n], zero, h0) for n in ("w_q", "w_k", "w_v"))
        c = np.zeros((N, k, k), dtype=f32)
        for d in range(E):
            c = replay._fmaf_np(q[:, :, None, d], key[:, None, :, d], c)
        c = (f32(w.norm) * c).astype(f32)
        e = replay._dexp_np(c - c.max(-1, keepdims=True))
        den = np.zeros((N, k), dtype=f32)
        for j in range(k):
            den = den + e[:, :, j]
        att = (e / den[:, :, None]).astype(f32)
        hd = np.zeros((N, k, E), dtype=f32)
        for j in range(k):
            hd = replay._fmaf_np(att[:, :, j:j + 1], v[:, j:j + 1, :], hd)
        h1 = h0 + replay._lin_np(W["w_o"], W["b_o"], hd)
        ff = relu(replay._lin_np(W["w_f1"], W["b_f1"], h1))
    return [("g", start_g, W["w_g1"][:, :F_], sf3), ("h0", wide(W["b_g2"], E), W["w_g2"], g), ("Q", wide(zero, E), W["w_q"], h0),
            ("K", wide(zero, E), W["w_k"], h0), ("V", wide(zero, E), W["w_v"], h0), ("W_out", wide(W["b_o"], E), W["w_o"], hd),
            ("ff1", wide(W["b_f1"], w.ff_hidden), W["w_f1"], h1), ("ff2", wide(W["b_f2"], E), W["w_f2"], ff)]


def moved_by_descending_order(W, obs, sf):
    """Per layer, the number of output elements (every row of the order network is valid) in which the chain summed with k
    DESCENDING differs from the definition's, and the number of elements."""
    res = {}
    with np.errstate(all="ignore"):
        for name, start, w, x in layers_np(W, obs, sf):
            up = replay._chain_np(start, np.ascontiguousarray(w), x)
            down = replay._chain_np(start, np.ascontiguousarray(w[:, ::-1]), np.ascontiguousarray(x[..., ::-1]))
            res[name] = int((up.view(np.uint32) != down.view(np.uint32)).sum()), up.size
    return res


# ------------------------------------------------------------------ the yardstick ------------
@pytest.mark.parametrize("name,N,k", CASES + [UNALIGNED])
def test_the_inputs_tell_the_order_of_a_chain(name, N, k):
    """Each of the eight layers, summed with k descending over the definition's own input, differs from the definition in at
    least one output element."""
    W, obs, sf, _ = case(name, N, k)
    moved = moved_by_descending_order(W, obs, sf)
    print(", ".join(f"{n}: {m} of {t} elements move" for n, (m, t) in moved.items()))
    assert len(moved) == 8 and all(m > 0 for m, _ in moved.values())


def test_the_layers_are_the_definitions():
    """layers_np restates replay's lines: its last layer and residual give replay.order_embed's x."""
    W, obs, sf, (want_x, _) = case("odd32", 3, 5)
    layers = dict((n, (s, w, x)) for n, s, w, x in layers_np(W, obs, sf))
    with np.errstate(all="ignore"):
        h1 = layers["ff1"][2]
        x = h1 + replay._chain_np(*layers["ff2"])
    same_bits(x, want_x)


# ------------------------------------------------------------------ the wrapper's argument rules ------------
def test_forms_are_named():
    assert replay.ORDER_EMBED_FORMS == ("chain", "mfma") and replay.ORDER_EMBED_HIP_DEFAULT is False


def test_an_unknown_form_is_refused():
    W, obs, sf, _ = case("fours", 1, 2)
    with pytest.raises(ValueError, match="form"):
        replay.order_embed(torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W), form="matrix")
    with pytest.raises(ValueError, match="form"):
        replay.order_embed(torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W), use_hip=False, form="")


@pytest.mark.parametrize("bad", [dict(feat=13), dict(proj_hidden=38), dict(embed=45), dict(ff_hidden=21)], ids=ids)
def test_mfma_with_a_width_that_is_no_multiple_of_four_is_refused(bad):
    rng = np.random.default_rng(3)
    cfg = dict(CONFIGS["odd32"], **bad)
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, 2, 3, cfg["L"], cfg["feat"])
    t_obs, t_sf, w = torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W)
    (name, value), = bad.items()
    with pytest.raises(ValueError, match=f"multiples of 4.*{name} {value}"):
        replay.order_embed(t_obs, t_sf, w, form="mfma")
    x, _ = replay.order_embed(t_obs, t_sf, w, form="chain")  # the chain form takes them
    assert x.shape == (2, 3, cfg["embed"])


def test_the_form_changes_nothing_on_cpu_tensors():
    W, obs, sf, (want_x, want_xg) = case("odd32", 3, 5)
    t_obs, t_sf, w = torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W)
    for use_hip in (None, False):
        x, xg = replay.order_embed(t_obs, t_sf, w, use_hip=use_hip, form="mfma")
        same_bits(x.numpy(), want_x)
        same_bits(xg.numpy(), want_xg)
    with pytest.raises(RuntimeError):
        replay.order_embed(t_obs, t_sf, w, use_hip=True, form="mfma")        # no HIP device holds these tensors


def test_order_network_greedy_action_hands_the_form_on(monkeypatch):
    from test_order_embed_cpu import network_case
    p = inspect.signature(replay.order_network_greedy_action).parameters
    assert p["order_form"].default == "chain" and p["streams_form"].default == "chain"
    assert inspect.signature(replay.order_embed).parameters["form"].default == "chain"
    k = 5
    W, obs, points, enc, indices, layers, support = network_case(SMALL, 2, k)
    import test_shape_features_cpu as shp
    args = (torch.from_numpy(obs), replay.ShapePoints(points, "cpu"), torch.from_numpy(indices), shp.weights_of(enc, "cpu"), weights_of(W),
            replay.StreamWeights(*layers), torch.from_numpy(support))
    seen = []
    real = replay.order_embed
    monkeypatch.setattr(replay, "order_embed", lambda *a, **kw: (seen.append(kw.get("form")), real(*a, **kw))[1])
    want = replay.order_network_greedy_action(*args)
    with pytest.raises(ValueError, match="multiples of 4"):                  # SMALL's ff_hidden is 21
        replay.order_network_greedy_action(*args, order_form="mfma")
    with pytest.raises(ValueError, match="form"):
        replay.order_network_greedy_action(*args, order_form="matrix")
    W4 = make_layers(np.random.default_rng(5), **dict(SMALL, ff_hidden=20))
    args4 = args[:4] + (weights_of(W4),) + args[5:]
    assert torch.equal(replay.order_network_greedy_action(*args4, order_form="mfma"), replay.order_network_greedy_action(*args4))
    assert seen == ["chain", "mfma", "chain"] and want.shape == (2,)


# ------------------------------------------------------------------ limits of the entry point ------------
def abi_call(lib, name="irbpp_order_embed_mfma", **kw):
    """test_order_embed_cpu.abi_call for either entry point: the same defaults (every width a multiple of 4)."""
    d = dict(w=dict(), map_len=8, c1=2, c2=2, c3=1, feat=4, proj_hidden=8, embed=8, ff_hidden=4, slope=0.01, obs=PTR, obs_stride=3 + 64,
             sf=PTR, feat_stride=4, k_slots=3, n_env=1, base=PTR, x=PTR, env_stride=24, row_stride=8, xg=PTR, xg_stride=8, no_struct=False)
    d.update(kw)
    ptrs = {n: PTR.value for n in NAMES}
    ptrs.update(d["w"])
    ws = replay._IrbppOrderEmbedWeights(*(ptrs[n] for n in NAMES), *(d[n] for n in replay._ORDER_SIZES), d["slope"])
    return getattr(lib, name)(None if d["no_struct"] else C.byref(ws), d["obs"], d["obs_stride"], d["sf"], d["feat_stride"], d["k_slots"],
                              d["n_env"], d["base"], d["x"], d["env_stride"], d["row_stride"], d["xg"], d["xg_stride"], None)


@pytest.mark.parametrize("bad", BAD, ids=ids)
def test_irbpp_order_embed_mfma_rejects_what_irbpp_order_embed_rejects(lib, bad):
    assert abi_call(lib, **bad) == -1                       # IRBPP_ERR_ARG before any HIP call


@pytest.mark.parametrize("bad", [dict(feat=6, feat_stride=6), dict(proj_hidden=6), dict(embed=6), dict(ff_hidden=6), dict(feat=1),
                                 dict(ff_hidden=255)], ids=ids)
def test_irbpp_order_embed_mfma_rejects_widths_that_are_no_multiple_of_four(lib, bad):
    assert abi_call(lib, **bad) == -1
