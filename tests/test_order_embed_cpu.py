"""The order network's embedding stage (csrc/irbpp_order_embed.hip) without a GPU: the definition restated here bin by bin
in numpy (``order_embed_cpu``: the convolutions tap by tap, gat_project_layer[0] as one chain from the bias over the map
feature FIRST and the slot's shape feature after it, Q / K / V, the compatibilities, the softmax with dueling_dexp, the two
residuals, the mean as dueling_mean's 16 parts) against replay.order_embed on CPU tensors, bit for bit.  Then the reference's
own forward (tests/golden/order_embed_ref.npz, written by tests/golden/make_order_embed_golden.py): the definition is as
close to the float64 evaluation of the reference's lines as the reference's float32 evaluation is.

Measured on the golden (max over all elements, against float64): the definition 4.27e-07 (embeddings) / 3.86e-07
(graph_embed), the reference's float32 forward 3.98e-07 / 3.35e-07."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from irbpp_amd import replay
import test_shape_features_cpu as shp
import test_streams_cpu as stm
from test_dueling_cpu import dexp_np, dueling_act_np
from test_embed_cpu import conv_def, fmaf, leaky, same_bits

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "order_embed_ref.npz")
# L, (c1, c2, c3), feat, proj_hidden, embed, ff_hidden
SMALL = dict(L=8, convs=(3, 5, 2), feat=40, proj_hidden=48, embed=36, ff_hidden=21)
REFERENCE = dict(L=32, convs=(16, 32, 4), feat=128, proj_hidden=256, embed=128, ff_hidden=128)
NAMES = replay._ORDER_FIELDS
BIASED = ("conv1", "conv2", "conv3", "g1", "g2", "o", "f1", "f2")     # the layers with a bias; q, k, v have none


def make_layers(rng, L, convs, feat, proj_hidden, embed, ff_hidden, slope=0.01):
    """-> dict of float32 arrays in torch's layouts under the names of irbpp_order_embed_weights, 'slope' and 'L'."""
    c1, c2, c3 = convs
    M, E = c3 * (L // 4) ** 2, embed
    shapes = dict(conv1=(c1, 1, 4, 4), conv2=(c2, c1, 4, 4), conv3=(c3, c2, 3, 3), g1=(proj_hidden, feat + M), g2=(E, proj_hidden),
                  q=(E, E), k=(E, E), v=(E, E), o=(E, E), f1=(ff_hidden, E), f2=(E, ff_hidden))
    W = {"slope": slope, "L": L}
    for name, shape in shapes.items():
        fan_in = int(np.prod(shape[1:]))
        W["w_" + name] = (rng.standard_normal(shape) / np.sqrt(fan_in)).astype(f32)
        if name in BIASED:
            W["b_" + name] = rng.uniform(-0.3, 0.3, shape[0]).astype(f32)
    assert set(W) == set(NAMES) | {"slope", "L"}
    return W


def layers_of(W, device="cpu", n_heads=1):
    """(height_encoder, gat_project_layer, embedder) as plain objects with the reference's attribute names."""
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    lin = lambda n: types.SimpleNamespace(weight=t(W["w_" + n]), bias=t(W["b_" + n]) if "b_" + n in W else None)  # noqa: E731
    att = types.SimpleNamespace(n_heads=n_heads, W_query=lin("q"), W_key=lin("k"), W_val=lin("v"), W_out=lin("o"))
    layer = [types.SimpleNamespace(module=att), types.SimpleNamespace(module=[lin("f1"), object(), lin("f2")])]
    embedder = types.SimpleNamespace(init_embed=None, layers=[layer])
    return [lin("conv1"), lin("conv2"), lin("conv3")], [lin("g1"), object(), lin("g2")], embedder


def weights_of(W, device="cpu"):
    return replay.OrderEmbedWeights(*layers_of(W, device), W["slope"], map_len=W["L"])


def make_obs(rng, N, k, L, feat):
    """An order observation block [N, k + L^2] (k item ids, heightmaps of both signs) and a shape feature [N k, feat]."""
    obs = rng.uniform(-1.0, 1.0, (N, k + L * L)).astype(f32)
    obs[:, :k] = rng.integers(0, 5, (N, k))
    return obs, rng.uniform(-0.5, 1.0, (N * k, feat)).astype(f32)


def chain_def(acc, w, x):
    """acc [R, J] continued over x [R, K] against w [J, K], c ascending."""
    for c in range(w.shape[1]):
        acc = fmaf(x[:, c:c + 1], w[None, :, c], acc)
    return acc


def lin_def(w, b, x):
    start = np.zeros((w.shape[0],), dtype=f32) if b is None else b
    return chain_def(np.broadcast_to(start, (x.shape[0], w.shape[0])).astype(f32), w, x)


def order_embed_cpu(obs, sf, W, k):
    """The definition: obs [N, k + L^2], sf [N k, F] -> x [N, k, E], xg [N, E]."""
    N, L, slope = obs.shape[0], W["L"], W["slope"]
    E, F_ = W["w_g2"].shape[0], sf.shape[1]
    nf = f32(1.0 / np.sqrt(np.float64(E)))
    x = np.zeros((N, k, E), dtype=f32)
    xg = np.zeros((N, E), dtype=f32)
    relu = lambda s: np.where(s > 0, s, f32(0)).astype(f32)  # noqa: E731
    with np.errstate(all="ignore"):
        for n in range(N):
            hm = obs[n, k:k + L * L].reshape(1, L, L)
            fmap = conv_def(conv_def(conv_def(hm, W["w_conv1"], W["b_conv1"], 2, slope), W["w_conv2"], W["b_conv2"], 2, slope),
                            W["w_conv3"], W["b_conv3"], 1, slope).reshape(1, -1)
            base = chain_def(W["b_g1"][None].astype(f32), W["w_g1"][:, F_:], fmap)                # once per bin: the map first
            g = leaky(chain_def(np.broadcast_to(base, (k, base.shape[1])), W["w_g1"][:, :F_], sf[n * k:(n + 1) * k]), slope)
            h0 = lin_def(W["w_g2"], W["b_g2"], g)
            Q, K, V = lin_def(W["w_q"], None, h0), lin_def(W["w_k"], None, h0), lin_def(W["w_v"], None, h0)
            c = np.zeros((k, k), dtype=f32)
            for d in range(E):
                c = fmaf(Q[:, d:d + 1], K[None, :, d], c)
            c = (nf * c).astype(f32)
            e = dexp_np(c - c.max(1, keepdims=True))
            den = np.zeros((k,), dtype=f32)
            for j in range(k):
                den = den + e[:, j]
            a = (e / den[:, None]).astype(f32)
            hd = np.zeros((k, E), dtype=f32)
            for j in range(k):
                hd = fmaf(a[:, j:j + 1], V[j][None, :], hd)
            h1 = h0 + lin_def(W["w_o"], W["b_o"], hd)
            h2 = h1 + lin_def(W["w_f2"], W["b_f2"], relu(lin_def(W["w_f1"], W["b_f1"], h1)))
            x[n] = h2
            parts = np.zeros((16, E), dtype=f32)
            for i in range(k):
                parts[i % 16] = parts[i % 16] + h2[i]
            total = parts[0]
            for gp in range(1, 16):
                total = total + parts[gp]
            xg[n] = total / f32(k)
    assert x.dtype == f32 and xg.dtype == f32
    return x, xg


def order_embed_replay(obs, sf, W):
    x, xg = replay.order_embed(torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W))
    return x.numpy(), xg.numpy()


@pytest.mark.parametrize("cfg,N,k", [(SMALL, 1, 2), (SMALL, 3, 5), (SMALL, 2, 33), (REFERENCE, 2, 10)], ids=["1x2", "3x5", "2x33", "reference"])
def test_cpu_form_is_the_definition(cfg, N, k):
    rng = np.random.default_rng(100 * N + k)
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, N, k, cfg["L"], cfg["feat"])
    want_x, want_xg = order_embed_cpu(obs, sf, W, k)
    x, xg = order_embed_replay(obs, sf, W)
    assert x.shape == (N, k, cfg["embed"]) and xg.shape == (N, cfg["embed"]) and x.dtype == np.float32
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    assert np.isfinite(x).all() and (x != 0).any(axis=-1).all()
    np.testing.assert_allclose(xg, x.astype(np.float64).mean(1), rtol=0, atol=1e-5)
    # slots with the same shape feature in one bin come out the same: attention is permutation-equivariant only up to the
    # summation order, but equal inputs give equal rows
    sf2 = sf.copy()
    sf2[1] = sf2[0]
    x2, _ = order_embed_replay(obs, sf2, W)
    same_bits(x2[0, 0], x2[0, 1])


def test_a_strided_state_a_3d_feature_and_out_slices():
    rng = np.random.default_rng(6)
    W = make_layers(rng, **SMALL)
    N, k, E, F_ = 3, 5, SMALL["embed"], SMALL["feat"]
    obs, sf = make_obs(rng, N, k, SMALL["L"], F_)
    want_x, want_xg = order_embed_cpu(obs, sf, W, k)
    wide = np.full((N, obs.shape[1] + 6), 1e30, dtype=f32)
    wide[:, 2:2 + obs.shape[1]] = obs
    sf_w = np.full((N, k, F_ + 2), 1e30, dtype=f32)
    sf_w[:, :, :F_] = sf.reshape(N, k, F_)
    out = torch.full((N, k + 1, E + 3), 1e30)
    out_g = torch.full((N, E + 2), 1e30)
    x, xg = replay.order_embed(torch.from_numpy(wide)[:, 2:2 + obs.shape[1]], torch.from_numpy(sf_w)[:, :, :F_], weights_of(W),
                               out=out[:, :k, 1:1 + E], out_global=out_g[:, :E])
    assert x.data_ptr() == out[:, :k, 1:1 + E].data_ptr() and xg.data_ptr() == out_g.data_ptr()
    same_bits(x.numpy(), want_x)
    same_bits(xg.numpy(), want_xg)
    assert (out[:, k] == 1e30).all() and (out[:, :, 0] == 1e30).all() and (out[:, :, 1 + E:] == 1e30).all() and (out_g[:, E:] == 1e30).all()


def network_case(cfg, N, k, seed=11):
    rng = np.random.default_rng(seed)
    atoms, n_shapes, P, n_idx = 31, 5, 50, 65
    W = make_layers(rng, **cfg)
    obs, _ = make_obs(rng, N, k, cfg["L"], cfg["feat"])
    points = shp.make_points(rng, n_shapes, P)
    enc = shp.make_encoder(rng, 20, cfg["feat"])
    indices = rng.integers(0, P, n_idx).astype(np.int32)
    layers = stm.make_layers(rng, cfg["embed"], 24, atoms)
    return W, obs, points, enc, indices, layers, np.linspace(-1.0, 8.0, atoms).astype(f32)


def network_forms(case, k, dev, use_hip):
    """order_network_greedy_action and the three stages one by one on `dev`: asserted equal; -> actions, q."""
    W, obs, points, enc, indices, layers, support = case
    sp, sw, ow = replay.ShapePoints(points, dev), shp.weights_of(enc, dev), weights_of(W, dev)
    tw = replay.StreamWeights(*[l.to(dev) for l in layers])
    state, idx, z = torch.from_numpy(obs).to(dev), torch.from_numpy(indices).to(dev), torch.from_numpy(support).to(dev)
    q = torch.zeros((obs.shape[0], k), dtype=torch.float32, device=dev)
    act = replay.order_network_greedy_action(state, sp, idx, sw, ow, tw, z, q_out=q, use_hip=use_hip)
    sf = replay.shape_features(state[:, :k].contiguous(), sp, idx, sw, use_hip=use_hip)
    x, xg = replay.order_embed(state, sf, ow, use_hip=use_hip)
    if x.is_cuda:
        q2 = torch.zeros_like(q)
        act2 = replay.streams_greedy_action(x, xg, tw, z, None, q_out=q2, use_hip=use_hip)
    else:                                                    # the head's definition (test_dueling_cpu) on the defined logits
        v, a = replay.streams_logits(x, xg, tw, use_hip=False)
        act2, q2, _ = dueling_act_np(v.numpy(), a.numpy(), support)
        act2, q2 = torch.from_numpy(act2), torch.from_numpy(q2)
    assert torch.equal(act, act2) and torch.equal(q.view(torch.int32), q2.view(torch.int32))
    return act.cpu().numpy(), q.cpu().numpy()


def test_order_network_greedy_action_is_the_three_stages():
    k = 5
    act, q = network_forms(network_case(SMALL, 4, k), k, "cpu", None)
    assert act.dtype == np.int64 and ((act >= 0) & (act < k)).all()
    np.testing.assert_array_equal(act, q.argmax(1))


# ------------------------------------------------------------------ the reference's own forward ------------
GOLDEN_ORDER = dict(conv1="height_encoder.0", conv2="height_encoder.1", conv3="height_encoder.2", g1="gat_project_layer.0",
                    g2="gat_project_layer.1", q="embedder.W_query", k="embedder.W_key", v="embedder.W_val", o="embedder.W_out",
                    f1="embedder.ff.0", f2="embedder.ff.1")


def golden_case():
    g = np.load(GOLDEN)
    W = {"slope": float(g["negative_slope"]), "L": int(g["map_len"])}
    for short, name in GOLDEN_ORDER.items():
        W["w_" + short] = g[name + ".weight"]
        if short in BIASED:
            W["b_" + short] = g[name + ".bias"]
    return g, W, int(g["buffer_size"])


def reference_lines_f64(g, W, k):
    """model.py:355-383 (with :88-120 and :136-141) restated on float64 torch tensors, with the concatenation in its order."""
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(np.asarray(a)).double()  # noqa: E731
    obs, sf, slope, L = t(g["obs"]), t(g["shape_feature"]), W["slope"], W["L"]
    B, E = obs.shape[0], W["w_g2"].shape[0]
    a = F.leaky_relu(F.conv2d(obs[:, k:].reshape(B, 1, L, L), t(W["w_conv1"]), t(W["b_conv1"]), stride=2, padding=1), slope)
    a = F.leaky_relu(F.conv2d(a, t(W["w_conv2"]), t(W["b_conv2"]), stride=2, padding=1), slope)
    fmap = F.leaky_relu(F.conv2d(a, t(W["w_conv3"]), t(W["b_conv3"]), stride=1, padding=1), slope).reshape(B, -1)
    cat = torch.cat((sf.reshape(B, k, -1), fmap.repeat(1, k).reshape(B, k, -1)), dim=2).view(B * k, -1)
    h = F.linear(F.leaky_relu(F.linear(cat, t(W["w_g1"]), t(W["b_g1"])), slope), t(W["w_g2"]), t(W["b_g2"])).view(B, k, E)
    Q, K, V = F.linear(h, t(W["w_q"])), F.linear(h, t(W["w_k"])), F.linear(h, t(W["w_v"]))
    attn = torch.softmax((1 / np.sqrt(E)) * torch.matmul(Q, K.transpose(1, 2)), dim=-1)
    h = h + F.linear(torch.matmul(attn, V), t(W["w_o"]), t(W["b_o"]))
    h = h + F.linear(F.relu(F.linear(h, t(W["w_f1"]), t(W["b_f1"]))), t(W["w_f2"]), t(W["b_f2"]))
    return h.numpy(), h.mean(1).numpy()


def golden_errors(x, xg):
    """-> per output (x, xg): (max|given - d64|, max|the reference's float32 forward - d64|)."""
    g, W, k = golden_case()
    d_x, d_xg = reference_lines_f64(g, W, k)
    return [(np.abs(a.astype(np.float64) - d).max(), np.abs(ref.astype(np.float64) - d).max())
            for a, d, ref in ((x, d_x, g["embeddings"]), (xg, d_xg, g["graph_embed"]))]


def check_golden_bound(x, xg, what):
    for name, (err, ref_err) in zip(("embeddings", "graph_embed"), golden_errors(x, xg)):
        print(f"{what}, {name}: {err:.3g} from float64, the reference's float32 forward {ref_err:.3g}")
        # two float32 evaluations of one expression in different summation orders: test_embed_cpu.check_golden_bound's factor
        assert err <= 4 * ref_err


def test_definition_against_the_reference_forward():
    g, W, k = golden_case()
    assert k == 5 and g["obs"].shape == (3, 5 + 32 * 32) and g["shape_feature"].shape == (15, 128)
    assert g["embeddings"].shape == (3, 5, 128) and g["graph_embed"].shape == (3, 128)
    assert sum(W[n].size for n in NAMES) + sum(g[f"shape_encoder.{i}.{p}"].size for i in (0, 1) for p in ("weight", "bias")) == 256820
    x, xg = order_embed_replay(g["obs"], g["shape_feature"], W)
    check_golden_bound(x, xg, "the definition")


# ------------------------------------------------------------------ limits ------------
def test_wrapper_limits():
    rng = np.random.default_rng(9)
    W = make_layers(rng, **SMALL)
    w = weights_of(W)
    obs, sf = make_obs(rng, 2, 3, SMALL["L"], SMALL["feat"])
    t_obs, t_sf = torch.from_numpy(obs), torch.from_numpy(sf)
    replay.order_embed(t_obs, t_sf, w)
    with pytest.raises(ValueError):
        replay.order_embed(t_obs[:, :-2], t_sf, w)           # k = 1
    with pytest.raises(ValueError):
        replay.order_embed(t_obs[0], t_sf, w)
    with pytest.raises(ValueError):
        replay.order_embed(torch.zeros((1, 65 + 64)), torch.zeros((65, SMALL["feat"])), w)         # k = 65
    with pytest.raises(ValueError):
        replay.order_embed(t_obs, t_sf[:, :-1], w)
    with pytest.raises(ValueError):
        replay.order_embed(t_obs, t_sf[:-1], w)
    with pytest.raises(ValueError):
        replay.order_embed(t_obs, t_sf, w, out=torch.zeros((2, 3, SMALL["embed"] + 1)))
    with pytest.raises(ValueError):
        replay.order_embed(t_obs, t_sf, w, out_global=torch.zeros((2, SMALL["embed"]), dtype=torch.float64))
    for bad in (dict(L=36), dict(L=10), dict(L=4), dict(convs=(17, 5, 2)), dict(convs=(3, 33, 2)), dict(convs=(3, 5, 5)), dict(proj_hidden=257),
                dict(embed=257), dict(feat=257), dict(ff_hidden=257), dict(slope=-0.1)):
        with pytest.raises(ValueError):
            weights_of(make_layers(rng, **dict(SMALL, **bad)))
    he, gp, emb = layers_of(W)
    with pytest.raises(ValueError):
        replay.OrderEmbedWeights(he, gp, emb, map_len=32)    # the project layer is narrower than that map feature
    with pytest.raises(ValueError):
        replay.OrderEmbedWeights(he, gp, layers_of(W, n_heads=2)[2], map_len=8)
    with pytest.raises(ValueError):
        replay.OrderEmbedWeights(he, gp, types.SimpleNamespace(init_embed=None, layers=emb.layers * 2), map_len=8)
    with pytest.raises(ValueError):
        replay.OrderEmbedWeights(he, gp, types.SimpleNamespace(init_embed=object(), layers=emb.layers), map_len=8)
    other = layers_of(make_layers(rng, **dict(SMALL, embed=35)))[2]
    with pytest.raises(ValueError):
        replay.OrderEmbedWeights(he, gp, other, map_len=8)   # the attention layer's width is not gat_project_layer's
    with pytest.raises(RuntimeError):
        replay.order_embed(t_obs, t_sf, w, use_hip=True)     # no HIP device holds these tensors


@pytest.fixture(scope="module")
def lib():
    from irbpp_amd import _lib, build
    build.build()
    return _lib.load()


NULL = C.c_void_p(0)
BUF = np.zeros(4096, dtype=f32)
PTR = C.c_void_p(BUF.ctypes.data)


def abi_call(lib, **kw):
    d = dict(w=dict(), map_len=8, c1=2, c2=2, c3=1, feat=4, proj_hidden=8, embed=8, ff_hidden=4, slope=0.01, obs=PTR, obs_stride=3 + 64,
             sf=PTR, feat_stride=4, k_slots=3, n_env=1, base=PTR, x=PTR, env_stride=24, row_stride=8, xg=PTR, xg_stride=8, no_struct=False)
    d.update(kw)
    ptrs = {n: PTR.value for n in NAMES}
    ptrs.update(d["w"])
    ws = replay._IrbppOrderEmbedWeights(*(ptrs[n] for n in NAMES), *(d[n] for n in replay._ORDER_SIZES), d["slope"])
    return lib.irbpp_order_embed(None if d["no_struct"] else C.byref(ws), d["obs"], d["obs_stride"], d["sf"], d["feat_stride"], d["k_slots"],
                                 d["n_env"], d["base"], d["x"], d["env_stride"], d["row_stride"], d["xg"], d["xg_stride"], None)


WIDE = dict(obs_stride=1 << 20, feat_stride=1 << 10, env_stride=1 << 20, row_stride=1 << 10, xg_stride=1 << 10)
BAD = [dict(map_len=4), dict(map_len=10), dict(map_len=36, **WIDE), dict(c1=0), dict(c1=17), dict(c2=0), dict(c2=33), dict(c3=0), dict(c3=5),
       dict(feat=0), dict(feat=257, **WIDE), dict(proj_hidden=0), dict(proj_hidden=257), dict(embed=0), dict(embed=257, **WIDE),
       dict(ff_hidden=0), dict(ff_hidden=257), dict(slope=-0.5), dict(slope=float("nan")), dict(k_slots=1), dict(k_slots=0),
       dict(k_slots=65, **WIDE), dict(n_env=0), dict(n_env=-1), dict(obs_stride=3 + 63), dict(feat_stride=3), dict(row_stride=7),
       dict(env_stride=23), dict(xg_stride=7), dict(obs=NULL), dict(sf=NULL), dict(base=NULL), dict(x=NULL), dict(xg=NULL),
       dict(no_struct=True)] + [dict(w={n: None}) for n in NAMES]
ids = lambda d: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in d.items())      # noqa: E731


@pytest.mark.parametrize("bad", BAD, ids=ids)
def test_irbpp_order_embed_rejects_what_is_outside_its_limits(lib, bad):
    assert abi_call(lib, **bad) == -1                       # IRBPP_ERR_ARG before any HIP call
