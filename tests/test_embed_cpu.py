"""The embedding stage's defined arithmetic (csrc/irbpp_embed.hip) without a GPU: the definition restated here row by row in
numpy -- the convolutions tap by tap, project_layer[0] as ONE chain over the reference's concatenation (shape feature, map
feature, candidate embedding), the mean as dueling_mean's 16 parts -- against replay.embed on CPU tensors, which runs the
factored form (the first F + M steps of every chain once per bin): bit for bit, so the factoring changes nothing.  Then the
reference's own forward (tests/golden/embed_ref.npz, written by tests/golden/make_embed_golden.py): the definition is as
close to the float64 evaluation of the reference's lines as the reference's float32 evaluation is.

Measured on the golden (max over all elements, against float64): the definition 7.05e-07 (embeddings) / 3.20e-07
(graph_embed), the reference's float32 forward 4.96e-07 / 2.47e-07."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from irbpp_amd import replay

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "embed_ref.npz")
# L, (c1, c2, c3), feat, cand_hidden, cand_embed, proj_hidden, embed
SMALL = dict(L=8, convs=(3, 5, 2), feat=40, cand_hidden=7, cand_embed=33, proj_hidden=48, embed=36)
REFERENCE = dict(L=32, convs=(16, 32, 4), feat=128, cand_hidden=32, cand_embed=128, proj_hidden=256, embed=128)
NAMES = replay._EMBED_FIELDS


def make_layers(rng, L, convs, feat, cand_hidden, cand_embed, proj_hidden, embed, slope=0.01):
    """-> dict of float32 arrays in torch's layouts under the names of irbpp_embed_weights, 'slope' and 'L'."""
    c1, c2, c3 = convs
    M = c3 * (L // 4) ** 2
    shapes = [(c1, 1, 4, 4), (c2, c1, 4, 4), (c3, c2, 3, 3), (cand_hidden, 4), (cand_embed, cand_hidden),
              (proj_hidden, feat + M + cand_embed), (embed, proj_hidden)]
    W = {"slope": slope, "L": L}
    for i, shape in enumerate(shapes):
        fan_in = int(np.prod(shape[1:]))
        W[NAMES[2 * i]] = (rng.standard_normal(shape) / np.sqrt(fan_in)).astype(f32)
        W[NAMES[2 * i + 1]] = rng.uniform(-0.3, 0.3, shape[0]).astype(f32)
    return W


def weights_of(W, device="cpu"):
    """replay.EmbedWeights from such a dict: three sequences of objects with a weight and a bias."""
    layers = [types.SimpleNamespace(weight=torch.from_numpy(W[NAMES[2 * i]]).to(device), bias=torch.from_numpy(W[NAMES[2 * i + 1]]).to(device))
              for i in range(7)]
    return replay.EmbedWeights(layers[:3], layers[3:5], layers[5:], W["slope"], map_len=W["L"])


def make_obs(rng, N, S, L, feat):
    """An observation block [N, 5 S + 9 + L^2] and a shape feature [N, feat]: masks 0 / 1 mixed, bin 0 all valid, the last bin
    (of more than one) all invalid, mask values 0.5 and NaN and an invalid row with a NaN candidate where there is room,
    heightmaps of both signs."""
    obs = rng.uniform(-1.0, 1.0, (N, 5 * S + 9 + L * L)).astype(f32)
    rows = obs[:, :5 * S].reshape(N, S, 5)
    rows[:, :, 4] = (rng.random((N, S)) < 0.6).astype(f32)
    rows[0, :, 4] = 1.0
    if N > 1:
        rows[N - 1, :, 4] = 0.0
    if S > 4:
        rows[0, 1, 4] = 0.5
        rows[0, 2, 4] = np.nan
        rows[0, 3, 4] = 0.0
        rows[0, 3, 1] = np.nan
        rows[N - 1, S - 1, 0] = np.inf
        rows[N - 1, S - 1, 4] = 0.0
    obs[:, 5 * S] = rng.integers(0, 5, N)
    return obs, rng.uniform(-0.5, 1.0, (N, feat)).astype(f32)


def fmaf(a, b, c):
    return replay._fmaf_np(np.asarray(a, dtype=f32), np.asarray(b, dtype=f32), np.asarray(c, dtype=f32))


def leaky(s, slope):
    return np.where(s > 0, s, f32(slope) * s).astype(f32)


def conv_def(x, w, b, stride, slope):
    """x [Cin, H, H] -> leaky(conv) [Cout, H', H'] with pad 1: the chains advance tap by tap in (c_in, ky, kx) order over a
    zero-padded copy, all outputs at once."""
    cin, H = x.shape[0], x.shape[1]
    k = w.shape[2]
    n = (H + 2 - k) // stride + 1
    xp = np.zeros((cin, H + 2, H + 2), dtype=f32)
    xp[:, 1:H + 1, 1:H + 1] = x
    acc = np.broadcast_to(b[:, None, None], (w.shape[0], n, n)).astype(f32)
    span = stride * (n - 1) + 1
    for ci in range(cin):
        for ky in range(k):
            for kx in range(k):
                acc = fmaf(xp[ci, ky:ky + span:stride, kx:kx + span:stride][None], w[:, ci, ky, kx][:, None, None], acc)
    return leaky(acc, slope)


def lin_def(w, b, x):
    """x [R, K] -> [R, J]: acc = b[j]; acc = fmaf(x[k], w[j][k], acc), k ascending."""
    acc = np.broadcast_to(b, (x.shape[0], w.shape[0])).astype(f32)
    for k in range(w.shape[1]):
        acc = fmaf(x[:, k:k + 1], w[None, :, k], acc)
    return acc


def embed_def(obs, sf, W, S):
    """The definition, unfactored: -> x [N, S, E], xg [N, E]."""
    N, L, slope = obs.shape[0], W["L"], W["slope"]
    E = W["w_p2"].shape[0]
    x = np.zeros((N, S, E), dtype=f32)
    xg = np.zeros((N, E), dtype=f32)
    with np.errstate(all="ignore"):
        for n in range(N):
            rows = obs[n, :5 * S].reshape(S, 5)
            hm = obs[n, 5 * S + 9:5 * S + 9 + L * L].reshape(1, L, L)
            fmap = conv_def(conv_def(conv_def(hm, W["w_conv1"], W["b_conv1"], 2, slope), W["w_conv2"], W["b_conv2"], 2, slope),
                            W["w_conv3"], W["b_conv3"], 1, slope).reshape(-1)
            e2 = lin_def(W["w_c2"], W["b_c2"], leaky(lin_def(W["w_c1"], W["b_c1"], rows[:, :4]), slope))
            cat = np.concatenate([np.broadcast_to(sf[n], (S, sf.shape[1])), np.broadcast_to(fmap, (S, fmap.shape[0])), e2], axis=1)
            xr = lin_def(W["w_p2"], W["b_p2"], leaky(lin_def(W["w_p1"], W["b_p1"], cat), slope))
            for r in range(S):
                x[n, r] = xr[r] if rows[r, 4] == f32(1) else f32(0)
            parts = np.zeros((16, E), dtype=f32)
            for r in range(S):                               # part r % 16 takes its rows in ascending order
                parts[r % 16] = parts[r % 16] + x[n, r]
            total = parts[0]
            for g in range(1, 16):
                total = total + parts[g]
            xg[n] = total / f32(S)
    return x, xg


def embed_cpu(obs, sf, W):
    x, xg = replay.embed(torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W))
    return x.numpy(), xg.numpy()


def same_bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("cfg,N,S", [(SMALL, 1, 1), (SMALL, 3, 17), (SMALL, 2, 33), (REFERENCE, 2, 5)], ids=["1x1", "3x17", "2x33", "reference"])
def test_factored_emulation_is_the_unfactored_definition(cfg, N, S):
    """replay.embed on CPU tensors (base once per bin, every row continuing from it) against one chain over the concatenation."""
    rng = np.random.default_rng(100 * N + S)
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, N, S, cfg["L"], cfg["feat"])
    want_x, want_xg = embed_def(obs, sf, W, S)
    x, xg = embed_cpu(obs, sf, W)
    assert x.shape == (N, S, cfg["embed"]) and xg.shape == (N, cfg["embed"]) and x.dtype == np.float32
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    valid = obs[:, :5 * S].reshape(N, S, 5)[:, :, 4] == 1
    assert (x[valid] != 0).any(axis=-1).all() and np.isfinite(x[valid]).all()


def test_invalid_rows_are_positive_zero_and_the_mean_is_over_all_rows():
    rng = np.random.default_rng(5)
    W = make_layers(rng, **SMALL)
    N, S = 3, 8
    obs, sf = make_obs(rng, N, S, SMALL["L"], SMALL["feat"])
    rows = obs[:, :5 * S].reshape(N, S, 5)
    rows[1, :, 4] = 0.0
    rows[1, 5, 4] = 1.0                                      # bin 1: one valid row of eight
    x, xg = embed_cpu(obs, sf, W)
    bits = x.view(np.uint32)
    for r, why in ((1, "mask 0.5"), (2, "a NaN mask"), (3, "mask 0 with a NaN candidate")):
        assert (bits[0, r] == 0).all(), why
    assert (bits[2] == 0).all() and (xg[2].view(np.uint32) == 0).all()       # the all-invalid bin, an infinity in its last row
    assert np.isfinite(x).all() and (x[0, 0] != 0).any()
    same_bits(xg[1], x[1, 5] / f32(8))                       # over S = 8, not over the one valid row: zeros add nothing
    np.testing.assert_allclose(xg[0], x[0].astype(np.float64).mean(0), rtol=0, atol=1e-6)


def test_a_slice_of_a_wider_block_and_out_tensors():
    rng = np.random.default_rng(6)
    W = make_layers(rng, **SMALL)
    N, S, E = 2, 5, SMALL["embed"]
    obs, sf = make_obs(rng, N, S, SMALL["L"], SMALL["feat"])
    want_x, want_xg = embed_cpu(obs, sf, W)
    wide = np.full((N, obs.shape[1] + 6), 1e30, dtype=f32)
    wide[:, 2:2 + obs.shape[1]] = obs
    out = torch.full((N, S + 1, E + 3), 1e30)
    out_g = torch.full((N, E + 2), 1e30)
    x, xg = replay.embed(torch.from_numpy(wide)[:, 2:2 + obs.shape[1]], torch.from_numpy(sf), weights_of(W), out=out[:, :S, 1:1 + E],
                         out_global=out_g[:, :E])
    assert x.data_ptr() == out[:, :S, 1:1 + E].data_ptr() and xg.data_ptr() == out_g.data_ptr()
    same_bits(x.numpy(), want_x)
    same_bits(xg.numpy(), want_xg)
    assert (out[:, S] == 1e30).all() and (out[:, :, 0] == 1e30).all() and (out[:, :, 1 + E:] == 1e30).all() and (out_g[:, E:] == 1e30).all()


def golden_case():
    g = np.load(GOLDEN)
    order = [("height_encoder", 0), ("height_encoder", 1), ("height_encoder", 2), ("init_candidate_embed", 0), ("init_candidate_embed", 1),
             ("project_layer", 0), ("project_layer", 1)]
    W = {"slope": float(g["negative_slope"]), "L": int(g["map_len"])}
    for i, (name, j) in enumerate(order):
        W[NAMES[2 * i]], W[NAMES[2 * i + 1]] = g[f"{name}.{j}.weight"], g[f"{name}.{j}.bias"]
    return g, W, int(g["selected_action"])


def reference_lines_f64(g, W, S):
    """model.py:318-326, :337-352 restated on float64 torch tensors, with the concatenation."""
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(np.asarray(a)).double()  # noqa: E731
    obs, sf, slope, L = t(g["obs"]), t(g["shape_feature"]), W["slope"], W["L"]
    B = obs.shape[0]
    rows = obs[:, :5 * S].reshape(B, S, 5)
    a = F.leaky_relu(F.conv2d(obs[:, 5 * S + 9:].reshape(B, 1, L, L), t(W["w_conv1"]), t(W["b_conv1"]), stride=2, padding=1), slope)
    a = F.leaky_relu(F.conv2d(a, t(W["w_conv2"]), t(W["b_conv2"]), stride=2, padding=1), slope)
    fmap = F.leaky_relu(F.conv2d(a, t(W["w_conv3"]), t(W["b_conv3"]), stride=1, padding=1), slope).reshape(B, -1)
    e2 = F.linear(F.leaky_relu(F.linear(rows[:, :, :4], t(W["w_c1"]), t(W["b_c1"])), slope), t(W["w_c2"]), t(W["b_c2"]))
    cat = torch.cat((sf.repeat(1, S).reshape(B, S, -1), fmap.repeat(1, S).reshape(B, S, -1), e2), dim=2)
    x = F.linear(F.leaky_relu(F.linear(cat, t(W["w_p1"]), t(W["b_p1"])), slope), t(W["w_p2"]), t(W["b_p2"]))
    x[(1 - rows[:, :, 4]).bool()] = 0
    return x.numpy(), x.mean(1).numpy()


def golden_errors(x, xg):
    """-> per output (x, xg): (max|given - d64|, max|the reference's float32 forward - d64|); the zero patterns are compared."""
    g, W, S = golden_case()
    d_x, d_xg = reference_lines_f64(g, W, S)
    np.testing.assert_array_equal((x == 0).all(-1), (g["embeddings"] == 0).all(-1))
    np.testing.assert_array_equal((x == 0).all(-1), g["obs"][:, :5 * S].reshape(-1, S, 5)[:, :, 4] != 1)
    return [(np.abs(a.astype(np.float64) - d).max(), np.abs(ref.astype(np.float64) - d).max())
            for a, d, ref in ((x, d_x, g["embeddings"]), (xg, d_xg, g["graph_embed"]))]


def check_golden_bound(x, xg, what):
    for name, (err, ref_err) in zip(("embeddings", "graph_embed"), golden_errors(x, xg)):
        print(f"{what}, {name}: {err:.3g} from float64, the reference's float32 forward {ref_err:.3g}")
        # two float32 evaluations of one expression in different summation orders: the factor covers the tail between them
        assert err <= 4 * ref_err


def test_definition_against_the_reference_forward():
    g, W, S = golden_case()
    assert sum(W[n].size for n in NAMES) + sum(g[f"shape_encoder.{i}.{p}"].size for i in (0, 1) for p in ("weight", "bias")) == 195284
    x, xg = embed_cpu(g["obs"], g["shape_feature"], W)
    check_golden_bound(x, xg, "the definition")
    assert (x[1] == 0).all() and (xg[1] == 0).all()          # the golden's all-invalid bin


def test_argument_limits():
    rng = np.random.default_rng(9)
    W = make_layers(rng, **SMALL)
    w = weights_of(W)
    obs, sf = make_obs(rng, 2, 3, SMALL["L"], SMALL["feat"])
    t_obs, t_sf = torch.from_numpy(obs), torch.from_numpy(sf)
    replay.embed(t_obs, t_sf, w)
    with pytest.raises(ValueError):
        replay.embed(t_obs[:, :-1], t_sf, w)                 # obs_len is not 5 S + 9 + L^2
    with pytest.raises(ValueError):
        replay.embed(t_obs[0], t_sf, w)
    with pytest.raises(ValueError):
        replay.embed(torch.zeros((1, 5 * 1025 + 9 + 64)), torch.zeros((1, SMALL["feat"])), w)       # S = 1025
    with pytest.raises(ValueError):
        replay.embed(t_obs, t_sf[:, :-1], w)
    with pytest.raises(ValueError):
        replay.embed(t_obs, t_sf, w, out=torch.zeros((2, 3, SMALL["embed"] + 1)))
    with pytest.raises(ValueError):
        replay.embed(t_obs, t_sf, w, out_global=torch.zeros((2, SMALL["embed"]), dtype=torch.float64))
    for bad in (dict(L=36), dict(L=10), dict(L=4), dict(convs=(17, 5, 2)), dict(convs=(3, 33, 2)), dict(convs=(3, 5, 5)), dict(cand_hidden=65),
                dict(cand_embed=257), dict(proj_hidden=257), dict(embed=257), dict(feat=257), dict(slope=-0.1)):
        with pytest.raises(ValueError):
            weights_of(make_layers(rng, **dict(SMALL, **bad)))
    layers = [types.SimpleNamespace(weight=torch.from_numpy(W[NAMES[2 * i]]), bias=torch.from_numpy(W[NAMES[2 * i + 1]])) for i in range(7)]
    with pytest.raises(ValueError):
        replay.EmbedWeights(layers[:3], layers[3:5], layers[5:], map_len=32)          # the project layer is narrower than that map feature
    with pytest.raises(ValueError):
        replay.EmbedWeights(layers[:2], layers[3:5], layers[5:], map_len=8)
    with pytest.raises(RuntimeError):
        replay.embed(t_obs, t_sf, w, use_hip=True)           # no HIP device holds these tensors


# ------------------------------------------------------------------ limits of the entry point ------------
@pytest.fixture(scope="module")
def lib():
    from irbpp_amd import _lib, build
    build.build()
    return _lib.load()


NULL = C.c_void_p(0)
BUF = np.zeros(4096, dtype=f32)
PTR = C.c_void_p(BUF.ctypes.data)


def abi_call(lib, **kw):
    d = dict(w=dict(), map_len=8, c1=2, c2=2, c3=1, feat=4, cand_hidden=4, cand_embed=4, proj_hidden=8, embed=8, slope=0.01, obs=PTR,
             obs_stride=5 * 3 + 9 + 64, sf=PTR, feat_stride=4, s_rows=3, n_env=1, base=PTR, x=PTR, env_stride=24, row_stride=8, xg=PTR,
             xg_stride=8, no_struct=False)
    d.update(kw)
    ptrs = {n: PTR.value for n in NAMES}
    ptrs.update(d["w"])
    ws = replay._IrbppEmbedWeights(*(ptrs[n] for n in NAMES), *(d[n] for n in replay._EMBED_SIZES), d["slope"])
    return lib.irbpp_embed(None if d["no_struct"] else C.byref(ws), d["obs"], d["obs_stride"], d["sf"], d["feat_stride"], d["s_rows"],
                           d["n_env"], d["base"], d["x"], d["env_stride"], d["row_stride"], d["xg"], d["xg_stride"], None)


WIDE = dict(obs_stride=1 << 20, feat_stride=1 << 10, env_stride=1 << 20, row_stride=1 << 10, xg_stride=1 << 10)
BAD = [dict(map_len=4), dict(map_len=10), dict(map_len=36, **WIDE), dict(c1=0), dict(c1=17), dict(c2=0), dict(c2=33), dict(c3=0), dict(c3=5),
       dict(feat=0), dict(feat=257, **WIDE), dict(cand_embed=0), dict(cand_embed=257), dict(proj_hidden=0), dict(proj_hidden=257),
       dict(embed=0), dict(embed=257, **WIDE), dict(cand_hidden=0), dict(cand_hidden=65), dict(slope=-0.5), dict(slope=float("nan")),
       dict(s_rows=0), dict(s_rows=1025, **WIDE), dict(n_env=0), dict(n_env=-1), dict(obs_stride=5 * 3 + 9 + 63), dict(feat_stride=3),
       dict(row_stride=7), dict(env_stride=23), dict(xg_stride=7), dict(obs=NULL), dict(sf=NULL), dict(base=NULL), dict(x=NULL), dict(xg=NULL),
       dict(no_struct=True)] + [dict(w={n: None}) for n in NAMES]
ids = lambda d: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in d.items())      # noqa: E731


@pytest.mark.parametrize("bad", BAD, ids=ids)
def test_irbpp_embed_rejects_what_is_outside_its_limits(lib, bad):
    assert abi_call(lib, **bad) == -1                       # IRBPP_ERR_ARG before any HIP call
