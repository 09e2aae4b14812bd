"""The shape branch (csrc/irbpp_shapefeat.hip, replay.ShapePoints / ShapeEncoderWeights / shape_features) without a GPU.

The kernels' arithmetic is defined (the header of irbpp_shapefeat.hip); this file carries that definition as numpy code
(``shape_features_np``: row by row, point by point, no de-duplication; tests/test_gpu_shape_features.py and
tests/test_shape_features_kernel_on_host.py hold the kernels to it bit for bit) and checks

* the wrapper's CPU form (de-duplicated) against it, with the edge cases of the definition;
* ``leaky(max) == max(leaky)`` bit for bit on the test inputs (what lets the kernel apply the second leaky once);
* the definition against torch's own layers within the forward-error bound of the chains (``shape_bounds``);
* the IRBPP_ERR_ARG limits of the entry point (checked before any HIP call)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_streams_cpu import fmaf_np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
SLOPE = 0.01


# ------------------------------------------------------------------ the definition, in numpy ------------
def leaky_np(s, slope=SLOPE):
    with np.errstate(all="ignore"):
        return np.where(s > 0, s, f32(slope) * s).astype(f32)


def chain_np(w, b, x):
    """x [K] -> [J]: acc = b[j]; acc = fmaf(x[k], w[j][k], acc), k ascending."""
    acc = np.asarray(b, f32).copy()
    with np.errstate(all="ignore"):
        for k in range(w.shape[1]):
            acc = fmaf_np(x[k], w[:, k], acc)
    return acc


def key_np(h):
    """float32 -> uint32 in the floats' order, -0 below +0, every NaN on top"""
    b = np.ascontiguousarray(h, dtype=f32).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000), np.uint32(0xffffffff), key)


def unkey_np(key):
    bits = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7fffffff), ~key)
    return np.where(key == np.uint32(0xffffffff), np.uint32(0x7fc00000), bits).astype(np.uint32).view(f32)


def max_sticky_np(h):
    """max over axis 0 with a sticky NaN (the quiet NaN 0x7fc00000) and +0 above -0"""
    return unkey_np(key_np(h).max(axis=0))


def ids_np(ids, n_shapes):
    """ids (float: truncated toward zero like .long(); NaN and infinities are bad) -> int64 with -1 for every bad id"""
    ids = np.asarray(ids).reshape(-1)
    if ids.dtype.kind == "f":
        ok = (ids > -1) & (ids < n_shapes)
        return np.where(ok, np.trunc(np.where(ok, ids, 0)), -1).astype(np.int64)
    return np.where((ids >= 0) & (ids < n_shapes), ids, -1).astype(np.int64)


def shape_pre_np(points, indices, u, W):
    """s_j[f] before the second leaky, for shape u: [k, F].  Point by point."""
    P = points.shape[1]
    out = np.empty((len(indices), W["w2"].shape[0]), dtype=f32)
    for j, i in enumerate(indices):
        p = points[u, i] if 0 <= i < P else np.full(3, np.nan, dtype=f32)
        out[j] = chain_np(W["w2"], W["b2"], leaky_np(chain_np(W["w1"], W["b1"], p), W["slope"]))
    return out


def shape_features_np(points, indices, ids, W):
    """The definition: row by row, no de-duplication (a cache only spares the test the same row twice when asked to)."""
    u = ids_np(ids, points.shape[0])
    out = np.full((len(u), W["w2"].shape[0]), np.nan, dtype=f32)
    for m, s in enumerate(u):
        if s >= 0:
            out[m] = max_sticky_np(leaky_np(shape_pre_np(points, indices, s, W), W["slope"]))
    return out


def shape_features_fast_np(points, indices, ids, W):
    """The same values for the larger shapes of the GPU and host tests: vectorised over the points, once per distinct id
    (test_fast_form_is_the_definition holds it to shape_features_np)."""
    u = ids_np(ids, points.shape[0])
    idx = np.asarray(indices, np.int64)
    bad = (idx < 0) | (idx >= points.shape[1])
    out = np.full((len(u), W["w2"].shape[0]), np.nan, dtype=f32)
    with np.errstate(all="ignore"):
        for s in np.unique(u[u >= 0]):
            p = points[s][np.where(bad, 0, idx)].astype(f32)
            p[bad] = np.nan
            h1 = leaky_np(replay._lin_np(W["w1"], W["b1"], p), W["slope"])
            out[u == s] = max_sticky_np(leaky_np(replay._lin_np(W["w2"], W["b2"], h1), W["slope"]))
    return out


class Linear(object):
    """What ShapeEncoderWeights.from_layers asks of a layer, and nothing else."""

    def __init__(self, w, b):
        self.weight, self.bias = torch.from_numpy(np.ascontiguousarray(w)), torch.from_numpy(np.ascontiguousarray(b))

    def to(self, dev):
        self.weight, self.bias = self.weight.to(dev), self.bias.to(dev)
        return self


def make_encoder(rng, H1, F_, slope=SLOPE, b2_shift=0.0):
    return dict(w1=rng.standard_normal((H1, 3)).astype(f32), b1=(rng.standard_normal(H1) * 0.3).astype(f32),
                w2=(rng.standard_normal((F_, H1)) / np.sqrt(H1)).astype(f32),
                b2=(rng.standard_normal(F_) * 0.3 + b2_shift).astype(f32), slope=slope)


def weights_of(W, dev="cpu"):
    return replay.ShapeEncoderWeights.from_layers(Linear(W["w1"], W["b1"]).to(dev), Linear(W["w2"], W["b2"]).to(dev), W["slope"])


def make_points(rng, n_shapes, P):
    return (rng.standard_normal((n_shapes, P, 3)) * 0.2).astype(f32)


# ------------------------------------------------------------------ the wrapper's CPU form ------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(3)
    n_shapes, P, k, H1, F_ = 5, 40, 37, 9, 6
    points = make_points(rng, n_shapes, P)
    W = make_encoder(rng, H1, F_)
    W["b2"][1] = -50.0                                       # a feature whose every activation is negative
    indices = rng.integers(0, P, k).astype(np.int32)
    indices[:5] = [0, P - 1, 7, 7, 0]                        # both ends, duplicates
    ids = np.array([3, 0, 3, 4, 0, 3, 1], dtype=np.int64)
    return points, W, indices, ids, shape_features_np(points, indices, ids, W)


def test_cpu_form_is_the_definition(small):
    points, W, indices, ids, want = small
    sp = replay.ShapePoints(points, "cpu")
    w = weights_of(W)
    got = replay.shape_features(torch.from_numpy(ids), sp, torch.from_numpy(indices), w)
    assert got.dtype == torch.float32 and tuple(got.shape) == (7, 6) and not got.requires_grad
    np.testing.assert_array_equal(got.numpy(), want)
    assert not np.isnan(want).any()
    # rows of equal ids are identical
    for a, b in ((0, 2), (0, 5), (1, 4)):
        np.testing.assert_array_equal(got.numpy()[a].view(np.uint32), got.numpy()[b].view(np.uint32))
    assert (got.numpy()[0] != got.numpy()[1]).any()
    # the points table as a tensor, the ids as other integer types
    sp2 = replay.ShapePoints(torch.from_numpy(points).double(), torch.device("cpu"))
    np.testing.assert_array_equal(replay.shape_features(torch.from_numpy(ids.astype(np.int32)), sp2, torch.from_numpy(indices).long(), w).numpy(), want)
    # out: a slice of a wider tensor
    wide = torch.full((9, 11), 1e30)
    res = replay.shape_features(torch.from_numpy(ids), sp, torch.from_numpy(indices), w, out=wide[1:8, 2:8])
    assert res.data_ptr() == wide[1:8, 2:8].data_ptr()
    np.testing.assert_array_equal(wide[1:8, 2:8].numpy(), want)
    wide[1:8, 2:8] = 1e30
    assert (wide == 1e30).all()
    with pytest.raises(ValueError):
        replay.shape_features(torch.from_numpy(ids), sp, torch.from_numpy(indices), w, out=torch.zeros((7, 5)))
    with pytest.raises(RuntimeError, match="HIP device"):
        replay.shape_features(torch.from_numpy(ids), sp, torch.from_numpy(indices), w, use_hip=True)
    assert replay.SHAPE_FEATURES_HIP_DEFAULT in (False, True)


def test_fast_form_is_the_definition(small):
    points, W, indices, ids, want = small
    np.testing.assert_array_equal(shape_features_fast_np(points, indices, ids, W), want)


def test_leaky_of_the_max_is_the_max_of_the_leakies(small):
    points, W, indices, ids, want = small
    some_negative = False
    for m, u in enumerate(ids):
        s = shape_pre_np(points, indices, u, W)
        some_negative |= bool((s.max(axis=0) < 0).any())
        once = leaky_np(max_sticky_np(s), W["slope"])
        np.testing.assert_array_equal(once.view(np.uint32), max_sticky_np(leaky_np(s, W["slope"])).view(np.uint32))
        np.testing.assert_array_equal(once.view(np.uint32), want[m].view(np.uint32))
    assert some_negative, "no feature with every activation negative: the slope side of the equality is not exercised"
    edge = np.array([[-0.0, 0.0, -1e-44, -np.inf, np.nan], [0.0, -0.0, -3e-45, -1.0, 1.0]], dtype=f32)
    np.testing.assert_array_equal(leaky_np(max_sticky_np(edge)).view(np.uint32), max_sticky_np(leaky_np(edge)).view(np.uint32))
    assert max_sticky_np(edge).view(np.uint32).tolist() == [0, 0, 0x80000002, 0xbf800000, 0x7fc00000]


def test_float_ids_truncate_and_2d_ids_flatten(small):
    points, W, indices, ids, want = small
    sp = replay.ShapePoints(points, "cpu")
    w = weights_of(W)
    obs = torch.full((7, 13), 1e30)
    obs[:, 4] = torch.from_numpy(ids.astype(f32) + np.array([0.0, 0.9, 0.5, 0.25, -0.5, 0.999, 0.0], dtype=f32))
    got = replay.shape_features(obs[:, 4], sp, torch.from_numpy(indices), w)
    np.testing.assert_array_equal(got.numpy(), want)          # 0 - 0.5 truncates to 0, as .long() does
    assert torch.equal(obs[:, 4].long(), torch.from_numpy(ids))
    two = torch.from_numpy(np.array([[3, 0, 3], [4, 0, 1]], dtype=np.int64))
    got = replay.shape_features(two, sp, torch.from_numpy(indices), w)
    np.testing.assert_array_equal(got.numpy(), shape_features_np(points, indices, two.numpy(), W))
    assert tuple(got.shape) == (6, 6)
    pts = sp.gather(two, torch.from_numpy(indices))
    assert tuple(pts.shape) == (6, len(indices), 3)
    np.testing.assert_array_equal(pts.numpy(), points[two.numpy().reshape(-1)][:, indices])
    idx = sp.draw_indices(1024, generator=torch.Generator().manual_seed(1))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (1024,) and 0 <= int(idx.min()) and int(idx.max()) < points.shape[1]
    assert len(torch.unique(idx)) == points.shape[1]          # with replacement: 1024 draws from 40


def test_bad_ids_bad_indices_and_nan_weights(small):
    points, W, indices, ids, want = small
    sp = replay.ShapePoints(points, "cpu")
    w = weights_of(W)
    n = points.shape[0]
    bad = np.array([3, -1, n, 0], dtype=np.int64)
    got = replay.shape_features(torch.from_numpy(bad), sp, torch.from_numpy(indices), w).numpy()
    np.testing.assert_array_equal(got, shape_features_np(points, indices, bad, W))
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all() and not np.isnan(got[[0, 3]]).any()
    np.testing.assert_array_equal(got[0], want[0])
    fbad = np.array([3.0, -1.0, float(n), np.nan, np.inf, -np.inf, n - 0.5, -0.99], dtype=f32)
    got = replay.shape_features(torch.from_numpy(fbad), sp, torch.from_numpy(indices), w).numpy()
    np.testing.assert_array_equal(got, shape_features_np(points, indices, fbad, W))
    assert np.isnan(got[1:6]).all() and not np.isnan(got[[0, 6, 7]]).any()
    for wrong in (-1, points.shape[1]):
        idx = indices.copy()
        idx[11] = wrong
        got = replay.shape_features(torch.from_numpy(ids), sp, torch.from_numpy(idx), w).numpy()
        assert np.isnan(got).all()
        assert np.isnan(shape_features_np(points, idx, ids, W)).all()
    W2 = dict(W, w2=W["w2"].copy())
    W2["w2"][2, 4] = np.nan
    got = replay.shape_features(torch.from_numpy(ids), sp, torch.from_numpy(indices), weights_of(W2)).numpy()
    np.testing.assert_array_equal(got, shape_features_np(points, indices, ids, W2))
    assert np.isnan(got[:, 2]).all() and not np.isnan(np.delete(got, 2, axis=1)).any()
    assert (got[:, 2].view(np.uint32) == 0x7fc00000).all()


def test_weights_are_copies_until_refreshed():
    rng = np.random.default_rng(4)
    W = make_encoder(rng, 7, 5)
    l1, l2 = Linear(W["w1"], W["b1"]), Linear(W["w2"], W["b2"])
    w = replay.ShapeEncoderWeights.from_layers(l1, l2)
    assert (w.hidden, w.feat, w.slope) == (7, 5, 0.01) and w.w1.dtype == torch.float32 and w.w2.is_contiguous()
    l2.weight += 1
    assert not torch.equal(w.w2, l2.weight)
    assert torch.equal(w.refresh().w2, l2.weight)
    with pytest.raises(ValueError):
        replay.ShapeEncoderWeights.from_layers(l2, l1)
    with pytest.raises(ValueError):
        replay.ShapeEncoderWeights.from_layers(Linear(np.zeros((257, 3), f32), np.zeros(257, f32)), Linear(np.zeros((4, 257), f32), np.zeros(4, f32)))
    with pytest.raises(ValueError):
        replay.ShapePoints(np.zeros((3, 4)), "cpu")


# ------------------------------------------------------------------ the definition against torch's layers ------------
def shape_bounds(points, indices, u, W):
    """Bound on |definition - exact| per feature of shape u (float64 stands for exact; u = 2^-24; first-order terms times
    1.02 for the higher orders), the manner of test_streams_cpu.stream_bounds.

    A chain of K fused multiply-adds that starts at the bias rounds K times, each within u of a partial sum of magnitude at
    most T = |b| + sum_k |x_k| |w_k|; the standard forward-error bound with the margin for the products' own error terms is
    |chain - exact| <= 1.02 (K + 2) u T, T in float64 from the absolute values.
    h1: d1 = 1.02 (3 + 2) u (|b1| + |p| |W1|^T); leaky is 1-Lipschitz (slope <= 1) and its product rounds once: + u |h1|.
    s:  the hidden errors pass through |W2| and the second chain rounds H1 times:
        d2 = d1' |W2|^T + 1.02 (H1 + 2) u (|b2| + (|h1| + d1') |W2|^T);  the second leaky: + u |s|.
    The max over the points is 1-Lipschitz in the sup norm: the bound of the max is the max of the bounds."""
    d = lambda t: np.abs(np.asarray(t, f64))               # noqa: E731
    p = points[u][indices].astype(f64)
    H1 = W["w1"].shape[0]
    s1 = p @ W["w1"].astype(f64).T + W["b1"].astype(f64)
    d1 = 1.02 * 5 * U * (d(W["b1"]) + d(p) @ d(W["w1"]).T)
    h1 = np.where(s1 > 0, s1, W["slope"] * s1)
    d1 = d1 + U * d(h1)
    s2 = h1 @ W["w2"].astype(f64).T + W["b2"].astype(f64)
    d2 = d1 @ d(W["w2"]).T + 1.02 * (H1 + 2) * U * (d(W["b2"]) + (d(h1) + d1) @ d(W["w2"]).T)
    d2 = d2 + U * (d(s2) + d2)
    return d2.max(axis=0)


def torch_layers(points, indices, u, W, dtype):
    p = torch.from_numpy(points[u][indices]).to(dtype)
    t = lambda k: torch.from_numpy(W[k]).to(dtype)          # noqa: E731
    h = F.leaky_relu(F.linear(F.leaky_relu(F.linear(p, t("w1"), t("b1")), W["slope"]), t("w2"), t("b2")), W["slope"])
    return torch.max(h, dim=0)[0].numpy()


@pytest.mark.parametrize("H1,F_,k", [(128, 128, 200), (5, 3, 64), (130, 67, 65), (256, 256, 33)])
def test_definition_against_the_reference(H1, F_, k):
    rng = np.random.default_rng(700 + H1)
    points = make_points(rng, 3, 500)
    W = make_encoder(rng, H1, F_)
    indices = rng.integers(0, 500, k).astype(np.int32)
    got = shape_features_fast_np(points, indices, np.array([0, 1, 2]), W)
    for u in range(3):
        bound = shape_bounds(points, indices, u, W)
        want64 = torch_layers(points, indices, u, W, torch.float64)
        got32 = torch_layers(points, indices, u, W, torch.float32)       # the slope in float64 there against float32 here: u |s|
        e_def, e_torch = np.abs(got[u] - want64), np.abs(got32 - want64)
        print(f"u {u}: definition {e_def.max():.3g}, torch float32 {e_torch.max():.3g}, bound {bound.min():.3g} .. {bound.max():.3g}")
        assert (e_def <= bound).all() and (e_torch <= bound).all()
        assert (bound < 1e-3).all(), "the bound says nothing beside values of order 1"


# ------------------------------------------------------------------ limits of the entry point ------------
@pytest.fixture(scope="module")
def lib():
    from irbpp_amd import _lib, build
    build.build()
    return _lib.load()


NULL = C.c_void_p(0)
BUF = np.zeros(4096, dtype=f32)
PTR = C.c_void_p(BUF.ctypes.data)


def call(lib, **kw):
    d = dict(points=PTR, n_shapes=4, n_points=10, indices=PTR, k=100, ids=PTR, ids_are_float=0, ids_stride=1, m_rows=3, w={}, hidden=8,
             feat=8, slope=0.01, partial=PTR, chunks=None, out=PTR, out_stride=8, no_struct=False)
    d.update(kw)
    ptrs = dict(w1=PTR.value, b1=PTR.value, w2=PTR.value, b2=PTR.value)
    ptrs.update(d["w"])
    enc = replay._IrbppShapeEncoder(ptrs["w1"], ptrs["b1"], ptrs["w2"], ptrs["b2"], d["hidden"], d["feat"], d["slope"])
    chunks = lib.irbpp_shape_features_chunks(d["n_shapes"], d["k"]) if d["chunks"] is None else d["chunks"]
    return lib.irbpp_shape_features(d["points"], d["n_shapes"], d["n_points"], d["indices"], d["k"], d["ids"], d["ids_are_float"],
                                    d["ids_stride"], d["m_rows"], None if d["no_struct"] else C.byref(enc), d["partial"], chunks,
                                    d["out"], d["out_stride"], None)


BAD = [dict(hidden=0), dict(hidden=257), dict(feat=0), dict(feat=257, out_stride=257), dict(k=0, chunks=1), dict(k=4097, chunks=1),
       dict(n_shapes=0, chunks=1), dict(n_shapes=65536, chunks=1), dict(n_points=0), dict(m_rows=0), dict(m_rows=-3), dict(ids_stride=0),
       dict(out_stride=7), dict(chunks=1), dict(chunks=3), dict(chunks=0), dict(slope=-0.5), dict(slope=float("nan")), dict(points=NULL),
       dict(indices=NULL), dict(ids=NULL), dict(partial=NULL), dict(out=NULL), dict(no_struct=True)] + \
      [dict(w={n: None}) for n in ("w1", "b1", "w2", "b2")]
ids_of = lambda d: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in d.items())      # noqa: E731


@pytest.mark.parametrize("bad", BAD, ids=ids_of)
def test_shape_features_rejects_what_is_outside_its_limits(lib, bad):
    assert call(lib, **bad) == -1                           # IRBPP_ERR_ARG before any HIP call


def test_chunks_fill_the_chip_for_small_sets_and_cover_every_point(lib):
    assert lib.irbpp_shape_features_chunks(4, 100) == 2      # what the rejected chunks=1 and chunks=3 above are beside
    assert lib.irbpp_shape_features_chunks(8, 1024) == lib.irbpp_shape_features_chunks(100, 1024) == 16
    assert lib.irbpp_shape_features_chunks(300, 1000) == 6 and lib.irbpp_shape_features_chunks(65535, 4096) == 1
    for bad in ((0, 5), (65536, 5), (3, 0), (3, 4097)):
        assert lib.irbpp_shape_features_chunks(*bad) == 0
    for k in (1, 63, 64, 65, 1000, 1024, 4096):
        got = [lib.irbpp_shape_features_chunks(n, k) for n in (1, 7, 100, 300, 2048, 5000)]
        assert got[0] == -(-k // 64) and got[-1] == 1 and got == sorted(got, reverse=True), (k, got)    # at most one wave of points each
