"""csrc/irbpp_shapefeat.hip on the GPU, bit for bit against the numpy definition of tests/test_shape_features_cpu.py
(assert_array_equal), through the C ABI on a stream of the test's own and through replay.shape_features(use_hip=True).

Every id and out argument is a slice of a wider tensor with 1e30 (999999 for integer ids: a bad id) around it, checked
untouched; the workspace is filled with 1e30 before the ABI call, so a read of an absent shape's rows would show in the
result, and those rows are checked unwritten.  Shapes (k, H1, F, n_shapes, M, P): k of {1, 63, 64, 65, 1000, 1024} (below, at
and above one wave of points, a short last chunk, the workload's value); (H1, F) of {(128, 128), (5, 3), (130, 67), (256, 256)}
(full, short and single short blocks of hidden units and features; the widest at k = 65 only); n_shapes {1, 7}, M {1, 5, 300}
with repeats, absent shapes, -1 and n_shapes among the ids; P {1, 100000}."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_shape_features_cpu import BAD, f32, ids_np, ids_of, make_encoder, make_points, shape_bounds, shape_features_fast_np, weights_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 1e30
OBS_LEN = 13
CASES = [(1, 5, 3, 1, 1, 1), (63, 128, 128, 7, 5, 100000), (64, 5, 3, 7, 300, 100000), (65, 130, 67, 7, 5, 100000),
         (65, 256, 256, 1, 1, 100000), (1000, 130, 67, 7, 300, 100000), (1024, 128, 128, 7, 5, 100000), (1000, 5, 3, 1, 300, 1),
         (1024, 5, 3, 7, 1, 100000)]


def make_ids(rng, n_shapes, M):
    if M == 1:
        return np.array([n_shapes - 1], dtype=np.int64)
    ids = rng.integers(0, n_shapes, M).astype(np.int64)
    if n_shapes > 2:
        ids[ids == 2] = 3                                    # shape 2 stays absent
        ids[0] = ids[M - 1] = 4                              # repeats
    ids[1], ids[3] = -1, n_shapes
    return ids


@functools.lru_cache(maxsize=None)
def case(k, H1, F_, n_shapes, M, P, b2_shift=0.0):
    """-> points, W, indices, ids and the definition's result: computed once and shared (treat as read-only)."""
    rng = np.random.default_rng(1000 * k + 7 * H1 + F_ + n_shapes + M)
    points = make_points(rng, n_shapes, P)
    W = make_encoder(rng, H1, F_, b2_shift=b2_shift)
    indices = rng.integers(0, P, k).astype(np.int32)
    indices[0], indices[-1] = P - 1, 0
    if k > 4:
        indices[2] = indices[3]                              # a duplicate for certain
    ids = make_ids(rng, n_shapes, M)
    return points, W, indices, ids, shape_features_fast_np(points, indices, ids, W)


def _lib():
    from irbpp_amd import _lib as L
    return L, L.load()


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


def dev_encoder(W):
    keep = [torch.from_numpy(np.ascontiguousarray(W[n])).to(DEV) for n in ("w1", "b1", "w2", "b2")]
    return keep, replay._IrbppShapeEncoder(*(t.data_ptr() for t in keep), W["w1"].shape[0], W["w2"].shape[0], W["slope"])


def abi_call(points, W, indices, ids, float_ids=False, expect_chunks=None):
    """irbpp_shape_features on a stream of the test's own: ids a column of a poisoned [M, OBS_LEN] block, out a slice of a
    poisoned wider tensor, the workspace poisoned.  -> out as numpy."""
    L, lib = _lib()
    n_shapes, P = points.shape[:2]
    M, k, F_ = len(ids), len(indices), W["w2"].shape[0]
    chunks = lib.irbpp_shape_features_chunks(n_shapes, k)
    if expect_chunks is not None:
        assert chunks == expect_chunks
    pts, idx = torch.from_numpy(points).to(DEV), torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(DEV)
    block = torch.full((M, OBS_LEN), POISON if float_ids else 999999, dtype=torch.float32 if float_ids else torch.int64, device=DEV)
    block[:, 5] = torch.from_numpy(np.asarray(ids)).to(DEV)
    before = block.clone()
    wide = torch.full((M + 2, F_ + 7), POISON, dtype=torch.float32, device=DEV)
    partial = torch.full((n_shapes, chunks, F_), POISON, dtype=torch.float32, device=DEV)
    keep, enc = dev_encoder(W)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        L.check(lib.irbpp_shape_features(_ptr(pts), n_shapes, P, _ptr(idx), k, _ptr(block, 5), int(float_ids), OBS_LEN, M, C.byref(enc),
                                         _ptr(partial), chunks, _ptr(wide, F_ + 7 + 3), F_ + 7, C.c_void_p(stream.cuda_stream)),
                "irbpp_shape_features")
    stream.synchronize()
    assert torch.equal(block.view(torch.int32), before.view(torch.int32))      # as bits: a NaN id is itself
    out = wide[1:1 + M, 3:3 + F_].cpu().numpy()
    wide[1:1 + M, 3:3 + F_] = POISON
    assert bool((wide == POISON).all())
    present = set(ids_np(ids, n_shapes).tolist())
    written = (partial != POISON).flatten(1).any(1).cpu().numpy()
    assert written.tolist() == [u in present for u in range(n_shapes)]        # absent shapes: never written
    return out


def wrapper_call(points, W, indices, ids, float_ids=True):
    """replay.shape_features(use_hip=True): the ids as the float32 column of an [M, OBS_LEN] observation block."""
    M, F_ = len(ids), W["w2"].shape[0]
    sp = replay.ShapePoints(points, DEV)
    w = weights_of(W, DEV)
    obs = torch.full((M, OBS_LEN), POISON, dtype=torch.float32, device=DEV)
    if float_ids:
        obs[:, 0] = torch.from_numpy(np.asarray(ids).astype(f32) + np.where(np.asarray(ids) >= 0, f32(0.5), f32(0))).to(DEV)
        arg = obs[:, 0]
        assert arg.stride(0) == OBS_LEN
    else:
        arg = torch.from_numpy(np.asarray(ids)).to(DEV)
    before = obs.clone()
    wide = torch.full((M + 1, F_ + 4), POISON, dtype=torch.float32, device=DEV)
    res = replay.shape_features(arg, sp, torch.from_numpy(indices).to(DEV), w, use_hip=True, out=wide[1:, 2:2 + F_])
    torch.cuda.synchronize()
    assert res.data_ptr() == wide[1:, 2:2 + F_].data_ptr() and torch.equal(obs, before)
    out = res.cpu().numpy()
    wide[1:, 2:2 + F_] = POISON
    assert bool((wide == POISON).all())
    return out


@pytest.mark.parametrize("k,H1,F_,n_shapes,M,P", CASES)
def test_kernels_are_the_definition(k, H1, F_, n_shapes, M, P):
    points, W, indices, ids, want = case(k, H1, F_, n_shapes, M, P)
    got = abi_call(points, W, indices, ids)
    np.testing.assert_array_equal(got, want)
    assert (got.view(np.uint32)[np.isnan(got)] == 0x7fc00000).all()
    np.testing.assert_array_equal(wrapper_call(points, W, indices, ids), want)
    if M > 1:
        assert np.isnan(want[1]).all() and np.isnan(want[3]).all() and not np.isnan(want[0]).any()


def test_every_activation_negative():
    """b2 strongly negative: every h2 < 0, so a padded lane of the short last chunk (1000 = 15 * 64 + 40) that brought a zero
    point's leaky(b2), or an initial 0, would win the max."""
    points, W, indices, ids, want = case(1000, 20, 40, 7, 5, 50, b2_shift=-40.0)
    assert (want[~np.isnan(want)] < 0).all()
    np.testing.assert_array_equal(abi_call(points, W, indices, ids, expect_chunks=16), want)
    np.testing.assert_array_equal(wrapper_call(points, W, indices, ids, float_ids=False), want)


@pytest.mark.parametrize("at", ["first", "last"])
def test_maximum_in_the_first_and_in_the_last_point(at):
    points, W, indices, ids, base = case(1000, 20, 40, 7, 5, 50, b2_shift=-40.0)
    far = points.copy()
    far[:, 7] = 30.0                                         # a far point that only one position samples
    idx = np.where(indices == 7, 8, indices).astype(np.int32)
    idx[0 if at == "first" else len(idx) - 1] = 7
    want = shape_features_fast_np(far, idx, ids, W)
    other = shape_features_fast_np(far, np.where(idx == 7, 8, idx), ids, W)
    assert (want[0] != other[0]).mean() > 0.25               # the maximum sits in that point for many features
    np.testing.assert_array_equal(abi_call(far, W, idx, ids), want)


def test_the_number_of_chunks_does_not_change_a_bit():
    """The same seven shapes as the head of a table of 300: the library then splits the 1000 points into 6 chunks of three
    trips instead of 16 of one; the shapes beyond the seventh are absent."""
    points, W, indices, ids, want = case(1000, 20, 40, 7, 5, 50, b2_shift=-40.0)
    rng = np.random.default_rng(5)
    more = np.concatenate([points, make_points(rng, 293, points.shape[1])])
    ids300 = np.where(ids == 7, 300, ids)
    a = abi_call(points, W, indices, ids, expect_chunks=16)
    b = abi_call(more, W, indices, ids300, expect_chunks=6)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_array_equal(b, want)
    points, W, indices, ids, want = case(1024, 128, 128, 7, 5, 100000)
    more = np.concatenate([points[:, :2000], make_points(rng, 293, 2000)])
    idx = (indices % 2000).astype(np.int32)
    ids300 = np.where(ids == 7, 300, ids)
    b = abi_call(more, W, idx, ids300, expect_chunks=6)
    np.testing.assert_array_equal(b, shape_features_fast_np(more, idx, ids300, W))
    np.testing.assert_array_equal(b.view(np.uint32), abi_call(np.ascontiguousarray(more[:7]), W, idx, ids, expect_chunks=16).view(np.uint32))


def test_float_id_column_of_an_observation_block():
    points, W, indices, ids, want = case(65, 130, 67, 7, 5, 100000)
    np.testing.assert_array_equal(abi_call(points, W, indices, ids.astype(f32) + np.where(ids >= 0, f32(0.75), f32(0)), float_ids=True), want)
    fids = np.array([0.5, np.nan, np.inf, -np.inf, -1.0, 7.0, 6.99, -0.5], dtype=f32)
    want = shape_features_fast_np(points, indices, fids, W)
    assert np.isnan(want[1:6]).all() and not np.isnan(want[[0, 6, 7]]).any()
    np.testing.assert_array_equal(abi_call(points, W, indices, fids, float_ids=True), want)
    # [B, K] ids of the buffered observation
    sp, w = replay.ShapePoints(points, DEV), weights_of(W, DEV)
    two = torch.from_numpy(ids[:4].reshape(2, 2)).to(DEV)
    got = replay.shape_features(two, sp, torch.from_numpy(indices).to(DEV), w, use_hip=True)
    assert tuple(got.shape) == (4, 67)
    np.testing.assert_array_equal(got.cpu().numpy(), shape_features_fast_np(points, indices, ids[:4], W))


def test_bad_index_and_nan_weight():
    points, W, indices, ids, want = case(65, 130, 67, 7, 5, 100000)
    for wrong in (-1, points.shape[1], 2 ** 31 - 1):
        idx = indices.copy()
        idx[64] = wrong                                      # the one point of the second chunk
        got = abi_call(points, W, idx, ids)
        assert np.isnan(got).all() and (got.view(np.uint32) == 0x7fc00000).all()
    Wn = dict(W, w2=W["w2"].copy())
    Wn["w2"][66, 129] = np.nan
    got = abi_call(points, Wn, indices, ids)
    np.testing.assert_array_equal(got, shape_features_fast_np(points, indices, ids, Wn))
    assert np.isnan(got[:, 66]).all() and not np.isnan(got[0, :66]).any()


@pytest.mark.parametrize("k,H1,F_,n_shapes,M,P", [(1024, 128, 128, 7, 5, 100000), (65, 256, 256, 1, 1, 100000), (1000, 130, 67, 7, 300, 100000)])
def test_torch_formulation_within_the_chains_bound(k, H1, F_, n_shapes, M, P):
    points, W, indices, ids, want = case(k, H1, F_, n_shapes, M, P)
    sp, w = replay.ShapePoints(points, DEV), weights_of(W, DEV)
    got = replay.shape_features(torch.from_numpy(ids).to(DEV), sp, torch.from_numpy(indices).to(DEV), w, use_hip=False).cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    for u in sorted(set(int(i) for i in ids if 0 <= i < n_shapes)):
        bound = shape_bounds(points, indices, u, W)          # each side within it of the exact value
        err = np.abs(got[ids == u].astype(np.float64) - want[ids == u]).max(axis=0)
        print(f"shape {u}: torch on the device against the definition {err.max():.3g}, twice the bound {2 * bound.min():.3g} .. {2 * bound.max():.3g}")
        assert (err <= 2 * bound).all()
    # the gather that feeds the forward with a gradient
    pts = sp.gather(torch.from_numpy(np.where((ids < 0) | (ids >= n_shapes), 0, ids)).to(DEV), torch.from_numpy(indices).to(DEV))
    np.testing.assert_array_equal(pts[0].cpu().numpy(), points[max(int(ids[0]), 0)][indices])
    idx = sp.draw_indices(k)
    assert idx.dtype == torch.int32 and idx.device.type == "cuda" and 0 <= int(idx.min()) and int(idx.max()) < P


@pytest.mark.parametrize("bad", BAD, ids=ids_of)
def test_status_codes_on_the_device(bad):
    L, lib = _lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=DEV)
    ptr = C.c_void_p(buf.data_ptr())
    d = dict(points=ptr, n_shapes=4, n_points=10, indices=ptr, k=100, ids=ptr, ids_are_float=0, ids_stride=1, m_rows=3, w={}, hidden=8, feat=8,
             slope=0.01, partial=ptr, chunks=None, out=ptr, out_stride=8, no_struct=False)
    d.update({k: (C.c_void_p(0) if isinstance(v, C.c_void_p) else v) for k, v in bad.items()})
    ptrs = dict(w1=ptr.value, b1=ptr.value, w2=ptr.value, b2=ptr.value)
    ptrs.update(d["w"])
    enc = replay._IrbppShapeEncoder(ptrs["w1"], ptrs["b1"], ptrs["w2"], ptrs["b2"], d["hidden"], d["feat"], d["slope"])
    chunks = lib.irbpp_shape_features_chunks(d["n_shapes"], d["k"]) if d["chunks"] is None else d["chunks"]
    rc = lib.irbpp_shape_features(d["points"], d["n_shapes"], d["n_points"], d["indices"], d["k"], d["ids"], d["ids_are_float"], d["ids_stride"],
                                  d["m_rows"], None if d["no_struct"] else C.byref(enc), d["partial"], chunks, d["out"], d["out_stride"], None)
    assert rc == -1
    # the device stays usable
    points, W, indices, ids, want = case(1, 5, 3, 1, 1, 1)
    np.testing.assert_array_equal(abi_call(points, W, indices, ids), want)
