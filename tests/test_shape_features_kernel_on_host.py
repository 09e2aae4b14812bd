"""The source of csrc/irbpp_shapefeat.hip compiled for the host (tests/host/shapefeat_host.cpp: the workgroup's threads in
lockstep, shuffles as real exchanges within a wave, fmaf the C library's) against the numpy definition of
tests/test_shape_features_cpu.py, bit for bit: the chains, the blocks of features and hidden units, short and whole trips,
chunks, the keys of the max, the id rules and the strided arguments, without a GPU.  The same harness as a program of its own
under -fsanitize=address,undefined, every buffer exactly as large as the kernels may touch, runs once here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from host_harness import HERE, build_shared
from test_shape_features_cpu import f32, ids_np, make_encoder, make_points, shape_features_fast_np

SRC = os.path.join(HERE, "host", "shapefeat_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libshapefeat_host.so")
LL = C.c_longlong
POISON = f32(1e30)


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_shape_features.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, LL, LL, C.c_void_p, C.c_int,
                                        C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, LL]
    lib.host_shape_features.restype = C.c_int
    lib.host_shape_chunks.argtypes = [C.c_int, C.c_int]
    lib.host_shape_chunks.restype = C.c_int
    return lib


def run(host, points, indices, ids, W, *, chunk_points=0, float_ids=False, obs_len=11, pad=5):
    """ids as a strided column of a poisoned [M, obs_len] block, out as a slice of a wider poisoned block, the workspace
    poisoned: -> out [M, F]; the surroundings are checked untouched."""
    n_shapes, P = points.shape[:2]
    M, F_, H1 = len(ids), W["w2"].shape[0], W["w1"].shape[0]
    block = np.full((M, obs_len), POISON if float_ids else 999999, dtype=f32 if float_ids else np.int64)
    block[:, 3] = ids
    before = block.copy()
    wide = np.full((M + 2, F_ + pad), POISON, dtype=f32)
    k = len(indices)
    chunks = -(-k // chunk_points) if chunk_points else host.host_shape_chunks(n_shapes, k)
    partial = np.full((n_shapes, chunks, F_), POISON, dtype=f32)
    w = [np.ascontiguousarray(W[n]) for n in ("w1", "b1", "w2", "b2")]
    wp = (C.c_void_p * 4)(*(a.ctypes.data for a in w))
    idx = np.ascontiguousarray(indices, dtype=np.int32)
    got = host.host_shape_features(points.ctypes.data, n_shapes, P, idx.ctypes.data, k, block.ctypes.data + 3 * block.itemsize, int(float_ids),
                                   obs_len, M, wp, H1, F_, W["slope"], partial.ctypes.data, chunk_points, wide.ctypes.data + (F_ + pad + 2) * 4,
                                   F_ + pad)
    assert got == chunks
    np.testing.assert_array_equal(block, before)
    out = wide[1:1 + M, 2:2 + F_].copy()
    wide[1:1 + M, 2:2 + F_] = POISON
    assert (wide == POISON).all()
    present = set(ids_np(ids, n_shapes).tolist())
    for u in range(n_shapes):                                # a shape that does not occur: its rows were never written
        assert (partial[u] == POISON).all() == (u not in present), u
    return out


# (n_shapes, P, k, H1, F, M): around one wave of points, every block form of the features and the hidden units
HOST_CASES = [(1, 1, 1, 5, 3, 1), (7, 30, 63, 128, 128, 5), (7, 30, 64, 5, 3, 5), (7, 30, 65, 130, 67, 5), (1, 30, 65, 256, 256, 1),
              (7, 100, 200, 16, 33, 300), (300, 6, 200, 5, 3, 5)]


@pytest.mark.parametrize("n_shapes,P,k,H1,F_,M", HOST_CASES)
def test_shape_features_source_on_host(host, n_shapes, P, k, H1, F_, M):
    rng = np.random.default_rng(900 + k + F_)
    points = make_points(rng, n_shapes, P)
    W = make_encoder(rng, H1, F_)
    indices = rng.integers(0, P, k).astype(np.int32)
    indices[0], indices[-1] = P - 1, 0
    ids = rng.integers(0, min(n_shapes, 7), M).astype(np.int64)
    if n_shapes > 1:
        ids[ids == 2] = 3                                    # shape 2 stays absent
    if M >= 5:
        ids[1], ids[3] = -1, n_shapes
    want = shape_features_fast_np(points, indices, ids, W)
    np.testing.assert_array_equal(run(host, points, indices, ids, W), want)
    fids = ids.astype(f32) + np.where(ids >= 0, f32(0.75), f32(0))
    np.testing.assert_array_equal(run(host, points, indices, fids, W, float_ids=True), want)
    # another split of the points: the same bits
    for cp in (64, 128, 4096):
        got = run(host, points, indices, ids, W, chunk_points=cp)
        np.testing.assert_array_equal(got, want)
        assert (got.view(np.uint32)[np.isnan(got)] == 0x7fc00000).all()


def test_negative_activations_extremes_and_nans_on_host(host):
    """Every h2 negative (a padded lane's zero point or an initial 0 would win the max), the maximum in the first and in the
    last point of a short last chunk, float ids that are no ids, a bad index, a NaN weight."""
    rng = np.random.default_rng(77)
    n_shapes, P, k, H1, F_ = 3, 50, 100, 20, 40
    points = make_points(rng, n_shapes, P)
    W = make_encoder(rng, H1, F_, b2_shift=-40.0)
    indices = rng.integers(1, P - 1, k).astype(np.int32)
    ids = np.array([0, 2, 0], dtype=np.int64)
    want = shape_features_fast_np(points, indices, ids, W)
    assert (want < 0).all()
    np.testing.assert_array_equal(run(host, points, indices, ids, W), want)
    for at in (0, k - 1):                                    # a far point only this position samples
        far = points.copy()
        far[:, 0] = 30.0
        idx = indices.copy()
        idx[at] = 0
        want = shape_features_fast_np(far, idx, ids, W)
        assert (want != shape_features_fast_np(far, indices, ids, W)).mean() > 0.25       # the maximum sits there for many features
        np.testing.assert_array_equal(run(host, far, idx, ids, W), want)
    fids = np.array([0.5, np.nan, np.inf, -np.inf, -1.0, 3.0, 2.99, -0.5], dtype=f32)
    want = shape_features_fast_np(points, indices, fids, W)
    assert np.isnan(want[1:6]).all() and not np.isnan(want[[0, 6, 7]]).any()
    np.testing.assert_array_equal(run(host, points, indices, fids, W, float_ids=True), want)
    for wrong in (-1, P, 2 ** 31 - 1, -2 ** 31):
        idx = indices.copy()
        idx[k - 1] = wrong
        assert np.isnan(run(host, points, idx, ids, W)).all()
    Wn = dict(W, w2=W["w2"].copy())
    Wn["w2"][33, 7] = np.nan
    got = run(host, points, indices, ids, Wn)
    np.testing.assert_array_equal(got, shape_features_fast_np(points, indices, ids, Wn))
    assert np.isnan(got[:, 33]).all() and not np.isnan(np.delete(got, 33, axis=1)).any()


def test_harness_runs_clean_under_the_sanitizers(tmp_path):
    """A program of its own (never loaded into Python): address and undefined-behaviour sanitizers over the kernels' source."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "shapefeat_host_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DSHAPEFEAT_HOST_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and "checksum" in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr
