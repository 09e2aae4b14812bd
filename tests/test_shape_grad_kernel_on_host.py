"""The source of csrc/irbpp_shapefeat_grad.hip compiled for the host (tests/host/shape_grad_host.cpp: the workgroup's threads
in lockstep, shuffles as real exchanges within a wave, fmaf the C library's) against the definition as replay's CPU form
carries it (replay._shape_grad_forward_np / _shape_grad_backward_np, held to the explicit loops of
tests/test_shape_grad_cpu.py there), bit for bit: the forward's values, the arg record and the four gradients, over short and
whole trips, several chunks and forced splits, every block form of the widths, absent shapes, bad ids, strided float ids, ties
and a bad index, without a GPU.  The same harness as a program of its own under -fsanitize=address,undefined, every buffer
exactly as large as the kernels may touch, runs once here; nothing of it is loaded into Python."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from irbpp_amd import replay
from host_harness import HERE, build_shared
from test_shape_features_cpu import f32, ids_np, make_encoder, make_points
from test_shape_grad_cpu import NAMES, same

SRC = os.path.join(HERE, "host", "shape_grad_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libshape_grad_host.so")
LL = C.c_longlong
POISON = f32(1e30)
VP = C.c_void_p


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_shape_features_arg.argtypes = [VP, C.c_int, C.c_int, VP, C.c_int, VP, C.c_int, LL, LL, VP, C.c_int, C.c_int, C.c_float, VP, VP,
                                            C.c_int, VP, LL, VP]
    lib.host_shape_features_arg.restype = C.c_int
    lib.host_shape_features_backward.argtypes = [VP, C.c_int, C.c_int, VP, C.c_int, VP, C.c_int, LL, LL, VP, C.c_int, C.c_int, C.c_float, VP,
                                                 VP, VP, VP, VP]
    lib.host_shape_features_backward.restype = None
    lib.host_shape_grad_chunks.argtypes = [C.c_int, C.c_int]
    lib.host_shape_grad_chunks.restype = C.c_int
    return lib


def aligned(shape, fill):
    """a float32 array of `shape` on a 16-byte boundary, filled"""
    n = int(np.prod(shape))
    raw = np.empty(n + 4, dtype=f32)
    off = (-raw.ctypes.data % 16) // 4
    a = raw[off:off + n].reshape(shape)
    a[...] = fill
    return a


def definition(points, indices, ids, W, g):
    u = ids_np(ids, points.shape[0])
    idx = np.asarray(indices, np.int64)
    w = [W[n] for n in NAMES]
    out, arg = replay._shape_grad_forward_np(points, idx, u, *w, W["slope"])
    return out, arg, dict(zip(NAMES, replay._shape_grad_backward_np(points, idx, u, *w, W["slope"], arg, g)))


def run(host, points, indices, ids, W, g, *, chunk_points=0, float_ids=False, obs_len=11, pad=5):
    """ids as a strided column of a poisoned [M, obs_len] block, out as a slice of a wider poisoned block, the workspaces and
    the gradients poisoned -> (out, arg, gradients); the surroundings are checked untouched."""
    n_shapes, P = points.shape[:2]
    M, F_, H1, k = len(ids), W["w2"].shape[0], W["w1"].shape[0], len(indices)
    block = np.full((M, obs_len), POISON if float_ids else 999999, dtype=f32 if float_ids else np.int64)
    block[:, 3] = ids
    before = block.copy()
    wide = np.full((M + 2, F_ + pad), POISON, dtype=f32)
    chunks = -(-k // chunk_points) if chunk_points else host.host_shape_grad_chunks(n_shapes, k)
    pkey, pj = np.full((n_shapes, chunks, F_), 0x12345678, dtype=np.uint32), np.full((n_shapes, chunks, F_), 7777, dtype=np.int32)
    arg = np.full((n_shapes, F_), 7777, dtype=np.int32)
    w = [np.ascontiguousarray(W[n]) for n in NAMES]
    wp = (VP * 4)(*(a.ctypes.data for a in w))
    idx = np.ascontiguousarray(indices, dtype=np.int32)
    ids_ptr = block.ctypes.data + 3 * block.itemsize
    got = host.host_shape_features_arg(points.ctypes.data, n_shapes, P, idx.ctypes.data, k, ids_ptr, int(float_ids), obs_len, M, wp, H1, F_,
                                       W["slope"], pkey.ctypes.data, pj.ctypes.data, chunk_points, wide.ctypes.data + (F_ + pad + 2) * 4,
                                       F_ + pad, arg.ctypes.data)
    assert got == chunks
    out = wide[1:1 + M, 2:2 + F_].copy()
    wide[1:1 + M, 2:2 + F_] = POISON
    assert (wide == POISON).all()
    present = set(ids_np(ids, n_shapes).tolist())
    for u in range(n_shapes):                                # a shape that does not occur: -1, and nothing of its keys written
        assert (arg[u] == -1).all() == (u not in present) and (pkey[u] == 0x12345678).all() == (u not in present), u
    pd, first = aligned((n_shapes, F_, 4), POISON), aligned((n_shapes, H1, 4), POISON)
    d = [np.full(a.shape, POISON, dtype=f32) for a in w]
    dp = (VP * 4)(*(a.ctypes.data for a in d))
    gg = np.ascontiguousarray(g, dtype=f32)
    host.host_shape_features_backward(points.ctypes.data, n_shapes, P, idx.ctypes.data, k, ids_ptr, int(float_ids), obs_len, M, wp, H1, F_,
                                      W["slope"], arg.ctypes.data, gg.ctypes.data, pd.ctypes.data, first.ctypes.data, dp)
    np.testing.assert_array_equal(block, before)
    for u in range(n_shapes):
        assert (pd[u] == POISON).all() == (u not in present) and (first[u] == POISON).all() == (u not in present), u
    return out, arg, dict(zip(NAMES, d))


def check(got, want):
    same(got[0], want[0], "forward")
    assert (got[0].view(np.uint32)[np.isnan(got[0])] == 0x7fc00000).all()
    np.testing.assert_array_equal(got[1], want[1])
    for n in NAMES:
        same(got[2][n], want[2][n], n)


# (n_shapes, P, k, H1, F, M): around one wave of points and three chunks, every block form of the features and the hidden units
HOST_CASES = [(1, 1, 1, 1, 1, 1), (5, 70, 63, 16, 32, 7), (5, 70, 64, 17, 33, 7), (5, 70, 65, 128, 128, 7), (5, 70, 130, 17, 33, 200),
              (2, 30, 65, 256, 256, 7), (300, 6, 200, 5, 3, 70)]


def make_ids(rng, n_shapes, M):
    ids = rng.integers(0, min(n_shapes, 7), M).astype(np.int64)
    if n_shapes > 2:
        ids[ids == 2] = 3                                    # shape 2 stays absent
    if M >= 5:
        ids[1], ids[3] = -1, n_shapes
    return ids


@pytest.mark.parametrize("n_shapes,P,k,H1,F_,M", HOST_CASES)
def test_shape_grad_source_on_host(host, n_shapes, P, k, H1, F_, M):
    rng = np.random.default_rng(500 + k + F_)
    points = make_points(rng, n_shapes, P)
    W = make_encoder(rng, H1, F_)
    indices = rng.integers(0, P, k).astype(np.int32)
    indices[0], indices[-1] = P - 1, 0
    if k > 4:
        indices[2] = indices[3]                              # a duplicate for certain
    ids = make_ids(rng, n_shapes, M)
    g = rng.standard_normal((M, F_)).astype(f32)
    want = definition(points, indices, ids, W, g)
    check(run(host, points, indices, ids, W, g), want)
    fids = ids.astype(f32) + np.where(ids >= 0, f32(0.75), f32(0))
    check(run(host, points, indices, fids, W, g, float_ids=True), want)
    for cp in (64, 4096):                                    # another split of the points: the same bits
        check(run(host, points, indices, ids, W, g, chunk_points=cp), want)


def test_ties_negative_activations_bad_ids_and_a_bad_index_on_host(host):
    rng = np.random.default_rng(78)
    n_shapes, P, k, H1, F_, M = 3, 50, 130, 20, 40, 9
    points = make_points(rng, n_shapes, P)
    points[0, 7] = points[0, 9]                              # two rows of the table with the same coordinates: exact ties
    W = make_encoder(rng, H1, F_, b2_shift=-40.0)            # every s2 negative: the slope side of d2 everywhere
    indices = rng.integers(0, P, k).astype(np.int32)
    indices[[5, 70, 129]] = [9, 7, 9]
    ids = np.array([0, 2, 0, 0, 2, 0, 2, 2, 0], dtype=np.int64)
    g = rng.standard_normal((M, F_)).astype(f32)
    want = definition(points, indices, ids, W, g)
    assert (want[0] < 0).all() and (want[1][1] == -1).all()
    check(run(host, points, indices, ids, W, g), want)
    for cp in (64, 128):
        check(run(host, points, indices, ids, W, g, chunk_points=cp), want)
    # a far point only positions 70 (the second chunk of three) and 129 sample, twice over: many maxima sit there, at 70
    far = points.copy()
    far[:, 7] = far[:, 9] = 30.0
    idx = np.where((indices == 7) | (indices == 9), 8, indices).astype(np.int32)
    idx[[70, 129]] = [9, 7]
    want = definition(far, idx, ids, W, g)
    assert (want[1][0] == 70).mean() > 0.25 and not (want[1] == 129).any()
    check(run(host, far, idx, ids, W, g), want)
    fids = np.array([0.5, np.nan, np.inf, -np.inf, -1.0, 3.0, 2.99, -0.5, 0.0], dtype=f32)
    want = definition(points, indices, fids, W, g)
    assert (want[1][1] == -1).all() and (want[1][[0, 2]] >= 0).all()
    check(run(host, points, indices, fids, W, g, float_ids=True), want)
    for wrong in (-1, P, 2 ** 31 - 1, -2 ** 31):
        idx = indices.copy()
        idx[k - 1] = wrong
        want = definition(points, idx, ids, W, g)
        assert (want[1][[0, 2]] == k - 1).all() and np.isnan(want[2]["w2"]).all()
        check(run(host, points, idx, ids, W, g), want)


def test_harness_runs_clean_under_the_sanitizers(tmp_path):
    """A program of its own (never loaded into Python): address and undefined-behaviour sanitizers over the kernels' source."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "shape_grad_host_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DSHAPE_GRAD_HOST_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and "checksum" in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr
