"""The source of csrc/irbpp_dueling_loss.hip compiled for the host (tests/host/dueling_loss_host.cpp: 512 threads in lockstep per
workgroup, barriers as real barriers, the backward kernel's two-dimensional grid) against the numpy float32 definition of
tests/test_dueling_loss_cpu.py, bit for bit and without a GPU: the column means from strided memory, the action's row, the
logarithm, the out-of-range rule, and the stepped stores of the backward kernel with either output missing.  Poison lies
around every output and around the strided `v` and `a`.  Same case builder as tests/test_gpu_dueling_loss.py, with batches
of 1 to 3 (a workgroup costs 512 host threads here); the seeds bring every action kind, every kind of m and the logits that
zero most e into those few samples."""
import ctypes as C
import os

import numpy as np
import pytest

from host_harness import build_shared
import test_gpu_dueling_loss as G
from test_dueling_kernel_on_host import _at, wide_a, wide_v
from test_dueling_loss_cpu import dlog_np, dueling_loss_backward_np, dueling_loss_np, f32

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "dueling_loss_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libdueling_loss_host.so")
LL = C.c_longlong


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_dueling_loss_chunk_rows.restype = C.c_int
    lib.host_dueling_dlog.argtypes = [C.c_float]
    lib.host_dueling_dlog.restype = C.c_float
    lib.host_dueling_loss.argtypes = [C.c_void_p, LL, C.c_void_p, LL, LL, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]
    lib.host_dueling_loss.restype = None
    lib.host_dueling_loss_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.host_dueling_loss_backward.restype = None
    return lib


def test_dlog_source_on_host(host):
    """dueling_dlog as compiled from the kernel's file against dlog_np: the ends, the powers of two, both sides of every
    mantissa fold, and 4096 arguments spread over the bit patterns of [1, 128]."""
    lo, hi = int(f32(1.0).view(np.uint32)), int(f32(128.0).view(np.uint32))
    bits = [np.linspace(lo, hi, 4096).astype(np.int64)]
    for k in range(7):
        fold = int((f32(1.4142135623730951) * f32(2.0 ** k)).view(np.uint32))
        bits.append(np.arange(fold - 4, fold + 5))
        bits.append(np.arange(max(lo, int(f32(2.0 ** k).view(np.uint32)) - 2), int(f32(2.0 ** k).view(np.uint32)) + 3))
    d = np.concatenate(bits).astype(np.uint32).view(f32)
    got = np.array([host.host_dueling_dlog(float(x)) for x in d], dtype=f32)
    G.same_bits(got, dlog_np(d), "dlog")
    assert host.host_dueling_dlog(1.0) == 0.0


# (S, atoms, b, seed): every shape of the GPU test; the seeds walk the scenarios of loss_case through the few samples
HOST_CASES = [(1, 2, 3, 0), (1, 2, 2, 3), (3, 2, 3, 2), (15, 31, 2, 1), (16, 31, 3, 4), (17, 31, 3, 0), (33, 51, 2, 3), (500, 31, 2, 2),
              (500, 31, 1, 6), (1024, 128, 1, 2), (1024, 128, 1, 1)]


def test_the_cases_cover_what_they_are_meant_to(host):
    assert host.host_dueling_loss_chunk_rows() == 64
    kinds, m_kinds, scaled, zero_w = set(), set(), 0, 0
    for s, atoms, b, seed in HOST_CASES:
        assert 1 <= b <= 3
        for k in range(b):
            i = k + seed
            kinds.add(i % 5)
            m_kinds.add(i % 3)
            scaled += i % 4 == 2
            zero_w += i % 7 == 6
    assert kinds == {0, 1, 2, 3, 4} and m_kinds == {0, 1, 2} and scaled >= 3 and zero_w >= 1
    assert {(s, a) for s, a, _, _ in HOST_CASES} == set(G.SHAPES)


@pytest.mark.parametrize("s,atoms,b,seed", HOST_CASES)
def test_loss_and_backward_source_on_host(host, s, atoms, b, seed):
    v, a, actions, m, w = G.loss_case(b, s, atoms, seed)
    want_loss, want_g = dueling_loss_np(v, a, actions, m)
    want_gv, want_ga = dueling_loss_backward_np(want_g, w, actions, s)
    keep_a, a_ptr, env_stride, row_stride = wide_a(a, 3, 2, 3)
    keep_v, v_ptr, v_stride = wide_v(v)
    loss = np.full(b + 2, -5.0, dtype=f32)
    g = np.full((b + 2, atoms), -5.0, dtype=f32)
    host.host_dueling_loss(v_ptr, v_stride, a_ptr, env_stride, row_stride, actions.ctypes.data, m.ctypes.data, atoms, s, b,
                           _at(loss, 1), _at(g, 1, 0))
    assert loss[0] == -5.0 and loss[b + 1] == -5.0 and (g[0] == -5.0).all() and (g[b + 1] == -5.0).all()
    G.same_bits(loss[1:b + 1], want_loss, "loss")
    G.same_bits(g[1:b + 1], want_g, "g")
    bad = (actions >= s) | (actions < -s)
    assert np.isnan(loss[1:b + 1][bad]).all() and np.isfinite(loss[1:b + 1][~bad]).all()
    if ((np.arange(b) + seed) % 4 == 2).any() and atoms > 2:
        scaled = (np.arange(b) + seed) % 4 == 2
        assert (want_g[scaled & ~bad] == -m[scaled & ~bad]).mean() > 0.5 or (scaled & ~bad).sum() == 0, \
            "the large logits are meant to drive most e (and p) to exactly 0"
    gin = np.ascontiguousarray(g[1:b + 1])
    for with_v, with_a in ((True, True), (True, False), (False, True)):
        gv = np.full((b + 2, atoms), -5.0, dtype=f32)
        ga = np.full(b * s * atoms + 8, -5.0, dtype=f32)
        host.host_dueling_loss_backward(gin.ctypes.data, w.ctypes.data, actions.ctypes.data, atoms, s, b,
                                        _at(gv, 1, 0) if with_v else None, _at(ga, 4) if with_a else None)
        assert (gv[0] == -5.0).all() and (gv[b + 1] == -5.0).all() and (ga[:4] == -5.0).all() and (ga[-4:] == -5.0).all()
        if with_v:
            G.same_bits(gv[1:b + 1], want_gv, "grad_v")
        else:
            assert (gv == -5.0).all()
        if with_a:
            G.same_bits(ga[4:-4].reshape(b, s, atoms), want_ga, "grad_a")
        else:
            assert (ga == -5.0).all()
