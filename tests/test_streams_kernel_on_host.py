"""The source of csrc/irbpp_streams.hip compiled for the host (tests/host/streams_host.cpp: 512 threads in lockstep per
workgroup; barriers and shuffles as real exchanges; fmaf the C library's) against the numpy definition of
tests/test_streams_cpu.py, bit for bit: the chains, the blocks of hidden units, both instantiations, the staging, masking and
tie rules, and both sides of the LDS threshold (the second launch included) without a GPU.  Same input builder and strided
layouts as tests/test_gpu_streams.py, with one to three workgroups (one costs 512 host threads here)."""
import ctypes as C
import os

import numpy as np
import pytest

from host_harness import build_shared
import test_gpu_streams as G
from test_streams_cpu import NAMES, f32

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "streams_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libstreams_host.so")
LL = C.c_longlong


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_streams_act.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, LL, C.c_void_p, LL, LL, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, LL, C.c_void_p, C.c_void_p, C.c_int]
    lib.host_streams_act.restype = C.c_int
    lib.host_noisy_weights.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.host_noisy_weights.restype = None
    return lib


def _at(a, *idx):
    return C.c_void_p(a.ctypes.data + int(np.ravel_multi_index(idx, a.shape)) * a.itemsize)


# (S, E, H, atoms, n): the GPU test's shapes with fewer envs where the rows are many
HOST_CASES = [(1, 5, 3, 2, 3), (2, 130, 67, 31, 3), (63, 128, 128, 31, 1), (64, 5, 3, 51, 3), (65, 256, 256, 31, 2), (500, 128, 128, 31, 1),
              (600, 130, 67, 51, 1), (65, 130, 67, 128, 2), (64, 128, 128, 2, 3), (1024, 5, 3, 128, 3), (500, 16, 17, 128, 2)]


@pytest.mark.parametrize("s,E,H,atoms,n", HOST_CASES)
def test_streams_source_on_host(host, s, E, H, atoms, n):
    z = G.support_np(atoms)
    _, W, xg, x, flags, (want_act, want_q, want_v, want_a), want_free = G.stream_case(s, E, H, atoms, n)
    w = [np.ascontiguousarray(W[k]) for k in NAMES]
    wp = (C.c_void_p * 8)(*(a.ctypes.data for a in w))
    fits = s * (atoms | 1) * 4 <= G.TILE_BYTES
    obs = np.full((n, s * 5 + 9), 3.0, dtype=f32)
    obs[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
    wide_g = np.full((n, E + 7), G.POISON, dtype=f32)
    wide_g[:, 3:3 + E] = xg
    for front, with_all, generic in ((4, True, 0), (1, False, 0), (4, True, 1)):
        if generic and atoms > 32:
            continue                                         # already the 128-accumulator instantiation
        wide = np.full((n, s + 3, E + 8), G.POISON, dtype=f32)
        wide[:, 1:1 + s, front:front + E] = x
        act = np.full(n + 1, -7, dtype=np.int64)
        q = np.full((n, s + 2), -5.0, dtype=f32)
        v = np.full(n * atoms + 4, -5.0, dtype=f32)
        a = np.full(n * s * atoms + 4, -5.0, dtype=f32)
        rc = host.host_streams_act(wp, E, H, atoms, _at(wide_g, 0, 3), E + 7, _at(wide, 0, 1, front), (s + 3) * (E + 8), E + 8,
                                   z.ctypes.data, obs.ctypes.data if with_all else None, s * 5 + 9, s, n, act.ctypes.data,
                                   q.ctypes.data if with_all else None, s + 2, v.ctypes.data if with_all else None,
                                   a.ctypes.data if with_all or not fits else None, generic)
        assert rc == 0 and act[n] == -7
        if with_all:
            assert (q[:, s:] == -5.0).all() and (v[n * atoms:] == -5.0).all() and (a[n * s * atoms:] == -5.0).all()
            np.testing.assert_array_equal(v[:n * atoms].reshape(n, atoms), want_v)
            np.testing.assert_array_equal(a[:n * s * atoms].reshape(n, s, atoms), want_a)
            np.testing.assert_array_equal(q[:, :s], want_q)
            np.testing.assert_array_equal(act[:n], want_act)
        else:
            assert (q == -5.0).all() and (v == -5.0).all()
            np.testing.assert_array_equal(act[:n], want_free)
    front = 4
    wide = np.full((n, s + 3, E + 8), G.POISON, dtype=f32)
    wide[:, 1:1 + s, front:front + E] = x
    if not fits:
        assert host.host_streams_act(wp, E, H, atoms, _at(wide_g, 0, 3), E + 7, _at(wide, 0, 1, front), (s + 3) * (E + 8), E + 8,
                                     z.ctypes.data, None, 0, s, n, act.ctypes.data, None, 0, None, None, 0) == -1
    # logits only: no action, no q_out
    v[:], a[:] = -5.0, -5.0
    assert host.host_streams_act(wp, E, H, atoms, _at(wide_g, 0, 3), E + 7, _at(wide, 0, 1, front), (s + 3) * (E + 8), E + 8, None, None, 0,
                                 s, n, None, None, 0, v.ctypes.data, a.ctypes.data, 0) == 0
    np.testing.assert_array_equal(v[:n * atoms].reshape(n, atoms), want_v)
    np.testing.assert_array_equal(a[:n * s * atoms].reshape(n, s, atoms), want_a)


def test_noisy_weights_source_on_host(host):
    rng = np.random.default_rng(2)
    out, inp = 67, 130
    t = [rng.standard_normal((out, inp)).astype(f32) for _ in range(3)] + [rng.standard_normal(out).astype(f32) for _ in range(3)]
    w = np.full(out * inp + 3, -5.0, dtype=f32)
    b = np.full(out + 3, -5.0, dtype=f32)
    host.host_noisy_weights(*(a.ctypes.data for a in t), out, inp, w.ctypes.data, b.ctypes.data)
    assert (w[out * inp:] == -5.0).all() and (b[out:] == -5.0).all()
    np.testing.assert_array_equal(w[:out * inp].reshape(out, inp), t[0] + t[1] * t[2])
    np.testing.assert_array_equal(b[:out], t[3] + t[4] * t[5])
