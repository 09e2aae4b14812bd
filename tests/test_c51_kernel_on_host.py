"""The source of csrc/irbpp_c51.hip compiled for the host (tests/host/c51_host.cpp: 64 threads in lockstep per workgroup,
barriers and shuffles as real exchanges) against the numpy float32 definition of tests/test_c51_cpu.py, bit for bit: the
kernels' staging, indexing, masking, tie rules and scatter order without a GPU.  Same input builders and strided layouts as
tests/test_gpu_c51.py, on the small end of its shapes (a workgroup costs 64 host threads here)."""
import ctypes as C
import os

import numpy as np
import pytest

from host_harness import build_shared
import test_gpu_c51 as G
from test_c51_cpu import EPS, act_np, target_np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "c51_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libc51_host.so")
f32 = np.float32
fp, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_c51_act.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_longlong]
    lib.host_c51_act.restype = None
    lib.host_c51_target.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.c_void_p, C.c_void_p]
    lib.host_c51_target.restype = None
    return lib


def _at(a, *idx):
    """address of a[idx] of a C-contiguous array"""
    return C.c_void_p(a.ctypes.data + int(np.ravel_multi_index(idx, a.shape)) * a.itemsize)


ACT_CASES = [c for c in G.ACT_CASES if c[2] <= 5] + [(65, 51, 70, True, True, 2)]


@pytest.mark.parametrize("s,atoms,n,with_obs,with_q,shift", ACT_CASES)
def test_act_source_on_host(host, s, atoms, n, with_obs, with_q, shift):
    z = G._support(atoms).numpy()
    p, flags, _ = G.act_inputs(s, atoms, n, shift)
    want_a, want_q = act_np(p, z, flags if with_obs else None)
    wide = np.full((n, s + 3, atoms + 5), G.POISON, dtype=f32)
    wide[:, 1:1 + s, 2:2 + atoms] = p
    obs = np.full((n, s * 5 + 9), 3.0, dtype=f32)
    obs[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
    act = np.full(n + 1, -7, dtype=np.int64)
    q = np.full((n, s + 2), -5.0, dtype=f32)
    host.host_c51_act(_at(wide, 0, 1, 2), (s + 3) * (atoms + 5), atoms + 5, z.ctypes.data, atoms,
                      obs.ctypes.data if with_obs else None, s * 5 + 9, s, n, act.ctypes.data,
                      q.ctypes.data if with_q else None, s + 2)
    assert act[n] == -7
    np.testing.assert_array_equal(act[:n], want_a)
    if with_q:
        assert (q[:, s:] == -5.0).all()
        np.testing.assert_array_equal(q[:, :s], want_q)
    else:
        assert (q == -5.0).all()


TARGET_CASES = [c for c in G.TARGET_CASES if c[0] <= 4] + [(16, 65, 51, True, 0), (16, 130, 128, False, 3), (9, 3, 2, True, 0)]


@pytest.mark.parametrize("b,s,atoms,dyadic,shift", TARGET_CASES)
@pytest.mark.parametrize("gamma_n", [0.99 ** 3, 0.0])
def test_target_source_on_host(host, b, s, atoms, dyadic, shift, gamma_n):
    v_min = -2.0
    v_max = v_min + 0.25 * (atoms - 1) if dyadic else 7.0
    delta_z = (v_max - v_min) / (atoms - 1)
    z = G._support(atoms, v_min, v_max).numpy()
    p_on, p_tg, returns, nonterm, _ = G.target_inputs(b, s, atoms, z, v_min, v_max, shift)
    want_m, want_a = target_np(p_on, p_tg, returns, nonterm, z, gamma_n, v_min, v_max, delta_z)
    on = np.full((b, s + 2, atoms + 3), G.POISON, dtype=f32)
    on[:, :s, 3:] = p_on
    tg = np.full((b, s + 1, atoms + 6), G.POISON, dtype=f32)
    tg[:, :s, 6:] = p_tg
    m = np.full((b + 1, atoms), -5.0, dtype=f32)
    a = np.full(b + 1, -7, dtype=np.int64)
    host.host_c51_target(_at(on, 0, 0, 3), (s + 2) * (atoms + 3), atoms + 3, _at(tg, 0, 0, 6), (s + 1) * (atoms + 6), atoms + 6,
                         returns.ctypes.data, nonterm.ctypes.data, z.ctypes.data, atoms, s, b, gamma_n, v_min, v_max, delta_z,
                         m.ctypes.data, a.ctypes.data)
    assert a[b] == -7 and (m[b] == -5.0).all()
    np.testing.assert_array_equal(a[:b], want_a)
    np.testing.assert_array_equal(m[:b], want_m)
    pns_a = p_tg[np.arange(b), want_a].astype(np.float64)
    assert np.abs(m[:b].astype(np.float64).sum(1) - pns_a.sum(1)).max() <= 2 * atoms * EPS
