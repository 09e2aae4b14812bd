"""The source of csrc/irbpp_dueling.hip compiled for the host (tests/host/dueling_host.cpp: 512 threads in lockstep per
workgroup, as many as the workgroup has; barriers and shuffles as real exchanges) against the numpy float32 definition of
tests/test_dueling_cpu.py, bit for bit: the kernels' staging, column sums, row loop, masking, tie rules, both forms (block
resident in the tile / staged in chunks of 256 rows) and the scatter order without a GPU.  Same input builders and strided
layouts as tests/test_gpu_dueling.py, with few workgroups (one costs 512 host threads here)."""
import ctypes as C
import os

import numpy as np
import pytest

from host_harness import build_shared
import test_gpu_dueling as G
from test_dueling_cpu import dueling_act_np, dueling_target_np, f32

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "dueling_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libdueling_host.so")
LL = C.c_longlong


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_dueling_tile_rows.argtypes = [C.c_int, C.c_int]
    lib.host_dueling_tile_rows.restype = C.c_int
    lib.host_dueling_act.argtypes = [C.c_void_p, LL, C.c_void_p, LL, LL, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, LL, C.c_void_p]
    lib.host_dueling_act.restype = None
    lib.host_dueling_target.argtypes = [C.c_void_p, LL, C.c_void_p, LL, LL, C.c_void_p, LL, C.c_void_p, LL, LL, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                        C.c_void_p]
    lib.host_dueling_target.restype = None
    return lib


def _at(a, *idx):
    """address of a[idx] of a C-contiguous array"""
    return C.c_void_p(a.ctypes.data + int(np.ravel_multi_index(idx, a.shape)) * a.itemsize)


def test_the_threshold_is_where_the_gpu_test_says(host):
    for s, atoms in G.RESIDENT:
        assert host.host_dueling_tile_rows(s, atoms) == s
    for s, atoms in G.STAGED:
        assert host.host_dueling_tile_rows(s, atoms) == 256
    assert host.host_dueling_tile_rows(285, 128) == 285 and host.host_dueling_tile_rows(286, 128) == 256


def wide_a(a, pad_rows, front, back):
    n, s, atoms = a.shape
    wide = np.full((n, s + pad_rows, atoms + front + back), G.POISON, dtype=f32)
    wide[:, 1:1 + s, front:front + atoms] = a
    return wide, _at(wide, 0, 1, front), (s + pad_rows) * (atoms + front + back), atoms + front + back


def wide_v(v):
    wide = np.full((v.shape[0], v.shape[1] + 7), G.POISON, dtype=f32)
    wide[:, 3:3 + v.shape[1]] = v
    return wide, _at(wide, 0, 3), v.shape[1] + 7


# (S, atoms, n, seed): every shape of the GPU test once, 286 x 128 just past the threshold (two trips, the second short), and
# seeds that bring scenarios 3..5 (masked best row, huge logits) into few envs
HOST_CASES = [(1, 2, 3, 0), (3, 2, 3, 3), (63, 31, 1, 1), (64, 31, 1, 0), (65, 31, 3, 2), (500, 31, 2, 0), (500, 31, 1, 4), (600, 5, 1, 0), (129, 128, 1, 1),
              (286, 128, 1, 0), (1024, 128, 1, 4)]


@pytest.mark.parametrize("s,atoms,n,seed", HOST_CASES)
def test_act_source_on_host(host, s, atoms, n, seed):
    z = G.support_np(atoms)
    v, a, flags, _ = G.head_case(s, atoms, n, seed)
    keep_a, a_ptr, env_stride, row_stride = wide_a(a, 3, 2, 3)
    keep_v, v_ptr, v_stride = wide_v(v)
    obs = np.full((n, s * 5 + 9), 3.0, dtype=f32)
    obs[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
    for with_all in (True, False):
        want_a, want_q, want_p = dueling_act_np(v, a, z, flags if with_all else None)
        act = np.full(n + 1, -7, dtype=np.int64)
        q = np.full((n, s + 2), -5.0, dtype=f32)
        p = np.full(n * s * atoms + 4, -5.0, dtype=f32)
        host.host_dueling_act(v_ptr, v_stride, a_ptr, env_stride, row_stride, z.ctypes.data, atoms, obs.ctypes.data if with_all else None,
                              s * 5 + 9, s, n, act.ctypes.data, q.ctypes.data if with_all else None, s + 2,
                              p.ctypes.data if with_all else None)
        assert act[n] == -7
        np.testing.assert_array_equal(act[:n], want_a)
        if with_all:
            assert (q[:, s:] == -5.0).all() and (p[n * s * atoms:] == -5.0).all()
            np.testing.assert_array_equal(p[:n * s * atoms].reshape(n, s, atoms), want_p)
            np.testing.assert_array_equal(q[:, :s], want_q)
        else:
            assert (q == -5.0).all() and (p == -5.0).all()


@pytest.mark.parametrize("s,atoms,b,seed", HOST_CASES)
def test_target_source_on_host(host, s, atoms, b, seed):
    z = G.support_np(atoms)
    delta_z = (G.V_MAX - G.V_MIN) / (atoms - 1)
    v_on, a_on, v_tg, a_tg, returns, nonterm = G.target_case(b, s, atoms, z, seed)
    keep1, on_ptr, on_env, on_row = wide_a(a_on, 2, 3, 0)
    keep2, tg_ptr, tg_env, tg_row = wide_a(a_tg, 1, 6, 1)
    keep3, von_ptr, von_stride = wide_v(v_on)
    keep4, vtg_ptr, vtg_stride = wide_v(v_tg)
    for gamma_n in (G.GAMMA_N, 0.0):
        want_m, want_a = dueling_target_np(v_on, a_on, v_tg, a_tg, returns, nonterm, z, gamma_n, G.V_MIN, G.V_MAX, delta_z)
        m = np.full((b + 1, atoms), -5.0, dtype=f32)
        a_star = np.full(b + 1, -7, dtype=np.int64)
        host.host_dueling_target(von_ptr, von_stride, on_ptr, on_env, on_row, vtg_ptr, vtg_stride, tg_ptr, tg_env, tg_row,
                                 returns.ctypes.data, nonterm.ctypes.data, z.ctypes.data, atoms, s, b, gamma_n, G.V_MIN, G.V_MAX,
                                 delta_z, m.ctypes.data, a_star.ctypes.data)
        assert a_star[b] == -7 and (m[b] == -5.0).all()
        np.testing.assert_array_equal(a_star[:b], want_a)
        np.testing.assert_array_equal(m[:b], want_m)
