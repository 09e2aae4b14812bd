"""The source of csrc/irbpp_streams_mfma.hip and csrc/irbpp_mfma_chain.h compiled for the host
(tests/host/streams_mfma_host.cpp: 512 threads in lockstep per workgroup, the matrix instruction replaced by
tests/host/mfma_shim.h, which computes every accumulator element as the k-ordered fmaf chain through the instruction's lane
maps) against replay._streams_logits_cpu and the numpy definition of tests/test_streams_cpu.py, bit for bit, with poison
around every output: the operand placement, the hand-over of the hidden tile between the two products, the padded rows and
columns, both instantiations and both sides of the LDS threshold, without a GPU.  Shapes and inputs are those of
tests/test_gpu_streams_mfma.py.  The same harness as a program of its own under -fsanitize=address,undefined, every buffer
exactly as large as the kernels may touch, runs once here.  And the yardstick itself is checked: on these inputs a chain
summed in descending order differs from the definition in every layer, so a kernel with the wrong order cannot pass."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from host_harness import build_shared
import test_gpu_streams as G
import test_gpu_streams_mfma as M
from irbpp_amd import replay
from test_streams_cpu import NAMES, f32, lin_np, relu_np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "streams_mfma_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libstreams_mfma_host.so")
LL = C.c_longlong


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_streams_act_mfma.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, LL, C.c_void_p, LL, LL, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, LL, C.c_void_p, C.c_void_p, C.c_int]
    lib.host_streams_act_mfma.restype = C.c_int
    return lib


def _at(a, *idx):
    return C.c_void_p(a.ctypes.data + int(np.ravel_multi_index(idx, a.shape)) * a.itemsize)


def same_bits(got, want):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.parametrize("n,s,E,H,atoms", M.CASES)
def test_streams_mfma_source_on_host(host, n, s, E, H, atoms):
    z = G.support_np(atoms)
    W, xg, x, flags, (want_act, want_q, want_v, want_a), want_free = M.mfma_case(n, s, E, H, atoms)
    cpu_v, cpu_a = replay._streams_logits_cpu(torch.from_numpy(x), torch.from_numpy(xg),
                                              types.SimpleNamespace(**{k: torch.from_numpy(W[k]) for k in NAMES}))
    same_bits(cpu_v.numpy(), want_v)                     # the wrappers' CPU form is the definition
    same_bits(cpu_a.numpy(), want_a)
    w = [np.ascontiguousarray(W[k]) for k in NAMES]
    wp = (C.c_void_p * 8)(*(a.ctypes.data for a in w))
    fits = s * (atoms | 1) * 4 <= G.TILE_BYTES
    obs = np.full((n, s * 5 + 9), 3.0, dtype=f32)
    obs[:, :s * 5].reshape(n, s, 5)[:, :, 4] = flags
    wide_g = np.full((n, E + 7), G.POISON, dtype=f32)
    wide_g[:, 3:3 + E] = xg
    for front, with_all, generic in ((4, True, 0), (1, False, 0), (4, True, 1)):
        if generic and (atoms > 32 or s > 100):
            continue                                         # already the 128-atom instantiation; the long cases run once
        wide = np.full((n, s + 3, E + 8), G.POISON, dtype=f32)
        wide[:, 1:1 + s, front:front + E] = x
        act = np.full(n + 1, -7, dtype=np.int64)
        q = np.full((n, s + 2), -5.0, dtype=f32)
        v = np.full(n * atoms + 4, -5.0, dtype=f32)
        a = np.full(n * s * atoms + 4, -5.0, dtype=f32)
        rc = host.host_streams_act_mfma(wp, E, H, atoms, _at(wide_g, 0, 3), E + 7, _at(wide, 0, 1, front), (s + 3) * (E + 8), E + 8,
                                        z.ctypes.data, obs.ctypes.data if with_all else None, s * 5 + 9, s, n, act.ctypes.data,
                                        q.ctypes.data if with_all else None, s + 2, v.ctypes.data if with_all else None,
                                        a.ctypes.data if with_all or not fits else None, generic)
        assert rc == 0 and act[n] == -7
        if with_all:
            assert (q[:, s:] == -5.0).all() and (v[n * atoms:] == -5.0).all() and (a[n * s * atoms:] == -5.0).all()
            same_bits(v[:n * atoms].reshape(n, atoms), cpu_v.numpy())
            same_bits(a[:n * s * atoms].reshape(n, s, atoms), cpu_a.numpy())
            same_bits(q[:, :s], want_q)
            np.testing.assert_array_equal(act[:n], want_act)
        else:
            assert (q == -5.0).all() and (v == -5.0).all()
            np.testing.assert_array_equal(act[:n], want_free)
    wide = np.full((n, s + 3, E + 8), G.POISON, dtype=f32)
    wide[:, 1:1 + s, 4:4 + E] = x
    act = np.full(n + 1, -7, dtype=np.int64)
    v = np.full(n * atoms + 4, -5.0, dtype=f32)
    a = np.full(n * s * atoms + 4, -5.0, dtype=f32)
    if not fits:                                             # the workspace rule
        assert host.host_streams_act_mfma(wp, E, H, atoms, _at(wide_g, 0, 3), E + 7, _at(wide, 0, 1, 4), (s + 3) * (E + 8), E + 8,
                                          z.ctypes.data, None, 0, s, n, act.ctypes.data, None, 0, None, None, 0) == -1
    # logits only: no action, no q_out
    assert host.host_streams_act_mfma(wp, E, H, atoms, _at(wide_g, 0, 3), E + 7, _at(wide, 0, 1, 4), (s + 3) * (E + 8), E + 8, None, None, 0,
                                      s, n, None, None, 0, v.ctypes.data, a.ctypes.data, 0) == 0
    assert (v[n * atoms:] == -5.0).all() and (a[n * s * atoms:] == -5.0).all() and act[n] == -7
    same_bits(v[:n * atoms].reshape(n, atoms), want_v)
    same_bits(a[:n * s * atoms].reshape(n, s, atoms), want_a)


def test_widths_that_are_no_multiple_of_four_are_refused(host):
    buf = np.zeros(4096, dtype=f32)
    wp = (C.c_void_p * 8)(*([buf.ctypes.data] * 8))
    for E, H in ((6, 8), (8, 6)):
        assert host.host_streams_act_mfma(wp, E, H, 31, buf.ctypes.data, E, buf.ctypes.data, 2 * E, E, buf.ctypes.data, None, 0, 2, 1,
                                          buf.ctypes.data, None, 0, None, None, 0) == -1


def lin_descending_np(w, b, x):
    return lin_np(w[:, ::-1], b, x[..., ::-1])


@pytest.mark.parametrize("n,s,E,H,atoms", M.CASES)
def test_the_inputs_tell_the_order_of_a_chain(n, s, E, H, atoms):
    """The yardstick: every one of the four layers, summed with k descending over the definition's own input, differs from the
    definition in at least one output element."""
    W, xg, x, _, _, _ = M.mfma_case(n, s, E, H, atoms)
    for hidden, out, inp in (("hv", "zv", xg), ("ha", "za", x)):
        h = lin_np(W["w_" + hidden], W["b_" + hidden], inp)
        moved_h = (lin_descending_np(W["w_" + hidden], W["b_" + hidden], inp).view(np.uint32) != h.view(np.uint32)).sum()
        r = relu_np(h)
        o = lin_np(W["w_" + out], W["b_" + out], r)
        moved_o = (lin_descending_np(W["w_" + out], W["b_" + out], r).view(np.uint32) != o.view(np.uint32)).sum()
        print(f"{hidden}: {moved_h} of {h.size} elements move, {out}: {moved_o} of {o.size}")
        assert moved_h > 0 and moved_o > 0


def test_harness_runs_clean_under_the_sanitizers(tmp_path):
    """A program of its own (never loaded into Python): address and undefined-behaviour sanitizers over the kernels' source."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "streams_mfma_host_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DSTREAMS_MFMA_HOST_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and "checksum" in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr
