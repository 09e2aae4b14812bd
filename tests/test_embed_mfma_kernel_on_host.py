"""The source of csrc/irbpp_embed_mfma.hip, csrc/irbpp_mfma_chain.h and csrc/irbpp_embed.hip compiled for the host
(tests/host/embed_mfma_host.cpp: 512 threads in lockstep per workgroup, the matrix instruction replaced by
tests/host/mfma_shim.h, which computes every accumulator element as the k-ordered fmaf chain through the instruction's lane
maps) against replay.embed on CPU tensors, which tests/test_embed_cpu.py proves to be the unfactored definition: bit for bit,
with poison around every output and the workspace, the dynamic LDS a heap block of exactly the launch's bytes.  The operand
placement, the (feature block, row half) pairs dealt to the waves, the hand-over of a layer through LDS, the padded features
and rows, the masks of both row halves and the element loads of unaligned weight rows, without a GPU.  Configurations, rows
and inputs are those of tests/test_embed_mfma_cpu.py, shared with tests/test_gpu_embed_mfma.py.  The same harness as a
program of its own under -fsanitize=address,undefined, every buffer exactly as large as the kernels may touch, runs once here.
And the yardstick itself is checked: on these inputs each of the three layers summed in descending k differs from the
definition in a valid row, so a kernel with another order cannot pass."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from host_harness import HERE, build_shared
from test_embed_kernel_on_host import LL, run
from test_embed_mfma_cpu import CASES, UNALIGNED, case, moved_by_descending_order, same_bits

SRC = os.path.join(HERE, "host", "embed_mfma_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libembed_mfma_host.so")


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_embed_mfma.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, LL, C.c_void_p, LL, C.c_int, C.c_int, C.c_void_p, C.c_void_p, LL,
                                    LL, C.c_void_p, LL]
    lib.host_embed_mfma.restype = LL
    lib.host_embed = lib.host_embed_mfma                     # test_embed_kernel_on_host.run calls its harness by this name
    return lib


@pytest.mark.parametrize("name,N,S", CASES)
def test_embed_mfma_source_on_host(host, name, N, S):
    """run: every argument a slice of a wider poisoned block (x from a leading offset of one float, so its rows are not
    16-byte aligned), the workspace poisoned, the surroundings checked untouched."""
    W, obs, sf, (want_x, want_xg) = case(name, N, S)
    x, xg = run(host, obs, sf, W, S)
    same_bits(x, want_x)
    same_bits(xg, want_xg)
    if N > 1:
        assert (want_x[N - 1] == 0).all() and (want_x[0, 0] != 0).any()      # the all-invalid and the all-valid bin


def off_by_one_float(a):
    """A contiguous copy of `a` that starts 4 bytes past a 16-byte boundary."""
    buf = np.zeros(a.size + 8, dtype=a.dtype)
    start = next(i for i in range(8) if (buf.ctypes.data + 4 * i) % 16 == 4)
    out = buf[start:start + a.size].reshape(a.shape)
    out[...] = a
    return out


def test_rows_that_are_not_aligned(host):
    """The element loads: feat + M = 49, so no row of project_layer[0]'s candidate columns is 16-byte aligned, and every
    weight array starts one float past a boundary."""
    name, N, S = UNALIGNED
    W, obs, sf, (want_x, want_xg) = case(name, N, S)
    moved = {k: (off_by_one_float(v) if isinstance(v, np.ndarray) else v) for k, v in W.items()}
    x, xg = run(host, obs, sf, moved, S)
    same_bits(x, want_x)
    same_bits(xg, want_xg)


def test_a_bin_alone_equals_itself_in_the_batch(host):
    W, obs, sf, (want_x, want_xg) = case("blocks", 3, 17)
    x, xg = run(host, obs[1:2], sf[1:2], W, 17, pad=0)
    same_bits(x[0], want_x[1])
    same_bits(xg[0], want_xg[1])


def test_widths_that_are_no_multiple_of_four_are_refused(host):
    buf = np.zeros(4096, dtype=np.float32)
    wp = (C.c_void_p * 14)(*([buf.ctypes.data] * 14))
    for hc, ec, p in ((6, 8, 8), (8, 6, 8), (8, 8, 6)):
        sz = (C.c_int * 9)(8, 2, 2, 1, 4, hc, ec, p, 8)
        assert host.host_embed_mfma(wp, sz, 0.01, buf.ctypes.data, 88, buf.ctypes.data, 4, 3, 1, buf.ctypes.data, buf.ctypes.data, 24, 8,
                                    buf.ctypes.data, 8) == -1


@pytest.mark.parametrize("name,N,S", CASES + [UNALIGNED])
def test_the_inputs_tell_the_order_of_a_chain(name, N, S):
    """The yardstick: each of the three layers, summed with k descending over the definition's own input, differs from the
    definition in at least one output element of a valid row."""
    W, obs, sf, _ = case(name, N, S)
    moved = moved_by_descending_order(W, obs, sf)
    print(", ".join(f"{k}: {m} of {n} elements move" for k, (m, n) in moved.items()))
    assert all(m > 0 for m, _ in moved.values())


def test_harness_runs_clean_under_the_sanitizers(tmp_path):
    """A program of its own (never loaded into Python): address and undefined-behaviour sanitizers over the kernels' source."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "embed_mfma_host_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DEMBED_MFMA_HOST_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and res.stdout.count("checksum") == 5 and "ERROR" not in res.stderr and "runtime error" not in res.stderr
