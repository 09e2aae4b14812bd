"""The source of csrc/irbpp_order_embed_mfma.hip, csrc/irbpp_mfma_chain.h and csrc/irbpp_order_embed.hip compiled for the host
(tests/host/order_embed_mfma_host.cpp: 512 threads in lockstep per workgroup, the matrix instruction replaced by
tests/host/mfma_shim.h, which computes every accumulator element as the k-ordered fmaf chain through the instruction's lane
maps) against replay.order_embed on CPU tensors, which tests/test_order_embed_cpu.py proves to be the definition: bit for bit,
with poison around every output and the workspace, the dynamic LDS a heap block of exactly the launch's bytes.  The operand
placement, the (feature block, row half) pairs dealt to the waves in one or two passes, the chains' starts (`base` of the
column's bin, a bias, +0.0), the residuals kept in registers across three layers, the hand-over of a layer through LDS, the
padded features, the lanes past the tile's last row, Q and K in two rounds and the element loads of unaligned weight rows,
without a GPU.  Width sets, (N, k) and inputs are those of tests/test_order_embed_mfma_cpu.py (which checks that they tell the
order of every layer's chain), shared with tests/test_gpu_order_embed_mfma.py.  The same harness as a program of its own under
-fsanitize=address,undefined, every buffer exactly as large as the kernels may touch, runs once here."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from host_harness import HERE, build_shared
from test_order_embed_kernel_on_host import LL, run
from test_order_embed_mfma_cpu import CASES, UNALIGNED, case, same_bits

SRC = os.path.join(HERE, "host", "order_embed_mfma_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "liborder_embed_mfma_host.so")


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_order_embed_mfma.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, LL, C.c_void_p, LL, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, LL, LL, C.c_void_p, LL]
    lib.host_order_embed_mfma.restype = LL
    lib.host_order_embed = lib.host_order_embed_mfma         # test_order_embed_kernel_on_host.run calls its harness by this name
    return lib


@pytest.mark.parametrize("name,N,k", CASES)
def test_order_embed_mfma_source_on_host(host, name, N, k):
    """run: every argument a slice of a wider poisoned block (x from a leading offset of one float, so its rows are not
    16-byte aligned), the workspace poisoned, the surroundings checked untouched."""
    W, obs, sf, (want_x, want_xg) = case(name, N, k)
    x, xg = run(host, obs, sf, W, k)
    same_bits(x, want_x)
    same_bits(xg, want_xg)


def off_by_one_float(a):
    """A contiguous copy of `a` that starts 4 bytes past a 16-byte boundary."""
    buf = np.zeros(a.size + 8, dtype=a.dtype)
    start = next(i for i in range(8) if (buf.ctypes.data + 4 * i) % 16 == 4)
    out = buf[start:start + a.size].reshape(a.shape)
    out[...] = a
    return out


def test_rows_that_are_not_aligned(host):
    """The element loads: feat + M = 21, so no row of gat_project_layer[0]'s shape columns is 16-byte aligned, and every
    weight array starts one float past a boundary."""
    name, N, k = UNALIGNED
    W, obs, sf, (want_x, want_xg) = case(name, N, k)
    assert W["w_g1"].shape[1] % 4 != 0
    moved = {n: (off_by_one_float(v) if isinstance(v, np.ndarray) else v) for n, v in W.items()}
    assert all(v.ctypes.data % 16 == 4 and v.flags.c_contiguous for v in moved.values() if isinstance(v, np.ndarray))
    x, xg = run(host, obs, sf, moved, k)
    same_bits(x, want_x)
    same_bits(xg, want_xg)


def test_a_bin_alone_equals_itself_in_the_batch(host):
    """Bin 6 of fourteen (rows 30 .. 34 of its tile, across the two row halves) alone, with other strides: the same bits."""
    W, obs, sf, (want_x, want_xg) = case("odd32", 14, 5)
    x, xg = run(host, obs[6:7], sf[30:35], W, 5, pad=0)
    same_bits(x[0], want_x[6])
    same_bits(xg[0], want_xg[6])


def test_widths_that_are_no_multiple_of_four_are_refused(host):
    buf = np.zeros(4096, dtype=np.float32)
    wp = (C.c_void_p * 19)(*([buf.ctypes.data] * 19))
    for f, p, e, hf in ((6, 8, 8, 8), (8, 6, 8, 8), (8, 8, 6, 8), (8, 8, 8, 6)):
        sz = (C.c_int * 8)(8, 2, 2, 1, f, p, e, hf)
        assert host.host_order_embed_mfma(wp, sz, 0.01, buf.ctypes.data, 67, buf.ctypes.data, 8, 3, 1, buf.ctypes.data, buf.ctypes.data, 24, 8,
                                          buf.ctypes.data, 8) == -1


def test_harness_runs_clean_under_the_sanitizers(tmp_path):
    """A program of its own (never loaded into Python): address and undefined-behaviour sanitizers over the kernels' source."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "order_embed_mfma_host_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DORDER_EMBED_MFMA_HOST_MAIN",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "host", "stub"),
                    SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and res.stdout.count("checksum") == 6 and "ERROR" not in res.stderr and "runtime error" not in res.stderr
