"""The source of csrc/irbpp_order_embed.hip compiled for the host (tests/host/order_embed_host.cpp: each workgroup's threads in
lockstep, the rows kernel's dynamic LDS a heap block of exactly the bytes the C API asks for, fmaf the C library's) against
the numpy definition of tests/test_order_embed_cpu.py, bit for bit: the convolutions through their padded tiles, base, tiles
of 64 / k whole bins (the smallest call, less than one tile, 12 bins per tile with a short second tile, six bins and four
idle lanes, one bin per tile with 31 idle lanes, a bin that is the tile), blocks of features and inputs whole and short, the
two LDS regions that take turns, Q and K in two blocks (embed 256), every width 1, and the strided arguments, without a GPU.
The same harness as a program of its own under -fsanitize=address,undefined, every buffer exactly as large as the kernels may
touch, runs once here."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from host_harness import HERE, build_shared
from test_order_embed_cpu import NAMES, REFERENCE, SMALL, f32, make_layers, make_obs, order_embed_replay, same_bits

SRC = os.path.join(HERE, "host", "order_embed_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "liborder_embed_host.so")
LL = C.c_longlong
POISON = f32(1e30)


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_order_embed.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, LL, C.c_void_p, LL, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     LL, LL, C.c_void_p, LL]
    lib.host_order_embed.restype = LL
    return lib


def sizes_of(W):
    L = W["L"]
    M = W["w_conv3"].shape[0] * (L // 4) ** 2
    return [L, W["w_conv1"].shape[0], W["w_conv2"].shape[0], W["w_conv3"].shape[0], W["w_g1"].shape[1] - M, W["w_g1"].shape[0],
            W["w_g2"].shape[0], W["w_f1"].shape[0]]


def run(host, obs, sf, W, k, pad=3):
    """Every argument a slice of a wider poisoned block, the workspace poisoned: -> x, xg; the surroundings checked untouched."""
    N, E, F_ = obs.shape[0], W["w_g2"].shape[0], sf.shape[1]
    sizes = sizes_of(W)
    obs_w = np.full((N, obs.shape[1] + pad + 2), POISON, dtype=f32)
    obs_w[:, 2:2 + obs.shape[1]] = obs
    sf_w = np.full((N * k, F_ + pad + 1), POISON, dtype=f32)
    sf_w[:, 1:1 + F_] = sf
    before = obs_w.copy(), sf_w.copy()
    x_w = np.full((N, k + 1, E + pad + 1), POISON, dtype=f32)
    xg_w = np.full((N, E + pad + 2), POISON, dtype=f32)
    base = np.full((N, sizes[5]), POISON, dtype=f32)
    w = [np.ascontiguousarray(W[n]) for n in NAMES]
    wp = (C.c_void_p * 19)(*(a.ctypes.data for a in w))
    sz = (C.c_int * 8)(*sizes)
    lds = host.host_order_embed(wp, sz, W["slope"], obs_w.ctypes.data + 8, obs_w.shape[1], sf_w.ctypes.data + 4, sf_w.shape[1], k, N,
                                base.ctypes.data, x_w.ctypes.data + 4, (k + 1) * x_w.shape[2], x_w.shape[2], xg_w.ctypes.data + 8, xg_w.shape[1])
    assert 0 < lds <= 160 * 1024 - 1024
    np.testing.assert_array_equal(obs_w.view(np.uint32), before[0].view(np.uint32))
    np.testing.assert_array_equal(sf_w.view(np.uint32), before[1].view(np.uint32))
    x, xg = x_w[:, :k, 1:1 + E].copy(), xg_w[:, 2:2 + E].copy()
    x_w[:, :k, 1:1 + E] = POISON
    xg_w[:, 2:2 + E] = POISON
    assert (x_w == POISON).all() and (xg_w == POISON).all() and (base != POISON).all()
    return x, xg


CONFIGS = {"small": SMALL, "reference": REFERENCE, "ones": dict(L=12, convs=(1, 1, 1), feat=1, proj_hidden=1, embed=1, ff_hidden=1),
           "widest": dict(L=16, convs=(16, 32, 4), feat=256, proj_hidden=256, embed=256, ff_hidden=256)}


@functools.lru_cache(maxsize=None)
def case(name, N, k):
    """-> W, obs, sf and the definition's result: computed once and shared (treat as read-only)."""
    cfg = CONFIGS[name]
    rng = np.random.default_rng(40 + 100 * N + k)
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, N, k, cfg["L"], cfg["feat"])
    return W, obs, sf, order_embed_replay(obs, sf, W)


@pytest.mark.parametrize("name,N,k", [("small", 1, 2), ("small", 3, 5), ("small", 14, 5), ("small", 7, 10), ("small", 3, 33), ("small", 2, 64),
                                      ("ones", 2, 3), ("widest", 1, 2), ("reference", 2, 10)])
def test_order_embed_source_on_host(host, name, N, k):
    W, obs, sf, (want_x, want_xg) = case(name, N, k)
    x, xg = run(host, obs, sf, W, k)
    same_bits(x, want_x)
    same_bits(xg, want_xg)


def test_strides_and_bins_do_not_change_a_bit(host):
    """Bin 1 of three alone, with other strides: the same bits."""
    W, obs, sf, (want_x, want_xg) = case("small", 3, 5)
    x, xg = run(host, obs[1:2], sf[5:10], W, 5, pad=0)
    same_bits(x[0], want_x[1])
    same_bits(xg[0], want_xg[1])


def test_harness_runs_clean_under_the_sanitizers(tmp_path):
    """A program of its own (never loaded into Python): address and undefined-behaviour sanitizers over the kernels' source."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "order_embed_host_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DORDER_EMBED_HOST_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and "checksum" in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr
