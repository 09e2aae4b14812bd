"""The arithmetic of the device-side episode metrics (irbpp_amd/csrc/irbpp_metrics.h) compiled for the HOST by
tests/host/metrics_host.cpp and held against what the trainer really computes (trainer.py:168-178, 215-222): Python's
round(r, 6) as the Monitor applies it, np.mean's summation order for every window length, and the tail merge of several
parts' windows against a sort -- plus the row conventions of irbpp_amd.metrics.  No GPU needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from episode_window_model import halfway_cases

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "metrics_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libmetrics_host.so")
f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def host():
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    # -ffp-contract=off as for the device build: p = x * 1e6 must be the rounded product, not part of a fused multiply-add
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-ffp-contract=off", SRC, "-o", OUT], check=True)
    lib = C.CDLL(OUT)
    lib.host_py_round6.argtypes = [f64p, f64p, C.c_int64]
    lib.host_np_mean.argtypes = [f64p, C.c_int]
    lib.host_np_mean.restype = C.c_double
    lib.host_tail_merge.argtypes = [i64p, i32p, C.c_int, C.c_int, C.c_int, i32p, i32p]
    return lib


def _round6(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    lib.host_py_round6(x.ctypes.data_as(f64p), out.ctypes.data_as(f64p), x.size)
    return out


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def _python_round(x):
    return np.array([round(float(v), 6) for v in x], dtype=np.float64)


def test_round6_is_pythons_round_on_random_values(host):
    rng = np.random.default_rng(5)
    parts = [rng.uniform(0.0, 20.0, 1_000_000),                                         # episode rewards: ratio * 10 sums
             rng.uniform(-1.0, 1.0, 300_000) * 10.0 ** rng.integers(-8, 4, 300_000),    # mixed magnitudes, both signs
             np.round(rng.uniform(0, 50, 300_000), 7),                                   # seven decimals: near-ties
             rng.integers(0, 10**9, 400_000) / 1e6 + rng.choice([-5e-7, 5e-7], 400_000)]  # k/1e6 +- half a unit
    x = np.concatenate(parts)
    assert _bits_equal(_round6(host, x), _python_round(x))


def test_round6_on_constructed_halfway_cases(host):
    x, exact_ties, near = halfway_cases()
    got, want = _round6(host, x), _python_round(x)
    assert _bits_equal(got, want), x[np.nonzero(got.view(np.int64) != want.view(np.int64))[0][:5]]
    lo = 2 * exact_ties.size
    assert not _bits_equal(np.round(near, 6), want[lo:lo + near.size])      # np.round (rint(x * 1e6) / 1e6) is another function


def test_mean_matches_np_mean_for_every_window_length(host):
    rng = np.random.default_rng(11)
    for n in range(1, 1025):
        vals = (rng.random(n) * 10.0 ** rng.integers(-7, 7, n)).tolist()
        a = np.ascontiguousarray(vals, dtype=np.float64)
        got = host.host_np_mean(a.ctypes.data_as(f64p), n)
        assert _bits_equal([got], [np.mean(vals)]), n
        counters = rng.integers(0, 200, n).tolist()                  # ints: the trainer's deque of counters
        c = np.ascontiguousarray(counters, dtype=np.float64)
        assert _bits_equal([host.host_np_mean(c.ctypes.data_as(f64p), n)], [np.mean(counters)]), n


def test_tail_merge_equals_a_sort_of_the_union(host):
    rng = np.random.default_rng(3)
    for case in range(120):
        P = int(rng.choice([1, 2, 3, 4, 7, 16, 64]))
        W = int(rng.choice([1, 2, 10, 37, 128]))
        per = 50                                             # bins per part: part p owns global bins [p*per, (p+1)*per)
        keys = np.full((P, W), -1, dtype=np.int64)
        fills = np.zeros(P, dtype=np.int32)
        for p in range(P):
            f = int(rng.integers(0, W + 1))
            steps = np.sort(rng.integers(1, 40, f))
            bins = rng.integers(p * per, (p + 1) * per, f)
            k = np.unique((steps.astype(np.int64) << 32) | bins)           # distinct, ascending
            keys[p, :k.size], fills[p] = k, k.size
        total = int(fills.sum())
        if total == 0:
            continue
        n = min(W, total)
        part = np.empty(n, np.int32)
        idx = np.empty(n, np.int32)
        host.host_tail_merge(keys.ctypes.data_as(i64p), fills.ctypes.data_as(i32p), P, W, n, part.ctypes.data_as(i32p),
                             idx.ctypes.data_as(i32p))
        union = np.sort(np.concatenate([keys[p, :fills[p]] for p in range(P)]))
        np.testing.assert_array_equal(keys[part, idx], union[-n:], err_msg=f"case {case}: P={P} W={W}")


def test_rows_and_scalars_conventions():
    from irbpp_amd import metrics
    rows = np.array([[1, 0] + [np.nan] * 5, [2, 2, 1.5, 2.0, 1.0, 0.5, 7.0], [3, -2] + [np.nan] * 5])
    kept, nxt = metrics.take_rows(rows, 1, 64)
    assert kept.shape == (2, 7) and nxt == 3
    tags = list(metrics.scalars(kept))
    assert tags == [("Metric/Reward mean", 1.5, 2), ("Metric/Reward max", 2.0, 2), ("Metric/Reward min", 1.0, 2),
                    ("Metric/Ratio", 0.5, 2), ("Metric/Length", 7.0, 2)]
    with pytest.raises(metrics.EpisodeMetricsOverrun):
        metrics.take_rows(np.array([[5, -1] + [np.nan] * 5, [6, 1, 1, 1, 1, 1, 1]]), 5, 1)
    with pytest.raises(Exception):
        metrics.take_rows(np.array([[5, -2] + [np.nan] * 5, [6, 1, 1, 1, 1, 1, 1]]), 5, 64)      # parts out of step
    assert metrics.window_words(10, 64) == 2 + 64 + 40 + 4 * 640
