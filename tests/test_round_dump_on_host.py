"""The two forms in which a trace wave's borders reach the polygon kernel (irbpp_amd/csrc/irbpp_rounds.h), compiled for the
HOST by tests/host/round_dump_host.cpp and run by 64 threads in lockstep: the RECORD form (the trace wave gathers every round's
positions and stores them) and the DUMP form (the trace wave stores its slots and a lane table once, the polygon wave gathers)
must hand approx_convex_segmented the same positions, element for element -- live, pv, jj, nn, sbq, prk, per round, in round
order -- and both must be the greedy partition of the wave's borders stated here in plain Python."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_device_contours_on_host import _images, _oracle_outer

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "round_dump_host.cpp")
u8p, i32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
MAX_ROUNDS = 64


@pytest.fixture(scope="module", params=[0, 8], ids=["one_class", "short_class_8"])
def lib(request):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    out = os.path.join(HERE, "host", "_build", f"libround_dump_host_{request.param}.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-Wno-unused-value", f"-DIRBPP_TRACE_SHORT={request.param}",
                    "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    lib.host_round_forms.argtypes = [C.c_int, u8p, u8p, i32p, i32p, C.c_int, i32p, i32p, i32p, u64p]
    lib.host_round_forms.restype = C.c_int
    k = (C.c_int * 6)()
    lib.host_round_constants(k)
    lib.K = dict(zip(("P", "LCAP", "CAP", "SLOT", "SPILL", "SHORT"), list(k)))
    assert lib.K["SHORT"] == request.param
    return lib


def _partition(ns, K):
    """The greedy rounds: per class (borders of up to SHORT points, then the rest), the lanes in order, each round the longest
    run of them that fits 64 * P positions.  -> [[(lane, start), ...], ...]"""
    left, rounds = list(ns), []
    for cls in (0, 1):
        while True:
            todo = [l for l in range(64) if left[l] > 0 and (cls == 1 or left[l] <= K["SHORT"])]
            if not todo:
                break
            tot, sel = 0, []
            for l in todo:
                if tot + left[l] > 64 * K["P"]:
                    break
                sel.append((l, tot))
                tot += left[l]
            for l, _ in sel:
                left[l] = 0
            rounds.append(sel)
    return rounds


def _run(lib, borders, rks, cpw=64):
    """borders: 64 point lists (x | y << 4 bytes; [] = a lane without a border).  Runs both forms, checks them against each
    other and against the plain statement; returns the number of rounds."""
    K = lib.K
    npos = 64 * K["P"]
    rng = np.random.RandomState(len(borders[0]) + 7)
    slots = rng.randint(0, 256, size=(64, K["SLOT"])).astype(np.uint8)       # whatever the walks left there
    spill = rng.randint(0, 256, size=(64, K["SPILL"])).astype(np.uint8)
    ns = np.zeros(64, dtype=np.int32)
    for l, b in enumerate(borders):
        assert len(b) <= K["CAP"] and (l < cpw or not b)
        ns[l] = len(b)
        slots[l, :min(len(b), K["LCAP"])] = b[:K["LCAP"]]
        spill[l, :max(0, len(b) - K["LCAP"])] = b[K["LCAP"]:]
    rk = np.asarray(rks, dtype=np.int32)
    rec = np.full((MAX_ROUNDS, 6, npos), -7, dtype=np.int32)
    dump = np.full((MAX_ROUNDS, 6, npos), -9, dtype=np.int32)
    plan = np.zeros((64, 2), dtype=np.int32)
    sels = np.zeros(MAX_ROUNDS, dtype=np.uint64)
    n = lib.host_round_forms(cpw, slots.ctypes.data_as(u8p), spill.ctypes.data_as(u8p), ns.ctypes.data_as(i32p), rk.ctypes.data_as(i32p),
                             MAX_ROUNDS, rec.ctypes.data_as(i32p), dump.ctypes.data_as(i32p), plan.ctypes.data_as(i32p),
                             sels.ctypes.data_as(u64p))
    want = _partition(ns, K)
    assert n == len(want)
    for r, sel in enumerate(want):
        for name, a, b in zip(("live", "pv", "jj", "nn", "sbq", "prk"), rec[r], dump[r]):
            np.testing.assert_array_equal(a, b, err_msg=f"{name}, round {r}")
        assert int(sels[r]) == sum(1 << l for l, _ in sel)
        live, pv, jj, nn, sbq, prk = dump[r]
        exp_live = np.zeros(npos, dtype=np.int32)
        for l, start in sel:
            assert tuple(plan[l]) == (r, start)
            q = slice(start, start + ns[l])
            exp_live[q] = 1
            np.testing.assert_array_equal(pv[q], np.asarray(borders[l], dtype=np.int32))
            np.testing.assert_array_equal(jj[q], np.arange(ns[l]))
            assert (nn[q] == ns[l]).all() and (sbq[q] == start).all() and (prk[q] == rk[l]).all()
        np.testing.assert_array_equal(live, exp_live)
        dead = exp_live == 0
        assert (pv[dead] == 0).all() and (jj[dead] == 0).all() and (nn[dead] == 1).all() and (sbq[dead] == 0).all()
    return n


def _walk(rng, n):
    return [int(v) for v in rng.randint(0, 256, size=n)]


@pytest.mark.parametrize("seed", range(3))
def test_borders_of_generated_images(lib, seed):
    """Waves of 64 candidates as the trace kernel meets them: the outer borders of the contour tests' images in the order they
    are found, a third of the lanes candidates that were no first pixel (0 points), borders beyond TRACE_CAP left to the redo."""
    rng = np.random.RandomState(40 + seed)
    lanes, rounds, waves = [], 0, 0
    for img in _images(700 + seed, 60):
        outer, _, _ = _oracle_outer(img)
        for c in outer:
            pts = [x | (y << 4) for x, y in c]
            lanes.append(pts if 2 <= len(pts) <= lib.K["CAP"] else [])          # (1-point borders are isolated pixels: never traced)
            if rng.rand() < 0.5:
                lanes.append([])
    for at in range(0, len(lanes) - 63, 64):
        rounds += _run(lib, lanes[at:at + 64], rng.randint(0, 1 << 20, size=64))
        waves += 1
    assert waves >= 3 and rounds > waves                                       # several rounds per wave were among them


def test_constructed_waves_hit_every_branch(lib):
    K = lib.K
    P, LCAP, CAP = K["P"], K["LCAP"], K["CAP"]
    rng = np.random.RandomState(3)
    rk = rng.randint(0, 1 << 20, size=64)
    # 64 borders of one point, and the same with every third lane empty
    assert _run(lib, [_walk(rng, 1) for _ in range(64)], rk) == 1
    assert _run(lib, [_walk(rng, 1) if l % 3 else [] for l in range(64)], rk) == 1
    # nothing at all
    assert _run(lib, [[] for _ in range(64)], rk) == 0
    # one border that fills a round alone (as long as a border can be), first, in the middle and last
    full = min(64 * P, CAP)
    for at in (0, 31, 63):
        assert _run(lib, [_walk(rng, full) if l == at else [] for l in range(64)], rk) == 1
        others = [_walk(rng, full) if l == at else _walk(rng, 3) for l in range(64)]
        assert _run(lib, others, rk) >= (2 if full == 64 * P else 1)
    # sums that end one point short of, exactly on, and one point past the round boundary
    for last in (-1, 0, 1):
        borders = [_walk(rng, 16) for _ in range(64 * P // 16 - 1)] + [_walk(rng, 16 + last)]
        borders += [[] for _ in range(64 - len(borders))]
        assert _run(lib, borders, rk) == (2 if last > 0 else 1)
    # spill bytes: a border of LCAP + 1 points, one of CAP points, both, and next to borders that stay in LDS
    assert _run(lib, [_walk(rng, LCAP + 1) if l == 5 else [] for l in range(64)], rk) == 1
    assert _run(lib, [_walk(rng, CAP) if l == 62 else [] for l in range(64)], rk) == 1
    mixed = [_walk(rng, (LCAP + 1, CAP, LCAP, 7, 0)[l % 5]) for l in range(64)]
    assert _run(lib, mixed, rk) > 8
    # every lane a border of CAP points: as many rounds as a wave can have
    assert _run(lib, [_walk(rng, CAP) for _ in range(64)], rk) == 64 // max(1, 64 * P // CAP)
    # a short final chunk: 9 candidates; and the 32- and 16-candidate launches' waves
    assert _run(lib, [_walk(rng, 11) if l < 9 else [] for l in range(64)], rk) >= 1
    for cpw in (32, 16):
        borders = [_walk(rng, int(rng.randint(0, 70))) if l < cpw else [] for l in range(64)]
        borders[cpw - 1] = _walk(rng, LCAP + 3)
        assert _run(lib, borders, rk, cpw=cpw) >= 1
    # short and long borders interleaved (two classes when TRACE_SHORT is compiled in)
    inter = [_walk(rng, (2, 40, 8, 9, 0, 120)[l % 6]) for l in range(64)]
    assert _run(lib, inter, rk) > 4
