"""Rotation aliases (irbpp_amd/csrc/irbpp_rotalias.h: the rotations of a shape whose observation inputs -- footprint sizes,
bottom table, has_out, ext_z_r -- are bit-identical), compiled for the host by tests/host/rotalias_host.cpp: the function
irbpp_load_shapes fills ShapeRot::alias with, on hand-made shapes and on the synthetic data sets."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import irbpp_amd  # noqa: F401
from irbpp_amd import synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "rotalias_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "librotalias_host.so")
EXE = os.path.join(HERE, "host", "_build", "rotalias_host")
RES_A = 0.02


@pytest.fixture(scope="module")
def host():
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", OUT], check=True)
    lib = C.CDLL(OUT)
    lib.host_rot_aliases.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    lib.host_rot_aliases.restype = None
    return lib


def aliases(host, extents, tables):
    """alias[r] of one shape given as irbpp_load_shapes gets it: per rotation raw extents and (T, B, maskH, maskB).  Only what
    the observation depends on is handed to the function under test -- the top table and ext_x / ext_y / ext_z are not."""
    R = len(tables)
    sizes = np.zeros((R, 5), dtype=np.int32)
    ezr = np.zeros(R, dtype=np.float64)
    offs = np.zeros(R, dtype=np.int64)
    mpool, bpool, pos = [], [], 0
    for r, (_T, B, _mH, mB) in enumerate(tables):
        e = np.round(np.asarray(extents[r], dtype=np.float64), 6)
        sizes[r] = (B.shape[0], B.shape[1], int(np.ceil(e[0] / RES_A)), int(np.ceil(e[1] / RES_A)), int((mB == 0).any()))
        ezr[r] = e[2]
        offs[r] = pos
        pos += B.size
        mpool.append(np.ascontiguousarray(mB, dtype=np.float64).reshape(-1))
        bpool.append(np.ascontiguousarray(B, dtype=np.float64).reshape(-1))
    m, b = np.concatenate(mpool), np.concatenate(bpool)
    out = np.full(R, -1, dtype=np.int32)
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    host.host_rot_aliases(R, sizes.ctypes.data_as(C.POINTER(C.c_int32)), f64(ezr), offs.ctypes.data_as(C.POINTER(C.c_int64)),
                          f64(m), f64(b), out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out.tolist()


def _polycube(occ, n_rot=4):
    ext0, tab0 = synthetic._voxel_tables(np.asarray(occ, dtype=bool), 0.04, 0.01)
    return synthetic._all_rotations(ext0, tab0, n_rot, 0.01)


def _pair(ext, tab):
    """Two rotations with the same extents and (copies of the) same tables."""
    return [np.array(ext), np.array(ext)], [tuple(a.copy() for a in tab), tuple(a.copy() for a in tab)]


BOX = ((0.06, 0.06, 0.05), synthetic._box_tables(np.array([0.06, 0.06, 0.05]), 0.01))


def test_cube_aliases_every_rotation_to_the_first(host):
    assert aliases(host, *_polycube(np.ones((1, 1, 1)))) == [0, 0, 0, 0]


def test_bar_aliases_opposite_rotations(host):
    assert aliases(host, *_polycube(np.ones((1, 2, 1)))) == [0, 1, 0, 1]


def test_l_tromino_has_no_aliases(host):
    occ = np.ones((2, 2, 1), dtype=bool)
    occ[1, 1, 0] = False
    assert aliases(host, *_polycube(occ)) == [0, 1, 2, 3]


def test_ext_z_r_alone_keeps_rotations_apart(host):
    exts, tabs = _pair(*BOX)
    assert aliases(host, exts, tabs) == [0, 0]
    exts[1][2] = 0.050001                            # (a difference np.round(., 6) keeps)
    assert aliases(host, exts, tabs) == [0, 1]
    exts[1][2] = 0.05 + 1e-9                         # ... and one it removes: ext_z_r is what counts, not ext_z
    assert aliases(host, exts, tabs) == [0, 0]


def test_one_ulp_of_a_bottom_height_keeps_rotations_apart(host):
    exts, tabs = _pair(*BOX)
    tabs[0][1][2, 3] = 0.01
    tabs[1][1][2, 3] = np.nextafter(0.01, 1.0)
    assert aliases(host, exts, tabs) == [0, 1]
    tabs[1][1][2, 3] = 0.01
    assert aliases(host, exts, tabs) == [0, 0]


def test_the_top_table_takes_no_part(host):
    exts, tabs = _pair(*BOX)
    tabs[1][0][:] += 0.01
    tabs[1][2][0, 0] = 0.0
    assert aliases(host, exts, tabs) == [0, 0]


def test_a_masked_out_cell_that_moved_keeps_rotations_apart(host):
    exts, tabs = _pair(*BOX)
    tabs[0][3][0, 0] = 0.0
    tabs[1][3][5, 5] = 0.0
    assert aliases(host, exts, tabs) == [0, 1]
    tabs[1][3][5, 5] = 1.0
    tabs[1][3][0, 0] = 0.0
    tabs[1][1][0, 0] = 3.0                           # a bottom height under a masked-out cell is never read
    assert aliases(host, exts, tabs) == [0, 0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _numpy_aliases(shapes, k, all_tables):
    """The relation restated in numpy.  all_tables=False: what the observation depends on (sizes, masked-in bottom cells,
    ext_z_r).  all_tables=True: the stricter relation the duplicate counts were first taken with -- all four tables and the raw
    extents bit for bit."""
    R = shapes.n_rot
    al = list(range(R))
    for r in range(R):
        Tr, Br, mHr, mBr = shapes.tables[k][r]
        er = np.round(shapes.extents[k][r], 6)
        for c in range(r):
            if al[c] != c:
                continue
            Tc, Bc, mHc, mBc = shapes.tables[k][c]
            ec = np.round(shapes.extents[k][c], 6)
            same = (Br.shape == Bc.shape and np.array_equal(np.ceil(er[:2] / RES_A), np.ceil(ec[:2] / RES_A)) and
                    _bits(er[2:]).tolist() == _bits(ec[2:]).tolist() and np.array_equal(mBr != 0, mBc != 0) and
                    np.array_equal(_bits(Br)[mBr != 0], _bits(Bc)[mBc != 0]))
            if same and all_tables:
                same = (np.array_equal(_bits(Br), _bits(Bc)) and np.array_equal(_bits(Tr), _bits(Tc)) and
                        np.array_equal(_bits(mHr), _bits(mHc)) and np.array_equal(_bits(mBr), _bits(mBc)) and
                        _bits(shapes.extents[k][r]).tolist() == _bits(shapes.extents[k][c]).tolist())
            if same:
                al[r] = c
                break
    return al


def _summary(per_shape):
    dup = sum(sum(1 for r, a in enumerate(al) if a != r) for al in per_shape)
    distinct = np.bincount([sum(1 for r, a in enumerate(al) if a == r) for al in per_shape])
    return dup, {int(d): int(c) for d, c in enumerate(distinct) if c}


@pytest.mark.parametrize("name,make,strict_want", [
    ("blockout_r4", lambda: synthetic.blockout_shapes(64, n_rot=4, seed=0), (51, {1: 7, 2: 15, 4: 42})),
    ("blockout_r8", lambda: synthetic.blockout_shapes(64, n_rot=8, seed=0), (102, {2: 7, 4: 15, 8: 42})),
    ("cube", lambda: synthetic.cube_shapes(), (25, {1: 25, 2: 100})),
    ("general", lambda: synthetic.general_shapes(32, n_rot=8), (0, {8: 32})),
])
def test_duplicate_counts_of_the_synthetic_data_sets(host, name, make, strict_want):
    """Rotations that are bit-identical in all four tables and the extents: 51 of BlockOut's 256 (R = 4), 102 of 512 (R = 8), 25 of
    the cubes' 250, none on free-form data.  The function under test ignores the top table, as it must, so it finds those and
    more (polycubes with a symmetric underside and an asymmetric top: 72 and 144 on BlockOut by the numpy restatement): per
    shape it has to equal the numpy restatement of its own relation, and every all-tables duplicate has to be an alias."""
    shapes = make()
    strict = [_numpy_aliases(shapes, k, True) for k in range(shapes.n_shapes)]
    assert _summary(strict) == strict_want
    want = [_numpy_aliases(shapes, k, False) for k in range(shapes.n_shapes)]
    got = [aliases(host, shapes.extents[k], shapes.tables[k]) for k in range(shapes.n_shapes)]
    assert got == want
    for al_strict, al in zip(strict, got):
        assert all(a != r for r, (s, a) in enumerate(zip(al_strict, al)) if s != r)
    if name == "cube":
        assert _summary(got) == strict_want          # boxes: the top table is as symmetric as the bottom table


def test_the_stand_alone_program_passes_its_own_cases(host):
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", SRC, "-o", EXE], check=True)
    res = subprocess.run([EXE], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
