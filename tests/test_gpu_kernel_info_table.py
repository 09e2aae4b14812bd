"""GpuPackingEnv.kernel_info() is rendered from the launch plan (csrc/irbpp_plan.h) that the launcher executes.  Before that
it was written out by hand beside the launcher; tests/golden/kernel_info_parent.json holds what that hand-written description
returned on the MI355X (the commit before the plan, loaded through IRBPP_LIBRARY) for the bench workloads crossed with launch
sizes on both sides of every size threshold and with the tunings of tests/test_gpu_features.py, plus the capacity path (a wide
grid, deep levels).  The rendered plan has to say the same, byte for byte -- except in the rows listed in `truthful`, where the
old description named a kernel the launcher did not launch.  Environments are created and closed one at a time; no step runs."""
import functools
import json
import os

import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from irbpp_amd.vec_env import GpuPackingEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_info_parent.json")

SIZES = (96, 1024, 2048, 4096, 8192)
WORKLOADS = ("blockout", "cube", "general", "abc_fine", "blockout_k10", "blockout_r8")
T = _lib
# test_specialised_builds_and_split_apply_change_nothing's tunings, then test_trace_launch_shapes_change_nothing's
TUNINGS = (0, T.TUNE_NO_SPECIALISED | T.TUNE_SPLIT_APPLY | T.TUNE_WAVE_EMIT, T.TUNE_FUSED_APPLY | T.TUNE_BLOCK_EMIT,
           T.TUNE_SPLIT_APPLY | T.TUNE_WAVE_EMIT | T.TUNE_GRAPH, T.TUNE_NO_SPECIALISED | T.TUNE_FUSED_APPLY | T.TUNE_BLOCK_EMIT,
           T.TUNE_NO_WG512, T.TUNE_WG512, T.TUNE_NARROW_KERNEL | T.TUNE_WG512, T.TUNE_NO_MIXED_PATH, T.TUNE_CHAIN, T.TUNE_WG128,
           T.TUNE_WG128 | T.TUNE_SPLIT_APPLY, T.TUNE_RECT,
           T.TUNE_TRACE_CPW64, T.TUNE_TRACE_CPW32, T.TUNE_TRACE_CPW16, T.TUNE_INLINE_POLYGON,
           T.TUNE_TRACE_CPW16 | T.TUNE_INLINE_POLYGON, T.TUNE_NO_HEAVY_FIRST, T.TUNE_TRACE_REFILL,
           T.TUNE_TRACE_REFILL | T.TUNE_INLINE_POLYGON)
CAPACITY = ("wide_grid", "wide_grid_k3", "deep_levels", "deep_levels_k3")    # irbpp_wide.hip: at 96 and 2048 bins, no tuning


@functools.lru_cache(maxsize=None)
def workload(name):
    if name in WORKLOADS:
        from bench import make_workload
        return make_workload(name)
    k = dict(bufferSize=3) if name.endswith("_k3") else {}
    if name.startswith("wide_grid"):
        sh = synthetic.general_shapes(n_shapes=16, n_rot=4, fmin=4, fmax=14, seed=3)
        return sh, synthetic.make_sequences(sh.n_shapes, 32, 80, seed=2), dict(resolutionA=0.01, resolutionH=0.01, **k)
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    return sh, synthetic.make_sequences(sh.n_shapes, 64, 150, seed=5), dict(resolutionZ=0.005, **k)


CASES = [(name, n) for name in WORKLOADS for n in SIZES] + [(name, n) for name in CAPACITY for n in (96, 2048)]


def rows_of(name, n):
    """(key in the golden file, tuning) of every row of one workload at one size"""
    return [(f"{name}/{n}/{t}", t) for t in ((0,) if name in CAPACITY else TUNINGS)]


def describe(name, n):
    """{key: kernel_info() string} of one workload's rows at one size, on whatever library irbpp_amd loads"""
    shapes, seqs, kw = workload(name)
    out = {}
    for key, tuning in rows_of(name, n):
        env = GpuPackingEnv(shapes, seqs[:64], n, device=DEV, tuning=tuning, **kw)
        try:
            out[key] = env.kernel_info()[1]
        finally:
            env.close()
    return out


def truthful(name, n, tuning, parent):
    """What the launcher does, in the rows where the hand-written description said something else (-> string, or None)."""
    split_pipeline = " + irbpp_trace_kernel" in parent
    # 1. IRBPP_TUNE_INLINE_POLYGON: every trace wave approximates its own borders and NO polygon kernel is launched; the
    #    description listed irbpp_polygon_kernel all the same.
    if (tuning & T.TUNE_INLINE_POLYGON) and split_pipeline:
        return parent.replace(" + irbpp_polygon_kernel", "")
    # 2. IRBPP_TUNE_CHAIN on a buffered environment of 2048 bins or more: the step's apply kernel is the wave-per-bin
    #    irbpp_apply_kernel there (a workgroup per bin only below 2048 bins); the description said irbpp_apply_wg_kernel at every size.
    if tuning == T.TUNE_CHAIN and name == "blockout_k10" and n >= 2048:
        return parent.replace("(step: irbpp_apply_wg_kernel alone)", "(step: irbpp_apply_kernel alone)")
    return None


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name,n", CASES)
def test_kernel_info_equals_the_parents(golden, name, n):
    assert torch.cuda.is_available()
    got = describe(name, n)
    corrected = 0
    for key, tuning in rows_of(name, n):
        parent = golden[key]
        want = truthful(name, n, tuning, parent)
        if want is not None:
            assert want != parent, key
            corrected += 1
        assert got[key] == (parent if want is None else want), key
    # the enumerated exceptions and no others: the three tunings with INLINE_POLYGON, CHAIN from 2048 bins of the k = 10 set on
    assert corrected == (0 if name in CAPACITY else 3 + (name == "blockout_k10" and n >= 2048))
    assert len(golden) == sum(len(rows_of(*case)) for case in CASES)
