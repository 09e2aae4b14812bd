"""The source of csrc/irbpp_optim.hip compiled for the host (tests/host/optim_host.cpp: 256 threads in lockstep per workgroup,
barriers as real barriers, the double shuffle of tests/host/optim_lockstep.h) against the numpy definition of
tests/test_clipped_adam_cpu.py, bit for bit and without a GPU: the chunk walk, the order of the float64 additions, the
16-byte / dword choice by the bases' alignment, the flags and the skipped step.  The tensor set is that of
tests/test_gpu_clipped_adam.py (SPEC: the chunk edge, the odd tail, bases that are 4-byte aligned only, more than 256
chunks); every array lies between poison."""
import ctypes as C
import os

import numpy as np
import pytest

from host_harness import build_shared
from test_clipped_adam_cpu import BETAS, CLIP_ONLY, EPS, LR, SYNC, WRITE, ZERO, bits_equal, f32, step_def
from test_gpu_clipped_adam import ACTIVE, SPEC, case_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "optim_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "liboptim_host.so")
POISON = f32(-5.0)


class Tensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("target", C.c_void_p), ("numel", C.c_int64)]


class Hyper(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("step_size", "rsq", "beta1", "one_minus_beta1", "beta2", "one_minus_beta2", "eps", "max_norm")] + \
               [("flags", C.c_int32)]


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_optim_chunk.restype = C.c_int
    lib.host_clipped_adam_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(Hyper), C.c_void_p, C.c_void_p]
    lib.host_clipped_adam_step.restype = C.c_int
    return lib


def placed(values, misalign):
    """-> (backing, view): `values` copied to an address that is 4 * misalign past a multiple of 16, 8 poison floats around."""
    back = np.full(values.size + 24, POISON, dtype=f32)
    start = 8 + (-(back.ctypes.data // 4 + 8) + misalign) % 4
    view = back[start:start + values.size]
    assert view.ctypes.data % 16 == 4 * misalign
    view[:] = values
    return back, view


def poison_intact(back, view):
    start = (view.ctypes.data - back.ctypes.data) // 4
    return (back[:start] == POISON).all() and (back[start + view.size:] == POISON).all()


def hyper_at(t, max_norm, flags):
    return Hyper(f32(LR / (1.0 - BETAS[0] ** t)), f32(np.sqrt(1.0 - BETAS[1] ** t)), f32(BETAS[0]), f32(1.0 - BETAS[0]), f32(BETAS[1]),
                 f32(1.0 - BETAS[1]), f32(EPS), f32(max_norm), flags)


class HostRun(object):
    """The ACTIVE tensors of SPEC in host memory, each array at the alignment its kind asks for, and their tables."""

    def __init__(self, params, with_target=True):
        self.arrays = []                                  # per active tensor: [(backing, view)] for p, g, m, v, target
        table, chunks = (Tensor * len(ACTIVE))(), []
        for k, i in enumerate(ACTIVE):
            kind, n = SPEC[i][1], params[i].size
            mis = {"view": (1, 0, 0, 0, 0), "gview": (0, 3, 0, 0, 0)}.get(kind, (0, 0, 0, 0, 0))
            vals = (params[i], np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32), np.full(n, 7.0, f32))
            arr = [placed(v, m) for v, m in zip(vals, mis)]
            self.arrays.append(arr)
            table[k] = Tensor(*[a[1].ctypes.data for a in arr[:4]], arr[4][1].ctypes.data if with_target else None, n)
            chunks += [(k, first) for first in range(0, n, 1024)]
        self.table, self.chunks = table, np.array(chunks, dtype=np.int32)
        self.partial = np.full(len(chunks) + 2, -5.0)
        self.total, self.skipped = np.full(3, POISON), np.array([-1, 0, -1], dtype=np.int64)

    def step(self, lib, gs, t, max_norm, flags):
        for arr, i in zip(self.arrays, ACTIVE):
            arr[1][1][:] = gs[i]
        h = hyper_at(t, max_norm, flags)
        rc = lib.host_clipped_adam_step(C.addressof(self.table), len(ACTIVE), self.chunks.ctypes.data, len(self.chunks),
                                        self.partial[1:].ctypes.data, C.byref(h), self.total[1:].ctypes.data, self.skipped[1:].ctypes.data)
        assert rc == 0
        assert all(poison_intact(*a) for arr in self.arrays for a in arr), "a store outside a tensor"
        assert self.partial[0] == -5.0 and self.partial[-1] == -5.0 and self.total[0] == POISON and self.total[2] == POISON
        assert self.skipped[0] == -1 and self.skipped[2] == -1
        return self.total[1]

    def column(self, j):
        return [arr[j][1] for arr in self.arrays]


def test_the_case_covers_what_it_is_meant_to(host):
    assert host.host_optim_chunk() == 1024
    sizes = [int(np.prod(SPEC[i][0])) for i in ACTIVE]
    assert {1, 3, 1023, 1024, 1025, 4099} <= set(sizes) and sum((n + 1023) // 1024 for n in sizes) > 256
    assert {SPEC[i][1] for i in ACTIVE} == {"plain", "view", "gview"}


# one step each: a workgroup costs 256 host threads here, and the set has 280 of them per launch
@pytest.mark.parametrize("flags,max_norm,t", [(WRITE, 1.0, 1), (ZERO | SYNC, 1.0, 3), (WRITE | SYNC, 1e6, 2), (ZERO, 1e6, 1), (CLIP_ONLY, 1.0, 1)])
def test_step_source_on_host(host, flags, max_norm, t):
    params, grads = case_arrays(10 + flags, steps=1)
    run = HostRun(params)
    rng = np.random.default_rng(5)
    for arr in run.arrays:                                # moments as after earlier steps: v >= 0
        arr[2][1][:] = rng.standard_normal(arr[2][1].size).astype(f32) * f32(0.01)
        arr[3][1][:] = np.abs(rng.standard_normal(arr[3][1].size)).astype(f32) * f32(1e-4)
    want = [[a.copy() for a in run.column(j)] for j in range(5)]
    want[1] = [grads[0][i].copy() for i in ACTIVE]
    total = run.step(host, grads[0], t, max_norm, flags)
    want_total, skipped = step_def(want[0], want[1], want[2], want[3], LR, BETAS, EPS, max_norm, t, flags, want[4])
    assert skipped == 0 and run.skipped[1] == 0
    bits_equal(total, want_total, "total")
    for j, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq", "target")):
        for k in range(len(ACTIVE)):
            bits_equal(run.column(j)[k], want[j][k], f"{name} of tensor {ACTIVE[k]}")
    if flags & SYNC:
        assert all((a == b).all() for a, b in zip(run.column(4), run.column(0)))
    else:
        assert all((a == 7.0).all() for a in run.column(4))


@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_skipped_step_source_on_host(host, bad):
    params, grads = case_arrays(20, steps=1)
    grads[0][ACTIVE[-1]][269311] = bad
    run = HostRun(params, with_target=False)
    before = [[a.copy() for a in run.column(j)] for j in range(5)]
    before[1] = [grads[0][i].copy() for i in ACTIVE]
    total = run.step(host, grads[0], 1, 1.0, WRITE | SYNC)
    assert run.skipped[1] == 1
    assert int(np.asarray(total).view(np.uint32)) == (0x7fc00000 if np.isnan(bad) else 0x7f800000)
    for j in range(5):
        for a, b in zip(run.column(j), before[j]):
            bits_equal(a, b, "a skipped step must change nothing")
