"""The source of csrc/irbpp_streams_grad.hip compiled for the host (tests/host/streams_grad_host.cpp: the workgroup's threads in
lockstep, the dynamic LDS a heap block of the launch's own size, fmaf the C library's) against the definition as replay's CPU
form carries it (replay._streams_grad_backward_np, held to the explicit loops of tests/test_streams_grad_cpu.py there), bit for
bit: dx, dxg and the sixteen parameter gradients, over one and several staging trips, a second trip past 512 rows, widths that
are no multiple of four, the widest case, strided inputs, poisoned workspaces and outputs, a missing gradient on either side
and eval mode, without a GPU.  The same harness as a program of its own under -fsanitize=address,undefined, every buffer
exactly as large as the kernels may touch, runs once here; nothing of it is loaded into Python."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from irbpp_amd import replay
from host_harness import HERE, build_shared
from test_streams_grad_cpu import NAMES, SHAPES, effective, f32, make_case, same

SRC = os.path.join(HERE, "host", "streams_grad_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libstreams_grad_host.so")
LL, VP = C.c_longlong, C.c_void_p
POISON = f32(np.nan)


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    lib.host_streams_backward.argtypes = [VP, VP, C.c_int, C.c_int, C.c_int, VP, LL, VP, LL, LL, VP, VP, C.c_int, C.c_int, VP, VP, VP, VP]
    lib.host_streams_backward.restype = None
    lib.host_streams_backward_workspace.argtypes = [C.c_int] * 4
    lib.host_streams_backward_workspace.restype = LL
    return lib


def aligned(a):
    """a copy of the float32 array on a 16-byte boundary"""
    raw = np.empty(a.size + 4, dtype=f32)
    off = (-raw.ctypes.data % 16) // 4
    out = raw[off:off + a.size].reshape(a.shape)
    out[...] = a
    return out


def run(host, w, eps, x, xg, ga, gv, *, want_dx=True, misalign=False):
    """x and xg as slices of wider poisoned blocks, the workspace and every output poisoned -> (dx, dxg, {name: gradient})"""
    B, S, E = x.shape
    H, A = w[4].shape[0], w[6].shape[0]
    w = [aligned(t) if not misalign else aligned(np.concatenate([[0], t.ravel()]).astype(f32))[1:].reshape(t.shape) for t in w]
    wide = np.full((B, S + 1, E + 3), POISON, dtype=f32)
    wide[:, :S, 2:2 + E] = x
    xs = wide[:, :S, 2:2 + E]
    gwide = np.full((B, E + 5), POISON, dtype=f32)
    gwide[:, 1:1 + E] = xg
    xgs = gwide[:, 1:1 + E]
    ws = np.full(host.host_streams_backward_workspace(E, H, A, B) // 4, POISON, dtype=f32)
    dx, dxg = np.full((B, S, E), POISON, dtype=f32), np.full((B, E), POISON, dtype=f32)
    shapes = [(H, E), (H,), (A, H), (A,)] * 2
    outs = [np.full(shapes[(i // 4) * 2 + (i % 4) // 2], POISON, dtype=f32) for i in range(16)]
    ptr = lambda a: None if a is None else a.ctypes.data     # noqa: E731
    wp = (VP * 8)(*(ptr(t) for t in w))
    ep = None if eps is None else (VP * 8)(*(ptr(t) for t in eps))
    op = (VP * 16)(*(ptr(t) for t in outs))
    ga = None if ga is None else np.ascontiguousarray(ga)
    gv = None if gv is None else np.ascontiguousarray(gv)
    host.host_streams_backward(wp, ep, E, H, A, ptr(xgs), xgs.strides[0] // 4, ptr(xs), xs.strides[0] // 4, xs.strides[1] // 4, ptr(ga),
                               ptr(gv), S, B, ptr(ws), ptr(dx) if want_dx else None, ptr(dxg), op)
    wide[:, :S, 2:2 + E] = POISON
    gwide[:, 1:1 + E] = POISON
    assert np.isnan(wide).all() and np.isnan(gwide).all()
    return dx, dxg, dict(zip(NAMES, outs))


def check(got, want, eps_given=True, want_dx=True):
    if want_dx:
        same(got[0], want[0], "dx")
    else:
        assert np.isnan(got[0]).all()
    same(got[1], want[1], "dxg")
    for n in NAMES:
        if want[2][n] is None:
            assert not eps_given and np.isnan(got[2][n]).all(), n        # eval mode: the sigma outputs are left alone
        else:
            same(got[2][n], want[2][n], n)


@pytest.mark.parametrize("B,S,E,H,A", SHAPES + [(2, 513, 8, 8, 5), (1, 64, 256, 256, 128)])
def test_streams_grad_source_on_host(host, B, S, E, H, A):
    layers, x, xg, gv, ga = make_case(300 + S + E, B, S, E, H, A)
    w, eps = effective(layers)
    x, xg, gv, ga = (t.numpy() for t in (x, xg, gv, ga))
    want = replay._streams_grad_backward_np(x, xg, w, eps, ga, gv)
    check(run(host, w, eps, x, xg, ga, gv), want)
    if (E, H) in ((12, 36), (8, 8)):                         # the weights off the 16-byte boundary: element by element, the same bits
        check(run(host, w, eps, x, xg, ga, gv, misalign=True), want)


def test_missing_gradients_eval_mode_and_no_dx_on_host(host):
    B, S, E, H, A = 3, 37, 12, 9, 7
    layers, x, xg, gv, ga = make_case(55, B, S, E, H, A)
    w, eps = effective(layers)
    x, xg, gv, ga = (t.numpy() for t in (x, xg, gv, ga))
    check(run(host, w, eps, x, xg, ga, None), replay._streams_grad_backward_np(x, xg, w, eps, ga, None))
    check(run(host, w, eps, x, xg, None, gv), replay._streams_grad_backward_np(x, xg, w, eps, None, gv))
    check(run(host, w, eps, x, xg, None, None), replay._streams_grad_backward_np(x, xg, w, eps, None, None))
    check(run(host, w, eps, x, xg, ga, gv, want_dx=False), replay._streams_grad_backward_np(x, xg, w, eps, ga, gv), want_dx=False)
    we, _ = effective(layers, training=False)
    check(run(host, we, None, x, xg, ga, gv), replay._streams_grad_backward_np(x, xg, we, None, ga, gv), eps_given=False)


def test_negative_zero_and_dead_units_on_host(host):
    """Biases that switch most hidden units off and gradients with exact zeros: the +0 of a dead unit, of a chain from +0 and of
    an empty sum are the definition's."""
    B, S, E, H, A = 2, 33, 5, 6, 3
    layers, x, xg, gv, ga = make_case(56, B, S, E, H, A)
    with np.errstate(all="ignore"):
        layers[2].bias_mu.data -= 3.0
        layers[0].bias_mu.data -= 3.0
    w, eps = effective(layers)
    x, xg, gv, ga = (t.numpy() for t in (x, xg, gv, ga))
    ga[:, ::2] = -0.0
    gv[0] = 0.0
    want = replay._streams_grad_backward_np(x, xg, w, eps, ga, gv)
    assert (want[0] == 0).mean() > 0.3
    check(run(host, w, eps, x, xg, ga, gv), want)


def test_harness_runs_clean_under_the_sanitizers(tmp_path):
    """A program of its own (never loaded into Python): address and undefined-behaviour sanitizers over the kernels' source."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "streams_grad_host_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DSTREAMS_GRAD_HOST_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr)
    assert res.returncode == 0 and "checksum" in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr
