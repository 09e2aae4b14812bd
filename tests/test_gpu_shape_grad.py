"""csrc/irbpp_shapefeat_grad.hip on the GPU, bit for bit against the definition as replay's CPU form carries it (held to the
explicit loops in tests/test_shape_grad_cpu.py): the forward's values (also against irbpp_shape_features on the device), the arg
record and the four gradients, through replay.shape_features_grad(use_hip=True) and through the C ABI on a stream of the
test's own with every workspace poisoned.

Shapes: n_shapes 5, P 70, k of {1, 63, 64, 65, 130} (below, at and above one wave of points; 130 gives three chunks) times (H1, F)
of {(1, 1), (16, 32), (17, 33), (128, 128), (256, 256)} (one full block, short blocks, the widest), M of {1, 7, 200} rotating so
that every k and every width meets every M.  Id and index cases: shapes that do not occur, ids -1, n_shapes and float NaN, a
strided float id column of an observation, an out-of-range index (NaN positions compared), forced duplicates, an exact tie
between two rows of the table.  One mid-size case (n_shapes 12, k 256, M 640) against torch's autograd on the device in float64,
within 4 * max(e_ref, 2^-24 max|ref64|), e_ref the device's float32 run (the rule and the gap condition of
tests/test_shape_grad_cpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_shape_features_cpu import f32, f64, ids_np, make_encoder, make_points, weights_of
from test_shape_grad_cpu import NAMES, assert_gaps, layers_of, make_case, reference_grads, run_wrapper, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 1e30
KS, WIDTHS, MS = (1, 63, 64, 65, 130), ((1, 1), (16, 32), (17, 33), (128, 128), (256, 256)), (1, 7, 200)
CASES = [(k, H1, F_, MS[(a + b) % 3]) for a, k in enumerate(KS) for b, (H1, F_) in enumerate(WIDTHS)]


def definition(points, indices, ids, W, g):
    u = ids_np(ids, points.shape[0])
    idx = np.asarray(indices, np.int64)
    w = [W[n] for n in NAMES]
    out, arg = replay._shape_grad_forward_np(points, idx, u, *w, W["slope"])
    return out, arg, dict(zip(NAMES, replay._shape_grad_backward_np(points, idx, u, *w, W["slope"], arg, g)))


def check(got, want):
    same(got[0], want[0], "forward")
    np.testing.assert_array_equal(got[1], want[1])
    for n in NAMES:
        same(got[2][n], want[2][n], n)


@functools.lru_cache(maxsize=None)
def case(k, H1, F_, M, n_shapes=5, P=70):
    """-> points, W, indices, ids, g and the definition's results: computed once and shared (treat as read-only)."""
    points, W, indices, ids, g = make_case(3000 + 1000 * k + 7 * H1 + F_ + M, n_shapes, P, k, H1, F_, M)
    indices[0], indices[-1] = P - 1, 0
    if k > 4:
        indices[2] = indices[3]                              # a duplicate for certain
    if M == 1:
        ids[0] = n_shapes - 1
    else:
        ids[ids == 2] = 3                                    # shape 2 does not occur
        ids[1], ids[3] = -1, n_shapes
    return points, W, indices, ids, g, definition(points, indices, ids, W, g)


@pytest.mark.parametrize("k,H1,F_,M", CASES)
def test_kernels_are_the_definition(k, H1, F_, M):
    points, W, indices, ids, g, want = case(k, H1, F_, M)
    got = run_wrapper(points, indices, ids, W, g, DEV, True)
    check(got, want)
    assert (got[0].view(np.uint32)[np.isnan(got[0])] == 0x7fc00000).all()
    sp = replay.ShapePoints(points, DEV)                     # the forward's bits are irbpp_shape_features'
    plain = replay.shape_features(torch.from_numpy(ids).to(DEV), sp, torch.from_numpy(indices).to(DEV), weights_of(W, DEV), use_hip=True)
    np.testing.assert_array_equal(plain.cpu().numpy().view(np.uint32), got[0].view(np.uint32))
    if M > 1:
        assert (want[1][2] == -1).all() and np.isnan(want[0][1]).all() and np.isnan(want[0][3]).all()


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


def test_c_abi_on_its_own_stream_with_poisoned_workspaces():
    """ids a float column of a poisoned observation block with a NaN id, out a slice of a poisoned wider tensor, all four
    workspaces poisoned: rows of shapes that do not occur are never written, nothing around the arguments is."""
    from irbpp_amd import _lib as L
    lib = L.load()
    points, W, indices, ids, g, _ = case(130, 17, 33, 200)
    n_shapes, P, k, H1, F_, M = 5, 70, 130, 17, 33, 200
    fids = ids.astype(f32) + np.where(ids >= 0, f32(0.75), f32(0))
    fids[5] = np.nan
    want = definition(points, indices, fids, W, g)
    chunks = lib.irbpp_shape_features_chunks(n_shapes, k)
    assert chunks == 3
    pts, idx = torch.from_numpy(points).to(DEV), torch.from_numpy(indices).to(DEV)
    block = torch.full((M, 13), POISON, dtype=torch.float32, device=DEV)
    block[:, 5] = torch.from_numpy(fids).to(DEV)
    before = block.clone()
    wide = torch.full((M + 2, F_ + 7), POISON, dtype=torch.float32, device=DEV)
    pkey = torch.full((n_shapes, chunks, F_), 0x12345678, dtype=torch.int32, device=DEV)
    pj = torch.full((n_shapes, chunks, F_), 7777, dtype=torch.int32, device=DEV)
    arg = torch.full((n_shapes + 2, F_), 7777, dtype=torch.int32, device=DEV)
    pd = torch.full((n_shapes + 2, F_, 4), POISON, dtype=torch.float32, device=DEV)
    first = torch.full((n_shapes + 2, H1, 4), POISON, dtype=torch.float32, device=DEV)
    keep = [torch.from_numpy(np.ascontiguousarray(W[n])).to(DEV) for n in NAMES]
    d = [torch.full((t.numel() + 8,), POISON, dtype=torch.float32, device=DEV) for t in keep]
    gg = torch.from_numpy(g).to(DEV)
    enc = replay._IrbppShapeEncoder(*(t.data_ptr() for t in keep), H1, F_, W["slope"])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        s = C.c_void_p(stream.cuda_stream)
        L.check(lib.irbpp_shape_features_arg(_ptr(pts), n_shapes, P, _ptr(idx), k, _ptr(block, 5), 1, 13, M, C.byref(enc), _ptr(pkey), _ptr(pj),
                                             chunks, _ptr(wide, F_ + 7 + 3), F_ + 7, _ptr(arg, F_), s), "irbpp_shape_features_arg")
        L.check(lib.irbpp_shape_features_backward(_ptr(pts), n_shapes, P, _ptr(idx), k, _ptr(block, 5), 1, 13, M, C.byref(enc), _ptr(arg, F_),
                                                  _ptr(gg), _ptr(pd, 4 * F_), _ptr(first, 4 * H1), *(_ptr(t, 4) for t in d), s),
                "irbpp_shape_features_backward")
    stream.synchronize()
    assert torch.equal(block.view(torch.int32), before.view(torch.int32))
    out = wide[1:1 + M, 3:3 + F_].cpu().numpy()
    wide[1:1 + M, 3:3 + F_] = POISON
    assert bool((wide == POISON).all())
    got = {n: t[4:-4].cpu().numpy().reshape(W[n].shape) for n, t in zip(NAMES, d)}
    check((out, arg[1:-1].cpu().numpy(), got), want)
    for t in d:
        assert bool((t[:4] == POISON).all()) and bool((t[-4:] == POISON).all())
    assert bool((arg[0] == 7777).all()) and bool((arg[-1] == 7777).all())
    present = set(ids_np(fids, n_shapes).tolist()) - {-1}
    assert present == {0, 1, 3, 4}
    for u in range(n_shapes):
        for ws in (pkey[u], pd[1 + u], first[1 + u]):
            assert bool((ws == ws.new_tensor(0x12345678 if ws.dtype == torch.int32 else POISON)).all()) == (u not in present), u
    assert bool((pd[0] == POISON).all()) and bool((pd[-1] == POISON).all()) and bool((first[0] == POISON).all()) and bool((first[-1] == POISON).all())
    # status codes: before any launch
    assert lib.irbpp_shape_features_arg(_ptr(pts), n_shapes, P, _ptr(idx), k, _ptr(block, 5), 1, 13, M, C.byref(enc), _ptr(pkey), _ptr(pj),
                                        chunks + 1, _ptr(wide), F_ + 7, _ptr(arg), None) == -1
    assert lib.irbpp_shape_features_backward(_ptr(pts), n_shapes, P, _ptr(idx), k, _ptr(block, 5), 1, 13, M, C.byref(enc), _ptr(arg), _ptr(gg),
                                             _ptr(pd, 1), _ptr(first), *(_ptr(t) for t in d), None) == -1      # a misaligned workspace


def test_float_id_column_bad_index_duplicates_and_a_tie():
    points, W, indices, ids, g, want = case(130, 17, 33, 7)
    obs = torch.full((7, 13), POISON, dtype=torch.float32, device=DEV)
    fids = np.array([0.5, np.nan, 4.99, 5.0, -1.0, -0.5, 3.0], dtype=f32)
    obs[:, 9] = torch.from_numpy(fids).to(DEV)
    assert obs[:, 9].stride(0) == 13
    check(run_wrapper(points, indices, obs[:, 9], W, g, DEV, True), definition(points, indices, fids, W, g))
    bad = indices.copy()
    bad[64] = 70                                             # the first point of the second chunk
    w_bad = definition(points, bad, ids, W, g)
    occ, u0 = want[1][:, 0] >= 0, int(ids[0])                # the shapes that occur; one of them
    assert np.isnan(w_bad[0]).all() and (w_bad[1][occ] == 64).all() and (w_bad[1][~occ] == -1).all() and np.isnan(w_bad[2]["w2"]).all()
    check(run_wrapper(points, bad, ids, W, g, DEV, True), w_bad)
    dup = indices.copy()
    dup[[0, 63, 64, 100, 129]] = indices[want[1][u0, 0]]     # the winner of (u0, 0) in the first and last lanes of trips and chunks
    w_dup = definition(points, dup, ids, W, g)
    assert w_dup[1][u0, 0] == 0
    check(run_wrapper(points, dup, ids, W, g, DEV, True), w_dup)
    far = points.copy()
    far[:, [11, 12]] = 30.0                                  # two rows of the table with the same coordinates, which win many features
    idx = np.where((indices == 11) | (indices == 12), 13, indices).astype(np.int32)
    idx[[70, 128, 129]] = [12, 12, 11]                       # sampled in the second chunk and twice in the third: the smallest j decides
    w_far = definition(far, idx, ids, W, g)
    assert (w_far[1][u0] == 70).mean() > 0.25 and not (w_far[1] >= 128).any()
    check(run_wrapper(far, idx, ids, W, g, DEV, True), w_far)


def test_two_calls_give_the_same_bits_and_gradients_accumulate():
    points, W, indices, ids, g, want = case(130, 128, 128, 200)
    a, b = (run_wrapper(points, indices, ids, W, g, DEV, True) for _ in range(2))
    check(a, b)
    check(a, want)
    sp = replay.ShapePoints(points, DEV)
    l1, l2 = layers_of(W, DEV)
    for _ in range(2):                                       # into the .grad the first backward left
        replay.shape_features_grad(torch.from_numpy(ids).to(DEV), sp, torch.from_numpy(indices).to(DEV), l1, l2, use_hip=True).backward(
            torch.from_numpy(g).to(DEV))
    for n, t in zip(NAMES, (l1.weight, l1.bias, l2.weight, l2.bias)):
        same(t.grad.cpu().numpy(), want[2][n] + want[2][n], n)
    # the torch form on the device: a grad_fn, close to the definition
    l1, l2 = layers_of(W, DEV)
    out = replay.shape_features_grad(torch.from_numpy(ids).to(DEV), sp, torch.from_numpy(indices).to(DEV), l1, l2, use_hip=False)
    assert out.grad_fn is not None
    np.testing.assert_array_equal(np.isnan(out.detach().cpu().numpy()), np.isnan(want[0]))
    keep = ~np.isnan(want[0])
    assert np.abs(out.detach().cpu().numpy()[keep] - want[0][keep]).max() < 1e-4


def test_mid_size_against_the_devices_autograd_in_float64():
    points, W, indices, ids, g = make_case(41, 12, 500, 256, 128, 128, 640)
    gap = assert_gaps(points, indices, ids, W)
    _, ref64 = reference_grads(points, indices, ids, W, g, torch.float64, DEV)
    _, ref32 = reference_grads(points, indices, ids, W, g, torch.float32, DEV)
    _, _, got = run_wrapper(points, indices, ids, W, g, DEV, True)
    for n in NAMES:
        e_ref = np.abs(ref32[n] - ref64[n]).max()
        scale = max(e_ref, 2.0 ** -24 * np.abs(ref64[n]).max())
        err = np.abs(got[n].astype(f64) - ref64[n]).max()
        print(f"{n}: error {err:.3g}, e_ref {e_ref:.3g}, error / scale {err / scale:.3f} (smallest gap {gap:.3g} |best|)")
        assert err <= 4 * scale, f"{n}: error {err:.3g} beside 4 x {scale:.3g}"
