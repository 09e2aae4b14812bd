"""The shape branch with a gradient (csrc/irbpp_shapefeat_grad.hip, replay.shape_features_grad) without a GPU.

The arithmetic is defined (the header of irbpp_shapefeat_grad.hip); this file restates it with explicit loops
(``shape_grad_np``: shape by shape and feature by feature, every chain written out) and checks

* replay's CPU form (vectorised over the features) and the autograd wrapper against it, bit for bit: forward values (also
  against ``_shape_features_cpu``), the arg record, the four gradients; bad ids, a bad index, duplicate indices, exact ties;
* the definition against the reference's own lines (``Sequential(Linear, LeakyReLU, Linear, LeakyReLU)``, ``max(dim=1)[0]``,
  ``backward``) run by torch in float64: per gradient tensor within 4 * max(e_ref, 2^-24 max|ref64|), e_ref the float32 torch
  run's own error on the same inputs (the rule of tests/test_agent_golden_cpu.py).  The comparison presumes that both
  precisions route every gradient to the same point, which is asserted, never skipped: for every occurring (u, f) the float64
  gap between the best and the second-best distinct point exceeds 2^-18 |best|; the seeds were picked for that.

Observed error / scale (the bound is 4), definition beside torch float64, largest over the four tensors:
(H1, F, k) = (16, 32, 70): 1.22 (w2); (17, 33, 65): 3.40 (b1; the other three at most 1.57); (128, 128, 200): 1.91 (b1)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_shape_features_cpu import Linear, f32, f64, ids_np, key_np, leaky_np, make_encoder, make_points, shape_pre_np
from test_streams_cpu import fmaf_np

NAMES = ("w1", "b1", "w2", "b2")


# ------------------------------------------------------------------ the definition, with explicit loops ------------
def point_np(points, indices, u, j):
    i = indices[j]
    return points[u, i].astype(f32) if 0 <= i < points.shape[1] else np.full(3, np.nan, dtype=f32)


def shape_grad_np(points, indices, ids, W, g):
    """-> (out [M, F], arg [n_shapes, F], dict of the four gradients)."""
    n_shapes, k = points.shape[0], len(indices)
    H1, F_ = W["w1"].shape[0], W["w2"].shape[0]
    slope = f32(W["slope"])
    u_of = ids_np(ids, n_shapes)
    out = np.full((len(u_of), F_), np.nan, dtype=f32)
    arg = np.full((n_shapes, F_), -1, dtype=np.int32)
    G = np.zeros((n_shapes, F_), dtype=f32)
    grads = dict(w1=np.zeros((H1, 3), f32), b1=np.zeros(H1, f32), w2=np.zeros((F_, H1), f32), b2=np.zeros(F_, f32))
    with np.errstate(all="ignore"):
        for m, u in enumerate(u_of):
            if u >= 0:
                G[u] = G[u] + g[m]
        for u in sorted(set(int(v) for v in u_of if v >= 0)):
            s = shape_pre_np(points, indices, u, W)          # s_j[f] [k, F], point by point
            keys = key_np(s)
            for f in range(F_):
                arg[u, f] = min(j for j in range(k) if keys[j, f] == keys[:, f].max())
            out[u_of == u] = leaky_np(s[arg[u], np.arange(F_)], slope)
            first, first_b = np.zeros((H1, 3), f32), np.zeros(H1, f32)
            for f in range(F_):
                p = point_np(points, indices, u, arg[u, f])
                s1 = W["b1"].copy()
                for c in range(3):
                    s1 = fmaf_np(p[c], W["w1"][:, c], s1)
                h1 = leaky_np(s1, slope)
                s2 = W["b2"][f]
                for i in range(H1):
                    s2 = fmaf_np(h1[i], W["w2"][f, i], s2)
                d2 = G[u, f] if s2 > 0 else f32(slope * G[u, f])
                grads["b2"][f] = grads["b2"][f] + d2
                grads["w2"][f] = fmaf_np(d2, h1, grads["w2"][f])
                e = (d2 * W["w2"][f]).astype(f32)
                ds1 = np.where(s1 > 0, e, slope * e).astype(f32)
                for c in range(3):
                    first[:, c] = fmaf_np(ds1, p[c], first[:, c])
                first_b = first_b + ds1
            grads["w1"], grads["b1"] = grads["w1"] + first, grads["b1"] + first_b
    nan = np.isnan(out)
    out[nan] = np.uint32(0x7fc00000).view(f32)
    return out, arg, grads


def layers_of(W, dev="cpu"):
    l1, l2 = nn.Linear(3, W["w1"].shape[0]), nn.Linear(W["w1"].shape[0], W["w2"].shape[0])
    with torch.no_grad():
        for t, n in ((l1.weight, "w1"), (l1.bias, "b1"), (l2.weight, "w2"), (l2.bias, "b2")):
            t.copy_(torch.from_numpy(W[n]))
    return l1.to(dev), l2.to(dev)


def grads_of(l1, l2):
    return dict(zip(NAMES, (t.grad.detach().cpu().numpy() for t in (l1.weight, l1.bias, l2.weight, l2.bias))))


def run_wrapper(points, indices, ids, W, g, dev="cpu", use_hip=None):
    """replay.shape_features_grad and a backward from g -> (out, arg, gradients) as numpy."""
    sp = replay.ShapePoints(points, dev)
    l1, l2 = layers_of(W, dev)
    out, arg = replay.shape_features_grad(torch.as_tensor(ids).to(dev), sp, torch.from_numpy(np.asarray(indices)).to(dev), l1, l2, W["slope"],
                                          use_hip=use_hip, return_arg=True)
    assert out.requires_grad and out.grad_fn is not None and out.dtype == torch.float32 and not arg.requires_grad
    out.backward(torch.from_numpy(g).to(dev))
    return out.detach().cpu().numpy(), arg.cpu().numpy(), grads_of(l1, l2)


def same(a, b, what=""):
    """the same bits, NaNs compared by position"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=what)
    np.testing.assert_array_equal(np.where(np.isnan(a), 0, a).view(np.uint32), np.where(np.isnan(b), 0, b).view(np.uint32), err_msg=what)


def make_case(seed, n_shapes, P, k, H1, F_, M, b2_shift=0.0):
    rng = np.random.default_rng(seed)
    points = make_points(rng, n_shapes, P)
    W = make_encoder(rng, H1, F_, b2_shift=b2_shift)
    indices = rng.integers(0, P, k).astype(np.int32)
    ids = rng.integers(0, n_shapes, M).astype(np.int64)
    g = rng.standard_normal((M, F_)).astype(f32)
    return points, W, indices, ids, g


@pytest.fixture(scope="module")
def small():
    points, W, indices, ids, g = make_case(11, 5, 40, 37, 9, 6, 9)
    W["b2"][1] = -50.0                                       # a feature whose every activation is negative: the slope side of d2
    indices[:5] = [0, 39, 7, 7, 0]
    ids[:] = [3, 0, 3, 4, 0, 3, 1, -1, 5]                     # shape 2 does not occur; two bad ids
    return points, W, indices, ids, g, shape_grad_np(points, indices, ids, W, g)


# ------------------------------------------------------------------ the CPU form ------------
def test_cpu_form_is_the_definition(small):
    points, W, indices, ids, g, (out, arg, grads) = small
    got_out, got_arg, got = run_wrapper(points, indices, ids, W, g)
    same(got_out, out, "forward")
    np.testing.assert_array_equal(got_arg, arg)
    assert (arg[2] == -1).all() and (arg[[0, 1, 3, 4]] >= 0).all() and arg.dtype == np.int32
    for n in NAMES:
        same(got[n], grads[n], n)
        assert np.abs(grads[n]).max() > 0
    assert np.isnan(out[7]).all() and np.isnan(out[8]).all() and not np.isnan(out[:7]).any()
    # the forward's bits are shape_features'
    sp, w = replay.ShapePoints(points, "cpu"), replay.ShapeEncoderWeights.from_layers(Linear(W["w1"], W["b1"]), Linear(W["w2"], W["b2"]), W["slope"])
    plain = replay._shape_features_cpu(torch.from_numpy(ids), sp, torch.from_numpy(indices), w).numpy()
    np.testing.assert_array_equal(got_out.view(np.uint32), plain.view(np.uint32))
    np.testing.assert_array_equal(plain.view(np.uint32), replay.shape_features(torch.from_numpy(ids), sp, torch.from_numpy(indices), w).numpy().view(np.uint32))
    assert (got["b2"][1] != 0) and replay.SHAPE_GRAD_HIP_DEFAULT in (False, True)


def test_a_bad_ids_row_leaves_the_gradient_unchanged(small):
    points, W, indices, ids, g, (out, arg, grads) = small
    keep = ids_np(ids, points.shape[0]) >= 0
    g2 = g.copy()
    g2[~keep] = 1e6                                          # whatever arrives for a NaN row
    _, _, got = run_wrapper(points, indices, ids, W, g2)
    _, arg3, got3 = run_wrapper(points, indices, ids[keep], W, g[keep])       # the rows taken out altogether
    np.testing.assert_array_equal(arg3, arg)
    for n in NAMES:
        same(got[n], grads[n], n)
        same(got3[n], grads[n], n)
    # float ids, truncated toward zero, as a strided column; NaN and infinite ids are bad ids
    obs = torch.full((len(ids), 7), 1e30)
    obs[:, 2] = torch.from_numpy(ids.astype(f32) + np.where(ids >= 0, f32(0.75), f32(0)))
    obs[7, 2], obs[8, 2] = float("nan"), float("inf")
    out_f, arg_f, got_f = run_wrapper(points, indices, obs[:, 2], W, g)
    same(out_f, out)
    np.testing.assert_array_equal(arg_f, arg)
    for n in NAMES:
        same(got_f[n], grads[n], n)


def test_duplicates_of_the_winning_point_change_nothing(small):
    """Every index appended once more (exact ties at a later position), and the winners' indices put in front: the arg moves
    to the smallest position of the same point, the gradients keep their bits."""
    points, W, indices, ids, g, (out, arg, grads) = small
    doubled = np.concatenate([indices, indices])
    out2, arg2, got2 = run_wrapper(points, doubled, ids, W, g)
    same(out2, out)
    np.testing.assert_array_equal(arg2, arg)                 # never the later copy
    winners = np.unique(indices[arg[arg >= 0]])
    front = np.concatenate([winners, indices]).astype(np.int32)
    out3, arg3, got3 = run_wrapper(points, front, ids, W, g)
    same(out3, out)
    occ = arg[:, 0] >= 0
    assert (arg3[occ] < len(winners)).all()
    np.testing.assert_array_equal(front[arg3[occ]], indices[arg[occ]])
    dedup, first_at = np.unique(indices, return_index=True)
    out4, arg4, got4 = run_wrapper(points, indices[np.sort(first_at)], ids, W, g)      # the de-duplicated index set
    same(out4, out)
    for n in NAMES:
        same(got2[n], grads[n], n)
        same(got3[n], grads[n], n)
        same(got4[n], grads[n], n)


def test_exact_tie_between_two_points_and_a_bad_index(small):
    points, W, indices, ids, g, (out, arg, grads) = small
    tied = points.copy()
    win = int(indices[arg[3, 0]])
    other = (win + 1) % points.shape[1]
    tied[3, other] = tied[3, win]                            # another row of the table with the same coordinates
    idx = np.concatenate([[other], indices]).astype(np.int32)
    want = shape_grad_np(tied, idx, ids, W, g)
    assert want[1][3, 0] == 0                                # the smallest j decides, whichever point it is
    got = run_wrapper(tied, idx, ids, W, g)
    same(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    for n in NAMES:
        same(got[2][n], want[2][n], n)
    bad = indices.copy()
    bad[11] = points.shape[1]                                # a NaN point: the NaN key is the largest, every arg is 11
    want = shape_grad_np(points, bad, ids, W, g)
    got = run_wrapper(points, bad, ids, W, g)
    assert np.isnan(want[0]).all() and (want[1][[0, 1, 3, 4]] == 11).all() and np.isnan(want[2]["w2"]).all()
    same(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    for n in NAMES:
        same(got[2][n], want[2][n], n)


def test_gradients_accumulate_and_arguments_are_checked(small):
    points, W, indices, ids, g, (out, arg, grads) = small
    sp = replay.ShapePoints(points, "cpu")
    l1, l2 = layers_of(W)
    for _ in range(2):
        replay.shape_features_grad(torch.from_numpy(ids[:7]), sp, torch.from_numpy(indices), l1, l2).backward(torch.from_numpy(g[:7]))
    once = run_wrapper(points, indices, ids[:7], W, g[:7])[2]
    for n, t in zip(NAMES, (l1.weight, l1.bias, l2.weight, l2.bias)):
        same(t.grad.numpy(), once[n] + once[n], n)
    two = replay.shape_features_grad(torch.from_numpy(ids[:6].reshape(2, 3)), sp, torch.from_numpy(indices), l1, l2)
    assert tuple(two.shape) == (6, 6)
    with pytest.raises(RuntimeError, match="HIP device"):
        replay.shape_features_grad(torch.from_numpy(ids), sp, torch.from_numpy(indices), l1, l2, use_hip=True)
    with pytest.raises(ValueError):
        replay.shape_features_grad(torch.from_numpy(ids), sp, torch.from_numpy(indices), l2, l1)
    with pytest.raises(ValueError):
        replay.shape_features_grad(torch.from_numpy(ids), sp, torch.zeros(0, dtype=torch.int32), l1, l2)


# ------------------------------------------------------------------ the definition against the reference's lines ------------
def reference_grads(points, indices, ids, W, g, dtype, dev="cpu"):
    """The reference's own lines by torch in `dtype` -> (shape_feature, the four gradients) as float64 numpy."""
    l1, l2 = layers_of(W)
    enc = nn.Sequential(l1, nn.LeakyReLU(W["slope"]), l2, nn.LeakyReLU(W["slope"])).to(dtype=dtype, device=dev)
    x = torch.from_numpy(points[ids][:, indices]).to(dtype=dtype, device=dev)
    feat = torch.max(enc(x), dim=1)[0]
    feat.backward(torch.from_numpy(g).to(dtype=dtype, device=dev))
    return feat.detach().double().cpu().numpy(), {n: t.astype(f64) for n, t in grads_of(enc[0], enc[2]).items()}


def assert_gaps(points, indices, ids, W):
    """For every occurring (u, f): the float64 gap between the best and the second-best distinct point > 2^-18 |best|."""
    smallest = np.inf
    distinct = np.unique(indices)
    for u in np.unique(ids):
        p = points[u][distinct].astype(f64)
        s1 = p @ W["w1"].astype(f64).T + W["b1"].astype(f64)
        s2 = np.where(s1 > 0, s1, W["slope"] * s1) @ W["w2"].astype(f64).T + W["b2"].astype(f64)
        top = np.sort(s2, axis=0)[-2:]
        rel = (top[1] - top[0]) / np.abs(top[1])
        smallest = min(smallest, rel.min())
        assert (rel > 2.0 ** -18).all(), f"shape {u}: a gap of {rel.min():.3g} |best|; pick another seed"
    return smallest


REFERENCE_CASES = [(21, 4, 60, 70, 16, 32, 12), (22, 4, 60, 65, 17, 33, 12), (24, 3, 300, 200, 128, 128, 20)]


@pytest.mark.parametrize("seed,n_shapes,P,k,H1,F_,M", REFERENCE_CASES)
def test_definition_against_the_reference(seed, n_shapes, P, k, H1, F_, M):
    points, W, indices, ids, g = make_case(seed, n_shapes, P, k, H1, F_, M)
    gap = assert_gaps(points, indices, ids, W)
    feat64, ref64 = reference_grads(points, indices, ids, W, g, torch.float64)
    _, ref32 = reference_grads(points, indices, ids, W, g, torch.float32)
    out, _, got = run_wrapper(points, indices, ids, W, g)
    assert np.abs(out - feat64).max() < 1e-4
    worst = 0.0
    for n in NAMES:
        e_ref = np.abs(ref32[n] - ref64[n]).max()
        scale = max(e_ref, 2.0 ** -24 * np.abs(ref64[n]).max())
        err = np.abs(got[n].astype(f64) - ref64[n]).max()
        worst = max(worst, err / scale)
        print(f"{n}: error {err:.3g}, e_ref {e_ref:.3g}, error / scale {err / scale:.3f} (smallest gap {gap:.3g} |best|)")
        assert err <= 4 * scale, f"{n}: error {err:.3g} beside 4 x {scale:.3g}"
    print(f"(H1, F, k) = ({H1}, {F_}, {k}): largest error / scale {worst:.2f}")
