"""The optimiser step's definition (csrc/irbpp_optim.hip's header) restated in numpy, chunk by chunk as the kernels walk it,
and held against three things without a GPU: torch's own clip_grad_norm_ + optim.Adam (how far float32 rounding order lets
them differ, measured against the same lines in float64), the vectorised form irbpp_amd/optim.py runs on the CPU (bit for
bit), and ClippedAdam's behaviour around it (flags, the skipped step, checkpoints in torch's layout, the table rebuild).

Measured with the inputs below (largest absolute parameter error after 4 steps against the float64 run):
clip active e_torch 4.089e-07, e_def 4.185e-07 (ratio 1.023); clip inactive e_torch 4.235e-07, e_def 4.235e-07 (ratio 1.000);
clip_only, on the gradients: 2.850e-09 both."""
import copy

import numpy as np
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

from irbpp_amd import optim as O
from irbpp_amd.optim import ClippedAdam
from irbpp_amd.replay import _fmaf_np

f32, f64 = np.float32, np.float64
CHUNK = 1024
WRITE, ZERO, SYNC, CLIP_ONLY = 1, 2, 4, 8
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1.5e-4


# ---- the definition --------------------------------------------------------------------------------------------------------
def block_sum(s):
    """256 float64, one per thread -> the workgroup's value: butterfly within each wave (o = 1 .. 32), ((w0+w1)+w2)+w3."""
    w = []
    for k in range(4):
        x = s[64 * k:64 * k + 64].copy()
        for o in (1, 2, 4, 8, 16, 32):
            x = x + x[np.arange(64) ^ o]
        w.append(x[0])
    return ((w[0] + w[1]) + w[2]) + w[3]


def chunk_table(sizes):
    return [(k, first) for k, n in enumerate(sizes) for first in range(0, n, CHUNK)]


def sumsq_def(grads):
    with np.errstate(all="ignore"):
        partial = []
        for k, first in chunk_table([g.size for g in grads]):
            q = np.zeros(CHUNK, dtype=f64)                                  # +0.0 past the end
            part = grads[k][first:first + CHUNK].astype(f64)
            q[:part.size] = part * part
            q = q.reshape(256, 4)                                           # thread t: elements 4t .. 4t+3
            partial.append(block_sum(((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]))
        s = np.zeros(256, dtype=f64)
        for i, x in enumerate(partial):                                     # thread t: partial t, t + 256, .. ascending
            s[i % 256] = s[i % 256] + x
        return f64(block_sum(s))


def step_def(params, grads, ms, vs, lr, betas, eps, max_norm, t, flags, targets=None):
    """One step of the definition on lists of flat float32 arrays, in place -> (total, skipped)."""
    with np.errstate(all="ignore"):
        s = sumsq_def(grads)
        bits = int(np.asarray(s).view(np.uint64))
        if (bits >> 52) & 0x7ff == 0x7ff:
            return np.array(0x7fc00000 if bits & ((1 << 52) - 1) else 0x7f800000, dtype=np.uint32).view(f32)[()], 1
        total = f32(np.sqrt(s))
        coef = f32(max_norm) / (total + f32(1e-6))
        if not coef < f32(1.0):
            coef = f32(1.0)
        step_size, rsq = f32(lr / (1.0 - betas[0] ** t)), f32(np.sqrt(1.0 - betas[1] ** t))
        b2, omb1, omb2 = f32(betas[1]), f32(1.0 - betas[0]), f32(1.0 - betas[1])
        for i in range(len(params)):
            g = grads[i] * coef
            if flags & CLIP_ONLY:
                grads[i][:] = g
                continue
            ms[i][:] = _fmaf_np(omb1, g - ms[i], ms[i])
            vs[i][:] = _fmaf_np(g * g, omb2, vs[i] * b2)
            d = np.sqrt(vs[i]) / rsq + f32(eps)
            params[i][:] = _fmaf_np(-step_size, ms[i] / d, params[i])
            if flags & ZERO:
                grads[i][:] = 0
            elif flags & WRITE:
                grads[i][:] = g
            if flags & SYNC and targets is not None:
                targets[i][:] = params[i]
        return total, 0


def bits_equal(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=f32).reshape(-1), np.ascontiguousarray(b, dtype=f32).reshape(-1)
    assert a.shape == b.shape, what
    bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[0]}: {a[bad[0]]!r} vs {b[bad[0]]!r}"


# ---- inputs ----------------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 7, 64, 257, 1023, 1024, 1025, 2051, 4099, 513, 3000]        # 12 tensors


def make_inputs(seed, steps=4, sizes=SIZES):
    """Parameters N(0, 1); per tensor a gradient magnitude spread over 1e-6 .. 1e2; `steps` gradient sets."""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(f32) for n in sizes]
    mags = 10.0 ** np.linspace(-6, 2, len(sizes))
    grads = [[(rng.standard_normal(n) * mags[i]).astype(f32) for i, n in enumerate(sizes)] for _ in range(steps)]
    return params, grads


def torch_run(params, grads, max_norm, dtype, *, clip=True, adam=True, sd=None, return_opt=False):
    """The reference's lines on copies: clip_grad_norm_ + optim.Adam with default arguments -> final (params, last grads)."""
    ps = [torch.nn.Parameter(torch.tensor(p, dtype=dtype)) for p in params]
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    if sd is not None:
        opt.load_state_dict(sd)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, dtype=dtype)
        if clip:
            clip_grad_norm_(ps, max_norm)
        if adam:
            opt.step()
    out = [p.detach().numpy().copy() for p in ps], [p.grad.numpy().copy() for p in ps]
    return (out + (opt,)) if return_opt else out


def def_run(params, grads, max_norm, flags=WRITE):
    ps = [p.copy() for p in params]
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    last = None
    for t, gs in enumerate(grads, 1):
        last = [g.copy() for g in gs]
        step_def(ps, last, ms, vs, LR, BETAS, EPS, max_norm, t, flags)
    return ps, last, ms, vs


def worst(a, b):
    return max(float(np.max(np.abs(x.astype(f64) - y.astype(f64)))) for x, y in zip(a, b))


# ---- the definition against torch's own lines ---------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [1.0, 1e6], ids=["clip_active", "clip_inactive"])
def test_definition_is_as_close_to_float64_as_torch_is(max_norm):
    params, grads = make_inputs(0)
    norm0 = np.sqrt(sum(float((g.astype(f64) ** 2).sum()) for g in grads[0]))
    assert (norm0 > max_norm) == (max_norm == 1.0), "the case is meant to have the clip active / inactive"
    p64, _ = torch_run(params, grads, max_norm, torch.float64)
    p32, _ = torch_run(params, grads, max_norm, torch.float32)
    pdef, _, _, _ = def_run(params, grads, max_norm)
    e_torch, e_def = worst(p32, p64), worst(pdef, p64)
    print(f"max_norm {max_norm}: e_torch {e_torch:.3e} e_def {e_def:.3e} ratio {e_def / e_torch:.3f}")
    assert e_torch > 0, "the reference's own error is 0 for these inputs: choose others"
    assert e_def <= 2 * e_torch


def test_clip_only_is_as_close_to_float64_as_clip_grad_norm():
    params, grads = make_inputs(1, steps=1)
    _, g64 = torch_run(params, grads, 1.0, torch.float64, adam=False)
    _, g32 = torch_run(params, grads, 1.0, torch.float32, adam=False)
    _, gdef, _, _ = def_run(params, grads, 1.0, CLIP_ONLY)
    e_torch, e_def = worst(g32, g64), worst(gdef, g64)
    print(f"clip only: e_torch {e_torch:.3e} e_def {e_def:.3e} ratio {e_def / e_torch:.3f}")
    assert e_torch > 0 and e_def <= 2 * e_torch
    pdef, _, ms, vs = def_run(params, grads, 1.0, CLIP_ONLY)
    for p, q, m, v in zip(pdef, params, ms, vs):
        bits_equal(p, q, "CLIP_ONLY must not touch the parameters")
        assert not m.any() and not v.any()


# ---- the wrapper's vectorised form is the definition ---------------------------------------------------------------------------
def wrapper_run(params, grads, max_norm, mode="write", *, targets=None, sync_at=()):
    ps = [torch.tensor(p) for p in params]
    opt = ClippedAdam(ps, LR, BETAS, EPS, max_norm, grads=mode, target_params=targets)
    totals = []
    for t, gs in enumerate(grads, 1):
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g)
        totals.append(opt.step(sync_target=t in sync_at))
    return ps, opt, totals


@pytest.mark.parametrize("max_norm", [1.0, 1e6])
@pytest.mark.parametrize("mode,flag", [("write", WRITE), ("zero", ZERO)])
def test_wrapper_on_cpu_tensors_is_the_definition_bit_for_bit(max_norm, mode, flag):
    params, grads = make_inputs(2, steps=3)
    ps, opt, totals = wrapper_run(params, grads, max_norm, mode)
    want_p, want_g, want_m, want_v = def_run(params, grads, max_norm, flag)
    for i in range(len(params)):
        bits_equal(ps[i].numpy(), want_p[i], f"param {i}")
        bits_equal(ps[i].grad.numpy(), want_g[i], f"grad {i}")
        bits_equal(opt.exp_avg[i].numpy(), want_m[i], f"exp_avg {i}")
        bits_equal(opt.exp_avg_sq[i].numpy(), want_v[i], f"exp_avg_sq {i}")
    assert totals[0].shape == () and totals[0].dtype == torch.float32 and opt.skipped() == 0
    if mode == "zero":
        assert all(not p.grad.any() for p in ps)
    bits_equal(O.grad_sumsq_np(grads[0]).astype(f32), f32(sumsq_def(grads[0])), "sum of squares")
    assert O.grad_sumsq_np(grads[0]) == sumsq_def(grads[0])


def test_sum_of_squares_with_more_than_256_chunks():
    """More than 256 chunks, so a thread of the second sum takes two partials: the chunk-by-chunk restatement and the
    vectorised one agree to the bit, and both are a float64 sum of the squares (within 1e-12 of numpy's pairwise one)."""
    rng = np.random.default_rng(3)
    grads = [rng.standard_normal(n).astype(f32) * f32(10.0 ** (i - 2)) for i, n in enumerate([270000, 1025, 5])]
    assert len(chunk_table([g.size for g in grads])) > 256
    s = sumsq_def(grads)
    assert s == O.grad_sumsq_np(grads)
    flat = np.concatenate(grads).astype(f64)
    pairwise = float(np.sum(flat * flat))
    assert abs(s - pairwise) <= 1e-12 * pairwise


# ---- edge cases ------------------------------------------------------------------------------------------------------------
def test_zero_gradients_leave_the_parameters_bit_unchanged():
    params, _ = make_inputs(4, steps=1)
    grads = [[np.zeros_like(p) for p in params]] * 3
    ps, opt, totals = wrapper_run(params, grads, 1.0)
    for p, q in zip(ps, params):
        bits_equal(p.numpy(), q)
    assert float(totals[-1]) == 0.0


def test_inactive_clip_has_coef_one_and_keeps_the_gradient_bits():
    params, grads = make_inputs(5, steps=1)
    grads[0][0][0] = f32(-0.0)
    grads[0][2][:3] = np.array([1e-42, -3e-45, 1e-39], dtype=f32)           # denormals
    total, coef, nonfinite = O.norm_and_coef_np(grads[0], 1e6)
    assert coef == f32(1.0) and coef.dtype == f32 and not nonfinite
    ps, _, _ = wrapper_run(params, grads, 1e6, "write")
    for p, g in zip(ps, grads[0]):
        bits_equal(p.grad.numpy(), g, "WRITE_GRADS with coef 1")


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("mode", ["write", "zero"])
def test_nonfinite_gradient_skips_the_step(bad, mode):
    params, grads = make_inputs(6, steps=2)
    ps = [torch.tensor(p) for p in params]
    targets = [torch.full_like(p, 7.0) for p in ps]
    opt = ClippedAdam(ps, LR, BETAS, EPS, 1.0, grads=mode, target_params=targets)
    for p, g in zip(ps, grads[0]):
        p.grad = torch.tensor(g)
    opt.step()
    before = [[x.clone() for x in xs] for xs in (ps, opt.exp_avg, opt.exp_avg_sq, targets)]
    poisoned = [g.copy() for g in grads[1]]
    poisoned[9][4098] = bad
    for p, g in zip(ps, poisoned):
        p.grad = torch.tensor(g)
    total = opt.step(sync_target=True)
    assert opt.skipped() == 1 and opt._t == 2
    assert torch.isnan(total) if np.isnan(bad) else torch.isinf(total)
    assert int(total.numpy().view(np.uint32)) == (0x7fc00000 if np.isnan(bad) else 0x7f800000)
    for xs, ys in zip((ps, opt.exp_avg, opt.exp_avg_sq, targets), before):
        for x, y in zip(xs, ys):
            bits_equal(x.numpy(), y.numpy(), "a skipped step must change nothing")
    for p, g in zip(ps, poisoned):
        bits_equal(p.grad.numpy(), g, "the gradients of a skipped step stay as they were")
    opt.clip_only()
    assert opt.skipped() == 2
    for p, g in zip(ps, poisoned):
        bits_equal(p.grad.numpy(), g)


def test_tiny_gradients_give_denormal_second_moments():
    p = [np.ones(5, dtype=f32)]
    g = [[np.full(5, 1e-20, dtype=f32)]]
    ps, opt, _ = wrapper_run(p, g, 1e6)
    v = opt.exp_avg_sq[0].numpy()
    tiny = np.finfo(f32).tiny
    assert (v > 0).all() and (v < tiny).all(), "g * g = 1e-40 is a float32 denormal and must be kept"
    _, _, _, want_v = def_run(p, g, 1e6)
    bits_equal(v, want_v[0])


def test_sync_target_and_argument_errors():
    params, grads = make_inputs(7, steps=2, sizes=[5, 1030])
    targets = [torch.full((n,), 7.0) for n in (5, 1030)]
    ps, opt, _ = wrapper_run(params, grads, 1.0, targets=targets, sync_at=(2,))
    for p, q in zip(ps, targets):
        bits_equal(p.numpy(), q.numpy(), "target after sync")
    ps, opt, _ = wrapper_run(params, grads[:1], 1.0, targets=[torch.full((n,), 7.0) for n in (5, 1030)])
    assert all((q == 7.0).all() for q in opt.targets), "a step without sync_target leaves the target alone"
    with pytest.raises(ValueError):
        ClippedAdam([torch.zeros(3)], LR, grads="keep")
    with pytest.raises(ValueError):
        ClippedAdam([torch.zeros(3)], LR).step(sync_target=True)
    with pytest.raises(ValueError):
        ClippedAdam([torch.zeros(3, dtype=torch.float64)], LR)
    with pytest.raises(ValueError):
        ClippedAdam([torch.zeros(4, 4).t()], LR)
    with pytest.raises(RuntimeError):
        ClippedAdam([torch.zeros(3)], LR, use_hip=True)


# ---- checkpoints in torch.optim.Adam's layout ------------------------------------------------------------------------------------
def test_state_dict_from_torch_and_on():
    """2 steps of torch's Adam, its state loaded here, one more step on each: the same yardstick."""
    params, grads = make_inputs(8, steps=3)
    p64, _ = torch_run(params, grads, 1.0, torch.float64)
    p32_2, _, opt32 = torch_run(params, grads[:2], 1.0, torch.float32, return_opt=True)
    p32, _ = torch_run(params, grads, 1.0, torch.float32)
    ps = [torch.tensor(p) for p in p32_2]
    mine = ClippedAdam(ps, 1.0, (0.5, 0.5), 1.0, 1.0)                        # hyper-parameters come from the checkpoint
    mine.load_state_dict(copy.deepcopy(opt32.state_dict()))
    assert mine._t == 2 and (mine.lr, mine.betas, mine.eps) == (LR, BETAS, EPS)
    for p, g in zip(ps, grads[2]):
        p.grad = torch.tensor(g)
    mine.step()
    got = [p.numpy() for p in ps]
    e_torch, e_def = worst(p32, p64), worst(got, p64)
    print(f"torch -> ClippedAdam: e_torch {e_torch:.3e} e_def {e_def:.3e}")
    assert e_torch > 0 and e_def <= 2 * e_torch


def test_state_dict_to_torch_and_on():
    """2 steps here, the state loaded into torch's Adam, one more step on each."""
    params, grads = make_inputs(9, steps=3)
    p64, _ = torch_run(params, grads, 1.0, torch.float64)
    p32, _ = torch_run(params, grads, 1.0, torch.float32)
    ps, mine, _ = wrapper_run(params, grads[:2], 1.0)
    sd = mine.state_dict()
    ref = torch.optim.Adam([torch.zeros(1)], lr=LR, betas=BETAS, eps=EPS).state_dict()
    assert set(sd) == set(ref) and set(sd["param_groups"][0]) == set(ref["param_groups"][0])
    assert set(sd["state"]) == set(range(len(params))) and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    got, _ = torch_run([p.numpy() for p in ps], grads[2:], 1.0, torch.float32, sd=copy.deepcopy(sd))
    e_torch, e_def = worst(p32, p64), worst(got, p64)
    print(f"ClippedAdam -> torch: e_torch {e_torch:.3e} e_def {e_def:.3e}")
    assert e_torch > 0 and e_def <= 2 * e_torch
    again = ClippedAdam([torch.tensor(p) for p in params], LR, BETAS, EPS, 1.0)
    again.load_state_dict(sd)
    for a, b in zip(again.exp_avg + again.exp_avg_sq, mine.exp_avg + mine.exp_avg_sq):
        bits_equal(a.numpy(), b.numpy())
    assert again._t == 2
    sd["state"][3]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="different steps"):
        again.load_state_dict(sd)


# ---- the tables follow the gradients ---------------------------------------------------------------------------------------------
def test_absent_gradient_drops_its_tensor_and_a_new_one_is_picked_up():
    params, grads = make_inputs(10, steps=3, sizes=[5, 1030, 300])
    ps = [torch.tensor(p) for p in params] + [torch.zeros(0)]
    opt = ClippedAdam(ps, LR, BETAS, EPS, 1.0)
    want_p, ms, vs = [p.copy() for p in params], [np.zeros_like(p) for p in params], [np.zeros_like(p) for p in params]
    present = [(0, 1, 2), (0, 2), (0, 1, 2)]
    ps[3].grad = torch.zeros(0)                                              # an empty tensor takes no part
    for t, (gs, act) in enumerate(zip(grads, present), 1):
        for i in range(3):
            ps[i].grad = torch.tensor(gs[i]) if i in act else None           # re-allocated every step
        total = opt.step()
        gd = [gs[i].copy() for i in act]
        want_total, _ = step_def([want_p[i] for i in act], gd, [ms[i] for i in act], [vs[i] for i in act], LR, BETAS, EPS, 1.0, t, WRITE)
        bits_equal(total.numpy(), want_total, f"total at step {t}")
        for i in range(3):
            bits_equal(ps[i].numpy(), want_p[i], f"param {i} at step {t}")
    assert set(opt.state_dict()["state"]) == {0, 1, 2}
    none = ClippedAdam([torch.zeros(3)], LR)
    assert float(none.step()) == 0.0 and none.state_dict()["state"] == {}
