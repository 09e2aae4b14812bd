"""csrc/irbpp_dueling_loss.hip on the GPU, bit for bit against the numpy float32 definition of tests/test_dueling_loss_cpu.py
(loss, g, grad_v, grad_a: the same 32 bits), through the C ABI with strided arguments on the current stream; then the autograd
Function of replay.dueling_c51_loss and replay.learn_loss.

Shapes (S, atoms): (1, 2) and (3, 2) the smallest block and fewer rows than partial sums; (15 | 16 | 17, 31) around the 16
interleaved parts; (33, 51) two full rounds of the parts plus one row and rows that do not divide 512; (500, 31) the learn
batch's block, 8 chunks of 64 rows in the backward grid, the last one short; (1024, 128) the largest block, 16 full chunks and
256 strides of 512 threads.  Batches of 1, 3 and 65.  Every case slices `a` out of a wider tensor (row and env stride, 1e30
around it) and `v` out of wider rows; its samples cycle through the scenarios of loss_case."""
import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_dueling_cpu import bounds, f32, head_inputs
from test_dueling_loss_cpu import dueling_loss_backward_np, dueling_loss_np, loss_bounds, loss_torch
from test_gpu_dueling import DEV, _lib, _ptr, _stream, widen, widen_v

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2), (3, 2), (15, 31), (16, 31), (17, 31), (33, 51), (500, 31), (1024, 128)]
CASES = [(s, a, b) for s, a in SHAPES for b in (1, 3, 65)]


def loss_case(b, s, atoms, seed=0):
    """-> v [b, atoms], a [b, s, atoms], actions int64 [b], m [b, atoms], w [b].  With i = sample index + seed:
    action (i mod 5): row 0;  row S - 1;  a middle row;  a negative index;  out of range (S, or -S - 1 for odd i // 5).
    m (i mod 3): a distribution with exact zeros;  the same times 0.37 (does not sum to 1);  one atom alone.
    logits (i mod 4 == 2): times 60, so that most e are exactly 0 (t < -80).   w (i mod 7 == 6): 0, else in (-1, 1)."""
    rng = np.random.default_rng(1000 * s + atoms + 17 * seed + b)
    v = rng.standard_normal((b, atoms)).astype(f32)
    a = rng.standard_normal((b, s, atoms)).astype(f32)
    m = rng.random((b, atoms))
    m[rng.random((b, atoms)) < 0.3] = 0
    m[:, 1] += 0.05
    m = (m / m.sum(-1, keepdims=True)).astype(f32)
    w = rng.uniform(-1, 1, b).astype(f32)
    actions = np.zeros(b, dtype=np.int64)
    for k in range(b):
        i = k + seed
        actions[k] = (0, s - 1, s // 2, -1 - (i // 5) % s, -s - 1 if (i // 5) % 2 else s)[i % 5]
        if i % 3 == 1:
            m[k] *= f32(0.37)
        elif i % 3 == 2:
            m[k] = 0
            m[k, i % atoms] = 1
        if i % 4 == 2:
            v[k] *= 60
            a[k] *= 60
        if i % 7 == 6:
            w[k] = 0
    return v, a, actions, m, w


def same_bits(got, want, what):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32), err_msg=what)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_loss(v, a, actions, m):
    L, lib = _lib()
    b, s, atoms = a.shape
    keep_a, a_d = widen(a, 3, 2, 3)
    keep_v, v_d = widen_v(v)
    act_d, m_d = dev(actions), dev(m)
    loss_d = torch.full((b + 1,), -5.0, dtype=torch.float32, device=DEV)
    g_d = torch.full((b + 1, atoms), -5.0, dtype=torch.float32, device=DEV)
    L.check(lib.irbpp_dueling_loss(_ptr(v_d), v_d.stride(0), _ptr(a_d), a_d.stride(0), a_d.stride(1), _ptr(act_d), _ptr(m_d), atoms, s,
                                   b, _ptr(loss_d), _ptr(g_d), _stream()), "irbpp_dueling_loss")
    torch.cuda.synchronize()
    loss, g = loss_d.cpu().numpy(), g_d.cpu().numpy()
    assert loss[b] == -5.0 and (g[b] == -5.0).all(), "written beyond the batch"
    return loss[:b], g[:b]


def run_backward(g, w, actions, s, with_v=True, with_a=True):
    L, lib = _lib()
    b, atoms = g.shape
    g_d, w_d, act_d = dev(g), dev(w), dev(actions)
    gv_d = torch.full((b + 1, atoms), -5.0, dtype=torch.float32, device=DEV)
    ga_d = torch.full((b * s * atoms + 4,), -5.0, dtype=torch.float32, device=DEV)
    L.check(lib.irbpp_dueling_loss_backward(_ptr(g_d), _ptr(w_d), _ptr(act_d), atoms, s, b, _ptr(gv_d if with_v else None),
                                            _ptr(ga_d if with_a else None), _stream()), "irbpp_dueling_loss_backward")
    torch.cuda.synchronize()
    gv, ga = gv_d.cpu().numpy(), ga_d.cpu().numpy()
    assert (gv[b] == -5.0).all() and (ga[b * s * atoms:] == -5.0).all(), "written beyond the batch"
    if not with_v:
        assert (gv == -5.0).all(), "grad_v written though it was NULL"
    if not with_a:
        assert (ga == -5.0).all(), "grad_a written though it was NULL"
    return gv[:b], ga[:b * s * atoms].reshape(b, s, atoms)


@pytest.mark.parametrize("s,atoms,b", CASES)
def test_kernels_bit_exact(s, atoms, b):
    v, a, actions, m, w = loss_case(b, s, atoms)
    want_loss, want_g = dueling_loss_np(v, a, actions, m)
    want_gv, want_ga = dueling_loss_backward_np(want_g, w, actions, s)
    loss, g = run_loss(v, a, actions, m)
    same_bits(loss, want_loss, "loss")
    same_bits(g, want_g, "g")
    bad = (actions >= s) | (actions < -s)
    assert np.isnan(loss[bad]).all() and (g[bad] == 0).all() and np.isfinite(loss[~bad]).all()
    gv, ga = run_backward(g, w, actions, s)
    same_bits(gv, want_gv, "grad_v")
    same_bits(ga, want_ga, "grad_a")
    gv, _ = run_backward(g, w, actions, s, with_a=False)
    same_bits(gv, want_gv, "grad_v alone")
    _, ga = run_backward(g, w, actions, s, with_v=False)
    same_bits(ga, want_ga, "grad_a alone")


# ------------------------------------------------------------------ the autograd Function ------------
def leaves(v, a):
    return dev(v).requires_grad_(), dev(a).requires_grad_()


@pytest.mark.parametrize("s,atoms,b", [(17, 31, 3), (500, 31, 6), (1024, 128, 2)])
def test_function_equals_the_definition_and_follows_torch(s, atoms, b):
    v, a, actions, m, w = loss_case(b, s, atoms, seed=5)
    actions = np.where((actions >= s) | (actions < -s), 1 % s, actions)        # the torch lines refuse an index out of range
    want_loss, g = dueling_loss_np(v, a, actions, m)
    want_gv, want_ga = dueling_loss_backward_np(g, w, actions, s)
    v_d, a_d = leaves(v, a)
    loss = replay.dueling_c51_loss(v_d, a_d, dev(actions), dev(m), use_hip=True)
    assert loss.dtype == torch.float32 and loss.shape == (b,) and loss.requires_grad
    (dev(w) * loss).sum().backward()
    same_bits(loss.detach().cpu().numpy(), want_loss, "loss")
    same_bits(v_d.grad.cpu().numpy(), want_gv, "v.grad")
    same_bits(a_d.grad.cpu().numpy(), want_ga, "a.grad")
    v64, a64 = dev(v).double().requires_grad_(), dev(a).double().requires_grad_()                # the torch lines, on the device
    loss64 = loss_torch(v64, a64, dev(actions), dev(m).double())
    (dev(w).double() * loss64).sum().backward()
    dloss, dgv, dga = loss_bounds(v, a, m, w)
    assert (loss.detach().double() - loss64.detach()).abs().max().item() <= dloss
    assert (v_d.grad.double() - v64.grad).abs().max().item() <= dgv
    assert (a_d.grad.double() - a64.grad).abs().max().item() <= dga


def test_function_shapes_strides_and_accumulation():
    s, atoms, b = 33, 51, 4
    v, a, actions, m, w = loss_case(b, s, atoms, seed=1)
    want_loss, g = dueling_loss_np(v, a, actions, m)
    ones_v, ones_a = dueling_loss_backward_np(g, np.ones(b, dtype=f32), actions, s)
    act_d, m_d = dev(actions), dev(m)
    # loss.sum().backward(): a stride-0 upstream gradient; v as [B, 1, atoms]
    v_d, a_d = dev(v.reshape(b, 1, atoms)).requires_grad_(), dev(a).requires_grad_()
    replay.dueling_c51_loss(v_d, a_d, act_d, m_d, use_hip=True).sum().backward()
    assert v_d.grad.shape == (b, 1, atoms)
    same_bits(v_d.grad.cpu().numpy().reshape(b, atoms), ones_v, "v.grad")
    same_bits(a_d.grad.cpu().numpy(), ones_a, "a.grad")
    # a non-contiguous a: a slice of a wider leaf (passed as it is) and a permuted one (made contiguous); the gradient arrives in
    # the leaf's own layout
    keep, a_slice = widen(a, 3, 2, 3)
    keep.requires_grad_()
    loss = replay.dueling_c51_loss(dev(v), keep[:, 1:1 + s, 2:2 + atoms], act_d, m_d, use_hip=True)
    same_bits(loss.detach().cpu().numpy(), want_loss, "loss of a slice")
    loss.sum().backward()
    wide = keep.grad.cpu().numpy()
    same_bits(wide[:, 1:1 + s, 2:2 + atoms], ones_a, "gradient of a slice")
    wide[:, 1:1 + s, 2:2 + atoms] = 0
    assert (wide == 0).all()
    a_perm = dev(np.ascontiguousarray(a.transpose(1, 0, 2))).requires_grad_()
    loss = replay.dueling_c51_loss(dev(v), a_perm.permute(1, 0, 2), act_d, m_d, use_hip=True)
    same_bits(loss.detach().cpu().numpy(), want_loss, "loss of a permuted block")
    loss.sum().backward()
    same_bits(a_perm.grad.cpu().numpy().transpose(1, 0, 2), ones_a, "gradient of a permuted block")
    # only one side requires a gradient; neither
    v_d, a_d = leaves(v, a)
    replay.dueling_c51_loss(v_d, dev(a), act_d, m_d, use_hip=True).sum().backward()
    replay.dueling_c51_loss(dev(v), a_d, act_d, m_d, use_hip=True).sum().backward()
    same_bits(v_d.grad.cpu().numpy(), ones_v, "v.grad alone")
    same_bits(a_d.grad.cpu().numpy(), ones_a, "a.grad alone")
    assert not replay.dueling_c51_loss(dev(v), dev(a), act_d, m_d, use_hip=True).requires_grad
    # a training-style loop: the second call accumulates into .grad
    v_d, a_d = leaves(v, a)
    v2, a2, actions2, m2, w2 = loss_case(b, s, atoms, seed=2)
    _, g2 = dueling_loss_np(v, a, actions2, m2)
    two_v, two_a = dueling_loss_backward_np(g2, w2, actions2, s)
    one_v, one_a = dueling_loss_backward_np(g, w, actions, s)
    (dev(w) * replay.dueling_c51_loss(v_d, a_d, act_d, m_d, use_hip=True)).sum().backward()
    (dev(w2) * replay.dueling_c51_loss(v_d, a_d, dev(actions2), dev(m2), use_hip=True)).sum().backward()
    same_bits(v_d.grad.cpu().numpy(), one_v + two_v, "accumulated v.grad")
    same_bits(a_d.grad.cpu().numpy(), one_a + two_a, "accumulated a.grad")


def test_learn_loss_on_the_device_against_its_cpu_form():
    """replay.learn_loss with the kernels against its CPU form in float64 on the same logits (the "networks" hand out fixed
    tensors, so both sides start from the same numbers).  The bound is loss_bounds' for the loss, plus what the two m
    contribute: m comes from dueling_c51_target on either side, within dm of the exact one (``bounds`` of test_dueling_cpu.py,
    the planted leader making a_star agree), and the loss is sum_k m[k] (-lp[k]) with |lp| <= LP = 2 (V + 2A) + log(atoms):
    at most atoms dm LP more."""
    b, s, atoms, v_min, v_max, gamma_n = 5, 40, 31, -1.0, 8.0, 0.99 ** 3
    rng = np.random.default_rng(21)
    support = torch.linspace(v_min, v_max, atoms)
    z = support.numpy()
    v, a, _ = head_inputs(rng, b, s, atoms, z, lead=0.0)
    v_on, a_on, _ = head_inputs(rng, b, s, atoms, z)
    v_tg, a_tg, _ = head_inputs(rng, b, s, atoms, z, lead=0.0)
    actions = rng.integers(0, s, b)
    returns = rng.uniform(v_min - 1, v_max + 1, b).astype(f32)
    nonterm = (rng.random((b, 1)) < 0.6).astype(f32)
    states, next_states = np.zeros((b, 1), dtype=f32), np.ones((b, 1), dtype=f32)

    def side(to):
        t = {k: to(x) for k, x in dict(v=v, a=a, v_on=v_on, a_on=a_on, v_tg=v_tg, a_tg=a_tg).items()}
        st, nx = to(states), to(next_states)
        online = lambda x: (t["v"], t["a"]) if x is st else (t["v_on"], t["a_on"])                 # noqa: E731
        target = lambda x: (t["v_tg"], t["a_tg"])                                                   # noqa: E731
        return online, target, (None, st, to(actions), to(returns), nx, to(nonterm), None)
    on_d, tg_d, batch_d = side(dev)
    got = replay.learn_loss(on_d, tg_d, batch_d, support.to(DEV), gamma_n, v_min, v_max, use_hip=True)
    to64 = lambda x: torch.from_numpy(x).double() if x.dtype == f32 else torch.from_numpy(x)     # noqa: E731
    on_c, tg_c, batch_c = side(to64)
    want = replay.learn_loss(on_c, tg_c, batch_c, support.double(), gamma_n, v_min, v_max)
    assert got.shape == (b,) and got.dtype == torch.float32 and want.dtype == torch.float64
    delta_z = (v_max - v_min) / (atoms - 1)
    dm = bounds(v_tg, a_tg, z, returns, delta_z)[2]
    m_max = np.full((b, atoms), 1.0 + dm)                                       # each m sums to at most 1 (+ dm per entry)
    dloss = loss_bounds(v, a, m_max / atoms, np.ones(b, dtype=f32))[0]
    LP = 2 * (float(np.abs(v).max()) + 2 * float(np.abs(a).max())) + float(np.log(atoms))
    assert (got.double().cpu() - want).abs().max().item() <= dloss + atoms * dm * LP


def test_status_codes_on_device_pointers():
    L, lib = _lib()
    b, s, atoms = 2, 4, 31
    buf = torch.zeros((b * s * atoms,), dtype=torch.float32, device=DEV)
    act = torch.zeros((b,), dtype=torch.int64, device=DEV)
    out, out2 = (torch.zeros((b * s * atoms,), dtype=torch.float32, device=DEV) for _ in range(2))

    def call(atoms=atoms, s=s, b=b, row=atoms):
        return lib.irbpp_dueling_loss(_ptr(buf), atoms, _ptr(buf), s * row, row, _ptr(act), _ptr(buf), atoms, s, b, _ptr(out), _ptr(out2),
                                      _stream())
    L.check(call(), "irbpp_dueling_loss")
    torch.cuda.synchronize()
    for bad in (dict(atoms=1), dict(atoms=129), dict(s=0), dict(s=1025), dict(b=0), dict(row=atoms - 1)):
        with pytest.raises(L.IrbppError):
            L.check(call(**bad), "irbpp_dueling_loss")

    def back(atoms=atoms, s=s, b=b):
        return lib.irbpp_dueling_loss_backward(_ptr(buf), _ptr(buf), _ptr(act), atoms, s, b, _ptr(out), _ptr(out2), _stream())
    L.check(back(), "irbpp_dueling_loss_backward")
    torch.cuda.synchronize()
    for bad in (dict(atoms=1), dict(atoms=129), dict(s=0), dict(s=1025), dict(b=0)):
        with pytest.raises(L.IrbppError):
            L.check(back(**bad), "irbpp_dueling_loss_backward")
