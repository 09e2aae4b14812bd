"""csrc/irbpp_optim.hip on the GPU through optim.ClippedAdam, bit for bit against the numpy definition of
tests/test_clipped_adam_cpu.py in every array: parameters, both moments, gradients, target, total and skipped, over 3 steps.

Tensor sizes, the smallest at which each part can go wrong: 1 and 3 (one thread, fewer elements than a thread takes); 1023,
1024, 1025 (the chunk edge); 4099 (a tail that is no multiple of 4); a 1-D view that starts one element into a larger buffer
(4-byte aligned only: the dword path) and a tensor whose gradient alone is such a view; [300, 900] (264 chunks: more than 256,
so a thread of the second kernel's sum takes two partials); a tensor with grad None; an empty tensor."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from irbpp_amd.optim import ClippedAdam
from test_clipped_adam_cpu import BETAS, CLIP_ONLY, EPS, LR, SYNC, WRITE, ZERO, bits_equal, f32, step_def, worst

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (shape, kind): "view" = the parameter one float into a larger buffer, "gview" = its gradient so, "nograd", "plain"
SPEC = [((1,), "plain"), ((3,), "plain"), ((1023,), "plain"), ((1024,), "plain"), ((1025,), "plain"), ((4099,), "plain"),
        ((2050,), "view"), ((1500,), "gview"), ((300, 900), "plain"), ((77,), "nograd"), ((0,), "plain")]
ACTIVE = [i for i, (shape, kind) in enumerate(SPEC) if kind != "nograd" and int(np.prod(shape)) > 0]
STEPS = 3


def case_arrays(seed, steps=STEPS, scale=1.0):
    """-> parameters and `steps` gradient sets as flat float32 arrays, one per SPEC entry; magnitudes 1e-6 .. 1e2 * scale."""
    rng = np.random.default_rng(seed)
    sizes = [int(np.prod(shape)) for shape, _ in SPEC]
    mags = 10.0 ** np.linspace(-6, 2, len(sizes)) * scale
    params = [rng.standard_normal(n).astype(f32) for n in sizes]
    grads = [[(rng.standard_normal(n) * mags[i]).astype(f32) for i, n in enumerate(sizes)] for _ in range(steps)]
    return params, grads


def offset_tensor(flat, shape, dev):
    """`flat` as a tensor of `shape` that starts one float into a larger buffer: contiguous, 4-byte aligned only."""
    buf = torch.full((flat.size + 9,), 1e30, dtype=torch.float32, device=dev)
    t = buf[1:1 + flat.size]
    t.copy_(torch.from_numpy(flat))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t.view(shape)


def device_params(params, dev=DEV):
    out = []
    for flat, (shape, kind) in zip(params, SPEC):
        t = offset_tensor(flat, shape, dev) if kind == "view" else torch.tensor(flat, device=dev).view(shape)
        out.append(t.detach().requires_grad_())
    return out


def set_grads(ps, gs, dev=DEV):
    for p, g, (shape, kind) in zip(ps, gs, SPEC):
        if kind == "nograd":
            p.grad = None
        elif kind == "gview":
            p.grad = offset_tensor(g, shape, dev)
        else:
            p.grad = torch.tensor(g, device=dev).view(shape)


def host(t):
    return t.detach().cpu().numpy().reshape(-1)


class Want(object):
    """The definition's run over the tensors that take part, on host copies."""

    def __init__(self, params, max_norm):
        self.p = [p.copy() for p in params]
        self.m, self.v = [np.zeros_like(p) for p in params], [np.zeros_like(p) for p in params]
        self.tg = [np.full_like(p, 7.0) for p in params]
        self.max_norm, self.t, self.skipped, self.g = max_norm, 0, 0, None

    def step(self, gs, flags, advance=True):
        self.t += advance
        self.g = [g.copy() for g in gs]
        pick = lambda xs: [xs[i] for i in ACTIVE]                              # noqa: E731
        total, skipped = step_def(pick(self.p), pick(self.g), pick(self.m), pick(self.v), LR, BETAS, EPS, self.max_norm,
                                  max(self.t, 1), flags, pick(self.tg))
        self.skipped += skipped
        return total

    def check(self, ps, opt, total, want_total, what):
        bits_equal(host(total), want_total, f"{what}: total")
        for i in range(len(SPEC)):
            bits_equal(host(ps[i]), self.p[i], f"{what}: param {i}")
            bits_equal(host(opt.exp_avg[i]), self.m[i], f"{what}: exp_avg {i}")
            bits_equal(host(opt.exp_avg_sq[i]), self.v[i], f"{what}: exp_avg_sq {i}")
            bits_equal(host(opt.targets[i]), self.tg[i], f"{what}: target {i}")
            if i in ACTIVE:
                bits_equal(host(ps[i].grad), self.g[i], f"{what}: grad {i}")
        assert opt.skipped() == self.skipped, what


def make(params, max_norm, mode, dev=DEV, use_hip=True):
    ps = device_params(params, dev)
    targets = [torch.full_like(p, 7.0, memory_format=torch.contiguous_format).detach() for p in ps]
    return ps, ClippedAdam(ps, LR, BETAS, EPS, max_norm, target_params=targets, grads=mode, use_hip=use_hip)


@pytest.mark.parametrize("max_norm", [1.0, 1e6], ids=["clip_active", "clip_inactive"])
@pytest.mark.parametrize("mode,flag", [("write", WRITE), ("zero", ZERO)])
def test_three_steps_bit_for_bit(max_norm, mode, flag):
    """Every array after every step; the target is written by the second step alone."""
    params, grads = case_arrays(0)
    ps, opt = make(params, max_norm, mode)
    want = Want(params, max_norm)
    assert len(ACTIVE) == 9 and opt._key is None
    for t, gs in enumerate(grads, 1):
        set_grads(ps, gs)
        total = opt.step(sync_target=t == 2)
        assert total.shape == () and total.device == ps[0].device
        want_total = want.step(gs, flag | (SYNC if t == 2 else 0))
        coef = f32(max_norm) / (want_total + f32(1e-6))
        assert (coef < 1) == (max_norm == 1.0), "the case is meant to have the clip active / inactive"
        want.check(ps, opt, total, want_total, f"step {t}")
        assert opt._tables[3] == 280 and len(opt._key) == 9                   # chunks, tensors in the device tables
        if t == 2:
            for i in ACTIVE:
                bits_equal(host(opt.targets[i]), host(ps[i]), "sync_target makes the target the parameters")
    assert (host(opt.targets[9]) == 7.0).all() and any((host(opt.targets[i]) != host(ps[i])).any() for i in ACTIVE)


def test_zeroed_gradients_take_the_next_backward():
    """grads="zero" leaves zeros in the same storage; a backward into them gives the step fresh gradients give."""
    params, grads = case_arrays(1, steps=2)
    ps, opt = make(params, 1.0, "zero")
    want = Want(params, 1.0)
    set_grads(ps, grads[0])
    opt.step()
    want.step(grads[0], ZERO)
    ptrs = [ps[i].grad.data_ptr() for i in ACTIVE]
    assert all(not ps[i].grad.any() for i in ACTIVE)
    key = opt._key
    sum((p * torch.from_numpy(g).to(DEV).view(p.shape)).sum() for i, (p, g) in enumerate(zip(ps, grads[1])) if i in ACTIVE).backward()
    assert [ps[i].grad.data_ptr() for i in ACTIVE] == ptrs, "autograd accumulates in place"
    total = opt.step()
    assert opt._key == key, "stable pointers: the device tables are not rebuilt"
    want.check(ps, opt, total, want.step(grads[1], ZERO), "after backward into the zeros")


def test_clip_only():
    params, grads = case_arrays(2, steps=1)
    ps, opt = make(params, 1.0, "write")
    want = Want(params, 1.0)
    set_grads(ps, grads[0])
    total = opt.clip_only()
    want_total = want.step(grads[0], CLIP_ONLY, advance=False)
    want.check(ps, opt, total, want_total, "clip_only")
    assert any((want.g[i] != grads[0][i]).any() for i in ACTIVE) and opt._t == 0
    ref = [torch.from_numpy(g.astype(np.float64)).requires_grad_() for g in grads[0]]
    for i, r in enumerate(ref):
        r.grad = r.detach().clone() if i in ACTIVE else None
    clip_grad_norm_(ref, 1.0)
    for i in ACTIVE:        # four float32 roundings on the way (total, + 1e-6f, the division, the product): 4 * 2^-24 < 3e-7
        np.testing.assert_allclose(want.g[i], ref[i].grad.numpy(), rtol=3e-7, atol=0)


@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_nonfinite_gradient_skips_the_step(bad):
    params, grads = case_arrays(3, steps=3)
    ps, opt = make(params, 1.0, "zero")
    want = Want(params, 1.0)
    grads[1][8][264 * 1024 - 1 - 1024] = bad                                  # in the matrix, far from thread 0's partials
    for t, gs in enumerate(grads, 1):
        set_grads(ps, gs)
        total = opt.step(sync_target=True)
        want.check(ps, opt, total, want.step(gs, ZERO | SYNC), f"step {t}")
    assert opt.skipped() == 1 and want.skipped == 1 and opt._t == 3


def test_two_runs_give_the_same_bits():
    params, grads = case_arrays(4)
    runs = []
    for _ in range(2):
        ps, opt = make(params, 1.0, "write")
        totals = []
        for gs in grads:
            set_grads(ps, gs)
            totals.append(host(opt.step()).copy())
        runs.append([host(p).copy() for p in ps] + [host(m).copy() for m in opt.exp_avg + opt.exp_avg_sq] + totals)
    for a, b in zip(*runs):
        bits_equal(a, b, "run to run")


def test_abi_argument_errors():
    """Null pointers, bad counts and contradicting flags come back as IRBPP_ERR_ARG before anything is launched: the tables
    handed over here are zeros, which no kernel could walk."""
    from irbpp_amd import _lib as L
    lib = L.load()
    z = torch.zeros(64, dtype=torch.int64, device=DEV)
    ptr, stream = z.data_ptr(), C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    hyper = lambda flags: C.byref(L.IrbppAdamHyper(1e-3, 1.0, 0.9, 0.1, 0.999, 0.001, 1e-8, 1.0, flags))    # noqa: E731
    call = lib.irbpp_clipped_adam_step
    for k in (0, 2, 4, 6, 7):
        args = [ptr, 1, ptr, 1, ptr, hyper(1), ptr, ptr, stream]
        args[k] = None
        assert call(*args) == -1, f"argument {k} NULL"
    assert call(ptr, 1, ptr, 1, ptr, None, ptr, ptr, stream) == -1
    assert call(ptr, 0, ptr, 1, ptr, hyper(1), ptr, ptr, stream) == -1
    assert call(ptr, 2, ptr, 1, ptr, hyper(1), ptr, ptr, stream) == -1        # fewer chunks than tensors
    assert call(ptr, 1, ptr, 0, ptr, hyper(1), ptr, ptr, stream) == -1
    for flags in (1 | 2, 8 | 2, 8 | 4, 16, -1):
        assert call(ptr, 1, ptr, 1, ptr, hyper(flags), ptr, ptr, stream) == -1, f"flags {flags}"
    torch.cuda.synchronize()
    assert not z.any()


# ---- learn_loss -> backward -> step on a stand-in network ------------------------------------------------------------------------
B, S, F, H, ATOMS = 8, 6, 12, 24, 31


class StandIn(torch.nn.Module):
    """states [B, S, F] -> (v [B, ATOMS], a [B, S, ATOMS]): two nn.Linear and a NoisyLinear-shaped value layer (mu / sigma
    parameters, fixed epsilon buffers)."""

    def __init__(self, rng, dtype, dev):
        super().__init__()
        mk = lambda *shape, s=0.3: torch.from_numpy((rng.standard_normal(shape) * s).astype(f32)).to(device=dev, dtype=dtype)   # noqa: E731
        self.lin1, self.lin2 = torch.nn.Linear(F, H), torch.nn.Linear(H, ATOMS)
        for lin in (self.lin1, self.lin2):
            lin.weight = torch.nn.Parameter(mk(*lin.weight.shape))
            lin.bias = torch.nn.Parameter(mk(*lin.bias.shape))
        self.weight_mu, self.weight_sigma = torch.nn.Parameter(mk(ATOMS, H)), torch.nn.Parameter(mk(ATOMS, H, s=0.05))
        self.bias_mu, self.bias_sigma = torch.nn.Parameter(mk(ATOMS)), torch.nn.Parameter(mk(ATOMS, s=0.05))
        self.register_buffer("weight_epsilon", mk(ATOMS, H, s=1.0))
        self.register_buffer("bias_epsilon", mk(ATOMS, s=1.0))

    def logits(self, x):
        h = torch.relu(self.lin1(x))
        v = torch.nn.functional.linear(h.mean(1), self.weight_mu + self.weight_sigma * self.weight_epsilon,
                                       self.bias_mu + self.bias_sigma * self.bias_epsilon)
        return v, self.lin2(h)


def learn_run(form, dev, dtype, steps=3, use_hip=None):
    """`steps` of learn: learn_loss -> backward -> the optimiser step in the given form -> the online parameters."""
    rng = np.random.default_rng(31)
    online, target = StandIn(rng, dtype, dev), StandIn(rng, dtype, dev)
    to = lambda x: torch.from_numpy(x).to(device=dev, dtype=dtype if x.dtype == f32 else None)    # noqa: E731
    support = torch.linspace(-1.0, 8.0, ATOMS).to(device=dev, dtype=dtype)
    params = list(online.parameters())
    if form == "torch":
        opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS)
    else:
        opt = ClippedAdam(params, LR, BETAS, EPS, 0.05, grads="zero", use_hip=form == "hip")
    for _ in range(steps):
        batch = (None, to(rng.standard_normal((B, S, F)).astype(f32)), to(rng.integers(0, S, B)), to(rng.uniform(-2, 9, B).astype(f32)),
                 to(rng.standard_normal((B, S, F)).astype(f32)), to((rng.random((B, 1)) < 0.7).astype(f32)), None)
        weights = to(rng.uniform(0.2, 1.0, B).astype(f32))
        loss = replay.learn_loss(online.logits, target.logits, batch, support, 0.99 ** 3, -1.0, 8.0, use_hip=use_hip)
        if form == "torch":
            online.zero_grad()
        (weights * loss).mean().backward()
        if form == "torch":
            assert float(clip_grad_norm_(params, 0.05)) > 0.05, "the clip is meant to be active"
        opt.step()
    return [p.detach().cpu().numpy() for p in params]


def test_learn_step_on_a_stand_in_network():
    """The reference's lines (clip_grad_norm_ + optim.Adam) and ClippedAdam, both behind learn_loss's kernels on the device,
    against the same lines in float64 on the CPU: the fused step may be at most twice as far from it as torch's own float32."""
    p64 = learn_run("torch", "cpu", torch.float64)
    p32 = learn_run("torch", DEV, torch.float32, use_hip=True)
    got = learn_run("hip", DEV, torch.float32, use_hip=True)
    e_torch, e_def = worst(p32, p64), worst(got, p64)
    print(f"learn step: e_torch {e_torch:.3e} e_def {e_def:.3e} ratio {e_def / e_torch:.3f}")
    assert e_torch > 0 and e_def <= 2 * e_torch
