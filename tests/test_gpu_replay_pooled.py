"""csrc/irbpp_replay_pool.hip -- irbpp_replay_pool_sample / _gather / _update -- against the numpy model of
tests/test_replay_pooled_cpu.py, with that file's equality rules: env, priority, data index, tree index, flags, actions, states
and the trees after updates bit for bit, n-step returns and importance weights within 1e-6.

Sizes are the smallest at which the kernels can still go wrong.  B = 1, 255, 257, 1024: the 256 threads' draw loop takes a
second trip, the reduction spans four waves.  N = 1, 3, 65, 4097 (a top tree beyond one wave's width) and 8192 (the LDS limit);
8193 is refused.  Capacity 11 (leaves at two depths) and 64, and one memory of capacity 8200 -- a tree row of 16399 floats,
past the per-env kernels' LDS row, which the pooled kernels walk in global memory.  obs_len 1 and 300 (the copy loop's second
trip).  The batch maximum of the weights owned by a sample of wave 0 and of wave 3."""
import ctypes as C

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_replay_pooled_cpu import assert_batch, f32, load_memory, make_model, random_triples, rebuild, values_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _memory(m):
    """The model on the device, on the HIP launches (a capacity past the per-env kernels' LDS row is no obstacle to them)."""
    mem = load_memory(m, DEV, use_hip=None if m.cap > 8192 else True)
    assert mem._pool_lib is not None
    return mem


# ------------------------------------------------------------------ sample + gather, supplied values -------------------------
@pytest.mark.parametrize("n_env,cap,obs_len,b,max_at", [
    (1, 11, 1, 1, 0), (3, 64, 300, 255, 200), (65, 11, 1, 257, 3), (3, 11, 300, 1024, 456), (4097, 11, 1, 1024, 5),
    (8192, 11, 1, 257, 256), (1, 8200, 1, 257, 250), (65, 64, 1, 64, 63)])
def test_pooled_sample_and_gather_for_supplied_values(n_env, cap, obs_len, b, max_at):
    """Every field of the batch against the model; the one smallest priority is read by sample `max_at` alone (thread
    max_at % 256: wave 0 or wave 3, first or second trip of the draw loop), so that sample's weight is the batch maximum."""
    rng = np.random.RandomState(n_env * 31 + cap + b)
    m = make_model(n_env, cap, obs_len, rng, rare=True)
    mem = _memory(m)
    values = values_for(m, b, rng, place={max_at: m.rare}, avoid=(m.rare,))
    want, prob, data_idx = m.sample_at(values)
    got = mem.sample_pooled(b, values=_dev(values))
    assert_batch(got, want)
    assert got[1].shape == (b, obs_len) and got[5].shape == (b, 1)
    w = got[6].cpu().numpy()
    assert w[max_at] == 1.0 and want[6][max_at] == 1.0 and (b == 1 or np.delete(w, max_at).max() < 0.5)
    # prob and data_idx, which sample_pooled does not hand out: the launch itself
    from irbpp_amd import _lib
    out = [torch.empty(b, dtype=dt, device=DEV) for dt in (torch.int64, torch.float32, torch.int64, torch.int64, torch.float32)]
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    view = mem._view()
    _lib.check(mem._pool_lib.irbpp_replay_pool_sample(C.byref(view), b, replay._p(_dev(values)), 0, 64, float(m.beta),
                                                      *[replay._p(t) for t in out], replay._p(failed), replay._stream(mem.device)),
               "irbpp_replay_pool_sample")
    assert int(failed.item()) == 0
    np.testing.assert_array_equal(out[0].cpu().numpy(), want[0][:, 0])
    np.testing.assert_array_equal(out[1].cpu().numpy(), prob)
    np.testing.assert_array_equal(out[2].cpu().numpy(), data_idx)
    np.testing.assert_array_equal(out[3].cpu().numpy(), want[0][:, 1])


def test_more_envs_than_the_top_tree_holds_is_an_argument_error():
    from irbpp_amd import _lib
    mem = replay.VectorReplayMemory(8193, 2, 1, device=DEV, use_hip=True)
    mem.sum_tree.fill_(1.0)
    out = [torch.full((4,), -7, dtype=dt, device=DEV) for dt in (torch.int64, torch.float32, torch.int64, torch.int64, torch.float32)]
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    view = mem._view()
    status = mem._pool_lib.irbpp_replay_pool_sample(C.byref(view), 4, replay._p(None), 0, 64, 0.4, *[replay._p(t) for t in out],
                                                    replay._p(failed), replay._stream(mem.device))
    torch.cuda.synchronize()
    assert status == -1                                                       # IRBPP_ERR_ARG
    assert all(bool((t == -7).all()) for t in out)                            # nothing was launched
    with pytest.raises(_lib.IrbppError):
        mem.sample_pooled(4)


def test_invalid_value_and_too_few_transitions_on_the_device():
    rng = np.random.RandomState(4)
    m = make_model(3, 11, 2, rng)
    mem = _memory(m)
    good = values_for(m, 5, rng)
    bad = good.copy()
    bad[3] = np.nextafter(m.total(), f32(np.inf)) * f32(1.5)                  # past T: the padding leaf of P = 4
    assert m.find(bad[3])[0] >= m.N
    with pytest.raises(ValueError):
        mem.sample_pooled(5, values=_dev(bad))
    e, d = next((e, d) for e in range(m.N) for d in range(m.cap)
                if m.tree[e, d + m.cap - 1] != 0 and not m.valid(e, m.tree[e, d + m.cap - 1], d))
    bad[3] = f32(m.leaf_offsets()[e, d] + 0.5 * float(m.tree[e, d + m.cap - 1]))
    assert m.find(bad[3])[:3:2] == (e, d)
    with pytest.raises(ValueError):
        mem.sample_pooled(5, values=_dev(bad))
    few = replay.VectorReplayMemory(3, 16, 2, multi_step=3, device=DEV, use_hip=True)
    for _ in range(3):
        few.append(torch.rand(3, 2, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV), torch.ones(3, device=DEV),
                   torch.zeros(3, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError):
        few.sample_pooled(2, generator=torch.Generator().manual_seed(1), max_tries=8)


# ------------------------------------------------------------------ drawn on the device -------------------------------------
def _invalid_share(m, b, offsets):
    """The largest share of a segment's mass that lies on leaves the validity test refuses (float64 on the model's nodes)."""
    leaves = m.tree[:, m.cap - 1:].astype(np.float64)
    bad = np.array([[not m.valid(e, m.tree[e, d + m.cap - 1], d) for d in range(m.cap)] for e in range(m.N)])
    keep = leaves.ravel() > 0
    off, p, bad = offsets.ravel()[keep], leaves.ravel()[keep], bad.ravel()[keep]
    order = np.argsort(off, kind="stable")
    xs = np.concatenate([off[order], [off[order][-1] + p[order][-1]]])
    cum = np.concatenate([[0.0], np.cumsum((p * bad)[order])])
    seg = float(f32(m.total()) / f32(b))
    edges = np.arange(b + 1) * seg
    mass = np.diff(np.interp(edges, xs, cum))
    return float(mass.max() / seg)


@pytest.mark.parametrize("n_env,cap,obs_len,b", [(1, 64, 1, 1), (3, 64, 300, 257), (65, 11, 1, 1024), (4097, 11, 1, 255),
                                                 (8192, 11, 1, 1024), (1, 8200, 1, 255)])
def test_pooled_sample_drawn_on_the_device(n_env, cap, obs_len, b):
    """values=None.  On the model no segment has more than half of its mass on invalid leaves, so with max_tries = 64 a draw
    fails with probability at most 2^-64: no failure is flagged, every draw is valid, lies in its own segment (the returned
    leaf's stretch of [0, T) meets [j, j + 1) * segment up to one float32 ulp of T at the segment's ends), the batch is the
    model's for those leaves, and the same seed gives the same batch twice."""
    rng = np.random.RandomState(n_env + cap + b)
    m = make_model(n_env, cap, obs_len, rng, invalid_prio=0.03)
    offsets = m.leaf_offsets()
    share = _invalid_share(m, b, offsets)
    print(f"largest invalid share of a segment: {share:.4f}")
    assert share <= 0.5
    mem = _memory(m)
    one = mem.sample_pooled(b, generator=torch.Generator().manual_seed(11), max_tries=64)       # raises if a failure is flagged
    two = mem.sample_pooled(b, generator=torch.Generator().manual_seed(11), max_tries=64)
    other = mem.sample_pooled(b, generator=torch.Generator().manual_seed(12), max_tries=64)
    for x, y in zip(one, two):
        assert torch.equal(x, y)
    assert b < 64 or not torch.equal(one[0], other[0])
    idx = one[0].cpu().numpy()
    T = m.total()
    seg, ulp = float(f32(T) / f32(b)), float(np.spacing(T))
    found = []
    for j, (e, t) in enumerate(idx):
        assert 0 <= e < m.N and cap - 1 <= t <= 2 * cap - 2
        d, p = t - (cap - 1), m.tree[e, t]
        assert m.valid(e, p, d), (j, e, d)
        assert offsets[e, d] <= (j + 1) * seg + ulp and offsets[e, d] + float(p) >= j * seg - ulp, (j, e, d)
        found.append((e, p, d, t))
    assert_batch(one, m.batch_for(found)[0])


# ------------------------------------------------------------------ update ---------------------------------------------------
@pytest.mark.parametrize("n_env,cap,b", [(1, 11, 1), (3, 64, 255), (65, 11, 257), (3, 11, 1024), (1, 8200, 257), (4097, 64, 1024)])
def test_pooled_update_against_the_model(n_env, cap, b):
    """Random triples with many duplicates (3 envs x 11 leaves under 1024 triples), ignored triples in their midst, and placed
    ones: a leaf listed at positions 3 and 200 and again at b - 2 (first and last occurrence in different waves), the two
    children of one node in one env (every ancestor shared above the leaf level), one tree index in two envs.  Trees and
    maxima equal the model's; the trees the update left are sums of their leaves throughout."""
    rng = np.random.RandomState(n_env * 7 + cap + b)
    m = make_model(n_env, cap, 1, rng)
    mem = _memory(m)
    env, ti, pr = random_triples(m, b, rng)
    if b >= 255:
        env[[3, 200, b - 2]], ti[[3, 200, b - 2]] = env[3], ti[3]
        pair = 2 * int(rng.randint((cap - 1) // 2, cap - 1)) + 1                # the left child of a node whose children are leaves
        assert pair >= cap - 1 and pair + 1 <= 2 * cap - 2
        env[[10, 130]], ti[10], ti[130] = env[10], pair, pair + 1
        env[20], env[150], ti[[20, 150]] = 0, n_env - 1, ti[20]
    before = m.tree.copy()
    m.update(zip(env, ti, pr))
    mem.update_priorities_pooled(_dev(np.stack([env, ti], axis=1)), _dev(pr), powered=True)
    np.testing.assert_array_equal(mem.sum_tree.cpu().numpy(), m.tree)
    np.testing.assert_array_equal(mem.max.cpu().numpy(), m.max)
    np.testing.assert_array_equal(m.tree, rebuild(m.tree[:, cap - 1:]))
    assert b == 1 or not np.array_equal(before, m.tree)


# ------------------------------------------------------------------ end to end -----------------------------------------------
def test_sample_learn_update_end_to_end():
    """256 memories, a learning batch of 64: sample_pooled -> learn_loss (stub networks: fixed linear maps of the states) ->
    update_priorities_pooled; afterwards the trees and maxima are the model's after the same triples."""
    n_env, cap, s_rows, atoms, b = 256, 64, 4, 31, 64
    rng = np.random.RandomState(9)
    m = make_model(n_env, cap, 5 * s_rows, rng, invalid_prio=1e-3)
    m.actions %= s_rows
    mem = _memory(m)
    g = torch.Generator().manual_seed(2)
    w_v = (torch.randn(5 * s_rows, atoms, generator=g) * 0.5).to(DEV)
    w_on = (torch.randn(5 * s_rows, s_rows * atoms, generator=g) * 0.5).to(DEV).requires_grad_()
    w_tg = (torch.randn(5 * s_rows, s_rows * atoms, generator=g) * 0.5).to(DEV)
    online = lambda st: (st @ w_v, (st @ w_on).view(-1, s_rows, atoms))         # noqa: E731
    target = lambda st: (st @ w_v, (st @ w_tg).view(-1, s_rows, atoms))         # noqa: E731
    batch = mem.sample_pooled(b, generator=torch.Generator().manual_seed(7))
    idx, weights = batch[0], batch[6]
    loss = replay.learn_loss(online, target, batch, torch.linspace(-1.0, 8.0, atoms, device=DEV), 0.99 ** 3, -1.0, 8.0)
    (weights * loss).mean().backward()
    assert loss.shape == (b,) and bool(torch.isfinite(loss).all()) and bool((loss >= 0).all()) and bool(w_on.grad.abs().sum() > 0)
    mem.update_priorities_pooled(idx, loss.detach())
    pr = torch.pow(loss.detach(), mem.priority_exponent).cpu().numpy()
    idx = idx.cpu().numpy()
    m.update(zip(idx[:, 0], idx[:, 1], pr))
    np.testing.assert_array_equal(mem.sum_tree.cpu().numpy(), m.tree)
    np.testing.assert_array_equal(mem.max.cpu().numpy(), m.max)
