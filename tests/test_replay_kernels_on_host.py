"""The source of csrc/irbpp_replay.hip and csrc/irbpp_replay_pool.hip compiled for the host (tests/host/replay_host.cpp: each
launch with the C API's grid, block and dynamic LDS bytes, its threads in lockstep) against the definitions, without a GPU:
oracle/replay.py per env and the bottom-up rebuild for the per-env kernels, PoolModel (tests/test_replay_pooled_cpu.py) for
the pooled ones, and for the device-drawn samples the generator restated in Python integers (uniform01 of
tests/test_gpu_replay_shapes.py) with each draw modelled as v = f32(f32(j) * seg + f32(u * seg)), attempts walked in order.

Indices, priorities, flags, actions, states, trees, maxima and the n-step returns (the chain f32(ret + f32(r * s)): the
harness is built with -ffp-contract=off) are compared bit for bit; the importance weights within the 1e-6 that
tests/test_replay.py states for them (powf is the C library's).  Every output has canary elements behind its end.

Shapes are the smallest at which each kernel can go wrong; one workgroup costs 256 host threads (1024 for the pooled update)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from host_harness import build_shared
from irbpp_amd import _lib as L
from oracle.replay import ReplayMemory as OracleReplay
import test_gpu_replay_shapes as G
from test_gpu_replay_shapes import POOL_RNG_ENV, uniform01
from test_replay_pooled_cpu import ATOL, PoolModel, assert_batch, f32, make_model, random_triples, rebuild, values_for

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "replay_host.cpp")
OUT = os.path.join(HERE, "host", "_build", "libreplay_host.so")
CANARY, TAIL = 77, 5
ENTRY_POINTS = ("sumtree_find", "sumtree_sample", "sumtree_update", "masked_argmax", "replay_gather", "replay_append",
                "replay_pool_sample", "replay_pool_gather", "replay_pool_update")


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(build_shared(SRC, OUT))
    for name in ENTRY_POINTS:                                  # the signatures of the C API's functions, stream included
        fn = getattr(lib, "host_" + name)
        fn.restype, fn.argtypes = L.SIGNATURES["irbpp_" + name]
    lib.host_uniform01.restype, lib.host_uniform01.argtypes = C.c_float, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    return lib


def _p(a):
    return C.c_void_p(None if a is None else a.ctypes.data)


def guarded(a):
    """A contiguous copy of `a` with TAIL canary elements behind it, and the view of its front."""
    a = np.asarray(a)
    buf = np.full(a.size + TAIL, CANARY, dtype=a.dtype)
    buf[:a.size] = a.ravel()
    return buf, buf[:a.size].reshape(a.shape)


def out(n, dtype):
    return np.full(n + TAIL, CANARY, dtype=dtype)


def intact(buf, n):
    """The first n elements of an output; the canaries behind them must have survived."""
    assert (buf[n:] == CANARY).all(), "a kernel wrote past the end of an output"
    return buf[:n]


class HostMemory(object):
    """The tensors of a VectorReplayMemory as numpy arrays, each with canaries behind it."""
    FIELDS = (("states", f32), ("actions", np.int64), ("rewards", f32), ("nonterminals", np.uint8), ("timesteps", np.int32),
              ("tree", f32), ("max", f32), ("index", np.int64), ("full", np.uint8), ("t", np.int32), ("scaling", f32))

    def __init__(self, n, cap, obs_len, n_step=3, discount=0.99, **arrays):
        self.n, self.cap, self.obs_len, self.n_step = n, cap, obs_len, n_step
        shapes = dict(states=(n, cap, obs_len), actions=(n, cap), rewards=(n, cap), nonterminals=(n, cap), timesteps=(n, cap),
                      tree=(n, 2 * cap - 1), max=(n,), index=(n,), full=(n,), t=(n,), scaling=(n_step,))
        arrays.setdefault("max", np.ones(n))
        arrays.setdefault("scaling", [discount ** i for i in range(n_step)])
        self._bufs = {}
        for name, dt in self.FIELDS:
            a = np.asarray(arrays.get(name, np.zeros(shapes[name]))).astype(dt).reshape(shapes[name])
            self._bufs[name], view = guarded(a)
            setattr(self, name, view)

    def check_canaries(self):
        for name, _ in self.FIELDS:
            intact(self._bufs[name], getattr(self, name).size)

    def view(self):
        return L.IrbppReplayView(*[self._bufs[k].ctypes.data for k in ("states", "actions", "rewards", "nonterminals", "tree", "index",
                                                                       "full", "scaling")], self.n, self.cap, self.obs_len, self.n_step)

    def store(self):
        return L.IrbppReplayStore(*[self._bufs[k].ctypes.data for k in ("states", "actions", "rewards", "nonterminals", "timesteps",
                                                                        "tree", "max", "index", "full", "t")], self.n, self.cap, self.obs_len)


def memory_of(m):
    """A PoolModel's arrays as a HostMemory."""
    return HostMemory(m.N, m.cap, m.states.shape[2], m.n, states=m.states, actions=m.actions, rewards=m.rewards,
                      nonterminals=m.nonterminals, tree=m.tree, max=m.max, index=m.index, full=m.full)


# ------------------------------------------------------------------ the generator --------------------------------------------
def test_uniform01_is_the_documented_counter_generator(host):
    """seed with the top bit set, env 0xFFFFFFFF (the pooled draws' field), j >= 256 (it is shifted by 8 bits: it meets the env
    field only from 2^24 on, as attempt meets j from 256 on), attempt >= 1 -- and one number moved from field to field, which
    gives another result."""
    table = [(0, 0, 0, 0), (1, 2, 3, 4), (0x8000000000000001, 5, 0, 0), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 1023, 63),
             (12345, POOL_RNG_ENV, 256, 1), (12345, 0, 257, 0), (12345, 257, 0, 0), (12345, 0, 0, 257), (12345, 0, 1, 0),
             (12345, 0, 0, 256), (7, 4096, 1 << 24, 2), (7, 4097, 0, 2), (0x9E3779B97F4A7C15, 8191, 255, 15), (7, 1, 0xFFFFFFFF, 0xFFFFFFFF)]
    got = [host.host_uniform01(*row) for row in table]
    want = [uniform01(*row) for row in table]
    assert [f32(g) for g in got] == want
    assert want[8] == want[9] and want[10] == want[11]          # the fields overlap: attempt 256 is j + 1, j = 2^24 is env + 1
    assert len(set(want)) == len(want) - 2
    rng = np.random.RandomState(3)
    for _ in range(2000):
        row = (int(rng.randint(0, 1 << 62)) * 4 + int(rng.randint(4)), int(rng.randint(0, 1 << 32)), int(rng.randint(0, 1 << 32)),
               int(rng.randint(0, 1 << 32)))
        assert f32(host.host_uniform01(*row)) == uniform01(*row), row


# ------------------------------------------------------------------ irbpp_sumtree_find ---------------------------------------
def _find(host, tree, n, cap, values):
    b = values.shape[1]
    prob, data_idx, tree_idx = out(n * b, f32), out(n * b, np.int64), out(n * b, np.int64)
    values = np.ascontiguousarray(values, dtype=f32)
    assert host.host_sumtree_find(_p(tree), n, cap, _p(values), b, _p(prob), _p(data_idx), _p(tree_idx), None) == 0
    return [intact(x, n * b).reshape(n, b) for x in (prob, data_idx, tree_idx)]


@pytest.mark.parametrize("n,b,cap", [(1, 255, 1), (1, 257, 2), (5, 51, 11), (1, 257, 11), (257, 1, 64), (3, 85, 64), (1, 257, 64)])
def test_find_at_the_comparison_edges(host, n, b, cap):
    """n * b = 255 and 257 (one workgroup and one thread into the second).  Values: 0, the total, the float above it, every
    internal node's `v <= left` tie with its two float32 neighbours, the leaves' prefix sums; each equals SegmentTree.find."""
    rng = np.random.RandomState(cap * 1000 + b)
    leaves = rng.uniform(0.05, 2.0, size=(n, cap)).astype(f32)
    leaves[rng.rand(n, cap) < 0.25] = 0.0
    leaves[:, 0] = np.maximum(leaves[:, 0], f32(0.5))
    tree = rebuild(leaves)
    values = np.zeros((n, b), dtype=f32)
    ties = 0
    for e in range(n):
        total = tree[e, 0]
        edges = np.array([G._boundary(tree[e], i) for i in range(cap - 1)], dtype=f32)
        pre = np.cumsum(leaves[e], dtype=f32)
        pool = np.concatenate([[f32(0), total, np.nextafter(total, f32(np.inf))], edges, np.nextafter(edges, f32(np.inf)),
                               np.nextafter(edges, f32(-np.inf)), pre]).astype(f32)
        pool = np.roll(pool, -e)                                            # (b = 1: env e takes the e-th value of the pool)
        values[e] = np.concatenate([pool, rng.uniform(0, total, size=b).astype(f32)])[:b]
        ties += len(set(values[e]) & set(edges))
    assert cap == 1 or ties > 0
    prob, data_idx, tree_idx = _find(host, tree, n, cap, values)
    for e in range(n):
        ref = [G._oracle_tree(tree[e], cap).find(v) for v in values[e]]
        np.testing.assert_array_equal(tree_idx[e], [r[2] for r in ref])
        np.testing.assert_array_equal(data_idx[e], [r[1] for r in ref])
        np.testing.assert_array_equal(prob[e], np.array([r[0] for r in ref], dtype=f32))


# ------------------------------------------------------------------ drawn samples, exact -------------------------------------
def _ring(n, cap, filled, w, n_step, b, rng):
    """Leaves, write indices and full flags of n rings: filled == cap a full ring written up to w, else `filled` transitions.
    A quarter of the leaves is 0.  Of the leaves the validity test refuses for their position, the one n_step behind the write
    index carries 0.6 of a segment's mass and the one at the write index (not full: the newest transition) 0.2, the others
    none: draws do meet them, and no segment lies wholly on them."""
    leaves = rng.uniform(0.05, 2.0, size=(n, cap)).astype(f32)
    leaves[rng.rand(n, cap) < 0.25] = 0.0
    full = filled == cap
    index = w if full else filled
    if not full:
        leaves[:, filled:] = 0.0
    for k in range(n_step + 1):
        leaves[:, (index - k) % cap] = 0.0
    seg = leaves.sum(1) / b
    leaves[:, (index - (0 if full else 1)) % cap] = 0.2 * seg
    leaves[:, (index - n_step) % cap] = 0.6 * seg
    return leaves, np.full(n, index, dtype=np.int64), np.full(n, full, dtype=np.uint8)


def _draw_per_env(tree, cap, w, n_step, b, env, j, seed, max_tries):
    """-> (prob, data_idx, tree_idx, attempts, ok, refused) of draw j of env: what irbpp_sumtree_sample_kernel is documented to
    do.  refused: the distances (w - d) % cap of the attempts that were redrawn."""
    oracle = G._oracle_tree(tree, cap)
    seg = f32(tree[0] / f32(b))
    lo = f32(f32(j) * seg)
    refused = []
    for attempt in range(max_tries):
        v = f32(lo + f32(uniform01(seed, env, j, attempt) * seg))
        p, d, t = oracle.find(v)
        if (w - d) % cap > n_step and (d - w) % cap >= 1 and p != 0:
            return p, d, t, attempt + 1, True, refused
        refused.append((w - d) % cap)
    return p, d, t, max_tries, False, refused


@pytest.mark.parametrize("n,cap,b,n_step,filled,w,tries", [
    (3, 64, 85, 3, 64, 0, 64), (1, 64, 257, 1, 64, 63, 64), (2, 11, 5, 3, 11, 5, 64), (3, 100, 20, 3, 40, 40, 64),
    (1, 11, 255, 1, 11, 10, 64), (2, 16, 2, 3, 3, 3, 8), (1, 1, 1, 1, 1, 0, 3)])
def test_sample_per_env_is_the_modelled_draw(host, n, cap, b, n_step, filled, w, tries):
    """Full rings written up to 0, mid-ring and cap - 1, a ring that is not full, n_step 1 and 3; n * b = 255 and 257.  The last
    two cases hold too few transitions: some draw exhausts max_tries and `failed` is set.  Env, leaf, priority and indices
    equal the model's, attempts counted through the generator's `attempt` field."""
    rng = np.random.RandomState(cap * 100 + b)
    leaves, index, _ = _ring(n, cap, filled, w, n_step, b, rng)
    starved = filled <= n_step
    if starved:
        leaves[:, :filled] = 1.0                                            # all the mass on transitions without successors
    tree = rebuild(leaves)
    for seed in range(0x8000000000000000 + cap * b, 0x8000000000000000 + cap * b + 8):
        want = [[_draw_per_env(tree[e], cap, int(index[e]), n_step, b, e, j, seed, tries) for j in range(b)] for e in range(n)]
        flat = [x for row in want for x in row]
        met = set(a for x in flat for a in x[5])
        if n * b < 255 or (n_step in met and max(x[3] for x in flat) > 1):
            break                                       # a seed with which some draw lands exactly n_step behind the write index,
    else:                                               # the last distance the test refuses, and is drawn again
        raise AssertionError("fixture: no draw meets the leaf n_step behind the write index")
    assert starved == (not all(x[4] for x in flat))
    prob, data_idx, tree_idx, failed = out(n * b, f32), out(n * b, np.int64), out(n * b, np.int64), out(1, np.int32)
    failed[0] = 0
    assert host.host_sumtree_sample(_p(tree), _p(index), n, cap, b, n_step, seed, tries, _p(prob), _p(data_idx), _p(tree_idx),
                                    _p(failed), None) == 0
    np.testing.assert_array_equal(intact(tree_idx, n * b), [x[2] for x in flat])
    np.testing.assert_array_equal(intact(data_idx, n * b), [x[1] for x in flat])
    np.testing.assert_array_equal(intact(prob, n * b), np.array([x[0] for x in flat], dtype=f32))
    assert intact(failed, 1)[0] == (1 if starved else 0)


def _draw_pooled(m, b, j, seed, max_tries):
    """-> (env, prob, data_idx, tree_idx), attempts, ok, padding met: what irbpp_replay_pool_sample_kernel is documented to do."""
    seg = f32(m.total() / f32(b))
    lo = f32(f32(j) * seg)
    padding = False
    for attempt in range(max_tries):
        v = f32(lo + f32(uniform01(seed, POOL_RNG_ENV, j, attempt) * seg))
        e, p, d, t, _ = m.find(v)
        if e >= m.N:                                                         # a padding leaf: the last env's first leaf, priority 0
            e, p, d, t, padding = m.N - 1, f32(0), 0, m.cap - 1, True
            continue
        if m.valid(e, p, d):
            return (e, p, d, t), attempt + 1, True, padding
    return (e, p, d, t), max_tries, False, padding


def _pool_sample(host, mem, b, values, seed, tries, beta):
    o = [out(b, dt) for dt in (np.int64, f32, np.int64, np.int64, f32)]
    failed = out(1, np.int32)
    failed[0] = 0
    view = mem.view()
    values = None if values is None else np.ascontiguousarray(values, dtype=f32)
    assert host.host_replay_pool_sample(C.byref(view), b, _p(values), seed, tries, beta, *[_p(x) for x in o], _p(failed), None) == 0
    return [intact(x, b) for x in o], int(intact(failed, 1)[0])


def _pool_gather(host, mem, env, data_idx):
    b, obs_len = len(env), mem.obs_len
    o = [out(b * obs_len, f32), out(b, np.int64), out(b, f32), out(b * obs_len, f32), out(b, f32)]
    view = mem.view()
    env, data_idx = np.ascontiguousarray(env, dtype=np.int64), np.ascontiguousarray(data_idx, dtype=np.int64)
    assert host.host_replay_pool_gather(C.byref(view), b, _p(env), _p(data_idx), *[_p(x) for x in o], None) == 0
    st, ac, re, ns, nt = [intact(x, x.size - TAIL) for x in o]
    return st.reshape(b, obs_len), ac, re, ns.reshape(b, obs_len), nt.reshape(b, 1)


def _assert_pooled_batch(host, mem, m, found, got, rows=None):
    """got: the five arrays of the sample launch for the leaves `found`; gathers (the first `rows` rows) and compares all."""
    env, prob, data_idx, tree_idx, weight = got
    want, wprob, wdata = m.batch_for(found)
    np.testing.assert_array_equal(env, want[0][:, 0])
    np.testing.assert_array_equal(tree_idx, want[0][:, 1])
    np.testing.assert_array_equal(prob, wprob)
    np.testing.assert_array_equal(data_idx, wdata)
    np.testing.assert_allclose(weight, want[6], rtol=0, atol=ATOL)
    r = len(found) if rows is None else rows
    st, ac, re, ns, nt = _pool_gather(host, mem, env[:r], data_idx[:r])
    batch = (np.stack([env, tree_idx], axis=1)[:r], st, ac, re, ns, nt, weight[:r])
    assert_batch([torch.from_numpy(np.ascontiguousarray(x)) for x in batch], [w[:r] for w in want])
    np.testing.assert_array_equal(re, want[3][:r])                           # the n-step chain, bit for bit
    mem.check_canaries()


@pytest.mark.parametrize("n_env,cap,b", [(1, 64, 1), (3, 11, 257), (65, 11, 1024), (4097, 11, 255), (3, 64, 255)])
def test_sample_pooled_is_the_modelled_draw(host, n_env, cap, b):
    """N = 1, 3 (a padding leaf), 65 (a top tree wider than a wave) and 4097 (wider than the workgroup); B = 1, 255, 257, 1024.
    Env, leaf, priority and indices of every draw equal the model's; weights, and the gathered batch, follow."""
    rng = np.random.RandomState(n_env + cap + b)
    m = make_model(n_env, cap, 2, rng, invalid_prio=0.01)
    mem = memory_of(m)
    for seed in range(0x8000000000000000 + 31 * b, 0x8000000000000000 + 31 * b + 8):
        drawn = [_draw_pooled(m, b, j, seed, 64) for j in range(b)]
        if b < 50 or max(a for _, a, _, _ in drawn) > 1:
            break                                                            # a seed with which some draw needs a second attempt
    else:
        raise AssertionError("fixture: every draw is valid at once")
    assert all(ok for _, _, ok, _ in drawn)
    got, failed = _pool_sample(host, mem, b, None, seed, 64, m.beta)
    assert failed == 0
    _assert_pooled_batch(host, mem, m, [f for f, _, _, _ in drawn], got, rows=min(b, 257))


def test_sample_pooled_redraws_after_a_padding_leaf(host):
    """Three memories under a top tree of four leaves.  The last segment's end is the one place where a drawn position can pass
    the pooled total (by the rounding of total / B and of j * segment): the seed is searched for, with the generator restated on
    numpy's uint64, until the MODEL's first attempt of the last draw lands on the padding leaf; the kernel must redraw it."""
    n_env, cap, b = 3, 11, 255
    j = b - 1
    seeds = np.arange(1 << 22, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = seeds + np.uint64(0x9E3779B97F4A7C15) * np.uint64(((POOL_RNG_ENV << 32) ^ (j << 8) ^ 0xD1B54A32D192ED03) & G.M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    top24 = (z >> np.uint64(40)).astype(np.int64)
    nearly_one = [int(s) for s in seeds[np.argsort(-top24, kind="stable")[:32]]]          # the largest u first
    for fixture in range(40):                                               # (whether total / B rounds up depends on the total)
        m = make_model(n_env, cap, 1, np.random.RandomState(fixture), invalid_prio=0.01)
        hits = [s for s in nearly_one if _draw_pooled(m, b, j, s, 1)[3]]
        if hits:
            break
    assert hits, "fixture: no seed sends the last draw past the pooled total"
    seed = hits[0]
    mem = memory_of(m)
    drawn = [_draw_pooled(m, b, k, seed, 64) for k in range(b)]
    assert drawn[j][3] and drawn[j][1] > 1 and all(ok for _, _, ok, _ in drawn)
    got, failed = _pool_sample(host, mem, b, None, seed, 64, m.beta)
    assert failed == 0
    _assert_pooled_batch(host, mem, m, [f for f, _, _, _ in drawn], got)
    # with one try the padding leaf is the answer: the last env's first leaf with priority 0, and the failure flag
    got, failed = _pool_sample(host, mem, b, None, seed, 1, m.beta)
    assert failed == 1 and (got[0][j], got[1][j], got[2][j], got[3][j]) == (n_env - 1, 0.0, 0, cap - 1)


def test_sample_pooled_with_too_few_transitions_sets_failed(host):
    """Every memory holds n_step transitions: nothing has its successors, max_tries is exhausted, the last attempt is reported."""
    n_env, cap, n_step, b = 3, 16, 3, 2
    leaves = np.zeros((n_env, cap), dtype=f32)
    leaves[:, :n_step] = 1.0
    mem = HostMemory(n_env, cap, 1, n_step, tree=rebuild(leaves), index=np.full(n_env, n_step))
    m = PoolModel(mem.tree, mem.index, mem.full, mem.states, mem.actions, mem.rewards, mem.nonterminals, n_step, 0.4)
    drawn = [_draw_pooled(m, b, j, 9, 8) for j in range(b)]
    assert not any(ok for _, _, ok, _ in drawn)
    got, failed = _pool_sample(host, mem, b, None, 9, 8, 0.4)
    assert failed == 1
    for k in range(4):
        np.testing.assert_array_equal(got[k], [f[k] for f, _, _, _ in drawn])


# ------------------------------------------------------------------ pooled: supplied values, gather, update ------------------
@pytest.mark.parametrize("n_env,cap,obs_len,b,max_at", [
    (1, 11, 1, 1, 0), (3, 64, 300, 255, 200), (65, 11, 1, 257, 3), (3, 11, 300, 1024, 456), (4097, 11, 1, 1024, 5),
    (8192, 11, 1, 257, 256), (1, 8200, 1, 257, 250), (65, 64, 1, 64, 63)])
def test_pooled_sample_and_gather_for_supplied_values(host, n_env, cap, obs_len, b, max_at):
    """tests/test_gpu_replay_pooled.py's cases; at obs_len 300 the first 257 rows are gathered (one workgroup a row)."""
    rng = np.random.RandomState(n_env * 31 + cap + b)
    m = make_model(n_env, cap, obs_len, rng, rare=True)
    mem = memory_of(m)
    values = values_for(m, b, rng, place={max_at: m.rare}, avoid=(m.rare,))
    found = [m.find(v)[:4] for v in values]
    got, failed = _pool_sample(host, mem, b, values, 0, 64, m.beta)
    assert failed == 0
    _assert_pooled_batch(host, mem, m, found, got, rows=min(b, 257) if obs_len > 1 else None)
    assert got[4][max_at] == 1.0 and (b == 1 or np.delete(got[4], max_at).max() < 0.5)


def test_pooled_invalid_values_set_failed_and_foreign_rows_are_zeros(host):
    """A value past the pooled total (the padding leaf of P = 4) and one on a leaf that memory.py:175 refuses set `failed`;
    the gather writes zeros for envs outside [0, N) and takes a negative data index modulo the capacity."""
    rng = np.random.RandomState(4)
    m = make_model(3, 11, 2, rng)
    mem = memory_of(m)
    good = values_for(m, 5, rng)
    assert _pool_sample(host, mem, 5, good, 0, 64, m.beta)[1] == 0
    bad = good.copy()
    bad[3] = np.nextafter(m.total(), f32(np.inf)) * f32(1.5)
    assert m.find(bad[3])[0] >= m.N
    got, failed = _pool_sample(host, mem, 5, bad, 0, 64, m.beta)
    assert failed == 1 and (got[0][3], got[1][3], got[2][3], got[3][3]) == (m.N - 1, 0.0, 0, m.cap - 1)
    e, d = next((e, d) for e in range(m.N) for d in range(m.cap)
                if m.tree[e, d + m.cap - 1] != 0 and not m.valid(e, m.tree[e, d + m.cap - 1], d))
    bad[3] = f32(m.leaf_offsets()[e, d] + 0.5 * float(m.tree[e, d + m.cap - 1]))
    got, failed = _pool_sample(host, mem, 5, bad, 0, 64, m.beta)
    assert failed == 1 and (got[0][3], got[2][3]) == (e, d)
    env = np.array([0, -1, 3, 2, 1 << 32], dtype=np.int64)
    data = np.array([-3, 1, 1, 5 + 11, 0], dtype=np.int64)
    st, ac, re, ns, nt = _pool_gather(host, mem, env, data)
    rows = {0: (0, 8), 3: (2, 5)}                                              # (-3 and 16 modulo 11)
    for k in range(5):
        if k in rows:
            s0, a, r, s1, flag = m.transition(*rows[k])
            assert np.array_equal(st[k], s0) and ac[k] == a and re[k] == r and np.array_equal(ns[k], s1) and nt[k, 0] == flag
        else:
            assert not st[k].any() and ac[k] == 0 and re[k] == 0 and not ns[k].any() and nt[k, 0] == 0


def _pool_update(host, mem, env, ti, pr):
    env, ti, pr = (np.ascontiguousarray(a, dtype=dt) for a, dt in ((env, np.int64), (ti, np.int64), (pr, f32)))
    return host.host_replay_pool_update(mem._bufs["tree"].ctypes.data, mem._bufs["max"].ctypes.data, mem.n, mem.cap, _p(env), _p(ti),
                                        _p(pr), len(env), None)


@pytest.mark.parametrize("n_env,cap,b", [(1, 11, 1), (3, 64, 255), (65, 11, 257), (3, 11, 1024), (1, 8200, 257), (4097, 64, 1024),
                                         (2, 1, 64), (3, 2, 65)])
def test_pooled_update_against_the_model(host, n_env, cap, b):
    """tests/test_gpu_replay_pooled.py's cases with its placed triples (a leaf listed at 3, 200 and b - 2; the two children of
    one node; one tree index in two envs), and capacities 1 and 2."""
    rng = np.random.RandomState(n_env * 7 + cap + b)
    m = make_model(n_env, cap, 1, rng)
    mem = memory_of(m)
    env, ti, pr = random_triples(m, b, rng)
    if b >= 255:
        env[[3, 200, b - 2]], ti[[3, 200, b - 2]] = env[3], ti[3]
        pair = 2 * int(rng.randint((cap - 1) // 2, cap - 1)) + 1
        assert pair >= cap - 1 and pair + 1 <= 2 * cap - 2
        env[[10, 130]], ti[10], ti[130] = env[10], pair, pair + 1
        env[20], env[150], ti[[20, 150]] = 0, n_env - 1, ti[20]
    before = m.tree.copy()
    m.update(zip(env, ti, pr))
    assert _pool_update(host, mem, env, ti, pr) == 0
    np.testing.assert_array_equal(mem.tree, m.tree)
    np.testing.assert_array_equal(mem.max, m.max)
    np.testing.assert_array_equal(m.tree, rebuild(m.tree[:, cap - 1:]))
    assert b == 1 or not np.array_equal(before, m.tree)
    mem.check_canaries()


def test_argument_refusals_answer_minus_one(host):
    """The C API's limits, mirrored: 1025 triples, 1025 pooled draws, 8193 envs under the top tree, 257 per-env draws, a
    capacity of 8193 for the per-env update; nothing is launched."""
    mem = HostMemory(1, 4, 1, tree=rebuild(np.ones((1, 4), dtype=f32)), full=[1])
    big = np.zeros(1025, dtype=np.int64)
    assert _pool_update(host, mem, big, big + 3, big.astype(f32)) == -1
    o = [out(1025, dt) for dt in (np.int64, f32, np.int64, np.int64, f32, np.int32)]
    view = mem.view()
    assert host.host_replay_pool_sample(C.byref(view), 1025, None, 0, 8, 0.4, *[_p(x) for x in o], None) == -1
    wide = HostMemory(8193, 1, 1)
    view = wide.view()
    assert host.host_replay_pool_sample(C.byref(view), 1, None, 0, 8, 0.4, *[_p(x) for x in o], None) == -1
    view = mem.view()
    g = [out(257, dt) for dt in (f32, np.int64, f32, f32, f32, f32)]
    assert host.host_replay_gather(C.byref(view), 257, 0.4, _p(big), _p(big.astype(f32)), *[_p(x) for x in g], None) == -1
    tree = np.zeros(2 * 8193 - 1, dtype=f32)
    ti, pr, mx = np.full(1, 8192, dtype=np.int64), np.ones(1, dtype=f32), np.ones(1, dtype=f32)
    assert host.host_sumtree_update(_p(tree), _p(mx), 1, 8193, _p(ti), _p(pr), 1, None, None) == -1
    assert not tree.any() and all((x == CANARY).all() for x in o + g)
    mem.check_canaries()


# ------------------------------------------------------------------ irbpp_sumtree_update -------------------------------------
def _update(host, tree_buf, max_buf, n, cap, ti, pr, mask):
    ti, pr = np.ascontiguousarray(ti, dtype=np.int64), np.ascontiguousarray(pr, dtype=f32)
    assert host.host_sumtree_update(_p(tree_buf), _p(max_buf), n, cap, _p(ti), _p(pr), ti.shape[1], _p(mask), None) == 0


@pytest.mark.parametrize("cap", [1, 2, 3, 11, 64, 130, 8192])
def test_update_per_env_rebuilds_every_level(host, cap):
    """tests/test_gpu_replay_shapes.py's three rounds on three envs, the middle one masked out: every leaf in one call; eight
    leaves with the first, the last and duplicates (the last value listed wins); then indices that are no leaf of the row --
    the last internal node, one past the row, negative, beyond 2^32 -- among real ones, with priorities that would show."""
    rng = np.random.RandomState(cap)
    n = 3
    mask = np.array([1, 0, 1], dtype=np.uint8)
    on = mask.astype(bool)
    junk = rng.uniform(1, 2, size=(n, 2 * cap - 1)).astype(f32)
    max0 = np.array([0.5, 7.0, 0.25], dtype=f32)
    tree_buf, tree = guarded(junk)
    max_buf, mx = guarded(max0)
    leaves = rng.uniform(0.05, 2.0, size=(n, cap)).astype(f32)
    leaves[rng.rand(n, cap) < 0.2] = 0.0
    order = np.stack([rng.permutation(cap) for _ in range(n)])
    _update(host, tree_buf, max_buf, n, cap, order + cap - 1, np.take_along_axis(leaves, order, axis=1), mask)
    want = rebuild(leaves)
    want[~on] = junk[~on]
    wmax = np.where(on, np.maximum(max0, leaves.max(1)), max0).astype(f32)
    np.testing.assert_array_equal(tree, want)
    np.testing.assert_array_equal(mx, wmax)

    x, y, z = (rng.randint(0, cap, size=n) for _ in range(3))
    d = np.stack([np.zeros(n, dtype=np.int64), np.full(n, cap - 1), x, y, x, z, np.full(n, cap - 1), x], axis=1)
    pr = rng.uniform(0.05, 3.0, size=(n, 8)).astype(f32)
    _update(host, tree_buf, max_buf, n, cap, d + cap - 1, pr, mask)
    for e in np.nonzero(on)[0]:
        for j in range(8):
            leaves[e, d[e, j]] = pr[e, j]
    want = rebuild(leaves)
    want[~on] = junk[~on]
    wmax = np.where(on, np.maximum(wmax, pr.max(1)), max0).astype(f32)
    np.testing.assert_array_equal(tree, want)
    np.testing.assert_array_equal(mx, wmax)

    real = np.stack([x, np.full(n, cap - 1), np.zeros(n, dtype=np.int64), y], axis=1) + cap - 1
    rp = rng.uniform(0.05, 3.0, size=(n, 4)).astype(f32)
    bad = [cap - 2, 2 * cap - 1, -1, (1 << 32) + cap - 1]
    mixed = np.stack([real[:, 0], np.full(n, bad[0]), real[:, 1], np.full(n, bad[1]), np.full(n, bad[2]), real[:, 2],
                      np.full(n, bad[3]), real[:, 3]], axis=1)
    mp = np.full((n, 8), 99.0, dtype=f32)
    mp[:, [0, 2, 5, 7]] = rp
    _update(host, tree_buf, max_buf, n, cap, mixed, mp, mask)
    for e in np.nonzero(on)[0]:
        for j in range(4):
            leaves[e, real[e, j] - (cap - 1)] = rp[e, j]
    want = rebuild(leaves)
    want[~on] = junk[~on]
    wmax = np.where(on, np.maximum(wmax, rp.max(1)), max0).astype(f32)
    np.testing.assert_array_equal(tree, want)
    np.testing.assert_array_equal(mx, wmax)
    intact(tree_buf, tree.size)
    intact(max_buf, n)


# ------------------------------------------------------------------ irbpp_replay_append --------------------------------------
@pytest.mark.parametrize("cap,obs_len", [(1, 1), (2, 300), (2, 1), (11, 1), (11, 300)])
def test_append_through_a_wrap_against_the_oracle(host, cap, obs_len):
    """Rings of capacity 1, 2 and 11 that start with priorities of their own (the sibling of a written leaf is no copy of it),
    written at even and odd leaves and at cap - 1, where the wrap sets `full`; rows of 1 and 300 floats handed over with a
    stride, int32 / int64 actions, float32 / float64 rewards, terminals, a valid mask.  After EVERY append all tensors equal the
    oracle's and each tree is the bottom-up rebuild of its leaves."""
    rng = np.random.RandomState(cap * 7 + obs_len)
    n, steps, pad = 4, 2 * cap + 3, 37
    leaves = rng.uniform(0.05, 2.0, size=(n, cap)).astype(f32)
    max0 = rng.uniform(0.5, 3.0, size=n).astype(f32)
    mem = HostMemory(n, cap, obs_len, tree=rebuild(leaves), max=max0)
    oracles = [OracleReplay(cap, obs_len, 0.99, 3) for _ in range(n)]
    for e, o in enumerate(oracles):
        o.transitions.sum_tree, o.transitions.max = mem.tree[e].copy(), max0[e]
    store = mem.store()
    for t in range(steps):
        wide = rng.uniform(0, 0.3, size=(n, obs_len + pad)).astype(f32)
        wide_buf = wide.ravel()[:(n - 1) * (obs_len + pad) + 5 + obs_len].copy()       # ends with the last env's row
        action = rng.randint(0, 500, size=n)
        reward = rng.uniform(0, 1, size=n)
        terminal = rng.rand(n) < 0.3
        valid = rng.rand(n) < 0.7 if t % 3 else np.ones(n, dtype=bool)
        a = action.astype(np.int32 if t % 2 else np.int64)
        r = reward.astype(f32) if t % 4 < 2 else reward.astype(np.float64)
        term, v = terminal.astype(np.uint8), None if valid.all() else valid.astype(np.uint8)
        state = C.c_void_p(wide_buf.ctypes.data + 5 * 4)
        assert host.host_replay_append(C.byref(store), state, obs_len + pad, _p(a), a.itemsize, _p(r), r.itemsize, _p(term), _p(v),
                                       None) == 0
        for e in np.nonzero(valid)[0]:
            oracles[e].append(wide[e, 5:5 + obs_len], action[e], r[e], bool(terminal[e]))
        tr = [o.transitions for o in oracles]
        np.testing.assert_array_equal(mem.tree, np.stack([x.sum_tree for x in tr]), err_msg=f"step {t}")
        np.testing.assert_array_equal(mem.tree, rebuild(mem.tree[:, cap - 1:]), err_msg=f"step {t}")
        np.testing.assert_array_equal(mem.states, np.stack([x.states for x in tr]))
        np.testing.assert_array_equal(mem.actions, np.stack([x.actions for x in tr]))
        np.testing.assert_array_equal(mem.rewards, np.stack([x.rewards for x in tr]))
        np.testing.assert_array_equal(mem.nonterminals, np.stack([x.nonterminals for x in tr]))
        np.testing.assert_array_equal(mem.timesteps, np.stack([x.timesteps for x in tr]))
        np.testing.assert_array_equal(mem.max, np.array([x.max for x in tr], dtype=f32))
        np.testing.assert_array_equal(mem.index, [x.index for x in tr])
        np.testing.assert_array_equal(mem.full, [x.full for x in tr])
        np.testing.assert_array_equal(mem.t, [o.t for o in oracles])
        mem.check_canaries()
    assert mem.full.all()
    assert host.host_replay_append(C.byref(store), state, obs_len - 1, _p(a), 4, _p(r), 4, _p(term), None, None) == -1
    assert host.host_replay_append(C.byref(store), state, obs_len + pad, _p(a), 2, _p(r), 4, _p(term), None, None) == -1


# ------------------------------------------------------------------ irbpp_masked_argmax --------------------------------------
@pytest.mark.parametrize("s", [1, 63, 64, 65, 500])
def test_masked_argmax_with_returned_waves(host, s):
    """One env (three waves of the workgroup return at once) and five (the second workgroup keeps one wave), q as a column slice
    (q_stride > S): the patterns of tests/test_gpu_replay_shapes.py -- maxima at the lanes' ends, ties between adjacent lanes,
    within one lane's stride and across the lane loop's trips, everything masked (0), -inf and +inf on valid candidates."""
    rng = np.random.RandomState(s)
    q, flags, want_first = G._argmax_rows(12, s, rng)
    want = np.where(flags, q, -np.inf).astype(f32).argmax(1)
    for e, i in want_first.items():
        assert want[e] == i, (e, i)
    for rows in ([0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [7, 8, 9, 10, 11], [5], [6], [7], [10]):
        n = len(rows)
        obs = rng.uniform(0.5, 1, size=(n, 5 * s + 9)).astype(f32)
        obs[:, :5 * s].reshape(n, s, 5)[:, :, 4] = flags[rows]
        wide = rng.randn(n, s + 11).astype(f32) + 100.0                        # larger than any q: a read outside the slice wins
        wide[:, 3:3 + s] = q[rows]
        wide_buf = wide.ravel()[:(n - 1) * (s + 11) + 3 + s].copy()            # both end with the last env's candidates
        obs_buf = obs.ravel()[:(n - 1) * (5 * s + 9) + 5 * s].copy()
        act = out(n, np.int64)
        assert host.host_masked_argmax(C.c_void_p(wide_buf.ctypes.data + 12), s + 11, _p(obs_buf), 5 * s + 9, s, n, _p(act), None) == 0
        np.testing.assert_array_equal(intact(act, n), want[rows], err_msg=f"S={s} envs {rows}")
    assert host.host_masked_argmax(_p(wide_buf), s - 1, _p(obs_buf), 5 * s + 9, s, 1, _p(act), None) == -1


# ------------------------------------------------------------------ irbpp_replay_gather --------------------------------------
@pytest.mark.parametrize("n,b,obs_len,beta,full,max_at", [
    (2, 1, 1, 0.4, True, 0), (2, 255, 1, 0.4, False, 200), (1, 256, 300, 1.0, True, 255), (2, 256, 1, 0.4, True, 197),
    (1, 65, 300, 0.0, False, 64)])
def test_gather_per_env_against_the_oracle(host, n, b, obs_len, beta, full, max_at):
    """tests/test_gpu_replay_shapes.py's fixture on numpy arrays: positions at the ring's end whose chain wraps, a terminal right
    behind a sample, at it and at the chain's end (for cap - 1 and cap - 3 that is the wrap), full and not-full rings, the
    largest weight owned by sample max_at (thread 197 and 255: wave 3).  data_idx comes from the find kernel, as in the product:
    it is never negative, and unlike the pooled gather this kernel has no guard for a negative index -- none is fed to it."""
    rng = np.random.RandomState(b * 1000 + obs_len)
    cap, n_step = 300, 3
    filled = cap if full else 200
    index = cap // 2 if full else filled
    ok = [d for d in range(filled) if (index - d) % cap > n_step and (d - index) % cap >= 1]
    special = [cap - 1, cap - 10, cap - 3] if full else [filled - n_step - 1, 0, 10]
    mid = [d for d in ok if 20 <= d < 140]
    rare = rng.choice(mid, size=n, replace=False)
    mid = [d for d in mid if d not in rare]
    pos = np.stack([np.array((special + list(rng.choice(mid, size=b)))[:b]) for _ in range(n)])
    pos[:, max_at] = rare
    states = rng.uniform(0, 0.3, size=(n, cap, obs_len)).astype(f32)
    actions = rng.randint(0, 500, size=(n, cap)).astype(np.int64)
    rewards = rng.uniform(0, 1, size=(n, cap)).astype(f32)
    nonterm = rng.rand(n, cap) >= 0.15
    leaves = rng.uniform(0.5, 2.0, size=(n, cap)).astype(f32)
    if not full:
        states[:, filled:], actions[:, filled:], rewards[:, filled:], nonterm[:, filled:], leaves[:, filled:] = 0, 0, 0, False, 0
    leaves[np.arange(n), rare] = 0.01
    for e in range(n):
        for k, off in enumerate((1, 0, n_step, 2)):
            if k < b:
                nonterm[e, (pos[e, k] + off) % cap] = False
        nonterm[e, pos[e, 0]] = True
        if b >= 3:
            nonterm[e, (pos[e, 2] + np.arange(n_step)) % cap] = True
    tree = rebuild(leaves)
    mem = HostMemory(n, cap, obs_len, n_step, states=states, actions=actions, rewards=rewards, nonterminals=nonterm, tree=tree,
                     index=np.full(n, index), full=np.full(n, full))
    chain = PoolModel(tree, mem.index, mem.full, states, actions, rewards, nonterm, n_step, beta)
    values = np.stack([[G._middle_of_leaf(tree[e], d + cap - 1) for d in pos[e]] for e in range(n)]).astype(f32)
    prob, data_idx, tree_idx = _find(host, mem._bufs["tree"], n, cap, values)
    np.testing.assert_array_equal(data_idx, pos)
    o = [out(n * b * obs_len, f32), out(n * b, np.int64), out(n * b, f32), out(n * b * obs_len, f32), out(n * b, f32), out(n * b, f32)]
    view = mem.view()
    prob, data_idx = np.ascontiguousarray(prob), np.ascontiguousarray(data_idx)
    assert host.host_replay_gather(C.byref(view), b, beta, _p(data_idx), _p(prob), *[_p(x) for x in o], None) == 0
    st, ac, re, ns, nt, w = [intact(x, x.size - TAIL) for x in o]
    st, ns = st.reshape(n * b, obs_len), ns.reshape(n * b, obs_len)
    for e in range(n):
        oracle = OracleReplay(cap, obs_len, 0.99, n_step, beta, 0.5)
        tr = oracle.transitions
        tr.states, tr.actions, tr.rewards, tr.nonterminals = states[e], actions[e], rewards[e], nonterm[e]
        tr.sum_tree, tr.index, tr.full = tree[e], index, full
        ti, wst, wac, wre, wns, wnt, ww = oracle.sample_at(values[e])
        sl = slice(e * b, (e + 1) * b)
        np.testing.assert_array_equal(tree_idx[e], ti)
        np.testing.assert_array_equal(st[sl], wst)
        np.testing.assert_array_equal(ac[sl], wac)
        np.testing.assert_allclose(re[sl], wre, rtol=0, atol=ATOL)
        np.testing.assert_array_equal(re[sl], np.array([chain.transition(e, int(d))[2] for d in pos[e]], dtype=f32))
        np.testing.assert_array_equal(ns[sl], wns)
        np.testing.assert_array_equal(nt[sl], wnt)
        np.testing.assert_allclose(w[sl], ww, rtol=0, atol=ATOL)
        assert w[sl][max_at] == 1.0 and (beta == 0.0 or b == 1 or np.delete(w[sl], max_at).max() < 0.5)
        if b >= 4:
            assert not ns[sl][0].any() and nt[sl][0] == 0.0                    # terminal at d + 1: blanked next state
            if max_at != 2:                                                    # terminal at d + n, chain alive: the flag alone
                assert nt[sl][2] == 0.0 and np.array_equal(ns[sl][2], states[e, (pos[e, 2] + n_step) % cap])
    mem.check_canaries()
