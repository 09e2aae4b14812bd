"""VectorReplayMemory.sample_pooled / update_priorities_pooled: the N per-env memories taken as ONE prioritised memory.

This file carries the definition as a plain numpy float32 model (PoolModel: loops, one value at a time) and holds the torch
formulation of irbpp_amd/replay.py to it: env, priority, data index and tree index for supplied values, flags, actions,
states and the trees after updates bit for bit; n-step returns and importance weights within the 1e-6 that
tests/test_gpu_replay_shapes.py grants those two.  The model itself is pinned to what exists: with N = 1 the pooled sample is
`sample`, with N > 1 a pooled draw ends at the leaf the env's own SegmentTree.find (oracle/replay.py) returns for the residual
value, and an update grouped by env leaves what `update_priorities` leaves.  tests/test_gpu_replay_pooled.py runs the HIP
launches against the same model."""
import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd.replay import VectorReplayMemory
from oracle.replay import SumTree

f32 = np.float32
ATOL = 1e-6                       # returns and weights (tests/test_gpu_replay_shapes.py)


def rebuild(leaves):
    """[N, cap] float32 leaves -> [N, 2*cap - 1] trees, every internal node f32(left + right)."""
    leaves = np.asarray(leaves, dtype=f32)
    n, cap = leaves.shape
    tree = np.zeros((n, 2 * cap - 1), dtype=f32)
    tree[:, cap - 1:] = leaves
    for i in range(cap - 2, -1, -1):
        tree[:, i] = tree[:, 2 * i + 1] + tree[:, 2 * i + 2]
    return tree


class PoolModel(object):
    """The definition.  Arrays of one VectorReplayMemory: tree [N, 2*cap-1], index, full, max [N], states [N, cap, obs_len],
    actions, rewards, nonterminals [N, cap]."""

    def __init__(self, tree, index, full, states, actions, rewards, nonterminals, n_step, beta, discount=0.99):
        self.tree = np.array(tree, dtype=f32)
        self.N, self.cap = self.tree.shape[0], (self.tree.shape[1] + 1) // 2
        self.index, self.full = np.array(index, dtype=np.int64), np.array(full, dtype=bool)
        self.max = np.ones(self.N, dtype=f32)
        self.states, self.actions = np.array(states, dtype=f32), np.array(actions, dtype=np.int64)
        self.rewards, self.nonterminals = np.array(rewards, dtype=f32), np.array(nonterminals, dtype=bool)
        self.n, self.beta = n_step, beta
        self.scaling = np.array([discount ** i for i in range(n_step)], dtype=f32)
        self._top = None

    # -- top tree: an implicit heap over P leaves, a function of the N totals alone (kept until the trees change: set_tree, update)
    def top(self):
        if self._top is None:
            P = 1
            while P < self.N:
                P *= 2
            heap = np.zeros(2 * P - 1, dtype=f32)
            heap[P - 1:P - 1 + self.N] = self.tree[:, 0]
            width = P // 2
            while width >= 1:                                    # one level at a time: node = f32(left + right)
                lo = width - 1
                heap[lo:lo + width] = heap[2 * lo + 1:4 * lo + 3:2] + heap[2 * lo + 2:4 * lo + 3:2]
                width //= 2
            assert heap.dtype == f32
            self._top = (heap, P)
        return self._top

    def set_tree(self, tree):
        self.tree, self._top = np.array(tree, dtype=f32), None

    def total(self):
        return self.top()[0][0]

    @staticmethod
    def _descend(heap, v):
        i = 0
        while 2 * i + 1 < len(heap):
            left = heap[2 * i + 1]
            if v <= left:
                i = 2 * i + 1
            else:
                v = f32(v - left)
                i = 2 * i + 2
        return i, v

    def find(self, v):
        """One walk: top tree, then env e's tree with the residual -> (env, prob, data_idx, tree_idx, residual); env >= N: padding."""
        heap, P = self.top()
        i, v = self._descend(heap, f32(v))
        e = i - (P - 1)
        if e >= self.N:
            return e, f32(0), None, None, v
        t, _ = self._descend(self.tree[e], v)
        return e, self.tree[e, t], t - (self.cap - 1), t, v

    def valid(self, e, prob, d):
        if e >= self.N:
            return False
        w = int(self.index[e])
        return (w - d) % self.cap > self.n and (d - w) % self.cap >= 1 and prob != 0          # memory.py:175

    def filled(self):
        return f32(int(sum(self.cap if self.full[e] else int(self.index[e]) for e in range(self.N))))

    def transition(self, e, d):
        alive, ret, pos = True, f32(0), d % self.cap
        for t in range(self.n):
            r = self.rewards[e, pos] if alive else f32(0)
            ret = f32(ret + f32(r * self.scaling[t]))
            alive = alive and bool(self.nonterminals[e, pos])
            pos = (pos + 1) % self.cap
        nxt = self.states[e, pos] if alive else np.zeros_like(self.states[e, pos])
        return self.states[e, d % self.cap], self.actions[e, d % self.cap], ret, nxt, f32(alive and bool(self.nonterminals[e, pos]))

    def sample_at(self, values):
        """-> (idx [B, 2], states, actions, returns, next_states, nonterminals [B, 1], weights), prob [B], data_idx [B]."""
        found = [self.find(v)[:4] for v in values]
        assert all(self.valid(e, p, d) for e, p, d, _ in found)
        return self.batch_for(found)

    def batch_for(self, found):
        """The batch of the leaves found, each (env, prob, data_idx, tree_idx): what sample_at returns."""
        T = self.total()
        rows = [self.transition(e, d) for e, _, d, _ in found]
        prob = np.array([p for _, p, _, _ in found], dtype=f32)
        w = (self.filled() * (prob / T)) ** f32(-self.beta)                  # memory.py:199-201 on the pooled memory
        w = (w / w.max()).astype(f32)
        idx = np.array([[e, t] for e, _, _, t in found], dtype=np.int64)
        cols = list(zip(*rows))
        batch = (idx, np.stack(cols[0]), np.array(cols[1], dtype=np.int64), np.array(cols[2], dtype=f32), np.stack(cols[3]),
                 np.array(cols[4], dtype=f32)[:, None], w)
        return batch, prob, np.array([d for _, _, d, _ in found], dtype=np.int64)

    def update(self, triples):
        """(env, tree_idx, priority) in list order, each one SegmentTree.update (memory.py:47-58)."""
        self._top = None
        for e, t, p in triples:
            if not (0 <= e < self.N) or not (self.cap - 1 <= t <= 2 * self.cap - 2):
                continue
            p = f32(p)
            self.tree[e, t] = p
            while t != 0:
                t = (t - 1) // 2
                self.tree[e, t] = f32(self.tree[e, 2 * t + 1] + self.tree[e, 2 * t + 2])
            self.max[e] = max(p, self.max[e])

    # -- where the leaves lie in [0, T): for choosing values and for judging drawn ones (float64 sums of the float32 nodes)
    def leaf_offsets(self):
        """[N, cap] float64: the mass that a walk passes on its left on the way to leaf (e, d)."""
        heap, P = self.top()

        def left_mass(tree, i):
            off = 0.0
            while i > 0:
                p = (i - 1) // 2
                if i == 2 * p + 2:
                    off += float(tree[2 * p + 1])
                i = p
            return off
        out = np.zeros((self.N, self.cap))
        for e in range(self.N):
            base = left_mass(heap, P - 1 + e)
            for d in range(self.cap):
                out[e, d] = base + left_mass(self.tree[e], d + self.cap - 1)
        return out

    def valid_leaves(self):
        return [(e, d) for e in range(self.N) for d in range(self.cap) if self.valid(e, self.tree[e, d + self.cap - 1], d)]


def make_model(n_env, cap, obs_len, rng, n_step=3, beta=0.4, invalid_prio=None, empty_envs=True, rare=False):
    """A pooled memory with full rings (write index mid-ring), part-filled rings and (N >= 8) empty ones; priorities with zeros
    among them.  invalid_prio: the priority of the leaves that memory.py:175 refuses (None: like any other leaf, except the
    newest n_step of a part-filled ring, which get 0.01 as in tests/test_gpu_replay_shapes.py).  rare: one valid leaf, m.rare =
    (env, d), gets the one smallest priority, so the sample that reads it owns the batch maximum of the weights."""
    kind = rng.randint(0, 3, size=n_env)                       # 0 full, 1 part-filled, 2 full again
    if empty_envs and n_env >= 8:
        kind[rng.choice(n_env, size=max(1, n_env // 16), replace=False)] = 3
    if cap < n_step + 4:
        kind[kind == 1] = 0                                      # too small a ring to hold a sampleable part
    index = np.zeros(n_env, dtype=np.int64)
    full = np.zeros(n_env, dtype=bool)
    leaves = rng.uniform(0.5, 2.0, size=(n_env, cap)).astype(f32)
    leaves[rng.rand(n_env, cap) < 0.1] = 0.0
    states = rng.uniform(0, 0.3, size=(n_env, cap, obs_len)).astype(f32)
    actions = rng.randint(0, 500, size=(n_env, cap)).astype(np.int64)
    rewards = rng.uniform(0, 1, size=(n_env, cap)).astype(f32)
    nonterm = rng.rand(n_env, cap) >= 0.15
    for e in range(n_env):
        if kind[e] == 3:
            filled = 0
        elif kind[e] == 1:
            filled = int(rng.randint(n_step + 2, cap))
        else:
            filled, full[e] = cap, True
        index[e] = filled if not full[e] else rng.randint(0, cap)
        if not full[e]:
            states[e, filled:], actions[e, filled:], rewards[e, filled:], nonterm[e, filled:], leaves[e, filled:] = 0, 0, 0, False, 0
            leaves[e, max(filled - n_step, 0):filled] = 0.01 if filled else 0.0
    m = PoolModel(rebuild(leaves), index, full, states, actions, rewards, nonterm, n_step, beta)
    if invalid_prio is not None:
        for e in range(n_env):
            for d in range(cap):
                if leaves[e, d] != 0 and not m.valid(e, leaves[e, d], d):
                    leaves[e, d] = invalid_prio
        m.set_tree(rebuild(leaves))
    if rare:
        pool = m.valid_leaves()
        m.rare = pool[rng.randint(len(pool))]
        leaves[m.rare] = 0.002
        m.set_tree(rebuild(leaves))
    m.max[:] = rng.uniform(0.5, 3.0, size=n_env).astype(f32)
    return m


def load_memory(m, device="cpu", use_hip=None):
    """The model's arrays in a VectorReplayMemory."""
    mem = VectorReplayMemory(m.N, m.cap, m.states.shape[2], multi_step=m.n, priority_weight=m.beta, device=device, use_hip=use_hip)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)                # noqa: E731
    for name, a in (("sum_tree", m.tree), ("index", m.index), ("full", m.full), ("max", m.max), ("states", m.states),
                    ("actions", m.actions), ("rewards", m.rewards), ("nonterminals", m.nonterminals)):
        getattr(mem, name).copy_(put(a))
    return mem


def values_for(m, b, rng, offsets=None, place=None, avoid=()):
    """b positions in [0, T), each the middle of a leaf the model finds valid: valid leaves at random (again and again if there
    are fewer than b; never one of `avoid`), position k the leaf place[k]."""
    offsets = m.leaf_offsets() if offsets is None else offsets
    pool = [x for x in m.valid_leaves() if x not in avoid]
    assert pool
    picks = [pool[i] for i in rng.randint(0, len(pool), size=b)]
    for k, leaf in (place or {}).items():
        picks[k] = leaf
    vals = np.array([offsets[e, d] + 0.5 * float(m.tree[e, d + m.cap - 1]) for e, d in picks[:b]]).astype(f32)
    for v, (e, d) in zip(vals, picks):
        got = m.find(v)
        assert (got[0], got[2]) == (e, d), "fixture: a leaf's middle does not lead to the leaf"
    return vals


def assert_batch(got, want, prob=None, data_idx=None):
    """got: the seven tensors of sample_pooled (anything with .cpu()); want: PoolModel.sample_at's batch."""
    got = [t.cpu().numpy() for t in got]
    for k in (0, 1, 2, 4, 5):                                    # idx, states, actions, next states, flags: bit for bit
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"field {k}")
    np.testing.assert_allclose(got[3], want[3], rtol=0, atol=ATOL)
    np.testing.assert_allclose(got[6], want[6], rtol=0, atol=ATOL)
    assert got[3].dtype == f32 and got[6].dtype == f32 and got[6].shape == want[6].shape


def random_triples(m, b, rng, junk=True):
    """b triples over the leaves of the model with duplicates (b >= 2: triple b-1 repeats triple 0's leaf), and -- junk -- in
    their midst triples that are to be ignored, with priorities that would show: an internal node, an index past the row,
    env = N, env = -1."""
    env = rng.randint(0, m.N, size=b).astype(np.int64)
    ti = rng.randint(0, m.cap, size=b).astype(np.int64) + m.cap - 1
    pr = rng.uniform(0.05, 3.0, size=b).astype(f32)
    if b >= 2:
        env[b - 1], ti[b - 1] = env[0], ti[0]
    if junk and b >= 8:
        for k, (e, t) in zip(rng.choice(np.arange(1, b - 1), size=4, replace=False),
                             ((env[1], m.cap - 2), (env[2], 2 * m.cap - 1), (m.N, ti[1]), (-1, ti[2]))):
            env[k], ti[k], pr[k] = e, t, 99.0
    return env, ti, pr


def test_library_exports_the_pooled_entry_points():
    from irbpp_amd import _lib, build
    build.build()
    lib = _lib.load()
    for name in ("irbpp_replay_pool_sample", "irbpp_replay_pool_gather", "irbpp_replay_pool_update"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


# ------------------------------------------------------------------ the torch formulation against the model ------------------
@pytest.mark.parametrize("cap", [8, 11, 64])
@pytest.mark.parametrize("n_env", [1, 3, 8, 130])
def test_sample_pooled_supplied_values_and_updates(n_env, cap):
    """Capacities 8, 11 (leaves at two depths) and 64; N = 1, 3 (P = 4: one padding leaf), 8, 130; B = 1, 5, 64 (below and
    above N); part-filled and full rings: every field of the batch, then the trees and maxima after an update with a
    duplicate leaf, a triple that is no leaf and one with env = N, then a sample from the updated memory."""
    rng = np.random.RandomState(1000 * n_env + cap)
    m = make_model(n_env, cap, 5, rng)
    mem = load_memory(m)
    for b in (1, 5, 64):
        offsets = m.leaf_offsets()
        values = values_for(m, b, rng, offsets)
        want, prob, data_idx = m.sample_at(values)
        got = mem.sample_pooled(b, values=torch.from_numpy(values))
        assert_batch(got, want)
        env, _, d, t, padding = mem._find_pooled(mem._top_tree(), torch.from_numpy(values))
        np.testing.assert_array_equal(mem.sum_tree[env, t].numpy(), prob)
        np.testing.assert_array_equal(d.numpy(), data_idx)
        assert not bool(padding.any())
        assert got[5].shape == (b, 1) and got[0].shape == (b, 2) and got[1].shape == (b, 5)
        env, ti, pr = random_triples(m, b, rng)
        m.update(zip(env, ti, pr))
        mem.update_priorities_pooled(torch.from_numpy(np.stack([env, ti], axis=1)), torch.from_numpy(pr), powered=True)
        np.testing.assert_array_equal(mem.sum_tree.numpy(), m.tree)
        np.testing.assert_array_equal(mem.max.numpy(), m.max)
    np.testing.assert_array_equal(mem.sum_tree.numpy(), rebuild(m.tree[:, cap - 1:]))       # every ancestor is left + right


def test_update_takes_the_power_unless_told_otherwise():
    rng = np.random.RandomState(5)
    m = make_model(3, 11, 2, rng)
    mem = load_memory(m)
    idx = torch.tensor([[0, 10], [2, 20], [0, 10]])
    loss = torch.tensor([4.0, 9.0, 16.0])
    mem.update_priorities_pooled(idx, loss)
    m.update([(0, 10, 2.0), (2, 20, 3.0), (0, 10, 4.0)])
    np.testing.assert_array_equal(mem.sum_tree.numpy(), m.tree)
    np.testing.assert_array_equal(mem.max.numpy(), m.max)


# ------------------------------------------------------------------ the model against what exists ---------------------------
@pytest.mark.parametrize("cap,b", [(8, 1), (11, 5), (64, 64)])
def test_one_memory_pooled_is_sample(cap, b):
    """N = 1: sample_pooled(B, values) is sample(B, values) field for field (the return is a matmul there and a running sum
    here: 1e-6), and the model agrees with both."""
    rng = np.random.RandomState(cap)
    m = make_model(1, cap, 4, rng)
    mem = load_memory(m)
    values = values_for(m, b, rng)
    pooled = mem.sample_pooled(b, values=torch.from_numpy(values))
    per_env = mem.sample(b, values=torch.from_numpy(values)[None, :])
    assert torch.equal(pooled[0][:, 1], per_env[0][0]) and not bool(pooled[0][:, 0].any())
    for k in (1, 2, 4, 5, 6):
        assert torch.equal(pooled[k], per_env[k]), k
    assert torch.allclose(pooled[3], per_env[3], rtol=0, atol=ATOL)
    assert_batch(pooled, m.sample_at(values)[0])


@pytest.mark.parametrize("n_env,cap", [(3, 11), (8, 8), (130, 64)])
def test_pooled_walk_carries_on_in_the_envs_own_tree(n_env, cap):
    """N > 1: a value in env e's share of [0, T) ends at the leaf that SegmentTree.find of env e returns for the residual."""
    rng = np.random.RandomState(n_env + cap)
    m = make_model(n_env, cap, 1, rng)
    T = m.total()
    seen = set()
    for v in rng.uniform(0, T, size=300).astype(f32):
        e, prob, d, t, residual = m.find(v)
        if e >= m.N:
            continue
        tree = SumTree(cap, 1)
        tree.sum_tree = m.tree[e]
        assert tree.find(residual) == (prob, d, t)
        seen.add(e)
    assert len(seen) > 1
    torch_env = load_memory(m)._find_pooled(load_memory(m)._top_tree(), torch.tensor([f32(T * 0.5)]))[0]
    assert int(torch_env) == m.find(f32(T * 0.5))[0]


@pytest.mark.parametrize("n_env,cap,per_env", [(3, 11, 4), (8, 64, 5), (130, 8, 2)])
def test_update_grouped_by_env_is_update_priorities(n_env, cap, per_env):
    rng = np.random.RandomState(n_env * cap)
    m = make_model(n_env, cap, 1, rng)
    a, b = load_memory(m), load_memory(m)
    ti = rng.randint(0, cap, size=(n_env, per_env)).astype(np.int64) + cap - 1
    ti[:, -1] = ti[:, 0]                                                     # a duplicate in every env
    pr = rng.uniform(0.05, 3.0, size=(n_env, per_env)).astype(f32)
    a.update_priorities(torch.from_numpy(ti), torch.from_numpy(pr), powered=True)
    env = np.repeat(np.arange(n_env), per_env)
    b.update_priorities_pooled(torch.from_numpy(np.stack([env, ti.reshape(-1)], axis=1)), torch.from_numpy(pr.reshape(-1)), powered=True)
    assert torch.equal(a.sum_tree, b.sum_tree) and torch.equal(a.max, b.max)
    m.update(zip(env, ti.reshape(-1), pr.reshape(-1)))
    np.testing.assert_array_equal(b.sum_tree.numpy(), m.tree)
    np.testing.assert_array_equal(b.max.numpy(), m.max)


# ------------------------------------------------------------------ drawn samples and the two errors ------------------------
@pytest.mark.parametrize("n_env,cap,b", [(3, 11, 5), (130, 64, 64), (8, 64, 1)])
def test_drawn_samples_are_valid_and_repeatable(n_env, cap, b):
    rng = np.random.RandomState(b)
    m = make_model(n_env, cap, 3, rng, invalid_prio=1e-3)
    mem = load_memory(m)
    one = mem.sample_pooled(b, generator=torch.Generator().manual_seed(3))
    two = mem.sample_pooled(b, generator=torch.Generator().manual_seed(3))
    for x, y in zip(one, two):
        assert torch.equal(x, y)
    idx = one[0].numpy()
    for e, t in idx:
        assert m.valid(e, m.tree[e, t], t - (cap - 1))
    assert float(one[6].max()) == 1.0


def test_too_few_transitions_raise_runtime_error():
    """Every env holds n transitions: nothing has its n successors, so no draw is valid."""
    n_env, n_step = 3, 3
    mem = VectorReplayMemory(n_env, 16, 2, multi_step=n_step)
    for _ in range(n_step):
        mem.append(torch.rand(n_env, 2), torch.zeros(n_env, dtype=torch.int64), torch.ones(n_env), torch.zeros(n_env, dtype=torch.bool))
    with pytest.raises(RuntimeError):
        mem.sample_pooled(2, generator=torch.Generator().manual_seed(1), max_tries=8)


def test_invalid_supplied_value_raises_value_error():
    rng = np.random.RandomState(2)
    m = make_model(3, 11, 2, rng)
    mem = load_memory(m)
    good = values_for(m, 3, rng)
    mem.sample_pooled(3, values=torch.from_numpy(good))
    # a leaf with mass that memory.py:175 refuses: at or just behind some env's write index
    e, d = next((e, d) for e in range(m.N) for d in range(m.cap)
                if m.tree[e, d + m.cap - 1] != 0 and not m.valid(e, m.tree[e, d + m.cap - 1], d))
    bad = good.copy()
    bad[1] = f32(m.leaf_offsets()[e, d] + 0.5 * float(m.tree[e, d + m.cap - 1]))
    assert not m.valid(*m.find(bad[1])[:3])
    with pytest.raises(ValueError):
        mem.sample_pooled(3, values=torch.from_numpy(bad))
    beyond = good.copy()
    beyond[2] = np.nextafter(m.total(), f32(np.inf)) * f32(1.5)              # past T: the padding leaf of P = 4
    assert m.find(beyond[2])[0] >= m.N
    with pytest.raises(ValueError):
        mem.sample_pooled(3, values=torch.from_numpy(beyond))
