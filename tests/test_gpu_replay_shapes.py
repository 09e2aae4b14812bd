"""csrc/irbpp_replay.hip at the sizes where its loops take a second trip, against plain references.

The other replay tests run the kernels at capacities up to 64, four samples and five-float observations: one trip of every
strided loop, one wave of samples, full rings.  Here: tree levels wider than a wave up to the largest capacity the library
accepts (8192), more than one workgroup of draws, samples in all four waves, observation rows around and beyond 256 floats,
rings that are not full, strided arguments.  References: oracle/replay.py per env (pinned to the reference's memory.py by
tests/golden/replay_*.npz) and a numpy float32 bottom-up rebuild (node = f32(left + right)) for whole trees.  Indices, trees,
maxima, states, actions, next states and flags bit-equal; n-step returns and importance weights within the 1e-6 that
tests/test_replay.py states for them."""
import ctypes as C

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd.replay import VectorReplayMemory, mask_from_state
from oracle.replay import ReplayMemory as OracleReplay, SumTree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def _lib():
    from irbpp_amd import _lib as L
    return L, L.load()


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rebuild(leaves):
    """[N, cap] float32 leaves -> [N, 2*cap - 1] tree, every internal node f32(left + right), bottom-up."""
    leaves = np.asarray(leaves, dtype=f32)
    n, cap = leaves.shape
    tree = np.zeros((n, 2 * cap - 1), dtype=f32)
    tree[:, cap - 1:] = leaves
    for i in range(cap - 2, -1, -1):
        tree[:, i] = tree[:, 2 * i + 1] + tree[:, 2 * i + 2]
    assert tree.dtype == f32
    return tree


def _oracle_tree(row, cap):
    t = SumTree(cap, 1)
    t.sum_tree = np.asarray(row, dtype=f32)
    return t


def _update(mem, tree_idx, prio, mask):
    """irbpp_sumtree_update through the C ABI: tree_idx int64 [N, B], prio float32 [N, B], env mask uint8 [N] or None."""
    L, lib = _lib()
    n, b = tree_idx.shape
    ti, pr = _dev(tree_idx.astype(np.int64)), _dev(prio.astype(f32))
    mk = None if mask is None else _dev(mask.astype(np.uint8))
    L.check(lib.irbpp_sumtree_update(_ptr(mem.sum_tree), _ptr(mem.max), n, mem.capacity, _ptr(ti), _ptr(pr), b, _ptr(mk), _stream()),
            "irbpp_sumtree_update")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ irbpp_sumtree_update -------------------------------------
@pytest.mark.parametrize("cap", [2, 3, 65, 100, 128, 129, 1000, 4096, 8191, 8192])
def test_sumtree_update_rebuilds_every_level(cap):
    """All leaves in one call (B = capacity: every level of the tree is rebuilt, the widest 4096 nodes for 64 lanes), then 8
    leaves per env with the first leaf, the last leaf and duplicates; then the same with indices that are not leaves of the
    row, which must change nothing.  Envs the mask skips keep their rows and maxima."""
    rng = np.random.RandomState(cap)
    n = 5
    mask = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    on = mask.astype(bool)
    mem = VectorReplayMemory(n, cap, 1, device=DEV, use_hip=True)
    junk = rng.uniform(1, 2, size=(n, 2 * cap - 1)).astype(f32)          # what the rows hold before: no sum of anything
    max0 = np.array([0.5, 7.0, 3.0, 0.25, 9.0], dtype=f32)
    mem.sum_tree.copy_(_dev(junk))
    mem.max.copy_(_dev(max0))
    leaves = rng.uniform(0.05, 2.0, size=(n, cap)).astype(f32)
    leaves[rng.rand(n, cap) < 0.2] = 0.0
    order = np.stack([rng.permutation(cap) for _ in range(n)])
    _update(mem, order + cap - 1, np.take_along_axis(leaves, order, axis=1), mask)
    want = rebuild(leaves)
    want[~on] = junk[~on]
    wmax = np.where(on, np.maximum(max0, leaves.max(1)), max0).astype(f32)
    np.testing.assert_array_equal(mem.sum_tree.cpu().numpy(), want)
    np.testing.assert_array_equal(mem.max.cpu().numpy(), wmax)

    # 8 leaves per env: first leaf, last leaf, x, y, x again, z, last again, x a third time -- the last value listed wins
    x, y, z = (rng.randint(0, cap, size=n) for _ in range(3))
    d = np.stack([np.zeros(n, dtype=np.int64), np.full(n, cap - 1), x, y, x, z, np.full(n, cap - 1), x], axis=1)
    pr = rng.uniform(0.05, 3.0, size=(n, 8)).astype(f32)
    _update(mem, d + cap - 1, pr, mask)
    for e in range(n):
        if on[e]:
            for j in range(8):
                leaves[e, d[e, j]] = pr[e, j]
    want2 = rebuild(leaves)
    want2[~on] = junk[~on]
    wmax2 = np.where(on, np.maximum(wmax, pr.max(1)), max0).astype(f32)
    np.testing.assert_array_equal(mem.sum_tree.cpu().numpy(), want2)
    np.testing.assert_array_equal(mem.max.cpu().numpy(), wmax2)

    # indices that are no leaf of the row (internal nodes, past the row, negative, beyond 2^32) with priorities that would
    # show in the tree and in the maximum: ignored; the tree equals the one built from the four real leaves alone.  (The index
    # beyond 2^32 is leaf 0 of the row once cut to 32 bits: a kernel that compared it as an int would take it for a leaf.)
    twin = VectorReplayMemory(n, cap, 1, device=DEV, use_hip=True)
    twin.sum_tree.copy_(mem.sum_tree)
    twin.max.copy_(mem.max)
    real = np.stack([x, np.full(n, cap - 1), np.zeros(n, dtype=np.int64), y], axis=1) + cap - 1
    rp = rng.uniform(0.05, 3.0, size=(n, 4)).astype(f32)
    bad = np.array([cap - 2, 2 * cap - 1, -1, (1 << 32) + cap - 1], dtype=np.int64)          # (cap - 2: the last internal node)
    mixed = np.stack([real[:, 0], np.full(n, bad[0]), real[:, 1], np.full(n, bad[1]), np.full(n, bad[2]), real[:, 2],
                      np.full(n, bad[3]), real[:, 3]], axis=1)
    mp = np.full((n, 8), 99.0, dtype=f32)
    mp[:, [0, 2, 5, 7]] = rp
    _update(mem, mixed, mp, mask)
    _update(twin, real, rp, mask)
    for e in range(n):
        if on[e]:
            for j in range(4):
                leaves[e, real[e, j] - (cap - 1)] = rp[e, j]
    want3 = rebuild(leaves)
    want3[~on] = junk[~on]
    wmax3 = np.where(on, np.maximum(wmax2, rp.max(1)), max0).astype(f32)
    np.testing.assert_array_equal(mem.sum_tree.cpu().numpy(), want3)
    np.testing.assert_array_equal(twin.sum_tree.cpu().numpy(), want3)
    np.testing.assert_array_equal(mem.max.cpu().numpy(), wmax3)
    np.testing.assert_array_equal(twin.max.cpu().numpy(), wmax3)


def test_capacity_beyond_the_lds_row_still_raises():
    with pytest.raises(RuntimeError):
        VectorReplayMemory(1, 8193, 1, device=DEV, use_hip=True)
    L, lib = _lib()
    tree, mx = torch.zeros(2 * 8193 - 1, device=DEV), torch.ones(1, device=DEV)
    ti, pr = torch.full((1,), 8192, dtype=torch.int64, device=DEV), torch.ones(1, device=DEV)
    assert lib.irbpp_sumtree_update(_ptr(tree), _ptr(mx), 1, 8193, _ptr(ti), _ptr(pr), 1, _ptr(None), _stream()) == -1     # IRBPP_ERR_ARG
    torch.cuda.synchronize()
    assert not bool(tree.any())


# ------------------------------------------------------------------ irbpp_sumtree_find ---------------------------------------
def _boundary(tree, idx):
    """The value whose descent reaches internal node idx with exactly tree[left child] left over: the `v <= left` edge."""
    off, i = 0.0, idx
    while i > 0:
        p = (i - 1) // 2
        if i == 2 * p + 2:
            off += float(tree[2 * p + 1])
        i = p
    return f32(off + float(tree[2 * idx + 1]))


def _middle_of_leaf(tree, idx):
    """A value whose descent ends at leaf idx: the mass to the left of the leaf on its path plus half its own.  (Leaves of a
    capacity that is no power of two sit at two depths: the descent does not meet them in index order.)"""
    off, i = 0.5 * float(tree[idx]), idx
    while i > 0:
        p = (i - 1) // 2
        if i == 2 * p + 2:
            off += float(tree[2 * p + 1])
        i = p
    return f32(off)


@pytest.mark.parametrize("n,b,cap,trailing_zeros", [(1, 256, 13, False), (1, 257, 1000, False), (3, 100, 8191, False),
                                                    (1, 257, 13, True), (3, 100, 1000, True)])
def test_sumtree_find_at_the_comparison_edges(n, b, cap, trailing_zeros):
    """One, just over one and two workgroups of draws per launch; trees with zero-priority leaves interspersed and half-filled
    trees whose trailing leaves are all zero.  Values: 0, the total and the float above it, the float32 prefix sums of the
    leaves, and the exact `v <= left` edge of internal nodes with its two float32 neighbours.  Up to capacity 1000 EVERY
    prefix sum and every internal node's edge is queried, over as many launches of n * b values as that takes; at 8191 a
    sample of them (24 launches).  Every result equals SegmentTree.find on the same float32 tree."""
    rng = np.random.RandomState(cap + b)
    leaves = rng.uniform(0.05, 2.0, size=(n, cap)).astype(f32)
    leaves[rng.rand(n, cap) < 0.25] = 0.0
    if trailing_zeros:
        leaves[:, cap // 2:] = 0.0
    tree = rebuild(leaves)
    pools = []
    for e in range(n):
        total = tree[e, 0]
        pre = np.cumsum(leaves[e], dtype=f32)
        nodes = np.arange(cap - 1) if cap <= 1000 else rng.permutation(cap - 1)[:600]
        edges = np.array([_boundary(tree[e], i) for i in nodes], dtype=f32)
        rest = np.concatenate([pre, np.nextafter(pre, f32(np.inf)), edges, np.nextafter(edges, f32(-np.inf)),
                               np.nextafter(edges, f32(np.inf))]).astype(f32)
        pools.append(np.concatenate([[f32(0), total, np.nextafter(total, f32(np.inf))], rest[rng.permutation(len(rest))]]).astype(f32))
    launches = -(-len(pools[0]) // b)
    if cap > 1000:
        launches = min(launches, 24)
    else:
        assert launches * b >= len(pools[0])                                   # nothing of the pool is left out
    mem = VectorReplayMemory(n, cap, 1, device=DEV, use_hip=True)
    mem.sum_tree.copy_(_dev(tree))
    oracles = [_oracle_tree(tree[e], cap) for e in range(n)]
    reached = [set() for _ in range(n)]
    for k in range(launches):
        values = np.zeros((n, b), dtype=f32)
        for e in range(n):
            part = pools[e][k * b:(k + 1) * b]
            values[e, :len(part)] = part
            values[e, len(part):] = rng.uniform(0, tree[e, 0], size=b - len(part)).astype(f32)
        prob, data_idx, tree_idx = (t.cpu().numpy() for t in mem.find(_dev(values)))
        assert prob.shape == (n, b) and prob.dtype == f32 and data_idx.dtype == np.int64 and tree_idx.dtype == np.int64
        for e in range(n):
            ref = [oracles[e].find(v) for v in values[e]]
            np.testing.assert_array_equal(tree_idx[e], [r[2] for r in ref])
            np.testing.assert_array_equal(data_idx[e], [r[1] for r in ref])
            np.testing.assert_array_equal(prob[e], np.array([r[0] for r in ref], dtype=f32))
            reached[e].update(r[2] for r in ref)
    for e in range(n):
        assert len(reached[e]) > (min(cap, 600) if cap > 1000 else cap) // 8                     # the values spread over the tree


# ------------------------------------------------------------------ fixtures for sample / gather -----------------------------
def _filled_memory(n, cap, obs_len, n_step, filled, rng, beta=0.4, min_leaf=None, keep=None):
    """A VectorReplayMemory and its per-env oracles holding the same `filled` transitions (filled == cap: a full ring whose
    write index sits mid-ring), written into the tensors directly: states, actions, rewards, terminal flags, priorities with
    zeros among them (not at the positions keep[e]).  min_leaf[e] gets the one smallest priority of env e (the largest
    importance weight)."""
    mem = VectorReplayMemory(n, cap, obs_len, multi_step=n_step, priority_weight=beta, device=DEV, use_hip=True)
    full = filled == cap
    index = cap // 2 if full else filled
    states = rng.uniform(0, 0.3, size=(n, cap, obs_len)).astype(f32)
    actions = rng.randint(0, 500, size=(n, cap)).astype(np.int64)
    rewards = rng.uniform(0, 1, size=(n, cap)).astype(f32)
    nonterm = rng.rand(n, cap) >= 0.15
    leaves = rng.uniform(0.5, 2.0, size=(n, cap)).astype(f32)
    leaves[rng.rand(n, cap) < 0.1] = 0.0
    if not full:
        states[:, filled:], actions[:, filled:], rewards[:, filled:], nonterm[:, filled:], leaves[:, filled:] = 0, 0, 0, False, 0
        leaves[:, filled - n_step:filled] = 0.01           # the newest transitions cannot be sampled yet (memory.py:175): with a
        #                                                    small priority no segment of the mass lies wholly inside them
    for e in range(n if keep is not None else 0):
        leaves[e, keep[e][leaves[e, keep[e]] == 0.0]] = 1.0
    if min_leaf is not None:
        leaves[np.arange(n), min_leaf] = 0.01
    tree = rebuild(leaves)
    mem.states.copy_(_dev(states))
    mem.actions.copy_(_dev(actions))
    mem.rewards.copy_(_dev(rewards))
    mem.nonterminals.copy_(_dev(nonterm))
    mem.sum_tree.copy_(_dev(tree))
    mem.index.fill_(index)
    mem.full.fill_(full)
    oracles = []
    for e in range(n):
        o = OracleReplay(cap, obs_len, 0.99, n_step, beta, 0.5)
        tr = o.transitions
        tr.states, tr.actions, tr.rewards, tr.nonterminals = states[e], actions[e], rewards[e], nonterm[e]
        tr.sum_tree, tr.index, tr.full = tree[e], index, full
        oracles.append(o)
    return mem, oracles, leaves


# ------------------------------------------------------------------ irbpp_sumtree_sample -------------------------------------
@pytest.mark.parametrize("b", [64, 256])
def test_sumtree_sample_on_a_ring_that_is_not_full(b):
    """Capacity 1000 filled to 40 %: every draw of the fused sampler satisfies the reference's validity test (memory.py:175)
    on a tree whose trailing 600 leaves are zero, lies in the filled part, and the same seed gives the same draws."""
    n, cap, n_step = 3, 1000, 3
    mem, oracles, leaves = _filled_memory(n, cap, 2, n_step, 400, np.random.RandomState(b))
    g1, g2, g3 = (torch.Generator().manual_seed(s) for s in (5, 5, 6))
    a, a2, c = mem.sample(b, generator=g1), mem.sample(b, generator=g2), mem.sample(b, generator=g3)
    assert torch.equal(a[0], a2[0]) and not torch.equal(a[0], c[0])
    for k in range(1, 7):
        assert torch.equal(a[k], a2[k])
    tree_idx = a[0].cpu().numpy()
    assert tree_idx.shape == (n, b)
    for e, o in enumerate(oracles):
        d = tree_idx[e] - (cap - 1)
        assert (d >= 0).all() and (d < 400 - n_step).all()
        assert all(o.valid(leaves[e, j], int(j)) for j in d)
        # and the batch the gather kernel assembled for these draws is the oracle's for the same positions
        rows = [o.transition(int(j)) for j in d]
        sl = slice(e * b, (e + 1) * b)
        np.testing.assert_array_equal(a[1].cpu().numpy()[sl], np.stack([r[0] for r in rows]))
        np.testing.assert_array_equal(a[2].cpu().numpy()[sl], np.array([r[1] for r in rows]))
        np.testing.assert_allclose(a[3].cpu().numpy()[sl], np.array([r[2] for r in rows]), rtol=0, atol=1e-6)
        np.testing.assert_array_equal(a[4].cpu().numpy()[sl], np.stack([r[3] for r in rows]))
        np.testing.assert_array_equal(a[5].cpu().numpy()[sl, 0], np.array([r[4] for r in rows]))


def test_sample_reports_failure_on_too_few_transitions():
    """n_step + 1 transitions: only position 0 has its n successors, so the second of two segments finds nothing valid within
    max_tries and the call raises instead of looping (the reference's rejection loop would not return)."""
    n, cap, n_step = 3, 100, 3
    mem = VectorReplayMemory(n, cap, 2, multi_step=n_step, device=DEV, use_hip=True)
    for t in range(n_step + 1):
        mem.append(torch.rand(n, 2, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV), torch.ones(n, device=DEV),
                   torch.zeros(n, dtype=torch.bool, device=DEV))
    assert int(mem.index[0]) == n_step + 1 < n_step + 2
    with pytest.raises(RuntimeError):
        mem.sample(2, generator=torch.Generator().manual_seed(1))


# ------------------------------------------------------------------ irbpp_replay_gather --------------------------------------
@pytest.mark.parametrize("b,obs_len,beta,full,max_at", [
    (1, 1, 0.4, True, 0), (63, 255, 0.0, True, 62), (64, 256, 1.0, False, 63), (65, 257, 0.4, True, 64),
    (256, 5, 0.4, True, 0), (256, 5, 0.4, False, 200), (256, 1000, 1.0, True, 255), (257, 5, 0.4, True, 256)])
def test_replay_gather_against_the_oracle(b, obs_len, beta, full, max_at):
    """Samples in one to four waves, the largest weight (the smallest priority) owned by sample `max_at` -- wave 0, wave 3, the
    last thread --, observation rows below, at and beyond the 256-thread copy loop, positions at the ring's end whose n-step
    chain wraps, terminals inside the chain, full and not-full rings (filled = index), beta 0 / 0.4 / 1.  B = 257 takes the
    torch formulation and agrees as well.  Against oracle sample_at per env."""
    rng = np.random.RandomState(b * 1000 + obs_len)
    n, cap, n_step = 2, 300, 3
    filled = cap if full else 200
    index = cap // 2 if full else filled
    # positions the reference's validity test admits, by its own expression; the ring's end first (full ring: the chain wraps)
    ok = [d for d in range(filled) if (index - d) % cap > n_step and (d - index) % cap >= 1]
    special = [cap - 1, cap - 10, cap - 3] if full else [filled - n_step - 1, 0, 10]
    mid = [d for d in ok if 20 <= d < 140]                                    # (clear of the chains of the special positions)
    rare = rng.choice(mid, size=n, replace=False)
    mid = [d for d in mid if d not in rare]
    pos = np.stack([np.array((special + list(rng.choice(mid, size=b)))[:b]) for _ in range(n)])
    pos[:, max_at] = rare                                                     # only sample max_at reads the smallest leaf
    mem, oracles, leaves = _filled_memory(n, cap, obs_len, n_step, filled, rng, beta=beta, min_leaf=rare, keep=pos)
    # sample 0: a terminal right behind it; sample 1: at its own position; sample 2: at the end of a chain that is alive up
    # to there (d + n; for cap - 3 that is slot 0, where sample 0's terminal sits as well); sample 3: two steps on
    nonterm = mem.nonterminals.cpu().numpy()
    for e in range(n):
        for k, off in enumerate((1, 0, n_step, 2)):
            if k < b:
                nonterm[e, (pos[e, k] + off) % cap] = False
        nonterm[e, pos[e, 0]] = True                                         # (sample 0's own transition is not the terminal one)
        if b >= 3:
            nonterm[e, (pos[e, 2] + np.arange(n_step)) % cap] = True
    mem.nonterminals.copy_(_dev(nonterm))
    for e, o in enumerate(oracles):
        o.transitions.nonterminals = nonterm[e]
    tree = mem.sum_tree.cpu().numpy()
    values = np.stack([[_middle_of_leaf(tree[e], d + cap - 1) for d in pos[e]] for e in range(n)]).astype(f32)
    got = [t.cpu().numpy() for t in mem.sample(b, values=_dev(values))]
    for e, o in enumerate(oracles):
        ti, st, ac, re, ns, nt, w = o.sample_at(values[e])
        assert [t - (cap - 1) for t in ti] == list(pos[e])                   # the fixture samples what it says it does
        sl = slice(e * b, (e + 1) * b)
        np.testing.assert_array_equal(got[0][e], ti)
        np.testing.assert_array_equal(got[1][sl], st)
        np.testing.assert_array_equal(got[2][sl], ac)
        np.testing.assert_allclose(got[3][sl], re, rtol=0, atol=1e-6)
        np.testing.assert_array_equal(got[4][sl], ns)
        np.testing.assert_array_equal(got[5][sl, 0], nt)
        np.testing.assert_allclose(got[6][sl], w, rtol=0, atol=1e-6)
        assert got[6][sl][max_at] == 1.0 and (beta == 0.0 or b == 1 or np.delete(got[6][sl], max_at).max() < 0.5)
        if b >= 4:
            k = 0                                                            # terminal at d + 1: blanked next state, truncated return
            assert not ns[k].any() and nt[k] == 0.0 and not got[4][sl][k].any()
            assert abs(got[3][sl][k] - (o.transitions.rewards[pos[e, k]] + f32(0.99) * o.transitions.rewards[(pos[e, k] + 1) % cap])) < 1e-6
            if max_at != 2:                                                  # terminal at d + n, chain alive: the flag alone --
                assert nt[2] == 0.0 and got[5][sl, 0][2] == 0.0              # the next state is the stored one, not zeros
                assert ns[2].any() and np.array_equal(got[4][sl][2], o.transitions.states[(pos[e, 2] + n_step) % cap])
    assert got[1].shape == (n * b, obs_len) and got[5].shape == (n * b, 1)


# ------------------------------------------------------------------ irbpp_replay_append --------------------------------------
@pytest.mark.parametrize("obs_len,cap", [(255, 3), (256, 100), (257, 3), (257, 100), (255, 100), (256, 3)])
def test_replay_append_strided_rows_through_a_wrap(obs_len, cap):
    """Observation rows below, at and above the 256-thread copy loop, handed over as a column slice of a wider tensor
    (state_stride > obs_len), a valid mask, int32 / int64 actions, float32 / float64 rewards, through one wrap of the ring:
    every tensor of the memory equals the oracle's."""
    rng = np.random.RandomState(obs_len * 7 + cap)
    n, steps, pad = 4, 2 * cap + 8, 37
    mem = VectorReplayMemory(n, cap, obs_len, multi_step=3, device=DEV, use_hip=True)
    oracles = [OracleReplay(cap, obs_len, 0.99, 3) for _ in range(n)]
    for t in range(steps):
        wide = rng.uniform(0, 0.3, size=(n, obs_len + pad)).astype(f32)
        action = rng.randint(0, 500, size=n)
        reward = rng.uniform(0, 1, size=n)
        terminal = rng.rand(n) < 0.2
        valid = rng.rand(n) < 0.7 if t % 3 else np.ones(n, dtype=bool)
        state = _dev(wide)[:, 5:5 + obs_len]
        assert state.stride(0) == obs_len + pad and state.data_ptr() % 16 != 0
        a = _dev(action.astype(np.int32 if t % 2 else np.int64))
        r = _dev(reward.astype(f32)) if t % 4 < 2 else _dev(reward)
        rew = reward.astype(f32) if t % 4 < 2 else reward
        v = None if valid.all() else _dev(valid.astype(np.uint8) if t % 2 else valid)
        # (the wrapper's own device path is called by name: append() would fall back to the torch formulation without a word
        # if it refused these arguments, and the test would compare torch with the oracle)
        assert mem._append_on_device(state, a, r, _dev(terminal), v)
        for e in range(n):
            if valid[e]:
                oracles[e].append(wide[e, 5:5 + obs_len], action[e], rew[e], bool(terminal[e]))
    torch.cuda.synchronize()
    tr = [o.transitions for o in oracles]
    assert all(t.full for t in tr) and len(set(t.index for t in tr)) > 1
    np.testing.assert_array_equal(mem.states.cpu().numpy(), np.stack([t.states for t in tr]))
    np.testing.assert_array_equal(mem.actions.cpu().numpy(), np.stack([t.actions for t in tr]))
    np.testing.assert_array_equal(mem.rewards.cpu().numpy(), np.stack([t.rewards for t in tr]))
    np.testing.assert_array_equal(mem.nonterminals.cpu().numpy(), np.stack([t.nonterminals for t in tr]))
    np.testing.assert_array_equal(mem.timesteps.cpu().numpy(), np.stack([t.timesteps for t in tr]))
    np.testing.assert_array_equal(mem.sum_tree.cpu().numpy(), np.stack([t.sum_tree for t in tr]))
    np.testing.assert_array_equal(mem.max.cpu().numpy(), np.array([t.max for t in tr], dtype=f32))
    np.testing.assert_array_equal(mem.index.cpu().numpy(), [t.index for t in tr])
    np.testing.assert_array_equal(mem.full.cpu().numpy(), [t.full for t in tr])
    np.testing.assert_array_equal(mem.t.cpu().numpy(), [o.t for o in oracles])


# ------------------------------------------------------------------ irbpp_masked_argmax --------------------------------------
def _argmax_rows(n, s, rng):
    """q [n, s] and candidate flags [n, s]: per env one of the patterns that a wave-wide arg-max can get wrong."""
    q = rng.randn(n, s).astype(f32)
    flags = rng.rand(n, s) < 0.5
    want_first = {}
    for e in range(n):
        kind = e % 12
        top = [0, 63, 64, s - 1][kind] if kind < 4 else None
        if top is not None and top < s:                                # the maximum at index 0, 63, 64, S - 1
            q[e, top], flags[e, top] = 50.0, True
            want_first[e] = top
        elif kind == 4 and s >= 2:                                     # a tie between adjacent lanes
            i = min(s - 2, 17)
            q[e, [i, i + 1]], flags[e, [i, i + 1]] = 60.0, True
            want_first[e] = i
        elif kind == 5 and s > 64:                                     # a tie within one lane: i and i + 64
            i = min(s - 65, 30)
            q[e, [i, i + 64]], flags[e, [i, i + 64]] = 60.0, True
            want_first[e] = i
        elif kind == 6:                                                # nothing valid
            flags[e] = False
            want_first[e] = 0
        elif kind == 7:                                                # every valid candidate is -inf
            q[e, flags[e]] = -np.inf
            want_first[e] = 0
        elif kind == 8 and s >= 2:                                     # +inf twice: the first
            i, j = sorted(rng.choice(s, size=2, replace=False))
            q[e, [i, j]], flags[e, [i, j]] = np.inf, True
            want_first[e] = i
        elif kind == 9:                                                # the largest q on a masked candidate
            i = int(rng.randint(s))
            q[e, i], flags[e, i] = 70.0, False
        elif kind == 10 and s > 65:                                    # a tie across the lane loop's trips, later lane first
            q[e, [3, 64]], flags[e, [3, 64]] = 60.0, True
            want_first[e] = 3
    return q, flags, want_first


@pytest.mark.parametrize("s", [1, 63, 64, 65, 500, 1000, 1024])
def test_masked_argmax_shapes_strides_ties_and_infinities(s):
    """Agent.act's two lines (sum_q[(1 - mask).bool()] = -inf; argmax(1)) for S below, at and above a wave and up to the
    1024 candidates of the wide grid, 1 / 3 / 4 / 5 / 257 envs (four envs per workgroup: partial last workgroups), q as a column
    slice of a wider tensor (q_stride > S), maxima at the lanes' ends, ties between adjacent lanes and within one lane,
    everything masked, -inf and +inf on valid candidates.  NaN q is out of scope: the library is built with -fno-honor-nans,
    so a comparison with NaN has no defined outcome in the kernel."""
    L, lib = _lib()
    rng = np.random.RandomState(s)
    for n in (1, 3, 4, 5, 257):
        q, flags, want_first = _argmax_rows(n, s, rng)
        obs = rng.uniform(0, 1, size=(n, 5 * s + 9)).astype(f32)
        obs[:, :5 * s].reshape(n, s, 5)[:, :, 4] = flags
        wide = rng.randn(n, s + 11).astype(f32) + 100.0                    # larger than any q: a read outside the slice wins
        wide[:, 3:3 + s] = q
        sum_q = torch.from_numpy(q).clone()
        mask = torch.from_numpy(obs[:, :5 * s].reshape(n, s, 5)[:, :, 4].copy())                # column 4 of the [S, 5] candidate block
        assert torch.equal(mask, mask_from_state(torch.from_numpy(obs), s))
        sum_q[(1 - mask).bool()] = -float("inf")                                                # the reference's two lines
        want = sum_q.argmax(1).numpy()
        for e, i in want_first.items():
            assert want[e] == i, (e, i)
        wd, od = _dev(wide), _dev(obs)
        out = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
        qs = wd[:, 3:3 + s]
        L.check(lib.irbpp_masked_argmax(_ptr(qs), qs.stride(0), _ptr(od), od.stride(0), s, n, _ptr(out), _stream()),
                "irbpp_masked_argmax")
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:n], want, err_msg=f"S={s} n_env={n}")
        assert got[n] == -7                                                 # the partial last workgroup wrote nothing past n_env


# ------------------------------------------------------------------ the generator's known answers ----------------------------
M64 = (1 << 64) - 1
POOL_RNG_ENV = 0xFFFFFFFF                                                  # uniform01's env field for pooled draws


def uniform01(seed, env, j, attempt):
    """The counter-based generator of csrc/irbpp_replay.hip in Python integers, from its text: splitmix64's finaliser over
    seed + golden * ((env << 32) ^ (j << 8) ^ attempt ^ constant), all modulo 2^64 (env, j and attempt 32-bit fields), the top
    24 bits as a float32 in [0, 1)."""
    counter = ((env << 32) ^ (j << 8) ^ attempt ^ 0xD1B54A32D192ED03) & M64
    z = (seed + 0x9E3779B97F4A7C15 * counter) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    u = f32(z >> 40) * f32(1.0 / 16777216.0)
    assert u.dtype == f32 and 0.0 <= u < 1.0
    return u


KA_CAP, KA_STEP, KA_TRIES = 8192, 3, 16


def _known_answer_tree():
    """A full ring of 8192 leaves, odd leaves of priority 1 and even ones 0: every node an integer, the total 4096.  With one
    draw per env lo = 0 and v = u * 4096 is exact whether the compiler fuses lo + u * segment or not."""
    leaves = np.zeros((1, KA_CAP), dtype=f32)
    leaves[0, 1::2] = 1.0
    tree = rebuild(leaves)[0]
    assert tree[0] == 4096.0 and (tree == np.round(tree)).all()
    return tree


def _known_answer_walk(tree, env_field, seed, w, first=0):
    """-> (leaf, priority, attempts used): attempts first, first + 1, ... until the reference's validity test (memory.py:175)
    holds against the write index w."""
    oracle = _oracle_tree(tree, KA_CAP)
    for attempt in range(first, KA_TRIES):
        v = f32(uniform01(seed, env_field, 0, attempt) * tree[0])
        p, d, t = oracle.find(v)
        if (w - d) % KA_CAP > KA_STEP and (d - w) % KA_CAP >= 1 and p != 0:
            return t, p, attempt + 1
    raise AssertionError("fixture: no valid draw")


@pytest.mark.parametrize("n", [1, 257])
def test_sumtree_sample_draws_the_generators_leaf(n):
    """irbpp_sumtree_sample's leaf is the one the Python-integer generator and the model's walk give, env by env.  Every
    fourth env has its write index on the leaf of its first attempt, so that draw is refused and the answer depends on
    `attempt` entering the counter."""
    L, lib = _lib()
    seed = 0x8000000000000000 | 20261019
    tree = _known_answer_tree()
    w = np.array([(e * 37) % KA_CAP for e in range(n)], dtype=np.int64)
    for e in range(0, n, 4):
        first = _oracle_tree(tree, KA_CAP).find(f32(uniform01(seed, e, 0, 0) * tree[0]))
        w[e] = first[1]
    want = [_known_answer_walk(tree, e, seed, int(w[e])) for e in range(n)]
    assert max(a for _, _, a in want) > 1                                 # some env needs more than one attempt
    trees, index = _dev(np.tile(tree, (n, 1))), _dev(w)
    prob = torch.full((n + 1,), -7.0, device=DEV)
    data_idx, tree_idx = (torch.full((n + 1,), -7, dtype=torch.int64, device=DEV) for _ in range(2))
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.check(lib.irbpp_sumtree_sample(_ptr(trees), _ptr(index), n, KA_CAP, 1, KA_STEP, seed, KA_TRIES, _ptr(prob), _ptr(data_idx),
                                     _ptr(tree_idx), _ptr(failed), _stream()), "irbpp_sumtree_sample")
    torch.cuda.synchronize()
    assert int(failed.item()) == 0
    np.testing.assert_array_equal(tree_idx.cpu().numpy()[:n], [t for t, _, _ in want])
    np.testing.assert_array_equal(data_idx.cpu().numpy()[:n], [t - (KA_CAP - 1) for t, _, _ in want])
    np.testing.assert_array_equal(prob.cpu().numpy()[:n], np.array([p for _, p, _ in want], dtype=f32))
    assert prob[n] == -7.0 and data_idx[n] == -7 and tree_idx[n] == -7


def test_pooled_sample_draws_the_generators_leaf():
    """The same for irbpp_replay_pool_sample with values NULL, one memory and one draw: the env field of the counter is
    0xFFFFFFFF whatever the env.  The write index sits on the first attempt's leaf."""
    import ctypes
    from irbpp_amd import replay
    L, _ = _lib()
    seed = 0x8000000000000000 | 77
    tree = _known_answer_tree()
    w = int(_oracle_tree(tree, KA_CAP).find(f32(uniform01(seed, POOL_RNG_ENV, 0, 0) * tree[0]))[1])
    t, p, attempts = _known_answer_walk(tree, POOL_RNG_ENV, seed, w)
    assert attempts > 1
    assert t != _known_answer_walk(tree, 0, seed, w)[0]                   # (env field 0 would give another leaf)
    mem = VectorReplayMemory(1, KA_CAP, 1, multi_step=KA_STEP, device=DEV, use_hip=True)
    mem.sum_tree.copy_(_dev(tree[None, :]))
    mem.index.fill_(w)
    mem.full.fill_(True)
    out = [torch.full((2,), -7, dtype=dt, device=DEV) for dt in (torch.int64, torch.float32, torch.int64, torch.int64, torch.float32)]
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    view = mem._view()
    L.check(mem._pool_lib.irbpp_replay_pool_sample(ctypes.byref(view), 1, replay._p(None), seed, KA_TRIES, 0.4,
                                                   *[replay._p(x) for x in out], replay._p(failed), replay._stream(mem.device)),
            "irbpp_replay_pool_sample")
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in out]
    assert int(failed.item()) == 0
    assert (got[0][0], got[1][0], got[2][0], got[3][0]) == (0, p, t - (KA_CAP - 1), t)
    assert got[4][0] == 1.0 and all(g[1] == -7 for g in got)
