"""The placement log (irbpp_set_placement_log: the device-side PackingGame.packed, binPhy.py:296) read RAW -- the uint32 words and
the float64 heights as the kernels left them -- against ``oracle.packing.PackingGame.packed``, on every kernel that writes it: the
fused step of the transition kernels, irbpp_apply_kernel / irbpp_apply_wg_kernel (candidate rows, a wave and a workgroup per bin),
irbpp_apply_cells_kernel (step_cells), the chain build, and the wide path (action grids of up to 32 cells a side, whose step is
irbpp_apply_kernel).  Word: item (bits 0..15) | rot (16..19) | lx (20..24) | ly (25..29), include/irbpp.h.

Every comparison is assert_array_equal, no tolerance: the fields decoded by ``irbpp_amd.evaluate.decode_placement_words`` against
``[item, rot, lx, ly]`` of ``packed``, the word against the fields packed again (no bit outside them), the float64 height against
``packed[i][4]``.  The oracle plays alone first (its scripted policy reads its own observations), the GPU is then handed the same
actions; a bin's log row is read right after the step that reported ``done`` for it.

NOTHING IS LEFT OUT of a comparison.  A refused placement whose cell lies outside the grid of its rotation (lx > Ax - ax) gets the
height 1e3 from the kernel, and the oracle records the same: Space.get_possible_position fills posZmap with 1e3 and writes only the
cells inside that range (space.py:44-58), PackingGame.step reads posZmap[rot, lx, ly] before it looks at ``success``
(binPhy.py:266).  ``left_out`` stays in the bookkeeping, 0, and every test asserts it against its number of finished episodes.

A GpuVecEnv with several groups does not hand out the log (it belongs to each group's own GpuPackingEnv): no grouped case."""
import functools

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from irbpp_amd.evaluate import decode_placement_words
from irbpp_amd.vec_env import GpuPackingEnv, _ptr
from oracle.packing import PackingGame
from cell_step_helpers import mix_cells, scenario
from helpers import minz_action
from test_placement_word_cpu import pack_words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 500
eq = np.testing.assert_array_equal


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.int32)).to(DEV)


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


# -- the oracle's side: played once per scenario, kept, never changed ---------------------------------------------------------------
class Run(object):
    """What the oracle played: per step the order actions [T, n] (buffered), the actions [T, n] or cells [T, n, 3], the done flags
    [T, n], and ``packed[(t, b)]``: PackingGame.packed of the episode bin b finished at step t, rows [item, rot, lx, ly, height]."""

    def __init__(self, n, k):
        self.n, self.k = n, k
        self.order, self.actions, self.cells, self.done, self.packed = [], [], [], [], {}
        self.off_rows_accepted = 0     # accepted placements whose cell was no valid candidate row (step_cells)
        self.slot_matters = 0          # buffered placements whose chosen slot held another item than slot 0

    def freeze(self):
        for name in ("order", "actions", "cells", "done"):
            a = np.array(getattr(self, name))
            a.setflags(write=False)
            setattr(self, name, a)
        return self


def _games(shapes, seqs, n, kw, k):
    return [PackingGame(shapes, seqs, first_traj=1 + g, traj_stride=n, bufferSize=k, **kw) for g in range(n)]


@functools.lru_cache(maxsize=None)
def _oracle_rows(name, n, steps, k=1, bin_dimension=None, selected=S):
    """n bins with auto-reset (OracleVecEnv's trajectory assignment), scripted MINZ on candidate rows; buffered: the rotating
    order actions of test_wide_hierarchical_matches_the_oracles."""
    sh, seqs, kw = _scenario(name)
    kw = dict(kw, selectedAction=selected)
    if bin_dimension is not None:
        kw["bin_dimension"] = bin_dimension
    envs = _games(sh, seqs, n, kw, k)
    run = Run(n, k)
    obs = [e.reset() for e in envs]
    for t in range(steps):
        oa = np.array([(t * 5 + 1 + i) % k for i in range(n)])
        act, done = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
        for i, e in enumerate(envs):
            loc = obs[i]
            if k > 1:
                queue = [int(v) for v in obs[i][:k]]
                loc = e.get_action_candidates(int(oa[i]))
                assert e.next_item_ID == queue[oa[i]]
                run.slot_matters += int(queue[oa[i]] != queue[0])
            act[i] = minz_action(_f32(loc), selected)
            o, _, d, _ = e.step(int(act[i]))
            if k > 1:
                assert e.packed[-1][0] == queue[oa[i]]               # the item field follows the chosen buffer slot
            if d:
                run.packed[(t, i)] = np.array(e.packed, dtype=np.float64)
                done[i] = True
                o = e.reset()
            obs[i] = o
        run.order.append(oa)
        run.actions.append(act)
        run.done.append(done)
    return run.freeze()


@functools.lru_cache(maxsize=None)
def _oracle_cells(name, n, steps, seed=7):
    """The plan of cell_step_helpers: the cell of get_heuristic_action (DBLF, flip 3), every fifth placement a uniformly drawn cell."""
    sh, seqs, kw = _scenario(name)
    envs = _games(sh, seqs, n, kw, 1)
    run = Run(n, 1)
    for e in envs:
        e.reset()
    rng = np.random.RandomState(seed)
    ax, ay = int(envs[0].rangeX_A), int(envs[0].rangeY_A)
    for t in range(steps):
        cells = np.array([e.space.get_heuristic_action("DBLF", e.next_item_ID, 3) if e.next_item_ID >= 0 else (0, 0, 0) for e in envs],
                         dtype=np.int32)
        cells = mix_cells(cells, t, rng, sh.n_rot, ax, ay)
        done = np.zeros(n, dtype=bool)
        for i, e in enumerate(envs):
            rot, lx, ly = (int(v) for v in cells[i])
            rows = e.candidates
            listed = bool(((rows[:, 0] == rot) & (rows[:, 1] == lx) & (rows[:, 2] == ly) & (rows[:, 4] == 1)).any())
            e.candidates = np.array([[rot, lx, ly, 0.0, 0.0]])
            _, _, d, _ = e.step(0)
            run.off_rows_accepted += int(not d and not listed)
            if d:
                run.packed[(t, i)] = np.array(e.packed, dtype=np.float64)
                done[i] = True
                e.reset()
        run.cells.append(cells)
        run.done.append(done)
    return run.freeze()


@functools.lru_cache(maxsize=None)
def _oracle_sequential(name, episodes, k=1):
    """tools.test's protocol (tools.py:303-358): ONE environment, episode e on trajectory e + 1, ``packed`` per episode.  Buffered:
    tools.test_hierachical with the rotating order actions.  -> per episode (order actions, actions, packed, info, reward sum)."""
    sh, seqs, kw = _scenario(name)
    env = PackingGame(sh, seqs, bufferSize=k, **kw)
    out = []
    for _ in range(episodes):
        obs, order, acts, rsum = env.reset(), [], [], 0.0
        while True:
            loc = obs
            if k > 1:
                order.append((len(acts) * 5 + 1) % k)
                loc = env.get_action_candidates(order[-1])
            acts.append(minz_action(_f32(loc), S))
            obs, r, d, info = env.step(acts[-1])
            rsum += r
            if d:
                break
        out.append((tuple(order), tuple(acts), np.array(env.packed, dtype=np.float64), dict(info), rsum))
    return out


def _scenario(name):
    if name == "wide_free_form":        # test_wide_online_free_form_matches_both_oracles
        sh = synthetic.general_shapes(n_shapes=16, n_rot=4, fmin=4, fmax=14, seed=3)
        return sh, synthetic.make_sequences(sh.n_shapes, 32, 80, seed=2), {"resolutionA": 0.01, "resolutionH": 0.01}
    if name == "wide_lattice":          # test_wide_hierarchical_matches_the_oracles
        sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
        return sh, synthetic.make_sequences(sh.n_shapes, 64, 150, seed=5), {"resolutionA": 0.01, "resolutionH": 0.01}
    if name == "wide_odd":              # test_wide_odd_grid_and_fine_heightmap (the 30 x 26 grid is the caller's bin_dimension)
        sh = synthetic.general_shapes(n_shapes=12, n_rot=4, fmin=4, fmax=12, seed=7)
        return sh, synthetic.make_sequences(sh.n_shapes, 32, 80, seed=8), {"resolutionA": 0.01, "resolutionH": 0.01}
    if name == "short":                 # trajectories of five items: every episode runs out of items
        sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
        return sh, synthetic.make_sequences(sh.n_shapes, 16, 5, seed=5), {}
    return scenario(name)


# -- the GPU's side ------------------------------------------------------------------------------------------------------------------
class Tally(object):
    def __init__(self):
        self.entries = self.episodes = self.left_out = 0
        self.wide = self.both_wide = 0             # entries with lx >= 16 or ly >= 16 / with both
        self.refused_off_origin = 0                # refused entries with lx + ly > 0
        self.refused_wide = 0                      # refused entries with lx >= 16 or ly >= 16
        self.exhausted = 0                         # refused entries with the 0xFFFF item mark


def _compare(words, z, packed, tally, msg=""):
    """One finished episode: words uint32-as-int32 [..., cap] and z float64 [..., cap] of one bin (or of many bins that played
    the same episode) against ``packed``, refused entry included."""
    m = len(packed)
    words, z = np.asarray(words)[..., :m], np.asarray(z)[..., :m]
    item, rot, lx, ly = decode_placement_words(words)
    want = packed[:, :4].astype(np.int64)
    want[:, 0] &= 0xFFFF                           # the exhausted trajectory's -1 is the 0xFFFF mark
    for got, col, what in ((item, 0, "item"), (rot, 1, "rot"), (lx, 2, "lx"), (ly, 3, "ly")):
        eq(got, np.broadcast_to(want[:, col], got.shape), err_msg=f"{what} {msg}")
    eq(pack_words(item, rot, lx, ly), words.astype(np.int64) & 0xFFFFFFFF, err_msg=f"bits outside the fields {msg}")
    eq(z, np.broadcast_to(packed[:, 4], z.shape), err_msg=f"height {msg}")
    tally.entries += m
    tally.episodes += 1
    tally.wide += int(((want[:, 2] >= 16) | (want[:, 3] >= 16)).sum())
    tally.both_wide += int(((want[:, 2] >= 16) & (want[:, 3] >= 16)).sum())
    tally.refused_off_origin += int(want[-1, 2] + want[-1, 3] > 0)
    tally.refused_wide += int(want[-1, 2] >= 16 or want[-1, 3] >= 16)
    tally.exhausted += int(want[-1, 0] == 0xFFFF)


def _play(env, run, meta, z, tally, every_bin_plays_bin0=False):
    """The oracle's actions on the GPU; each bin's row read right after the step that reported done for it."""
    n = env.num_bins
    pick = (lambda a: np.repeat(a[:1], n, axis=0)) if every_bin_plays_bin0 else (lambda a: a)
    for t in range(len(run.done)):
        if run.k > 1:
            env.get_action_candidates(_dev(pick(run.order[t])))
        if len(run.cells):
            env.step_cells(_dev(pick(run.cells[t])))
        else:
            env.step(_dev(pick(run.actions[t])))
        h = env.step_info_host()
        eq(h["done"], pick(run.done[t]), err_msg=f"step {t}")
        if every_bin_plays_bin0:
            if run.done[t][0]:
                packed = run.packed[(t, 0)]
                eq(h["counter"], len(packed) - 1)
                _compare(meta.cpu().numpy(), z.cpu().numpy(), packed, tally, f"(step {t}, all {n} bins)")
            continue
        idx = np.nonzero(h["done"])[0]
        if len(idx):
            m, zz = meta[idx].cpu().numpy(), z[idx].cpu().numpy()
            for row, b in enumerate(idx):
                packed = run.packed[(t, int(b))]
                assert h["counter"][b] == len(packed) - 1
                _compare(m[row], zz[row], packed, tally, f"(step {t}, bin {b})")
    env.check_device_error()


def _env(name, n, k=1, tuning=0, seqs=None, **extra):
    sh, sq, kw = _scenario(name)
    return GpuPackingEnv(sh, sq if seqs is None else seqs, n, device=DEV, bufferSize=k, tuning=tuning, **dict(kw, **extra))


# -- a. the fused step, K = 1, 16-cell grid ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["free_form", "lattice"])
def test_fused_step_log_equals_packed(name):
    n, steps = 4, 40
    run = _oracle_rows(name, n, steps)
    env = _env(name, n)
    info = env.kernel_info()[1]
    assert "irbpp_apply" not in info and "chain" not in info and "wide" not in info, info     # the transition kernel places
    meta, z = env.enable_placement_log(64)
    env.reset()
    tally = Tally()
    _play(env, run, meta, z, tally)
    env.close()
    assert tally.episodes >= 2 and tally.left_out <= tally.episodes and tally.left_out == 0, vars(tally)


# -- b. a buffered step: get_action_candidates + step, irbpp_apply_wg_kernel on candidate rows --------------------------------------
@pytest.mark.parametrize("k", [3, 4])
def test_buffered_step_log_equals_packed(k):
    n, steps = 3, 45
    run = _oracle_rows("lattice", n, steps, k)
    assert run.slot_matters >= 10, run.slot_matters          # (asserted per placement in _oracle_rows: packed's item is the chosen slot's)
    env = _env("lattice", n, k)
    assert "irbpp_apply_wg_kernel alone" in env.kernel_info()[1]
    meta, z = env.enable_placement_log(64)
    env.reset()
    tally = Tally()
    _play(env, run, meta, z, tally)
    env.close()
    assert tally.episodes >= 2 and tally.left_out == 0, vars(tally)


# -- c. step_cells: irbpp_apply_cells_kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice", "free_form"])
def test_step_cells_log_equals_packed(name):
    """Drawn cells: refused entries away from cell (0, 0), and accepted cells that are no candidate row, whose height is
    recomputed from the footprint's bottom cells where the observation's validity bits do not list them."""
    n, steps = 4, 40
    run = _oracle_cells(name, n, steps)
    env = _env(name, n)
    meta, z = env.enable_placement_log(64)
    env.reset()
    tally = Tally()
    _play(env, run, meta, z, tally)
    env.close()
    assert tally.episodes >= 2 and tally.left_out == 0, vars(tally)
    assert tally.refused_off_origin >= 1 and run.off_rows_accepted >= 1, (vars(tally), run.off_rows_accepted)


# -- d. the wide path: resolutionA = 0.01, up to 32 cells a side ---------------------------------------------------------------------
WIDE_EPISODES = 4
WIDE_REFUSED_FLOOR = 9      # the oracle alone, _oracle_cells("wide32", 3, 25): all 9 episodes end on a refused cell with a coordinate >= 16


def test_wide_step_log_equals_packed():
    """K = 1 on 32 x 32 cells: the four episodes of the sequential protocol (shared with the evaluate() test below), one per bin;
    a bin that has finished goes on with action 0 and is not read again."""
    eps = _oracle_sequential("wide_free_form", WIDE_EPISODES)
    n = len(eps)
    env = _env("wide_free_form", n)
    assert "irbpp_wide_kernel alone" in env.kernel_info()[1]
    meta, z = env.enable_placement_log(64)
    env.reset()
    tally = Tally()
    finished = np.zeros(n, dtype=bool)
    for t in range(max(len(e[1]) for e in eps)):
        env.step(_dev([e[1][t] if t < len(e[1]) else 0 for e in eps]))
        h = env.step_info_host()
        for b in range(n):
            if not finished[b]:
                assert h["done"][b] == (t == len(eps[b][1]) - 1)
                if h["done"][b]:
                    finished[b] = True
                    _compare(meta[b].cpu().numpy(), z[b].cpu().numpy(), eps[b][2], tally, f"(bin {b})")
    env.check_device_error()
    env.close()
    assert tally.episodes == n and tally.left_out == 0
    # the oracle alone: 42 of the 78 entries of these four episodes have a coordinate >= 16, 8 have both
    assert 3 * tally.wide >= tally.entries and tally.both_wide >= 1, vars(tally)


@pytest.mark.parametrize("name,n,steps,k,kw", [
    ("wide_lattice", 3, 32, 3, {}),
    ("wide_odd", 3, 24, 1, {"bin_dimension": (0.30, 0.26, 0.30), "selected": 300})])
def test_wide_buffered_and_odd_grid_log_equals_packed(name, n, steps, k, kw):
    """K = 3 on 32 x 32 cells (the apply kernel alone), and a 30 x 26 grid."""
    run = _oracle_rows(name, n, steps, k, kw.get("bin_dimension"), kw.get("selected", S))
    extra = {"selectedAction": kw["selected"], "bin_dimension": kw["bin_dimension"]} if kw else {}
    env = _env(name, n, k, **extra)
    assert "irbpp_wide_kernel alone" in env.kernel_info()[1]
    assert (env.Ax, env.Ay) == ((30, 26) if kw else (32, 32))
    meta, z = env.enable_placement_log(64)
    env.reset()
    tally = Tally()
    _play(env, run, meta, z, tally)
    env.close()
    assert tally.episodes >= 2 and tally.left_out == 0, vars(tally)
    assert 3 * tally.wide >= tally.entries and tally.both_wide >= 1, vars(tally)


def test_wide_step_cells_log_has_refused_entries_beyond_cell_15():
    """step_cells on 32 x 32 cells with drawn cells (the wide path accepts irbpp_step_cells): the REFUSED branch at coordinates
    >= 16.  The oracle alone (seed 7, 3 bins, 25 steps): 9 episodes, 70 entries, 57 with a coordinate >= 16, 19 with both."""
    n, steps = 3, 25
    run = _oracle_cells("wide32", n, steps)
    env = _env("wide32", n)
    assert "irbpp_wide_kernel alone" in env.kernel_info()[1]
    meta, z = env.enable_placement_log(64)
    env.reset()
    tally = Tally()
    _play(env, run, meta, z, tally)
    env.close()
    assert tally.left_out == 0
    assert tally.refused_wide >= WIDE_REFUSED_FLOOR and tally.wide >= 1, vars(tally)




# -- e. the launch forms: a wave per bin, the apply kernel in front, the chain build -------------------------------------------------
@pytest.mark.parametrize("k,n,tuning,kernel", [
    (3, 2048, 0, "irbpp_apply_kernel alone"),                   # buffered: a wave per bin from 2048 bins on (irbpp_plan.h: plan_transition)
    (1, 4096, 0, "irbpp_apply_kernel in front"),                # online, lattice data: split from 4096 bins on (irbpp_plan.h: split_apply)
    (1, 3, _lib.TUNE_CHAIN, "irbpp_env_kernel_chain"),          # the chain build accepts any size
    (3, 3, _lib.TUNE_CHAIN, "irbpp_apply_wg_kernel alone")])
def test_every_bin_of_a_launch_form_logs_the_same_episode(k, n, tuning, kernel):
    """Every bin replays the trajectories of the oracle's single environment (test_gpu_large_forms._replay_table): one oracle
    episode checks every row of the log."""
    from test_gpu_large_forms import _replay_table
    episodes = 2
    eps = _oracle_sequential("lattice", episodes, k)
    _, seqs, _ = _scenario("lattice")
    env = _env("lattice", n, k, tuning, seqs=_replay_table(seqs, n, episodes))
    info = env.kernel_info()[1]
    assert kernel in info, info
    meta, z = env.enable_placement_log(48)
    env.reset()
    tally = Tally()
    for order, acts, packed, oinfo, _ in eps:
        assert len(packed) <= 48
        for t, a in enumerate(acts):
            if k > 1:
                env.get_action_candidates(_dev(np.full(n, order[t])))
            env.step(_dev(np.full(n, a)))
            h = env.step_info_host()
            assert (h["done"] == (t == len(acts) - 1)).all(), t
        eq(h["counter"], oinfo["counter"])
        _compare(meta.cpu().numpy(), z.cpu().numpy(), packed, tally, f"(all {n} bins)")
    env.check_device_error()
    env.close()
    assert tally.episodes == episodes and tally.left_out == 0


# -- f. capacity, detaching, re-attaching, the exhausted trajectory ------------------------------------------------------------------
GUARD_WORD, GUARD_Z = 0x5A5A5A5A, -777.25
ERR_ARG = -1                                             # IRBPP_ERR_ARG (include/irbpp.h)


def _raw_log(n, cap, guard):
    meta = torch.full((n * cap + guard,), GUARD_WORD, dtype=torch.int32, device=DEV)
    z = torch.full((n * cap + guard,), GUARD_Z, dtype=torch.float64, device=DEV)
    return meta, z


def _attach(env, meta, z, cap):
    return env.lib.irbpp_set_placement_log(env._h, _ptr(meta), _ptr(z), cap)


@pytest.mark.parametrize("k", [1, 3])
def test_capacity_four_keeps_the_first_four_entries_and_nothing_else(k):
    """capacity = 4 over a row stride of 4, one guard element behind the last row, episodes longer than 4 (fused step, and the
    workgroup-per-bin apply kernel): entries 0 .. 3 are the oracle's, an index >= 4 touches neither the next bin's row nor the guard."""
    n, steps, cap = 4, 30, 4
    run = _oracle_rows("lattice", n, steps, k)
    env = _env("lattice", n, k)
    meta, z = _raw_log(n, cap, 1)
    assert _attach(env, meta, z, cap) == 0
    env.reset()
    episodes = 0
    for t in range(steps):
        if k > 1:
            env.get_action_candidates(_dev(run.order[t]))
        env.step(_dev(run.actions[t]))
        h = env.step_info_host()
        eq(h["done"], run.done[t])
        m, zz = meta.cpu().numpy(), z.cpu().numpy()
        assert m[-1] == GUARD_WORD and zz[-1] == GUARD_Z, f"guard written at step {t}"
        m, zz = m[:-1].reshape(n, cap), zz[:-1].reshape(n, cap)
        for b in np.nonzero(h["done"])[0]:
            packed = run.packed[(t, int(b))]
            assert len(packed) > cap
            _compare(m[b], zz[b], packed[:cap], Tally(), f"(step {t}, bin {b})")
            episodes += 1
        if t < cap - 1:                                  # t + 1 placements so far: the rest of every row still holds the pattern
            assert (m[:, t + 1:] == GUARD_WORD).all() and (zz[:, t + 1:] == GUARD_Z).all()
    env.check_device_error()
    env.close()
    assert episodes >= 2


def test_capacity_zero_and_detached_write_nothing_and_a_null_pair_is_refused():
    n, steps = 4, 12
    run = _oracle_rows("lattice", n, 40)
    env = _env("lattice", n)
    meta, z = _raw_log(n, 4, 0)
    assert _attach(env, None, z, 4) == ERR_ARG and _attach(env, meta, None, 4) == ERR_ARG
    assert _attach(env, meta, z, -1) == ERR_ARG
    assert _attach(env, meta, z, 0) == 0                 # attached with room for nothing
    env.reset()
    for t in range(steps):
        env.step(_dev(run.actions[t]))
    env.step_info_host()
    assert (meta == GUARD_WORD).all() and (z == GUARD_Z).all()
    assert _attach(env, meta, z, 4) == 0 and _attach(env, None, None, 0) == 0       # attached, then detached again
    for t in range(steps, 2 * steps):
        env.step(_dev(run.actions[t]))
    env.step_info_host()
    env.check_device_error()
    env.close()
    assert (meta == GUARD_WORD).all() and (z == GUARD_Z).all()
    assert run.done[:2 * steps].any()                    # (the refused branch ran too)


def test_reattached_log_continues_at_the_episodes_own_index():
    """A log attached after `late` steps: a bin still in its first episode gets entries late .. end of that episode at their own
    indices (the slots before stay untouched); episodes begun afterwards are logged whole."""
    n, steps, late, cap = 4, 40, 5, 64
    run = _oracle_rows("free_form", n, steps)
    assert not run.done[:late + 2].any()
    env = _env("free_form", n)
    env.reset()
    for t in range(late):
        env.step(_dev(run.actions[t]))
    meta, z = _raw_log(n, cap, 0)
    assert _attach(env, meta, z, cap) == 0
    first = np.ones(n, dtype=bool)
    partial = whole = 0
    for t in range(late, steps):
        env.step(_dev(run.actions[t]))
        h = env.step_info_host()
        eq(h["done"], run.done[t])
        for b in np.nonzero(h["done"])[0]:
            packed = run.packed[(t, int(b))]
            m, zz = meta.view(n, cap)[b].cpu().numpy(), z.view(n, cap)[b].cpu().numpy()
            if first[b]:
                assert (m[:late] == GUARD_WORD).all() and (zz[:late] == GUARD_Z).all()
                item, rot, lx, ly = decode_placement_words(m[late:len(packed)])
                eq(np.stack([item, rot, lx, ly], axis=1), packed[late:, :4].astype(np.int64))
                eq(zz[late:len(packed)], packed[late:, 4])
                first[b] = False
                partial += 1
            else:
                _compare(m, zz, packed, Tally(), f"(step {t}, bin {b})")
                whole += 1
    env.check_device_error()
    env.close()
    assert partial == n and whole >= 1, (partial, whole)


@pytest.mark.parametrize("k", [1, 3])
def test_exhausted_trajectory_is_logged_with_the_item_mark(k):
    """Trajectories of five items in an empty bin: every episode ends because nothing is left to place -- the refused entry carries
    item 0xFFFF (PackingGame's next_item_ID of -1; the reference's None), which evaluate() stops at, and the height 1e3."""
    n, steps = 3, 14
    run = _oracle_rows("short", n, steps, k)
    env = _env("short", n, k)
    meta, z = env.enable_placement_log(16)
    env.reset()
    tally = Tally()
    _play(env, run, meta, z, tally)
    env.close()
    assert tally.episodes >= 2 and tally.exhausted == tally.episodes, vars(tally)
    for packed in run.packed.values():
        assert packed[-1][0] == -1 and packed[-1][4] == 1e3 and (k > 1 or len(packed) == 6)


# -- evaluate() on the wide grid ------------------------------------------------------------------------------------------------------
def test_batched_evaluation_on_the_wide_grid_matches_the_sequential_protocol():
    """test_batched_evaluation_matches_sequential_reference_protocol at resolutionA = 0.01: statistics and trajs of evaluate()
    against the oracle run sequentially, positions after the same np.round(...) * scale / scale arithmetic on both sides."""
    from irbpp_amd.evaluate import evaluate, rotation_quaternion_xyzw
    sh, seqs, kw = _scenario("wide_free_form")
    eps = _oracle_sequential("wide_free_form", WIDE_EPISODES)
    out = evaluate(sh, seqs, WIDE_EPISODES, device=DEV, **kw)
    assert out["episodes"] == WIDE_EPISODES and out["unfinished"] == 0
    scale, res_a, wide = np.array([100.0, 100.0, 100.0]), kw["resolutionA"], 0
    for ep, (_, acts, packed, info, rsum) in enumerate(eps):
        assert out["ratio"][ep] == info["ratio"] and out["length"][ep] == len(acts) and out["reward_sum"][ep] == rsum
        assert len(out["trajs"][ep]) == len(packed) == info["counter"] + 1
        for got, (item, rot, lx, ly, height) in zip(out["trajs"][ep], packed):
            assert got[0] == item and got[1] == "%d.obj" % item
            flb = np.round((lx * res_a, ly * res_a, 0.30), decimals=6) * scale      # addObject (Interface.py:201)
            flb[2] = height * scale[2]                                              # adjustHeight (Interface.py:185-187)
            eq(got[2], flb / scale)
            eq(got[3], rotation_quaternion_xyzw(int(rot)))
            wide += int(lx >= 16 or ly >= 16)
    assert wide >= 20, wide
