"""The plain model of the episode windows and the synthetic scenarios of tests/episode_window_model.py, checked without a
GPU: the multi-part model against the trainer's own loop on the concatenated bins, and every scenario against what its name
promises -- F per step, more than one bin per thread, a cut inside a segment, a wrap of a part-filled ring, a halfway reward
among the kept entries -- so that a scenario cannot quietly degenerate into the one-bin-per-thread corner."""
import numpy as np
import pytest

import episode_window_model as M
from episode_window_model import BIN_COUNTS, EXTRA_PAIRS, WINDOWS


def _infos(step):
    """(done, infos) of one step as the trainer sees them (vec_env._Infos)."""
    done, ep_reward, ratio, counter = step
    infos = [{"Valid": True} if not done[b] else
             {"counter": int(counter[b]), "ratio": float(ratio[b]), "Valid": True, "episode": {"r": round(float(ep_reward[b]), 6)}}
             for b in range(len(done))]
    return done != 0, infos


def _concat(steps_of_parts):
    return M.Step(*(np.concatenate(col) for col in zip(*steps_of_parts)))


def _fills(sc):
    """(fill before, F, fill after) per step of a scenario: fill' = min(W, fill + F)."""
    out, fill = [], 0
    for st in sc.steps:
        F = M.finished(st)
        out.append((fill, F, min(sc.W, fill + F)))
        fill = out[-1][2]
    return out


@pytest.mark.parametrize("P,W", [(1, 10), (3, 1), (3, 10), (64, 37), (63, 1000), (64, 1024)])
def test_multi_part_model_equals_the_trainer_loop_on_the_concatenated_bins(P, W):
    ms = M.merge_scenario(P, W)
    model = M.WindowModel(W)
    for t in range(1, M.MERGE_STEPS + 1):
        model.step(M.merge_parts(ms, t))
    want = M.trainer_rows([_infos(_concat(parts)) for parts in ms.steps], W)
    M.assert_rows_equal(model.rows_array(), want)
    for t, entries in enumerate(model.entries, start=1):                       # the recorded deques: ascending keys, newest at T
        keys = [e[0] for e in entries]
        assert keys == sorted(set(keys)) and len(keys) == want[t - 1, 1]
        assert all(k >> 32 <= t for k in keys)
    assert np.isnan(want[0, 2]) and want[0, 1] == 0


def test_single_window_model_equals_the_trainer_loop():
    for n, W in ((63, 10), (1025, 37), (2500, 38)):
        for sc in M.scenarios(n, W):
            model = M.WindowModel(W)
            for st in sc.steps:
                model.step([(0,) + tuple(st)])
            M.assert_rows_equal(model.rows_array(), M.trainer_rows([_infos(st) for st in sc.steps], W))


def test_entries_array_is_the_device_layout():
    e = M.entries_array([((3 << 32) | 7, 1.5, 0.25, 9), ((4 << 32) | 2, -2.0, 0.5, 0)])
    assert e.dtype == np.int64 and e.shape == (2, 4)
    assert e[0].tolist() == [(3 << 32) | 7, np.float64(1.5).view(np.int64), np.float64(0.25).view(np.int64), 9]
    assert M.entries_array([]).shape == (0, 4)


def test_halfway_pool_membership():
    pool = M.halfway_pool()
    assert pool.size == 600_008 and M.is_halfway(pool).all()
    assert not M.is_halfway(np.array([0.123, 7.0, np.nextafter(np.nextafter(np.nextafter(0.5 / 1e6, 1), 1), 1) * 3])).any()
    # the pool is about round(x, 6): on thousands of its members the rounded product alone (np.round) gives another answer
    x = pool[80_000:120_000]
    assert np.count_nonzero(np.round(x, 6) != np.array([round(float(v), 6) for v in x])) > 1000


@pytest.mark.parametrize("n", BIN_COUNTS)
def test_every_scenario_is_what_its_name_says(n):
    seg = M.seg_of(n)
    assert seg == {1: 1, 63: 1, 1023: 1, 1024: 1, 1025: 2, 2047: 2, 2048: 2, 2500: 3, 4096: 4, 8192: 8}[n]
    threads_with_bins = -(-n // seg)
    if n == 1025:
        assert 1024 - threads_with_bins == 511        # ceil(1025 / 2) = 513 threads hold bins; the last of them one bin
    if n == 2500:
        assert 1024 - threads_with_bins == 190 and n % seg == 1
    if n == 2047:
        assert n % seg == 1
    have = set()
    for W in WINDOWS + tuple(w for m, w in EXTRA_PAIRS if m == n):
        for sc in M.scenarios(n, W):
            script, prefill = sc.name.split("/")[:2]
            have.add((script, W))
            fills = _fills(sc)
            own = fills[sc.first:]
            Fs = [F for _, F, _ in own]
            assert all(st.done.shape == (n,) and st.done.dtype == np.uint8 for st in sc.steps)
            # the window in front of the script
            before = fills[sc.first][0]
            if prefill == "empty":
                assert sc.first == 0 and before == 0
            elif prefill == "partial":
                assert before == min(n, max(1, W // 3)) and (before < W or W == 1)
            else:
                assert before == W and sum(F for _, F, _ in fills[:sc.first]) > W        # overflowed: the ring's head has moved
            # F of the script's own steps
            if script == "none":
                assert Fs == [0, 0]
            elif script == "first":
                assert Fs == [1, 1] and all(st.done[0] for st in sc.steps[sc.first:])
            elif script == "last":
                assert Fs == [1, 1] and all(st.done[n - 1] for st in sc.steps[sc.first:])
            elif script == "exactly_W":
                assert Fs == [W, W]
            elif script == "W_plus_1":
                assert Fs == [W + 1, W + 1]
                if seg >= 2:
                    assert M.straddles(sc.steps[sc.first].done, W, n)        # first_kept = 1, inside segment 0
            elif script == "all":
                assert Fs == [n, n]
            elif script == "all_but_one":
                assert Fs == [n - 1, n - 1]
            elif script == "random_0.01":
                assert all(F <= 0.05 * n + 2 for F in Fs) and (n < 1000 or all(F > 0 for F in Fs))
            elif script == "random_0.5":
                assert all(0.3 * n <= F <= 0.7 * n for F in Fs) or n == 1
            elif script == "wrap":
                fill, F, _ = own[1]
                m = min(F, W)
                assert fill < W < fill + m, (fill, W, m)
            elif script == "flag_bytes":
                vals = np.unique(np.concatenate([st.done for st in sc.steps[sc.first:]]))
                assert set(vals.tolist()) <= {0, 2, 255} and (n < 63 or {2, 255} <= set(vals.tolist()))
            # a halfway reward among the kept entries: the newest entry of every non-empty append
            for st in sc.steps:
                idx = np.flatnonzero(st.done)
                if idx.size:
                    assert M.is_halfway(st.ep_reward[idx[-1]:idx[-1] + 1])[0]
    # every n plays the all-done and the random scripts, and -- where W + 1 bins exist -- the W + 1 script
    assert {s for s, _ in have} >= {"none", "first", "last", "all", "random_0.01", "random_0.5", "flag_bytes"}
    if n > 1:
        assert any(s == "W_plus_1" for s, _ in have) and any(s == "exactly_W" for s, _ in have)
    if n >= 63:
        assert any(s == "wrap" for s, _ in have)
    if n >= 1025:
        assert {W for s, W in have if s == "W_plus_1"} == set(WINDOWS) | {w for m, w in EXTRA_PAIRS if m == n}
    # more than one bin per thread: some all-done step cuts inside a segment (first_kept % seg != 0) ...
    if seg >= 2:
        inside = [W for W in WINDOWS + tuple(w for m, w in EXTRA_PAIRS if m == n) if (n - W) % seg != 0]
        assert inside, "no window puts the cut of an all-done step inside a segment"
        for W in inside:
            assert M.straddles(np.ones(n, np.uint8), W, n)
        # ... and with bin n-2 unfinished the cut moves off the segment's start wherever it sat on one
        for W in WINDOWS:
            sc = M.scenario("all_but_one", n, W)
            if W >= 2 and (n - W) % seg == 0:
                assert M.straddles(sc.steps[0].done, W, n), (n, W)


def test_the_kept_entries_hold_halfway_rewards():
    """Through the model: the window after every non-empty step of a scenario holds an entry whose raw reward is a halfway
    case, stored as Python rounds it."""
    for n, W in ((63, 10), (2500, 38), (1025, 1)):
        for sc in M.scenarios(n, W):
            model = M.WindowModel(W)
            for st in sc.steps:
                model.step([(5,) + tuple(st)])
                idx = np.flatnonzero(st.done)
                if idx.size:
                    key, r, _, _ = model.entries[-1][-1]
                    assert key == (model.T << 32) | (5 + int(idx[-1]))
                    assert M.is_halfway([st.ep_reward[idx[-1]]])[0] and r == round(float(st.ep_reward[idx[-1]]), 6)


def test_rounds_scenario_pushes_the_whole_pool_through():
    sc = M.rounds_scenario()
    assert sc.n == sc.W == 1024 and len(sc.steps) >= 40 and all(M.finished(st) == 1024 for st in sc.steps)
    values = np.concatenate([st.ep_reward for st in sc.steps])
    half = M.is_halfway(values)
    assert np.count_nonzero(half) >= M.halfway_pool().size
    rest = values[~half]
    assert rest.size >= 100_000 and rest.min() >= 0.0 and rest.max() < 20.0
    assert np.array_equal(np.sort(values[half].view(np.int64))[:5], np.sort(M.halfway_pool().view(np.int64))[:5])


@pytest.mark.parametrize("P", M.MERGE_PARTS)
@pytest.mark.parametrize("W", M.MERGE_WINDOWS)
def test_merge_scenarios_reach_their_cases(P, W):
    ms = M.merge_scenario(P, W)
    assert len(ms.steps) == M.MERGE_STEPS == 64 and all(len(parts) == P for parts in ms.steps)
    per_part = np.array([[M.finished(st) for st in parts] for parts in ms.steps])              # [step][part]
    cum = np.cumsum(per_part, axis=0)
    fills = np.minimum(cum, W)
    total = fills.sum(axis=1)
    assert (total[:3] == 0).all()                                       # all parts empty: the NaN rows
    e = ms.equal_step
    assert total[e - 1] == W and cum[e - 1].sum() == W                  # exactly W entries in all, none dropped yet
    if W > 1:
        assert any(0 < x < W for x in total[:e - 1])                   # below W
    assert cum[e].sum() > W                                             # above W: entries are dropped from here on ...
    if P - len(ms.silent) >= 2:
        assert total[-1] > W                                            # ... and the parts' fills together exceed W
    # parts that never finish a bin beside full windows
    if P > 1:
        before_last = fills[ms.last_start - 2]
        assert before_last[P - 1] == 0 and before_last.max() == W
        assert all(cum[-1][p] == 0 for p in ms.silent if p != P - 1)
    if P >= 3:
        assert fills[-1].min() == 0 and fills[-1].max() == W
    # all the newest entries in the last part
    assert (per_part[ms.last_start - 1:, :P - 1] == 0).all() and per_part[ms.last_start - 1:, P - 1].sum() >= W
    model = M.WindowModel(W)
    for t in range(1, M.MERGE_STEPS + 1):
        model.step(M.merge_parts(ms, t))
    assert len(model.entries[-1]) == W and all((k & 0xFFFFFFFF) >= (P - 1) * M.PART_BINS for k, _, _, _ in model.entries[-1])
