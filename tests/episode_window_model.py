"""A plain model of the device-side episode windows (irbpp_amd/csrc/irbpp_metrics.hip) and the synthetic step outputs the
window-kernel tests feed them: the trainer's three deque(maxlen=W) (trainer.py:145-147, 168-178) with the key of every entry
beside them, the rows the trainer logs from them (trainer.py:215-222), and scenario builders that put the update kernel on
every path of its segment loop.  numpy only: tests/test_episode_window_model_cpu.py checks all of it without a GPU."""
from collections import deque, namedtuple

import numpy as np

UPDATE_THREADS = 1024                    # WINDOW_UPDATE_THREADS of irbpp_metrics.hip: one workgroup, thread t owns seg bins


def seg_of(n):
    """Bins per thread of the update kernel at n bins."""
    return (n + UPDATE_THREADS - 1) // UPDATE_THREADS


# ---------------------------------------------------------------------------------------------------------------------------
# the rows the trainer logs
# ---------------------------------------------------------------------------------------------------------------------------
def logged_row(T, episode_rewards, episode_ratio, episode_counter):
    """trainer.py:215-222 at step T: (T, len, mean r, max r, min r, mean ratio, mean counter), NaN where nothing is logged."""
    row = [T, len(episode_rewards)] + [np.nan] * 5
    if len(episode_rewards) != 0:
        row[2:5] = np.mean(episode_rewards), np.max(episode_rewards), np.min(episode_rewards)
    if len(episode_ratio) != 0:
        row[5] = np.mean(episode_ratio)
    if len(episode_counter) != 0:
        row[6] = np.mean(episode_counter)
    return row


def trainer_rows(steps, W):
    """trainer.py:145-147, 168-178, 215-222 over (done, infos) per step: one row per step, NaN where nothing is logged."""
    episode_rewards = deque(maxlen=W)
    episode_ratio = deque(maxlen=W)
    episode_counter = deque(maxlen=W)
    rows = []
    for T, (done, infos) in enumerate(steps, start=1):
        for _ in range(len(infos)):
            if done[_] and infos[_]['Valid']:
                if 'reward' in infos[_].keys():
                    episode_rewards.append(infos[_]['reward'])
                else:
                    episode_rewards.append(infos[_]['episode']['r'])
                if 'ratio' in infos[_].keys():
                    episode_ratio.append(infos[_]['ratio'])
                if 'counter' in infos[_].keys():
                    episode_counter.append(infos[_]['counter'])
        rows.append(logged_row(T, episode_rewards, episode_ratio, episode_counter))
    return np.array(rows, dtype=np.float64)


def assert_rows_equal(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(nan_g, nan_w)
    g, w = np.where(nan_g, 0.0, got), np.where(nan_w, 0.0, want)
    bad = np.nonzero(g.view(np.int64) != w.view(np.int64))
    assert bad[0].size == 0, f"first differing row {got[bad[0][0]]} vs {want[bad[0][0]]}"


# ---------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------
class WindowModel(object):
    """The trainer's deques fed one step at a time.  step(parts): parts in global-bin order, each (global_offset, done,
    ep_reward, ratio, counter) with the bins in index order; every done != 0 appends round(float(r), 6), ratio and counter.
    entries[T - 1] is the window after step T, oldest first: (T_finished << 32 | global bin, r, ratio, counter) per entry;
    rows[T - 1] the row the trainer logs at T."""

    def __init__(self, W):
        self.W, self.T = W, 0
        self.keys = deque(maxlen=W)
        self.episode_rewards = deque(maxlen=W)
        self.episode_ratio = deque(maxlen=W)
        self.episode_counter = deque(maxlen=W)
        self.entries, self.rows = [], []

    def step(self, parts):
        self.T += 1
        for offset, done, ep_reward, ratio, counter in parts:
            for b in np.flatnonzero(np.asarray(done) != 0).tolist():
                self.keys.append((self.T << 32) | (offset + b))
                self.episode_rewards.append(round(float(ep_reward[b]), 6))
                self.episode_ratio.append(float(ratio[b]))
                self.episode_counter.append(int(counter[b]))
        self.entries.append(list(zip(self.keys, self.episode_rewards, self.episode_ratio, self.episode_counter)))
        self.rows.append(logged_row(self.T, self.episode_rewards, self.episode_ratio, self.episode_counter))

    def rows_array(self, first=1, count=None):
        """rows of steps first .. first + count - 1 as float64[count][7]"""
        last = len(self.rows) if count is None else first - 1 + count
        return np.array(self.rows[first - 1:last], dtype=np.float64).reshape(-1, 7)


def entries_array(entries):
    """A window's entries as the device stores them: int64[len][4] = key, bits of r, bits of ratio, counter (reserved 0)."""
    out = np.zeros((len(entries), 4), dtype=np.int64)
    if entries:
        k, r, q, c = zip(*entries)
        out[:, 0] = k
        out[:, 1] = np.array(r, dtype=np.float64).view(np.int64)
        out[:, 2] = np.array(q, dtype=np.float64).view(np.int64)
        out[:, 3] = np.array(c, dtype=np.int64) & 0xFFFFFFFF
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# rewards: Python's round(r, 6) is decided in the seventh decimal
# ---------------------------------------------------------------------------------------------------------------------------
HalfwayCases = namedtuple("HalfwayCases", "x exact_ties near")


def halfway_cases():
    """Values on and next to the half-way points of round(x, 6): x is the whole list, exact_ties and near two of its runs
    (x = exact_ties, -exact_ties, near, -near, the neighbours of near, ulp steps around near, a few specials)."""
    k = np.arange(-20000, 20000, dtype=np.float64)
    exact_ties = (2 * k + 1) / 128.0                    # seven decimals ending in 5, exact in binary: true ties, half to even
    near = (k + 0.5) / 1e6                              # p = x * 1e6 rounds to (or next to) a half-integer
    around = [np.nextafter(near, np.inf), np.nextafter(near, -np.inf),
              np.nextafter(np.nextafter(near, np.inf), np.inf), np.nextafter(np.nextafter(near, -np.inf), -np.inf)]
    # x whose rounded product is exactly k + 0.5 while the exact product is not: every ulp step of x around (k+0.5)/1e6
    steps = [near * (1 + d * 2.0 ** -52) for d in range(-3, 4)]
    x = np.concatenate([exact_ties, -exact_ties, near, -near] + around + steps + [np.array([0.0, -0.0, 5e-7, -5e-7, 1.5e-6,
                                                                                              2.5e-6, 1e-300, -1e-300])])
    return HalfwayCases(x, exact_ties, near)


_POOL = None
_POOL_BITS = None


def halfway_pool():
    """halfway_cases().x, built once."""
    global _POOL, _POOL_BITS
    if _POOL is None:
        _POOL = halfway_cases().x
        _POOL.setflags(write=False)
        _POOL_BITS = np.unique(_POOL.view(np.int64))
    return _POOL


def is_halfway(values):
    """Which of `values` are (bit for bit) members of the halfway pool."""
    halfway_pool()
    bits = np.asarray(values, np.float64).view(np.int64)
    at = np.minimum(np.searchsorted(_POOL_BITS, bits), _POOL_BITS.size - 1)
    return _POOL_BITS[at] == bits


# ---------------------------------------------------------------------------------------------------------------------------
# scenarios for the update kernel: synthetic step outputs of n bins
# ---------------------------------------------------------------------------------------------------------------------------
BIN_COUNTS = (1, 63, 1023, 1024, 1025, 2047, 2048, 2500, 4096, 8192)
WINDOWS = (1, 10, 37, 1000, 1024)
# every W above is 1 mod 3 and so is 2500: with every bin done, first_kept = n - W is a multiple of seg = 3 for all of them.
# W = 38 at 2500 bins puts that cut inside a segment (2462 = 3 * 820 + 2).
EXTRA_PAIRS = ((2500, 38),)
PREFILLS = ("empty", "partial", "wrapped")
SCRIPTS = ("none", "first", "last", "exactly_W", "W_plus_1", "all", "all_but_one", "random_0.01", "random_0.5", "wrap",
           "flag_bytes")

Step = namedtuple("Step", "done ep_reward ratio counter")            # uint8[n], float64[n], float64[n], int32[n]
Scenario = namedtuple("Scenario", "name n W steps first")            # first: index in steps of the script's own first step


def _outputs(rng, n, done):
    """Step outputs for the given flags: rewards half from the halfway pool, half uniform in [0, 20); the LAST finished bin
    (always kept: m >= 1) gets a halfway reward, so every non-empty append puts one into the window."""
    pool = halfway_pool()
    ep_reward = np.where(rng.random(n) < 0.5, pool[rng.integers(0, pool.size, n)], rng.uniform(0.0, 20.0, n))
    idx = np.flatnonzero(done)
    if idx.size:
        ep_reward[idx[-1]] = pool[rng.integers(0, pool.size)]
    return Step(np.ascontiguousarray(done, dtype=np.uint8), np.ascontiguousarray(ep_reward), rng.random(n),
                rng.integers(0, 200, n).astype(np.int32))


def _pick(rng, n, count):
    """`count` finished bins out of n, anywhere."""
    done = np.zeros(n, dtype=np.uint8)
    done[rng.choice(n, size=count, replace=False)] = 1
    return done


def _script_flags(script, n, W, rng):
    """The done flags of the script's own steps (a list of uint8[n]), or None where n bins cannot play it."""
    z = lambda: np.zeros(n, dtype=np.uint8)                                        # noqa: E731
    if script == "none":
        return [z(), z()]
    if script == "first":
        d = z(); d[0] = 1
        return [d, d.copy()]
    if script == "last":
        d = z(); d[n - 1] = 1
        return [d, d.copy()]
    if script == "exactly_W":
        return None if n < W else [_pick(rng, n, W), _pick(rng, n, W)]
    if script == "W_plus_1":
        if n < W + 1:
            return None
        d = z(); d[:W + 1] = 1                # the first W + 1 bins: rank == bin, the cut first_kept = 1 lies inside segment 0
        return [d, _pick(rng, n, W + 1)]
    if script == "all":
        return [np.ones(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)]
    if script == "all_but_one":               # bin n-2 unfinished: the oldest kept bin moves one down, off a segment's start
        if n < 3:
            return None
        d = np.ones(n, dtype=np.uint8); d[n - 2] = 0
        return [d, d.copy()]
    if script.startswith("random_"):
        p = float(script.split("_")[1])
        return [(rng.random(n) < p).astype(np.uint8) for _ in range(3)]
    if script == "wrap":                      # fill = k < W, then a burst of m <= W with k + m = W + 1: the append wraps the ring
        k, m = (W + 1) // 2, W // 2 + 1
        if W < 2 or n < max(k, m):
            return None
        return [_pick(rng, n, k), _pick(rng, n, m), _pick(rng, n, m)]
    if script == "flag_bytes":                # any non-zero byte is a finished bin
        return [rng.choice(np.array([0, 2, 255], dtype=np.uint8), size=n) for _ in range(3)]
    raise ValueError(script)


def _prefill_flags(prefill, n, W, rng):
    """Steps in front of the script: none; a partly filled window (head 0); or an overflowed one (full, head moved; None
    where n bins would need more than six steps for that)."""
    if prefill == "empty":
        return []
    if prefill == "partial":
        return [_pick(rng, n, min(n, max(1, W // 3)))]
    if prefill == "wrapped":
        c = min(n, W // 2 + 2)
        if 6 * c < W + 3:                     # too few bins to overflow the window in a handful of steps
            return None
        return [_pick(rng, n, c) for _ in range(-(-(W + 3) // c))]
    raise ValueError(prefill)


def scenario(script, n, W, prefill="empty", seed=0):
    """The scenario of that name, or None where it does not exist (W + 1 finished bins out of fewer; the wrap needs an
    empty window in front and W >= 2; an overflowed window in front needs bins enough)."""
    if script == "wrap" and prefill != "empty":
        return None
    rng = np.random.default_rng([seed, n, W, SCRIPTS.index(script), PREFILLS.index(prefill)])
    own = _script_flags(script, n, W, rng)
    if own is None:
        return None
    pre = _prefill_flags(prefill, n, W, rng)
    if pre is None:
        return None
    steps = [_outputs(rng, n, d) for d in pre + own]
    return Scenario(f"{script}/{prefill}/n{n}/W{W}", n, W, steps, len(pre))


def scenarios(n, W, seed=0):
    """Every scenario that exists at (n, W)."""
    out = [scenario(s, n, W, p, seed) for s in SCRIPTS for p in PREFILLS]
    return [s for s in out if s is not None]


def finished(step):
    """F of a step."""
    return int(np.count_nonzero(step.done))


def straddles(done, W, n):
    """True if the cut between dropped and kept finished bins falls INSIDE a thread's segment: F > W and the segment that
    holds the first kept bin also holds a finished bin that is dropped."""
    idx = np.flatnonzero(done)
    F, seg = idx.size, seg_of(n)
    if F <= W:
        return False
    first_kept = F - W
    return bool(idx[first_kept] // seg == idx[first_kept - 1] // seg)


def rounds_scenario(seed=0, steps=700):
    """n = W = 1024, every bin done in every step: each step pushes 1024 rewards through py_round6 and all of them are in
    the snapshot.  40 such steps hold 40 960 values; the halfway pool alone has 600 008, so the script runs `steps` = 700 of
    them: the whole pool, then uniform values in [0, 20) (116 792 of them), shuffled."""
    rng = np.random.default_rng([seed, 1024])
    n, pool = 1024, halfway_pool()
    total = steps * n
    assert total - pool.size >= 100_000
    values = np.concatenate([pool, rng.uniform(0.0, 20.0, total - pool.size)])
    rng.shuffle(values)
    values = values.reshape(steps, n)
    done = np.ones(n, dtype=np.uint8)
    out = [Step(done, np.ascontiguousarray(values[t]), rng.random(n), rng.integers(0, 200, n).astype(np.int32))
           for t in range(steps)]
    return Scenario("rounds/n1024/W1024", n, 1024, out, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# scenarios for the merge: P parts of 40 bins
# ---------------------------------------------------------------------------------------------------------------------------
MERGE_PARTS = (1, 2, 3, 63, 64)
MERGE_WINDOWS = (1, 10, 1000, 1024)
PART_BINS = 40
MERGE_STEPS = 64

MergeScenario = namedtuple("MergeScenario", "P W steps silent ramp_end equal_step last_start")   # steps[t][p] = Step


def merge_scenario(P, W, seed=0):
    """64 steps of P parts (part p owns global bins [40 p, 40 p + 40)):
      - steps 1..3: nothing finishes anywhere (every window empty: the NaN row);
      - a ramp of sparse steps until the finished bins of all parts number exactly W (step `equal_step`; the step that would
        cross W is trimmed to hit it), the total below W before it;
      - heavy steps (each bin finishes with probability 0.7; every bin where W >= 1000, or 40 bins a step would not fill the
        window in the steps there are): the total is above W, the working parts' windows fill up;
      - from `last_start` on only part P-1 finishes bins, all 40 per step, for ceil(W / 40) + 1 steps: the newest W entries
        all sit in the last part.
    Parts p % 3 == 1 never finish a bin, and part P-1 (P > 1) none before `last_start`: fill 0 beside full windows."""
    rng = np.random.default_rng([seed, P, W, 77])
    nb = PART_BINS
    last_len = -(-W // nb) + 1
    last_start = MERGE_STEPS - last_len + 1
    silent = [p for p in range(P) if P > 1 and (p % 3 == 1 or p == P - 1)]
    working = [p for p in range(P) if p not in silent]
    flags = np.zeros((MERGE_STEPS, P, nb), dtype=np.uint8)
    prob = min(1.0, max(W / 6.0, 1.0) / (len(working) * nb))
    total, t, equal_step = 0, 3, None
    while equal_step is None:                                # ramp: steps t + 1 ...
        d = np.zeros((P, nb), dtype=np.uint8)
        d[working] = rng.random((len(working), nb)) < prob
        if total + int(d.sum()) >= W:                        # trim the newest flags of the crossing step: exactly W in all
            flat = d.reshape(-1)
            on = np.flatnonzero(flat)
            flat[on[W - total:]] = 0
            equal_step = t + 1
        total += int(d.sum())
        flags[t] = d
        t += 1
        assert t < last_start - 2, "the ramp must leave room for heavy steps"
    for u in range(t, last_start - 1):                       # heavy
        flags[u][working] = rng.random((len(working), nb)) < (1.0 if W >= 1000 else 0.7)
    for u in range(last_start - 1, MERGE_STEPS):             # the last part alone
        flags[u][P - 1] = 1
    steps = [[_outputs(rng, nb, flags[u][p]) for p in range(P)] for u in range(MERGE_STEPS)]
    return MergeScenario(P, W, steps, silent, t, equal_step, last_start)


def merge_parts(ms, t):
    """Step t (1-based) of a merge scenario as WindowModel.step wants it."""
    return [(p * PART_BINS,) + tuple(ms.steps[t - 1][p]) for p in range(ms.P)]


def random_part_steps(P, count, density=0.3, seed=0):
    """`count` steps of P parts of 40 bins, each bin finished with probability `density`: steps[t][p] = Step."""
    rng = np.random.default_rng([seed, P, count, 5])
    return [[_outputs(rng, PART_BINS, rng.random(PART_BINS) < density) for _ in range(P)] for _ in range(count)]
