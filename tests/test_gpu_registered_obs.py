"""Registered observation buffers (irbpp_register_obs_buffer) on every path that emits an observation.

For a registered buffer the library keeps one int32 per bin -- the candidate rows it stored last time -- and the next emit
through that pointer writes max(previous, current) rows only.  There are three writers of that count (the workgroup-per-bin
emit routine, the wave-per-bin emit kernel with its hand-off to the workgroup routine, irbpp_wide_kernel), a host decision
per launch (irbpp_plan.h: ROWS_TRACK / ROWS_FORGET) and the calls that invalidate.  A count that is off by one leaves a stale
candidate row in an observation and raises nothing, so every case here plays TWINS: environment A writes into registered
buffers (poisoned before the hand-over, visited in an irregular order), environment B -- same data, configuration, tuning
and actions -- takes a fresh unregistered tensor per call, and every observation, reward, done flag and step output is
bit-equal.  The online data sets also run once with OracleVecEnv as a third player, which pins twin B to the truth.

A schedule in which no count ever falls would pass with the clearing code deleted: every run records the row counts of
twin B's observations per buffer and asserts what it contained (RunLog.check).  The seeds below were chosen on the host with
the C oracle alone, which meets the same conditions on them."""
import functools

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from irbpp_amd.vec_env import GpuPackingEnv, GpuVecEnv, _ptr
from helpers import minz_action

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 500


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


# -------------------------------------------------------------------------------------------------------------------
# data sets: (shapes, sequences, keyword arguments); "blockout" and "general" are the ones of
# test_registered_obs_buffers_deliver_the_same_observations
# -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def data(kind):
    from bench import make_workload
    if kind in ("blockout", "general", "blockout_r8"):
        sh, seqs, kw = make_workload(kind)
        return sh, seqs[:400], dict(kw)
    if kind == "blockout_k3":
        sh, seqs, kw = make_workload("blockout")
        return sh, seqs[:400], dict(kw, bufferSize=3)
    if kind == "blockout_k10":
        sh, seqs, kw = make_workload("blockout_k10")
        return sh, seqs[:400], dict(kw)
    if kind == "handoff":           # test_wave_emit_serves_bins_that_need_the_workgroup: more than S = 40 candidates at most steps
        sh = synthetic.cube_shapes()
        return sh, synthetic.make_sequences(sh.n_shapes, 64, 60, seed=77), dict(selectedAction=40)
    if kind == "wide":              # test_wide_online_free_form_matches_both_oracles: a 32 x 32 action grid
        sh = synthetic.general_shapes(n_shapes=16, n_rot=4, fmin=4, fmax=14, seed=3)
        return sh, synthetic.make_sequences(sh.n_shapes, 32, 80, seed=2), dict(resolutionA=0.01, resolutionH=0.01)
    if kind == "levels":            # test_levels_16x16_blockout_r4: 60 height levels
        sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
        return sh, synthetic.make_sequences(sh.n_shapes, 32, 150, seed=5), dict(resolutionZ=0.005)
    if kind == "small":             # the oracle's size: the blockout set of the online parity tests
        sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
        return sh, synthetic.make_sequences(sh.n_shapes, 64, 150, seed=5), {}
    if kind == "small_general":
        sh = synthetic.general_shapes(n_shapes=24, n_rot=8, seed=1)
        return sh, synthetic.make_sequences(sh.n_shapes, 64, 60, seed=9), {}
    raise KeyError(kind)


# -------------------------------------------------------------------------------------------------------------------
# host-side helpers (numpy only: the seed search on the host imports them)
# -------------------------------------------------------------------------------------------------------------------
def ring_order(seed, steps, nbuf=3):
    """Which buffer of the ring each step writes: drawn, not round-robin -- a buffer waits for several steps and then receives
    bins whose counts have moved both ways since."""
    return np.random.default_rng(seed).integers(0, nbuf, size=steps)


def row_counts(obs, s):
    """leading candidate rows of the [S][5] block that are not all zero, per bin"""
    rows = np.asarray(obs)[:, :5 * s].reshape(len(obs), s, 5)
    return np.cumprod((rows != 0).any(axis=2), axis=1).sum(axis=1)


def fallback_bins(obs, s, bin_z):
    """bins whose rows are the no-candidate fallback (binPhy.py:217-225): H = the bin's height in every row"""
    rows = np.asarray(obs)[:, :5 * s].reshape(len(obs), s, 5)
    return rows[:, 0, 3] == np.float32(bin_z)


def script_actions(obs, t, s, rng):
    """MINZ, and at every seventh step a quarter of the bins act at random over all S rows (zero-padded ones included)"""
    act = np.array([minz_action(o, s) for o in np.asarray(obs)], dtype=np.int32)
    if t % 7 == 3:
        rnd = rng.integers(0, s, size=len(act)).astype(np.int32)
        act = np.where(np.arange(len(act)) % 4 == t % 4, rnd, act).astype(np.int32)
    return act


class RunLog(object):
    """What a run contained, from twin B's observations: per observation the buffer it went to in twin A and the row count
    of every bin."""

    def __init__(self, s, bin_z=0.30):
        self.s, self.bin_z, self.steps = s, bin_z, []

    def add(self, buf, obs, done=None):
        obs = obs.cpu().numpy() if isinstance(obs, torch.Tensor) else np.asarray(obs)
        done = np.zeros(len(obs), bool) if done is None else np.asarray(done.cpu() if isinstance(done, torch.Tensor) else done).astype(bool)
        self.steps.append((buf, row_counts(obs, self.s), fallback_bins(obs, self.s, self.bin_z), done))

    def forget(self, buf):
        """the buffer's contents are no longer what the log last saw go into it (another layout, a new registration)"""
        self.steps.append((buf, None, None, None))

    def facts(self):
        last, prev = {}, None
        f = dict(falls=0, rises=0, full=0, fallbacks=0, resets=0, fall_rows=0, written=0, order_matters=0)
        for buf, c, fb, done in self.steps:
            if c is None:
                last.pop(buf, None)
                continue
            f["full"] += int(((c == self.s) & ~fb).sum())
            f["fallbacks"] += int(fb.sum())
            f["resets"] += int(done.sum())
            if buf in last:
                d = last[buf] - c
                per_buf = int(np.maximum(d, 0).sum())
                f["falls"] += int((d > 0).sum())
                f["rises"] += int((d < 0).sum())
                f["fall_rows"] += per_buf
                f["written"] += int(np.maximum(last[buf], c).sum())
                if prev is not None and per_buf != int(np.maximum(prev - c, 0).sum()):
                    f["order_matters"] += 1
            last[buf] = c
            prev = c
        return f

    def check(self, full=False, fallback=True, resets=True, order=True, share=0.05):
        f = self.facts()
        print("run contained:", f)
        assert f["falls"] > 0 and f["rises"] > 0, f                  # prev > nrows for the SAME buffer, and the reverse
        assert not full or f["full"] > 0, f                          # a bin at exactly S rows from the more-than-S selection
        assert not fallback or f["fallbacks"] > 0, f                 # a no-candidate fallback
        assert not resets or f["resets"] > 0, f                      # an auto-reset
        assert f["fall_rows"] >= share * f["written"], f             # the rows only the clearing code zeroes: >= 5 % of the rows written
        assert not order or f["order_matters"] > 0, f                # measured against the previous STEP the falls are other ones
        return f


# -------------------------------------------------------------------------------------------------------------------
# device-side helpers
# -------------------------------------------------------------------------------------------------------------------
def twins(kind, n, tuning=0, tuning_b=None, **extra):
    sh, seqs, kw = data(kind)
    kw = dict(kw, **extra)
    a = GpuPackingEnv(sh, seqs, n, device=DEV, tuning=tuning, **kw)
    b = GpuPackingEnv(sh, seqs, n, device=DEV, tuning=tuning if tuning_b is None else tuning_b, **kw)
    return a, b


def poisoned(n, width, j=0):
    """a buffer full of a non-zero pattern (nothing the library leaves unwritten can pass for a zero row)"""
    t = torch.arange(n * width, dtype=torch.float32, device=DEV).reshape(n, width) % 13.0 + 1.5 + j
    return t.contiguous()


def make_ring(env, nbuf=3, width=None):
    bufs = [poisoned(env.num_bins, env.loc_obs_len if width is None else width, j) for j in range(nbuf)]
    for t in bufs:
        env.register_obs_buffer(t)
    return bufs


def reset_into(env, out):
    _lib.check(env.lib.irbpp_reset(env._h, _ptr(out), env._stream()), "irbpp_reset")
    return out


def reset_bins_into(env, bins, out):
    _lib.check(env.lib.irbpp_reset_bins(env._h, _ptr(bins), int(bins.numel()), _ptr(out), env._stream()), "irbpp_reset_bins")
    return out


def same_info(a, b, what):
    ia, ib = a.step_info_host(), b.step_info_host()
    for key in ib:
        np.testing.assert_array_equal(ia[key], ib[key], err_msg=f"{key}, {what}")
    return ib


def same_step(ra, rb, a, b, what):
    """(obs, reward, done) of a step of both twins and their step outputs -> B's done flags"""
    assert torch.equal(ra[0], rb[0]), f"{what}: the registered buffer differs"
    assert torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2]), f"{what}: reward / done"
    return same_info(a, b, what)["done"]


def play(regs, b, order, steps, log, seed, ob, oracle=None, oobs=None, t0=0, tag=""):
    """`steps` steps: every (environment, ring) of `regs` steps into ring[order[t]], B into a fresh tensor, scripted actions
    from B's observation.  -> B's last observation (and the oracle's)."""
    s = b.S
    rng = np.random.default_rng(seed)
    for t in range(t0, t0 + steps):
        act_np = script_actions(ob.cpu().numpy(), t, s, rng)
        act = torch.from_numpy(act_np).to(DEV)
        rb = b.step(act)
        for j, (a, ring) in enumerate(regs):
            dst = ring[int(order[t])]
            ra = a.step(act, obs_out=dst)
            assert ra[0].data_ptr() == dst.data_ptr()
            done = same_step(ra, rb, a, b, f"{tag} step {t}, env {j}")
        ob = rb[0]
        log.add(int(order[t]), ob, done)
        if oracle is not None:
            oobs, orew, odone, _ = oracle.step(act_np)
            oobs = _f32(oobs)
            np.testing.assert_array_equal(ob.cpu().numpy(), oobs, err_msg=f"{tag} step {t}: twin B against the oracle")
            np.testing.assert_array_equal(done, odone)
    return ob, oobs


def finish(*envs):
    for e in envs:
        e.check_device_error()
        e.close()


def run_form(kind, n, steps, tuning, seed, expect=(), full=False, nbuf=3, order=None, tuning_b=None, oracle=False, **extra):
    a, b = twins(kind, n, tuning, tuning_b, **extra)
    info = a.kernel_info()[1]
    for name in expect:
        assert name in info, info
    if tuning & _lib.TUNE_NO_SPECIALISED:                # (the builds that read Params: no "_s<k>" kernel in the plan)
        assert not any(f"_s{k}" in info for k in range(1, 6)), info
    ring = make_ring(a, nbuf)
    order = ring_order(seed, steps, nbuf) if order is None else order
    log = RunLog(b.S, b.bin_dimension[2])
    oa, ob = a.reset(), b.reset()                     # (A: an unregistered tensor, a plain full write)
    assert torch.equal(oa, ob)
    oenv = oobs = None
    if oracle:
        from oracle.c_oracle import COracleVecEnv
        from oracle.packing import OracleVecEnv
        sh, seqs, kw = data(kind)
        oenv = (COracleVecEnv if oracle == "c" else OracleVecEnv)(n, sh, seqs, **dict(kw, **extra))
        oobs = _f32(oenv.reset())
        np.testing.assert_array_equal(ob.cpu().numpy(), oobs)
    play([(a, ring)], b, order, steps, log, seed, ob, oenv, oobs, tag=kind)
    log.check(full=full)
    finish(a, b)
    return log


# -------------------------------------------------------------------------------------------------------------------
# kernel forms
# -------------------------------------------------------------------------------------------------------------------
WAVE, BLOCK = "irbpp_emit_wave_kernel", "irbpp_emit_kernel"
FORMS = [
    # id, data, bins, steps, tuning, kernels the plan must name, a bin at exactly S rows
    ("block-blockout", "blockout", 67, 150, _lib.TUNE_BLOCK_EMIT, (BLOCK,), False),
    ("block-general", "general", 67, 50, _lib.TUNE_BLOCK_EMIT, (BLOCK,), True),
    ("wave-67", "blockout", 67, 150, _lib.TUNE_WAVE_EMIT, (WAVE,), False),                 # a partial last workgroup (four bins each)
    ("wave-130", "blockout", 130, 150, _lib.TUNE_WAVE_EMIT, (WAVE,), False),               # more than one round of waves
    ("wave-handoff", "handoff", 67, 60, _lib.TUNE_WAVE_EMIT, (WAVE,), True),               # bins with more than S candidates: need[wave]
    ("block-handoff", "handoff", 67, 60, _lib.TUNE_BLOCK_EMIT, (BLOCK,), True),
    ("split-wave", "blockout", 67, 150, _lib.TUNE_SPLIT_APPLY | _lib.TUNE_WAVE_EMIT, ("irbpp_apply_kernel", WAVE), False),
    ("split-block", "blockout", 67, 150, _lib.TUNE_SPLIT_APPLY | _lib.TUNE_BLOCK_EMIT, ("irbpp_apply_kernel", BLOCK), False),
    ("split-block-general", "general", 67, 50, _lib.TUNE_SPLIT_APPLY | _lib.TUNE_BLOCK_EMIT, ("irbpp_apply_kernel", BLOCK), True),
    ("fused-wave", "blockout", 67, 150, _lib.TUNE_FUSED_APPLY | _lib.TUNE_WAVE_EMIT, (WAVE,), False),
    ("fused-block", "blockout", 67, 150, _lib.TUNE_FUSED_APPLY | _lib.TUNE_BLOCK_EMIT, (BLOCK,), False),
    ("run-time-builds", "blockout", 67, 150, _lib.TUNE_NO_SPECIALISED | _lib.TUNE_WAVE_EMIT, (WAVE,), False),
    ("run-time-builds-general", "general", 67, 50, _lib.TUNE_NO_SPECIALISED, (BLOCK,), True),
    ("chain-blockout", "blockout", 33, 150, _lib.TUNE_CHAIN, ("irbpp_env_kernel_chain",), False),
    ("chain-general", "general", 33, 50, _lib.TUNE_CHAIN, ("irbpp_env_kernel_chain",), True),
    ("wide-grid", "wide", 4, 70, 0, ("irbpp_wide_kernel alone",), True),
    ("wide-levels", "levels", 4, 50, 0, ("irbpp_wide_kernel alone",), False),
    ("wg512", "general", 16, 50, _lib.TUNE_WG512, ("w512",), True),
]
# seed of the ring order and the random actions of the form cases (2 for the oracle cases): with it the C oracle alone, played on
# the host through ring_order / script_actions / RunLog, meets every condition of RunLog.check on every data set and size here
FORM_SEED = 1


@pytest.mark.parametrize("kind,n,steps,tuning,expect,full", [f[1:] for f in FORMS], ids=[f[0] for f in FORMS])
def test_kernel_forms_with_registered_buffers(kind, n, steps, tuning, expect, full):
    """Every form of the emit stage, a ring of three registered buffers in an irregular order against fresh tensors."""
    log = run_form(kind, n, steps, tuning, FORM_SEED, expect, full)
    assert len(log.steps) == steps


@pytest.mark.parametrize("emit", [_lib.TUNE_WAVE_EMIT, _lib.TUNE_BLOCK_EMIT], ids=["wave", "block"])
def test_graph_replay_with_registered_buffers(emit):
    """IRBPP_TUNE_GRAPH: the row-count pointer is a captured argument.  The ring in FIXED order and one persistent action
    tensor: three argument sets, each captured at its second use and replayed from its third on (50 uses each) -- the other
    parts of the graph key stand still: heavy_turn (lattice data have no heavy-first list) and obs_epoch (nothing is registered
    after the ring).  The library has no accessor for its replay count and launches directly, without a word, where capture
    or instantiation fails: this case pins the results of the IRBPP_TUNE_GRAPH path, not that a step was replayed."""
    n, steps = 64, 150
    a, b = twins("blockout", n, _lib.TUNE_GRAPH | emit)
    ring = make_ring(a, 3)
    act_a, act_b = (torch.zeros((n,), dtype=torch.int32, device=DEV) for _ in range(2))
    fresh = [torch.empty((n, b.obs_len), dtype=torch.float32, device=DEV) for _ in range(steps)]     # B: a tensor per step, none twice
    log = RunLog(S)
    oa, ob = a.reset(), b.reset()
    assert torch.equal(oa, ob)
    rng = np.random.default_rng(FORM_SEED)
    for t in range(steps):
        act = torch.from_numpy(script_actions(ob.cpu().numpy(), t, S, rng)).to(DEV)
        act_a.copy_(act)
        act_b.copy_(act)
        ra = a.step(act_a, obs_out=ring[t % 3])
        rb = b.step(act_b, obs_out=fresh[t])
        done = same_step(ra, rb, a, b, f"step {t}")
        ob = rb[0]
        log.add(t % 3, ob, done)
    log.check(order=True)
    finish(a, b)


def test_rotation_aliases_with_registered_buffers():
    """BlockOut at eight rotations: duplicate rotations list another rotation's vertex bits (alias_map) -- the default and
    IRBPP_TUNE_NO_ROT_ALIAS, BOTH into registered rings, against fresh tensors."""
    n, steps, seed = 32, 120, 1
    a, b = twins("blockout_r8", n, 0)
    a2 = GpuPackingEnv(*data("blockout_r8")[:2], n, device=DEV, tuning=_lib.TUNE_NO_ROT_ALIAS, **data("blockout_r8")[2])
    rings = [make_ring(a), make_ring(a2)]
    log = RunLog(S)
    oa, oa2, ob = a.reset(), a2.reset(), b.reset()
    assert torch.equal(oa, ob) and torch.equal(oa2, ob)
    play([(a, rings[0]), (a2, rings[1])], b, ring_order(seed, steps), steps, log, seed, ob, tag="blockout_r8")
    log.check()
    finish(a, a2, b)


def test_eight_registered_buffers_and_a_ninth():
    """The library holds eight registrations; the ninth is refused and changes nothing; all eight are cycled through."""
    n, steps, seed = 16, 96, 3
    a, b = twins("blockout", n, 0)
    ring = make_ring(a, 8)
    ninth = poisoned(n, a.loc_obs_len, 9)
    assert a.lib.irbpp_register_obs_buffer(a._h, _ptr(ninth)) != 0
    order = np.concatenate([np.random.default_rng(seed + k).permutation(8) for k in range(steps // 8)])
    assert set(order[:8]) == set(range(8))
    log = RunLog(S)
    oa, ob = a.reset(), b.reset()
    assert torch.equal(oa, ob)
    ob, _ = play([(a, ring)], b, order, steps, log, seed, ob, tag="eight")
    act = b.policy_minz(ob)                           # the refused one is a plain buffer: a full write
    same_step(a.step(act, obs_out=ninth), b.step(act), a, b, "the ninth buffer")
    log.check()
    finish(a, b)


ORACLE_CASES = [
    # id, data, bins, steps, tuning, a bin at exactly S rows, the oracle
    ("blockout-wave", "blockout", 2, 150, _lib.TUNE_WAVE_EMIT, False, "python"),      # (an episode of this set takes ~130 steps)
    ("general", "general", 5, 40, 0, True, "python"),
    ("blockout_r8", "blockout_r8", 3, 150, 0, False, "c"),      # (OracleVecEnv needs 10 s for this one: its restatement in C)
    ("small-wave", "small", 6, 60, _lib.TUNE_WAVE_EMIT, False, "python"),              # the set of the entry-point cases
    ("small-block", "small", 6, 60, _lib.TUNE_BLOCK_EMIT, False, "python"),
    ("small-general", "small_general", 5, 30, 0, True, "python"),
    ("handoff", "handoff", 5, 40, _lib.TUNE_WAVE_EMIT, True, "python"),
    ("wide", "wide", 3, 30, 0, True, "python"),
    ("levels", "levels", 3, 40, 0, False, "python"),
]


@pytest.mark.parametrize("kind,n,steps,tuning,full,oracle", [c[1:] for c in ORACLE_CASES], ids=[c[0] for c in ORACLE_CASES])
def test_twins_and_the_oracle(kind, n, steps, tuning, full, oracle):
    """Each data set once more with OracleVecEnv as the third player, at a handful of bins: twin B is the truth.  (The buffered
    sets' twin B -- get_action_candidates and the buffered step on unregistered tensors -- is what test_gpu_parity.py plays
    against the oracles on these data; here it is pinned to twin A.)"""
    run_form(kind, n, steps, tuning, 2, full=full, oracle=oracle)            # seed 2


# -------------------------------------------------------------------------------------------------------------------
# entry points
# -------------------------------------------------------------------------------------------------------------------
EMITS = pytest.mark.parametrize("emit", [_lib.TUNE_WAVE_EMIT, _lib.TUNE_BLOCK_EMIT], ids=["wave", "block"])


@EMITS
def test_reset_into_registered_buffers(emit):
    """irbpp_reset through a registered pointer (ROWS_TRACK in MODE_RESET): after steps into buffer 0, a reset into buffer 1
    while buffer 0's counts are old, steps into both, and a reset into buffer 0 over counts of mid-episode bins."""
    n, seed = 67, 4
    a, b = twins("small", n, emit)                                       # (episodes of about 30 steps)
    ring = make_ring(a, 2)
    log = RunLog(S)
    assert torch.equal(reset_into(a, ring[0]), ob := b.reset())
    log.add(0, ob)
    order = np.zeros(200, dtype=np.int64)
    ob, _ = play([(a, ring)], b, order, 35, log, seed, ob, tag="after the first reset")
    assert torch.equal(reset_into(a, ring[1]), ob := b.reset())        # another buffer; buffer 0 keeps counts of step 34
    log.add(1, ob)
    order[35:70] = np.arange(35) % 2 == 0                                # 1, 0, 1, 0 ...: buffer 0 next sees bins 36 steps on
    ob, _ = play([(a, ring)], b, order, 35, log, seed + 1, ob, t0=35, tag="after the second reset")
    assert torch.equal(reset_into(a, ring[0]), ob := b.reset())        # full bins' counts fall to an empty bin's
    log.add(0, ob)
    play([(a, ring)], b, order, 15, log, seed + 2, ob, t0=70, tag="after the third reset")
    log.check()
    finish(a, b)


@EMITS
def test_reset_bins_into_a_registered_buffer(emit):
    """irbpp_reset_bins of a third of the bins through a registered pointer writes a row per LISTED bin, and the next step into
    the same buffer is complete.  This pins the CONTENTS on that path, not the forgetting (ROWS_FORGET): an empty bin's
    observation holds the fewest rows any observation holds (16 here), so a count left standing never under-writes the rows a
    listed reset stored.  The memset itself is pinned by the same-storage cases of test_buffered_location_buffers."""
    n, seed = 67, 5
    a, b = twins("small", n, emit)
    ring = make_ring(a, 2)
    log = RunLog(S)
    ob = b.reset()
    assert torch.equal(a.reset(), ob)
    order = ring_order(seed, 90, 2)
    listed = torch.arange(1, n, 3, dtype=torch.int32, device=DEV)
    t0 = 0
    for part in range(3):
        ob, _ = play([(a, ring)], b, order, 20, log, seed + part, ob, t0=t0, tag=f"part {part}")
        t0 += 20
        dst = ring[part % 2]
        before = dst.clone()
        reset_bins_into(a, listed, dst)
        log.forget(part % 2)
        rows_b = b.reset_bins(listed)
        assert torch.equal(dst[:listed.numel()], rows_b), f"part {part}: the listed bins' reset observations"
        assert torch.equal(dst[listed.numel():], before[listed.numel():])          # (rows by list position, nothing beyond)
        ob = ob.clone()
        ob[listed.long()] = rows_b                                                  # what the caller acts on next
        order[t0] = part % 2                                                        # the same buffer, straight away
    play([(a, ring)], b, order, 20, log, seed + 3, ob, t0=t0, tag="last part")
    log.check()
    finish(a, b)


@pytest.mark.parametrize("kind,emit", [("blockout", _lib.TUNE_WAVE_EMIT), ("blockout", _lib.TUNE_BLOCK_EMIT), ("general", 0), ("wide", 0)],
                         ids=["wave", "block", "general", "wide"])
def test_cell_and_heuristic_steps_into_registered_buffers(kind, emit):
    """irbpp_step_cells and irbpp_heuristic_step (every method the configuration supports) with obs_out registered."""
    n = 4 if kind == "wide" else 35
    a, b = twins(kind, n, emit)
    ring = make_ring(a, 3)
    log = RunLog(a.S, a.bin_dimension[2])
    oa, ob = a.reset(), b.reset()
    assert torch.equal(oa, ob)
    methods = ["MINZ", "DBLF", "FIRSTFIT"] + ([] if kind == "wide" else ["HM"])
    order = ring_order(6, 120)
    for t in range(120):
        dst = ring[int(order[t])]
        m = methods[(t // 5) % len(methods)]
        if t % 3 == 2 and kind == "wide":                    # the caller's cells: those of the MINZ candidate row
            pick = b.policy_minz(ob).long()
            cells = ob[:, :5 * a.S].reshape(n, a.S, 5)[torch.arange(n, device=DEV), pick, :3].to(torch.int32).contiguous()
            ra, rb = a.step_cells(cells.clone(), obs_out=dst), b.step_cells(cells)
        elif t % 3 == 2:                                     # ... or another heuristic's choice
            cells = b.heuristic_action(methods[(t // 3) % len(methods)], t % 4)
            ra, rb = a.step_cells(cells.clone(), obs_out=dst), b.step_cells(cells)
        else:
            ra, rb = a.heuristic_step(m, t % 4, obs_out=dst), b.heuristic_step(m, t % 4)
        done = same_step(ra, rb, a, b, f"step {t} ({m})")
        ob = rb[0]
        log.add(int(order[t]), ob, done)
    log.check(full=kind in ("general", "wide"))
    finish(a, b)


@pytest.mark.parametrize("k,same_storage", [(3, True), (3, False), (10, True), (10, False)],
                         ids=["k3-same-storage", "k3-invalidate", "k10-same-storage", "k10-invalidate"])
@EMITS
def test_buffered_location_buffers(emit, k, same_storage):
    """A buffered environment: get_action_candidates into registered location buffers, interleaved with steps.  Either the
    buffered step gets the SAME storage as obs_out (it writes the order observation through the registered pointer:
    ROWS_FORGET, irbpp_apply_wg_kernel's row of the plan), or the caller invalidates in between and the step writes elsewhere."""
    n, steps, seed = 35, 100, 7
    a, b = twins("blockout_k3" if k == 3 else "blockout_k10", n, emit)
    assert "irbpp_apply_wg_kernel alone" in a.kernel_info()[1]
    locs = make_ring(a, 3, a.loc_obs_len)
    assert a.obs_len <= a.loc_obs_len
    order = ring_order(seed, steps)
    log = RunLog(S)
    assert torch.equal(a.reset(), b.reset())
    rng = np.random.default_rng(seed)
    done = None                                              # (a location observation carries no done flag: the step's before it)
    for t in range(steps):
        slot = torch.from_numpy(rng.integers(0, k, size=n).astype(np.int32)).to(DEV)
        u = int(order[t])
        la, lb = a.get_action_candidates(slot, obs_out=locs[u]), b.get_action_candidates(slot)
        assert torch.equal(la, lb), f"step {t}: location observation in buffer {u}"
        log.add(u, lb, done)
        act = torch.from_numpy(script_actions(lb.cpu().numpy(), t, S, rng)).to(DEV)
        if same_storage:
            v = int(order[(t * 5 + 1) % steps])              # any of the three, the one just written included
            out = locs[v].view(-1)[:n * a.obs_len].view(n, a.obs_len)
            ra = a.step(act, obs_out=out)
            log.forget(v)
        else:
            if t % 2:
                a.invalidate_obs_buffers(locs[u] if t % 4 == 1 else None)
                for w in ([u] if t % 4 == 1 else range(3)):
                    log.forget(w)
            ra = a.step(act)
        rb = b.step(act)
        done = same_step(ra, rb, a, b, f"step {t}: order observation")
    log.check()
    finish(a, b)


@EMITS
def test_load_and_copy_bins_under_registered_buffers(emit):
    """load_bins / copy_bins move the bins to another state while the registered buffers hold counts of the old one; with the
    caller's observation rows travelling (fork_bins(obs=...)) the buffer is invalidated.  The next steps are complete."""
    n, seed = 34, 8
    a, b = twins("small", n, emit)
    src_a, src_b = twins("small", n, emit, traj_start=40)
    ring = make_ring(a, 3)
    log = RunLog(S)
    ob = b.reset()
    assert torch.equal(reset_into(a, ring[0]), ob)
    sa, sb = src_a.reset(), src_b.reset()
    for t in range(30):                                      # the source: 30 steps ahead
        act = src_b.policy_minz(sb)
        sa, sb = src_a.step(act)[0], src_b.step(act)[0].clone()
    order = ring_order(seed, 120)
    ob, _ = play([(a, ring)], b, order, 12, log, seed, ob, tag="before save")
    blob_a, blob_b = a.save_bins(np.arange(n)), b.save_bins(np.arange(n))
    saved = ob.clone()
    ob, _ = play([(a, ring)], b, order, 25, log, seed + 1, ob, t0=12, tag="before load")
    a.load_bins(np.arange(n), blob_a)                        # back to step 12: every buffer holds counts of later states
    b.load_bins(np.arange(n), blob_b)
    ob, _ = play([(a, ring)], b, order, 25, log, seed + 2, saved, t0=37, tag="after load")
    # a third of the bins continue from the source environment's bins; the observation rows travel inside the registered buffer
    dst_bins = np.arange(0, n, 3)
    cur = ring[int(order[61])]
    cur_b = ob.clone()
    a.fork_bins(dst_bins, dst_bins, src_env=src_a, obs=cur, src_obs=sa)
    b.fork_bins(dst_bins, dst_bins, src_env=src_b, obs=cur_b, src_obs=sb)
    assert torch.equal(cur, cur_b)
    log.forget(int(order[61]))                               # (a registered buffer the caller's rows went into: invalidated)
    order[62] = order[61]                                    # straight into the buffer the rows were copied into
    play([(a, ring)], b, order, 40, log, seed + 3, cur_b, t0=62, tag="after fork")
    log.check()
    finish(a, b, src_a, src_b)


@EMITS
def test_set_heightmaps_under_registered_buffers(emit):
    """irbpp_set_heightmaps puts other heightmaps under the bins: the next observation has other row counts than the buffers hold."""
    n, seed = 34, 9
    a, b = twins("small", n, emit)
    ring = make_ring(a, 3)
    log = RunLog(S)
    ob = b.reset()
    assert torch.equal(a.reset(), ob)
    order = ring_order(seed, 90)
    ob, _ = play([(a, ring)], b, order, 40, log, seed, ob, tag="before")
    full_hm = b.get_heightmaps()
    empty = torch.zeros_like(full_hm)
    t0 = 40
    for part, hm in enumerate((empty, full_hm, empty)):
        a.set_heightmaps(hm)
        b.set_heightmaps(hm)
        ob, _ = play([(a, ring)], b, order, 15, log, seed + 1 + part, ob, t0=t0, tag=f"after set_heightmaps {part}")
        t0 += 15
    log.check()
    finish(a, b)


def test_unregister_free_and_allocate_again():
    """unregister, free, allocate: where the allocator hands the old address out again it is registered afresh (contents
    unknown); where it does not, the new tensor's registration is a first one.  Either way complete observations."""
    n, seed = 34, 10
    a, b = twins("blockout", n, _lib.TUNE_WAVE_EMIT)
    ring = make_ring(a, 3)
    log = RunLog(S)
    ob = b.reset()
    assert torch.equal(a.reset(), ob)
    order = ring_order(seed, 120)
    t0 = 0
    for part in range(4):
        ob, _ = play([(a, ring)], b, order, 30, log, seed + part, ob, t0=t0, tag=f"part {part}")
        t0 += 30
        if part == 3:
            break
        j = part % 3
        a.unregister_obs_buffer(ring[j])
        ring[j] = None
        torch.cuda.synchronize()
        fresh = torch.empty((n, a.loc_obs_len), dtype=torch.float32, device=DEV)       # (the caching allocator: usually the same block)
        fresh.copy_(poisoned(n, a.loc_obs_len, 20 + part))
        ring[j] = a.register_obs_buffer(fresh)
        log.forget(j)
    assert a.lib.irbpp_unregister_obs_buffer(a._h, _ptr(ob)) != 0                       # never registered
    log.check()
    finish(a, b)


@EMITS
def test_two_environments_register_halves_of_one_tensor(emit):
    """As GroupedPackingEnv does: two environments register t[:n] and t[n:] of the same tensors; each keeps counts of its own."""
    n, steps, seed = 34, 100, 11
    sh, seqs, kw = data("blockout")
    a = [GpuPackingEnv(sh, seqs, n, device=DEV, tuning=emit, global_offset=g * n, global_bins=2 * n, **kw) for g in range(2)]
    b = GpuPackingEnv(sh, seqs, 2 * n, device=DEV, tuning=emit, **kw)
    whole = [poisoned(2 * n, b.loc_obs_len, j) for j in range(3)]
    for t in whole:
        for g in range(2):
            a[g].register_obs_buffer(t[g * n:(g + 1) * n])
    log = RunLog(S)
    ob = b.reset()
    for g in range(2):
        assert torch.equal(a[g].reset(), ob[g * n:(g + 1) * n])
    orders = [ring_order(seed, steps), ring_order(seed + 1, steps)]          # the halves go their own ways through the ring
    logs = [RunLog(S), RunLog(S)]
    rng = np.random.default_rng(seed)
    for t in range(steps):
        act = torch.from_numpy(script_actions(ob.cpu().numpy(), t, S, rng)).to(DEV)
        rb = b.step(act)
        ib = b.step_info_host()
        for g in range(2):
            rows = slice(g * n, (g + 1) * n)
            u = int(orders[g][t])
            ra = a[g].step(act[rows].contiguous(), obs_out=whole[u][rows])
            assert torch.equal(ra[0], rb[0][rows]), f"step {t}, half {g}"
            assert torch.equal(ra[1], rb[1][rows]) and torch.equal(ra[2], rb[2][rows])
            ia = a[g].step_info_host()
            for key in ib:
                np.testing.assert_array_equal(ia[key], ib[key][rows], err_msg=f"{key}, step {t}, half {g}")
            logs[g].add(u, rb[0][rows], ib["done"][rows])
        ob = rb[0]
    for g in range(2):
        logs[g].check()
    finish(b, *a)


# -------------------------------------------------------------------------------------------------------------------
# GpuVecEnv: its own ring of registered buffers (obs_ring=3) against a fresh tensor per call (obs_ring=0)
# -------------------------------------------------------------------------------------------------------------------
def _same_vec_step(ra, rb, what):
    assert torch.equal(ra[0], rb[0]), f"{what}: observation"
    assert torch.equal(ra[1], rb[1]), f"{what}: reward"
    np.testing.assert_array_equal(ra[2], rb[2], err_msg=f"{what}: done")
    for ia, ib in zip(ra[3], rb[3]):
        ia, ib = dict(ia), dict(ib)
        for i in (ia, ib):
            if "episode" in i:
                i["episode"] = {k: v for k, v in i["episode"].items() if k != "t"}        # (wall-clock seconds)
        assert ia == ib, what


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("k", [1, 3], ids=["online", "buffered"])
def test_vec_env_ring_against_fresh_tensors(k, groups):
    """60 steps with auto-resets through reset, step, step_async(group=g) / step_wait(group=g) in alternating group order,
    reset_specific with its documented pattern (the rows copied into the held ring buffer), save_state / load_state and
    fork_bins from a second environment; every returned observation compared before the next call (the ring overwrites it
    three calls later).  Buffered: the location ring is the registered one.  (The ring order is the environment's own,
    round-robin -- three observations apart, still not the previous step's counts.)"""
    n, seed = 32, 12
    sh, seqs, kw = data("small")                            # (episodes of about 30 steps)
    kw = dict(kw, bufferSize=k)
    a = GpuVecEnv(sh, seqs, n, device=DEV, num_groups=groups, obs_ring=3, **kw)
    b = GpuVecEnv(sh, seqs, n, device=DEV, num_groups=groups, obs_ring=0, **kw)
    other = [GpuVecEnv(sh, seqs, n, device=DEV, num_groups=groups, obs_ring=0, traj_start=40, **kw) for _ in range(2)]
    for e in (a, b, *other):
        e.candidates_on_device = True
    assert len(a._ring) == 3 and len(a._loc_ring) == (3 if k > 1 else 0) and not b._ring
    log = RunLog(S)
    rng = np.random.default_rng(seed)
    ha, hb = a.reset(), b.reset()                           # the observations the callers hold
    assert torch.equal(ha, hb)
    src_obs = [e.reset() for e in other]
    blobs = last_done = None

    def sync():
        if groups > 1:
            a.env.synchronize()
            b.env.synchronize()

    for t in range(60):
        if t == 8:
            ha, hb = a.reset(), b.reset()
            assert torch.equal(ha, hb), "second reset"
            last_done = None
        if t in (12, 40):                                   # reset_specific: the rows go into the tensor the caller holds
            idx = list(range(t % 3, n, 3))
            rows_a, rows_b = a.reset_specific(idx), b.reset_specific(idx)
            assert torch.equal(rows_a, rows_b)
            ha[idx] = rows_a
            hb = hb.clone()
            hb[idx] = rows_b
            for u in range(3):
                log.forget(u)
        if t == 30:
            blobs = (a.save_state(ha), b.save_state(hb))
        if t == 45:
            ha, hb = a.load_state(blobs[0]), b.load_state(blobs[1])
            assert torch.equal(ha, hb), "load_state"
            last_done = None
        if t == 52:                                         # a third of the envs continue from the second environment's
            dst = np.arange(1, n, 3)
            a.env.fork_bins(dst, dst, src_env=other[0].env, obs=ha, src_obs=src_obs[0])
            b.env.fork_bins(dst, dst, src_env=other[1].env, obs=hb, src_obs=src_obs[1])
            sync()
            assert torch.equal(ha, hb), "fork_bins"
            for u in range(3):
                log.forget(u)
        if k > 1:
            slot = rng.integers(0, k, size=n).astype(np.int32)
            u = a._loc_turn
            la, lb = a.get_action_candidates(slot), b.get_action_candidates(slot)
            sync()
            assert torch.equal(la, lb), f"step {t}: location observation"
            assert la.data_ptr() == a._loc_ring[u].data_ptr()
            log.add(u, lb, last_done)             # (a location observation carries no done flag: the step's before it)
            act = script_actions(lb.cpu().numpy(), t, S, rng)
        else:
            act = script_actions(hb.cpu().numpy(), t, S, rng)
        if groups > 1 and t % 4 == 1:                       # one group at a time, in alternating order
            parts_a, parts_b, dones = [None] * groups, [None] * groups, [None] * groups
            for g in (range(groups) if t % 8 == 1 else reversed(range(groups))):
                rows = a.env.rows(g)
                a.step_async(act[rows], group=g)
                b.step_async(act[rows], group=g)
                ra, rb = a.step_wait(group=g), b.step_wait(group=g)
                _same_vec_step(ra, rb, f"step {t}, group {g}")
                parts_a[g], parts_b[g], dones[g] = ra[0], rb[0], rb[2]
            ha, hb = torch.cat(parts_a), torch.cat(parts_b)
            last_done = np.concatenate(dones)
        else:
            u = a._turn
            ra, rb = a.step(act), b.step(act)
            _same_vec_step(ra, rb, f"step {t}")
            assert ra[0].data_ptr() == a._ring[u].data_ptr()
            ha, hb = ra[0], rb[0]
            last_done = rb[2]
            if k == 1:
                log.add(u, hb, rb[2])
        for i, e in enumerate(other):                       # the second environment moves on by itself
            if k > 1:
                loc = e.get_action_candidates(np.zeros(n, dtype=np.int32))
                if groups > 1:
                    e.env.synchronize()                     # (policy_minz reads it on the caller's stream)
                src_obs[i] = e.step(e.env.policy_minz(loc).cpu().numpy())[0]
            else:
                src_obs[i] = e.step(e.env.policy_minz(src_obs[i]).cpu().numpy())[0]
    log.check()
    for e in (a, b, *other):
        e.env.check_device_error()
        e.close()
