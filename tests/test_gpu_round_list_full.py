"""A FULL list of polygon rounds on the device.  The trace kernel hands closed borders to the polygon kernel through eight
per-die lists (State::w_round / w_nround, Params::round_cap entries each).  A wave whose reservation does not fit approximates
its borders in place and writes empty records into the entries it reserved below the cap, a wave that starts past the cap
writes nothing, and the polygon kernel clamps every list to the cap.  At the default cap ((bins / 8 + 64) * 16) none of this
runs at test sizes, so every case here shrinks the cap with GpuPackingEnv.debug_round_cap -- to 1, 3 and 16, next to one
environment at the default cap as the in-run control -- and steps against the oracle: observations, policy_minz next actions,
reward, done and the step infos are byte-exact at every step, through auto-resets, in both round forms (dump, and
IRBPP_TUNE_TRACE_PACK's records).

That the lists really were full is asserted, not assumed.  After every checked observation debug_round_counts() gives the
eight reservation totals.  A round holds at most 64 * TRACE_P = 128 contour points, so a launch whose borders have `points`
points reserves at least lb = ceil(points / 128) rounds, and with eight lists lb > 8 * cap forces one of them past its cap.
`points` comes from the oracle alone (traced_points below): wherever lb > 8 * cap the test demands counts.max() > cap of the
device, and every case demands that its oracle run contains such observations for the caps PROVEN lists for it.  An empty
bin has one 4-point border per rotation, so the reset observation and the first steps of an episode can never be among them.
Every case is sized so that the oracle proves a full list at each of its caps, 16 included (lb > 128), in a stated number
of observations; the device's counts must show it there.

The totals are NOT equal between two environments that step the same actions: the die a wave runs on (a hardware register)
decides which list it joins, and which die a bin's workgroup ran on decides how its border starts fall into waves.  Asserted
instead: sum >= lb for every environment, and every shrunken environment's sum within SUM_TOLERANCE of the control's -- a
tolerance as OBSERVED (differences of up to 7 % of the control's sum on an MI355X, held to 12 %; profiles/round_list/README.md has the
figures of every case), not derived."""
import functools
import math

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from irbpp_amd.vec_env import GpuPackingEnv, GpuVecEnv
from oracle import contours as OC
from oracle.c_oracle import COracleVecEnv
from oracle.cvtools import find_out_contour
from helpers import minz_action
from test_gpu_round_dump import _actions, _f32, _snake_image, _unit_item_shapes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 500
PACK = _lib.TUNE_TRACE_PACK
FORMS = pytest.mark.parametrize("form", [0, PACK], ids=["dump", "pack"])
CAPS = (1, 3, 16)
ROUND_POINTS = 128               # 64 * TRACE_P (irbpp_device.h)
TRACE_CAP = 128                  # longer borders take the sequential redo and reserve nothing (irbpp_rounds.h)


def sum_tolerance(control_sum):
    """SUM_TOLERANCE: rounds by which an environment's total may differ from the control's (observed, see the module docstring)."""
    return max(4, math.ceil(0.12 * control_sum))


def default_cap(n):
    return (n // 8 + 64) * 16


def traced_points(posz, mask, aliased=True, res=0.01):
    """Contour points the trace kernel has to hand on for one bin's grids, counted from below with the oracle's own border
    following: per rotation and height level the outer borders of cvtools.convexHulls, without isolated pixels (the
    transition kernel answers those) and without borders of more than 128 points (sequential redo).  aliased: rotations
    with identical grids count once (the library traces a duplicate rotation once; identical grids are all it could merge)."""
    total, seen = 0, set()
    for r in range(len(posz)):
        key = (posz[r].tobytes(), mask[r].tobytes())
        if aliased and key in seen:
            continue
        seen.add(key)
        m = (posz[r] // res).astype(np.int32)
        m[mask[r] == 0] = -1
        for h in np.unique(m):
            if h == -1:
                continue
            cs, hier, _ = OC.find_contours(np.where(m == h, 255, 0).astype(np.uint8))
            outer, _ = find_out_contour(cs, hier[0])
            total += sum(len(c) for c in outer if 2 <= len(c) <= TRACE_CAP)
    return total


def lower_bound(points):
    return math.ceil(points / ROUND_POINTS)


class Fill(object):
    """The round counts of the shrunken environments (caps) and the control (last) over a run."""

    def __init__(self, caps, n):
        self.caps, self.n = caps, n
        self.proved = {c: 0 for c in caps}       # observations whose oracle point count forces a full list
        self.full = {c: 0 for c in caps}         # observations in which the device reported one
        self.bad = []

    def observe(self, envs, lb, what):
        counts = [e.debug_round_counts() for e in envs]
        print(f"{what}: lb {lb} control {counts[-1].tolist()} " + " ".join(f"cap{c} {k.tolist()}" for c, k in zip(self.caps, counts)))
        if counts[-1].max() > default_cap(self.n):
            self.bad.append(f"{what}: the control's own list is full {counts[-1].tolist()}")
        if counts[-1].sum() < lb:
            self.bad.append(f"{what}: {counts[-1].sum()} rounds reserved, the oracle's points need {lb}")
        for c, k in zip(self.caps, counts):
            if k.sum() < lb:
                self.bad.append(f"{what}: cap {c} reserved {k.sum()} rounds, the oracle's points need {lb}")
            if abs(int(k.sum()) - int(counts[-1].sum())) > sum_tolerance(int(counts[-1].sum())):
                self.bad.append(f"{what}: cap {c} reserved {k.sum()} rounds, the control {counts[-1].sum()}")
            if lb > 8 * c:
                self.proved[c] += 1
                if not k.max() > c:
                    self.bad.append(f"{what}: cap {c}, lb {lb} > {8 * c} but counts {k.tolist()}")
            self.full[c] += int(k.max() > c)

    def check(self, at_least, seen=()):
        """at_least[cap]: in how many observations the oracle run must force a full list of that cap (every cap of the run has
        an entry; the device's counts were held to each of them in observe).  seen: caps whose full list must show in the
        device's counts in some observation, where the oracle's points cannot force it."""
        assert not self.bad, "\n".join(self.bad)
        for c in self.caps:
            assert self.proved[c] >= at_least[c], f"cap {c}: the oracle run forces a full list in {self.proved[c]} observations only"
            assert self.full[c] >= self.proved[c]
            assert c not in seen or self.full[c] >= 1, f"cap {c}: no observation of the run filled a list"


# ---- online environments against the C oracle ------------------------------------------------------------------------
def _blockout70():
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.04, seed=3)
    return sh, synthetic.make_sequences(sh.n_shapes, 70, 60, seed=17), 70, 20, 99, {}


def _blockout128():
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.04, seed=3)
    return sh, synthetic.make_sequences(sh.n_shapes, 128, 60, seed=17), 128, 16, 99, {}


def _speckled96():
    sh = synthetic.general_shapes(n_shapes=16, n_rot=8, seed=1)
    return sh, synthetic.make_sequences(sh.n_shapes, 96, 60, seed=9), 96, 8, 13, {}


def _blockout8():
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=8, cube=0.04, seed=3)
    return sh, synthetic.make_sequences(sh.n_shapes, 64, 60, seed=17), 8, 20, 37, {}


SCENARIOS = {"blockout70": _blockout70, "blockout128": _blockout128, "speckled96": _speckled96, "blockout8": _blockout8}


@functools.lru_cache(maxsize=None)
def oracle_run(name, aliased=True, listed_reset=None):
    """The oracle's side of a scenario, computed once and shared by every case that steps it: per observation the float32
    rows and the lower bound of its rounds, per step the actions, rewards and dones.  listed_reset = (step, bins): those bins
    are reset by list after that step."""
    sh, seqs, n, steps, seed, kw = SCENARIOS[name]()
    cenv = COracleVecEnv(n, sh, seqs, threads=16, **kw)
    bound = lambda: lower_bound(sum(traced_points(*e.grids(), aliased=aliased) for e in cenv.envs))   # noqa: E731
    obs, lbs, acts, rews, dones, raw, subs, ends = [_f32(cenv.reset())], [], [], [], [], {}, {}, []
    lbs.append(bound())
    rng = np.random.RandomState(seed)
    for t in range(steps):
        acts.append(_actions(obs[-1], t, rng))
        o, r, d, infos = cenv.step(acts[-1])
        o = _f32(o)
        ends.append({b: (i["counter"], i["ratio"]) for b, i in enumerate(infos) if d[b]})
        lbs.append(bound())
        if listed_reset is not None and listed_reset[0] == t:        # obs[t + 1]: the rows the next actions are drawn from
            raw[t], subs[t] = o, _f32(cenv.reset_specific(list(listed_reset[1])))
            o = o.copy()
            o[list(listed_reset[1])] = subs[t]
        obs.append(o)
        rews.append(r.astype(np.float32))
        dones.append(d)
    for a in obs + acts + rews + dones + list(subs.values()) + list(raw.values()):
        a.setflags(write=False)
    assert sum(int(d.sum()) for d in dones) > 0, "no episode ended: the run has no auto-reset"
    return dict(shapes=sh, seqs=seqs, n=n, obs=obs, lb=lbs, act=acts, rew=rews, done=dones, raw=raw, sub=subs, end=ends, kw=kw,
                minz=[np.array([minz_action(row, S) for row in o], dtype=np.int32) for o in obs])


def _open(ref, tuning, caps):
    envs = []
    for cap in tuple(caps) + (None,):
        e = GpuPackingEnv(ref["shapes"], ref["seqs"], ref["n"], device=DEV, tuning=tuning, **ref["kw"])
        if cap is not None:
            e.debug_round_cap(cap)
        assert e.debug_round_counts().tolist() == [0] * 8                   # (the first call switches the recording on)
        envs.append(e)
    assert all("irbpp_trace_kernel" in e.kernel_info()[1] and "irbpp_polygon_kernel" in e.kernel_info()[1] for e in envs)
    return envs


def _step_all(ref, tuning, at_least, listed_reset=None, fixed_buffers=False):
    caps = tuple(at_least)
    n = ref["n"]
    envs = _open(ref, tuning, caps)
    fill = Fill(caps, n)
    obs = [e.reset() for e in envs]
    for o in obs:
        np.testing.assert_array_equal(o.cpu().numpy(), ref["obs"][0], err_msg="reset observation")
    fill.observe(envs, ref["lb"][0], "reset")
    bufs = [[torch.empty((n, e.obs_len), dtype=torch.float32, device=DEV) for _ in range(2)] for e in envs]
    dacts = [torch.empty((n,), dtype=torch.int32, device=DEV) for _ in envs]
    for t, act in enumerate(ref["act"]):
        nxt = [e.policy_minz(o) for e, o in zip(envs, obs)]
        for x in nxt:
            np.testing.assert_array_equal(x.cpu().numpy(), ref["minz"][t], err_msg=f"next action, step {t}")
        for d in dacts:
            d.copy_(torch.from_numpy(act))
        res = [e.step(d, obs_out=b[t & 1] if fixed_buffers else None) for e, d, b in zip(envs, dacts, bufs)]
        info = [e.step_info_host() for e in envs]
        want = ref["raw"].get(t, ref["obs"][t + 1])
        for r, i in zip(res, info):
            np.testing.assert_array_equal(r[0].cpu().numpy(), want, err_msg=f"observation, step {t}")
            np.testing.assert_array_equal(i["done"], ref["done"][t], err_msg=f"done, step {t}")
            np.testing.assert_array_equal(i["reward"].astype(np.float32), ref["rew"][t], err_msg=f"reward, step {t}")
            for b, (counter, ratio) in ref["end"][t].items():
                assert i["counter"][b] == counter and i["ratio"][b] == ratio, f"episode info of bin {b}, step {t}"
            for key in info[-1]:
                np.testing.assert_array_equal(i[key], info[-1][key], err_msg=f"{key}, step {t}")
        fill.observe(envs, ref["lb"][t + 1], f"step {t}")
        obs = [r[0] for r in res]
        if listed_reset is not None and listed_reset[0] == t:
            bins = torch.tensor(list(listed_reset[1]), dtype=torch.int32, device=DEV)
            obs = [o.clone() for o in obs]
            for e, o in zip(envs, obs):
                sub = e.reset_bins(bins)
                np.testing.assert_array_equal(sub.cpu().numpy(), ref["sub"][t], err_msg="listed reset")
                o[bins.long()] = sub
                np.testing.assert_array_equal(o.cpu().numpy(), ref["obs"][t + 1])
    for e in envs:
        e.check_device_error()
        e.close()
    fill.check(at_least)


# 128 bins (24 shapes x 4 rotations): several bins per chunk, more than one chunk per die, 32 starts per wave by default.  70 bins
# of this data fill lists of 1 and 3 but peak at 16 rounds on a die, one short of a full list of 16; 128 bins have the points
# that force it: lb > 24 from the first step on and lb > 128 in three observations (the oracle run: 6 at the reset, 33, 53, 72 ... 134, 125, 131, 133).
@FORMS
@pytest.mark.parametrize("launch", [0, _lib.TUNE_TRACE_CPW64, _lib.TUNE_TRACE_CPW16], ids=["cpw32", "cpw64", "cpw16"])
def test_blockout_full_lists(launch, form):
    _step_all(oracle_run("blockout128"), launch | form, at_least={1: 16, 3: 16, 16: 3})


# Speckled level images (16 free-form shapes x 8 rotations): hundreds of border starts per bin, so waves stride over later
# chunks (record form after a dump); TRACE_REFILL is the second copy of the list code.  Five bins have at most ~1300 border
# points (lb <= 11) and 18 rounds in all, so this runs 96 bins -- which is past the 64 bins from which the emit kernel serves
# heavy bins first (the 5-bin size had that off; the trace and polygon kernels do not depend on it): 96 bins have lb > 24 in every observation after the reset and lb > 128 in the first two (176, 162).
@FORMS
@pytest.mark.parametrize("launch", [0, _lib.TUNE_TRACE_CPW64, _lib.TUNE_TRACE_REFILL], ids=["default", "cpw64", "refill"])
def test_speckled_full_lists(launch, form):
    _step_all(oracle_run("speckled96"), launch | form, at_least={1: 8, 3: 8, 16: 2})


@FORMS
def test_listed_reset_of_three_bins_under_cap_1(form):
    """reset_bins of three bins mid-episode (a launch over three launch slots into lists that the step before it filled)."""
    _step_all(oracle_run("blockout70", listed_reset=(9, (3, 40, 69))), form, at_least={1: 15}, listed_reset=(9, (3, 40, 69)))


@FORMS
@pytest.mark.parametrize("graph", [0, _lib.TUNE_GRAPH], ids=["direct", "graph"])
def test_graph_holds_the_shrunken_cap(graph, form):
    """A captured graph holds Params by value: the cap set before the first launch is the one its trace and polygon nodes run
    with (replays from the third step on: fixed observation and action buffers).  BlockOut at eight rotations, every rotation
    traced (IRBPP_TUNE_NO_ROT_ALIAS), so that eight bins have the points that force a full list at cap 3."""
    _step_all(oracle_run("blockout8", aliased=False), graph | form | _lib.TUNE_NO_ROT_ALIAS, at_least={3: 3}, fixed_buffers=True)


# ---- buffered environment, level images dialled in through the heightmap ----------------------------------------------
@FORMS
def test_dialled_images_long_borders_in_full_lists(form):
    """The recipe of test_gpu_round_dump.test_long_borders_spill_bytes_and_a_border_alone_in_its_round (k = 2, MODE_CANDS
    launches) under caps 1, 3 and 16: snakes of 61 / 92 / 123 border points, whose spill bytes an inline wave reads itself, the
    5-zigzag snake of more than 128 points (sequential redo), speckle.  The unit item at eight rotations with every rotation
    traced (IRBPP_TUNE_NO_ROT_ALIAS): six bins then carry eight times the points of their images.  Every other round is LIGHT:
    one speckled bin beside five flat ones (one rectangle per rotation), so that short lists follow full ones over the same
    entries (the trace waves of a launch spread over the dies whatever the bins hold: 1 ... 5 rounds a die after 6 ... 21).
  Six bins of 16 x 16 images cannot
    carry the 16 384 points that prove a full list of 16: that cap is held to the device's own counts, once in the run."""
    from oracle.packing import OracleVecEnv
    sh = _unit_item_shapes(n_rot=8)
    seqs = np.zeros((8, 40), dtype=np.int32)
    n, k = 6, 2
    genvs = [GpuVecEnv(sh, seqs, n, device=DEV, bufferSize=k, tuning=form | _lib.TUNE_NO_ROT_ALIAS) for _ in CAPS + (None,)]
    for g, cap in zip(genvs, CAPS):
        g.env.debug_round_cap(cap)
    for g in genvs:
        g.candidates_on_device = True
        assert g.env.debug_round_counts().tolist() == [0] * 8               # (the first call switches the recording on)
    oenv = OracleVecEnv(n, sh, seqs, bufferSize=k)
    want0 = _f32(oenv.reset())
    for g in genvs:
        np.testing.assert_array_equal(g.reset().cpu().numpy(), want0)
    fill = Fill(CAPS, n)
    big = _snake_image(5)
    outer = [c for c, hole in zip(*(lambda r: (r[0], r[2]))(OC.find_contours(big.astype(np.uint8)))) if not hole]
    assert len(outer) == 1 and len(outer[0]) > TRACE_CAP
    mids = [_snake_image(z) for z in (2, 3, 4)]
    rng = np.random.RandomState(12)
    ndone = 0
    for t in range(8):
        imgs = []
        for i in range(n):
            kind = (t + i) % 3
            if kind == 0:
                m = big if (t + i) % 4 == 0 else mids[(t + i // 3) % 3]
                imgs.append(m if i % 2 == 0 else m.T.copy())
            elif kind == 1:
                imgs.append(rng.rand(16, 16) < rng.uniform(0.3, 0.7))
            else:
                imgs.append(np.kron(rng.rand(4, 4) < 0.5, np.ones((4, 4), dtype=bool)) ^ (rng.rand(16, 16) < 0.05))
        if t % 2 == 1:                                                      # a light round
            imgs = [rng.rand(16, 16) < 0.5 if i == t % n else np.ones((16, 16), dtype=bool) for i in range(n)]
        hm = np.zeros((n, 32, 32))
        for i, im in enumerate(imgs):                                       # image pixel (x, y) = action cell (row y, col x)
            lv = np.where(im, 0.05, 0.11) + rng.randint(0, 2, size=(16, 16)) * np.where(im, 0.0, 0.03)
            hm[i] = np.kron(lv, np.ones((2, 2)))
        if t in (3, 6):
            hm[(t + 1) % n] = 0.29                                             # no room for the item anywhere: this bin's episode ends
        for i in range(n):
            oenv.envs[i].space.heightmapC[:] = hm[i]
        oa = np.array([t % k] * n)
        oloc = _f32(oenv.get_action_candidates(oa))
        lb = lower_bound(sum(traced_points(e.space.posZValid, e.space.naiveMask, aliased=False) for e in oenv.envs))
        act = np.array([int(np.argmin(np.where(c.reshape(S, 5)[:, 4] == 1, c.reshape(S, 5)[:, 3], np.inf)))
                        if (c.reshape(S, 5)[:, 4] == 1).any() else 0 for c in oloc[:, :5 * S]])
        oord, orew, odone, _ = oenv.step(act)
        ndone += int(odone.sum())
        for g in genvs:
            g.env.set_heightmaps(torch.from_numpy(hm).to(DEV))
            np.testing.assert_array_equal(g.get_action_candidates(oa).cpu().numpy(), oloc, err_msg=f"round {t}")
        fill.observe([g.env for g in genvs], lb, f"round {t}")
        for g in genvs:
            gord, grew, gdone, _ = g.step(act)
            np.testing.assert_array_equal(gord.cpu().numpy(), _f32(oord))
            np.testing.assert_array_equal(gdone, odone)
            np.testing.assert_array_equal(grew.numpy().reshape(-1).astype(np.float32), np.asarray(orew, dtype=np.float32))
    assert ndone > 0
    for g in genvs:
        g.env.check_device_error()
        g.close()
    fill.check({1: 8, 3: 4, 16: 0}, seen=(16,))


@FORMS
def test_one_long_list_beside_empty_ones_over_stale_records(form):
    """The consumer's clamp.  A trace wave takes one chunk of up to 32 border starts of one die's candidate list and its rounds
    join the list of the die it runs on, so a launch with fewer than eight chunks leaves whole lists at 0 while their entries
    still hold the records of an earlier observation.  The unit item's rotations are duplicates (one traced image per bin), so
    six bins make at most six chunks.  MEDIUM rounds: six blocky images of at most 128 border points -- one chunk and ONE
    round per bin, which fits a list of cap 1 exactly and leaves a real record in its entry.  LIGHT rounds: one bin with the
    123-point snake on a plain background (two borders that cannot share a round: one chunk, two rounds), five bins whose
    valid cells are isolated pixels (answered by the transition kernel: no chunk at all).  Asserted from debug_round_counts at
    cap 1: the only list in use holds more than the cap, its neighbour is at 0 now and held one round in the medium round
    before.  A polygon kernel that read a list to its count, not to the cap, would walk into that neighbour's stale record
    and set the vertices of a blocky image in a bin of isolated pixels."""
    from oracle.packing import OracleVecEnv
    caps = (1, 3)
    sh = _unit_item_shapes(n_rot=8)
    seqs = np.zeros((8, 40), dtype=np.int32)
    n, k = 6, 2
    genvs = [GpuVecEnv(sh, seqs, n, device=DEV, bufferSize=k, tuning=form) for _ in caps + (None,)]
    for g, cap in zip(genvs, caps):
        g.env.debug_round_cap(cap)
    for g in genvs:
        g.candidates_on_device = True
        assert g.env.debug_round_counts().tolist() == [0] * 8               # (the first call switches the recording on)
    oenv = OracleVecEnv(n, sh, seqs, bufferSize=k)
    want0 = _f32(oenv.reset())
    for g in genvs:
        np.testing.assert_array_equal(g.reset().cpu().numpy(), want0)
    fill = Fill(caps, n)
    snake = _snake_image(4)
    dots = np.full((16, 16), 0.29)
    dots[::2, ::2] = 0.05                                                   # 64 valid cells, none next to another
    rng = np.random.RandomState(21)
    past_a_stale_record, before = 0, None
    for t in range(10):
        light = t % 2 == 1
        hm = np.zeros((n, 32, 32))
        for i in range(n):
            if not light:
                lv = np.where(np.kron(rng.rand(4, 4) < 0.5, np.ones((4, 4), dtype=bool)), 0.05, 0.11)
            elif i == (t // 2) % n:
                lv = np.where(snake if t % 4 == 1 else snake.T, 0.05, 0.11)
            else:
                lv = dots
            hm[i] = np.kron(lv, np.ones((2, 2)))
        for i in range(n):
            oenv.envs[i].space.heightmapC[:] = hm[i]
        oa = np.array([t % k] * n)
        oloc = _f32(oenv.get_action_candidates(oa))
        points = [traced_points(e.space.posZValid, e.space.naiveMask) for e in oenv.envs]
        if light:
            assert sorted(points) == [0] * (n - 1) + [123 + 35], points      # two borders, more than one round's points
        else:
            assert 0 < min(points) and max(points) <= ROUND_POINTS, points  # one round per bin
        act = np.array([minz_action(c, S) for c in oloc])
        oord, orew, odone, _ = oenv.step(act)
        for g in genvs:
            g.env.set_heightmaps(torch.from_numpy(hm).to(DEV))
            np.testing.assert_array_equal(g.get_action_candidates(oa).cpu().numpy(), oloc, err_msg=f"round {t}")
        fill.observe([g.env for g in genvs], lower_bound(sum(points)), f"round {t}")
        c1 = genvs[0].env.debug_round_counts()
        if light:
            assert sorted(c1.tolist()) == [0] * 7 + [2], f"round {t}: {c1.tolist()}"
            d = int(c1.argmax())
            past_a_stale_record += int(d < 7 and before[d + 1] == 1)
        else:
            assert c1.max() == 1 and c1.sum() == n, f"round {t}: {c1.tolist()}"
            before = c1
        for g in genvs:
            gord, grew, gdone, _ = g.step(act)
            np.testing.assert_array_equal(gord.cpu().numpy(), _f32(oord))
            np.testing.assert_array_equal(gdone, odone)
            np.testing.assert_array_equal(grew.numpy().reshape(-1).astype(np.float32), np.asarray(orew, dtype=np.float32))
    for g in genvs:
        g.env.check_device_error()
        g.close()
    fill.check({1: 0, 3: 0})
    assert past_a_stale_record >= 3, f"the full list had a stale record behind it in {past_a_stale_record} of 5 light rounds"


# ---- the entry point's refusals ---------------------------------------------------------------------------------------
def test_refusals_leave_the_environment_usable():
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.04, seed=3)
    seqs = synthetic.make_sequences(sh.n_shapes, 64, 60, seed=17)
    n = 8
    env = GpuPackingEnv(sh, seqs, n, device=DEV)
    lib, h = env.lib, env._h
    assert lib.irbpp_debug_round_cap(h, 0) == -1                            # IRBPP_ERR_ARG
    assert lib.irbpp_debug_round_cap(h, -5) == -1
    assert lib.irbpp_debug_round_cap(h, default_cap(n) + 1) == -1
    assert lib.irbpp_debug_round_cap(None, 1) == -1
    assert lib.irbpp_debug_round_cap(h, default_cap(n)) == 0                # the default itself, and a smaller one after it
    assert lib.irbpp_debug_round_cap(h, 2) == 0
    with pytest.raises(_lib.IrbppError, match="argument"):
        env.debug_round_cap(0)
    assert env.debug_round_counts().tolist() == [0] * 8
    cenv = COracleVecEnv(n, sh, seqs)
    obs, oobs = env.reset(), _f32(cenv.reset())
    np.testing.assert_array_equal(obs.cpu().numpy(), oobs)
    assert lib.irbpp_debug_round_cap(h, 1) == -3                            # IRBPP_ERR_STATE: a transition has been launched
    with pytest.raises(_lib.IrbppError, match="order"):
        env.debug_round_cap(1)
    rng = np.random.RandomState(4)
    for t in range(4):                                                      # ... and the environment goes on, at cap 2
        act = _actions(oobs, t, rng)
        obs = env.step(torch.from_numpy(act).to(DEV))[0]
        oobs = _f32(cenv.step(act)[0])
        np.testing.assert_array_equal(obs.cpu().numpy(), oobs, err_msg=f"step {t}")
    assert env.debug_round_counts().sum() > 0
    env.check_device_error()
    env.close()
    wide = GpuPackingEnv(sh, seqs, 2, device=DEV, resolutionA=0.01)         # 32 x 32 action cells: the wide path has no lists
    assert "irbpp_trace_kernel" not in wide.kernel_info()[1]
    assert wide.lib.irbpp_debug_round_cap(wide._h, 1) == -1
    out = (np.zeros(8, dtype=np.int32))
    assert wide.lib.irbpp_debug_round_counts(wide._h, out.ctypes.data_as(_lib.c_i32_p), None) == -1
    wcenv = COracleVecEnv(2, sh, seqs, resolutionA=0.01)
    np.testing.assert_array_equal(wide.reset().cpu().numpy(), _f32(wcenv.reset()))
    wide.check_device_error()
    wide.close()
