"""irbpp_step_cells / irbpp_heuristic_step on the MI355X against the numpy oracle (cell_step_helpers.OracleCellEnv: PackingGame.step
with ``candidates`` overwritten by the cell) and against irbpp_step itself.  Every comparison is bit-exact: float32 observations,
float64 heightmaps, rewards, dones, counters, ratios, the episode's r / l.  Each test also asserts the conditions that keep it from
passing vacuously (cells outside the candidate rows, refusals, finished episodes, the all-invalid case)."""
import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib
from irbpp_amd.evaluate import evaluate, rotation_quaternion_xyzw
from irbpp_amd.vec_env import GpuPackingEnv, GpuVecEnv, GroupedPackingEnv
from cell_step_helpers import OracleCellEnv, f32, mix_cells, scenario

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 500
eq = np.testing.assert_array_equal


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _check_step(h, gobs, ghm, oenv, oobs, orew, odone, oinfo, gbins, msg):
    """GPU bins `gbins` (one per oracle env, in order) against the oracle's step outputs."""
    eq(gobs[gbins], f32(oobs), err_msg=msg)
    eq(h["reward"][gbins], orew, err_msg=msg)
    eq(h["done"][gbins], odone, err_msg=msg)
    eq(ghm[gbins], oenv.heightmaps(), err_msg=msg)
    for j, b in enumerate(gbins):
        if odone[j]:
            assert h["counter"][b] == oinfo[j]["counter"] and h["ratio"][b] == oinfo[j]["ratio"], msg
            assert h["ep_reward"][b] == oinfo[j]["episode"]["raw"] and h["ep_len"][b] == oinfo[j]["episode"]["l"], msg


# -- 1. step_cells against the oracle helper ----------------------------------------------------------------------------------------
SETS = ["lattice", "box", "free_form", "r8", "hm64"]


@pytest.mark.parametrize("name", SETS)
def test_step_cells_matches_oracle_small(name):
    """N = 4 through GpuVecEnv.step_cells: cells from the oracle's get_heuristic_action (DBLF, flip 3), every fifth placement a
    uniformly drawn cell (seed 7)."""
    sh, seqs, kw = scenario(name)
    n, steps = 4, (12 if name == "hm64" else 25)
    genv = GpuVecEnv(sh, seqs, n, device=DEV, **kw)
    oenv = OracleCellEnv(range(n), n, sh, seqs, **kw)
    eq(genv.reset().cpu().numpy(), f32(oenv.reset()))
    rng = np.random.RandomState(7)
    for t in range(steps):
        cells = mix_cells(oenv.heuristic_cells("DBLF", 3), t, rng, sh.n_rot, genv.env.Ax, genv.env.Ay)
        gobs, grew, gdone, ginfo = genv.step_cells(cells)
        oobs, orew, odone, oinfo = oenv.step_cells(cells)
        eq(gobs.cpu().numpy(), f32(oobs), err_msg=f"{name} step {t}")
        eq(grew.numpy()[:, 0], orew.astype(np.float32))
        eq(gdone, odone)
        eq(genv.env.get_heightmaps().cpu().numpy(), oenv.heightmaps())
        for i in range(n):
            if odone[i]:
                assert ginfo[i]["counter"] == oinfo[i]["counter"] and ginfo[i]["ratio"] == oinfo[i]["ratio"]
                assert ginfo[i]["episode"]["r"] == oinfo[i]["episode"]["r"] and ginfo[i]["episode"]["l"] == oinfo[i]["episode"]["l"]
    genv.env.check_device_error()
    genv.close()
    # the drawn cells did what they are there for: cells outside naiveMask, the footprint-overhang prejudge, refusals
    assert oenv.off_rows >= 1 and oenv.outside_mask >= 1 and oenv.overhang >= 1 and oenv.episodes >= 1, \
        (oenv.off_rows, oenv.outside_mask, oenv.overhang, oenv.episodes)


@pytest.mark.parametrize("name", SETS)
def test_step_cells_matches_oracle_2048_bins(name):
    """N = 2048 over 64 trajectories.  Oracle sample: the 64 bins 0 .. 31 and 2016 .. 2047 (first and last included), one
    PackingGame each; bin b plays trajectory (1 + b) % 64 in every episode (2048 is a multiple of 64), so the 64 sampled bins
    play 64 DIFFERENT trajectories and get different cells.  A bin outside the sample is handed the cells of the sampled bin
    with its trajectory and must equal that bin in every output; every bin with a cell of its own is comparison 2's
    (test_step_cells_on_row_cells_equals_step)."""
    sh, seqs, kw = scenario(name, n_traj=64)
    n, cls = 2048, 64
    steps = 6 if name == "hm64" else (8 if name == "r8" else 12)
    genv = GpuPackingEnv(sh, seqs, n, device=DEV, **kw)
    sample = np.r_[0:32, n - 32:n]
    oenv = OracleCellEnv(sample, n, sh, seqs, **kw)
    assert sorted((1 + sample) % cls) == list(range(cls))
    pos = np.empty(cls, dtype=np.int64)                 # trajectory -> its bin's position in the sample
    pos[(1 + sample) % cls] = np.arange(cls)
    of = pos[(1 + np.arange(n)) % cls]                  # bin -> position in the sample of the bin it copies (itself, if sampled)
    assert (of[sample] == np.arange(cls)).all()
    eq(genv.reset().cpu().numpy()[sample], f32(oenv.reset()))
    rng = np.random.RandomState(7)
    for t in range(steps):
        cells = mix_cells(oenv.heuristic_cells("DBLF", 3), t, rng, sh.n_rot, genv.Ax, genv.Ay)
        gobs, _, _ = genv.step_cells(_dev(cells[of]))
        h = genv.step_info_host()
        gobs, ghm = gobs.cpu().numpy(), genv.get_heightmaps().cpu().numpy()
        oobs, orew, odone, oinfo = oenv.step_cells(cells)
        _check_step(h, gobs, ghm, oenv, oobs, orew, odone, oinfo, sample, f"{name} step {t}")
        twin = sample[of]
        eq(gobs, gobs[twin])
        eq(ghm, ghm[twin])
        for k in ("reward", "done", "ep_len"):
            eq(h[k], h[k][twin])
        for k in ("counter", "ratio", "ep_reward"):
            eq(h[k][h["done"]], h[k][twin][h["done"]])
    genv.check_device_error()
    genv.close()
    assert len({seqs[(1 + b) % cls].tobytes() for b in sample}) == cls      # (the sampled bins play different item sequences)
    assert oenv.off_rows >= 1 and oenv.outside_mask >= 1 and oenv.overhang >= 1 and oenv.episodes >= 1, \
        (oenv.off_rows, oenv.outside_mask, oenv.overhang, oenv.episodes)


# -- 2. step_cells(cell of candidate row a) == step(a) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,k,tuning", [("lattice", 2048, 1, 0), ("box", 2048, 1, 0), ("free_form", 2048, 1, 0), ("r8", 2048, 1, 0),
                                             ("hm64", 2048, 1, 0), ("lattice", 8192, 1, 0), ("lattice", 1024, 3, 0), ("lattice", 4096, 3, 0),
                                             ("wide32", 256, 1, 0), ("levels60", 512, 3, 0),
                                             ("lattice", 2048, 1, _lib.TUNE_GRAPH)])
def test_step_cells_on_row_cells_equals_step(name, n, k, tuning):
    """Two environments side by side over whole episodes: A steps candidate row a (the scripted MINZ policy; every fifth step a
    uniformly drawn row, zero-padded rows included), B is handed the (rot, lx, ly) of that row of its own observation.  Every bin,
    every output, the heightmaps."""
    sh, seqs, kw = scenario(name, n_traj=64)
    kw = dict(kw, bufferSize=k, tuning=tuning)
    a_env, b_env = GpuPackingEnv(sh, seqs, n, device=DEV, **kw), GpuPackingEnv(sh, seqs, n, device=DEV, **kw)
    oa_, ob_ = a_env.reset(), b_env.reset()
    eq(oa_.cpu().numpy(), ob_.cpu().numpy())
    gen = torch.Generator(device="cpu").manual_seed(3)
    steps = 20 if name in ("hm64", "wide32") else 40
    dones = 0
    for t in range(steps):
        if k > 1:
            slot = _dev((np.arange(n) + t) % k)
            la, lb = a_env.get_action_candidates(slot), b_env.get_action_candidates(slot)
            eq(la.cpu().numpy(), lb.cpu().numpy())
        else:
            la, lb = oa_, ob_
        act = a_env.policy_minz(la)
        if t % 5 == 4:
            act = torch.randint(0, S, (n,), generator=gen, dtype=torch.int32).to(DEV)
        rows = lb[:, :5 * S].reshape(n, S, 5)
        cells = rows[torch.arange(n, device=DEV), act.long(), :3].to(torch.int32).contiguous()
        oa_, ra, da = a_env.step(act)
        ob_, rb, db = b_env.step_cells(cells)
        ha, hb = a_env.step_info_host(), b_env.step_info_host()
        eq(oa_.cpu().numpy(), ob_.cpu().numpy(), err_msg=f"{name} step {t}")
        for key in ("reward", "done", "ep_len", "stable"):
            eq(ha[key], hb[key], err_msg=key)
        for key in ("counter", "ratio", "ep_reward"):
            eq(ha[key][ha["done"]], hb[key][hb["done"]], err_msg=key)
        dones += int(ha["done"].sum())
        if t % 5 == 4 or t == steps - 1:
            eq(a_env.get_heightmaps().cpu().numpy(), b_env.get_heightmaps().cpu().numpy())
    eq(a_env.episode_totals().cpu().numpy(), b_env.episode_totals().cpu().numpy())
    a_env.close()
    b_env.close()
    assert dones >= 1, dones            # (an auto-reset was among the steps compared)


# -- 3. heuristic_step == heuristic_action + step_cells == oracle ------------------------------------------------------------------------
def _heuristic_run(name, method, dir_idx, n, steps, two_step=True, k=1):
    sh, seqs, kw = scenario(name, length=80 if name in ("free_form", "wide32") else 120)
    kw = dict(kw, bufferSize=k)
    envs = [GpuPackingEnv(sh, seqs, n, device=DEV, **kw)]
    pair = GpuPackingEnv(sh, seqs, n, device=DEV, **kw) if two_step else None           # heuristic_action, then step_cells
    oenv = OracleCellEnv(range(n), n, sh, seqs, **kw)
    oobs = f32(oenv.reset())
    for e in envs + ([pair] if pair else []):
        eq(e.reset().cpu().numpy(), oobs)
    for t in range(steps):
        if k > 1:
            slot = (np.arange(n) + 2 * t + 1) % k
            oloc = f32(oenv.get_action_candidates(slot))
            for e in envs + ([pair] if pair else []):
                eq(e.get_action_candidates(_dev(slot)).cpu().numpy(), oloc)
        cells = oenv.heuristic_cells(method, dir_idx)
        oobs, orew, odone, oinfo = oenv.step_cells(cells)
        if pair is not None:
            gc = pair.heuristic_action(method, dir_idx)
            eq(gc.cpu().numpy(), cells, err_msg=f"{name} {method} {dir_idx} step {t}")
            gobs, _, _ = pair.step_cells(gc)
            _check_step(pair.step_info_host(), gobs.cpu().numpy(), pair.get_heightmaps().cpu().numpy(), oenv, oobs, orew, odone, oinfo,
                        np.arange(n), f"pair {name} {method} {dir_idx} step {t}")
        for i, e in enumerate(envs):
            gobs, _, _ = e.heuristic_step(method, dir_idx)
            _check_step(e.step_info_host(), gobs.cpu().numpy(), e.get_heightmaps().cpu().numpy(), oenv, oobs, orew, odone, oinfo,
                        np.arange(n), f"env {i} {name} {method} {dir_idx} step {t}")
    for e in envs + ([pair] if pair else []):
        e.check_device_error()
        e.close()
    # in EVERY heuristic run the chosen cell is absent from the valid candidate rows at least once: irbpp_step could not have
    # played it (the oracle alone decides this; 12 placements of 3 bins are enough on every set used here)
    assert oenv.off_rows >= 1, (name, method, dir_idx, oenv.off_rows)
    return oenv


@pytest.mark.parametrize("method", ["MINZ", "DBLF", "FIRSTFIT", "HM"])
@pytest.mark.parametrize("dir_idx", [0, 1, 2, 3])
def test_heuristic_step_16x16_all_methods_and_flips(method, dir_idx):
    oenv = _heuristic_run("lattice04", method, dir_idx, 3, 12)
    assert oenv.in_rows + oenv.off_rows == 36


@pytest.mark.parametrize("method,dir_idx", [("DBLF", 3), ("MINZ", 1)])
def test_heuristic_step_free_form_whole_episodes(method, dir_idx):
    """The issue's free-form probe: 3 bins, 40 placements: cells outside the candidate rows, at least 2 finished episodes and
    the all-invalid argmin (0, 0, 0) followed by a refusal."""
    oenv = _heuristic_run("free_form", method, dir_idx, 3, 40)
    assert oenv.off_rows >= 1 and oenv.episodes >= 2 and oenv.all_invalid >= 1, (oenv.off_rows, oenv.episodes, oenv.all_invalid)


@pytest.mark.parametrize("method", ["MINZ", "DBLF", "FIRSTFIT", "HM"])
def test_heuristic_step_blockout_leaves_the_candidate_rows(method):
    """The issue's BlockOut probe (3 bins, 60 placements, flip 0): it found 7 of 180 off the rows at the lowest (MINZ)."""
    oenv = _heuristic_run("lattice04", method, 0, 3, 60, two_step=False)
    assert oenv.off_rows >= 7, oenv.off_rows


@pytest.mark.parametrize("method,dir_idx", [("MINZ", 1), ("DBLF", 3), ("FIRSTFIT", 2)])
def test_heuristic_step_32x32_cells(method, dir_idx):
    oenv = _heuristic_run("wide32", method, dir_idx, 2, 25, two_step=False)
    assert oenv.episodes >= 2, oenv.episodes


@pytest.mark.parametrize("method,dir_idx", [("MINZ", 0), ("DBLF", 1), ("FIRSTFIT", 3)])
def test_heuristic_step_more_than_31_levels(method, dir_idx):
    oenv = _heuristic_run("levels60", method, dir_idx, 3, 30, two_step=False)
    assert oenv.episodes >= 1, oenv.episodes


@pytest.mark.parametrize("name", ["wide32", "levels60"])
def test_hm_raises_on_the_capacity_path(name):
    sh, seqs, kw = scenario(name)
    env = GpuPackingEnv(sh, seqs, 2, device=DEV, **kw)
    assert env.kernel_info()[1].startswith("irbpp_wide_kernel alone")
    env.reset()
    with pytest.raises(_lib.IrbppError, match="irbpp_heuristic_step"):
        env.heuristic_step("HM", 0)
    with pytest.raises(_lib.IrbppError):                       # unchanged: the stage-level scorer is not there either
        env.heuristic_action("MINZ", 0)
    env.heuristic_step("MINZ", 0)
    env.check_device_error()
    env.close()


# -- 4. buffered ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,dir_idx", [("DBLF", 0), ("HM", 2)])
def test_heuristic_step_buffered_k3(method, dir_idx):
    oenv = _heuristic_run("lattice", method, dir_idx, 3, 30, k=3)
    assert oenv.episodes >= 1, oenv.episodes


# -- 5. errors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [(4, 0, 0), (0, 16, 0), (0, 0, 16), (-1, 0, 0), (0, -1, 3)])
def test_out_of_range_cell_raises_bad_action(cell):
    sh, seqs, kw = scenario("lattice")
    env = GpuPackingEnv(sh, seqs, 4, device=DEV)
    env.reset()
    cells = np.zeros((4, 3), dtype=np.int32)
    cells[2] = cell
    env.step_cells(_dev(cells))
    with pytest.raises(_lib.IrbppError, match="BAD_ACTION"):
        env.step_info_host()
    env.close()


@pytest.mark.parametrize("kw", [dict(stability=1), dict(tuning=_lib.TUNE_FUSED_APPLY), dict(tuning=_lib.TUNE_CHAIN)])
def test_configurations_that_apply_in_the_transition_kernel_refuse(kw):
    sh, seqs, _ = scenario("lattice")
    env = GpuPackingEnv(sh, seqs, 4, device=DEV, **kw)
    obs = env.reset()
    with pytest.raises(_lib.IrbppError, match="irbpp_step_cells"):
        env.step_cells(_dev(np.zeros((4, 3))))
    with pytest.raises(_lib.IrbppError, match="irbpp_heuristic_step"):
        env.heuristic_step("MINZ", 0)
    env.step(env.policy_minz(obs))                             # the environment is still usable
    env.step_info_host()
    env.close()


def test_heuristic_step_after_set_heightmaps_is_a_state_error():
    """irbpp_set_heightmaps clears the stored grids: IRBPP_ERR_STATE until the next observation of all bins; step_cells still
    works (its drop height is recomputed on the new map, as for irbpp_step)."""
    sh, seqs, _ = scenario("lattice")
    env = GpuPackingEnv(sh, seqs, 4, device=DEV)
    obs = env.reset()
    env.heuristic_step("DBLF", 0)
    hm = env.get_heightmaps()
    env.set_heightmaps(hm)
    with pytest.raises(_lib.IrbppError, match="status -3"):
        env.heuristic_step("DBLF", 0)
    env.step_cells(env.heuristic_action("DBLF", 0))            # observes again
    env.heuristic_step("DBLF", 0)
    env.step_info_host()
    env.close()
    benv = GpuPackingEnv(sh, seqs, 4, device=DEV, bufferSize=3)
    benv.reset()
    with pytest.raises(_lib.IrbppError, match="status -3"):     # buffered: no location observation yet
        benv.heuristic_step("DBLF", 0)
    benv.get_action_candidates(_dev(np.zeros(4)))
    benv.heuristic_step("DBLF", 0)
    with pytest.raises(_lib.IrbppError, match="status -3"):
        benv.heuristic_step("DBLF", 0)
    benv.close()


def test_grouped_env_forms_equal_one_env():
    sh, seqs, _ = scenario("lattice")
    n = 64
    one, grp = GpuPackingEnv(sh, seqs, n, device=DEV), GroupedPackingEnv(sh, seqs, n, 2, device=DEV)
    eq(one.reset().cpu().numpy(), grp.reset().cpu().numpy())
    for t in range(20):
        if t % 2:
            cells = one.heuristic_action("MINZ", 1)
            o1, _, _ = one.step_cells(cells)
            o2 = grp.step_cells(cells)
        else:
            o1, _, _ = one.heuristic_step("DBLF", 2)
            o2 = grp.heuristic_step("DBLF", 2)
        h1, h2 = one.step_info_host(), grp.step_info_host()
        eq(o1.cpu().numpy(), o2.cpu().numpy())
        for key in ("reward", "done", "ep_len"):
            eq(h1[key], h2[key])
    eq(one.get_heightmaps().cpu().numpy(), grp.get_heightmaps().cpu().numpy())
    one.close()
    grp.close()


# -- 6. evaluate(heuristic=...) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,heuristic,k", [("lattice", ("DBLF", 0), 1), ("free_form", ("MINZ", 1), 1), ("lattice", ("HM", 3), 3)])
def test_evaluate_heuristic_equals_oracle_rollout(name, heuristic, k):
    sh, seqs, kw = scenario(name, length=80)
    n = 4
    kw = dict(kw, bufferSize=k)
    order = (lambda e, o: torch.full((n,), 1, dtype=torch.int32, device=DEV)) if k > 1 else None
    res = evaluate(sh, seqs, n, heuristic=heuristic, order_policy=order, device=DEV, **kw)
    assert res["episodes"] == n
    oenv = OracleCellEnv(range(n), n, sh, seqs, **kw)
    oenv.reset()
    res_a = kw.get("resolutionA", 0.02)
    bin_z = float(np.round(kw.get("bin_dimension", (0.32, 0.32, 0.30))[2], 6))
    first, off_first = {}, 0
    for _ in range(200):
        if k > 1:
            oenv.get_action_candidates([1] * n)
        if len(first) == 0:
            off_first = -oenv.off_rows
        _, _, odone, oinfo = oenv.step_cells(oenv.heuristic_cells(*heuristic))
        if len(first) == 0:
            off_first += oenv.off_rows          # (placements while every bin is still in its first, evaluated episode)
        for i in range(n):
            if odone[i] and i not in first:
                first[i] = oinfo[i]
        if len(first) == n:
            break
    assert len(first) == n
    assert off_first >= 1, off_first        # the evaluated episodes hold placements at cells that are no candidate row
    for i in range(n):
        info = first[i]
        assert res["ratio"][i] == info["ratio"] and res["length"][i] == info["episode"]["l"]
        assert res["reward_sum"][i] == info["episode"]["raw"]
        packed = [p for p in info["packed"] if p[0] is not None and p[0] >= 0]
        assert len(res["trajs"][i]) == len(packed) and len(packed) >= 2
        for row, (item, rot, lx, ly, z) in zip(res["trajs"][i], packed):
            assert row[0] == item
            flb = np.round((lx * res_a, ly * res_a, bin_z), decimals=6) * 100.0     # evaluate's decode of (lx, ly, z), unchanged
            flb[2] = z * 100.0
            eq(row[2], flb / 100.0)
            eq(row[3], rotation_quaternion_xyzw(rot))
