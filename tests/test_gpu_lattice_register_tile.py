"""The observe-only lattice launch without its LDS tile (cell_tile_stage in csrc/irbpp_kernels.hip): behind irbpp_apply_kernel
the transition kernel's thread of action cell t loads that cell's own step x step heightmap cells, keeps their maximum for the
block-max grid and writes their float32 copy into the observation -- no float64 tile in LDS.  IRBPP_TUNE_LDS_TILE keeps the
tile.  Same observations (heightmap tail included), rewards, done flags, episode info and float64 heightmaps as the C oracle
and as the old form, step for step."""
import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from irbpp_amd.vec_env import GpuPackingEnv
from oracle.c_oracle import COracleVecEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 500
SPLIT, FUSED, NOSPEC, TILE = _lib.TUNE_SPLIT_APPLY, _lib.TUNE_FUSED_APPLY, _lib.TUNE_NO_SPECIALISED, _lib.TUNE_LDS_TILE


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _actions(obs, t, rng, S=S):
    """A random VALID candidate row per bin (row 0 where there is none: the refused placement ends the episode); every
    fifth bin, in turn, draws from all S rows, zero padding included, so that episodes end within a dozen steps too."""
    c = np.asarray(obs)[:, :5 * S].reshape(len(obs), S, 5)
    act = np.zeros(len(obs), dtype=np.int32)
    for b in range(len(obs)):
        rows = np.flatnonzero(c[b, :, 4] == 1)
        if (b + t) % 5 == 0:
            act[b] = rng.randint(0, S)
        elif len(rows):
            act[b] = rows[rng.randint(0, len(rows))]
    return act


def _envs_kernel(env):
    return env.kernel_info()[1].split(" + ")[0]


def _check_step(env, res, ores, cenv, t):
    """one step of `env` against the oracle's: observation, reward, done, info, float64 heightmaps"""
    gobs, _, _ = res
    oobs, orew, odone, oinfo = ores
    np.testing.assert_array_equal(gobs.cpu().numpy(), _f32(oobs), err_msg=f"observation, step {t}")
    info = env.step_info_host()
    np.testing.assert_array_equal(info["done"], odone, err_msg=f"done, step {t}")
    np.testing.assert_array_equal(info["reward"].astype(np.float32), orew.astype(np.float32), err_msg=f"reward, step {t}")
    for b in np.flatnonzero(odone):
        assert info["counter"][b] == oinfo[b]["counter"] and info["ratio"][b] == oinfo[b]["ratio"], f"info, step {t}, bin {b}"
    hm = env.get_heightmaps().cpu().numpy().reshape(env.num_bins, -1)
    for b, e in enumerate(cenv.envs):
        np.testing.assert_array_equal(hm[b], e.heightmap().reshape(-1), err_msg=f"heightmap, step {t}, bin {b}")
    return info


# (bins, tuning, steps, environment arguments, cube edge, transition kernel that must launch)
#   2048 / 4096: up to two partial-free rounds of workgroups; irbpp_plan.h's split_apply splits lattice data by itself from 4096
#   bins on (tests/test_launch_plan_host.py pins that), so 4096 is the launch that takes the new form with no tuning bit at all
#   5 bins, split forced: one partial round, the last bin of the environment
#   step 4 (resolutionH 0.005) on the run-time build: a 10 x 10 action grid, because the 16 x 16 one's 32 KB tile goes to the
#   build that decides its path at run time, which keeps the tile; step 1: the heightmap cell is the action cell
CASES = {
    "2048": (2048, 0, 12, {}, 0.04, "irbpp_env_kernel_s1"),
    "4096": (4096, 0, 12, {}, 0.04, "irbpp_env_kernel_s1"),
    "5_split": (5, SPLIT, 12, {}, 0.04, "irbpp_env_kernel_s1"),
    "5_split_runtime": (5, SPLIT | NOSPEC, 12, {}, 0.04, "irbpp_env_kernel"),
    "step4": (64, SPLIT, 12, dict(resolutionH=0.005, bin_dimension=(0.20, 0.20, 0.30), selectedAction=120), 0.04, "irbpp_env_kernel"),
    "step1": (7, SPLIT, 12, dict(resolutionH=0.02), 0.04, "irbpp_env_kernel"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_blockout_matches_the_c_oracle(case):
    n, tuning, steps, kw, cube, kernel = CASES[case]
    sh = synthetic.blockout_shapes(n_shapes=24, res_h=kw.get("resolutionH", 0.01), n_rot=4, cube=cube, seed=3)
    seqs = synthetic.make_sequences(sh.n_shapes, max(64, n), 60, seed=17)
    env = GpuPackingEnv(sh, seqs, n, device=DEV, tuning=tuning, **kw)
    assert _envs_kernel(env) == kernel
    assert ("irbpp_apply_kernel in front" in env.kernel_info()[1]) == (n >= 4096 or bool(tuning & SPLIT)), env.kernel_info()[1]
    cenv = COracleVecEnv(n, sh, seqs, threads=16, **kw)
    gobs, oobs = env.reset(), cenv.reset()
    np.testing.assert_array_equal(gobs.cpu().numpy(), _f32(oobs))
    rng = np.random.RandomState(29)
    ndone = 0
    for t in range(steps):
        act = _actions(_f32(oobs), t, rng, kw.get("selectedAction", S))
        res = env.step(torch.from_numpy(act).to(DEV))
        ores = cenv.step(act)
        _check_step(env, res, ores, cenv, t)
        oobs = ores[0]
        ndone += int(ores[2].sum())
    assert ndone > 0                                          # terminal steps and auto-resets were among them
    env.check_device_error()
    env.close()


def test_old_form_and_new_form_agree_on_both_builds():
    """The specialised build against the run-time build, each with and without IRBPP_TUNE_LDS_TILE, and the fused apply (which
    has the tile in any case): identical outputs on the same seeded trajectory."""
    n, steps = 160, 40
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.04, seed=3)
    seqs = synthetic.make_sequences(sh.n_shapes, 256, 60, seed=17)
    flags = [SPLIT, SPLIT | TILE, SPLIT | NOSPEC, SPLIT | NOSPEC | TILE, FUSED, FUSED | TILE]
    envs = [GpuPackingEnv(sh, seqs, n, device=DEV, tuning=f) for f in flags]
    names = [_envs_kernel(e) for e in envs]
    assert names == ["irbpp_env_kernel_s1", "irbpp_env_kernel_s1", "irbpp_env_kernel", "irbpp_env_kernel",
                     "irbpp_env_kernel_s1", "irbpp_env_kernel_s1"], names
    obs = [e.reset() for e in envs]
    assert all(torch.equal(obs[0], o) for o in obs[1:])
    rng = np.random.RandomState(31)
    ndone = 0
    for t in range(steps):
        act = torch.from_numpy(_actions(obs[0].cpu().numpy(), t, rng)).to(DEV)
        res = [e.step(act) for e in envs]
        info = [e.step_info_host() for e in envs]
        for j in range(1, len(envs)):
            for x, y in zip(res[0], res[j]):
                assert torch.equal(x, y), f"step {t}, env {j}"
            for key in info[0]:
                np.testing.assert_array_equal(info[0][key], info[j][key], err_msg=f"{key}, step {t}, env {j}")
        hm = [e.get_heightmaps() for e in envs]
        assert all(torch.equal(hm[0], h) for h in hm[1:]), f"heightmaps, step {t}"
        obs = [r[0] for r in res]
        ndone += int(info[0]["done"].sum())
    assert ndone > 0
    for e in envs:
        e.check_device_error()
        e.close()


def test_odd_action_grid_matches_the_oracle_and_padded_planes_cannot_occur():
    """An odd action grid: 15 x 13 cells over a 30 x 26 heightmap (no multiple of a wave, rows of 13 cells, threads beyond
    the grid) on the run-time build, both forms, against the oracle.  A heightmap that is NOT step times the action grid --
    0.31 m: 31 cells under 16 action cells, the phase planes would have padding entries (tile_words > Hc) -- is refused by
    irbpp_create, so the kernel's tile_words == Hc condition never sends a live configuration to the old form."""
    n, kw = 8, dict(bin_dimension=(0.30, 0.26, 0.30), selectedAction=150)
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.04, seed=3)
    seqs = synthetic.make_sequences(sh.n_shapes, 64, 60, seed=17)
    with pytest.raises(_lib.IrbppError, match="irbpp_create"):
        GpuPackingEnv(sh, seqs, n, device=DEV, tuning=SPLIT, bin_dimension=(0.31, 0.31, 0.30))
    envs = [GpuPackingEnv(sh, seqs, n, device=DEV, tuning=f, **kw) for f in (SPLIT, SPLIT | TILE)]
    assert all((e.Hx, e.Hy, e.Ax, e.Ay) == (30, 26, 15, 13) and _envs_kernel(e) == "irbpp_env_kernel" for e in envs)
    cenv = COracleVecEnv(n, sh, seqs, **kw)
    gobs, oobs = [e.reset() for e in envs], cenv.reset()
    for g in gobs:
        np.testing.assert_array_equal(g.cpu().numpy(), _f32(oobs))
    rng = np.random.RandomState(37)
    ndone = 0
    for t in range(30):
        act = _actions(_f32(oobs), t, rng, 150)
        ores = cenv.step(act)
        for e in envs:
            _check_step(e, e.step(torch.from_numpy(act).to(DEV)), ores, cenv, t)
        oobs = ores[0]
        ndone += int(ores[2].sum())
    assert ndone > 0
    for e in envs:
        e.check_device_error()
        e.close()


def test_fused_apply_places_on_what_a_register_tile_observe_left():
    """What the next step consumes of an observation -- the drop heights w_posz, the naiveMask rows w_valid, the queue, the
    heightmap -- handed to an environment that applies inside the transition kernel (IRBPP_TUNE_FUSED_APPLY): every state the
    new form leaves is forked there, stepped once with the same actions, and equals the split environment's own next step and
    the oracle's."""
    n = 48
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.04, seed=3)
    seqs = synthetic.make_sequences(sh.n_shapes, 64, 60, seed=17)
    split = GpuPackingEnv(sh, seqs, n, device=DEV, tuning=SPLIT)
    fused = GpuPackingEnv(sh, seqs, n, device=DEV, tuning=FUSED)
    cenv = COracleVecEnv(n, sh, seqs)
    bins = torch.arange(n, dtype=torch.int32, device=DEV)
    sobs, oobs = split.reset(), cenv.reset()
    fused.reset()
    rng = np.random.RandomState(41)
    ndone = 0
    for t in range(25):
        act = _actions(_f32(oobs), t, rng)
        dact = torch.from_numpy(act).to(DEV)
        fused.fork_bins(bins, bins, src_env=split)           # state after a register-tile observe (t = 0: after the reset)
        fres = fused.step(dact)
        sres = split.step(dact)
        ores = cenv.step(act)
        finfo = _check_step(fused, fres, ores, cenv, t)
        sinfo = _check_step(split, sres, ores, cenv, t)
        for x, y in zip(fres, sres):
            assert torch.equal(x, y), f"step {t}"
        for key in sinfo:
            np.testing.assert_array_equal(sinfo[key], finfo[key], err_msg=f"{key}, step {t}")
        oobs = ores[0]
        ndone += int(ores[2].sum())
    assert ndone > 0
    for e in (split, fused):
        e.check_device_error()
        e.close()
