"""More than 31 height levels -- resolutionZ = 0.005 / 0.0025 on the 0.30 m bin (60 / 120 levels), a 0.60 m bin at 0.01 -- through
irbpp_wide.hip's capacity path (level codes level + 32 in a byte, up to 256 per rotation) against BOTH oracles and against the
reference's own PackingGame (tests/golden/make_levels_golden.py).  Every test also checks that a level above 31 was reached: the
highest floor(H / resolutionZ) over the valid candidate rows."""
import os
import types

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from irbpp_amd.vec_env import GpuPackingEnv, GpuVecEnv
from oracle.c_oracle import COracleVecEnv
from oracle.packing import OracleVecEnv
from helpers import minz_action
from test_height_levels_cpu import levels_scenario, max_level

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 500
WIDE = "irbpp_wide_kernel alone"


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _play(shapes, seqs, n, steps, numpy_steps, **kw):
    """GPU against the C oracle for `steps` steps, the numpy oracle beside them for the first `numpy_steps`; returns (episodes
    ended, observations whose S rows are all candidates, the highest level among the candidate rows)."""
    res_z, s_sel = kw["resolutionZ"], kw.get("selectedAction", S)
    genv = GpuVecEnv(shapes, seqs, n, device=DEV, **kw)
    genv.candidates_on_device = True
    assert genv.env.kernel_info()[1].startswith(WIDE)
    cenv = COracleVecEnv(n, shapes, seqs, **kw)
    oenv = OracleVecEnv(n, shapes, seqs, **kw)
    gobs = genv.reset()
    craw = cenv.reset()
    cobs = _f32(craw)
    np.testing.assert_array_equal(gobs.cpu().numpy(), cobs)
    np.testing.assert_array_equal(_f32(oenv.reset()), cobs)
    done_total, full, top = 0, 0, max_level(craw, res_z, s_sel)
    for t in range(steps):
        act = genv.env.policy_minz(gobs).cpu().numpy()
        np.testing.assert_array_equal(act, np.array([minz_action(o, s_sel) for o in cobs]))
        gobs, grew, gdone, ginfo = genv.step(act)
        craw, crew, cdone, cinfo = cenv.step(act)
        cobs = _f32(craw)
        np.testing.assert_array_equal(gobs.cpu().numpy(), cobs, err_msg=f"step {t}")
        np.testing.assert_array_equal(gdone, cdone)
        np.testing.assert_array_equal(grew.numpy()[:, 0], crew.astype(np.float32))
        for i in range(n):
            if cdone[i]:
                assert ginfo[i]["counter"] == cinfo[i]["counter"] and ginfo[i]["ratio"] == cinfo[i]["ratio"]
                assert ginfo[i]["episode"]["r"] == cinfo[i]["episode"]["r"]
        if t < numpy_steps:
            oobs, orew, odone, _ = oenv.step(act)
            np.testing.assert_array_equal(_f32(oobs), cobs, err_msg=f"numpy oracle, step {t}")
            np.testing.assert_array_equal(odone, cdone)
        hm = genv.env.get_heightmaps().cpu().numpy()
        for i in range(n):
            np.testing.assert_array_equal(hm[i], cenv.envs[i].heightmap())
        rows = cobs[:, :5 * s_sel].reshape(n, s_sel, 5)
        full += int((rows[:, :, 4] == 1).all(axis=1).sum())
        done_total += int(cdone.sum())
        top = max(top, max_level(craw, res_z, s_sel))
    genv.env.check_device_error()
    genv.close()
    return done_total, full, top


@pytest.mark.parametrize("res_z", [0.005, 0.0025])
def test_levels_16x16_blockout_r4(res_z):
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    seqs = synthetic.make_sequences(sh.n_shapes, 32, 150, seed=5)
    done, _, top = _play(sh, seqs, 4, 50, 4, resolutionZ=res_z)
    assert done >= 2 and top > 31, (done, top)


@pytest.mark.parametrize("res_z", [0.005, 0.0025])
def test_levels_16x16_free_form_r8_more_than_s(res_z):
    sh = synthetic.general_shapes(n_shapes=16, n_rot=8, seed=1)
    seqs = synthetic.make_sequences(sh.n_shapes, 32, 80, seed=9)
    done, full, top = _play(sh, seqs, 4, 40, 3, resolutionZ=res_z, selectedAction=150)
    assert done >= 2 and full >= 10 and top > 31, (done, full, top)


def test_levels_32x32_grid():
    sh = synthetic.general_shapes(n_shapes=16, n_rot=4, fmin=4, fmax=14, seed=3)
    seqs = synthetic.make_sequences(sh.n_shapes, 32, 80, seed=2)
    done, full, top = _play(sh, seqs, 3, 40, 3, resolutionZ=0.005, resolutionA=0.01, resolutionH=0.01)
    assert done >= 1 and full >= 1 and top > 31, (done, full, top)


def test_levels_tall_bin():
    """A 0.32 x 0.32 x 0.60 m bin at the default resolutionZ = 0.01: 60 levels."""
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    seqs = synthetic.make_sequences(sh.n_shapes, 32, 200, seed=5)
    done, _, top = _play(sh, seqs, 3, 90, 3, resolutionZ=0.01, bin_dimension=(0.32, 0.32, 0.60))
    assert done >= 1 and top > 31, (done, top)


def test_levels_hierarchical():
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    seqs = synthetic.make_sequences(sh.n_shapes, 64, 150, seed=5)
    n, k = 3, 3
    kw = dict(resolutionZ=0.005, bufferSize=k)
    genv = GpuVecEnv(sh, seqs, n, device=DEV, **kw)
    genv.candidates_on_device = True
    assert genv.env.kernel_info()[1].startswith(WIDE)
    cenv = COracleVecEnv(n, sh, seqs, **kw)
    oenv = OracleVecEnv(n, sh, seqs, **kw)
    gord = genv.reset()
    np.testing.assert_array_equal(gord.cpu().numpy(), _f32(cenv.reset()))
    oenv.reset()
    done_total, top = 0, -1
    for t in range(50):
        oa = np.array([(t * 5 + 1 + i) % k for i in range(n)])
        gloc = genv.get_action_candidates(oa)
        craw = cenv.get_action_candidates(oa)
        cloc = _f32(craw)
        np.testing.assert_array_equal(gloc.cpu().numpy(), cloc, err_msg=f"location observation, placement {t}")
        top = max(top, max_level(craw, 0.005))
        if t < 4:
            np.testing.assert_array_equal(_f32(oenv.get_action_candidates(oa)), cloc)
        act = genv.env.policy_minz(gloc).cpu().numpy()
        gord, grew, gdone, _ = genv.step(act)
        cord, crew, cdone, _ = cenv.step(act)
        np.testing.assert_array_equal(gord.cpu().numpy(), _f32(cord))
        np.testing.assert_array_equal(gdone, cdone)
        np.testing.assert_array_equal(grew.numpy()[:, 0], crew.astype(np.float32))
        if t < 4:
            oenv.step(act)
        done_total += int(cdone.sum())
    genv.env.check_device_error()
    genv.close()
    assert done_total >= 1 and top > 31, (done_total, top)


@pytest.mark.parametrize("n", [1, 96])
def test_levels_match_the_reference_goldens(golden_dir, n):
    """The reference's own PackingGame at resolutionZ = 0.005 (online_levels60, hier_levels60_k3), replayed by one bin and by every
    bin of a 96-bin launch."""
    from test_gpu_large_forms import _replay_table
    g = np.load(os.path.join(golden_dir, "online_levels60.npz"))
    assert max_level(g["obs"]) > 31
    sh, _ = levels_scenario("online_levels60")
    env = GpuPackingEnv(sh, _replay_table(g["seq"], n, int(g["done"].sum())), n, device=DEV, resolutionZ=0.005)
    assert env.kernel_info()[1].startswith(WIDE)
    ref = torch.from_numpy(_f32(g["obs"])).to(DEV)
    obs = env.reset()
    assert torch.equal(obs, ref[0].expand(n, -1))
    fb = torch.from_numpy(np.array([[c // 256, (c % 256) // 16, c % 16, 0.30, 0.0] for c in range(S)]).astype(np.float32).reshape(-1)).to(DEV)
    act = torch.empty((n,), dtype=torch.int32, device=DEV)
    for t in range(len(g["act"])):
        act.fill_(int(g["act"][t]))
        obs, rew, done = env.step(act)
        h = env.step_info_host()
        assert (h["done"] == bool(g["done"][t])).all() and (h["reward"].astype(np.float32) == np.float32(g["rew"][t])).all(), t
        if g["done"][t]:
            assert (h["counter"] == g["counter"][t]).all() and (h["ratio"] == g["ratio"][t]).all()
        r = ref[t + 1]
        if bool((r[:5 * S].reshape(S, 5)[:, 4] == 1).any()):
            assert torch.equal(obs, r.expand(n, -1)), f"step {t}"
        else:                                                # fallback rows: the reference's order is its numpy build's (binPhy.py:217-225)
            assert torch.equal(obs[:, 5 * S:], r[5 * S:].expand(n, -1)) and torch.equal(obs[:, :5 * S], fb.expand(n, -1))
    env.check_device_error()
    env.close()
    g = np.load(os.path.join(golden_dir, "hier_levels60_k3.npz"))
    assert max_level(g["loc_obs"]) > 31
    sh, _ = levels_scenario("hier_levels60_k3")
    env = GpuPackingEnv(sh, _replay_table(g["seq"], n, int(g["done"].sum())), n, device=DEV, resolutionZ=0.005, bufferSize=3)
    order_ref = torch.from_numpy(_f32(g["order_obs"])).to(DEV)
    loc_ref = torch.from_numpy(_f32(g["loc_obs"])).to(DEV)
    assert torch.equal(env.reset(), order_ref[0].expand(n, -1))
    oa = torch.empty((n,), dtype=torch.int32, device=DEV)
    for t in range(len(g["act"])):
        oa.fill_(int(g["order_act"][t]))
        loc = env.get_action_candidates(oa)
        r = loc_ref[t]
        assert torch.equal(loc[:, 5 * S:], r[5 * S:].expand(n, -1)), t
        if bool((r[:5 * S].reshape(S, 5)[:, 4] == 1).any()):
            assert torch.equal(loc, r.expand(n, -1)), f"placement {t}"
        act.fill_(int(g["act"][t]))
        order, rew, done = env.step(act)
        assert bool((done.bool() == bool(g["done"][t])).all())
        assert torch.equal(order, order_ref[t + 1].expand(n, -1)), t
    env.check_device_error()
    env.close()


def test_levels_make_vec_envs():
    """make_vec_envs(args) with args.resolutionZ = 0.005: the VecEnv surface, against the C oracle."""
    from irbpp_amd.vec_env import make_vec_envs
    sh = synthetic.general_shapes(n_shapes=16, n_rot=4, fmin=4, fmax=14, seed=3)
    seqs = synthetic.make_sequences(sh.n_shapes, 32, 80, seed=2)
    n = 4
    args = types.SimpleNamespace(
        num_processes=n, device=0, seed=1, shapes=sh, sequences=seqs, resolutionA=0.02, resolutionH=0.01, resolutionZ=0.005,
        bin_dimension=np.round([0.32, 0.32, 0.30], 6), selectedAction=S, bufferSize=1, scale=[100, 100, 100], evaluate=True)
    envs, _, _ = make_vec_envs(args, "./logs/runinfo", True)
    assert envs.env.kernel_info()[1].startswith(WIDE)
    cenv = COracleVecEnv(n, sh, seqs, resolutionZ=0.005)
    gobs, craw = envs.reset(), cenv.reset()
    np.testing.assert_array_equal(gobs.cpu().numpy(), _f32(craw))
    top = max_level(craw)
    for t in range(40):
        act = np.array([minz_action(o, S) for o in _f32(craw)])
        gobs, grew, gdone, _ = envs.step(act)
        craw, crew, cdone, _ = cenv.step(act)
        np.testing.assert_array_equal(gobs.cpu().numpy(), _f32(craw), err_msg=f"step {t}")
        np.testing.assert_array_equal(gdone, cdone)
        top = max(top, max_level(craw))
    envs.env.check_device_error()
    envs.close()
    assert top > 31


def test_levels_evaluate():
    """evaluate(..., resolutionZ=0.005) on the 16 x 16 grid: statistics and placement records equal the oracle's episodes."""
    from irbpp_amd.evaluate import evaluate
    from oracle.packing import PackingGame
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    seqs = synthetic.make_sequences(sh.n_shapes, 16, 150, seed=5)
    E = 3
    out = evaluate(sh, seqs, E, device=DEV, resolutionZ=0.005)
    assert out["episodes"] == E and out["unfinished"] == 0
    env = PackingGame(sh, seqs, resolutionZ=0.005)
    top = -1
    for ep in range(E):
        obs = env.reset()
        rsum, steps = 0.0, 0
        while True:
            top = max(top, max_level(obs[None]))
            obs, r, d, info = env.step(minz_action(_f32(obs), S))
            rsum += r
            steps += 1
            if d:
                break
        assert out["ratio"][ep] == info["ratio"] and out["length"][ep] == steps
        assert out["reward_sum"][ep] == rsum
        placed = env.packed
        assert len(out["trajs"][ep]) == len(placed) == info["counter"] + 1
        for got, (item, rot, lx, ly, height) in zip(out["trajs"][ep], placed):
            assert got[0] == item
            np.testing.assert_allclose(got[2], [lx * 0.02, ly * 0.02, height], rtol=0, atol=1e-12)
    assert top > 31


def test_levels_boundaries():
    """222 levels (a 2.22 m bin at 0.01) is created and plays: level images chosen at will through the heightmap of bins that observe
    a one-cell item, up to level 220 -- hundreds of level images a bin, the > S selection over them -- against the C oracle; 223
    levels is IRBPP_ERR_ARG; the stage-level entry points answer IRBPP_ERR_ARG on the capacity path."""
    from irbpp_amd.shapes import ShapeSet
    from irbpp_amd.synthetic import _box_tables
    ext = np.array([0.01, 0.01, 0.01])
    sh = ShapeSet(np.array([[ext] * 2]), np.array([1e-6]), [[_box_tables(ext, 0.01) for _ in range(2)]], name="unit1")
    seqs = np.zeros((8, 40), dtype=np.int32)
    n, k = 4, 2
    kw = dict(bufferSize=k, bin_dimension=(0.32, 0.32, 2.22))
    genv = GpuVecEnv(sh, seqs, n, device=DEV, **kw)
    genv.candidates_on_device = True
    name = genv.env.kernel_info()[1]
    assert name.startswith(WIDE) and "222 height levels" in name, name
    cenv = COracleVecEnv(n, sh, seqs, **kw)
    np.testing.assert_array_equal(genv.reset().cpu().numpy(), _f32(cenv.reset()))
    rng = np.random.RandomState(3)
    top, full = -1, 0
    for t in range(6):
        hm = rng.randint(0, 221, size=(n, 32, 32)) * 0.01 + rng.uniform(0.0, 0.009, size=(n, 32, 32))
        hm[:, :, :16] = np.minimum(hm[:, :, :16], 0.005 * (t + 1) * rng.randint(0, 40, size=(n, 32, 16)))   # low levels beside the high ones
        genv.env.set_heightmaps(torch.from_numpy(hm).to(DEV))
        for i in range(n):
            cenv.envs[i].set_heightmap(hm[i])
        oa = np.array([t % k] * n)
        gloc = genv.get_action_candidates(oa).cpu().numpy()
        craw = cenv.get_action_candidates(oa)
        cloc = _f32(craw)
        np.testing.assert_array_equal(gloc, cloc, err_msg=f"round {t}")
        top = max(top, max_level(craw, 0.01))
        full += int((cloc[:, :5 * S].reshape(n, S, 5)[:, :, 4] == 1).all(axis=1).sum())
        act = np.array([minz_action(c, S) for c in cloc])
        gord, _, gdone, _ = genv.step(act)
        cord, _, cdone, _ = cenv.step(act)
        np.testing.assert_array_equal(gord.cpu().numpy(), _f32(cord))
        np.testing.assert_array_equal(gdone, cdone)
    genv.env.check_device_error()
    assert top > 200 and full >= 1, (top, full)
    env = genv.env
    with pytest.raises(_lib.IrbppError):
        env.possible_position(torch.zeros(n, dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.IrbppError):
        env.heuristic_action("MINZ")
    genv.close()
    with pytest.raises(_lib.IrbppError, match="argument"):
        GpuPackingEnv(sh, seqs, 2, device=DEV, bin_dimension=(0.32, 0.32, 2.23))


def test_bench_workloads_keep_the_tuned_kernels():
    """The switch is the level count: 31 levels (resolutionZ = 0.30 / 31) keep every bench workload on the kernels it takes at the
    default 0.01, 32 levels move it to the capacity path."""
    from bench import make_workload
    for wl in ("blockout", "blockout_r8", "blockout_k10", "general", "abc_fine", "cube"):
        sh, seqs, kw = make_workload(wl)
        names = []
        for res_z in (0.01, 0.30 / 31, 0.30 / 32):
            env = GpuPackingEnv(sh, seqs[:64], 256, device=DEV, resolutionZ=res_z, **kw)
            names.append(env.kernel_info())
            env.close()
        assert WIDE not in names[0][1] and names[1] == names[0], (wl, names)
        assert names[2][1].startswith(WIDE) and "32 height levels" in names[2][1], (wl, names)
