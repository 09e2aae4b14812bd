"""Rotation aliases on the device (ShapeRot::alias, irbpp_rotalias.h): a rotation of an item whose footprint sizes, bottom table
and ext_z_r equal a lower rotation's bit for bit takes that rotation's drop heights, hands no level images over and has its
vertex bits read from that rotation's rows.  Every case plays the same seeded actions through two environments -- default, and
IRBPP_TUNE_NO_ROT_ALIAS (every rotation on its own, as before) -- and asserts bit-equality of everything a caller can see at
every step; the first steps also against the C oracle."""
import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from irbpp_amd.shapes import ShapeSet
from irbpp_amd.vec_env import GpuPackingEnv
from oracle.c_oracle import COracleVecEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 500
N, STEPS, ORACLE_STEPS = 64, 60, 20


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _aliased_general_shapes(res_h=0.01, fmin=4, fmax=20, n_shapes=24):
    """Free-form solids at four rotations in which rotation 2 IS rotation 0 (all four tables and the extents), and rotation 3
    has rotation 1's bottom table and mask under its own top table: the generic overlap path then has aliases (2 -> 0, 3 -> 1),
    and placing rotation 3 must still raise the heightmap by rotation 3's top."""
    sh = synthetic.general_shapes(n_shapes=n_shapes, res_h=res_h, n_rot=4, fmin=fmin, fmax=fmax, seed=4)
    for k in range(sh.n_shapes):
        sh.extents[k, 2] = sh.extents[k, 0]
        sh.tables[k][2] = tuple(a.copy() for a in sh.tables[k][0])
        T3, _, mH3, _ = sh.tables[k][3]
        sh.tables[k][3] = (T3, sh.tables[k][1][1].copy(), mH3, sh.tables[k][1][3].copy())
    return sh


def _all_cubes():
    """Boxes with a square footprint at four rotations: every rotation aliases to rotation 0 (box path)."""
    exts, vols, tabs = [], [], []
    for e in (0.04, 0.06, 0.10):
        for ez in (0.03, 0.07):
            ext = np.array([e, e, ez])
            exts.append([ext] * 4)
            tabs.append([synthetic._box_tables(ext, 0.01) for _ in range(4)])
            vols.append(e * e * ez)
    return ShapeSet(np.array(exts), np.array(vols), tabs, name="squares")


def _random_valid_rows(obs, gen):
    """A candidate row with V == 1 per bin, drawn with the seeded generator (row 0 where a bin has none)."""
    v = obs[:, :5 * S].reshape(obs.shape[0], S, 5)[:, :, 4].cpu()
    w = torch.rand(v.shape, generator=gen) + 1.0
    return torch.argmax(w * (v == 1), dim=1).to(torch.int32)


def _play(shapes, seqs, tuning=0, n=N, steps=STEPS, k=1, want_alias=True, **kw):
    envs = [GpuPackingEnv(shapes, seqs, n, device=DEV, tuning=f, bufferSize=k, **kw) for f in (tuning, tuning | _lib.TUNE_NO_ROT_ALIAS)]
    cenv = COracleVecEnv(n, shapes, seqs, bufferSize=k, **{a: b for a, b in kw.items() if a != "selectedAction"})
    logs = [e.enable_placement_log(256) for e in envs]
    gen = torch.Generator(device="cpu").manual_seed(17)
    obs = [e.reset() for e in envs]
    cobs = _f32(cenv.reset())
    slots = [torch.full((n,), j, dtype=torch.int32, device=DEV) for j in range(k)]
    done_total = 0
    for t in range(steps):
        assert torch.equal(obs[0], obs[1]), f"observation, step {t}"
        if t <= ORACLE_STEPS:
            np.testing.assert_array_equal(obs[0].cpu().numpy(), cobs, err_msg=f"observation against the oracle, step {t}")
        if k > 1:
            loc = [e.get_action_candidates(slots[t % k]) for e in envs]
            assert torch.equal(loc[0], loc[1]), f"location observation, step {t}"
            if t < ORACLE_STEPS:
                cloc = _f32(cenv.get_action_candidates(np.full(n, t % k)))
                np.testing.assert_array_equal(loc[0].cpu().numpy(), cloc, err_msg=f"location observation against the oracle, step {t}")
        else:
            loc = obs
        # posZmap / naiveMask of the observed item (what w_posz / w_valid hold), every rotation's own rows
        items = loc[0][:, 5 * S].to(torch.int32)
        grids = [e.possible_position(items) for e in envs]
        assert torch.equal(grids[0][0], grids[1][0]) and torch.equal(grids[0][1], grids[1][1]), f"grids, step {t}"
        if t < ORACLE_STEPS:
            for i in range(0, n, 7):
                pz, mk = cenv.envs[i].grids()
                np.testing.assert_array_equal(grids[0][1][i].cpu().numpy(), mk.astype(np.uint8), err_msg=f"naiveMask, bin {i}, step {t}")
                np.testing.assert_array_equal(grids[0][0][i].cpu().numpy(), pz, err_msg=f"posZmap, bin {i}, step {t}")
        act = envs[0].policy_minz(loc[0]) if t % 3 == 2 else _random_valid_rows(loc[0], gen).to(DEV)
        assert torch.equal(act, envs[1].policy_minz(loc[1])) or t % 3 != 2
        res = [e.step(act.clone()) for e in envs]
        info = [e.step_info_host() for e in envs]
        for x, y in zip(res[0], res[1]):
            assert torch.equal(x, y), f"step {t}"
        for key in info[0]:
            np.testing.assert_array_equal(info[0][key], info[1][key], err_msg=f"{key}, step {t}")
        assert torch.equal(envs[0].get_heightmaps(), envs[1].get_heightmaps()), f"heightmaps, step {t}"
        assert torch.equal(logs[0][0], logs[1][0]) and torch.equal(logs[0][1], logs[1][1]), f"placement log, step {t}"
        if t < ORACLE_STEPS:
            cstep = cenv.step(act.cpu().numpy())
            cobs = _f32(cstep[0])
            np.testing.assert_array_equal(res[0][2].cpu().numpy().astype(bool), np.asarray(cstep[2], dtype=bool), err_msg=f"done, step {t}")
            np.testing.assert_array_equal(_f32(res[0][1].cpu().numpy()), _f32(cstep[1]), err_msg=f"reward, step {t}")
            np.testing.assert_array_equal(envs[0].get_heightmaps()[::9].cpu().numpy(),
                                          np.stack([cenv.envs[i].heightmap() for i in range(0, n, 9)]), err_msg=f"heightmaps, step {t}")
        obs = [r[0].clone() for r in res]
        done_total += int(res[0][2].sum())
    # rows of rotations that are aliases were really handed out (so their vertex bits came from another rotation's rows)
    rows = loc[0][:, :5 * S].reshape(n, S, 5).cpu().numpy()
    rots_seen = set(np.unique(rows[:, :, 0][rows[:, :, 4] == 1]).astype(int).tolist())
    assert done_total > 0
    if want_alias:
        assert len(rots_seen) > 1, rots_seen
    for e in envs:
        e.check_device_error()
        e.close()


def _blockout(n_rot=4):
    sh = synthetic.blockout_shapes(64, n_rot=n_rot, seed=0)
    return sh, synthetic.make_sequences(sh.n_shapes, 200, 80, seed=31)


@pytest.mark.parametrize("case", ["blockout_r4", "blockout_r8", "cube"])
def test_lattice_and_box_paths(case):
    if case == "cube":
        sh = synthetic.cube_shapes()
        seqs = synthetic.make_sequences(sh.n_shapes, 200, 80, seed=31)
    else:
        sh, seqs = _blockout(8 if case == "blockout_r8" else 4)
    _play(sh, seqs)


@pytest.mark.parametrize("wg512", [False, True])
def test_generic_path_with_aliases_under_a_different_top(wg512):
    """Free-form data with duplicate rotations, 256- and 512-thread workgroups.  (irbpp_load_shapes stores identity aliases for
    rotations that walk their cell lists -- DESIGN section 3 -- so today both environments do the same work here; the case holds
    whichever way the list loop treats an aliased rotation.)"""
    if wg512:
        sh = _aliased_general_shapes(res_h=0.005, fmin=8, fmax=40)
        kw = dict(resolutionA=0.02, resolutionH=0.005)
        tuning, n = _lib.TUNE_WG512, 16
    else:
        sh, kw, tuning, n = _aliased_general_shapes(), {}, 0, N
    seqs = synthetic.make_sequences(sh.n_shapes, 200, 80, seed=31)
    # the aliased rotation's own top table is what gets placed: same cell, rotation 1 against rotation 3
    a, b = [GpuPackingEnv(sh, seqs, 4, device=DEV, tuning=tuning, **kw) for _ in range(2)]
    assert ("w512" in a.kernel_info()[1]) == wg512, a.kernel_info()
    a.reset(), b.reset()
    a.step_cells(torch.tensor([[1, 0, 0]] * 4, dtype=torch.int32, device=DEV))
    b.step_cells(torch.tensor([[3, 0, 0]] * 4, dtype=torch.int32, device=DEV))
    ha, hb = a.get_heightmaps(), b.get_heightmaps()
    assert all(not torch.equal(ha[i], hb[i]) for i in range(4))
    for e in (a, b):
        e.check_device_error()
        e.close()
    _play(sh, seqs, tuning=tuning, n=n, **kw)


@pytest.mark.parametrize("case", ["all_cubes", "no_duplicates"])
def test_degenerate_shape_sets(case):
    if case == "all_cubes":
        sh = _all_cubes()
    else:
        sh = synthetic.general_shapes(n_shapes=24, n_rot=4, seed=4)
    _play(sh, synthetic.make_sequences(sh.n_shapes, 200, 80, seed=31))


@pytest.mark.parametrize("form", ["WAVE_EMIT", "BLOCK_EMIT", "SPLIT_APPLY", "FUSED_APPLY", "NO_SPECIALISED"])
def test_forced_kernel_forms_on_blockout(form):
    sh, seqs = _blockout()
    _play(sh, seqs, tuning=getattr(_lib, "TUNE_" + form))


def test_buffered():
    sh, seqs = _blockout()
    _play(sh, seqs, k=3)


@pytest.mark.parametrize("tuning", [0, _lib.TUNE_WAVE_EMIT, _lib.TUNE_NO_BOX_PATH])
def test_more_than_s_candidates_on_aliased_rotations(tuning):
    """A one-cell item whose two rotations are one (rotation 1 aliases rotation 0) over speckled heightmaps: posZmap is then the
    speckle itself, each rotation has far more than S / 2 vertices, and the selection of the S lowest (radix select: the
    workgroup-per-bin emit kernel, the wave-per-bin kernel's hand-back, the heavy-first route of the generic path) reads rotation
    1's vertex bits from rotation 0's rows.  S = 40; against the NO_ROT_ALIAS environment and the C oracle."""
    ext = np.array([0.02, 0.02, 0.02])
    sh = ShapeSet(np.array([[ext] * 2]), np.array([8e-6]), [[synthetic._box_tables(ext, 0.01) for _ in range(2)]], name="unit")
    seqs = np.zeros((8, 40), dtype=np.int32)
    n, s_sel, k = 8, 40, 2
    envs = [GpuPackingEnv(sh, seqs, n, device=DEV, selectedAction=s_sel, bufferSize=k, tuning=f) for f in (tuning, tuning | _lib.TUNE_NO_ROT_ALIAS)]
    cenv = COracleVecEnv(n, sh, seqs, selectedAction=s_sel, bufferSize=k)
    for e in envs:
        e.reset()
    cenv.reset()
    rng = np.random.RandomState(3)
    full = 0
    for t in range(10):
        hm = np.zeros((n, 32, 32))
        for i in range(n):
            im = rng.rand(16, 16) < rng.uniform(0.3, 0.7)
            lv = np.where(im, 0.05, 0.11) + rng.randint(0, 2, size=(16, 16)) * np.where(im, 0.0, 0.03)
            hm[i] = np.kron(lv, np.ones((2, 2)))
            cenv.envs[i].set_heightmap(hm[i])
        for e in envs:
            e.set_heightmaps(torch.from_numpy(hm).to(DEV))
        slot = torch.full((n,), t % k, dtype=torch.int32, device=DEV)
        loc = [e.get_action_candidates(slot) for e in envs]
        cloc = _f32(cenv.get_action_candidates(np.full(n, t % k)))
        assert torch.equal(loc[0], loc[1]), f"round {t}"
        np.testing.assert_array_equal(loc[0].cpu().numpy(), cloc, err_msg=f"round {t}")
        rows = loc[0][:, :5 * s_sel].reshape(n, s_sel, 5)
        full += int(((rows[:, :, 4] == 1).all(dim=1) & (rows[:, :, 0] == 1).any(dim=1)).sum())
        act = envs[0].policy_minz(loc[0])
        res = [e.step(act.clone()) for e in envs]
        cobs = _f32(cenv.step(act.cpu().numpy())[0])
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(envs[0].get_heightmaps(), envs[1].get_heightmaps()), f"round {t}"
        np.testing.assert_array_equal(res[0][0].cpu().numpy(), cobs, err_msg=f"round {t}")
    assert full >= 20, full                          # all S rows are candidates, rows of the aliased rotation among them
    for e in envs:
        e.check_device_error()
        e.close()
