"""Polygon rounds as a DUMP of the trace wave's slots (csrc/irbpp_rounds.h; the default) against the RECORD form, in which the
trace wave packs every round itself (IRBPP_TUNE_TRACE_PACK): byte-identical observations, next actions of the scripted policy
and step infos, step for step, and both equal to the C oracle.  (A FULL round list runs on the device in
tests/test_gpu_round_list_full.py, with Params::round_cap shrunk; tests/test_round_dump_on_host.py covers the routines it shares.)"""
import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from irbpp_amd.vec_env import GpuPackingEnv, GpuVecEnv
from oracle.c_oracle import COracleVecEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 500
PACK = _lib.TUNE_TRACE_PACK


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _actions(obs, t, rng):
    """A random VALID candidate row per bin (row 0 where there is none); every fifth bin, in turn, draws from all S rows, zero
    padding included, so that episodes end within a dozen steps too."""
    c = np.asarray(obs)[:, :5 * S].reshape(len(obs), S, 5)
    act = np.zeros(len(obs), dtype=np.int32)
    for b in range(len(obs)):
        rows = np.flatnonzero(c[b, :, 4] == 1)
        if (b + t) % 5 == 0:
            act[b] = rng.randint(0, S)
        elif len(rows):
            act[b] = rows[rng.randint(0, len(rows))]
    return act


def _both_forms_and_the_oracle(sh, seqs, n, steps, seed, extra_tuning=0, **kw):
    envs = [GpuPackingEnv(sh, seqs, n, device=DEV, tuning=extra_tuning | f, **kw) for f in (0, PACK)]
    assert all("irbpp_trace_kernel" in e.kernel_info()[1] and "irbpp_polygon_kernel" in e.kernel_info()[1] for e in envs)
    cenv = COracleVecEnv(n, sh, seqs, threads=16, **kw)
    obs, oobs = [e.reset() for e in envs], cenv.reset()
    for o in obs:
        np.testing.assert_array_equal(o.cpu().numpy(), _f32(oobs))
    rng = np.random.RandomState(seed)
    ndone = 0
    for t in range(steps):
        nxt = [e.policy_minz(o) for e, o in zip(envs, obs)]
        assert torch.equal(nxt[0], nxt[1]), f"next action, step {t}"
        act = _actions(_f32(oobs), t, rng)
        dact = torch.from_numpy(act).to(DEV)
        res = [e.step(dact) for e in envs]
        info = [e.step_info_host() for e in envs]
        oobs, orew, odone, _ = cenv.step(act)
        for x, y in zip(res[0], res[1]):
            assert torch.equal(x, y), f"step {t}"
        for key in info[0]:
            np.testing.assert_array_equal(info[0][key], info[1][key], err_msg=f"{key}, step {t}")
        np.testing.assert_array_equal(res[0][0].cpu().numpy(), _f32(oobs), err_msg=f"observation, step {t}")
        np.testing.assert_array_equal(info[0]["done"], odone, err_msg=f"done, step {t}")
        np.testing.assert_array_equal(info[0]["reward"].astype(np.float32), orew.astype(np.float32), err_msg=f"reward, step {t}")
        obs = [r[0] for r in res]
        ndone += int(odone.sum())
    assert ndone > 0
    for e in envs:
        e.check_device_error()
        e.close()


# 1 bin; 3 bins (one trace chunk spans bins); 70 bins (more than one chunk in an XCD's list, a short last chunk)
@pytest.mark.parametrize("n", [1, 3, 70])
def test_blockout_both_forms_equal_the_oracle(n):
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.04, seed=3)
    seqs = synthetic.make_sequences(sh.n_shapes, max(64, n), 60, seed=17)
    _both_forms_and_the_oracle(sh, seqs, n, 40, 29 + n)


def test_blockout_at_full_width_candidates_per_wave():
    """... and with 64 candidates per wave forced (few bins take the 16-candidate launch by themselves): several bins per chunk."""
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.04, seed=3)
    seqs = synthetic.make_sequences(sh.n_shapes, 64, 60, seed=17)
    _both_forms_and_the_oracle(sh, seqs, 70, 40, 5, extra_tuning=_lib.TUNE_TRACE_CPW64)


def test_speckled_images_several_rounds_per_wave():
    sh = synthetic.general_shapes(n_shapes=16, n_rot=8, seed=1)
    seqs = synthetic.make_sequences(sh.n_shapes, 32, 60, seed=9)
    _both_forms_and_the_oracle(sh, seqs, 5, 30, 13)


def _unit_item_shapes(n_rot=2):
    """One 2 cm cube: its footprint is exactly one action cell, so posZmap[r, X, Y] is the maximum of heightmap block (X, Y) --
    any 16 x 16 level image can be dialled in."""
    from irbpp_amd.shapes import ShapeSet
    from irbpp_amd.synthetic import _box_tables
    ext = np.array([0.02, 0.02, 0.02])
    return ShapeSet(np.array([[ext] * n_rot]), np.array([8e-6]), [[_box_tables(ext, 0.01) for _ in range(n_rot)]], name="unit")


def _snake_image(zigzags):
    """One 8-connected component of zigzag rows joined at alternating ends (its border runs along both sides of a one-pixel line
    and turns at every pixel): 2, 3, 4 rows give outer borders of 61, 92, 123 points -- more than the trace kernel keeps in LDS
    (spill bytes), the longest nearly a round of its own."""
    img = np.zeros((16, 16), dtype=bool)
    for j, y0 in enumerate((0, 3, 6, 9, 12)[:zigzags]):
        for x in range(16):
            img[y0 + (x & 1), x] = True
        if j < zigzags - 1:
            xe = 15 if j % 2 == 0 else 0
            img[y0 + 2, xe] = True
            img[y0 + 1, xe] = True
            img[y0 + 3, xe] = True
    return img


@pytest.mark.parametrize("cpw", [0, _lib.TUNE_TRACE_CPW64], ids=["cpw16", "cpw64"])
def test_long_borders_spill_bytes_and_a_border_alone_in_its_round(cpw):
    """Level images dialled in through the heightmap of bins that observe a one-cell item (buffered, k = 2: MODE_CANDS launches):
    snakes of 61 / 92 / 123 border points beside speckle, through both forms, against the oracle."""
    from oracle import contours as OC
    from oracle.packing import OracleVecEnv
    sh = _unit_item_shapes()
    seqs = np.zeros((8, 40), dtype=np.int32)
    n, k = 6, 2
    genvs = [GpuVecEnv(sh, seqs, n, device=DEV, bufferSize=k, tuning=cpw | f) for f in (0, PACK)]
    for g in genvs:
        g.candidates_on_device = True
    oenv = OracleVecEnv(n, sh, seqs, bufferSize=k)
    want0 = _f32(oenv.reset())
    for g in genvs:
        np.testing.assert_array_equal(g.reset().cpu().numpy(), want0)
    mids = [_snake_image(z) for z in (2, 3, 4)]
    for m, want in zip(mids, (61, 92, 123)):
        got = [len(c) for c, hole in zip(*(lambda r: (r[0], r[2]))(OC.find_contours(m.astype(np.uint8)))) if not hole]
        assert got == [want], got
    rng = np.random.RandomState(12)
    for t in range(8):
        imgs = []
        for i in range(n):
            kind = (t + i) % 3
            if kind == 0:
                m = mids[(t + i // 3) % 3]
                imgs.append(m if i % 2 == 0 else m.T.copy())
            elif kind == 1:
                imgs.append(rng.rand(16, 16) < rng.uniform(0.3, 0.7))
            else:
                imgs.append(np.kron(rng.rand(4, 4) < 0.5, np.ones((4, 4), dtype=bool)) ^ (rng.rand(16, 16) < 0.05))
        hm = np.zeros((n, 32, 32))
        for i, im in enumerate(imgs):                                       # image pixel (x, y) = action cell (row y, col x)
            lv = np.where(im, 0.05, 0.11) + rng.randint(0, 2, size=(16, 16)) * np.where(im, 0.0, 0.03)
            hm[i] = np.kron(lv, np.ones((2, 2)))
        for i in range(n):
            oenv.envs[i].space.heightmapC[:] = hm[i]
        oa = np.array([t % k] * n)
        oloc = _f32(oenv.get_action_candidates(oa))
        act = np.array([int(np.argmin(np.where(c.reshape(S, 5)[:, 4] == 1, c.reshape(S, 5)[:, 3], np.inf)))
                        if (c.reshape(S, 5)[:, 4] == 1).any() else 0 for c in oloc[:, :5 * S]])
        oord, _, odone, _ = oenv.step(act)
        for g in genvs:
            g.env.set_heightmaps(torch.from_numpy(hm).to(DEV))
            np.testing.assert_array_equal(g.get_action_candidates(oa).cpu().numpy(), oloc, err_msg=f"round {t}")
            gord, _, gdone, _ = g.step(act)
            np.testing.assert_array_equal(gord.cpu().numpy(), _f32(oord))
            np.testing.assert_array_equal(gdone, odone)
    for g in genvs:
        g.env.check_device_error()
        g.close()


def test_buffered_placements_candidate_launches():
    """k = 3, 2 bins, 10 placements: the MODE_CANDS launches of a buffered environment, both forms, against the C oracle."""
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    seqs = synthetic.make_sequences(sh.n_shapes, 64, 150, seed=5)
    n, k = 2, 3
    genvs = [GpuVecEnv(sh, seqs, n, device=DEV, bufferSize=k, tuning=f) for f in (0, PACK)]
    for g in genvs:
        g.candidates_on_device = True
    cenv = COracleVecEnv(n, sh, seqs, bufferSize=k)
    want0 = _f32(cenv.reset())
    for g in genvs:
        np.testing.assert_array_equal(g.reset().cpu().numpy(), want0)
    for t in range(10):
        order = (np.arange(n) * 5 + t) % k
        cloc = _f32(cenv.get_action_candidates(order))
        act = np.array([int(np.argmin(np.where(c.reshape(S, 5)[:, 4] == 1, c.reshape(S, 5)[:, 3], np.inf)))
                        if (c.reshape(S, 5)[:, 4] == 1).any() else 0 for c in cloc[:, :5 * S]])
        cobs, _, cdone, _ = cenv.step(act)
        for g in genvs:
            np.testing.assert_array_equal(g.get_action_candidates(order).cpu().numpy(), cloc, err_msg=f"location obs, placement {t}")
            gobs, _, gdone, _ = g.step(act)
            np.testing.assert_array_equal(gobs.cpu().numpy(), _f32(cobs), err_msg=f"placement {t}")
            np.testing.assert_array_equal(gdone, cdone)
    for g in genvs:
        g.env.check_device_error()
        g.close()
