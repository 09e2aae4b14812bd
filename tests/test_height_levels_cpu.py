"""More than 31 height levels without a GPU: both oracles against episodes the reference's own PackingGame played at
resolutionZ = 0.005 (tests/golden/make_levels_golden.py: 60 levels on the 0.30 m bin), and irbpp_create's argument checks of
the level count (include/irbpp.h, Limits: up to 222 levels, the capacity path beyond 31)."""
import ctypes
import os

import numpy as np
import pytest

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, build, synthetic
from oracle.c_oracle import CPackingGame
from oracle.packing import PackingGame
from helpers import assert_fallback_rows_legal, minz_action

S = 500
RES_Z = 0.005


def levels_scenario(name):
    """Shape set and sequences of a recording of make_levels_golden.py (same seeds)."""
    if name == "online_levels60":
        sh = synthetic.general_shapes(n_shapes=16, n_rot=4, fmin=4, fmax=14, seed=3)
        return sh, synthetic.make_sequences(sh.n_shapes, 16, 80, seed=2)
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    return sh, synthetic.make_sequences(sh.n_shapes, 16, 150, seed=5)


def max_level(obs, res_z=RES_Z, s=S):
    """Highest level floor(H / resolutionZ) among the valid candidate rows of one or more observations."""
    obs = np.asarray(obs)
    rows = obs.reshape(-1, obs.shape[-1])[:, :5 * s].reshape(-1, 5)
    h = rows[rows[:, 4] == 1, 3].astype(np.float64)
    return int(np.floor_divide(h, res_z).max()) if h.size else -1


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def _oracle(kind, sh, seq, **kw):
    return (PackingGame(sh, seq, selectedAction=S, resolutionZ=RES_Z, **kw) if kind == "numpy"
            else CPackingGame(sh, seq, selectedAction=S, resolutionZ=RES_Z, **kw))


def test_goldens_reach_levels_beyond_31(golden_dir):
    g = _load(golden_dir, "online_levels60")
    assert max_level(g["obs"]) > 31 and g["done"].sum() >= 1
    np.testing.assert_array_equal(g["seq"], levels_scenario("online_levels60")[1])
    h = _load(golden_dir, "hier_levels60_k3")
    assert max_level(h["loc_obs"]) > 31 and h["done"].sum() >= 1
    np.testing.assert_array_equal(h["seq"], levels_scenario("hier_levels60_k3")[1])


@pytest.mark.parametrize("kind", ["numpy", "c"])
def test_oracles_replay_the_online_golden(golden_dir, kind):
    g = _load(golden_dir, "online_levels60")
    sh, _ = levels_scenario("online_levels60")
    env = _oracle(kind, sh, g["seq"], bufferSize=1)
    obs = env.reset()
    np.testing.assert_array_equal(obs, g["obs"][0])
    rewards = []
    for t in range(len(g["act"])):
        a = minz_action(obs, S)
        assert a == g["act"][t]
        obs, r, d, info = env.step(a)
        rewards.append(r)
        assert r == g["rew"][t] and d == g["done"][t]
        if d:
            assert info["counter"] == g["counter"][t] and info["ratio"] == g["ratio"][t]
            assert round(sum(rewards), 6) == g["ep_r"][t]
            rewards = []
            obs = env.reset()
        np.testing.assert_array_equal(obs[5 * S:], g["obs"][t + 1][5 * S:])
        if (obs[:5 * S].reshape(S, 5)[:, 4] == 1).any():
            np.testing.assert_array_equal(obs, g["obs"][t + 1], err_msg=f"step {t}")
        else:   # fallback rows come from np.argsort of an all-equal vector: tie order unspecified
            assert_fallback_rows_legal(obs[:5 * S].reshape(S, 5), sh.n_rot)
        pz, mk = (env.space.posZmap, env.space.naiveMask) if kind == "numpy" else env.grids()
        np.testing.assert_array_equal(pz, g["posz"][t + 1])
        np.testing.assert_array_equal(mk, g["mask"][t + 1])


@pytest.mark.parametrize("kind", ["numpy", "c"])
def test_oracles_replay_the_hierarchical_golden(golden_dir, kind):
    g = _load(golden_dir, "hier_levels60_k3")
    sh, _ = levels_scenario("hier_levels60_k3")
    env = _oracle(kind, sh, g["seq"], bufferSize=3)
    np.testing.assert_array_equal(env.reset(), g["order_obs"][0])
    for t in range(len(g["act"])):
        loc = env.get_action_candidates(int(g["order_act"][t]))
        if (loc[:5 * S].reshape(S, 5)[:, 4] == 1).any():
            np.testing.assert_array_equal(loc, g["loc_obs"][t], err_msg=f"placement {t}")
        a = minz_action(loc, S)
        assert a == g["act"][t]
        order, r, d, info = env.step(a)
        assert r == g["rew"][t] and d == g["done"][t]
        if d:
            assert info["counter"] == g["counter"][t] and info["ratio"] == g["ratio"][t]
            order = env.reset()
        np.testing.assert_array_equal(order, g["order_obs"][t + 1])


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _cfg(bin_z, res_z, res_a=0.02):
    return _lib.IrbppConfig(num_bins=2, n_rot=4, selected=500, buffer_size=1, resolution_a=res_a, resolution_h=0.01,
                            resolution_z=res_z, bin=(ctypes.c_double * 3)(0.32, 0.32, bin_z), scale_z=100.0, traj_start=1)


def test_create_level_limits(lib):
    """222 levels is the most the capacity path codes (level + 32 <= 254 in a byte); more is IRBPP_ERR_ARG before any HIP
    call.  Deep-level configurations refused up to now (60 levels at resolutionZ = 0.005, 120 at 0.0025, a 0.60 m bin) pass the
    argument checks: without a GPU they then fail at the device (IRBPP_ERR_HIP), never with IRBPP_ERR_ARG."""
    h = ctypes.c_void_p()
    for bin_z, res_z in ((2.23, 0.01), (0.30, 0.001)):
        assert lib.irbpp_create(ctypes.byref(_cfg(bin_z, res_z)), ctypes.byref(h)) == -1, (bin_z, res_z)
    for bin_z, res_z, res_a in ((0.30, 0.005, 0.02), (0.30, 0.0025, 0.02), (0.60, 0.01, 0.02), (2.22, 0.01, 0.02), (0.30, 0.005, 0.01)):
        h = ctypes.c_void_p()
        rc = lib.irbpp_create(ctypes.byref(_cfg(bin_z, res_z, res_a)), ctypes.byref(h))
        assert rc != -1, (bin_z, res_z, res_a)
        if rc == 0:
            lib.irbpp_destroy(h)
    cfg = _cfg(0.30, 0.005)
    cfg.stability = 1                                        # no stability proxy on the capacity path
    assert lib.irbpp_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
