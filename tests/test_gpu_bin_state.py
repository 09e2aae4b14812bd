"""Save, restore and fork bins on the device (irbpp_save_bins / irbpp_load_bins / irbpp_copy_bins; vec_env.save_bins, load_bins,
fork_bins, GpuVecEnv.save_state / load_state) against the numpy oracle on every pipeline.

The oracle side of a fork is ``copy.deepcopy`` of the source's PackingGame with the item creator moved to the destination's
trajectory rows: the running episode goes on reading the source's row, the next one is trajectory
``traj_start + d + episode * bins`` of the destination's own index d.  Comparisons between two device bins (a fork and its
source, a restored environment and the one it was saved from) and with the oracle are exact: observations after the oracle's
float32 cast, rewards, the episode's reward sum and length, dones, counters, ratios, heightmaps and the per-bin totals in
float64."""
import copy

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from irbpp_amd.vec_env import BinBlob, GpuPackingEnv, GpuVecEnv, GroupedPackingEnv
from cell_step_helpers import OracleCellEnv, f32, scenario

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
eq = np.testing.assert_array_equal


class Oracle(OracleCellEnv):
    """OracleCellEnv over bins 0 .. n-1 plus row steps, forks and the per-bin totals the device keeps."""

    def __init__(self, n, shapes, seqs, **kw):
        super().__init__(range(n), n, shapes, seqs, **kw)
        self.n = n
        self.ep_r = np.zeros(n)                  # running sum of the episode's rewards (BinState::ep_reward)
        self.ep_l = np.zeros(n, dtype=np.int64)  # steps of the episode (BinState::ep_len)
        self.totals = np.zeros((n, 4))           # State::totals: episodes, sum ratio, sum counter, sum reward

    def _book(self, rews, dones, infos):
        for i in range(self.n):
            self.ep_r[i] += rews[i]
            self.ep_l[i] += 1
            if dones[i]:
                infos[i]["ep_reward"], infos[i]["ep_len"] = self.ep_r[i], int(self.ep_l[i])
                self.totals[i] += (1.0, infos[i]["ratio"], infos[i]["counter"], self.ep_r[i])
                self.ep_r[i], self.ep_l[i] = 0.0, 0

    def step(self, actions):
        obs, rews, dones, infos = [], [], [], []
        for i, (e, a) in enumerate(zip(self.envs, actions)):
            o, r, d, info = e.step(int(a))
            if d:
                o = e.reset()
            obs.append(o); rews.append(r); dones.append(d); infos.append(info)
        self._book(rews, dones, infos)
        return np.array(obs), np.array(rews), np.array(dones), infos

    def step_cells(self, cells):
        out = super().step_cells(cells)
        self._book(out[1], out[2], out[3])
        return out

    def fork(self, src, dst, src_oracle=None):
        so = self if src_oracle is None else src_oracle
        games = []
        for s, d in zip(src, dst):
            g = copy.deepcopy(so.envs[s], {id(so.envs[s].shapes): so.envs[s].shapes})
            ic = g.item_creator
            episode = (ic.traj_index - 1 - s) // so.n          # (traj_start = 1)
            ic.traj_index, ic.stride = 1 + d + episode * self.n, self.n
            games.append((d, g, so.ep_r[s], so.ep_l[s]))
        for d, g, r, l in games:
            self.envs[d], self.ep_r[d], self.ep_l[d] = g, r, l

    def device_totals(self):
        """irbpp_totals_kernel's sum of the bins' totals (n <= 64: lane b holds bin b, a butterfly over the wave)"""
        v = np.zeros((64, 4))
        v[:self.n] = self.totals
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[np.arange(64) ^ o]
        return v[0]


class Twin(object):
    """A GpuPackingEnv and the oracle, stepped together and compared after every call."""

    def __init__(self, shapes, seqs, n, **kw):
        self.n, self.K = n, kw.get("bufferSize", 1)
        self.g = GpuPackingEnv(shapes, seqs, n, device=DEV, **kw)
        self.o = Oracle(n, shapes, seqs, **kw)
        self.obs = self.g.reset()
        eq(self.obs.cpu().numpy(), f32(self.o.reset()))
        self.loc = None
        self.dones = np.zeros(n, dtype=np.int64)
        self.last = None

    def _compare(self, oobs, orew, odone, oinfo):
        h = self.g.step_info_host()
        eq(self.obs.cpu().numpy(), f32(oobs))
        eq(h["done"], odone)
        eq(h["reward"], orew)
        for i in np.nonzero(odone)[0]:
            assert h["counter"][i] == oinfo[i]["counter"] and h["ratio"][i] == oinfo[i]["ratio"]
            assert h["ep_reward"][i] == oinfo[i]["ep_reward"] and h["ep_len"][i] == oinfo[i]["ep_len"]
        eq(self.g.get_heightmaps().cpu().numpy(), self.o.heightmaps())
        self.dones += odone
        self.last = h

    def candidates(self, order):
        self.order = np.asarray(order, dtype=np.int32)
        self.loc = self.g.get_action_candidates(torch.from_numpy(self.order).to(DEV))
        eq(self.loc.cpu().numpy(), f32(self.o.get_action_candidates(self.order)))

    def step(self):
        act = self.g.policy_minz(self.obs if self.K == 1 else self.loc)
        self.obs, _, _ = self.g.step(act)
        self.acts = act.cpu().numpy()
        self._compare(*self.o.step(self.acts))

    def play(self, steps, t0=0):
        for t in range(t0, t0 + steps):
            if self.K > 1:
                self.candidates([(t * 7 + 3 + i) % self.K for i in range(self.n)])
            self.step()

    def fork(self, src, dst, obs):
        self.g.fork_bins(src, dst, obs=obs)
        self.o.fork(src, dst)

    def bin_totals(self, bins=None):
        """State::totals of the listed bins (all by default), float64[len, 4]: the last segment of a saved bin's row when no
        placement log is attached (irbpp_binstate.h; tests/test_bin_state_cpu.py pins the order)"""
        bins = list(range(self.n)) if bins is None else list(bins)
        data = self.g.save_bins(bins).data
        return data[:, -32:].contiguous().view(torch.float64).cpu().numpy()

    def close(self):
        eq(self.bin_totals(), self.o.totals)                       # per bin, not only their sum
        eq(self.g.episode_totals().cpu().numpy(), self.o.device_totals())
        self.g.check_device_error()
        self.g.close()


def cut(seqs, lo=3, hi=10, seed=7):
    """trajectories of lo .. hi items (the rest is the exhausted-trajectory sentinel): episodes end within a few steps"""
    rng = np.random.RandomState(seed)
    seqs = seqs.copy()
    for row in seqs:
        row[rng.randint(lo, hi + 1):] = -1
    return seqs


def blockout():
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    return sh, synthetic.make_sequences(sh.n_shapes, 40, 60, seed=5)


# ---- 1 / 2: a fork continues like its source, then as its own bin, on every pipeline ----
def _fork_online(shapes, seqs, n, src, dst, before, after, **kw):
    tw = Twin(shapes, seqs, n, **kw)
    tw.play(before)
    totals = tw.bin_totals()
    tw.fork(src, dst, tw.obs)
    eq(tw.bin_totals(), totals)                                      # a fork moves no totals: every bin's own, the destinations' too
    eq(tw.bin_totals(dst), tw.o.totals[dst])
    eq(tw.obs[dst].cpu().numpy(), tw.obs[src].cpu().numpy())
    together = np.ones(len(src), dtype=bool)                         # the pair is still in the forked episode
    for t in range(after):
        tw.step()
        h = tw.last
        eq(tw.acts[dst][together], tw.acts[src][together])           # forked bins get the same actions as their sources
        for key in ("reward", "done", "counter", "ratio", "ep_reward", "ep_len"):
            eq(h[key][dst][together], h[key][src][together])
        together &= ~h["done"][src]
        o, hm = tw.obs.cpu().numpy(), tw.g.get_heightmaps().cpu().numpy()
        eq(hm[dst][together], hm[src][together])
        eq(o[dst][together], o[src][together])
    dones = tw.dones.copy()
    tw.close()
    return dones


def test_fork_continues_like_its_source_online():
    sh, seqs = blockout()
    dones = _fork_online(sh, cut(seqs), 8, [0, 1, 2], [5, 6, 7], 7, 12)
    assert (dones[[5, 6, 7]] >= 1).all() and dones.sum() >= 8         # whole episodes of the forked bins' own were covered


@pytest.mark.parametrize("name", ["r8", "box", "wide32", "levels60"])
def test_fork_on_the_other_pipelines(name):
    """Trajectories of at most 10 items: the forked episode, begun before the fork, ends within the 12 steps behind it at the
    latest, so every destination bin starts an episode of its own on every pipeline."""
    sh, seqs, kw = scenario(name, n_traj=40, length=60)
    n = 4 if name == "wide32" else 8
    src, dst = ([0, 1], [3, 2]) if n == 4 else ([0, 1, 2], [5, 6, 7])
    dones = _fork_online(sh, cut(seqs), n, src, dst, 7, 12, **kw)
    assert (dones[dst] >= 1).all()


def test_fork_buffered():
    """bufferSize = 3: a fork between get_action_candidates and step (the location observation, the candidate keys, the chosen
    slot and the stored grids travel), and one right after a step (the queue travels; the grids are not current)."""
    sh, seqs = blockout()
    tw = Twin(sh, seqs, 8, bufferSize=3)
    src, dst = [0, 1, 2], [5, 6, 7]
    tw.play(5)
    assert tw.g.bin_blob_info()["grids_current"] == 0                # a buffered step observes nothing
    tw.candidates([(i + 1) % 3 for i in range(8)])
    assert tw.g.bin_blob_info()["grids_current"] == 1
    tw.fork(src, dst, tw.loc)
    assert tw.g.bin_blob_info()["grids_current"] == 1
    tw.step()                                                        # pops the COPIED slot of the copied queue
    eq(tw.obs[dst].cpu().numpy(), tw.obs[src].cpu().numpy())         # order observation: queue + heightmap
    eq(tw.acts[dst], tw.acts[src])
    tw.play(4, t0=6)
    tw.fork(src, dst, tw.obs)                                        # right after a step
    assert tw.g.bin_blob_info()["grids_current"] == 0
    order = [(i + 2) % 3 for i in range(8)]
    for s, d in zip(src, dst):
        order[d] = order[s]
    tw.candidates(order)
    eq(tw.loc[dst].cpu().numpy(), tw.loc[src].cpu().numpy())
    tw.step()
    eq(tw.obs[dst].cpu().numpy(), tw.obs[src].cpu().numpy())
    tw.play(8, t0=11)
    tw.close()


# ---- 3: the stored grids travel ----
def test_stored_grids_travel():
    sh, seqs = blockout()
    tw = Twin(sh, seqs, 8)
    src, dst = [0, 1, 2], [5, 6, 7]
    tw.play(6)
    tw.fork(src, dst, tw.obs)
    for _ in range(3):                                               # no fresh observation between the fork and the first of them
        cells = tw.o.heuristic_cells("DBLF", 3)
        tw.obs, _, _ = tw.g.heuristic_step("DBLF", 3)
        tw._compare(*tw.o.step_cells(cells))
        eq(tw.obs[dst].cpu().numpy()[:, :5 * tw.g.S], tw.obs[src].cpu().numpy()[:, :5 * tw.g.S])
    # set_heightmaps clears the SOURCE environment's grids: after a fork from it the destination's are not current either
    other = Twin(sh, seqs, 8)
    other.play(4)
    other.g.set_heightmaps(other.g.get_heightmaps())
    assert other.g.bin_blob_info()["grids_current"] == 0
    tw.g.fork_bins(src, dst, src_env=other.g, obs=tw.obs, src_obs=other.obs)
    tw.o.fork(src, dst, src_oracle=other.o)
    with pytest.raises(_lib.IrbppError, match="out of order"):
        tw.g.heuristic_step("DBLF", 3)
    cells = tw.o.heuristic_cells("MINZ", 0)                          # step_cells still plays: drop heights from the bottom cells
    tw.obs, _, _ = tw.g.step_cells(torch.from_numpy(cells).to(DEV))
    tw._compare(*tw.o.step_cells(cells))
    tw.play(3)
    other.close()
    tw.close()


# ---- 4: look-ahead: every root bin forked into B search bins of a second environment ----
def test_cross_environment_fork_look_ahead():
    sh, seqs = blockout()
    n, B = 4, 6
    root = Twin(sh, seqs, n)
    root.play(6)
    search = Twin(sh, seqs, n * B)
    search.play(2)                                                   # (its bins are somewhere else entirely)
    hm0, obs0 = root.g.get_heightmaps().cpu().numpy(), root.obs.cpu().numpy().copy()
    src = np.repeat(np.arange(n), B)
    dst = np.arange(n * B)
    search.g.fork_bins(src, dst, src_env=root.g, obs=search.obs, src_obs=root.obs)
    search.o.fork(src, dst, src_oracle=root.o)
    rows = root.obs[:, :5 * root.g.S].reshape(n, root.g.S, 5).cpu().numpy()
    act = np.zeros(n * B, dtype=np.int32)
    for b in range(n):
        valid = np.nonzero(rows[b, :, 4] == 1)[0][:B]                # the first six valid candidate rows, or fewer
        assert len(valid) >= 2
        act[b * B:b * B + len(valid)] = valid
        act[b * B + len(valid):(b + 1) * B] = valid[-1]
    search.obs, _, _ = search.g.step(torch.from_numpy(act).to(DEV))
    search._compare(*search.o.step(act))                             # reward, done, heightmap of a fresh oracle copy of the root
    eq(root.g.get_heightmaps().cpu().numpy(), hm0)                   # the root is untouched ...
    eq(root.obs.cpu().numpy(), obs0)
    root.play(2)                                                     # ... in its next observations too
    search.play(2)
    search.close()
    root.close()


# ---- 5: save, load, checkpoint ----
def _infos(infos):
    """``infos`` without the wall-clock field episode['t']"""
    out = []
    for i in infos:
        i = dict(i)
        if "episode" in i:
            i["episode"] = {k: v for k, v in i["episode"].items() if k != "t"}
        out.append(i)
    return out


@pytest.mark.parametrize("log", [False, True])
def test_checkpoint_and_resume(tmp_path, log):
    sh, seqs = blockout()
    seqs = cut(seqs, 4, 12)
    n = 6

    def make():
        env = GpuVecEnv(sh, seqs, n, device=DEV)
        logs = env.env.enable_placement_log(32) if log else None
        return env, logs

    def run(env, obs, steps):
        out = []
        for _ in range(steps):
            obs, rew, done, infos = env.step(env.env.policy_minz(obs))
            out.append((obs.cpu().numpy().copy(), rew.numpy().copy(), done.copy(), _infos(infos)))
        return out, obs

    env, logs = make()
    _, obs = run(env, env.reset(), 9)
    env.save_state(obs).to_file(tmp_path / "envs.pt")
    want, _ = run(env, obs, 10)
    want_totals = env.env.episode_totals().cpu().numpy()
    want_logs = [t.cpu().numpy().copy() for t in logs] if log else None
    assert sum(int(w[2].sum()) for w in want) >= 3
    env.close()

    env, logs = make()
    env.reset()
    obs = env.load_state(BinBlob.from_file(tmp_path / "envs.pt", DEV))
    got, _ = run(env, obs, 10)
    for w, g in zip(want, got):
        eq(g[0], w[0]); eq(g[1], w[1]); eq(g[2], w[2])
        assert g[3] == w[3]
    eq(env.env.episode_totals().cpu().numpy(), want_totals)
    if log:
        for t, w in zip(logs, want_logs):
            eq(t.cpu().numpy(), w)
    env.env.check_device_error()
    env.close()


# ---- 6: refusals ----
def test_refusals():
    sh, seqs = blockout()
    env = GpuPackingEnv(sh, seqs, 4, device=DEV)
    with pytest.raises(_lib.IrbppError, match="out of order"):       # before reset
        env.fork_bins([0], [1])
    with pytest.raises(_lib.IrbppError, match="out of order"):
        env.save_bins([0])
    obs = env.reset()
    for _ in range(3):
        obs, _, _ = env.step(env.policy_minz(obs))
    blob = env.save_bins([0, 2])
    assert blob.data.shape == (2, blob.info["bytes_per_bin"]) and blob.info["version"] == 1

    def refused(shapes, sequences, b=blob, **kw):
        e = GpuPackingEnv(shapes, sequences, 4, device=DEV, **kw)
        e.reset()
        with pytest.raises(_lib.IrbppError, match="bad argument"):
            e.load_bins([0, 2], b)
        with pytest.raises(_lib.IrbppError, match="bad argument"):
            e.fork_bins([0], [1], src_env=env)
        e.close()

    refused(synthetic.blockout_shapes(n_shapes=24, n_rot=8, cube=0.06, seed=0), seqs)        # R = 4 into R = 8
    changed = copy.deepcopy(sh)
    T, B, mH, mB = changed.tables[3][1]
    T = T.copy()
    T[T > 0] += 0.01
    changed.tables[3][1] = (T, B, mH, mB)
    refused(changed, seqs)                                           # one shape table changed
    seqs2 = seqs.copy()
    seqs2[17, 30] = (seqs2[17, 30] + 1) % sh.n_shapes
    refused(sh, seqs2)                                               # one sequence id changed
    edited = BinBlob(dict(blob.info, version=2), blob.data)
    with pytest.raises(_lib.IrbppError, match="bad argument"):
        env.load_bins([0, 2], edited)
    env.load_bins([1, 3], blob)                                      # (the unedited blob loads, into other bins too)
    hm = env.get_heightmaps().cpu().numpy()
    eq(hm[1], hm[0]); eq(hm[3], hm[2])

    with pytest.raises(ValueError, match="distinct"):
        env.fork_bins([0, 1], [2, 2])
    with pytest.raises(ValueError, match="both"):
        env.fork_bins([0, 1], [1, 2])
    with pytest.raises(ValueError, match="outside"):
        env.fork_bins([0], [4])
    env.fork_bins([1, 0], [1, 3])                                    # a bin paired with itself is a no-op
    env.check_device_error()
    hm = env.get_heightmaps().cpu().numpy()
    eq(hm[3], hm[0])
    env.fork_bins([0, 4, 2], [1, 2, 3], validate=False)              # a source index == N: that pair is skipped, the others are served
    hm2 = env.get_heightmaps().cpu().numpy()
    eq(hm2[1], hm[0]); eq(hm2[3], hm[2]); eq(hm2[2], hm[2])
    with pytest.raises(_lib.IrbppError, match="BAD_BIN"):
        env.check_device_error()
    env.close()

    ring = synthetic.make_sequences(sh.n_shapes, 4, 64, seed=3)
    stream = GpuPackingEnv(sh, ring, 4, device=DEV, item_stream=1)
    stream.reset()
    with pytest.raises(_lib.IrbppError, match="bad argument"):
        stream.save_bins([0])
    with pytest.raises(_lib.IrbppError, match="bad argument"):
        stream.load_bins([0, 2], blob)
    with pytest.raises(_lib.IrbppError, match="bad argument"):
        stream.fork_bins([0], [1])
    stream.close()


# ---- 7: launch sizes beyond one round, cross-group pairs ----
def test_fork_4096_bins_across_groups():
    sh, seqs = blockout()
    n, half = 4096, 2048
    env = GroupedPackingEnv(sh, seqs, n, 2, device=DEV)
    twin = GpuPackingEnv(sh, seqs, half, device=DEV, global_bins=n)  # the lower half, never forked
    obs, tobs = env.reset(), twin.reset()
    for _ in range(5):
        obs = env.step(env.policy_minz(obs))
        env.synchronize()
        tobs, _, _ = twin.step(twin.policy_minz(tobs))
    low, up = np.arange(half), np.arange(half, n)
    env.fork_bins(low, up, obs=obs)                                  # every pair crosses from group 0 to group 1
    env.synchronize()                                                # (row block g of obs belongs to stream g, as after a step)
    together = np.ones(half, dtype=bool)                             # the pair is still in the forked episode
    for _ in range(3):
        obs = env.step(env.policy_minz(obs))
        h = env.step_info_host()
        tobs, _, _ = twin.step(twin.policy_minz(tobs))
        th = twin.step_info_host()
        for key in ("reward", "done", "counter", "ratio", "ep_reward", "ep_len"):
            eq(h[key][half:][together], h[key][:half][together])
        together &= ~h["done"][:half]                                # a bin that finished the forked episode is on its own rows
        o, hm = obs.cpu().numpy(), env.get_heightmaps().cpu().numpy()
        eq(hm[half:][together], hm[:half][together])
        eq(o[half:][together], o[:half][together])
        eq(o[:half], tobs.cpu().numpy())                             # the lower half of the whole launch == the never-forked twin
        for key in ("reward", "done", "counter", "ratio"):
            eq(h[key][:half], th[key])
    assert together.sum() > half // 2
    env.check_device_error()
    env.close()
    twin.close()


def test_grouped_save_and_load_put_the_bins_back():
    """GroupedPackingEnv.save_bins / load_bins with global indices in any order: after the load the same actions give the same
    outputs again."""
    sh, seqs = blockout()
    env = GroupedPackingEnv(sh, cut(seqs), 8, 2, device=DEV)
    obs = env.reset()
    for _ in range(4):
        obs = env.step(env.policy_minz(obs))
        env.synchronize()
    bins = [6, 1, 4, 3, 0, 7, 2, 5]
    blob = env.save_bins(bins)
    saved_obs, totals = obs.clone(), env.episode_totals().cpu().numpy()

    def play(obs):
        out = []
        for _ in range(5):
            obs = env.step(env.policy_minz(obs))
            h = env.step_info_host()
            out.append((obs.cpu().numpy().copy(), h, env.get_heightmaps().cpu().numpy()))
        return out, env.episode_totals().cpu().numpy()

    want, want_totals = play(saved_obs)
    assert sum(int(w[1]["done"].sum()) for w in want) >= 2 and (want_totals != totals).any()
    env.load_bins(bins, blob)
    eq(env.episode_totals().cpu().numpy(), totals)                   # a load restores the totals as well
    got, got_totals = play(saved_obs)
    for w, g in zip(want, got):
        eq(g[0], w[0]); eq(g[2], w[2])
        for key in w[1]:
            eq(g[1][key], w[1][key])
    eq(got_totals, want_totals)
    env.check_device_error()
    env.close()
