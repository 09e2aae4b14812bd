"""The trainer's logged episode metrics kept on the device (irbpp_amd.metrics.EpisodeMetrics) against a literal copy of the
trainer's own deque loop (trainer.py:145-147, 168-178, 215-222) fed with the per-step infos of the same run: every row bit for
bit, for online, buffered and capacity-path configurations, grouped and sharded bins, graph replay, detaching and refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib
from irbpp_amd.metrics import EpisodeMetrics, EpisodeMetricsOverrun
from irbpp_amd.vec_env import GpuPackingEnv, GroupedPackingEnv, _Infos
from episode_window_model import assert_rows_equal, trainer_rows
from helpers import _bench_workload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _play(env, metrics, steps, read_every=50, buffered=False, host_infos=True):
    """MINZ roll-out; (device rows, host (done, infos) per step)."""
    obs = env.reset()
    order = torch.zeros((env.num_bins,), dtype=torch.int32, device=DEV)
    host, rows = [], []
    for T in range(1, steps + 1):
        loc = env.get_action_candidates(order) if buffered else obs
        res = env.step(env.policy_minz(loc))
        obs = res[0] if isinstance(res, tuple) else res
        if isinstance(env, GroupedPackingEnv):
            env.synchronize()
        if host_infos:
            h = env.step_info_host()
            host.append((h["done"], _Infos(h, 0.0)))
        if T % read_every == 0:
            rows.append(metrics.read())
    rows.append(metrics.read())
    return np.concatenate(rows), host


@pytest.mark.parametrize("workload,extra", [("blockout", {}), ("general", {}), ("general", {"resolutionA": 0.01})])
def test_rows_equal_the_trainer_loop(workload, extra):
    shapes, seqs, kw = _bench_workload(workload)
    kw = dict(kw, **extra)
    env = GpuPackingEnv(shapes, seqs, 1024, device=DEV, **kw)
    for W in (1, 10, 37, 128, 1000):
        m = EpisodeMetrics(env, window=W, history=64)
        rows, host = _play(env, m, 200)
        want = trainer_rows(host, W)
        assert rows.shape[0] == 200 and np.array_equal(rows[:, 0], np.arange(1, 201))
        assert want[-1, 1] == min(W, sum(int(d.sum()) for d, _ in host)) and want[-1, 1] > 0
        assert_rows_equal(rows, want)
        m.close()
    env.check_device_error()
    env.close()


def test_rows_equal_the_trainer_loop_beyond_a_workgroup_of_bins():
    """2560 bins: every thread of the update kernel's one workgroup owns a segment of three bins (seg = 3), 854 threads hold
    bins (the last of them one bin only) and 170 none."""
    shapes, seqs, kw = _bench_workload("blockout")
    env = GpuPackingEnv(shapes, seqs, 2560, device=DEV, **kw)
    for W in (10, 1000):
        m = EpisodeMetrics(env, window=W, history=64)
        rows, host = _play(env, m, 120)
        want = trainer_rows(host, W)
        assert rows.shape[0] == 120 and np.array_equal(rows[:, 0], np.arange(1, 121))
        assert want[-1, 1] == min(W, sum(int(d.sum()) for d, _ in host)) and want[-1, 1] > 0
        assert_rows_equal(rows, want)
        m.close()
    env.check_device_error()
    env.close()


def test_reading_after_more_than_history_steps_raises():
    shapes, seqs, kw = _bench_workload("blockout")
    env = GpuPackingEnv(shapes, seqs, 256, device=DEV, **kw)
    m = EpisodeMetrics(env, window=10, history=64)
    obs = env.reset()
    for _ in range(64):
        obs, _, _ = env.step(env.policy_minz(obs))
    assert m.read().shape == (64, 7)                     # exactly H steps: all still there
    for _ in range(65):
        obs, _, _ = env.step(env.policy_minz(obs))
    with pytest.raises(EpisodeMetricsOverrun):
        m.read()
    for _ in range(3):
        obs, _, _ = env.step(env.policy_minz(obs))
    rows = m.read()                                      # goes on after the steps that read covered
    assert np.array_equal(rows[:, 0], [129, 130, 131, 132])
    m.reset()
    assert m.steps_recorded() == 0
    env.step(env.policy_minz(obs))
    rows = m.read()
    assert rows.shape == (1, 7) and rows[0, 0] == 1
    m.close()
    env.close()


@pytest.mark.parametrize("groups", [2, 4])
def test_groups_and_shards_give_the_rows_of_one_env(groups):
    shapes, seqs, kw = _bench_workload("blockout")
    W, steps = 37, 150
    one = GpuPackingEnv(shapes, seqs, 1024, device=DEV, **kw)
    m1 = EpisodeMetrics(one, window=W, history=64)
    want, host = _play(one, m1, steps)
    assert_rows_equal(want, trainer_rows(host, W))
    grouped = GroupedPackingEnv(shapes, seqs, 1024, num_groups=groups, device=DEV, **kw)
    mg = EpisodeMetrics(grouped, window=W, history=64)
    got, _ = _play(grouped, mg, steps, host_infos=False)
    assert_rows_equal(got, want)
    # shards of one process: global_offset, merged by irbpp_episode_metrics like ranks
    per = 1024 // groups
    shards = [GpuPackingEnv(shapes, seqs, per, device=DEV, global_offset=r * per, global_bins=1024, **kw) for r in range(groups)]
    ms = EpisodeMetrics(shards, window=W, history=64)
    obs = [s.reset() for s in shards]
    rows = []
    for T in range(1, steps + 1):
        obs = [s.step(s.policy_minz(o))[0] for s, o in zip(shards, obs)]
        if T % 50 == 0:
            rows.append(ms.read())
    assert_rows_equal(np.concatenate(rows), want)
    for e in [one, grouped] + shards:
        e.close()


def test_buffered_hierarchical_loop():
    shapes, seqs, kw = _bench_workload("blockout_k10")
    env = GpuPackingEnv(shapes, seqs, 512, device=DEV, **kw)
    m = EpisodeMetrics(env, window=10, history=64)
    rows, host = _play(env, m, 150, buffered=True)
    assert_rows_equal(rows, trainer_rows(host, 10))
    assert np.nanmax(rows[:, 1]) == 10
    env.close()


def test_graph_replay_keeps_the_window():
    shapes, seqs, kw = _bench_workload("blockout")
    env = GpuPackingEnv(shapes, seqs, 512, device=DEV, tuning=_lib.TUNE_GRAPH, **kw)
    m = EpisodeMetrics(env, window=10, history=64)
    rows, host = _play(env, m, 120)
    assert_rows_equal(rows, trainer_rows(host, 10))
    env.close()


def test_refusals_and_detaching():
    shapes, seqs, kw = _bench_workload("blockout")
    a = GpuPackingEnv(shapes, seqs, 256, device=DEV, **kw)
    b = GpuPackingEnv(shapes, seqs, 256, device=DEV, **kw)
    m = EpisodeMetrics(a, window=10, history=64)
    lib, st = a.lib, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    oa, ob = a.reset(), b.reset()
    act = a.policy_minz(oa)
    spare = torch.empty_like(oa)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                   # noqa: E731
    assert lib.irbpp_step(a._h, ptr(act), ptr(spare), None, st) == -1          # attached: a step without outputs is refused
    part = _lib.IrbppStepOut(done_dev=a._step_out.done_dev)
    assert lib.irbpp_step(a._h, ptr(act), ptr(spare), C.byref(part), st) == -1
    bad = _lib.IrbppEpisodeWindow(window=1025, history=4)
    assert lib.irbpp_set_episode_window(a._h, C.byref(bad)) == -1
    s = m._structs[0]
    arr = (_lib.IrbppEpisodeWindow * 1)(s)
    out = torch.empty((65, 7), dtype=torch.float64, device=DEV)
    assert lib.irbpp_episode_metrics(arr, 1, 1, 65, ptr(out), st) == -1       # more steps than the history holds
    for t in range(40):
        if t == 20:
            m.close()                                                          # detached: no launch from here on
        oa, _, _ = a.step(a.policy_minz(oa))
        ob, _, _ = b.step(b.policy_minz(ob))
        ha, hb = a.step_info_host(), b.step_info_host()
        assert torch.equal(oa, ob)
        for k in ha:
            assert np.array_equal(ha[k], hb[k]), k
    assert m.steps_recorded() == 20
    assert lib.irbpp_step(a._h, ptr(a.policy_minz(oa)), ptr(spare), None, st) == 0   # detached: outputs optional again
    torch.cuda.synchronize()
    a.close()
    b.close()


_RCCL = r"""
import os, sys, json
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, torch
from irbpp_amd import distributed as D
from irbpp_amd.metrics import EpisodeMetrics
from irbpp_amd.vec_env import GpuPackingEnv
from helpers import _bench_workload
rank, world, local = D.init_from_env("nccl", force=True)
torch.cuda.set_device(local)
dev = "cuda:%%d" %% local
shapes, seqs, kw = _bench_workload("blockout")
envs = [GpuPackingEnv(shapes, seqs, 1024, device=dev, **kw) for _ in range(2)]
ms = [EpisodeMetrics(e, window=10, history=256) for e in envs]
obs = [e.reset() for e in envs]
for _ in range(150):
    obs = [e.step(e.policy_minz(o))[0] for e, o in zip(envs, obs)]
local_rows, gathered_rows = ms[0].read(), ms[1].read(group=True)
ok = local_rows.shape == gathered_rows.shape and np.array_equal(np.nan_to_num(local_rows), np.nan_to_num(gathered_rows))
print(json.dumps({"ok": bool(ok), "rows": int(local_rows.shape[0]), "n_last": float(local_rows[-1, 1]),
                  "backend": torch.distributed.get_backend()}))
torch.distributed.destroy_process_group()
""" % (ROOT, ROOT)


def test_single_rank_rccl_read():
    import json
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    res = subprocess.run([sys.executable, "-c", _RCCL], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert out["ok"] and out["rows"] == 150 and out["n_last"] == 10 and out["backend"] == "nccl", out
