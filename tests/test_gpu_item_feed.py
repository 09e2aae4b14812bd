"""The device item generator (csrc/irbpp_itemgen.hip) and the device-fed item rings: ``DeviceItemStreams.draw`` against the
host generator element for element, ``irbpp_stream_refill`` against what the host feeder writes, and the protocol of
test_gpu_features.test_make_vec_envs_trains_on_the_reference_item_streams with ``args.item_feed = "device"``."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, itemgen, synthetic
from irbpp_amd.vec_env import GpuPackingEnv, GpuVecEnv, make_vec_envs
from oracle.packing import OracleVecEnv, RandomStreamItemCreator
from helpers import minz_action
from test_itemgen import _dicts, _episode_protocol
from test_itemgen_device_host import CALLS, SEEDS, STRUCTURES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 500
L = 64                                            # ring length of the refill tests

_host_rows = {}


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _host_stream(structure, seed):
    """sum(CALLS) items of the host generator for (structure, seed): drawn once, shared, never written to."""
    key = (structure, seed)
    if key not in _host_rows:
        groups, item_set = STRUCTURES[structure]
        row = itemgen.ItemStream(seed, groups, item_set).draw(sum(CALLS))
        row.setflags(write=False)
        _host_rows[key] = row
    return _host_rows[key]


@pytest.mark.parametrize("n_streams", [6, 67])                        # 67: seventeen workgroups, the last with three idle waves
@pytest.mark.parametrize("structure", sorted(STRUCTURES))
def test_device_draws_equal_the_host_generator(structure, n_streams):
    groups, item_set = STRUCTURES[structure]
    seeds = [(SEEDS[i % 4] + i // 4) % 2 ** 32 for i in range(n_streams)]        # the CPU test's seeds, then their neighbours
    ds = itemgen.DeviceItemStreams(seeds, groups, item_set, device=DEV)
    got = torch.cat([ds.draw(c) for c in CALLS], dim=1).cpu().numpy()
    want = np.stack([_host_stream(structure, s) for s in seeds])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ds.delivered().cpu().numpy(), np.full(n_streams, sum(CALLS)))
    ds.close()


def test_device_streams_equal_the_reference_creators_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "random_creators.npz"))
    inst, cate = _dicts(g)
    seed = int(g["seed"])
    n = g["stream_instance"].shape[1]
    seeds = [seed + rank for rank in range(4)]
    for groups, item_set, key in ((itemgen.instance_groups(inst), None, "stream_instance"),
                                  (itemgen.category_groups(cate), None, "stream_category"), (None, list(range(29)), "stream_pose")):
        ds = itemgen.DeviceItemStreams(seeds, groups, item_set, device=DEV)
        raw = torch.cat([ds.draw(7), ds.draw(n + 33)], dim=1).cpu().numpy()
        for rank in range(4):
            np.testing.assert_array_equal(_episode_protocol(raw[rank], n), g[key][rank])
        ds.close()


def _instance_dic():
    return {i: "%s_%d.obj" % (["tee", "ell", "bar", "zig"][i % 4], i // 4) for i in range(20)}


def _env_kw(k):
    return dict(resolutionA=0.02, resolutionH=0.01, resolutionZ=0.01, bin_dimension=np.round([0.32, 0.32, 0.30], 6),
                selectedAction=S, bufferSize=k, scale_z=100.0, item_stream=1)


def _table(env) -> np.ndarray:
    t = torch.empty((env.num_bins, L), dtype=torch.int32, device=env.device)
    _lib.check(env.lib.irbpp_stream_table(env._h, C.c_void_p(t.data_ptr()), env._stream()), "irbpp_stream_table")
    return t.cpu().numpy()


def _cursors(env, values=None) -> np.ndarray:
    t = torch.zeros((env.num_bins,), dtype=torch.int32, device=env.device) if values is None else \
        torch.tensor(values, dtype=torch.int32, device=env.device)
    _lib.check(env.lib.irbpp_stream_cursors(env._h, C.c_void_p(t.data_ptr()), 0 if values is None else 1, env._stream()),
               "irbpp_stream_cursors")
    return t.cpu().numpy()


@pytest.mark.parametrize("k", [1, 3])
def test_refills_write_what_the_host_feeder_writes(k):
    """Two environments over the same streams and the same actions, one fed by StreamFeeder, one by DeviceStreamFeeder:
    the first refill fills the ring, a refill with nothing consumed writes nothing, and after a run of steps (the
    feeders refill on their own cadence, then once more by hand) rings, cursors and delivered counts are the same."""
    sh = synthetic.blockout_shapes(n_shapes=20, n_rot=4, cube=0.06, seed=7)
    groups = itemgen.instance_groups(_instance_dic())
    n, seed = 6, 321
    seeds = [seed + i for i in range(n)]
    hf = itemgen.StreamFeeder([itemgen.ItemStream(s, groups) for s in seeds], ring_len=L, buffer_size=k)
    df = itemgen.DeviceStreamFeeder(itemgen.DeviceItemStreams(seeds, groups, device=DEV), ring_len=L, buffer_size=k)
    assert (df.initial == -1).all() and df.every == hf.every
    first = hf.initial.copy()
    a = GpuVecEnv(sh, hf.initial, n, device=DEV, feeder=hf, obs_ring=0, **_env_kw(k))
    b = GpuVecEnv(sh, df.initial, n, device=DEV, feeder=df, obs_ring=0, **_env_kw(k))
    np.testing.assert_array_equal(_table(b.env), first)                # the first refill filled every ring
    np.testing.assert_array_equal(df.delivered(), np.full(n, L))
    df.refill()                                                        # nothing consumed: nothing written
    np.testing.assert_array_equal(_table(b.env), first)
    np.testing.assert_array_equal(df.delivered(), np.full(n, L))
    a.candidates_on_device = b.candidates_on_device = True
    oa, ob = a.reset(), b.reset()
    assert torch.equal(oa, ob)
    for t in range(90):
        if k > 1:
            order = (np.arange(n) + t) % k
            la, lb = a.get_action_candidates(order), b.get_action_candidates(order)
            assert torch.equal(la, lb)
            loc = la.cpu().numpy()
        else:
            loc = oa.cpu().numpy()
        act = np.array([minz_action(o, S) for o in loc])
        oa, ob = a.step(act)[0], b.step(act)[0]
        assert torch.equal(oa, ob), f"step {t}"
        if t == 40:                                                    # mid-cadence, consumed slots still marked
            np.testing.assert_array_equal(_cursors(b.env), _cursors(a.env))
    hf.refill()
    df.refill()
    np.testing.assert_array_equal(_table(b.env), _table(a.env))
    np.testing.assert_array_equal(_cursors(b.env), _cursors(a.env))
    np.testing.assert_array_equal(df.delivered(), hf.written)
    assert int(hf.written.min()) > L                                   # the rings went round
    a.env.check_device_error()
    b.env.check_device_error()
    a.close()
    b.close()


def test_first_stream_offsets_feed_the_right_rows():
    """Bin b is fed by stream first_stream + b: the groups of a grouped environment, and an environment under a generator
    with more streams than it has bins; a draw in between two refills continues the same streams."""
    sh = synthetic.blockout_shapes(n_shapes=20, n_rot=4, cube=0.06, seed=7)
    groups = itemgen.instance_groups(_instance_dic())
    seed = 1000
    host = lambda s, count: itemgen.ItemStream(seed + s, groups).draw(count)       # noqa: E731
    # grouped: three groups of two bins, group g fed by streams 2g, 2g + 1 on its own HIP stream
    df = itemgen.DeviceStreamFeeder(itemgen.DeviceItemStreams([seed + i for i in range(6)], groups, device=DEV), ring_len=L)
    envs = GpuVecEnv(sh, df.initial, 6, device=DEV, feeder=df, num_groups=3, obs_ring=0, **_env_kw(1))
    envs.env.synchronize()
    for g, e in enumerate(envs.env.groups):
        np.testing.assert_array_equal(_table(e), np.stack([host(2 * g + i, L) for i in range(2)]))
    envs.close()
    # ten streams, six bins, fed from stream 3 on
    ds = itemgen.DeviceItemStreams([seed + i for i in range(10)], groups, device=DEV)
    env = GpuPackingEnv(sh, np.full((6, L), -1, dtype=np.int32), 6, device=DEV, **_env_kw(1))
    refill = lambda first: env.lib.irbpp_stream_refill(env._h, ds._h, first, env._stream())       # noqa: E731
    assert refill(5) == -1 and refill(-1) == -1                        # IRBPP_ERR_ARG: 5 + 6 bins > 10 streams
    assert (_table(env) == -1).all()
    assert refill(3) == 0
    np.testing.assert_array_equal(_table(env), np.stack([host(3 + b, L) for b in range(6)]))
    np.testing.assert_array_equal(ds.delivered().cpu().numpy(), [0, 0, 0, L, L, L, L, L, L, 0])
    # a draw takes items L .. L+4 of every stream; then bins that have consumed 0, 3, 10, 64, 5, 7 items are refilled: the
    # streams have delivered L + 5, so bins at 10 and 7 get 5 and 2 items, the bin at 64 a whole lap minus 5, the others nothing
    got = ds.draw(5).cpu().numpy()
    np.testing.assert_array_equal(got, np.stack([host(s, L + 5)[L:] if 3 <= s < 9 else host(s, 5) for s in range(10)]))
    consumed = [0, 3, 10, 64, 5, 7]
    _cursors(env, consumed)
    assert refill(3) == 0
    want = np.stack([host(3 + b, L) for b in range(6)])
    for b, c in enumerate(consumed):
        count = max(0, c + L - (L + 5))
        items = host(3 + b, L + 5 + count)
        for j in range(count):
            want[b, (L + 5 + j) % L] = items[L + 5 + j]
    np.testing.assert_array_equal(_table(env), want)
    np.testing.assert_array_equal(ds.delivered().cpu().numpy(),
                                  [5, 5, 5] + [L + 5 + max(0, c - 5) for c in consumed] + [5])
    env.check_device_error()
    # an environment without item streams refuses a refill
    plain = GpuPackingEnv(sh, synthetic.make_sequences(sh.n_shapes, 8, 10), 6, device=DEV, **dict(_env_kw(1), item_stream=0))
    assert plain.lib.irbpp_stream_refill(plain._h, ds._h, 0, plain._stream()) == -3            # IRBPP_ERR_STATE
    plain.close()
    env.close()
    ds.close()


@pytest.mark.parametrize("k,sample,groups", [(1, "instance", 1), (3, "instance", 1), (1, "category", 1), (3, "category", 2),
                                             (1, "pose", 1), (3, "pose", 2), (1, "instance", 2)])
def test_make_vec_envs_trains_on_device_drawn_item_streams(k, sample, groups):
    """The protocol of test_make_vec_envs_trains_on_the_reference_item_streams with the generator on the device: every
    observation equals the oracle over the reference's creators restated on numpy's RandomState, through 170 steps, a
    mid-run reset() and a reset_specific, with rings of 64 items that go round more than once."""
    sh = synthetic.blockout_shapes(n_shapes=20, n_rot=4, cube=0.06, seed=7)
    if sample == "instance":
        dic = _instance_dic()
    elif sample == "category":
        dic = {i: "%s/%d.obj" % (["objects", "concave", "board"][(i * 5) % 3], i) for i in range(20)}
    else:
        dic = {i: "%d.obj" % i for i in range(20)}
    n, seed = 6, 321
    args = types.SimpleNamespace(
        num_processes=n, device=0, seed=seed, shapes=sh, dicPath=dic, dataSample=sample, resolutionA=0.02,
        resolutionH=0.01, resolutionZ=0.01, bin_dimension=np.round([0.32, 0.32, 0.30], 6), selectedAction=S,
        bufferSize=k, scale=[100, 100, 100], evaluate=False, item_ring=L, num_groups=groups, item_feed="device")
    envs, spaces, obs_len = make_vec_envs(args, "./logs/runinfo", True)
    assert isinstance(envs.feeder, itemgen.DeviceStreamFeeder) and envs.num_groups == groups
    envs.candidates_on_device = True
    creators = [RandomStreamItemCreator(seed + i, dic, sample, n_items=20) for i in range(n)]
    oenv = OracleVecEnv(n, sh, None, item_creators=creators, bufferSize=k)
    gobs, oobs = envs.reset(), _f32(oenv.reset())
    np.testing.assert_array_equal(gobs.cpu().numpy(), oobs)
    ndone = 0
    for t in range(170):
        if k > 1:
            order = (np.arange(n) + t) % k
            gloc = envs.get_action_candidates(order)
            oloc = _f32(oenv.get_action_candidates(order))
            np.testing.assert_array_equal(gloc.cpu().numpy(), oloc)
        else:
            oloc = oobs
        act = np.array([minz_action(o, S) for o in oloc])
        gobs, grew, gdone, ginfo = envs.step(act)
        oobs, orew, odone, oinfo = oenv.step(act)
        oobs = _f32(oobs)
        np.testing.assert_array_equal(gobs.cpu().numpy(), oobs, err_msg=f"step {t}")
        np.testing.assert_array_equal(gdone, odone)
        ndone += int(odone.sum())
        if t == 60:                                     # a mid-episode reset(): queues are dropped, the streams go on
            gobs, oobs = envs.reset(), _f32(oenv.reset())
            np.testing.assert_array_equal(gobs.cpu().numpy(), oobs)
        if t == 100:                                    # ... and a per-env reset
            sub = envs.reset_specific([4, 1])
            ref = _f32(oenv.reset_specific([4, 1]))
            np.testing.assert_array_equal(sub.cpu().numpy(), ref)
            for j, i in enumerate([4, 1]):
                gobs[i] = sub[j]
                oobs[i] = ref[j]
    delivered = envs.feeder.delivered()                 # the device-side count
    envs.env.check_device_error()
    envs.close()
    assert ndone >= 6 and int(delivered.min()) > 2 * L  # every ring went round more than once after its first fill


def test_a_ring_that_runs_dry_raises_stream_dry():
    """STREAM_DRY is an error word, not a fault: a bin stepped past its ring without a refill reports it at the fetch, and a
    refill that finds a cursor beyond what the stream has delivered raises it too (and writes nothing)."""
    sh = synthetic.blockout_shapes(n_shapes=20, n_rot=4, cube=0.06, seed=7)
    groups = itemgen.instance_groups(_instance_dic())
    ds = itemgen.DeviceItemStreams([7 + i for i in range(6)], groups, device=DEV)
    env = GpuPackingEnv(sh, np.full((6, L), -1, dtype=np.int32), 6, device=DEV, **_env_kw(1))
    _lib.check(env.lib.irbpp_stream_refill(env._h, ds._h, 0, env._stream()), "irbpp_stream_refill")
    obs = env.reset()
    for t in range(L + 4):                              # one item per bin and step, and nobody refills
        obs = env.step(env.policy_minz(obs))[0]
    with pytest.raises(_lib.IrbppError, match="STREAM_DRY"):
        env.check_device_error()
    env.close()
    env = GpuPackingEnv(sh, np.full((6, L), -1, dtype=np.int32), 6, device=DEV, **_env_kw(1))
    ds2 = itemgen.DeviceItemStreams([7 + i for i in range(6)], groups, device=DEV)
    _lib.check(env.lib.irbpp_stream_refill(env._h, ds2._h, 0, env._stream()), "irbpp_stream_refill")
    env.check_device_error()
    before = _table(env)
    _cursors(env, [0, 0, L + 1, 0, 0, 0])               # bin 2 claims an item the stream never delivered
    _lib.check(env.lib.irbpp_stream_refill(env._h, ds2._h, 0, env._stream()), "irbpp_stream_refill")
    with pytest.raises(_lib.IrbppError, match="STREAM_DRY"):
        env.check_device_error()
    np.testing.assert_array_equal(_table(env), before)
    np.testing.assert_array_equal(ds2.delivered().cpu().numpy(), np.full(6, L))
    env.close()
    ds.close()
    ds2.close()


def test_the_host_feeder_stays_the_default():
    sh = synthetic.blockout_shapes(n_shapes=20, n_rot=4, cube=0.06, seed=7)
    args = types.SimpleNamespace(
        num_processes=4, device=0, seed=5, shapes=sh, dicPath=_instance_dic(), dataSample="instance", resolutionA=0.02,
        resolutionH=0.01, resolutionZ=0.01, bin_dimension=np.round([0.32, 0.32, 0.30], 6), selectedAction=S,
        bufferSize=1, scale=[100, 100, 100], evaluate=False, item_ring=L)
    for feed in (None, "host"):
        if feed is not None:
            args.item_feed = feed
        envs, _, _ = make_vec_envs(args, None, True)
        assert type(envs.feeder) is itemgen.StreamFeeder
        envs.close()
    args.item_feed = "gpu"
    with pytest.raises(ValueError):
        make_vec_envs(args, None, True)
