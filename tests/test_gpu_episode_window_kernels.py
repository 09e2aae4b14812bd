"""The two episode-window kernels (irbpp_amd/csrc/irbpp_metrics.hip) on synthetic step outputs, without an environment:
irbpp_episode_window_update -- the launch a windowed step ends with -- fed the scenarios of tests/episode_window_model.py
(more than one bin per thread, short last segments, bursts beyond the window, wraps, odd flag bytes, halfway rewards), and
irbpp_episode_metrics merging up to 64 such windows.  After every step the raw buffers -- snapshot row, (T, fill), the ring
read from its head -- and the logged rows are held against the plain deque model, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, metrics
import episode_window_model as M
from episode_window_model import BIN_COUNTS, EXTRA_PAIRS, WINDOWS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN5 = [np.nan] * 5


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


class DeviceWindow(object):
    """One window's buffer (metrics.window_words / window_struct on a zeroed int64 tensor) and the entry point that steps it."""

    def __init__(self, lib, W, H, offset=0):
        self.lib, self.W, self.H, self.offset = lib, W, H, offset
        self.buf = torch.zeros(metrics.window_words(W, H), dtype=torch.int64, device=DEV)
        self.struct = metrics.window_struct(self.buf, W, H)

    def update(self, done, ep_reward, ratio, counter):
        """One step from device tensors uint8[n], float64[n], float64[n], int32[n]."""
        _lib.check(self.lib.irbpp_episode_window_update(C.byref(self.struct), _ptr(done), _ptr(ep_reward), _ptr(ratio),
                                                        _ptr(counter), done.numel(), self.offset, _stream()),
                   "irbpp_episode_window_update")

    def raw(self):
        """state int32[4], rows int32[H][2], ring int64[W][4], snapshots int64[H][W][4] (an entry: key, r, ratio, counter)."""
        W, H = self.W, self.H
        words = self.buf.cpu().numpy()
        ring_at = 2 + H
        snap_at = ring_at + 4 * W
        return (words[:2].view(np.int32), words[2:ring_at].view(np.int32).reshape(H, 2),
                words[ring_at:snap_at].reshape(W, 4), words[snap_at:].reshape(H, W, 4))


def _upload(steps):
    """Step outputs stacked on the device: [steps][n] each, row t the inputs of step t + 1."""
    return tuple(torch.from_numpy(np.stack(col)).to(DEV) for col in zip(*steps))


def _assert_entries(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} entries differ, first at {bad[0]}: {got[bad[0]].tolist()} vs {want[bad[0]].tolist()}"


def _check(win, model, first, last, what):
    """The window's buffers after step `last` against the model, for the steps first .. last (at most H of them)."""
    W, H = win.W, win.H
    assert 1 <= last - first + 1 <= H
    state, rows, ring, snap = win.raw()
    for t in range(first, last + 1):
        want = M.entries_array(model.entries[t - 1])
        assert rows[t % H].tolist() == [t, len(want)], (what, t, rows[t % H].tolist(), len(want))
        _assert_entries(snap[t % H, :len(want)], want, f"{what}: snapshot of step {t}")
    want = M.entries_array(model.entries[last - 1])
    fill, head = int(state[1]), int(state[2])
    assert int(state[0]) == last and fill == len(want) and 0 <= head < W, (what, state.tolist(), len(want))
    _assert_entries(ring[(head + np.arange(fill)) % W], want, f"{what}: ring from its head after step {last}")
    got = metrics.rows_from_device(win.lib, [win.struct], first, last - first + 1, DEV).cpu().numpy()
    M.assert_rows_equal(got, model.rows_array(first, last - first + 1))


def _run(lib, sc, H, offset, read_every):
    """Plays a scenario on a fresh window and checks it at least every H steps (and after the last one)."""
    win, model = DeviceWindow(lib, sc.W, H, offset), M.WindowModel(sc.W)
    dev = _upload(sc.steps)
    seen = 0
    for T in range(1, len(sc.steps) + 1):
        win.update(*(col[T - 1] for col in dev))
        model.step([(offset,) + tuple(sc.steps[T - 1])])
        if T - seen == read_every or T == len(sc.steps):
            _check(win, model, seen + 1, T, f"{sc.name} H={H}")
            seen = T
    torch.cuda.synchronize()
    return win, model


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# every (n, W) with H = 8 and a global offset; the sizes at which the segment loop changes shape again with H = 1
_CASES = [(n, W, 8) for n in BIN_COUNTS for W in WINDOWS] + [(n, W, 8) for n, W in EXTRA_PAIRS] + \
         [(n, W, 1) for n in (1, 1025, 2500, 8192) for W in WINDOWS] + [(n, W, 1) for n, W in EXTRA_PAIRS]


@pytest.mark.parametrize("n,W,H", _CASES)
def test_update_kernel_against_the_deque_model(lib, n, W, H):
    """Every script that exists at (n, W) -- nothing, bin 0, bin n-1, exactly W, W + 1, all, all but one, random at 0.01 and
    0.5, the wrap of a part-filled ring, flag bytes 2 and 255 -- over an empty, a part-filled and an overflowed window."""
    offset = 0 if H == 1 else 100_000 + n
    played = set()
    for i, sc in enumerate(M.scenarios(n, W)):
        _run(lib, sc, H, offset, read_every=1 if i % 2 else H)
        played.add(sc.name.split("/")[0])
    assert {"none", "first", "last", "all", "random_0.01", "random_0.5", "flag_bytes"} <= played
    if n > W:
        assert {"exactly_W", "W_plus_1"} <= played


def test_the_keys_carry_the_global_offset(lib):
    sc = M.scenario("all", 2500, 37)
    win, model = _run(lib, sc, 8, (1 << 20) - 2500, 8)
    keys = win.raw()[3][len(sc.steps) % 8, :37, 0]
    assert ((keys & 0xFFFFFFFF) == (1 << 20) - 37 + np.arange(37)).all() and ((keys >> 32) == len(sc.steps)).all()


def test_every_reward_is_rounded_as_python_rounds(lib):
    """n = W = 1024, every bin done in each of 700 consecutive steps: the whole halfway pool and 116 792 uniform rewards in
    [0, 20) pass through py_round6 as the device compiles it, and every one of them is in a snapshot that is compared."""
    sc = M.rounds_scenario()
    assert len(sc.steps) >= 40
    _run(lib, sc, 8, 0, 8)


def test_update_entry_point_status_codes(lib):
    n, W, H = 4, 3, 2
    win = DeviceWindow(lib, W, H)
    done = torch.ones(n, dtype=torch.uint8, device=DEV)
    r = torch.ones(n, dtype=torch.float64, device=DEV)
    q = torch.ones(n, dtype=torch.float64, device=DEV)
    c = torch.ones(n, dtype=torch.int32, device=DEV)
    call = lib.irbpp_episode_window_update
    good = [C.byref(win.struct), _ptr(done), _ptr(r), _ptr(q), _ptr(c), n, 0, _stream()]
    assert call(*good) == 0
    for i in range(5):                                                            # a NULL pointer
        args = list(good)
        args[i] = None
        assert call(*args) == -1, i
    for bad_n in (0, -1):
        assert call(*(good[:5] + [bad_n, 0, _stream()])) == -1
    s = win.struct
    fields = dict(ring_dev=s.ring_dev, snapshot_dev=s.snapshot_dev, rows_dev=s.rows_dev, state_dev=s.state_dev, window=W,
                  history=H)
    for change in (dict(window=0), dict(window=1025), dict(window=-1), dict(history=0), dict(ring_dev=None),
                   dict(snapshot_dev=None), dict(rows_dev=None), dict(state_dev=None)):
        bad = _lib.IrbppEpisodeWindow(**dict(fields, **change))                   # what irbpp_set_episode_window refuses
        assert call(*([C.byref(bad)] + good[1:])) == -1, change
    torch.cuda.synchronize()
    state, rows, _, snap = win.raw()
    assert state.tolist()[:2] == [1, 3] and rows[1].tolist() == [1, 3]            # the refused calls launched nothing
    assert (snap[1, :, 0] == (1 << 32) + np.arange(1, 4)).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the merge
# ---------------------------------------------------------------------------------------------------------------------------
class Parts(object):
    """P windows of 40 bins each (part p: global bins [40 p, 40 p + 40)) stepped through the update entry point."""

    def __init__(self, lib, P, W, H, steps):
        self.lib, self.P, self.H = lib, P, H
        self.wins = [DeviceWindow(lib, W, H, p * M.PART_BINS) for p in range(P)]
        self.structs = [w.struct for w in self.wins]
        self.dev = _upload_parts(steps)

    def step(self, t, only=None):
        """Step t (1-based) of every part, or of the parts in `only`."""
        for p in (range(self.P) if only is None else only):
            self.wins[p].update(*(col[t - 1, p] for col in self.dev))

    def rows(self, first, count):
        return metrics.rows_from_device(self.lib, self.structs, first, count, DEV).cpu().numpy()


def _upload_parts(steps):
    """steps[t][p] = Step -> device tensors [steps][P][40]"""
    cols = [np.stack([np.stack([part[k] for part in parts]) for parts in steps]) for k in range(4)]
    return tuple(torch.from_numpy(np.ascontiguousarray(col)).to(DEV) for col in cols)


def _global_model(steps, W, upto):
    model = M.WindowModel(W)
    for t in range(1, upto + 1):
        model.step([(p * M.PART_BINS,) + tuple(st) for p, st in enumerate(steps[t - 1])])
    return model


@pytest.mark.parametrize("W", M.MERGE_WINDOWS)
@pytest.mark.parametrize("P", M.MERGE_PARTS)
def test_merge_of_parts_against_the_global_deque(lib, P, W):
    """64 steps: every window empty (NaN rows), the total fill below, at and above W, parts that never finish a bin beside
    full ones, and at the end the newest W entries all in part P-1 (tests/test_episode_window_model_cpu.py pins each)."""
    H = 8
    ms = M.merge_scenario(P, W)
    parts = Parts(lib, P, W, H, ms.steps)
    model = _global_model(ms.steps, W, M.MERGE_STEPS)
    got = []
    for t in range(1, M.MERGE_STEPS + 1):
        parts.step(t)
        if t % H == 0:
            got.append(parts.rows(t - H + 1, H))
    got = np.concatenate(got)
    want = model.rows_array()
    assert np.isnan(want[0, 2]) and want[0, 1] == 0 and want[ms.equal_step - 1, 1] == W and want[-1, 1] == W
    M.assert_rows_equal(got, want)


@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("P", M.MERGE_PARTS)
def test_a_part_one_step_behind_answers_minus_two(lib, P, which):
    """Every part has recorded 11 steps, all but one 13: n_steps = H = 8 from step 6 crosses the T % H wrap at 8; steps 12 and
    13 are n = -2 with NaN statistics, the steps before them the global rows."""
    W, H = 10, 8
    lag = 0 if which == "first" else P - 1
    steps = M.random_part_steps(P, 13)
    parts = Parts(lib, P, W, H, steps)
    for t in range(1, 12):
        parts.step(t)
    for t in (12, 13):
        parts.step(t, only=[p for p in range(P) if p != lag])
    model = _global_model(steps, W, 11)
    want = np.concatenate([model.rows_array(6, 6), np.array([[12, -2] + NAN5, [13, -2] + NAN5])])
    M.assert_rows_equal(parts.rows(6, H), want)


@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("P", M.MERGE_PARTS)
def test_an_overwritten_snapshot_row_answers_minus_one(lib, P, which):
    """One part has recorded 13 steps, the others 11: its snapshot rows of steps 4 and 5 now hold steps 12 and 13.  n_steps =
    H = 8 from step 4: n = -1 with NaN statistics for those two, the global rows for steps 6 .. 11."""
    W, H = 10, 8
    ahead = 0 if which == "first" else P - 1
    steps = M.random_part_steps(P, 13, seed=1)
    parts = Parts(lib, P, W, H, steps)
    for t in range(1, 12):
        parts.step(t)
    for t in (12, 13):
        parts.step(t, only=[ahead])
    model = _global_model(steps, W, 11)
    want = np.concatenate([np.array([[4, -1] + NAN5, [5, -1] + NAN5]), model.rows_array(6, 6)])
    M.assert_rows_equal(parts.rows(4, H), want)
