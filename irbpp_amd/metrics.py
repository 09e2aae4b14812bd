"""The trainer's logged episode metrics, kept on the device (trainer.py:145-147, 168-178, 215-222).

The reference appends round(r, 6), ratio and counter of every finished, valid episode (env index order) to three
``deque(maxlen=10)`` and logs their mean / max / min every step.  ``EpisodeMetrics`` attaches a window of the same kind to
the environment (irbpp_set_episode_window): one small kernel behind every step updates it and stores a snapshot per step,
and ``read()`` turns the snapshots of the steps since the last read into the rows the trainer would have logged, bit for bit,
with one merge launch and one device-to-host copy::

    metrics = EpisodeMetrics(envs)                  # window=10: the trainer's deques
    for T in range(1, T_max + 1):
        state, reward, done = actor_step(envs, policy, memory, state)
        if T % 100 == 0:
            for tag, value, step in metrics.scalars(metrics.read()):
                writer.add_scalar(tag, value, step)
"""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np
import torch

from . import _lib

ROW_COLUMNS = ("T", "n", "reward_mean", "reward_max", "reward_min", "ratio_mean", "counter_mean")
ENTRY_WORDS = 4          # irbpp_episode_entry: 32 bytes = 4 int64 words


def window_words(window: int, history: int) -> int:
    """int64 words of one window's buffer: state (16 B) | rows [H][2] int32 | ring [W] | snapshots [H][W] entries."""
    return 2 + history + ENTRY_WORDS * window + ENTRY_WORDS * history * window


def window_struct(buf: torch.Tensor, window: int, history: int) -> _lib.IrbppEpisodeWindow:
    """The irbpp_episode_window that describes one window's buffer (a flat int64 device tensor of window_words words)."""
    assert buf.dtype == torch.int64 and buf.dim() == 1 and buf.numel() == window_words(window, history) and buf.is_contiguous()
    base, w = buf.data_ptr(), 8
    rows = base + 2 * w
    ring = rows + history * w
    snap = ring + ENTRY_WORDS * window * w
    return _lib.IrbppEpisodeWindow(ring_dev=ring, snapshot_dev=snap, rows_dev=rows, state_dev=base, window=window,
                                   history=history)


def scalars(rows: np.ndarray):
    """(tag, value, T) triples: one writer.add_scalar(tag, value, T) each reproduces trainer.py:215-222 for those steps (nothing
    where the deques were empty)."""
    for row in np.asarray(rows).reshape(-1, 7):
        if row[1] <= 0:
            continue
        T = int(row[0])
        yield "Metric/Reward mean", float(row[2]), T
        yield "Metric/Reward max", float(row[3]), T
        yield "Metric/Reward min", float(row[4]), T
        yield "Metric/Ratio", float(row[5]), T
        yield "Metric/Length", float(row[6]), T


class EpisodeMetricsOverrun(_lib.IrbppError):
    """More than ``history`` steps passed between two reads: the oldest snapshots were overwritten."""


def _parts_of(envs) -> list:
    """(GpuPackingEnv, stream or None) per part, in global bin order: a GpuPackingEnv, a GroupedPackingEnv (one part per group,
    on the group's stream) or a list of those (e.g. shards of one process)."""
    from .vec_env import GpuPackingEnv, GroupedPackingEnv
    if isinstance(envs, (list, tuple)):
        return [p for e in envs for p in _parts_of(e)]
    if isinstance(envs, GroupedPackingEnv):
        return list(zip(envs.groups, envs.streams))
    if isinstance(envs, GpuPackingEnv):
        return [(envs, None)]
    raise TypeError("EpisodeMetrics needs a GpuPackingEnv, a GroupedPackingEnv or a list of them")


def rows_from_device(lib, structs: List[_lib.IrbppEpisodeWindow], first: int, count: int, device) -> torch.Tensor:
    """irbpp_episode_metrics on the current stream: float64[count][7] device tensor."""
    out = torch.empty((count, 7), dtype=torch.float64, device=device)
    arr = (_lib.IrbppEpisodeWindow * len(structs))(*structs)
    _lib.check(lib.irbpp_episode_metrics(arr, len(structs), int(first), int(count), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "irbpp_episode_metrics")
    return out


def take_rows(rows: np.ndarray, first: int, history: int):
    """The recorded rows of a metrics read (n >= 0), and the next step to read.  Raises EpisodeMetricsOverrun if the first ones
    were overwritten (the read then resumes after the last recorded step) and IrbppError if the parts disagree."""
    n = rows[:, 1]
    recorded = int(np.count_nonzero(n != -2))
    if np.any(n[recorded:] != -2):
        raise _lib.IrbppError("episode windows out of step: some part recorded steps another did not (join their streams)")
    lost = int(np.count_nonzero(n[:recorded] == -1))
    if lost:
        raise EpisodeMetricsOverrun(f"steps {first} .. {first + lost - 1} were overwritten before this read: read at least every "
                                    f"{history} steps (EpisodeMetrics(history=...))")
    return rows[:recorded], first + recorded


class EpisodeMetrics(object):
    """A device-side window of the last ``window`` finished episodes per environment part (one per group of a
    GroupedPackingEnv, updated on the group's own stream), snapshotted after every step for ``history`` steps.
    ``read()`` returns float64[steps, 7] rows (ROW_COLUMNS) for the steps since the last read."""

    def __init__(self, envs, window: int = 10, history: int = 1024):
        if not 1 <= int(window) <= 1024:
            raise ValueError("window must be 1 .. 1024")
        if int(history) < 1:
            raise ValueError("history must be >= 1")
        self.window, self.history = int(window), int(history)
        self._parts = _parts_of(envs)
        if not 1 <= len(self._parts) <= 64:
            raise ValueError("1 .. 64 environment parts")
        self.device = self._parts[0][0].device
        self.lib = _lib.load()
        words = window_words(self.window, self.history)
        self.buffers = torch.zeros((len(self._parts), words), dtype=torch.int64, device=self.device)
        self._structs = [window_struct(self.buffers[i], self.window, self.history) for i in range(len(self._parts))]
        torch.cuda.current_stream(self.device).synchronize()          # zeroed before any part's stream can step into it
        self._next = 1
        for (env, _), s in zip(self._parts, self._structs):
            _lib.check(self.lib.irbpp_set_episode_window(env._h, C.byref(s)), "irbpp_set_episode_window")
        self.attached = True

    def _join(self) -> None:
        cur = torch.cuda.current_stream(self.device)
        for _, st in self._parts:
            if st is not None and st != cur:
                cur.wait_stream(st)

    def _fork(self) -> None:
        cur = torch.cuda.current_stream(self.device)
        for _, st in self._parts:
            if st is not None and st != cur:
                st.wait_stream(cur)

    def steps_recorded(self) -> int:
        """Steps recorded since creation / reset (synchronises)."""
        self._join()
        return int(self.buffers[0, 0].item()) & 0xFFFFFFFF            # state[0]: the low half of word 0

    def reset(self) -> None:
        """Empty windows, steps counted from 1 again (the trainer's fresh deques of a new run)."""
        self._join()
        self.buffers[:, :2 + self.history].zero_()
        self._fork()
        self._next = 1

    def read(self, group=None) -> np.ndarray:
        """The rows of every step since the last read: float64[steps, 7].  ``group``: a torch.distributed process group (or
        True for the default one) -- every rank calls read together, one all_gather of the ranks' windows, merged in rank
        order (= global bin order under distributed.shard)."""
        self._join()
        if group is None:
            structs = self._structs
        else:
            from . import distributed
            gathered = distributed.gather_windows(self.buffers, None if group is True else group)
            self._gathered = gathered                  # kept alive until the merge has read it
            structs = [window_struct(gathered[i], self.window, self.history) for i in range(gathered.shape[0])]
        out = rows_from_device(self.lib, structs, self._next, self.history, self.device)
        rows = out.cpu().numpy()                      # the one device-to-host copy
        self._gathered = None
        first = self._next
        try:
            kept, self._next = take_rows(rows, first, self.history)
        except EpisodeMetricsOverrun:
            self._next = first + int(np.count_nonzero(rows[:, 1] != -2))
            raise
        return kept

    scalars = staticmethod(scalars)

    def close(self) -> None:
        """Detach: later steps launch exactly what they launched before the window was attached."""
        if getattr(self, "attached", False):
            for env, _ in self._parts:
                if getattr(env, "_h", None) is not None and env._h.value:
                    _lib.check(self.lib.irbpp_set_episode_window(env._h, None), "irbpp_set_episode_window")
            self.attached = False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

