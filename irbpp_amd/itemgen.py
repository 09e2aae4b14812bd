"""The reference's random item creators as per-environment item streams (training-time item supply).

In training every environment process draws its items with ``np.random.choice`` on the process-global legacy
generator (RandomItemCreator / RandomInstanceCreator / RandomCateCreator, IRcreator.py:26-72), seeded with
``args.seed + rank`` (envs.py:41 -> PackingGame.seed, binPhy.py:118-123).  ``ItemStream`` reproduces that stream
bit for bit (host code of libirbpp_hip.so: csrc/irbpp_itemgen.h); ``StreamFeeder`` keeps the per-bin item rings of an
environment created with ``item_stream=1`` ahead of the bins, so that ``make_vec_envs(args)`` needs nothing but the
reference's own namespace to train on the same item sequence the reference's workers would have drawn.
``DeviceItemStreams`` / ``DeviceStreamFeeder`` are the same streams and the same rings with the generator on the device
(csrc/irbpp_itemgen.hip): a refill is one kernel on the group's stream, and the host neither reads nor waits.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib


def instance_groups(dic_path: Dict[int, str]) -> List[List[int]]:
    """RandomInstanceCreator.__init__ (IRcreator.py:35-46): ids grouped by ``name[0:-6]`` in dict order."""
    inverse: Dict[str, List[int]] = {}
    for k in dic_path.keys():
        inverse.setdefault(dic_path[k][0:-6], []).append(k)
    return [inverse[name] for name in inverse.keys()]


def category_groups(dic_path: Dict[int, str]) -> List[List[int]]:
    """RandomCateCreator.__init__ (IRcreator.py:53-68): ids per category in the fixed order objects, concave, board
    (the probabilities in ``self.categories`` are never passed to np.random.choice: the draw is uniform)."""
    cates: Dict[str, List[int]] = {"objects": [], "concave": [], "board": []}
    for k, item in zip(dic_path.keys(), dic_path.values()):
        cate, _ = item.split("/")
        cates[cate].append(k)
    return [cates[c] for c in ("objects", "concave", "board")]


class ItemStream(object):
    """One environment's item stream.  ``groups``: list of id lists for the two-stage creators, or ``None`` with
    ``item_set`` for RandomItemCreator."""

    def __init__(self, seed: int, groups: Optional[Sequence[Sequence[int]]] = None, item_set: Optional[Sequence[int]] = None):
        self.lib = _lib.load()
        if groups is not None:
            members = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.int32) for g in groups]))
            offs = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32))
            n_groups, offs_p = len(groups), offs.ctypes.data_as(_lib.c_i32_p)
        else:
            members = np.ascontiguousarray(np.asarray(item_set, dtype=np.int32))
            n_groups, offs_p = 0, None
        if not 0 <= int(seed) <= 2 ** 32 - 1:
            raise ValueError("Seed must be between 0 and 2**32 - 1")           # np.random.seed's own rule
        self._h = C.c_void_p()
        _lib.check(self.lib.irbpp_itemgen_create(int(seed), n_groups, offs_p, members.ctypes.data_as(_lib.c_i32_p),
                                                 len(members), C.byref(self._h)), "irbpp_itemgen_create")

    def draw(self, count: int) -> np.ndarray:
        out = np.empty((int(count),), dtype=np.int32)
        _lib.check(self.lib.irbpp_itemgen_draw(self._h, int(count), out.ctypes.data_as(_lib.c_i32_p)), "irbpp_itemgen_draw")
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.irbpp_itemgen_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def streams_for_args(args, num_envs: int, rank_offset: int = 0, device=False):
    """The creators PackingGame.__init__ picks for training (binPhy.py:58-67), one per environment, seeded
    ``args.seed + rank`` like envs.py:41.  ``args.dicPath`` may be the dict itself or the path of ``id2shape.pt``.
    ``device``: False -> a list of host ``ItemStream``; True (``args.device``) or a device -> one ``DeviceItemStreams``."""
    dic = args.dicPath
    if isinstance(dic, str):
        import torch
        dic = torch.load(dic, weights_only=False)
    sample = getattr(args, "dataSample", "instance")
    if sample == "category":
        groups, item_set = category_groups(dic), None
    elif sample == "instance":
        groups, item_set = instance_groups(dic), None
    else:
        assert sample == "pose"
        groups, item_set = None, list(range(len(dic)))                      # np.arange(0, len(shapeDict))
    if device is not False and device is not None:
        if device is True:
            device = args.device
        if not isinstance(device, str) and not hasattr(device, "type"):
            device = f"cuda:{int(device)}"
        return DeviceItemStreams([int(args.seed) + rank_offset + i for i in range(num_envs)], groups, item_set, device=device)
    return [ItemStream(int(args.seed) + rank_offset + i, groups, item_set) for i in range(num_envs)]


class StreamFeeder(object):
    """Host side of the item rings of a ``GpuPackingEnv(item_stream=1)``: row b of the environment's sequence table
    is a ring of ``ring_len`` items that only bin b reads; every ``ring_len // (4 * bufferSize)`` ticks the feeder
    reads the bins' cursors and rewrites what they have consumed.  A tick is anything that can cost a bin up to
    ``bufferSize`` items: a step (one item, or a whole new queue when the step ends the episode), a reset, a
    reset_specific -- ``GpuVecEnv`` ticks from all three.  Should a ring run dry all the same, the bin notices at the
    fetch itself: consumed ring slots are poisoned by the kernel, reading one raises IRBPP_DEVERR_STREAM_DRY in the
    step's error word (and ``refill`` raises when it sees a cursor beyond what it has delivered).
    Grouped environments (``GroupedPackingEnv``): group g's sub-environment owns rows [g*per, (g+1)*per) of the table
    and is fed on its own stream."""

    def __init__(self, streams: Sequence[ItemStream], ring_len: int = 4096, buffer_size: int = 1):
        self.streams = list(streams)
        self.ring_len = int(ring_len)
        self.K = int(buffer_size)
        if self.ring_len < 16 * self.K:
            raise ValueError("ring_len must be at least 16 * bufferSize")
        self.n = len(self.streams)
        self.written = np.full((self.n,), self.ring_len, dtype=np.int64)     # items drawn per stream so far
        self.initial = np.stack([s.draw(self.ring_len) for s in self.streams])
        self.every = max(1, self.ring_len // (4 * self.K))
        self.steps = 0
        self.env = None
        self.parts = []

    def attach(self, env) -> None:
        """``env``: the GpuPackingEnv (or GroupedPackingEnv) that was created with ``sequences=self.initial,
        item_stream=1``."""
        import torch
        assert env.num_bins == self.n
        self.env = env
        if hasattr(env, "groups"):                                           # (sub-environment, its rows, its stream)
            self.parts = [(e, env.rows(g), env.streams[g]) for g, e in enumerate(env.groups)]
        else:
            self.parts = [(env, slice(0, self.n), None)]
        self._cur = [torch.zeros((rows.stop - rows.start,), dtype=torch.int32, device=env.device) for _, rows, _ in self.parts]

    def tick(self, steps: int = 1) -> None:
        """Call once per environment step (or get_action_candidates + step pair), reset or reset_specific."""
        self.steps += steps
        if self.steps >= self.every:
            self.refill()

    def refill(self) -> None:
        import contextlib
        import torch
        L = self.ring_len
        self.steps = 0
        for (env, rows, st), cur_dev in zip(self.parts, self._cur):
            with (torch.cuda.stream(st) if st is not None else contextlib.nullcontext()):
                _lib.check(env.lib.irbpp_stream_cursors(env._h, C.c_void_p(cur_dev.data_ptr()), 0, env._stream()), "irbpp_stream_cursors")
                cur = cur_dev.cpu().numpy().astype(np.int64)                 # synchronises this part's stream
                written = self.written[rows]
                if (cur > written).any():
                    raise RuntimeError("an item ring ran dry: a bin consumed items the stream had not delivered (ring_len too small)")
                count = (cur + L - written).astype(np.int32)                 # what each bin has consumed since the last refill
                width = int(count.max())
                if width <= 0:
                    continue
                ids = np.zeros((len(count), width), dtype=np.int32)
                for i, s in enumerate(self.streams[rows]):
                    if count[i] > 0:
                        ids[i, :count[i]] = s.draw(int(count[i]))
                first = (written % L).astype(np.int32)
                dev = env.device
                t_ids, t_first, t_count = (torch.from_numpy(a).to(dev) for a in (ids, first, count))
                _lib.check(env.lib.irbpp_stream_write(env._h, C.c_void_p(t_ids.data_ptr()), C.c_void_p(t_first.data_ptr()),
                                                      C.c_void_p(t_count.data_ptr()), width, env._stream()), "irbpp_stream_write")
                torch.cuda.current_stream(dev).synchronize()                 # the staging tensors may go now
                self.written[rows] += count


class DeviceItemStreams(object):
    """``len(seeds)`` item streams over one set of lists, generated on the device: stream i equals
    ``ItemStream(seeds[i], groups, item_set)`` item for item.  The state (624 key words, position, items delivered per
    stream) lives in device memory; seeding runs there too, so construction uploads the seeds and the lists only."""

    def __init__(self, seeds: Sequence[int], groups: Optional[Sequence[Sequence[int]]] = None,
                 item_set: Optional[Sequence[int]] = None, device="cuda:0"):
        import torch
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("DeviceItemStreams needs a HIP device; the host generator is ItemStream")
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        if groups is not None:
            members = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.int32) for g in groups]))
            offs = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32))
            n_groups, offs_p = len(groups), offs.ctypes.data_as(_lib.c_i32_p)
        else:
            members = np.ascontiguousarray(np.asarray(item_set, dtype=np.int32))
            n_groups, offs_p = 0, None
        if any(not 0 <= int(s) <= 2 ** 32 - 1 for s in seeds):
            raise ValueError("Seed must be between 0 and 2**32 - 1")           # np.random.seed's own rule
        seeds_np = np.ascontiguousarray(np.asarray([int(s) for s in seeds], dtype=np.uint32))
        self.n = len(seeds_np)
        self._h = C.c_void_p()
        _lib.check(self.lib.irbpp_itemgen_dev_create(index, self.n, seeds_np.ctypes.data_as(C.POINTER(C.c_uint32)), n_groups, offs_p,
                                                     members.ctypes.data_as(_lib.c_i32_p), len(members), self._stream(),
                                                     C.byref(self._h)), "irbpp_itemgen_dev_create")

    def __len__(self) -> int:
        return self.n

    def _stream(self, stream=None):
        import torch
        return C.c_void_p((stream if stream is not None else torch.cuda.current_stream(self.device)).cuda_stream)

    def draw(self, count: int):
        """The next ``count`` items of every stream: int32[n, count] on the device, in flight on the current stream."""
        import torch
        out = torch.empty((self.n, int(count)), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.irbpp_itemgen_dev_draw(self._h, int(count), C.c_void_p(out.data_ptr()), self._stream()),
                   "irbpp_itemgen_dev_draw")
        return out

    def delivered(self):
        """Items every stream has written so far (draws and refills): int64[n] on the device, current stream."""
        import torch
        out = torch.empty((self.n,), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.irbpp_itemgen_dev_delivered(self._h, C.c_void_p(out.data_ptr()), self._stream()),
                   "irbpp_itemgen_dev_delivered")
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.irbpp_itemgen_dev_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceStreamFeeder(object):
    """``StreamFeeder`` with the generator on the device: same rings, same cadence (a refill every
    ``ring_len // (4 * bufferSize)`` ticks), same parts (group g's sub-environment is fed by streams
    [g*per, (g+1)*per) on the group's own HIP stream) -- but a refill is ``irbpp_stream_refill``, one kernel that reads
    the bins' cursors, draws what they have consumed and writes it into the rings, ordered with the steps on that stream.
    Nothing is read back and nothing waits: a ring that ran dry shows as IRBPP_DEVERR_STREAM_DRY in the error word, at
    the bin's fetch or at the refill that finds the cursor beyond what was delivered.  The environment is created over
    ``initial``, a placeholder table of -1; ``attach`` fills the rings."""

    def __init__(self, streams: DeviceItemStreams, ring_len: int = 4096, buffer_size: int = 1):
        self.streams = streams
        self.ring_len = int(ring_len)
        self.K = int(buffer_size)
        if self.ring_len < 16 * self.K:
            raise ValueError("ring_len must be at least 16 * bufferSize")
        self.n = len(streams)
        self.initial = np.full((self.n, self.ring_len), -1, dtype=np.int32)
        self.every = max(1, self.ring_len // (4 * self.K))
        self.steps = 0
        self.env = None
        self.parts = []

    def attach(self, env) -> None:
        """``env``: the GpuPackingEnv (or GroupedPackingEnv) that was created with ``sequences=self.initial,
        item_stream=1``.  The first refill happens here: nothing delivered, nothing consumed, so every ring is filled."""
        import torch
        assert env.num_bins == self.n
        self.env = env
        if hasattr(env, "groups"):                                           # (sub-environment, its first stream, its HIP stream)
            self.parts = [(e, g * env.per, env.streams[g]) for g, e in enumerate(env.groups)]
            cur = torch.cuda.current_stream(self.streams.device)
            for st in env.streams:
                st.wait_stream(cur)                                          # the streams were seeded on the current stream
        else:
            self.parts = [(env, 0, None)]
        self.refill()

    def tick(self, steps: int = 1) -> None:
        """Call once per environment step (or get_action_candidates + step pair), reset or reset_specific."""
        self.steps += steps
        if self.steps >= self.every:
            self.refill()

    def refill(self) -> None:
        self.steps = 0
        for env, first, st in self.parts:
            _lib.check(env.lib.irbpp_stream_refill(env._h, self.streams._h, first, env._stream(st)), "irbpp_stream_refill")

    def delivered(self) -> np.ndarray:
        """Items delivered per stream so far, on the host (tests and tooling: this one synchronises)."""
        if self.env is not None and hasattr(self.env, "synchronize"):
            self.env.synchronize()
        return self.streams.delivered().cpu().numpy()
