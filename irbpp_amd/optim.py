"""The optimiser step of Agent.learn as one call: what the reference writes as

    online_net.zero_grad()
    ...
    clip_grad_norm_(online_net.parameters(), norm_clip)        # agent.py:120
    optimiser.step()                                           # agent.py:121, optim.Adam (agent.py:44)
    target_net.load_state_dict(online_net.state_dict())        # agent.py:127-128, every target_update steps

is ``ClippedAdam.step`` here: two kernel launches over all parameter tensors at once (csrc/irbpp_optim.hip through
irbpp_clipped_adam_step) in a defined arithmetic, reproducible bit for bit: the gradient norm from float64 partial sums added
in one fixed order, torch's Adam update with two fmaf.  ``clipped_adam_np`` below is that definition in numpy; it is what
``step`` runs on CPU tensors and with ``use_hip=False``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Iterable, List, Optional

import numpy as np
import torch

from .replay import _fmaf_np, _hip_lib, _stream

# Which form ClippedAdam.step takes on a HIP device when the caller does not say (use_hip=None).  The kernels, since
# tools/optimiser_step_rates.py measured the two launches on an MI355X at 0.032 ms against 0.223 ms for torch's best form
# (clip_grad_norm_ + Adam(fused=True)) over DQNBPP's 34 tensors and 0.039 ms against 0.261 ms over the order network's 47, with
# spreads of at most 0.031 ms ("The optimiser step"; profiles/optimiser_step/).
FUSED_STEP_HIP_DEFAULT = True

CHUNK = 1024                                             # elements per chunk = per workgroup (OPTIM_CHUNK)
WRITE_GRADS, ZERO_GRADS, SYNC_TARGET, CLIP_ONLY = 1, 2, 4, 8

_f32, _f64 = np.float32, np.float64
_LANE = np.arange(64)


def _block_sum_np(s):
    """[..., 256] float64 -> [...]: the butterfly s = s + s[lane ^ o], o = 1 .. 32, within each wave of 64, then
    ((w0 + w1) + w2) + w3 over the four waves."""
    s = s.reshape(s.shape[:-1] + (4, 64))
    for o in (1, 2, 4, 8, 16, 32):
        s = s + s[..., _LANE ^ o]
    w = s[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def grad_sumsq_np(grads: List[np.ndarray]) -> np.float64:
    """The float64 sum of squares of the definition: per chunk of 1024 (thread t: elements 4t .. 4t+3 in ascending order,
    +0.0 past the end), then the partial sums in the same shape (thread t: partial t, t + 256, ..)."""
    with np.errstate(all="ignore"):
        partial = []
        for g in grads:
            n = g.size
            q = np.zeros((n + CHUNK - 1) // CHUNK * CHUNK, dtype=_f64)
            q[:n] = g.reshape(-1).astype(_f64)
            q = (q * q).reshape(-1, 256, 4)
            partial.append(_block_sum_np(((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]))
        partial = np.concatenate(partial) if partial else np.zeros(0, dtype=_f64)
        rows = np.zeros((partial.size + 255) // 256 * 256, dtype=_f64)
        rows[:partial.size] = partial
        s = np.zeros(256, dtype=_f64)
        for row in rows.reshape(-1, 256):
            s = s + row
        return _f64(_block_sum_np(s))


def norm_and_coef_np(grads: List[np.ndarray], max_norm: float):
    """-> (total float32, coef float32, nonfinite): the norm, the clip coefficient and the skip rule of the definition."""
    with np.errstate(all="ignore"):
        s = grad_sumsq_np(grads)
        bits = int(np.asarray(s).view(np.uint64))
        nonfinite = (bits >> 52) & 0x7ff == 0x7ff
        if nonfinite:
            total = np.array(0x7fc00000 if bits & ((1 << 52) - 1) else 0x7f800000, dtype=np.uint32).view(_f32)[()]
            return total, _f32(1.0), True
        total = _f32(np.sqrt(s))
        coef = _f32(max_norm) / (total + _f32(1e-6))
        return total, (coef if coef < _f32(1.0) else _f32(1.0)), False


def adam_hyper(lr: float, beta1: float, beta2: float, eps: float, max_norm: float, t: int):
    """The eight float32 values the update uses at the 1-based step t (float64 on the host, rounded once)."""
    return dict(step_size=_f32(lr / (1.0 - beta1 ** t)), rsq=_f32(math.sqrt(1.0 - beta2 ** t)), beta1=_f32(beta1),
                one_minus_beta1=_f32(1.0 - beta1), beta2=_f32(beta2), one_minus_beta2=_f32(1.0 - beta2), eps=_f32(eps),
                max_norm=_f32(max_norm))


def clipped_adam_np(params, grads, exp_avgs, exp_avg_sqs, hyper: dict, flags: int, targets=None):
    """The definition of csrc/irbpp_optim.hip on lists of float32 numpy arrays, updated in place -> (total, skipped: 0 or 1).
    ``hyper`` is adam_hyper's; ``targets`` (entries may be None) is written with SYNC_TARGET."""
    total, coef, nonfinite = norm_and_coef_np(grads, hyper["max_norm"])
    if nonfinite:
        return total, 1
    with np.errstate(all="ignore"):
        for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
            gc = g * coef
            if flags & CLIP_ONLY:
                g[...] = gc
                continue
            m[...] = _fmaf_np(hyper["one_minus_beta1"], gc - m, m)
            v[...] = _fmaf_np(gc * gc, hyper["one_minus_beta2"], v * hyper["beta2"])
            d = np.sqrt(v) / hyper["rsq"] + hyper["eps"]
            p[...] = _fmaf_np(-hyper["step_size"], m / d, p)
            if flags & ZERO_GRADS:
                g[...] = 0
            elif flags & WRITE_GRADS:
                g[...] = gc
            if flags & SYNC_TARGET and targets is not None and targets[i] is not None:
                targets[i][...] = p
    return total, 0


class ClippedAdam(object):
    """``clip_grad_norm_(params, max_norm)`` followed by ``optim.Adam(params, lr, betas, eps).step()`` as one call, with the
    next step's ``zero_grad`` and the target network's parameter copy folded in.

    ``params``: float32 contiguous tensors on one device.  A tensor whose ``grad`` is None, or with no element, takes no
    part in a step, as in torch.  ``grads="write"`` leaves the clipped gradients behind as ``clip_grad_norm_`` does;
    ``grads="zero"`` leaves zeros in the same storage: the next ``backward`` accumulates into them, which is the next
    step's ``zero_grad`` (do not call ``zero_grad(set_to_none=True)`` then: stable gradient pointers keep the device tables).
    ``target_params`` (one per parameter, same shapes) are written by ``step(sync_target=True)``: update_target_net for
    the parameters.  The noisy layers' ``*_epsilon`` buffers are not copied: ``learn`` redraws the target's noise
    (agent.py:94) before every use of it.

    ``step`` returns the total gradient norm as a 0-dim tensor on the parameters' device; nothing is read back and nothing
    waits.  A non-finite norm (an infinite or NaN gradient) skips the step: no tensor changes, ``skipped()`` goes up by one,
    and the step count still advances.  There is one step count for all tensors: a tensor whose gradient was absent for a
    while rejoins with the common bias correction (torch counts per tensor).

    ``use_hip=True`` asks for the kernels (a HIP device), ``None`` takes FUSED_STEP_HIP_DEFAULT; otherwise, and on CPU
    tensors, the same definition runs in numpy on the host (``clipped_adam_np``: the reference form, not a fast one)."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_norm: float = float("inf"), *, target_params: Optional[Iterable[torch.Tensor]] = None, grads: str = "write",
                 use_hip: Optional[bool] = None):
        self.params = list(params)
        if not self.params:
            raise ValueError("no parameters")
        if grads not in ("write", "zero"):
            raise ValueError('grads must be "write" or "zero"')
        self.lr, self.betas, self.eps, self.max_norm, self.grads = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(max_norm), grads
        self.device = self.params[0].device
        for p in self.params:
            self._check(p, "parameter")
        self.targets = None if target_params is None else list(target_params)
        if self.targets is not None:
            if len(self.targets) != len(self.params):
                raise ValueError("target_params must hold one tensor per parameter")
            for p, q in zip(self.params, self.targets):
                self._check(q, "target parameter")
                if q.shape != p.shape:
                    raise ValueError("a target parameter's shape differs from its parameter's")
        lib = _hip_lib(self.device)
        if use_hip and lib is None:
            raise RuntimeError("use_hip=True needs a HIP device")
        self._lib = lib if (FUSED_STEP_HIP_DEFAULT if use_hip is None else use_hip) else None
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in self.params]
        self._seen = [False] * len(self.params)           # took part in a step: has a state of its own in state_dict()
        self._t = 0
        self._skipped = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._key = None                                 # what the device tables were built from
        self._tables = None

    def _check(self, t: torch.Tensor, what: str) -> None:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device or t.numel() >= 2 ** 31:
            raise ValueError(f"every {what} must be float32, contiguous, on {self.device} and below 2^31 elements")

    # ---- the tables ----------------------------------------------------------------------------------------------------
    def _active(self) -> List[int]:
        act = []
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None or p.numel() == 0:
                continue
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.device or g.numel() != p.numel():
                raise ValueError("every gradient must be float32, contiguous and on its parameter's device")
            act.append(i)
        return act

    def _device_tables(self, act: List[int]):
        """(tensor table, chunk table, partial sums, number of chunks) on the device, rebuilt only when a data_ptr, a numel
        or the set of present gradients changed since the last call."""
        key = tuple((i, self.params[i].data_ptr(), self.params[i].grad.data_ptr(), self.params[i].numel(),
                     0 if self.targets is None else self.targets[i].data_ptr()) for i in act)
        if key == self._key:
            return self._tables
        from ._lib import IrbppOptimTensor
        table = (IrbppOptimTensor * len(act))()
        chunks = []
        for k, (i, p_ptr, g_ptr, n, t_ptr) in enumerate(key):
            table[k] = IrbppOptimTensor(p_ptr, g_ptr, self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr(), t_ptr or None, n)
            chunks += [(k, first) for first in range(0, n, CHUNK)]
        table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.device)
        chunks_dev = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(self.device)
        partial = torch.empty(len(chunks), dtype=torch.float64, device=self.device)
        self._key, self._tables = key, (table_dev, chunks_dev, partial, len(chunks))
        return self._tables

    # ---- the step ------------------------------------------------------------------------------------------------------
    def _run(self, flags: int, t: int) -> torch.Tensor:
        act = self._active()
        if not act:                                      # torch: a norm of 0 and no update
            return torch.zeros((), dtype=torch.float32, device=self.device)
        h = adam_hyper(self.lr, self.betas[0], self.betas[1], self.eps, self.max_norm, max(t, 1))
        if not flags & CLIP_ONLY:
            for i in act:
                self._seen[i] = True
        if self._lib is None:
            return self._run_np(act, h, flags)
        from . import _lib
        table_dev, chunks_dev, partial, n_chunks = self._device_tables(act)
        total = torch.empty((), dtype=torch.float32, device=self.device)
        hyper = _lib.IrbppAdamHyper(flags=flags, **{k: float(v) for k, v in h.items()})
        _lib.check(self._lib.irbpp_clipped_adam_step(table_dev.data_ptr(), len(act), chunks_dev.data_ptr(), n_chunks, partial.data_ptr(),
                                                     C.byref(hyper), total.data_ptr(), self._skipped.data_ptr(), _stream(self.device)),
                   "irbpp_clipped_adam_step")
        return total

    def _run_np(self, act: List[int], h: dict, flags: int) -> torch.Tensor:
        host = lambda t: t.detach().cpu().numpy().reshape(-1)         # noqa: E731  (shares memory with a CPU tensor)
        sets = [[host(ts[i]) for i in act] for ts in (self.params, [p.grad for p in self.params], self.exp_avg, self.exp_avg_sq)]
        targets = None if self.targets is None else [host(self.targets[i]) for i in act]
        total, skipped = clipped_adam_np(*sets, h, flags, targets)
        self._skipped += skipped
        if self.device.type != "cpu" and not skipped:
            with torch.no_grad():
                for k, i in enumerate(act):
                    for dst, src in zip((self.params[i], self.params[i].grad, self.exp_avg[i], self.exp_avg_sq[i]), (s[k] for s in sets)):
                        dst.copy_(torch.from_numpy(src).view_as(dst))
                    if flags & SYNC_TARGET and targets is not None:
                        self.targets[i].copy_(torch.from_numpy(targets[k]).view_as(self.targets[i]))
        return torch.from_numpy(np.asarray(total, dtype=_f32).copy()).to(self.device)

    def step(self, sync_target: bool = False) -> torch.Tensor:
        """Clip, update, write or zero the gradients, and with ``sync_target`` copy the new parameters to the targets
        -> the total norm, float32 0-dim on the device."""
        if sync_target and self.targets is None:
            raise ValueError("sync_target=True needs target_params")
        flags = (WRITE_GRADS if self.grads == "write" else ZERO_GRADS) | (SYNC_TARGET if sync_target else 0)
        self._t += 1
        return self._run(flags, self._t)

    def clip_only(self) -> torch.Tensor:
        """``clip_grad_norm_(params, max_norm)`` alone: the gradients scaled in place -> the total norm.  No moment, no
        parameter and no step count changes; a non-finite norm leaves the gradients as they are and counts as skipped."""
        return self._run(CLIP_ONLY, self._t)

    def skipped(self) -> int:
        """How many steps a non-finite norm skipped so far.  Reads the device counter: the one call here that synchronises."""
        return int(self._skipped.item())

    # ---- checkpoints, in torch.optim.Adam's layout ------------------------------------------------------------------------
    def state_dict(self) -> dict:
        group = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps).state_dict()["param_groups"][0]
        group["params"] = list(range(len(self.params)))
        state = {i: {"step": torch.tensor(float(self._t)), "exp_avg": self.exp_avg[i].clone(), "exp_avg_sq": self.exp_avg_sq[i].clone()}
                 for i in range(len(self.params)) if self._seen[i]}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: dict) -> None:
        groups = sd["param_groups"]
        if len(groups) != 1 or list(groups[0]["params"]) != list(range(len(self.params))):
            raise ValueError("the checkpoint must hold one parameter group over this optimiser's parameters")
        g = groups[0]
        if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("weight_decay, amsgrad and maximize have no form here")
        steps = {int(float(s["step"])) for s in sd["state"].values()}
        if len(steps) > 1:
            raise ValueError(f"the checkpoint's tensors are at different steps {sorted(steps)}: there is one step count here")
        for i, s in sd["state"].items():
            if tuple(s["exp_avg"].shape) != tuple(self.params[i].shape) or tuple(s["exp_avg_sq"].shape) != tuple(self.params[i].shape):
                raise ValueError(f"the moments of tensor {i} have another shape than the parameter")
        self.lr, self.betas, self.eps = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        self._t = steps.pop() if steps else 0
        with torch.no_grad():
            for i in range(len(self.params)):
                s = sd["state"].get(i)
                self._seen[i] = s is not None
                if s is None:
                    self.exp_avg[i].zero_()
                    self.exp_avg_sq[i].zero_()
                else:                                    # copied into the buffers the device tables point to
                    self.exp_avg[i].copy_(s["exp_avg"])
                    self.exp_avg_sq[i].copy_(s["exp_avg_sq"])
