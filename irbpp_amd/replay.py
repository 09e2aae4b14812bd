"""Caller-side scaling: the reference keeps one ``ReplayMemory`` object per
environment process (main.py:61-63) and feeds/samples them in Python loops (trainer.py:184-186,
agent.py:69-75), each with its own recursive sum tree on the CPU (memory.py:15-100).  With
thousands of bins per GPU that loop is the bottleneck, so here the N memories are ONE set of
device tensors and every operation handles all environments at once:

    reference (per env i)                         here (all envs)
    mem[i].append(state[i], action[i], r[i], d[i])   append(state, action, reward, done, valid)
    mem[i].sample(segment_size)  (agent.py:72-75)    sample(segment_size)  -> env-major batch
    mem[i].update_priorities(idxs[i], loss[...])     update_priorities(tree_idxs, losses)
    (none: its batch is never smaller than N rows)   sample_pooled(batch_size) -> one batch over all memories as one
                                                     update_priorities_pooled(idx, losses)   (csrc/irbpp_replay_pool.hip)

Semantics follow memory.py line by line (cited below): cyclic buffer + sum tree per env with
float32 node sums, new transitions enter with the env's maximum priority, stratified sampling
with the reference's validity test, n-step returns that blank everything after a terminal
transition, importance weights normalised per env.  On a HIP device the three sequential pieces -- the tree
descent of ``find``, the leaf-to-root update, and the masked greedy action of ``Agent.act`` -- are one kernel
launch each (csrc/irbpp_replay.hip through the C ABI); on the CPU (the CPU tests) the same results come from
the torch formulation kept below, which is also the fallback for capacities beyond the kernel's LDS row.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch


def _hip_lib(device: torch.device):
    """The HIP library if ``device`` is a HIP device (raises like every product path if it is missing)."""
    if device.type != "cuda":
        return None
    from . import _lib
    return _lib.load()


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


_WARNED_TORCH_PATH = False


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _pinned(*tensors) -> list:
    """[(tensor, its version counter now)]: what a hand-written backward will read, or what its caller handed over, beyond the
    reach of ``ctx.save_for_backward`` (a tensor held by a plain object, or the caller's own tensor where the forward went on
    with a converted copy).  A detached alias or a view shares its base's counter."""
    return [(t, t._version) for t in tensors if t is not None]


def _check_pinned(pinned: list, what: str) -> None:
    """autograd's own complaint for a _pinned tensor that was written in place since: the top of every such backward."""
    for t, version in pinned:
        if t._version != version:
            raise RuntimeError(f"{what}: one of the variables needed for gradient computation has been modified by an inplace "
                               f"operation: a {t.dtype} tensor of shape {list(t.shape)} is at version {t._version}; expected "
                               f"version {version} instead")


class VectorReplayMemory(object):
    def __init__(self, num_envs: int, capacity: int, obs_len: int, *, discount: float = 0.99, multi_step: int = 3,
                 priority_weight: float = 0.4, priority_exponent: float = 0.5, device="cpu",
                 state_dtype=torch.float32, use_hip: Optional[bool] = None):
        """``capacity`` is per environment (main.py:62: memory_capacity / num_processes)."""
        self.N, self.capacity, self.obs_len = int(num_envs), int(capacity), int(obs_len)
        self.device = torch.device(device)
        self.discount, self.n = float(discount), int(multi_step)
        self.priority_weight = float(priority_weight)        # beta, annealed by the trainer (trainer.py:196)
        self.priority_exponent = float(priority_exponent)    # omega
        d, N, cap = self.device, self.N, self.capacity
        # SegmentTree (memory.py:15-45): data arrays + sum tree, one row per env
        self.sum_tree = torch.zeros((N, 2 * cap - 1), dtype=torch.float32, device=d)
        self.timesteps = torch.zeros((N, cap), dtype=torch.int32, device=d)
        self.states = torch.zeros((N, cap, obs_len), dtype=state_dtype, device=d)
        self.actions = torch.zeros((N, cap), dtype=torch.int64, device=d)
        self.rewards = torch.zeros((N, cap), dtype=torch.float32, device=d)
        self.nonterminals = torch.zeros((N, cap), dtype=torch.bool, device=d)
        self.index = torch.zeros((N,), dtype=torch.int64, device=d)      # next write position
        self.full = torch.zeros((N,), dtype=torch.bool, device=d)
        self.max = torch.ones((N,), dtype=torch.float32, device=d)       # initial max priority 1 (memory.py:27)
        self.t = torch.zeros((N,), dtype=torch.int32, device=d)          # episode timestep counter (memory.py:111)
        self.n_step_scaling = torch.tensor([self.discount ** i for i in range(self.n)], dtype=torch.float32, device=d)
        self._rows = torch.arange(N, device=d)
        self._depth = max(1, (2 * cap - 1).bit_length())                 # >= height of the implicit tree
        # HIP kernels for find / update (one launch each) where the tree row fits their LDS buffer
        self._lib = _hip_lib(self.device) if use_hip in (None, True) else None
        self._append_hip = self._lib is not None              # (irbpp_replay_append walks one leaf's ancestors in global memory: any capacity)
        self._pool_lib = self._lib                            # (so do the pooled launches: sample_pooled / update_priorities_pooled)
        if use_hip and self._lib is None:
            raise RuntimeError("use_hip=True needs a HIP device")
        if self._lib is not None and 2 * cap - 1 > 16384:
            # said once per process, not silently: every sum-tree call of this memory is torch indexing from here on
            if use_hip:
                raise RuntimeError(f"use_hip=True: a sum tree of {2 * cap - 1} floats per env exceeds the HIP kernels' LDS row (16384)")
            global _WARNED_TORCH_PATH
            if not _WARNED_TORCH_PATH:
                import warnings
                warnings.warn(f"VectorReplayMemory: capacity {cap} per env (tree row of {2 * cap - 1} floats) exceeds the HIP sum-tree "
                              "kernels' LDS row of 16384 floats: using the torch formulation (several launches per call)", RuntimeWarning)
                _WARNED_TORCH_PATH = True
            self._lib = None

    # ------------------------------------------------------------------ sum tree ------------
    def _set_leaves(self, rows: torch.Tensor, tree_idx: torch.Tensor, value: torch.Tensor) -> None:
        """SegmentTree.update (memory.py:55-58) for one leaf per listed env: set, then recompute
        every ancestor as left + right in float32 (``_propagate``, :47-52)."""
        if self._lib is not None:
            from . import _lib
            N = self.N
            mask = None
            if rows.numel() != N:                                  # a subset of the envs: full-length arguments + mask
                mask = torch.zeros((N,), dtype=torch.uint8, device=self.device)
                mask[rows] = 1
                ti = torch.zeros((N,), dtype=torch.int64, device=self.device)
                ti[rows] = tree_idx
                va = torch.zeros((N,), dtype=torch.float32, device=self.device)
                va[rows] = value
                tree_idx, value = ti, va
            _lib.check(self._lib.irbpp_sumtree_update(_p(self.sum_tree), _p(self.max), N, self.capacity,
                                                      _p(tree_idx.contiguous()), _p(value.to(torch.float32).contiguous()), 1,
                                                      _p(mask), _stream(self.device)), "irbpp_sumtree_update")
            return
        self.sum_tree[rows, tree_idx] = value
        self.max[rows] = torch.maximum(self.max[rows], value)
        cap = self.capacity
        if cap & (cap - 1) == 0 and rows.numel() * 4 >= self.N:
            # power-of-two capacity: depth d of the implicit heap is the slice [2^d - 1, 2^(d+1) - 1), so every
            # level is one dense pairwise add over all envs -- the same left + right per node, far fewer launches
            width = cap // 2
            while width >= 1:
                lo = width - 1
                child = self.sum_tree[:, 2 * lo + 1: 4 * lo + 3].view(self.N, width, 2)
                self.sum_tree[:, lo: lo + width] = child[:, :, 0] + child[:, :, 1]
                width //= 2
            return
        idx = tree_idx
        for _ in range(self._depth):
            idx = torch.div(idx - 1, 2, rounding_mode="floor").clamp_(min=0)
            self.sum_tree[rows, idx] = self.sum_tree[rows, 2 * idx + 1] + self.sum_tree[rows, 2 * idx + 2]
        # (rows that reached the root early recompute it again: same two operands, same sum)

    def total(self) -> torch.Tensor:
        return self.sum_tree[:, 0]

    def find(self, values: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """SegmentTree.find / _retrieve (memory.py:72-86) for ``values[N, B]``:
        -> (priority, data index, tree index), each [N, B]."""
        N, B = values.shape
        if self._lib is not None:
            from . import _lib
            v = values.to(device=self.device, dtype=torch.float32).contiguous()
            prob = torch.empty((N, B), dtype=torch.float32, device=self.device)
            data_idx = torch.empty((N, B), dtype=torch.int64, device=self.device)
            tree_idx = torch.empty((N, B), dtype=torch.int64, device=self.device)
            _lib.check(self._lib.irbpp_sumtree_find(_p(self.sum_tree), N, self.capacity, _p(v), B, _p(prob), _p(data_idx),
                                                    _p(tree_idx), _stream(self.device)), "irbpp_sumtree_find")
            return prob, data_idx, tree_idx
        rows = self._rows[:, None].expand(N, B)
        idx = torch.zeros((N, B), dtype=torch.int64, device=self.device)
        v = values.to(torch.float32).clone()
        last = 2 * self.capacity - 2
        for _ in range(self._depth):
            left = 2 * idx + 1
            inner = left <= last                                   # `left >= len(sum_tree)` -> leaf
            lval = self.sum_tree[rows, left.clamp(max=last)]
            go_left = v <= lval
            nxt = torch.where(go_left, left, left + 1)
            v = torch.where(inner & ~go_left, v - lval, v)
            idx = torch.where(inner, nxt, idx)
        return self.sum_tree[rows, idx], idx - (self.capacity - 1), idx

    # ------------------------------------------------------------------ append --------------
    def _append_on_device(self, state, action, reward, terminal, valid) -> bool:
        """One launch of irbpp_replay_append for the whole call when the arguments are what an actor loop on the device
        hands over (float32 observation rows, int32 / int64 actions, float32 / float64 rewards, one-byte flags, all on
        this device) -- no conversion launches in front of it; False: the caller takes the torch formulation."""
        d = self.device
        if d.type != "cuda" or self.states.dtype != torch.float32:
            return False
        def on_dev(x, dtypes, n):        # noqa: E306
            return isinstance(x, torch.Tensor) and x.device == d and x.dtype in dtypes and x.numel() == n and x.is_contiguous()
        if not (isinstance(state, torch.Tensor) and state.device == d and state.dtype == torch.float32 and state.dim() == 2 and
                state.shape == (self.N, self.obs_len) and state.stride(1) == 1 and state.stride(0) >= self.obs_len):
            return False
        flags = (torch.bool, torch.uint8)
        if not (on_dev(action, (torch.int32, torch.int64), self.N) and on_dev(reward, (torch.float32, torch.float64), self.N) and
                on_dev(terminal, flags, self.N) and (valid is None or on_dev(valid, flags, self.N))):
            return False
        from . import _lib
        lib = self._lib if self._lib is not None else _lib.load()
        store = _lib.IrbppReplayStore(
            self.states.data_ptr(), self.actions.data_ptr(), self.rewards.data_ptr(), self.nonterminals.data_ptr(),
            self.timesteps.data_ptr(), self.sum_tree.data_ptr(), self.max.data_ptr(), self.index.data_ptr(), self.full.data_ptr(),
            self.t.data_ptr(), self.N, self.capacity, self.obs_len)
        _lib.check(lib.irbpp_replay_append(C.byref(store), _p(state), state.stride(0), _p(action), action.element_size(),
                                           _p(reward), reward.element_size(), _p(terminal), _p(valid), _stream(d)),
                   "irbpp_replay_append")
        return True

    def append(self, state: torch.Tensor, action: torch.Tensor, reward: torch.Tensor, terminal,
               valid: Optional[torch.Tensor] = None) -> None:
        """ReplayMemory.append (memory.py:117-121) for every env whose sample is valid
        (trainer.py:184-186): state/action at time t, reward/terminal at t+1; the new transition
        gets the env's maximum priority."""
        d = self.device
        if self._lib is not None or self._append_hip:
            if self._append_on_device(state, action, reward, terminal, valid):
                return
        terminal = torch.as_tensor(terminal, device=d).reshape(self.N).to(torch.bool)
        everyone = valid is None
        rows = self._rows if everyone else self._rows[torch.as_tensor(valid, device=d).reshape(self.N).to(torch.bool)]
        if rows.numel() == 0:
            return
        pick = (lambda x: x) if everyone else (lambda x: x[rows])
        pos = self.index[rows]
        self.timesteps[rows, pos] = self.t[rows]
        self.states[rows, pos] = pick(state.to(device=d, dtype=self.states.dtype))
        self.actions[rows, pos] = pick(action.to(d).reshape(self.N)).to(torch.int64)
        self.rewards[rows, pos] = pick(reward.to(d).reshape(self.N)).to(torch.float32)
        self.nonterminals[rows, pos] = ~pick(terminal)
        self._set_leaves(rows, pos + self.capacity - 1, self.max[rows])              # SegmentTree.append (:60-70)
        nxt = (pos + 1) % self.capacity
        self.index[rows] = nxt
        self.full[rows] = self.full[rows] | (nxt == 0)
        self.t[rows] = torch.where(terminal[rows], torch.zeros_like(self.t[rows]), self.t[rows] + 1)

    # ------------------------------------------------------------------ sample --------------
    def _valid(self, prob, data_idx):
        """memory.py:175: not straddling the write index, non-zero probability."""
        w = self.index[:, None]
        return ((w - data_idx) % self.capacity > self.n) & ((data_idx - w) % self.capacity >= 1) & (prob != 0)

    def _transitions(self, data_idx: torch.Tensor):
        """ReplayMemory._get_transition_new (memory.py:123-139) for data_idx[N, B]: the n+1
        consecutive transitions, blanked from the first one that follows a terminal transition."""
        N, B = data_idx.shape
        steps = torch.arange(self.n + 1, device=self.device)
        pos = (data_idx[:, :, None] + steps) % self.capacity                      # getBatch wraps (:89-91)
        rows = self._rows[:, None, None].expand(N, B, self.n + 1)
        nonterm = self.nonterminals[rows, pos]
        alive = torch.ones_like(nonterm)
        for t in range(1, self.n + 1):
            alive[:, :, t] = alive[:, :, t - 1] & nonterm[:, :, t - 1]
        state = self.states[self._rows[:, None].expand(N, B), pos[:, :, 0]]
        last = self.states[self._rows[:, None].expand(N, B), pos[:, :, self.n]]
        next_state = torch.where(alive[:, :, self.n, None], last, torch.zeros_like(last))
        rewards = torch.where(alive, self.rewards[rows, pos], torch.zeros((), device=self.device))
        action = self.actions[self._rows[:, None].expand(N, B), pos[:, :, 0]]
        returns = torch.matmul(rewards[:, :, :self.n], self.n_step_scaling)        # R^n (:186-188)
        nonterminal = (alive[:, :, self.n] & nonterm[:, :, self.n]).to(torch.float32)
        return state, action, returns, next_state, nonterminal

    def sample(self, segment_size: int, values: Optional[torch.Tensor] = None, generator=None, max_tries: int = 64):
        """ReplayMemory.sample (memory.py:194-204) on every env at once, concatenated env-major
        exactly as Agent.learn builds its batch (agent.py:69-84).

        ``values`` (optional, [N, segment_size]) are the tree positions to look up, as drawn by
        ``np.random.uniform(i*segment, (i+1)*segment)``; when omitted they are drawn here and
        invalid draws are redrawn like the reference's rejection loop (:170-176).
        Returns (tree_idxs [N,B], states, actions, returns, next_states, nonterminals [N*B,1], weights)."""
        N, B = self.N, int(segment_size)
        p_total = self.total()                                                    # [N]
        if values is not None or self._lib is None:
            segment = p_total / B
            lo = torch.arange(B, device=self.device, dtype=torch.float32)[None, :] * segment[:, None]
        if values is not None:
            prob, data_idx, tree_idx = self.find(values.to(self.device))
            if not bool(self._valid(prob, data_idx).all()):
                raise ValueError("a supplied sample position is invalid (memory.py:175)")
        elif self._lib is not None:
            # draw + tree walk + the rejection loop of memory.py:170-176 in ONE launch; the only host round trip is
            # the failure flag
            from . import _lib
            gdev = "cpu" if generator is None else generator.device          # a CPU generator costs no device round trip
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=gdev).item())
            prob = torch.empty((N, B), dtype=torch.float32, device=self.device)
            data_idx = torch.empty((N, B), dtype=torch.int64, device=self.device)
            tree_idx = torch.empty((N, B), dtype=torch.int64, device=self.device)
            failed = torch.zeros((1,), dtype=torch.int32, device=self.device)
            _lib.check(self._lib.irbpp_sumtree_sample(_p(self.sum_tree), _p(self.index), N, self.capacity, B, self.n, seed,
                                                      int(max_tries), _p(prob), _p(data_idx), _p(tree_idx), _p(failed),
                                                      _stream(self.device)), "irbpp_sumtree_sample")
            if int(failed.item()):
                raise RuntimeError("could not draw a valid sample from every segment; append more transitions first")
        else:
            draw = lambda: lo + torch.rand((N, B), device=self.device, generator=generator) * segment[:, None]  # noqa: E731
            prob, data_idx, tree_idx = self.find(draw())
            for _ in range(max_tries):
                bad = ~self._valid(prob, data_idx)
                if not bool(bad.any()):
                    break
                p2, d2, t2 = self.find(draw())
                prob, data_idx, tree_idx = torch.where(bad, p2, prob), torch.where(bad, d2, data_idx), torch.where(bad, t2, tree_idx)
            else:
                raise RuntimeError("could not draw a valid sample from every segment; append more transitions first")
        if self._lib is not None and self.states.dtype == torch.float32 and B <= 256:
            # one launch: transitions, n-step returns, next states, weights -- env-major rows as below
            from . import _lib
            dev, NB = self.device, N * B
            view = _lib.IrbppReplayView(
                states_dev=self.states.data_ptr(), actions_dev=self.actions.data_ptr(), rewards_dev=self.rewards.data_ptr(),
                nonterminals_dev=self.nonterminals.data_ptr(), tree_dev=self.sum_tree.data_ptr(), index_dev=self.index.data_ptr(),
                full_dev=self.full.data_ptr(), scaling_dev=self.n_step_scaling.data_ptr(), n_env=N, capacity=self.capacity,
                obs_len=self.obs_len, n_step=self.n)
            st = torch.empty((NB, self.obs_len), dtype=torch.float32, device=dev)
            nx = torch.empty((NB, self.obs_len), dtype=torch.float32, device=dev)
            ac = torch.empty((NB,), dtype=torch.int64, device=dev)
            re = torch.empty((NB,), dtype=torch.float32, device=dev)
            nt = torch.empty((NB, 1), dtype=torch.float32, device=dev)
            we = torch.empty((NB,), dtype=torch.float32, device=dev)
            _lib.check(self._lib.irbpp_replay_gather(C.byref(view), B, float(self.priority_weight), _p(data_idx.contiguous()),
                                                     _p(prob.contiguous()), _p(st), _p(ac), _p(re), _p(nx), _p(nt), _p(we),
                                                     _stream(dev)), "irbpp_replay_gather")
            return tree_idx, st, ac, re, nx, nt, we
        state, action, returns, next_state, nonterminal = self._transitions(data_idx)
        probs = prob / p_total[:, None]                                           # (:199)
        filled = torch.where(self.full, torch.full_like(self.index, self.capacity), self.index).to(torch.float32)
        weights = (filled[:, None] * probs) ** -self.priority_weight               # (:200-201)
        weights = weights / weights.max(dim=1, keepdim=True).values                # (:202) per memory
        flat = lambda x: x.reshape((N * B,) + tuple(x.shape[2:]))                  # noqa: E731
        return (tree_idx, flat(state).to(torch.float32), flat(action), flat(returns), flat(next_state).to(torch.float32),
                flat(nonterminal).reshape(N * B, 1), flat(weights))

    # ------------------------------------------------------------------ priorities ----------
    def update_priorities(self, tree_idxs: torch.Tensor, priorities: torch.Tensor, powered: bool = False) -> None:
        """ReplayMemory.update_priorities (memory.py:207-209): priority^omega into the listed
        leaves.  Position j of every env is applied before position j+1, so a leaf listed twice
        keeps its last value as in the reference's sequential loop.  The power is taken with
        torch.pow on the device; the reference's ``np.power`` (float32 powf on the host) can differ
        from it in the last bit, so ``powered=True`` accepts values that already are priority^omega
        (used by the parity tests to feed numpy's)."""
        N, B = tree_idxs.shape
        pr = priorities.to(self.device, torch.float32).reshape(N, B)
        if not powered:
            pr = torch.pow(pr, self.priority_exponent)
        if self._lib is not None:                                  # all B leaves of every env in one launch
            from . import _lib
            _lib.check(self._lib.irbpp_sumtree_update(_p(self.sum_tree), _p(self.max), N, self.capacity,
                                                      _p(tree_idxs.to(self.device, torch.int64).contiguous()), _p(pr.contiguous()), B, _p(None),
                                                      _stream(self.device)), "irbpp_sumtree_update")
            return
        for j in range(B):
            self._set_leaves(self._rows, tree_idxs[:, j].to(self.device), pr[:, j])

    # ------------------------------------------------------------------ pooled: the N memories as one ----
    def _view(self):
        from . import _lib
        return _lib.IrbppReplayView(
            states_dev=self.states.data_ptr(), actions_dev=self.actions.data_ptr(), rewards_dev=self.rewards.data_ptr(),
            nonterminals_dev=self.nonterminals.data_ptr(), tree_dev=self.sum_tree.data_ptr(), index_dev=self.index.data_ptr(),
            full_dev=self.full.data_ptr(), scaling_dev=self.n_step_scaling.data_ptr(), n_env=self.N, capacity=self.capacity,
            obs_len=self.obs_len, n_step=self.n)

    def _top_tree(self) -> torch.Tensor:
        """The implicit heap over P leaves (P the power of two >= N): leaf e is the total of env e, padding 0, every
        internal node left + right in float32; [0] is the pooled total."""
        P = 1 << (self.N - 1).bit_length()
        level = torch.zeros((P,), dtype=torch.float32, device=self.device)
        level[:self.N] = self.sum_tree[:, 0]
        levels = [level]
        while level.numel() > 1:
            level = level[0::2] + level[1::2]
            levels.append(level)
        return torch.cat(levels[::-1])

    def _find_pooled(self, top: torch.Tensor, v: torch.Tensor):
        """One walk per value of v[B] through the top tree and on, with the residual value, through the env's own tree
        -> (env, priority, data index, tree index, landed on a padding leaf)."""
        B, P = v.numel(), (top.numel() + 1) // 2
        idx = torch.zeros((B,), dtype=torch.int64, device=self.device)
        v = v.to(device=self.device, dtype=torch.float32).clone()
        for _ in range(P.bit_length() - 1):
            lval = top[2 * idx + 1]
            go_left = v <= lval
            v = torch.where(go_left, v, v - lval)
            idx = torch.where(go_left, 2 * idx + 1, 2 * idx + 2)
        env = idx - (P - 1)
        padding = env >= self.N
        env = env.clamp(max=self.N - 1)
        idx = torch.zeros_like(idx)
        last = 2 * self.capacity - 2
        for _ in range(self._depth):
            left = 2 * idx + 1
            inner = left <= last
            lval = self.sum_tree[env, left.clamp(max=last)]
            go_left = v <= lval
            v = torch.where(inner & ~go_left, v - lval, v)
            idx = torch.where(inner, torch.where(go_left, left, left + 1), idx)
        return env, self.sum_tree[env, idx], idx - (self.capacity - 1), idx, padding

    def _transitions_pooled(self, env: torch.Tensor, data_idx: torch.Tensor):
        """_get_transition_new (memory.py:123-139) for the rows (env[j], data_idx[j]); the return summed in the order of
        irbpp_replay_gather_kernel: ret = ret + r * scaling[t]."""
        pos = data_idx % self.capacity
        d0 = pos
        alive = torch.ones_like(pos, dtype=torch.bool)
        ret = torch.zeros(pos.shape, dtype=torch.float32, device=self.device)
        for t in range(self.n):
            r = torch.where(alive, self.rewards[env, pos], torch.zeros((), device=self.device))
            ret = ret + r * self.n_step_scaling[t]
            alive = alive & self.nonterminals[env, pos]
            pos = (pos + 1) % self.capacity
        last = self.states[env, pos]
        next_state = torch.where(alive[:, None], last, torch.zeros_like(last))
        nonterminal = (alive & self.nonterminals[env, pos]).to(torch.float32)
        return self.states[env, d0], self.actions[env, d0], ret, next_state, nonterminal

    def sample_pooled(self, batch_size: int, values: Optional[torch.Tensor] = None, generator=None, max_tries: int = 64):
        """One learning batch of ``batch_size`` transitions from the N memories taken as ONE prioritised memory, whatever N
        is (``batch_size < N`` included): the draws are stratified over the pooled priority mass T -- draw j is
        ``j * T/B + u * T/B`` -- and walked through a top tree over the N totals and on through that env's own tree; validity
        (memory.py:175, against that env's write index), n-step transitions and the importance weights of memory.py:199-202
        (``filled`` the transitions held by all envs together, normalised by the batch maximum) as in ``sample``.

        ``values`` (optional, [B]) are positions in [0, T) looked up as they are (ValueError if one is invalid); otherwise
        invalid draws are redrawn within their segment up to ``max_tries`` times (RuntimeError after that).
        Returns (idx int64 [B, 2] = (env, tree_idx), states, actions, returns, next_states, nonterminals [B, 1], weights):
        the tuple shape of ``sample``, so ``learn_loss`` takes it unchanged; ``update_priorities_pooled`` takes ``idx``."""
        B, dev = int(batch_size), self.device
        if B < 1:
            raise ValueError("batch_size must be at least 1")
        if values is not None:
            values = values.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if values.numel() != B:
                raise ValueError(f"values must hold {B} positions")
        if self._pool_lib is not None and self.states.dtype == torch.float32:
            from . import _lib
            lib, view = self._pool_lib, self._view()
            seed = 0
            if values is None:
                gdev = "cpu" if generator is None else generator.device
                seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=gdev).item())
            env = torch.empty((B,), dtype=torch.int64, device=dev)
            prob = torch.empty((B,), dtype=torch.float32, device=dev)
            data_idx = torch.empty((B,), dtype=torch.int64, device=dev)
            tree_idx = torch.empty((B,), dtype=torch.int64, device=dev)
            we = torch.empty((B,), dtype=torch.float32, device=dev)
            failed = torch.zeros((1,), dtype=torch.int32, device=dev)
            _lib.check(lib.irbpp_replay_pool_sample(C.byref(view), B, _p(values), seed, int(max_tries), float(self.priority_weight),
                                                    _p(env), _p(prob), _p(data_idx), _p(tree_idx), _p(we), _p(failed), _stream(dev)),
                       "irbpp_replay_pool_sample")
            if int(failed.item()):                                 # the one host round trip, as in sample()
                if values is not None:
                    raise ValueError("a supplied sample position is invalid (memory.py:175)")
                raise RuntimeError("could not draw a valid sample from every segment; append more transitions first")
            st = torch.empty((B, self.obs_len), dtype=torch.float32, device=dev)
            nx = torch.empty((B, self.obs_len), dtype=torch.float32, device=dev)
            ac = torch.empty((B,), dtype=torch.int64, device=dev)
            re = torch.empty((B,), dtype=torch.float32, device=dev)
            nt = torch.empty((B, 1), dtype=torch.float32, device=dev)
            _lib.check(lib.irbpp_replay_pool_gather(C.byref(view), B, _p(env), _p(data_idx), _p(st), _p(ac), _p(re), _p(nx), _p(nt),
                                                    _stream(dev)), "irbpp_replay_pool_gather")
            return torch.stack([env, tree_idx], dim=1), st, ac, re, nx, nt, we
        top = self._top_tree()
        p_total = top[0]
        w = self.index

        def lookup(v):
            env, prob, data_idx, tree_idx, padding = self._find_pooled(top, v)
            ok = (((w[env] - data_idx) % self.capacity > self.n) & ((data_idx - w[env]) % self.capacity >= 1) & (prob != 0) &
                  ~padding)
            return env, prob, data_idx, tree_idx, ok

        if values is not None:
            env, prob, data_idx, tree_idx, ok = lookup(values)
            if not bool(ok.all()):
                raise ValueError("a supplied sample position is invalid (memory.py:175)")
        else:
            segment = p_total / B
            lo = torch.arange(B, device=dev, dtype=torch.float32) * segment
            draw = lambda: lo + torch.rand((B,), device=dev, generator=generator) * segment  # noqa: E731
            env, prob, data_idx, tree_idx, ok = lookup(draw())
            for _ in range(int(max_tries) - 1):
                if bool(ok.all()):
                    break
                e2, p2, d2, t2, ok2 = lookup(draw())
                env, prob, data_idx, tree_idx = (torch.where(ok, a, b) for a, b in ((env, e2), (prob, p2), (data_idx, d2), (tree_idx, t2)))
                ok = ok | ok2
            if not bool(ok.all()):
                raise RuntimeError("could not draw a valid sample from every segment; append more transitions first")
        state, action, returns, next_state, nonterminal = self._transitions_pooled(env, data_idx)
        filled = torch.where(self.full, torch.full_like(self.index, self.capacity), self.index).sum().to(torch.float32)
        weights = (filled * (prob / p_total)) ** -self.priority_weight                # memory.py:199-201 on the pooled memory
        weights = weights / weights.max()                                             # (:202) over the batch
        return (torch.stack([env, tree_idx], dim=1), state.to(torch.float32), action, returns, next_state.to(torch.float32),
                nonterminal.reshape(B, 1), weights)

    def update_priorities_pooled(self, idx: torch.Tensor, priorities: torch.Tensor, powered: bool = False) -> None:
        """``update_priorities`` for the rows of a pooled batch: ``idx`` int64 [B, 2] = (env, tree_idx) as ``sample_pooled``
        returns it, ``priorities`` [B]; priority^omega (``powered=True``: the values already are) goes into the listed
        leaves in list order, so a leaf listed twice keeps its last value, each env's maximum priority takes in every value
        listed for it, and every ancestor of a touched leaf ends as left + right.  Only those leaves and their ancestors are
        touched.  A row whose tree_idx is no leaf or whose env is outside [0, N) is ignored."""
        dev = self.device
        idx = idx.to(device=dev, dtype=torch.int64).reshape(-1, 2)
        B = idx.shape[0]
        pr = priorities.to(dev, torch.float32).reshape(B)
        if not powered:
            pr = torch.pow(pr, self.priority_exponent)
        env, ti = idx[:, 0].contiguous(), idx[:, 1].contiguous()
        if self._pool_lib is not None:
            from . import _lib
            _lib.check(self._pool_lib.irbpp_replay_pool_update(_p(self.sum_tree), _p(self.max), self.N, self.capacity, _p(env), _p(ti),
                                                               _p(pr.contiguous()), B, _stream(dev)), "irbpp_replay_pool_update")
            return
        cap = self.capacity
        keep = (env >= 0) & (env < self.N) & (ti >= cap - 1) & (ti <= 2 * cap - 2)
        env, ti, pr = env[keep], ti[keep], pr[keep]
        if env.numel() == 0:
            return
        self.max.scatter_reduce_(0, env, pr, reduce="amax", include_self=True)        # overwritten duplicates included
        key = env * (2 * cap - 1) + ti
        live = ~torch.triu(key[:, None] == key[None, :], diagonal=1).any(dim=1)       # no later triple names the same leaf
        env, node, pr = env[live], ti[live], pr[live]
        self.sum_tree[env, node] = pr
        # ancestors by actual depth floor(log2(idx + 1)), deepest level first (a capacity that is no power of two has its
        # leaves at two depths); rows that meet at a node write the same sum of the same final children
        depth = torch.floor(torch.log2((node + 1).to(torch.float64))).to(torch.int64)
        for d in range((2 * cap - 1).bit_length() - 1, 0, -1):
            at = depth == d
            node = torch.where(at, (node - 1) // 2, node)
            e, i = env[at], node[at]
            self.sum_tree[e, i] = self.sum_tree[e, 2 * i + 1] + self.sum_tree[e, 2 * i + 2]
            depth = torch.where(at, depth - 1, depth)

    def anneal(self, increase: float) -> None:
        """trainer.py:195-196."""
        self.priority_weight = min(self.priority_weight + increase, 1.0)

    def __len__(self) -> int:
        return self.N


def mask_from_state(state: torch.Tensor, selected_action: int) -> torch.Tensor:
    """get_mask_from_state (tools.py:283-300) for the candidate-selection layout: column 4 of the
    [S, 5] block is the validity flag of each candidate."""
    return state[:, :selected_action * 5].reshape(state.shape[0], selected_action, 5)[:, :, -1]


def masked_greedy_action(q: torch.Tensor, state: torch.Tensor, selected_action: int) -> torch.Tensor:
    """The tail of Agent.act (agent.py:55-58): ``q[(1 - mask).bool()] = -inf; q.argmax(1)`` with the mask taken from
    the observation (get_mask_from_state).  On a HIP device one kernel reads the flags straight from ``state``."""
    lib = _hip_lib(q.device)
    if lib is None:
        masked = q.masked_fill(mask_from_state(state, selected_action) == 0, float("-inf"))
        return masked.argmax(1)
    from . import _lib
    q = q.to(torch.float32).contiguous()
    state = state.to(torch.float32).contiguous()         # the kernel reads the validity flags as float32
    out = torch.empty((q.shape[0],), dtype=torch.int64, device=q.device)
    _lib.check(lib.irbpp_masked_argmax(_p(q), q.stride(0), _p(state), state.stride(0), int(selected_action), q.shape[0],
                                       _p(out), _stream(q.device)), "irbpp_masked_argmax")
    return out


# Which form the two distributional-head wrappers below take on a HIP device when the caller does not say (use_hip=None).
# The torch lines: tools/c51_head_rates.py on an MI355X found the act kernel faster than them at 4096 environments but slower
# at 1024 ("The distributional head"; profiles/c51_head/): use_hip=True asks for the kernels.
C51_HIP_DEFAULT = False


def _head_lib(t: torch.Tensor, use_hip: Optional[bool], default: bool):
    """The library if a head wrapper is to take its kernels on t's device, else None; ``default``: its *_HIP_DEFAULT."""
    lib = _hip_lib(t.device)
    if use_hip and lib is None:
        raise RuntimeError("use_hip=True needs a HIP device")
    return lib if (default if use_hip is None else use_hip) else None


def _f32(x: torch.Tensor, device) -> torch.Tensor:
    return x.to(device=device, dtype=torch.float32).contiguous()


def _obs_arg(state: Optional[torch.Tensor]):
    """(state as float32 with contiguous rows, its env stride); (None, 0) without a mask."""
    if state is None:
        return None, 0
    state = state.to(torch.float32)
    if state.stride(1) != 1:
        state = state.contiguous()
    return state, state.stride(0)


def _q_out_arg(q_out: Optional[torch.Tensor], N: int, S: int, device, name: str) -> int:
    """q_out's row stride (0 without one); ``name``: the caller's word for the tensor whose device q_out must share."""
    if q_out is None:
        return 0
    if q_out.dtype != torch.float32 or q_out.device != device or tuple(q_out.shape) != (N, S) or q_out.stride(1) != 1:
        raise ValueError(f"q_out must be a float32 [N, S] tensor on {name}'s device with contiguous rows")
    return q_out.stride(0)


def _c51_block(p: torch.Tensor) -> torch.Tensor:
    """float32 [N, S, atoms] with the atoms contiguous, whatever the row and env strides (slices pass as they are)."""
    if p.dim() != 3:
        raise ValueError("probabilities must be [N, S, atoms]")
    p = p.to(torch.float32)
    ok = p.stride(2) == 1 and p.stride(1) >= p.shape[2] and p.stride(0) >= (p.shape[1] - 1) * p.stride(1) + p.shape[2]
    return p if ok else p.contiguous()


def distributional_greedy_action(p: torch.Tensor, support: torch.Tensor, state: Optional[torch.Tensor] = None,
                                 selected_action: Optional[int] = None, q_out: Optional[torch.Tensor] = None, *,
                                 use_hip: Optional[bool] = None) -> torch.Tensor:
    """All of Agent.act after the network (agent.py:51-58): ``(p * support).sum(2)``, ``-inf`` where the observation's
    validity flag is 0 (``state=None``: no mask, as orderDQN.act(state, None) at trainer.py:266), ``argmax(1)`` -> int64[N].
    ``p`` is the network's [N, S, atoms] probabilities, ``support`` the caller's ``torch.linspace(Vmin, Vmax, atoms)``;
    ``q_out`` (optional float32 [N, S]) receives the unmasked expected values (evaluate_q, logging).  With ``use_hip=True``
    (a HIP device; ``None`` takes C51_HIP_DEFAULT) one kernel reads ``p`` once and sums each row's atoms left to right in
    float32 (irbpp_categorical_act: reproducible bit for bit); otherwise, and on the CPU, the reference's torch lines run."""
    N, S, atoms = p.shape
    if selected_action is not None and int(selected_action) != S:
        raise ValueError(f"selected_action {selected_action} != {S} candidate rows")
    lib = _head_lib(p, use_hip, C51_HIP_DEFAULT)
    if lib is None:
        q = (p * support).sum(2)
        if q_out is not None:
            q_out.copy_(q)
        if state is not None:
            q[(1 - mask_from_state(state, S)).bool()] = float("-inf")
        return q.argmax(1)
    from . import _lib
    p = _c51_block(p)
    support = _f32(support, p.device)
    state, obs_stride = _obs_arg(state)
    q_stride = _q_out_arg(q_out, N, S, p.device, "p")
    out = torch.empty((N,), dtype=torch.int64, device=p.device)
    _lib.check(lib.irbpp_categorical_act(_p(p), p.stride(0), p.stride(1), _p(support), atoms, _p(state), obs_stride, S, N, _p(out),
                                         _p(q_out), q_stride, _stream(p.device)), "irbpp_categorical_act")
    return out


def c51_target(p_online: torch.Tensor, p_target: torch.Tensor, returns: torch.Tensor, nonterminals: torch.Tensor,
               support: torch.Tensor, gamma_n: float, v_min: float, v_max: float, *,
               use_hip: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Agent.learn between the two forwards and the loss (agent.py:90-115): the double-Q selection
    ``a_star = (support * p_online).sum(2).argmax(1)``, ``pns_a = p_target[range(B), a_star]`` and the projection of
    ``Tz = returns + nonterminals * gamma_n * support`` onto the support -> (m float32 [B, atoms], a_star int64 [B]).
    ``gamma_n`` is ``discount ** n``.  With ``use_hip=True`` (a HIP device; ``None`` takes C51_HIP_DEFAULT) one kernel does it
    without atomics (irbpp_categorical_target: ``m`` is the same from run to run, which torch's index_add_ on the GPU is
    not); otherwise, and on the CPU, the reference's torch lines run."""
    B, S, atoms = p_online.shape
    if tuple(p_target.shape) != (B, S, atoms):
        raise ValueError("p_online and p_target must have the same [B, S, atoms] shape")
    delta_z = (v_max - v_min) / (atoms - 1)
    returns, nonterminals = returns.reshape(B), nonterminals.reshape(B)
    lib = _head_lib(p_online, use_hip, C51_HIP_DEFAULT)
    if lib is None:
        a_star = (support.expand_as(p_online) * p_online).sum(2).argmax(1)
        pns_a = p_target[torch.arange(B, device=p_target.device), a_star]
        Tz = returns.unsqueeze(1) + nonterminals.unsqueeze(1) * gamma_n * support.unsqueeze(0)
        Tz = Tz.clamp(min=v_min, max=v_max)
        b = (Tz - v_min) / delta_z
        l, u = b.floor().to(torch.int64), b.ceil().to(torch.int64)
        l[(u > 0) * (l == u)] -= 1
        u[(l < (atoms - 1)) * (l == u)] += 1
        m = p_target.new_zeros(B, atoms)
        offset = (torch.arange(B, device=m.device) * atoms).unsqueeze(1).expand(B, atoms)
        m.view(-1).index_add_(0, (l + offset).view(-1), (pns_a * (u.float() - b)).view(-1))
        m.view(-1).index_add_(0, (u + offset).view(-1), (pns_a * (b - l.float())).view(-1))
        return m, a_star
    from . import _lib
    dev = p_online.device
    p_online, p_target = _c51_block(p_online), _c51_block(p_target)
    returns, nonterminals, support = _f32(returns, dev), _f32(nonterminals, dev), _f32(support, dev)
    m = torch.empty((B, atoms), dtype=torch.float32, device=dev)
    a_star = torch.empty((B,), dtype=torch.int64, device=dev)
    _lib.check(lib.irbpp_categorical_target(_p(p_online), p_online.stride(0), p_online.stride(1), _p(p_target), p_target.stride(0),
                                            p_target.stride(1), _p(returns), _p(nonterminals), _p(support), atoms, S, B, float(gamma_n),
                                            float(v_min), float(v_max), float(delta_z), _p(m), _p(a_star), _stream(dev)),
               "irbpp_categorical_target")
    return m, a_star


# The same question for the two wrappers below, which start from the network's logits ("The dueling
# head"): the kernels, since tools/dueling_head_rates.py measured them on an MI355X at 0.22 ms against 0.63 ms for the torch
# lines (4096 envs) and 0.031 ms against 0.48 ms (a learn batch of 64), far outside the spread (profiles/dueling_head/).
DUELING_HIP_DEFAULT = True


def _dueling_logits(v: torch.Tensor, a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(v [N, atoms] or [N, 1, atoms], a [N, S, atoms]) -> v as [N, atoms]; shapes checked."""
    if a.dim() != 3:
        raise ValueError("a must be [N, S, atoms]")
    N, _, atoms = a.shape
    if v.dim() == 3 and v.shape[1] == 1:
        v = v[:, 0]
    if tuple(v.shape) != (N, atoms):
        raise ValueError(f"v must be [{N}, {atoms}] (or [{N}, 1, {atoms}]) beside a {tuple(a.shape)}")
    return v, a


def _dueling_softmax(v: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """model.py:395-400 (log=False) on v [N, atoms], a [N, S, atoms]."""
    v = v.unsqueeze(1)
    q = v + a - a.mean(1, keepdim=True)
    return torch.softmax(q, dim=2)


def _dueling_v(v: torch.Tensor) -> torch.Tensor:
    v = v.to(torch.float32)
    return v if v.stride(1) == 1 and v.stride(0) >= v.shape[1] else v.contiguous()


def dueling_greedy_action(v: torch.Tensor, a: torch.Tensor, support: torch.Tensor, state: Optional[torch.Tensor] = None,
                          selected_action: Optional[int] = None, q_out: Optional[torch.Tensor] = None,
                          p_out: Optional[torch.Tensor] = None, *, use_hip: Optional[bool] = None) -> torch.Tensor:
    """The end of DQNBPP.forward (model.py:395-400: ``v + a - a.mean(1)``, softmax over the atoms) and all of Agent.act after it
    (agent.py:51-58), from the value logits ``v`` [N, atoms] (or [N, 1, atoms]) and the advantage logits ``a`` [N, S, atoms]
    -> int64[N].  ``state`` / ``selected_action`` / ``q_out`` as in distributional_greedy_action; ``p_out`` (optional,
    contiguous float32 [N, S, atoms]) receives the probabilities.  With ``use_hip=True`` (a HIP device; ``None`` takes
    DUELING_HIP_DEFAULT) one kernel does all of it in a defined float32 arithmetic (irbpp_dueling_act: reproducible bit for
    bit, the probabilities stay in LDS unless ``p_out`` is given); otherwise, and on the CPU, the reference's torch lines run."""
    v, a = _dueling_logits(v, a)
    N, S, atoms = a.shape
    if selected_action is not None and int(selected_action) != S:
        raise ValueError(f"selected_action {selected_action} != {S} candidate rows")
    lib = _head_lib(a, use_hip, DUELING_HIP_DEFAULT)
    if lib is None:
        p = _dueling_softmax(v, a)
        if p_out is not None:
            p_out.copy_(p)
        return distributional_greedy_action(p, support, state, selected_action, q_out, use_hip=False)
    from . import _lib
    v, a = _dueling_v(v), _c51_block(a)
    support = _f32(support, a.device)
    state, obs_stride = _obs_arg(state)
    q_stride = _q_out_arg(q_out, N, S, a.device, "a")
    if p_out is not None and (p_out.dtype != torch.float32 or p_out.device != a.device or tuple(p_out.shape) != (N, S, atoms) or
                              not p_out.is_contiguous()):
        raise ValueError("p_out must be a contiguous float32 [N, S, atoms] tensor on a's device")
    out = torch.empty((N,), dtype=torch.int64, device=a.device)
    _lib.check(lib.irbpp_dueling_act(_p(v), v.stride(0), _p(a), a.stride(0), a.stride(1), _p(support), atoms, _p(state), obs_stride,
                                     S, N, _p(out), _p(q_out), q_stride, _p(p_out), _stream(a.device)), "irbpp_dueling_act")
    return out


def dueling_c51_target(v_online: torch.Tensor, a_online: torch.Tensor, v_target: torch.Tensor, a_target: torch.Tensor,
                       returns: torch.Tensor, nonterminals: torch.Tensor, support: torch.Tensor, gamma_n: float, v_min: float,
                       v_max: float, *, use_hip: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Agent.learn's no_grad block (agent.py:90-115) from the logits of the online and the target network (each ``v``
    [B, atoms] or [B, 1, atoms], ``a`` [B, S, atoms]) -> (m float32 [B, atoms], a_star int64 [B]); the other arguments as in
    c51_target.  With ``use_hip=True`` (a HIP device; ``None`` takes DUELING_HIP_DEFAULT) one kernel does it
    (irbpp_dueling_target: neither network's probabilities are written; of the target net's only row a_star is computed);
    otherwise, and on the CPU, the reference's torch lines run."""
    v_online, a_online = _dueling_logits(v_online, a_online)
    v_target, a_target = _dueling_logits(v_target, a_target)
    B, S, atoms = a_online.shape
    if tuple(a_target.shape) != (B, S, atoms):
        raise ValueError("a_online and a_target must have the same [B, S, atoms] shape")
    lib = _head_lib(a_online, use_hip, DUELING_HIP_DEFAULT)
    if lib is None:
        return c51_target(_dueling_softmax(v_online, a_online), _dueling_softmax(v_target, a_target), returns, nonterminals,
                          support, gamma_n, v_min, v_max, use_hip=False)
    from . import _lib
    dev = a_online.device
    delta_z = (v_max - v_min) / (atoms - 1)
    v_online, v_target, a_online, a_target = _dueling_v(v_online), _dueling_v(v_target), _c51_block(a_online), _c51_block(a_target)
    returns, nonterminals, support = _f32(returns.reshape(B), dev), _f32(nonterminals.reshape(B), dev), _f32(support, dev)
    m = torch.empty((B, atoms), dtype=torch.float32, device=dev)
    a_star = torch.empty((B,), dtype=torch.int64, device=dev)
    _lib.check(lib.irbpp_dueling_target(_p(v_online), v_online.stride(0), _p(a_online), a_online.stride(0), a_online.stride(1),
                                        _p(v_target), v_target.stride(0), _p(a_target), a_target.stride(0), a_target.stride(1),
                                        _p(returns), _p(nonterminals), _p(support), atoms, S, B, float(gamma_n), float(v_min),
                                        float(v_max), float(delta_z), _p(m), _p(a_star), _stream(dev)), "irbpp_dueling_target")
    return m, a_star


# The same question for the loss below ("The dueling loss"): the kernels, since tools/dueling_loss_rates.py
# measured forward + backward on an MI355X at 0.189 ms against 0.311 ms for the torch lines at a batch of 64 and 0.225 ms against
# 0.425 ms at 512, with spreads of at most 0.031 ms (profiles/dueling_loss/).
DUELING_LOSS_HIP_DEFAULT = True


class _DuelingLossFunction(torch.autograd.Function):
    """irbpp_dueling_loss / irbpp_dueling_loss_backward around autograd: v float32 [B, atoms] and a float32 [B, S, atoms] as
    _dueling_v / _c51_block leave them, actions int64 [B] and m float32 [B, atoms] contiguous, all on one HIP device."""

    @staticmethod
    def forward(ctx, v, a, actions, m, pinned):
        from . import _lib
        lib = _lib.load()
        B, S, atoms = a.shape
        loss = torch.empty((B,), dtype=torch.float32, device=a.device)
        g = torch.empty((B, atoms), dtype=torch.float32, device=a.device)
        _lib.check(lib.irbpp_dueling_loss(_p(v), v.stride(0), _p(a), a.stride(0), a.stride(1), _p(actions), _p(m), atoms, S, B,
                                          _p(loss), _p(g), _stream(a.device)), "irbpp_dueling_loss")
        ctx.save_for_backward(g, actions, v, a, m)            # v, a and m only for their version check: g holds what they gave
        ctx.rows, ctx.pinned = S, pinned
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        need_v, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_v or need_a):
            return None, None, None, None, None
        from . import _lib
        lib = _lib.load()
        g, actions = ctx.saved_tensors[:2]                    # raises if one of the five was written in place since the forward
        _check_pinned(ctx.pinned, "dueling_c51_loss")
        B, atoms = g.shape
        grad_loss = grad_loss.to(torch.float32).contiguous()      # loss.sum().backward() hands over a stride-0 expanded tensor
        grad_v = torch.empty((B, atoms), dtype=torch.float32, device=g.device) if need_v else None
        grad_a = torch.empty((B, ctx.rows, atoms), dtype=torch.float32, device=g.device) if need_a else None
        _lib.check(lib.irbpp_dueling_loss_backward(_p(g), _p(grad_loss), _p(actions), atoms, ctx.rows, B, _p(grad_v), _p(grad_a),
                                                   _stream(g.device)), "irbpp_dueling_loss_backward")
        return grad_v, grad_a, None, None, None


def dueling_c51_loss(v: torch.Tensor, a: torch.Tensor, actions: torch.Tensor, m: torch.Tensor, *,
                     use_hip: Optional[bool] = None) -> torch.Tensor:
    """The part of Agent.learn that carries the gradient, from the online network's logits of ``states`` (``v`` [B, atoms] or
    [B, 1, atoms], ``a`` [B, S, atoms]): the end of DQNBPP.forward with log=True (model.py:395-398: ``v + a - a.mean(1)``,
    log_softmax over the atoms), ``log_ps[range(B), actions]`` and ``-torch.sum(m * log_ps_a, 1)`` (agent.py:85-86, 117)
    -> loss float32 [B], differentiable with respect to ``v`` and ``a``; ``m`` (dueling_c51_target's) is a constant.  With
    ``use_hip=True`` (a HIP device; ``None`` takes DUELING_LOSS_HIP_DEFAULT) one kernel computes the loss in a defined float32
    arithmetic (irbpp_dueling_loss: only the action's row and the column means, no [B, S, atoms] log-probabilities) and one
    more writes the gradients (irbpp_dueling_loss_backward, only the sides that require one; ``v.grad`` in the shape ``v``
    was given in); an action outside [-S, S) then gives a NaN loss and zero gradients; an in-place write to ``v``, ``a``,
    ``actions`` or ``m`` before the backward makes it raise autograd's "modified by an inplace operation" RuntimeError.
    Otherwise, and on the CPU, the reference's torch lines run under ordinary autograd (and refuse such an action as torch
    indexing does): torch's own graph keeps ``actions`` and ``m`` to that rule and never reads ``v`` or ``a`` again."""
    v, a = _dueling_logits(v, a)
    B, S, atoms = a.shape
    if tuple(actions.shape) != (B,) or actions.dtype.is_floating_point:
        raise ValueError(f"actions must be {B} integers")
    if tuple(m.shape) != (B, atoms):
        raise ValueError(f"m must be [{B}, {atoms}]")
    m = m.detach()
    if _head_lib(a, use_hip, DUELING_LOSS_HIP_DEFAULT) is None:
        q = v.unsqueeze(1) + a - a.mean(1, keepdim=True)
        log_ps = torch.log_softmax(q, dim=2)
        log_ps_a = log_ps[torch.arange(B, device=a.device), actions.to(device=a.device, dtype=torch.int64)]
        return -torch.sum(m.to(a.device) * log_ps_a, 1)
    dev = a.device
    return _DuelingLossFunction.apply(_dueling_v(v), _c51_block(a), actions.to(device=dev, dtype=torch.int64).contiguous(),
                                      _f32(m, dev), _pinned(v, a, actions, m))


def learn_loss(online_logits, target_logits, batch, support: torch.Tensor, gamma_n: float, v_min: float, v_max: float, *,
               use_hip: Optional[bool] = None) -> torch.Tensor:
    """Agent.learn from the sampled batch to the per-sample loss (agent.py:84-117) as three network calls and two head calls.
    ``online_logits`` / ``target_logits`` are callables ``states -> (v, a)``: the networks up to their logits (DQNBPP.forward
    before model.py:395); ``batch`` is what VectorReplayMemory.sample returns.  -> loss float32 [B], attached to the online
    network's graph.  What stays the caller's (agent.py:118-124)::

        tree_idxs, *_, weights = batch
        loss = learn_loss(online_net.logits, target_net.logits, batch, support, discount ** n, Vmin, Vmax)
        online_net.zero_grad()
        (weights * loss).mean().backward()
        clip_grad_norm_(online_net.parameters(), norm_clip)
        optimiser.step()
        memory.update_priorities(tree_idxs, loss.detach())

    or, with ``optimiser = optim.ClippedAdam(online_net.parameters(), lr, betas, eps, norm_clip, grads="zero",
    target_params=target_net.parameters())`` (irbpp_amd/optim.py: the clip, Adam, the next zero_grad and the target's
    parameter copy as two launches)::

        (weights * loss).mean().backward()
        optimiser.step(sync_target=T % target_update == 0)
        memory.update_priorities(tree_idxs, loss.detach())

    ``use_hip`` is handed to both head calls (``None``: each one's own default)."""
    _, states, actions, returns, next_states, nonterminals, _ = batch
    v, a = online_logits(states)
    with torch.no_grad():
        v_on, a_on = online_logits(next_states)
        v_tg, a_tg = target_logits(next_states)
        m, _ = dueling_c51_target(v_on, a_on, v_tg, a_tg, returns, nonterminals, support, gamma_n, v_min, v_max, use_hip=use_hip)
    return dueling_c51_loss(v, a, actions, m, use_hip=use_hip)


# The same question for the streams in front of the dueling head ("The noisy streams"): torch's layers
# followed by dueling_greedy_action, since tools/streams_rates.py measured them on an MI355X at 1.79 ms against 5.76 ms for the
# fused call at 4096 envs and 0.47 ms against 1.46 ms at 1024 (profiles/noisy_streams/): the matrix units win over the defined
# fmaf chain.  use_hip=True asks for the kernels (the reproducible forward).  form="mfma" runs the same chains on the matrix
# cores, the same bits: 2.38 ms and 0.62 ms at the two sizes in a later run of the same tool ("The noisy
# streams on the matrix cores"), still behind torch's layers, so the default stays.
STREAMS_HIP_DEFAULT = False

STREAMS_MAX_WIDTH, STREAMS_MAX_ATOMS, STREAMS_MAX_ROWS = 256, 128, 1024
_STREAM_LAYERS = ("fc_h_v", "fc_z_v", "fc_h_a", "fc_z_a")


class _IrbppStreamWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_hv", "b_hv", "w_zv", "b_zv", "w_ha", "b_ha", "w_za", "b_za")] + \
               [("embed", C.c_int32), ("hidden", C.c_int32), ("atoms", C.c_int32)]


def _fmaf_np(a, b, c):
    """fmaf on float32 numpy arrays, exactly: the product of two float32 is exact in float64; the float64 sum is brought to
    round-to-odd by its TwoSum error, which makes the final rounding to float32 the single rounding of the exact value."""
    import numpy as np
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = np.broadcast_to(c, p.shape).astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64)
        fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
        step = np.where((err > 0) == (s > 0), 1, -1)
        return np.where(fix, bits + step, bits).view(np.float64).astype(np.float32)


def _lin_np(w, b, x):
    """The defined linear layer on float32 numpy arrays: x [..., K], w [J, K], b [J] -> [..., J], one fmaf chain per output."""
    import numpy as np
    acc = np.broadcast_to(b, x.shape[:-1] + b.shape).astype(np.float32)
    for k in range(w.shape[1]):
        acc = _fmaf_np(x[..., k:k + 1], w[:, k], acc)
    return acc


def _streams_logits_cpu(x: torch.Tensor, xg: torch.Tensor, w: "StreamWeights") -> Tuple[torch.Tensor, torch.Tensor]:
    import numpy as np
    relu = lambda t: np.where(t > 0, t, np.float32(0))   # noqa: E731
    n = lambda t: t.detach().to(torch.float32).cpu().numpy()  # noqa: E731
    v = _lin_np(n(w.w_zv), n(w.b_zv), relu(_lin_np(n(w.w_hv), n(w.b_hv), n(xg))))
    a = _lin_np(n(w.w_za), n(w.b_za), relu(_lin_np(n(w.w_ha), n(w.b_ha), n(x))))
    return torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(np.ascontiguousarray(a))


class StreamWeights(object):
    """The four effective layers of DQNBPP's value and advantage streams (model.py:393-394) as float32 device tensors, row-major
    [out][in]: what streams_greedy_action / streams_logits multiply by.  Built from any four objects that expose
    ``weight_mu / weight_sigma / weight_epsilon / bias_mu / bias_sigma / bias_epsilon`` (the reference's NoisyLinear): with
    ``training=True`` the effective weights are ``mu + sigma * epsilon`` (irbpp_noisy_weights on a HIP device, torch's two ops
    on the CPU: the same bits), with ``training=False`` the ``mu`` tensors as they are.  Call ``refresh()`` after every
    ``reset_noise`` (and after every optimiser step that changes mu or sigma)."""

    def __init__(self, fc_h_v, fc_z_v, fc_h_a, fc_z_a, training: bool = True):
        self.layers = (fc_h_v, fc_z_v, fc_h_a, fc_z_a)
        self.training = bool(training)
        self.hidden, self.embed = (int(d) for d in fc_h_v.weight_mu.shape)
        self.atoms = int(fc_z_v.weight_mu.shape[0])
        want = [(self.hidden, self.embed), (self.atoms, self.hidden), (self.hidden, self.embed), (self.atoms, self.hidden)]
        for name, layer, shape in zip(_STREAM_LAYERS, self.layers, want):
            if tuple(layer.weight_mu.shape) != shape or tuple(layer.bias_mu.shape) != shape[:1]:
                raise ValueError(f"{name}: weight_mu {tuple(layer.weight_mu.shape)} beside the expected {shape}")
        if not (1 <= self.embed <= STREAMS_MAX_WIDTH and 1 <= self.hidden <= STREAMS_MAX_WIDTH and
                2 <= self.atoms <= STREAMS_MAX_ATOMS):
            raise ValueError("streams: 1 <= embed, hidden <= 256 and 2 <= atoms <= 128")
        self.device = fc_h_v.weight_mu.device
        self.refresh()

    @classmethod
    def from_layers(cls, fc_h_v, fc_z_v, fc_h_a, fc_z_a, training: bool = True) -> "StreamWeights":
        return cls(fc_h_v, fc_z_v, fc_h_a, fc_z_a, training)

    @torch.no_grad()
    def refresh(self) -> "StreamWeights":
        lib = _hip_lib(self.device)
        out = []
        for layer in self.layers:
            t = [_f32(getattr(layer, n).detach(), self.device) for n in ("weight_mu", "weight_sigma", "weight_epsilon", "bias_mu",
                                                                         "bias_sigma", "bias_epsilon")]
            if not self.training:
                out += [t[0].clone(), t[3].clone()]
            elif lib is None:
                out += [t[0] + t[1] * t[2], t[3] + t[4] * t[5]]
            else:
                from . import _lib
                w, b = torch.empty_like(t[0]), torch.empty_like(t[3])
                _lib.check(lib.irbpp_noisy_weights(*(_p(x) for x in t), t[0].shape[0], t[0].shape[1], _p(w), _p(b),
                                                   _stream(self.device)), "irbpp_noisy_weights")
                out += [w, b]
        self.w_hv, self.b_hv, self.w_zv, self.b_zv, self.w_ha, self.b_ha, self.w_za, self.b_za = out
        return self

    def _struct(self) -> _IrbppStreamWeights:
        return _IrbppStreamWeights(*(x.data_ptr() for x in (self.w_hv, self.b_hv, self.w_zv, self.b_zv, self.w_ha, self.b_ha, self.w_za,
                                                            self.b_za)), self.embed, self.hidden, self.atoms)


def _streams_inputs(x: torch.Tensor, x_global: torch.Tensor, w: StreamWeights) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [N, S, E] and x_global [N, E] (or [N, 1, E]) as float32 with contiguous rows, slices as they are; limits checked."""
    if x.dim() != 3 or x.shape[2] != w.embed:
        raise ValueError(f"x must be [N, S, {w.embed}]")
    N, S, _ = x.shape
    if x_global.dim() == 3 and x_global.shape[1] == 1:
        x_global = x_global[:, 0]
    if tuple(x_global.shape) != (N, w.embed):
        raise ValueError(f"x_global must be [{N}, {w.embed}] (or [{N}, 1, {w.embed}]) beside x {tuple(x.shape)}")
    if not (N >= 1 and 1 <= S <= STREAMS_MAX_ROWS):
        raise ValueError("streams: N >= 1 and 1 <= S <= 1024")
    return _c51_block(x), _dueling_v(x_global)


STREAMS_FORMS = ("chain", "mfma")


def _streams_form(form: str, w: "StreamWeights") -> str:
    """``form`` of the HIP path: "chain" (irbpp_streams_act, one fmaf chain per thread) or "mfma" (irbpp_streams_act_mfma, the
    same chains on the matrix cores: the same bits).  "mfma" needs embed and hidden to be multiples of 4 and says so."""
    if form not in STREAMS_FORMS:
        raise ValueError(f"streams: form must be one of {STREAMS_FORMS}, not {form!r}")
    if form == "mfma" and (w.embed % 4 or w.hidden % 4):
        raise ValueError(f"streams: form='mfma' needs embed and hidden to be multiples of 4 (embed {w.embed}, hidden {w.hidden})")
    return form


def _streams_call(lib, x, xg, w, support, state, q_out, want_action, want_logits, form="chain"):
    from . import _lib
    name = "irbpp_streams_act_mfma" if form == "mfma" else "irbpp_streams_act"
    N, S, _ = x.shape
    dev = x.device
    fits = S * (w.atoms | 1) * 4 <= 144 * 1024           # DUELING_TILE_BYTES: a larger block needs a_out as its workspace
    state, obs_stride = _obs_arg(state)
    q_stride = _q_out_arg(q_out, N, S, dev, "x")
    action = torch.empty((N,), dtype=torch.int64, device=dev) if want_action else None
    v = torch.empty((N, w.atoms), dtype=torch.float32, device=dev) if want_logits else None
    a = torch.empty((N, S, w.atoms), dtype=torch.float32, device=dev) if want_logits or not fits else None
    ws = w._struct()
    _lib.check(getattr(lib, name)(C.byref(ws), _p(xg), xg.stride(0), _p(x), x.stride(0), x.stride(1), _p(support), _p(state),
                                  obs_stride, S, N, _p(action), _p(q_out), q_stride, _p(v), _p(a), _stream(dev)), name)
    return action, v, a


@torch.no_grad()
def streams_greedy_action(x: torch.Tensor, x_global: torch.Tensor, weights: StreamWeights, support: torch.Tensor,
                          state: Optional[torch.Tensor] = None, *, q_out: Optional[torch.Tensor] = None,
                          use_hip: Optional[bool] = None, form: str = "chain") -> torch.Tensor:
    """The last stage of DQNBPP.forward (model.py:393-400: the four noisy layers of the value and advantage streams, the
    combine and the softmax) and all of Agent.act after it (agent.py:51-58), from the embeddings ``x`` [N, S, E] and
    ``x_global`` [N, E] (or [N, 1, E]) -> int64[N].  ``weights``: a StreamWeights; ``support`` / ``state`` / ``q_out`` as in
    dueling_greedy_action.  With ``use_hip=True`` (a HIP device; ``None`` takes STREAMS_HIP_DEFAULT) one kernel does all of it
    in a defined float32 arithmetic (irbpp_streams_act: every layer output one ascending fmaf chain, then the arithmetic of
    irbpp_dueling_act; neither the hidden block nor the logits reach memory).  Otherwise the same definition runs in two steps:
    streams_logits (on the CPU an exact numpy emulation of the chains, on a HIP device torch's layers) and
    dueling_greedy_action.  ``form`` chooses between the two kernels of the HIP path, which give the same bits: "chain"
    (irbpp_streams_act) or "mfma" (irbpp_streams_act_mfma, the chains on the matrix cores; embed and hidden multiples of 4, a
    ValueError otherwise); the other paths have one form and ignore it."""
    x, xg = _streams_inputs(x, x_global, weights)
    lib = _head_lib(x, use_hip, STREAMS_HIP_DEFAULT)
    if lib is None:
        v, a = streams_logits(x, xg, weights, use_hip=False)
        return dueling_greedy_action(v, a, support, state, None, q_out, use_hip=None if x.is_cuda else False)
    return _streams_call(lib, x, xg, weights, _f32(support, x.device), state, q_out, True, False, _streams_form(form, weights))[0]


@torch.no_grad()
def streams_logits(x: torch.Tensor, x_global: torch.Tensor, weights: StreamWeights, *,
                   use_hip: Optional[bool] = None, form: str = "chain") -> Tuple[torch.Tensor, torch.Tensor]:
    """The value and advantage streams alone, without a gradient: -> (v float32 [N, atoms], a float32 [N, S, atoms]), what
    dueling_c51_target consumes (the two no_grad network calls of Agent.learn, agent.py:90, 96).  Forms as in
    streams_greedy_action; on a HIP device without the kernels torch's ``F.linear`` / ``relu`` lines run (rocBLAS's own
    summation order: close to, not bit-equal with, the definition).  ``form`` as in streams_greedy_action."""
    x, xg = _streams_inputs(x, x_global, weights)
    lib = _head_lib(x, use_hip, STREAMS_HIP_DEFAULT)
    if lib is not None:
        _, v, a = _streams_call(lib, x, xg, weights, None, None, None, False, True, _streams_form(form, weights))
        return v, a
    if x.is_cuda:
        F = torch.nn.functional
        w = weights
        return (F.linear(F.relu(F.linear(xg, w.w_hv, w.b_hv)), w.w_zv, w.b_zv),
                F.linear(F.relu(F.linear(x, w.w_ha, w.b_ha)), w.w_za, w.b_za))
    return _streams_logits_cpu(x, xg, weights)


# The streams in the forward that carries a gradient ("The noisy streams with a gradient"): torch's four
# layers under autograd or the forward's kernel and the launches of irbpp_streams_backward.  Torch's layers, since
# tools/streams_grad_rates.py measured forward plus backward on an MI355X at 0.99 ms against 1.63 ms for the kernels (1.46 ms
# with form="mfma") at B = 64, S = 500, widths 128, 31 atoms, and 2.49 against 3.05 (2.57) ms at B = 512
# (profiles/streams_grad/): the kernels are ahead at neither size; what they buy is a backward that gives the same bits on
# every run.  use_hip=True asks for the kernels.
STREAMS_GRAD_HIP_DEFAULT = False

STREAMS_GRAD_MAX_BATCH = 1024
_NOISY_PARAMS = ("weight_mu", "weight_sigma", "bias_mu", "bias_sigma")


class _IrbppStreamNoise(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_hv", "b_hv", "w_zv", "b_zv", "w_ha", "b_ha", "w_za", "b_za")]


class _IrbppStreamGrads(C.Structure):
    _fields_ = [(f"{layer}_{p}", C.c_void_p) for layer in ("hv", "zv", "ha", "za") for p in _NOISY_PARAMS]


def _streams_grad_stream_np(x, w_h, b_h, w_z, g):
    """One stream of the definition's backward on float32 numpy arrays, per row: x [..., E], g [..., A] ->
    (h = relu(pre-activation) [..., H], d [..., H], dx [..., E]), every chain ascending from its start."""
    import numpy as np
    f32 = np.float32
    p = _lin_np(w_h, b_h, x)
    on = p > 0
    e = np.zeros(p.shape, f32)
    for t in range(w_z.shape[0]):
        e = _fmaf_np(g[..., t:t + 1], w_z[t], e)
    d = np.where(on, e, f32(0)).astype(f32)
    dx = np.zeros(x.shape, f32)
    for j in range(w_h.shape[0]):
        dx = _fmaf_np(d[..., j:j + 1], w_h[j], dx)
    return np.where(on, p, f32(0)).astype(f32), d, dx


def _streams_grad_backward_np(x, xg, w, eps, ga, gv):
    """The definition of csrc/irbpp_streams_grad.hip on float32 numpy arrays: x [B, S, E], xg [B, E], w the eight effective
    arrays in StreamWeights' order (w_hv, b_hv, w_zv, b_zv, w_ha, b_ha, w_za, b_za), eps the eight epsilon arrays in the same
    order or None (eval mode), ga [B, S, A] or None, gv [B, A] or None -> (dx, dxg, grads): grads maps "hv_weight_mu" ...
    "za_bias_sigma" to arrays (the sigmas to None in eval mode).  A missing gradient counts as zeros."""
    import numpy as np
    f32 = np.float32
    w_hv, b_hv, w_zv, b_zv, w_ha, b_ha, w_za, b_za = w
    B, S, E = x.shape
    H, A = w_ha.shape[0], w_za.shape[0]
    d_w = {n: np.zeros(s, f32) for n, s in (("hv_w", (H, E)), ("hv_b", (H,)), ("zv_w", (A, H)), ("zv_b", (A,)), ("ha_w", (H, E)),
                                            ("ha_b", (H,)), ("za_w", (A, H)), ("za_b", (A,)))}
    dx, dxg = np.zeros((B, S, E), f32), np.zeros((B, E), f32)
    with np.errstate(all="ignore"):
        if ga is not None:
            ha, d, dx = _streams_grad_stream_np(x, w_ha, b_ha, w_za, ga)
            p_za, p_ha = np.zeros((B, A, H), f32), np.zeros((B, H, E), f32)
            pb_za, pb_ha = np.zeros((B, A), f32), np.zeros((B, H), f32)
            for s in range(S):                               # per sample, s ascending
                p_za = _fmaf_np(ga[:, s, :, None], ha[:, s, None, :], p_za)
                p_ha = _fmaf_np(d[:, s, :, None], x[:, s, None, :], p_ha)
                pb_za, pb_ha = pb_za + ga[:, s], pb_ha + d[:, s]
            for b in range(B):                               # plain adds, b ascending
                d_w["za_w"], d_w["ha_w"] = d_w["za_w"] + p_za[b], d_w["ha_w"] + p_ha[b]
                d_w["za_b"], d_w["ha_b"] = d_w["za_b"] + pb_za[b], d_w["ha_b"] + pb_ha[b]
        if gv is not None:
            hv, dv, dxg = _streams_grad_stream_np(xg, w_hv, b_hv, w_zv, gv)
            for b in range(B):                               # one chain over b
                d_w["zv_w"] = _fmaf_np(gv[b][:, None], hv[b][None, :], d_w["zv_w"])
                d_w["hv_w"] = _fmaf_np(dv[b][:, None], xg[b][None, :], d_w["hv_w"])
                d_w["zv_b"], d_w["hv_b"] = d_w["zv_b"] + gv[b], d_w["hv_b"] + dv[b]
        grads = {}
        for i, layer in enumerate(("hv", "zv", "ha", "za")):
            dw, db = d_w[layer + "_w"], d_w[layer + "_b"]
            grads[layer + "_weight_mu"], grads[layer + "_bias_mu"] = dw, db
            grads[layer + "_weight_sigma"] = None if eps is None else (dw * eps[2 * i]).astype(f32)
            grads[layer + "_bias_sigma"] = None if eps is None else (db * eps[2 * i + 1]).astype(f32)
    return dx, dxg, grads


def _streams_grad_workspace(lib, w: StreamWeights, S: int, B: int, dev) -> torch.Tensor:
    n = int(lib.irbpp_streams_backward_workspace(w.embed, w.hidden, w.atoms, S, B))
    if n <= 0:
        raise ValueError("streams_logits_grad: 1 <= embed, hidden <= 256, 2 <= atoms <= 128, 1 <= S <= 1024 and 1 <= B <= 1024")
    return torch.empty((n // 4,), dtype=torch.float32, device=dev)


class _StreamsLogitsGrad(torch.autograd.Function):
    """streams_logits over the four layers' live parameters with the defined backward: the numpy definition on CPU tensors,
    irbpp_streams_act(_mfma) and irbpp_streams_backward on a HIP device.  The sixteen parameters follow x and xg, layer by
    layer (fc_h_v, fc_z_v, fc_h_a, fc_z_a), each as weight_mu, weight_sigma, bias_mu, bias_sigma; then the eight epsilon buffers,
    layer by layer as weight_epsilon, bias_epsilon.  All twenty-six are saved for the backward, in either mode, so that autograd
    refuses a backward after any of them was written in place; ``pinned`` holds the call's own effective weights and the
    caller's x and x_global to the same rule."""

    @staticmethod
    def forward(ctx, x, xg, *rest):
        weights, lib, form, pinned = rest[24:]
        ctx.weights, ctx.lib, ctx.pinned = weights, lib, pinned
        if lib is None:
            v, a = _streams_logits_cpu(x, xg, weights)
        else:
            _, v, a = _streams_call(lib, x, xg, weights, None, None, None, False, True, form)
        ctx.save_for_backward(x, xg, *rest[:24])
        return v, a

    @staticmethod
    def backward(ctx, gv, ga):
        saved = ctx.saved_tensors                            # raises if one of them was written in place since the forward
        _check_pinned(ctx.pinned, "streams_logits_grad")
        x, xg = saved[:2]
        w, lib = ctx.weights, ctx.lib
        B, S, _ = x.shape
        need = ctx.needs_input_grad
        names = [f"{layer}_{p}" for layer in ("hv", "zv", "ha", "za") for p in _NOISY_PARAMS]
        eps = [_f32(t.detach(), x.device) for t in saved[18:]] if w.training else None      # unchanged since the forward
        eff = (w.w_hv, w.b_hv, w.w_zv, w.b_zv, w.w_ha, w.b_ha, w.w_za, w.b_za)
        if lib is None:
            import numpy as np
            n = lambda t: None if t is None else t.detach().to(torch.float32).contiguous().numpy()    # noqa: E731
            dx, dxg, grads = _streams_grad_backward_np(n(x), n(xg), [n(t) for t in eff], None if eps is None else [n(t) for t in eps],
                                                       n(ga), n(gv))
            t = lambda arr: None if arr is None else torch.from_numpy(np.ascontiguousarray(arr))       # noqa: E731
            out = [t(dx) if need[0] else None, t(dxg) if need[1] else None]
            out += [t(grads[nm]) if need[2 + i] else None for i, nm in enumerate(names)]
            return tuple(out) + (None,) * 12
        from . import _lib
        dev = x.device
        gv = None if gv is None else gv.detach().to(torch.float32).contiguous()
        ga = None if ga is None else ga.detach().to(torch.float32).contiguous()
        dx = torch.empty((B, S, w.embed), dtype=torch.float32, device=dev) if need[0] else None
        dxg = torch.empty((B, w.embed), dtype=torch.float32, device=dev) if need[1] else None
        shapes = {"weight": {"hv": (w.hidden, w.embed), "zv": (w.atoms, w.hidden), "ha": (w.hidden, w.embed), "za": (w.atoms, w.hidden)},
                  "bias": {"hv": (w.hidden,), "zv": (w.atoms,), "ha": (w.hidden,), "za": (w.atoms,)}}
        outs = []
        for i, nm in enumerate(names):
            layer, kind, which = nm.split("_")
            want = need[2 + i] and (which == "mu" or eps is not None)
            outs.append(torch.empty(shapes[kind][layer], dtype=torch.float32, device=dev) if want else None)
        ws = _streams_grad_workspace(lib, w, S, B, dev)
        noise = _IrbppStreamNoise(*(t.data_ptr() for t in eps)) if eps is not None else None
        grads = _IrbppStreamGrads(*(0 if t is None else t.data_ptr() for t in outs))
        wst = w._struct()
        _lib.check(lib.irbpp_streams_backward(C.byref(wst), C.byref(noise) if noise is not None else None, _p(xg), xg.stride(0), _p(x),
                                              x.stride(0), x.stride(1), _p(ga), _p(gv), S, B, _p(ws), _p(dx), _p(dxg), C.byref(grads),
                                              _stream(dev)), "irbpp_streams_backward")
        return (dx, dxg) + tuple(outs) + (None,) * 12


def streams_logits_grad(x: torch.Tensor, x_global: torch.Tensor, fc_h_v, fc_z_v, fc_h_a, fc_z_a, *,
                        training: Optional[bool] = None, use_hip: Optional[bool] = None,
                        form: str = "chain") -> Tuple[torch.Tensor, torch.Tensor]:
    """The value and advantage streams in the forward that carries a gradient (Agent.learn's online forward, model.py:393-394)
    over the four NoisyLinear layers' live parameters -> (v float32 [B, atoms], a float32 [B, S, atoms]) with a ``grad_fn``:
    the logits ``DQNBPP.forward`` combines, in place of ``fc_z_v(relu(fc_h_v(xGlobal)))`` and ``fc_z_a(relu(fc_h_a(x)))``.
    ``training=None`` follows ``fc_h_v.training`` where the layer has one, else True: the effective weights are
    ``mu + sigma * epsilon`` in training mode and ``mu`` in eval mode, in which the sigmas get no gradient.  Nothing is kept
    between calls: every call reads the parameters and the noise as they are, into effective weights of its own.  Until its
    backward has run, x, x_global, the sixteen parameters and the eight epsilon buffers must stay as they are: an in-place
    write to any of them (``reset_noise()``, an optimiser step, a copy from another network) makes the backward raise
    autograd's "modified by an inplace operation" RuntimeError, in either mode, instead of returning another gradient.

    Forms: on CPU tensors the numpy emulation of the definition, the forward's (streams_logits') and the backward's
    (csrc/irbpp_streams_grad.hip); on a HIP device with ``use_hip=True`` (``None`` takes STREAMS_GRAD_HIP_DEFAULT) the forward
    is irbpp_noisy_weights and irbpp_streams_act (``form="mfma"``: irbpp_streams_act_mfma, the same bits) and the backward
    irbpp_streams_backward: ordered fmaf chains without atomics, so x's, x_global's and the sixteen parameters' gradients are
    the same bits on every run and equal to the CPU form's; else torch's ``F.linear`` / ``relu`` on ``mu + sigma * epsilon``
    under ordinary autograd.  The kernels take 1 <= B <= 1024 besides streams_logits' limits (ValueError otherwise); a
    detached ``x`` skips its gradient's launch work."""
    if training is None:
        training = bool(getattr(fc_h_v, "training", True))
    layers = (fc_h_v, fc_z_v, fc_h_a, fc_z_a)
    lib = _head_lib(x, use_hip, STREAMS_GRAD_HIP_DEFAULT)
    if lib is None and x.is_cuda:
        F = torch.nn.functional
        eff = [(l.weight_mu + l.weight_sigma * l.weight_epsilon, l.bias_mu + l.bias_sigma * l.bias_epsilon) if training else
               (l.weight_mu, l.bias_mu) for l in layers]
        if x_global.dim() == 3 and x_global.shape[1] == 1:
            x_global = x_global[:, 0]
        return (F.linear(F.relu(F.linear(x_global, *eff[0])), *eff[1]), F.linear(F.relu(F.linear(x, *eff[2])), *eff[3]))
    weights = StreamWeights(*layers, training=training)
    if weights.device != x.device:
        raise ValueError("streams_logits_grad: the layers and x live on different devices")
    xs, xg = _streams_inputs(x, x_global, weights)
    if xs.shape[0] > STREAMS_GRAD_MAX_BATCH:
        raise ValueError("streams_logits_grad: 1 <= B <= 1024")
    if lib is not None:
        form = _streams_form(form, weights)
    # The backward reads x, x_global and the epsilon buffers where they lie (no copy is taken) and this call's own effective
    # weights (``weights``: built above, private to the call, so a later forward cannot overwrite them).  Everything the caller
    # handed over goes to save_for_backward, and ``pinned`` covers what that cannot reach: a reset_noise(), an optimiser step
    # or a target copy into any of them before the backward raises there instead of changing the gradient.
    params = [getattr(layer, n) for layer in layers for n in _NOISY_PARAMS]
    noise = [getattr(layer, n) for layer in layers for n in ("weight_epsilon", "bias_epsilon")]
    w = weights
    pinned = _pinned(x, x_global, w.w_hv, w.b_hv, w.w_zv, w.b_zv, w.w_ha, w.b_ha, w.w_za, w.b_za)
    return _StreamsLogitsGrad.apply(xs, xg, *params, *noise, weights, lib, form, pinned)


# The same question for the shape branch in front of the network ("The shape branch"): the
# de-duplicated torch formulation or the two launches of irbpp_shape_features.  The kernels: tools/shape_feature_rates.py
# measured them on an MI355X at 0.073 ms against 0.446 ms for torch's layers on the unique ids at 4096 rows of 8 shapes, 0.189
# against 0.515 ms with 100 shapes, and 0.061 / 0.164 against 0.323 / 0.373 ms at 1024 rows: beyond the larger spread at every
# acting size (profiles/shape_features/).  use_hip=False asks for torch's layers.
SHAPE_FEATURES_HIP_DEFAULT = True

SHAPE_MAX_WIDTH, SHAPE_MAX_POINTS, SHAPE_MAX_SHAPES = 256, 4096, 65535


class _IrbppShapeEncoder(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w1", "b1", "w2", "b2")] + [("hidden", C.c_int32), ("feat", C.c_int32), ("slope", C.c_float)]


class ShapePoints(object):
    """The reference's ``args.shapeArray`` (float [n_shapes, P, 3], numpy or a tensor: P surface points per shape) as one float32
    table on ``device``, uploaded once: the shape branch then never leaves the device (model.py:328-335 indexes the CPU array
    with ``next_item_ID.cpu()`` and copies the gathered points back on every forward).  ``updateShapeArray``'s periodic
    re-subsampling is the caller's business: build a new ShapePoints."""

    def __init__(self, shape_array, device):
        t = torch.as_tensor(shape_array)
        if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("shape_array must be [n_shapes, P, 3]")
        self.points = t.detach().to(device=device, dtype=torch.float32).contiguous()
        if self.points.data_ptr() == t.data_ptr():           # a float32 array on the CPU: a table of its own, once, since a write
            self.points = self.points.clone()                # to the caller's array would pass every version check
        self.device = self.points.device
        self.n_shapes, self.n_points = int(t.shape[0]), int(t.shape[1])
        self._workspace = {}

    def draw_indices(self, k: int, generator=None) -> torch.Tensor:
        """int32 [k] on the device, uniform in [0, P) with replacement: the role of model.py's ``np.random.randint`` (not its
        global stream: a caller who needs the reference's draws passes its own indices)."""
        return torch.randint(0, self.n_points, (int(k),), device=self.device, generator=generator, dtype=torch.int32)

    def gather(self, ids: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
        """``shapeArray[ids][:, indices]`` -> float32 [M, k, 3] by torch indexing on the device: what the forward that carries
        a gradient feeds to ``self.shapeEncoder``."""
        ids = ids.reshape(-1).to(device=self.device, dtype=torch.long)
        return self.points[ids[:, None], indices.to(device=self.device, dtype=torch.long)[None, :]]

    def _partial(self, chunks: int, feat: int) -> torch.Tensor:
        key = (chunks, feat)
        if key not in self._workspace:
            self._workspace[key] = torch.empty((self.n_shapes, chunks, feat), dtype=torch.float32, device=self.device)
        return self._workspace[key]

    def _partial_arg(self, chunks: int, feat: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """irbpp_shape_features_arg's two workspaces: the chunks' keys and positions, int32 [n_shapes, chunks, feat] each."""
        key = ("arg", chunks, feat)
        if key not in self._workspace:
            self._workspace[key] = tuple(torch.empty((self.n_shapes, chunks, feat), dtype=torch.int32, device=self.device) for _ in range(2))
        return self._workspace[key]

    def _grad_workspace(self, hidden: int, feat: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """irbpp_shape_features_backward's two workspaces: float32 [n_shapes, feat, 4] and [n_shapes, hidden, 4]."""
        key = ("grad", hidden, feat)
        if key not in self._workspace:
            self._workspace[key] = tuple(torch.empty((self.n_shapes, n, 4), dtype=torch.float32, device=self.device) for n in (feat, hidden))
        return self._workspace[key]


class ShapeEncoderWeights(object):
    """``shapeEncoder``'s two Linear layers as float32 contiguous tensors (w1 [H1, 3], b1 [H1], w2 [F, H1], b2 [F]) and the
    LeakyReLU's slope: what shape_features multiplies by.  Copies: call ``refresh()`` after every optimiser step."""

    def __init__(self, linear1, linear2, negative_slope: float = 0.01):
        self.layers = (linear1, linear2)
        self.slope = float(negative_slope)
        self.hidden, three = (int(d) for d in linear1.weight.shape)
        self.feat = int(linear2.weight.shape[0])
        if three != 3 or tuple(linear2.weight.shape) != (self.feat, self.hidden) or tuple(linear1.bias.shape) != (self.hidden,) or \
                tuple(linear2.bias.shape) != (self.feat,):
            raise ValueError("shape encoder: Linear(3, H1) and Linear(H1, F) with biases")
        if not (1 <= self.hidden <= SHAPE_MAX_WIDTH and 1 <= self.feat <= SHAPE_MAX_WIDTH and self.slope >= 0):
            raise ValueError("shape encoder: 1 <= H1, F <= 256 and negative_slope >= 0")
        self.device = linear1.weight.device
        self.refresh()

    @classmethod
    def from_layers(cls, linear1, linear2, negative_slope: float = 0.01) -> "ShapeEncoderWeights":
        return cls(linear1, linear2, negative_slope)

    @torch.no_grad()
    def refresh(self) -> "ShapeEncoderWeights":
        l1, l2 = self.layers
        self.w1, self.b1, self.w2, self.b2 = (_f32(t.detach(), self.device).clone() for t in (l1.weight, l1.bias, l2.weight, l2.bias))
        return self

    def _struct(self) -> _IrbppShapeEncoder:
        return _IrbppShapeEncoder(self.w1.data_ptr(), self.b1.data_ptr(), self.w2.data_ptr(), self.b2.data_ptr(), self.hidden,
                                  self.feat, self.slope)


def _max_sticky_np(h):
    """max over axis 0 of a float32 array as the kernels take it: on keys (the bits mapped to uint32 in the floats' order, -0
    below +0, every NaN on top), so any NaN gives the quiet NaN 0x7fc00000."""
    import numpy as np
    b = np.ascontiguousarray(h, dtype=np.float32).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    key = np.where((b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000), np.uint32(0xffffffff), key).max(axis=0)
    bits = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7fffffff), ~key)
    return np.where(key == np.uint32(0xffffffff), np.uint32(0x7fc00000), bits).astype(np.uint32).view(np.float32)


def _shape_ids(ids: torch.Tensor, n_shapes: int) -> torch.Tensor:
    """ids (float: truncated toward zero like .long(); NaN and infinities are bad) -> int64 with -1 for every bad id."""
    if ids.is_floating_point():
        v = ids.to(torch.float32)
        ok = (v > -1) & (v < n_shapes)
        return torch.where(ok, torch.where(ok, v, torch.zeros_like(v)).long(), torch.full_like(v, -1, dtype=torch.long))
    v = ids.long()
    return torch.where((v >= 0) & (v < n_shapes), v, torch.full_like(v, -1))


def _shape_features_cpu(ids: torch.Tensor, points: ShapePoints, indices: torch.Tensor, w: ShapeEncoderWeights) -> torch.Tensor:
    import numpy as np
    f32 = np.float32
    n = lambda t: t.detach().to(torch.float32).cpu().numpy()  # noqa: E731
    leaky = lambda s: np.where(s > 0, s, f32(w.slope) * s).astype(f32)  # noqa: E731
    u = _shape_ids(ids, points.n_shapes).numpy()
    idx = indices.detach().cpu().numpy().astype(np.int64)
    bad = (idx < 0) | (idx >= points.n_points)
    out = np.full((u.shape[0], w.feat), np.nan, dtype=f32)
    table = n(points.points)
    with np.errstate(all="ignore"):
        for s in np.unique(u[u >= 0]):
            p = table[s][np.where(bad, 0, idx)].copy()
            p[bad] = np.nan
            h2 = leaky(_lin_np(n(w.w2), n(w.b2), leaky(_lin_np(n(w.w1), n(w.b1), p))))
            out[u == s] = _max_sticky_np(h2)
    return torch.from_numpy(out)


def _shape_features_torch(ids, points: ShapePoints, indices, w: ShapeEncoderWeights) -> torch.Tensor:
    F = torch.nn.functional
    u = _shape_ids(ids, points.n_shapes)
    idx = indices.long()
    bad_idx = ((idx < 0) | (idx >= points.n_points)).any()
    uniq, inv = torch.unique(u.clamp(min=0), return_inverse=True)
    p = points.points[uniq[:, None], idx.clamp(0, points.n_points - 1)[None, :]]
    h = F.leaky_relu(F.linear(F.leaky_relu(F.linear(p, w.w1, w.b1), w.slope), w.w2, w.b2), w.slope)
    feat = torch.max(h, dim=1)[0][inv]
    return torch.where((u < 0)[:, None] | bad_idx, torch.full_like(feat, float("nan")), feat)


@torch.no_grad()
def shape_features(ids: torch.Tensor, points: ShapePoints, indices: torch.Tensor, weights: ShapeEncoderWeights, *,
                   use_hip: Optional[bool] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The shape branch of DQNBPP.forward without a gradient (model.py:328-335, :365-372): the observation's item ids ->
    ``shape_feature`` float32 [M, F], on ``points``' device.  ``ids``: any shape (flattened: [B, K] gives [B*K, F]), integers or
    the observation's float32 column itself (truncated toward zero like ``.long()``), strided columns as they are;
    ``indices``: the forward's one index set, int [k] (``points.draw_indices``); ``out``: a float32 [M, F] tensor with
    contiguous rows (a slice of a wider tensor passes) to write into.  Defined arithmetic (csrc/irbpp_shapefeat.hip: fmaf chains
    from the bias, a max with a sticky NaN); an id outside [0, n_shapes) gives a NaN row, an index outside [0, P) makes every
    row NaN.  The feature is computed once per distinct id in every form: on CPU tensors the exact numpy emulation of the
    definition, on a HIP device with ``use_hip=True`` (``None`` takes SHAPE_FEATURES_HIP_DEFAULT) the two launches of
    irbpp_shape_features, else torch's layers on the unique ids (rocBLAS's summation order: close to, not bit-equal with, the
    definition)."""
    dev = points.device
    ids = ids.detach()
    if ids.device != dev:
        ids = ids.to(dev)
    if ids.is_floating_point():
        ids = ids if ids.dtype == torch.float32 else ids.to(torch.float32)
    elif ids.dtype != torch.int64:
        ids = ids.long()
    ids = ids.reshape(-1)                                # a view where the strides allow it (a column of the observation)
    indices = indices.detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    M, k, F_ = int(ids.shape[0]), int(indices.shape[0]), weights.feat
    if not (1 <= k <= SHAPE_MAX_POINTS) or M < 1 or points.n_shapes > SHAPE_MAX_SHAPES:
        raise ValueError("shape_features: indices int [k] with 1 <= k <= 4096, at least one id, at most 65535 shapes")
    if weights.device != dev:
        raise ValueError("shape_features: the weights and the points live on different devices")
    if out is not None and (out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (M, F_) or
                            (F_ > 1 and out.stride(1) != 1) or out.stride(0) < F_):
        raise ValueError(f"out must be a float32 [{M}, {F_}] tensor on the points' device with contiguous rows")
    lib = _head_lib(points.points, use_hip, SHAPE_FEATURES_HIP_DEFAULT)
    if lib is None:
        res = _shape_features_torch(ids, points, indices, weights) if dev.type == "cuda" else \
            _shape_features_cpu(ids, points, indices, weights)
        if out is None:
            return res
        out.copy_(res)
        return out
    from . import _lib
    if out is None:
        out = torch.empty((M, F_), dtype=torch.float32, device=dev)
    if M > 1 and ids.stride(0) < 1:
        ids = ids.contiguous()
    chunks = lib.irbpp_shape_features_chunks(points.n_shapes, k)
    enc = weights._struct()
    _lib.check(lib.irbpp_shape_features(_p(points.points), points.n_shapes, points.n_points, _p(indices), k, _p(ids),
                                        1 if ids.is_floating_point() else 0, max(int(ids.stride(0)), 1), M, C.byref(enc),
                                        _p(points._partial(chunks, F_)), chunks, _p(out), max(int(out.stride(0)), F_),
                                        _stream(dev)), "irbpp_shape_features")
    return out


# The shape branch in the forward that carries a gradient ("The shape branch with a gradient"): the
# parent's path (ShapePoints.gather into torch's layers, per row), torch's layers on the unique ids, or the four launches of
# irbpp_shape_features_arg / irbpp_shape_features_backward.  The kernels: tools/shape_grad_rates.py measured forward plus
# backward on an MI355X at 0.27 ms against 1.01 ms for torch on the unique ids and 4.14 ms for the parent's path at 640 rows of
# the 64 BlockOut shapes, 0.43 against 1.80 and 4.15 ms with 200 shapes, and 0.27 / 0.22 against 0.79 / 0.77 and 0.68 / 0.67 ms
# at 64 rows: beyond the larger spread at every measured size (profiles/shape_grad/).  use_hip=False asks for torch's layers.
SHAPE_GRAD_HIP_DEFAULT = True


def _shape_points_np(table, s: int, idx):
    """table[s][idx] as float32 [len(idx), 3], a NaN point for every index outside the table."""
    import numpy as np
    bad = (idx < 0) | (idx >= table.shape[1])
    p = table[s][np.where(bad, 0, idx)].astype(np.float32)
    p[bad] = np.nan
    return p


def _shape_key_np(h):
    import numpy as np
    b = np.ascontiguousarray(h, dtype=np.float32).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where((b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000), np.uint32(0xffffffff), key)


def _shape_grad_forward_np(table, idx, u, w1, b1, w2, b2, slope: float):
    """The definition of csrc/irbpp_shapefeat_grad.hip's forward on numpy arrays: table float32 [n_shapes, P, 3], idx int64
    [k], u int64 [M] with -1 for a bad id -> (out float32 [M, F], the bits of _shape_features_cpu; arg int32 [n_shapes, F])."""
    import numpy as np
    f32 = np.float32
    leaky = lambda s: np.where(s > 0, s, f32(slope) * s).astype(f32)  # noqa: E731
    out = np.full((u.shape[0], w2.shape[0]), np.nan, dtype=f32)
    arg = np.full((table.shape[0], w2.shape[0]), -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        for s in np.unique(u[u >= 0]):
            s2 = _lin_np(w2, b2, leaky(_lin_np(w1, b1, _shape_points_np(table, s, idx))))
            out[u == s] = _max_sticky_np(leaky(s2))
            arg[s] = np.argmax(_shape_key_np(s2), axis=0)          # the first position of the largest key
    return out, arg


def _shape_grad_backward_np(table, idx, u, w1, b1, w2, b2, slope: float, arg, g):
    """The definition's backward: g float32 [M, F] -> (dW1 [H1, 3], db1 [H1], dW2 [F, H1], db2 [F]), every chain in its order."""
    import numpy as np
    f32 = np.float32
    sl = f32(slope)
    H1, F_ = w1.shape[0], w2.shape[0]
    G = np.zeros((table.shape[0], F_), dtype=f32)
    d_w1, d_b1, d_w2, d_b2 = np.zeros((H1, 3), f32), np.zeros(H1, f32), np.zeros((F_, H1), f32), np.zeros(F_, f32)
    with np.errstate(all="ignore"):
        for m in range(u.shape[0]):                          # m ascending; a bad id's row adds nothing
            if u[m] >= 0:
                G[u[m]] = G[u[m]] + g[m]
        for s in np.unique(u[u >= 0]):                       # u ascending
            j = arg[s].astype(np.int64)
            p = _shape_points_np(table, s, np.where((j >= 0) & (j < idx.shape[0]), idx[np.clip(j, 0, idx.shape[0] - 1)], -1))   # [F, 3]
            s1 = _lin_np(w1, b1, p)                          # [F, H1]
            h1 = np.where(s1 > 0, s1, sl * s1).astype(f32)
            s2 = b2.astype(f32)
            for i in range(H1):
                s2 = _fmaf_np(h1[:, i], w2[:, i], s2)
            d2 = np.where(s2 > 0, G[s], sl * G[s]).astype(f32)
            d_b2 = d_b2 + d2
            d_w2 = _fmaf_np(d2[:, None], h1, d_w2)
            e = d2[:, None] * w2
            ds1 = np.where(s1 > 0, e, sl * e).astype(f32)
            first, first_b = np.zeros((H1, 3), f32), np.zeros(H1, f32)
            for f in range(F_):                              # f ascending
                first = _fmaf_np(ds1[f][:, None], p[f][None, :], first)
                first_b = first_b + ds1[f]
            d_w1, d_b1 = d_w1 + first, d_b1 + first_b
    return d_w1, d_b1, d_w2, d_b2


class _ShapeFeaturesGrad(torch.autograd.Function):
    """shape_features with the arg record kept for a backward that reaches the encoder's four arrays: the numpy definition on
    CPU tensors, irbpp_shape_features_arg / irbpp_shape_features_backward on a HIP device."""

    @staticmethod
    def forward(ctx, w1, b1, w2, b2, ids, indices, points, slope, lib, pinned):
        dev = points.device
        M, k, H1, F_ = int(ids.shape[0]), int(indices.shape[0]), int(w1.shape[0]), int(w2.shape[0])
        ctx.points, ctx.slope, ctx.lib, ctx.pinned = points, slope, lib, pinned
        if lib is None:
            import numpy as np
            n = lambda t: t.detach().cpu().numpy()           # noqa: E731
            out, arg = _shape_grad_forward_np(n(points.points), n(indices).astype(np.int64), _shape_ids(ids, points.n_shapes).numpy(),
                                              n(w1), n(b1), n(w2), n(b2), slope)
            out, arg = torch.from_numpy(out), torch.from_numpy(arg)
        else:
            from . import _lib
            out = torch.empty((M, F_), dtype=torch.float32, device=dev)
            arg = torch.empty((points.n_shapes, F_), dtype=torch.int32, device=dev)
            chunks = lib.irbpp_shape_features_chunks(points.n_shapes, k)
            key_ws, j_ws = points._partial_arg(chunks, F_)
            enc = _IrbppShapeEncoder(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), H1, F_, slope)
            _lib.check(lib.irbpp_shape_features_arg(_p(points.points), points.n_shapes, points.n_points, _p(indices), k, _p(ids),
                                                    1 if ids.is_floating_point() else 0, max(int(ids.stride(0)), 1), M, C.byref(enc),
                                                    _p(key_ws), _p(j_ws), chunks, _p(out), F_, _p(arg), _stream(dev)),
                       "irbpp_shape_features_arg")
        ctx.save_for_backward(w1, b1, w2, b2, ids, indices, arg, points.points)     # the table as this forward read it
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        w1, b1, w2, b2, ids, indices, arg, table = ctx.saved_tensors     # raises if one was written in place since the forward
        _check_pinned(ctx.pinned, "shape_features_grad")       # the caller's own tensors, where the ones above are converted copies
        points, slope, lib = ctx.points, ctx.slope, ctx.lib
        g = grad_out.detach().to(torch.float32).contiguous()
        if lib is None:
            import numpy as np
            n = lambda t: t.detach().cpu().numpy()           # noqa: E731
            grads = _shape_grad_backward_np(n(table), n(indices).astype(np.int64), _shape_ids(ids, points.n_shapes).numpy(),
                                            n(w1), n(b1), n(w2), n(b2), slope, n(arg), n(g))
            grads = tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in grads)
        else:
            from . import _lib
            dev = points.device
            H1, F_ = int(w1.shape[0]), int(w2.shape[0])
            grads = tuple(torch.empty_like(t) for t in (w1, b1, w2, b2))
            pd_ws, first_ws = points._grad_workspace(H1, F_)
            enc = _IrbppShapeEncoder(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), H1, F_, slope)
            _lib.check(lib.irbpp_shape_features_backward(_p(table), points.n_shapes, points.n_points, _p(indices),
                                                         int(indices.shape[0]), _p(ids), 1 if ids.is_floating_point() else 0,
                                                         max(int(ids.stride(0)), 1), int(ids.shape[0]), C.byref(enc), _p(arg), _p(g),
                                                         _p(pd_ws), _p(first_ws), *(_p(t) for t in grads), _stream(dev)),
                       "irbpp_shape_features_backward")
        return grads + (None,) * 6


def _shape_features_grad_torch(ids, points: ShapePoints, indices, w1, b1, w2, b2, slope: float) -> torch.Tensor:
    """torch's layers on the unique ids, with autograd (the bad ids' rows and a bad index as in _shape_features_torch)."""
    F = torch.nn.functional
    u = _shape_ids(ids, points.n_shapes)
    idx = indices.long()
    bad_idx = ((idx < 0) | (idx >= points.n_points)).any()
    uniq, inv = torch.unique(u.clamp(min=0), return_inverse=True)
    p = points.points[uniq[:, None], idx.clamp(0, points.n_points - 1)[None, :]]
    h = F.leaky_relu(F.linear(F.leaky_relu(F.linear(p, w1, b1), slope), w2, b2), slope)
    feat = torch.max(h, dim=1)[0][inv]
    return torch.where((u < 0)[:, None] | bad_idx, torch.full_like(feat, float("nan")), feat)


def shape_features_grad(ids: torch.Tensor, points: ShapePoints, indices: torch.Tensor, linear1, linear2,
                        negative_slope: float = 0.01, *, use_hip: Optional[bool] = None, return_arg: bool = False):
    """The shape branch of the forward that carries a gradient (Agent.learn's online forward, model.py:328-335, :365-372):
    ``shape_features`` over the live parameters of ``shapeEncoder``'s two Linear layers -> ``shape_feature`` float32 [M, F]
    with a ``grad_fn``, in place of ``torch.max(shapeEncoder(points.gather(ids, indices)), dim=1)[0]``.  ``ids`` and
    ``indices`` as shape_features takes them.  The feature is computed once per distinct id and the max routes each feature's
    gradient to one point, so the backward costs (distinct ids) x F x H1 fused multiply-adds and keeps no activation block.

    Forms: on CPU tensors the numpy emulation of the definition (csrc/irbpp_shapefeat_grad.hip), forward and backward; on a
    HIP device with ``use_hip=True`` (``None`` takes SHAPE_GRAD_HIP_DEFAULT) irbpp_shape_features_arg and, in the backward,
    irbpp_shape_features_backward: the forward's bits are shape_features', the four gradients are reproducible bit for bit
    (ordered chains, no atomics) and equal to the CPU form's; else torch's layers on the unique ids with torch's autograd.
    The points and the ids carry no gradient.  The backward reads the four parameters, ``ids``, ``indices`` and the points'
    table where they lie: an in-place write to any of them before it makes it raise autograd's "modified by an inplace
    operation" RuntimeError.  ``return_arg=True`` returns ``(shape_feature, arg)``, arg int32 [n_shapes, F]:
    the position in ``indices`` of each feature's maximum per shape that occurs (the smallest one among ties), -1 elsewhere;
    the torch form keeps no such record and raises."""
    dev = points.device
    slope = float(negative_slope)
    w1, b1, w2, b2 = linear1.weight, linear1.bias, linear2.weight, linear2.bias
    H1, F_ = int(w1.shape[0]), int(w2.shape[0])
    if tuple(w1.shape) != (H1, 3) or tuple(w2.shape) != (F_, H1) or tuple(b1.shape) != (H1,) or tuple(b2.shape) != (F_,):
        raise ValueError("shape encoder: Linear(3, H1) and Linear(H1, F) with biases")
    if not (1 <= H1 <= SHAPE_MAX_WIDTH and 1 <= F_ <= SHAPE_MAX_WIDTH and slope >= 0):
        raise ValueError("shape encoder: 1 <= H1, F <= 256 and negative_slope >= 0")
    if any(t.device != dev for t in (w1, b1, w2, b2)):
        raise ValueError("shape_features_grad: the layers and the points live on different devices")
    given_ids, given_indices = ids, indices
    ids = ids.detach()
    if ids.device != dev:
        ids = ids.to(dev)
    if ids.is_floating_point():
        ids = ids if ids.dtype == torch.float32 else ids.to(torch.float32)
    elif ids.dtype != torch.int64:
        ids = ids.long()
    ids = ids.reshape(-1)
    indices = indices.detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    M, k = int(ids.shape[0]), int(indices.shape[0])
    if not (1 <= k <= SHAPE_MAX_POINTS) or M < 1 or points.n_shapes > SHAPE_MAX_SHAPES:
        raise ValueError("shape_features_grad: indices int [k] with 1 <= k <= 4096, at least one id, at most 65535 shapes")
    lib = _head_lib(points.points, use_hip, SHAPE_GRAD_HIP_DEFAULT)
    if lib is None and dev.type == "cuda":
        if return_arg:
            raise ValueError("shape_features_grad: torch's layers keep no arg record")
        return _shape_features_grad_torch(ids, points, indices, w1, b1, w2, b2, slope)
    if lib is not None and M > 1 and ids.stride(0) < 1:
        ids = ids.contiguous()
    live = tuple(t.to(torch.float32).contiguous() for t in (w1, b1, w2, b2))     # the parameters themselves where they are both
    out, arg = _ShapeFeaturesGrad.apply(*live, ids, indices, points, slope, lib, _pinned(w1, b1, w2, b2, given_ids, given_indices))
    return (out, arg) if return_arg else out


# The same question for the embedding stage between the two ("The embedding stage"): torch's layers in
# the factored form (MIOpen's convolutions, rocBLAS for the project layers) or the two launches of irbpp_embed.  Torch's
# layers, since tools/embed_rates.py measured them on an MI355X at 5.38 ms against 11.14 ms for the kernels at 4096 bins x 500
# candidates and 1.43 against 2.84 ms at 1024 (profiles/embed/): the matrix units win over the defined fmaf chain, as for the
# streams.  use_hip=True asks for the kernels (the reproducible forward).
EMBED_HIP_DEFAULT = False

EMBED_MAX_WIDTH, EMBED_MAX_CAND_HIDDEN, EMBED_MAX_ROWS = 256, 64, 1024
_EMBED_FIELDS = ("w_conv1", "b_conv1", "w_conv2", "b_conv2", "w_conv3", "b_conv3", "w_c1", "b_c1", "w_c2", "b_c2", "w_p1", "b_p1",
                 "w_p2", "b_p2")
_EMBED_SIZES = ("map_len", "c1", "c2", "c3", "feat", "cand_hidden", "cand_embed", "proj_hidden", "embed")


class _IrbppEmbedWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _EMBED_FIELDS] + [(n, C.c_int32) for n in _EMBED_SIZES] + [("slope", C.c_float)]


class _FrontWeights(object):
    """What EmbedWeights and OrderEmbedWeights share: the heightmap encoder's three Conv2d with their checks, and what follows
    from a subclass's ``_NAME`` (the prefix of its messages), ``_FIELDS`` (the tensors, in ``layers``' order, a bias after its
    weight), ``_SIZES``, ``_STRUCT`` (the C struct of the three), ``_MAX`` (the limits of the widths, ``_MAX_WIDTH`` where it
    names none) and ``_LIMITS`` (what the limits' message says after the prefix)."""
    _MAX = {}

    @staticmethod
    def _weighted(modules, dim: int) -> list:
        """The members with a weight of ``dim`` dimensions, in order: the activations between them are skipped."""
        return [m for m in modules if getattr(m, "weight", None) is not None and m.weight.dim() == dim]

    def _encoder(self, convs, negative_slope: float, map_len: int) -> None:
        """slope, map_len, c1, c2, c3 and map_feat from the three Conv2d and the heightmap's side."""
        self.slope, self.map_len = float(negative_slope), int(map_len)
        for m, (k, s, p) in zip(convs, ((4, 2, 1), (4, 2, 1), (3, 1, 1))):
            if tuple(m.weight.shape[2:]) != (k, k) or tuple(getattr(m, "stride", (s, s))) != (s, s) or \
                    tuple(getattr(m, "padding", (p, p))) != (p, p):
                raise ValueError(f"{self._NAME}: Conv2d(1, c1, 4, 2, 1), Conv2d(c1, c2, 4, 2, 1), Conv2d(c2, c3, 3, 1, 1)")
        self.c1, self.c2, self.c3 = (int(m.weight.shape[0]) for m in convs)
        if self.map_len % 4 != 0 or not 8 <= self.map_len <= 32:
            raise ValueError(f"{self._NAME}: map_len is a multiple of 4 in [8, 32]")
        self.map_feat = self.c3 * (self.map_len // 4) ** 2

    def _finish(self, want) -> None:
        """``layers`` against the shapes ``want``, the limits, and the first copy."""
        for m, shape in zip(self.layers, want):
            if tuple(m.weight.shape) != shape or (m.bias is not None and tuple(m.bias.shape) != shape[:1]):
                raise ValueError(f"{self._NAME}: a weight of shape {tuple(m.weight.shape)} beside the expected {shape}")
        if not (1 <= self.c1 <= 16 and 1 <= self.c2 <= 32 and 1 <= self.c3 <= 4 and self.slope >= 0 and
                all(1 <= getattr(self, n) <= self._MAX.get(n, self._MAX_WIDTH) for n in self._SIZES[4:])):
            raise ValueError(f"{self._NAME}: 1 <= c1 <= 16, 1 <= c2 <= 32, 1 <= c3 <= 4, {self._LIMITS} and negative_slope >= 0")
        self.device = self.layers[0].weight.device
        self._workspace = {}
        self.refresh()

    @classmethod
    def from_layers(cls, *args, **kw):
        return cls(*args, **kw)

    @torch.no_grad()
    def refresh(self):
        names = iter(self._FIELDS)
        for m in self.layers:
            setattr(self, next(names), _f32(m.weight.detach(), self.device).clone())
            if m.bias is not None:
                setattr(self, next(names), _f32(m.bias.detach(), self.device).clone())
        return self

    def _struct(self):
        return self._STRUCT(*(getattr(self, n).data_ptr() for n in self._FIELDS), *(getattr(self, n) for n in self._SIZES), self.slope)

    def _base(self, n_env: int) -> torch.Tensor:
        if n_env not in self._workspace:
            self._workspace = {n_env: torch.empty((n_env, self.proj_hidden), dtype=torch.float32, device=self.device)}
        return self._workspace[n_env]


class EmbedWeights(_FrontWeights):
    """The layers of DQNBPP's embedding stage as float32 contiguous tensors in torch's layouts: ``heightEncoder``'s three
    Conv2d (4x4 stride 2 pad 1, 4x4 stride 2 pad 1, 3x3 stride 1 pad 1), ``init_candidate_embed``'s two Linear and
    ``project_layer``'s two Linear, and the LeakyReLUs' slope: what embed multiplies by.  Takes the three ``nn.Sequential``s
    (any iterables whose Conv2d / Linear members come in order; the activations between them are skipped) and checks that the
    shapes fit each other; ``map_len`` is the heightmap's side L (the reference asserts 32), from which the shape feature's
    width follows: F = project_layer[0].in_features - c3 (L/4)^2 - cand_embed.  Copies: call ``refresh()`` after every
    optimiser step."""
    _NAME, _FIELDS, _SIZES, _STRUCT = "embed", _EMBED_FIELDS, _EMBED_SIZES, _IrbppEmbedWeights
    _MAX_WIDTH, _MAX = EMBED_MAX_WIDTH, {"cand_hidden": EMBED_MAX_CAND_HIDDEN}
    _LIMITS = "1 <= cand_hidden <= 64, 1 <= feat, cand_embed, proj_hidden, embed <= 256"

    def __init__(self, height_encoder, init_candidate_embed, project_layer, negative_slope: float = 0.01, *, map_len: int = 32):
        convs, cands, projs = self._weighted(height_encoder, 4), self._weighted(init_candidate_embed, 2), self._weighted(project_layer, 2)
        if len(convs) != 3 or len(cands) != 2 or len(projs) != 2:
            raise ValueError("embed: three Conv2d, two Linear (candidates) and two Linear (project layer)")
        self.layers = tuple(convs + cands + projs)
        if any(m.bias is None for m in self.layers):
            raise ValueError("embed: every layer has a bias")
        self._encoder(convs, negative_slope, map_len)
        self.cand_hidden, self.cand_embed = int(cands[0].weight.shape[0]), int(cands[1].weight.shape[0])
        self.proj_hidden, self.embed = int(projs[0].weight.shape[0]), int(projs[1].weight.shape[0])
        self.feat = int(projs[0].weight.shape[1]) - self.map_feat - self.cand_embed
        self._finish([(self.c1, 1, 4, 4), (self.c2, self.c1, 4, 4), (self.c3, self.c2, 3, 3), (self.cand_hidden, 4),
                      (self.cand_embed, self.cand_hidden), (self.proj_hidden, self.feat + self.map_feat + self.cand_embed),
                      (self.embed, self.proj_hidden)])


def _chain_np(acc, w, x):
    """The chains acc [..., J] continued over x [..., K] against w [J, K], k ascending: _lin_np from where another left off."""
    for k in range(w.shape[1]):
        acc = _fmaf_np(x[..., k:k + 1], w[:, k], acc)
    return acc


def _conv_np(x, w, b, stride: int, pad: int):
    """The defined convolution on float32 numpy arrays: x [N, Cin, H, H], w [Cout, Cin, k, k] -> [N, Cout, H', H'], every
    output _lin_np over its zero-padded patch in (c_in, ky, kx) order."""
    import numpy as np
    k = w.shape[2]
    n_out = (x.shape[2] + 2 * pad - k) // stride + 1
    xp = np.zeros(x.shape[:2] + (x.shape[2] + 2 * pad, x.shape[3] + 2 * pad), dtype=np.float32)
    xp[:, :, pad:pad + x.shape[2], pad:pad + x.shape[3]] = x
    span = stride * (n_out - 1) + 1
    patches = np.stack([xp[:, ci, ky:ky + span:stride, kx:kx + span:stride] for ci in range(x.shape[1]) for ky in range(k)
                        for kx in range(k)], axis=-1)
    return np.ascontiguousarray(np.moveaxis(_lin_np(w.reshape(w.shape[0], -1), b, patches), -1, 1))


def _mean_rows_np(x):
    """dueling_mean over axis 1 of a float32 [N, S, E] array: 16 interleaved parts from 0.0, added left to right, over S."""
    import numpy as np
    S = x.shape[1]
    total = None
    for g in range(16):
        s = np.zeros((x.shape[0], x.shape[2]), dtype=np.float32)
        for i in range(g, S, 16):
            s = s + x[:, i]
        total = s if total is None else total + s
    return total / np.float32(S)


def _np32(t: torch.Tensor):
    return t.detach().to(torch.float32).cpu().numpy()


def _height_map_np(hm, w, leaky):
    """The heightmap encoder in the defined arithmetic: hm float32 numpy [N, 1, L, L] -> map [N, M]."""
    a = leaky(_conv_np(hm, _np32(w.w_conv1), _np32(w.b_conv1), 2, 1))
    a = leaky(_conv_np(a, _np32(w.w_conv2), _np32(w.b_conv2), 2, 1))
    return leaky(_conv_np(a, _np32(w.w_conv3), _np32(w.b_conv3), 1, 1)).reshape(hm.shape[0], w.map_feat)


def _height_map_torch(hm: torch.Tensor, w) -> torch.Tensor:
    """The heightmap encoder as torch's layers: hm [N, 1, L, L] -> map [N, M]."""
    F = torch.nn.functional
    a = F.leaky_relu(F.conv2d(hm, w.w_conv1, w.b_conv1, stride=2, padding=1), w.slope)
    a = F.leaky_relu(F.conv2d(a, w.w_conv2, w.b_conv2, stride=2, padding=1), w.slope)
    return F.leaky_relu(F.conv2d(a, w.w_conv3, w.b_conv3, stride=1, padding=1), w.slope).reshape(hm.shape[0], -1)


def _embed_cpu(state: torch.Tensor, sf: torch.Tensor, w: EmbedWeights, S: int) -> Tuple[torch.Tensor, torch.Tensor]:
    import numpy as np
    f32, n = np.float32, _np32
    leaky = lambda s: np.where(s > 0, s, f32(w.slope) * s).astype(f32)  # noqa: E731
    obs, sf = n(state), n(sf)
    N, L, F_, M = obs.shape[0], w.map_len, w.feat, w.map_feat
    with np.errstate(all="ignore"):
        rows = obs[:, :5 * S].reshape(N, S, 5)
        fmap = _height_map_np(obs[:, 5 * S + 9:5 * S + 9 + L * L].reshape(N, 1, L, L), w, leaky)
        w_p1 = n(w.w_p1)
        base = np.broadcast_to(n(w.b_p1), (N, w.proj_hidden)).astype(f32)
        base = _chain_np(_chain_np(base, w_p1[:, :F_], sf), w_p1[:, F_:F_ + M], fmap)
        e2 = _lin_np(n(w.w_c2), n(w.b_c2), leaky(_lin_np(n(w.w_c1), n(w.b_c1), rows[:, :, :4])))
        h = leaky(_chain_np(np.broadcast_to(base[:, None, :], (N, S, w.proj_hidden)), w_p1[:, F_ + M:], e2))
        x = _lin_np(n(w.w_p2), n(w.b_p2), h)
        x = np.where((rows[:, :, 4] == f32(1))[:, :, None], x, f32(0)).astype(f32)
        xg = _mean_rows_np(x)
    return torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(xg))


def _embed_torch(state: torch.Tensor, sf: torch.Tensor, w: EmbedWeights, S: int) -> Tuple[torch.Tensor, torch.Tensor]:
    F = torch.nn.functional
    N, L, FM = state.shape[0], w.map_len, w.feat + w.map_feat
    rows = state[:, :5 * S].reshape(N, S, 5)
    fmap = _height_map_torch(state[:, 5 * S + 9:5 * S + 9 + L * L].reshape(N, 1, L, L), w)
    base = F.linear(torch.cat((sf, fmap), 1), w.w_p1[:, :FM], w.b_p1)         # once per bin, not once per row
    e2 = F.linear(F.leaky_relu(F.linear(rows[:, :, :4], w.w_c1, w.b_c1), w.slope), w.w_c2, w.b_c2)
    h = F.leaky_relu(F.linear(e2, w.w_p1[:, FM:]).add_(base[:, None, :]), w.slope)
    x = F.linear(h, w.w_p2, w.b_p2)
    x = torch.where((rows[:, :, 4] == 1)[:, :, None], x, torch.zeros((), dtype=x.dtype, device=x.device))
    return x, x.mean(1)


def _front_state(state: torch.Tensor, dev) -> torch.Tensor:
    """The observation block as float32 on the weights' device, rows contiguous and apart (a slice passes as it is)."""
    state = state.detach().to(device=dev, dtype=torch.float32)
    if state.stride(1) != 1 or (state.shape[0] > 1 and state.stride(0) < state.shape[1]):
        state = state.contiguous()
    return state


def _front_out(out: Optional[torch.Tensor], out_global: Optional[torch.Tensor], N: int, S: int, E: int, dev, allocate: bool):
    """``out`` [N, S, E] / ``out_global`` [N, E] of embed and order_embed checked and, with ``allocate`` (the kernels' path),
    made where missing -> (out, out_global, env_stride, row_stride, xg_stride): the strides irbpp_embed / irbpp_order_embed
    take, None without ``allocate``.  A dimension of one element has no stride of its own: the library gets what contiguous
    rows would have."""
    if out is not None and (out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (N, S, E) or
                            (E > 1 and out.stride(2) != 1) or (S > 1 and out.stride(1) < E) or
                            (N > 1 and out.stride(0) < (S - 1) * int(out.stride(1)) + E)):
        raise ValueError(f"out must be a float32 [{N}, {S}, {E}] tensor on the weights' device with contiguous rows")
    if out_global is not None and (out_global.dtype != torch.float32 or out_global.device != dev or
                                   tuple(out_global.shape) != (N, E) or (E > 1 and out_global.stride(1) != 1) or
                                   (N > 1 and out_global.stride(0) < E)):
        raise ValueError(f"out_global must be a float32 [{N}, {E}] tensor on the weights' device with contiguous rows")
    if not allocate:
        return out, out_global, None, None, None
    if out is None:
        out = torch.empty((N, S, E), dtype=torch.float32, device=dev)
    if out_global is None:
        out_global = torch.empty((N, E), dtype=torch.float32, device=dev)
    row_stride = int(out.stride(1)) if S > 1 else E
    env_stride = int(out.stride(0)) if N > 1 else (S - 1) * row_stride + E
    return out, out_global, env_stride, row_stride, int(out_global.stride(0)) if N > 1 else E


def _front_copy(x: torch.Tensor, xg: torch.Tensor, out: Optional[torch.Tensor], out_global: Optional[torch.Tensor]):
    """What a fallback computed, in ``out`` / ``out_global`` where the caller gave them."""
    return x if out is None else out.copy_(x), xg if out_global is None else out_global.copy_(xg)


def _embed_rows(state: torch.Tensor, w: EmbedWeights) -> int:
    """S of an observation block [N, obs_len] = 5 S + 9 + L^2 floats per row."""
    if state.dim() != 2:
        raise ValueError("state must be [N, obs_len]")
    S, rest = divmod(int(state.shape[1]) - 9 - w.map_len ** 2, 5)
    if rest != 0 or not 1 <= S <= EMBED_MAX_ROWS or state.shape[0] < 1:
        raise ValueError(f"embed: obs_len = 5 S + 9 + {w.map_len}^2 with 1 <= S <= 1024, and at least one row")
    return S


EMBED_FORMS = ("chain", "mfma")


def _embed_form(form: str, w: EmbedWeights) -> str:
    """``form`` of embed's HIP path: "chain" (irbpp_embed, the fmaf chains on the vector unit) or "mfma" (irbpp_embed_mfma, the
    three per-row layers on the matrix cores: the same bits).  "mfma" needs cand_hidden, cand_embed and proj_hidden to be
    multiples of 4 and says so."""
    if form not in EMBED_FORMS:
        raise ValueError(f"embed: form must be one of {EMBED_FORMS}, not {form!r}")
    if form == "mfma" and (w.cand_hidden % 4 or w.cand_embed % 4 or w.proj_hidden % 4):
        raise ValueError(f"embed: form='mfma' needs cand_hidden, cand_embed and proj_hidden to be multiples of 4 "
                         f"(cand_hidden {w.cand_hidden}, cand_embed {w.cand_embed}, proj_hidden {w.proj_hidden})")
    return form


@torch.no_grad()
def embed(state: torch.Tensor, shape_feature: torch.Tensor, weights: EmbedWeights, *, use_hip: Optional[bool] = None,
          out: Optional[torch.Tensor] = None, out_global: Optional[torch.Tensor] = None,
          form: str = "chain") -> Tuple[torch.Tensor, torch.Tensor]:
    """The embedding stage of DQNBPP.forward without a gradient (model.py:318-326, :337-352, bufferSize == 1): the observation
    ``state`` [N, obs_len] (a slice of a wider tensor passes as it is; S follows from obs_len and ``weights.map_len``) and
    ``shape_feature`` [N, F] (shape_features' result) -> (``x`` float32 [N, S, E], ``x_global`` float32 [N, E]): the reference's
    ``embeddings`` with the invalid rows zeroed and ``graph_embed``, what streams_greedy_action / streams_logits consume.
    ``out`` / ``out_global``: float32 tensors of those shapes with contiguous rows (slices pass) to write into.  Defined
    arithmetic (csrc/irbpp_embed.hip): every layer output one ascending fmaf chain from its bias, a convolution's over its
    zero-padded taps in (c_in, ky, kx) order, project_layer[0]'s over (shape feature, map feature, candidate embedding) as over
    the reference's concatenation -- its first F + M steps run once per bin, which changes no bit; a row whose mask is not
    exactly 1 is +0.0; the mean is over all S rows in irbpp_dueling_act's summation.  On CPU tensors the exact numpy emulation
    of the definition runs, on a HIP device with ``use_hip=True`` (``None`` takes EMBED_HIP_DEFAULT) the two launches of
    irbpp_embed, else torch's layers in the same factored form (MIOpen's and rocBLAS's summation orders: close to, not
    bit-equal with, the definition).  ``learn``'s forward with a gradient keeps torch's layers.  ``form`` chooses between the
    two row kernels of the HIP path, which give the same bits: "chain" (irbpp_embed) or "mfma" (irbpp_embed_mfma, the three
    per-row layers on the matrix cores; cand_hidden, cand_embed and proj_hidden multiples of 4).  An unknown form and
    "mfma" with other widths raise a ValueError on every path; the CPU emulation and torch's layers have one form and
    otherwise ignore it."""
    w = weights
    form = _embed_form(form, w)
    S = _embed_rows(state, w)
    N, E = int(state.shape[0]), w.embed
    dev = w.device
    state = _front_state(state, dev)
    sf = shape_feature.detach().to(device=dev, dtype=torch.float32)
    if tuple(sf.shape) != (N, w.feat):
        raise ValueError(f"shape_feature must be [{N}, {w.feat}]")
    if (w.feat > 1 and sf.stride(1) != 1) or (N > 1 and sf.stride(0) < w.feat):
        sf = sf.contiguous()
    lib = _head_lib(w.w_p1, use_hip, EMBED_HIP_DEFAULT)
    out, out_global, env_stride, row_stride, xg_stride = _front_out(out, out_global, N, S, E, dev, lib is not None)
    if lib is None:
        return _front_copy(*(_embed_torch(state, sf, w, S) if dev.type == "cuda" else _embed_cpu(state, sf, w, S)), out, out_global)
    from . import _lib
    ws = w._struct()
    name = "irbpp_embed_mfma" if form == "mfma" else "irbpp_embed"
    _lib.check(getattr(lib, name)(C.byref(ws), _p(state), int(state.stride(0)) if N > 1 else int(state.shape[1]), _p(sf),
                                  int(sf.stride(0)) if N > 1 else w.feat, S, N, _p(w._base(N)), _p(out), env_stride, row_stride,
                                  _p(out_global), xg_stride, _stream(dev)), name)
    return out, out_global


@torch.no_grad()
def network_greedy_action(state: torch.Tensor, points: ShapePoints, indices: torch.Tensor, shape_weights: ShapeEncoderWeights,
                          embed_weights: EmbedWeights, stream_weights: StreamWeights, support: torch.Tensor, *,
                          q_out: Optional[torch.Tensor] = None, use_hip: Optional[bool] = None,
                          streams_form: str = "chain", embed_form: str = "chain", mask: bool = True) -> torch.Tensor:
    """Agent.act from the observation (agent.py:51-58 with all of DQNBPP.forward, bufferSize == 1): ``state`` [N, obs_len] ->
    int64[N], the three stages chained with no torch layer in between: shape_features on the id column ``state[:, 5 S]``,
    embed, streams_greedy_action (which masks by the observation's validity flags; ``mask=False`` is ``Agent.act(state, None)``:
    the arg-max over all S rows, the invalid ones, whose embeddings are zero, included).  ``indices``: the forward's one index set
    (``points.draw_indices``); ``q_out`` as in streams_greedy_action; ``use_hip`` is handed to all three (``None``: each
    one's own default; ``True``: the whole forward in the defined float32 arithmetic, bit for bit what the CPU form gives);
    ``streams_form`` is streams_greedy_action's ``form``, ``embed_form`` embed's."""
    S = _embed_rows(state, embed_weights)
    sf = shape_features(state[:, 5 * S], points, indices, shape_weights, use_hip=use_hip)
    x, xg = embed(state, sf, embed_weights, use_hip=use_hip, form=embed_form)
    return streams_greedy_action(x, xg, stream_weights, support, state.to(x.device) if mask else None, q_out=q_out, use_hip=use_hip,
                                 form=streams_form)


# The same question for the order network's embedding stage ("The order network"): torch's layers in the
# factored form or the two launches of irbpp_order_embed.  Torch's layers, since tools/order_embed_rates.py measured on an
# MI355X, k = 10: 0.80 ms against 1.19 ms for the kernels at 4096 bins (spreads 0.01 ms) and 0.50 against 0.39 ms at 1024
# (spreads 0.05 / 0.01 ms): the kernels win at one size only, and the default changes only for a win beyond the larger spread
# at both (profiles/order_embed/).  The reference's lines with their host gather: 135 and 27 ms.  Measured for the stage from
# a given shape feature; the whole acting forward: 1.04 / 0.73 ms with every stage's default, 4.78 / 1.38 ms with
# use_hip=True throughout (irbpp_streams_act is most of that).  Not measured: other k, and bins below 1024.
# use_hip=True asks for the kernels (the reproducible forward).  form="mfma" (the eight linear layers on the matrix cores, the
# same bits) measured in a later run of the same tool: 0.825 ms against 1.197 (chain) and 0.821 (torch) at 4096 bins, 0.254
# against 0.394 and 0.523 at 1024: level with torch's layers at 4096, not beyond the spread, so the rule is still not met.
ORDER_EMBED_HIP_DEFAULT = False

ORDER_MAX_WIDTH, ORDER_MAX_SLOTS = 256, 64
_ORDER_FIELDS = ("w_conv1", "b_conv1", "w_conv2", "b_conv2", "w_conv3", "b_conv3", "w_g1", "b_g1", "w_g2", "b_g2", "w_q", "w_k", "w_v",
                 "w_o", "b_o", "w_f1", "b_f1", "w_f2", "b_f2")
_ORDER_SIZES = ("map_len", "c1", "c2", "c3", "feat", "proj_hidden", "embed", "ff_hidden")


class _IrbppOrderEmbedWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _ORDER_FIELDS] + [(n, C.c_int32) for n in _ORDER_SIZES] + [("slope", C.c_float)]


class OrderEmbedWeights(_FrontWeights):
    """The layers of the order network's embedding stage (DQNBPP with bufferSize > 1) as float32 contiguous tensors in torch's
    layouts: ``heightEncoder``'s three Conv2d, ``gat_project_layer``'s two Linear and ``embedder``, a GraphAttentionEncoder of
    one layer and one head, read as ``embedder.layers[0]``: ``[0].module`` gives ``W_query``, ``W_key``, ``W_val`` (no bias)
    and ``W_out``, ``[1].module`` the feed-forward pair Linear ReLU Linear.  Raises on ``n_heads != 1``, on more than one
    layer, on an ``init_embed`` and on widths that do not line up.  ``map_len`` is the heightmap's side L, from which the
    shape feature's width follows: F = gat_project_layer[0].in_features - c3 (L/4)^2.  Copies: call ``refresh()`` after every
    optimiser step."""
    _NAME, _FIELDS, _SIZES, _STRUCT = "order_embed", _ORDER_FIELDS, _ORDER_SIZES, _IrbppOrderEmbedWeights
    _MAX_WIDTH = ORDER_MAX_WIDTH
    _LIMITS = "1 <= feat, proj_hidden, embed, ff_hidden <= 256"

    def __init__(self, height_encoder, gat_project_layer, embedder, negative_slope: float = 0.01, *, map_len: int = 32):
        convs, projs = self._weighted(height_encoder, 4), self._weighted(gat_project_layer, 2)
        if len(convs) != 3 or len(projs) != 2:
            raise ValueError("order_embed: three Conv2d and two Linear (gat_project_layer)")
        if getattr(embedder, "init_embed", None) is not None:
            raise ValueError("order_embed: an embedder with an init_embed is not supported")
        layers = list(embedder.layers)
        if len(layers) != 1:
            raise ValueError("order_embed: one attention layer")
        att, ff = layers[0][0].module, layers[0][1].module
        if int(getattr(att, "n_heads", 1)) != 1:
            raise ValueError("order_embed: one attention head")
        ffs = self._weighted(ff, 2) if hasattr(ff, "__iter__") else []
        if len(ffs) != 2:
            raise ValueError("order_embed: the feed-forward pair Linear ReLU Linear")
        qkv = (att.W_query, att.W_key, att.W_val)
        if any(getattr(m, "bias", None) is not None for m in qkv):
            raise ValueError("order_embed: W_query, W_key and W_val have no bias")
        self.layers = tuple(convs + projs) + qkv + (att.W_out,) + tuple(ffs)
        if any(m.bias is None for m in convs + projs + [att.W_out] + ffs):
            raise ValueError("order_embed: every other layer has a bias")
        self._encoder(convs, negative_slope, map_len)
        self.proj_hidden, self.embed = int(projs[0].weight.shape[0]), int(projs[1].weight.shape[0])
        self.ff_hidden = int(ffs[0].weight.shape[0])
        self.feat = int(projs[0].weight.shape[1]) - self.map_feat
        E = self.embed
        self._finish([(self.c1, 1, 4, 4), (self.c2, self.c1, 4, 4), (self.c3, self.c2, 3, 3), (self.proj_hidden, self.feat + self.map_feat),
                      (E, self.proj_hidden), (E, E), (E, E), (E, E), (E, E), (self.ff_hidden, E), (E, self.ff_hidden)])
        import numpy as np
        self.norm = float(np.float32(1.0 / np.sqrt(np.float64(E))))     # nf: 1 / sqrt(E) in float64, rounded to float32 once


def _dexp_np(t):
    """dueling_dexp (csrc/irbpp_head.h) on a float32 numpy array of arguments <= 0: exactly 0 below -80."""
    import numpy as np
    f32 = np.float32
    tc = np.maximum(t.astype(f32), f32(-80.0))
    n = np.floor(tc * f32(1.4426950408889634) + f32(0.5))
    r = (tc - n * f32(0.693145751953125)) - n * f32(1.4286068203094172e-06)
    p = np.full(tc.shape, f32(1.9841269841269841e-04), dtype=f32)
    for c in (1.3888888888888889e-03, 8.3333333333333332e-03, 4.1666666666666664e-02, 1.6666666666666666e-01, 0.5, 1.0, 1.0):
        p = p * r + f32(c)
    scale = ((n.astype(np.int32) + 127) << 23).astype(np.uint32).view(f32)
    return np.where(t < f32(-80.0), f32(0), p * scale).astype(f32)


def _order_embed_cpu(state: torch.Tensor, sf: torch.Tensor, w: OrderEmbedWeights, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    import numpy as np
    f32, n = np.float32, _np32
    leaky = lambda s: np.where(s > 0, s, f32(w.slope) * s).astype(f32)  # noqa: E731
    relu = lambda s: np.where(s > 0, s, f32(0)).astype(f32)  # noqa: E731
    obs, sf = n(state), n(sf)
    N, L, F_, E = obs.shape[0], w.map_len, w.feat, w.embed
    with np.errstate(all="ignore"):
        fmap = _height_map_np(obs[:, k:k + L * L].reshape(N, 1, L, L), w, leaky)
        w_g1 = n(w.w_g1)
        base = _chain_np(np.broadcast_to(n(w.b_g1), (N, w.proj_hidden)).astype(f32), w_g1[:, F_:], fmap)     # the map goes first
        g = leaky(_chain_np(np.broadcast_to(base[:, None, :], (N, k, w.proj_hidden)), w_g1[:, :F_], sf))
        h0 = _lin_np(n(w.w_g2), n(w.b_g2), g)
        zero = np.zeros((E,), dtype=f32)
        q, key, v = (_lin_np(n(t), zero, h0) for t in (w.w_q, w.w_k, w.w_v))
        c = np.zeros((N, k, k), dtype=f32)
        for d in range(E):
            c = _fmaf_np(q[:, :, None, d], key[:, None, :, d], c)
        c = (f32(w.norm) * c).astype(f32)
        e = _dexp_np(c - c.max(-1, keepdims=True))
        den = np.zeros((N, k), dtype=f32)
        for j in range(k):
            den = den + e[:, :, j]
        att = (e / den[:, :, None]).astype(f32)
        hd = np.zeros((N, k, E), dtype=f32)
        for j in range(k):
            hd = _fmaf_np(att[:, :, j:j + 1], v[:, j:j + 1, :], hd)
        h1 = h0 + _lin_np(n(w.w_o), n(w.b_o), hd)
        x = h1 + _lin_np(n(w.w_f2), n(w.b_f2), relu(_lin_np(n(w.w_f1), n(w.b_f1), h1)))
        xg = _mean_rows_np(x)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=f32)), torch.from_numpy(np.ascontiguousarray(xg, dtype=f32))


def _order_embed_torch(state: torch.Tensor, sf: torch.Tensor, w: OrderEmbedWeights, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    F = torch.nn.functional
    N, L, F_ = state.shape[0], w.map_len, w.feat
    fmap = _height_map_torch(state[:, k:k + L * L].reshape(N, 1, L, L), w)
    base = F.linear(fmap, w.w_g1[:, F_:], w.b_g1)                                # once per bin, not once per slot
    h0 = F.linear(F.leaky_relu(F.linear(sf, w.w_g1[:, :F_]).add_(base[:, None, :]), w.slope), w.w_g2, w.b_g2)
    q, key, v = F.linear(h0, w.w_q), F.linear(h0, w.w_k), F.linear(h0, w.w_v)
    att = torch.softmax(w.norm * torch.matmul(q, key.transpose(1, 2)), dim=-1)
    h1 = h0 + F.linear(torch.matmul(att, v), w.w_o, w.b_o)
    x = h1 + F.linear(F.relu(F.linear(h1, w.w_f1, w.b_f1)), w.w_f2, w.b_f2)
    return x, x.mean(1)


def _order_slots(state: torch.Tensor, w: OrderEmbedWeights) -> int:
    """k of an order observation block [N, obs_len] = k + L^2 floats per row."""
    if state.dim() != 2:
        raise ValueError("state must be [N, obs_len]")
    k = int(state.shape[1]) - w.map_len ** 2
    if not 2 <= k <= ORDER_MAX_SLOTS or state.shape[0] < 1:
        raise ValueError(f"order_embed: obs_len = k + {w.map_len}^2 with 2 <= k <= 64, and at least one row")
    return k


ORDER_EMBED_FORMS = ("chain", "mfma")


def _order_embed_form(form: str, w: "OrderEmbedWeights") -> str:
    """``form`` of order_embed's HIP path: "chain" (irbpp_order_embed, the fmaf chains on the vector unit) or "mfma"
    (irbpp_order_embed_mfma, the eight linear layers on the matrix cores: the same bits).  "mfma" needs feat, proj_hidden, embed
    and ff_hidden to be multiples of 4 and says so."""
    if form not in ORDER_EMBED_FORMS:
        raise ValueError(f"order_embed: form must be one of {ORDER_EMBED_FORMS}, not {form!r}")
    if form == "mfma" and (w.feat % 4 or w.proj_hidden % 4 or w.embed % 4 or w.ff_hidden % 4):
        raise ValueError(f"order_embed: form='mfma' needs feat, proj_hidden, embed and ff_hidden to be multiples of 4 "
                         f"(feat {w.feat}, proj_hidden {w.proj_hidden}, embed {w.embed}, ff_hidden {w.ff_hidden})")
    return form


@torch.no_grad()
def order_embed(state: torch.Tensor, shape_feature: torch.Tensor, weights: OrderEmbedWeights, *, use_hip: Optional[bool] = None,
                out: Optional[torch.Tensor] = None, out_global: Optional[torch.Tensor] = None,
                form: str = "chain") -> Tuple[torch.Tensor, torch.Tensor]:
    """The embedding stage of the order network, DQNBPP.forward without a gradient for bufferSize > 1 (model.py:355-383): the
    order observation ``state`` [N, k + L^2] (k buffered item ids, then the heightmap; a slice of a wider tensor passes as it
    is; k follows from obs_len and ``weights.map_len``) and ``shape_feature`` [N*k, F] or [N, k, F] (shape_features over the
    N k ids, bin-major) -> (``x`` float32 [N, k, E], ``x_global`` float32 [N, E]): the reference's ``embeddings`` and
    ``graph_embed``, what streams_greedy_action consumes with ``state=None``.  ``out`` / ``out_global`` as in embed.  Defined
    arithmetic (csrc/irbpp_order_embed.hip): every layer output one ascending fmaf chain; gat_project_layer[0]'s runs over the
    map feature first (once per bin) and then over the slot's shape feature -- a fixed permutation of the reference's
    concatenation order; one attention head without a mask, its softmax with irbpp_dueling_act's exp; the mean in its
    summation.  On CPU tensors the exact numpy emulation of the definition runs, on a HIP device with ``use_hip=True``
    (``None`` takes ORDER_EMBED_HIP_DEFAULT) the two launches of irbpp_order_embed, else torch's layers in the same factored
    form (close to, not bit-equal with, the definition).  ``learn``'s forward with a gradient keeps torch's layers.  ``form``
    chooses between the two row kernels of the HIP path, which give the same bits: "chain" (irbpp_order_embed) or "mfma"
    (irbpp_order_embed_mfma, the eight linear layers on the matrix cores; feat, proj_hidden, embed and ff_hidden multiples of
    4).  An unknown form and "mfma" with other widths raise a ValueError on every path; the CPU emulation and torch's layers
    have one form and otherwise ignore it."""
    w = weights
    form = _order_embed_form(form, w)
    k = _order_slots(state, w)
    N, E, F_ = int(state.shape[0]), w.embed, w.feat
    dev = w.device
    state = _front_state(state, dev)
    sf = shape_feature.detach().to(device=dev, dtype=torch.float32)
    if tuple(sf.shape) not in ((N * k, F_), (N, k, F_)):
        raise ValueError(f"shape_feature must be [{N * k}, {F_}] or [{N}, {k}, {F_}]")
    if sf.dim() == 3:
        sf = sf.reshape(N * k, F_)                       # a view where the strides allow it, else a copy
    if (F_ > 1 and sf.stride(1) != 1) or sf.stride(0) < F_:
        sf = sf.contiguous()
    lib = _head_lib(w.w_g1, use_hip, ORDER_EMBED_HIP_DEFAULT)
    out, out_global, env_stride, row_stride, xg_stride = _front_out(out, out_global, N, k, E, dev, lib is not None)
    if lib is None:
        sf = sf.reshape(N, k, F_)
        return _front_copy(*(_order_embed_torch(state, sf, w, k) if dev.type == "cuda" else _order_embed_cpu(state, sf, w, k)), out, out_global)
    from . import _lib
    ws = w._struct()
    name = "irbpp_order_embed_mfma" if form == "mfma" else "irbpp_order_embed"
    _lib.check(getattr(lib, name)(C.byref(ws), _p(state), int(state.stride(0)) if N > 1 else int(state.shape[1]), _p(sf),
                                  int(sf.stride(0)), k, N, _p(w._base(N)), _p(out), env_stride, row_stride, _p(out_global),
                                  xg_stride, _stream(dev)), name)
    return out, out_global


@torch.no_grad()
def order_network_greedy_action(state: torch.Tensor, points: ShapePoints, indices: torch.Tensor, shape_weights: ShapeEncoderWeights,
                                order_weights: OrderEmbedWeights, stream_weights: StreamWeights, support: torch.Tensor, *,
                                q_out: Optional[torch.Tensor] = None, use_hip: Optional[bool] = None,
                                streams_form: str = "chain", order_form: str = "chain") -> torch.Tensor:
    """The order network's Agent.act from the observation (``orderDQN.act(orderState, None)``, trainer.py:266, with all of
    DQNBPP.forward for bufferSize > 1): ``state`` [N, k + L^2] -> int64[N] in [0, k), the three stages chained with no torch
    layer in between: shape_features on the N k ids ``state[:, :k]`` (one small strided copy makes them contiguous), order_embed,
    streams_greedy_action without a mask.  ``indices``, ``q_out`` and ``use_hip`` as in network_greedy_action (``True``: the
    whole forward in the defined float32 arithmetic, bit for bit what the CPU form gives: on CPU tensors the head is a numpy
    emulation of irbpp_dueling_act, not streams_greedy_action's torch lines); ``streams_form`` is streams_greedy_action's
    ``form``, ``order_form`` order_embed's."""
    order_form = _order_embed_form(order_form, order_weights)
    k = _order_slots(state, order_weights)
    sf = shape_features(state[:, :k].contiguous(), points, indices, shape_weights, use_hip=use_hip)
    x, xg = order_embed(state, sf, order_weights, use_hip=use_hip, form=order_form)
    if x.is_cuda:
        return streams_greedy_action(x, xg, stream_weights, support, None, q_out=q_out, use_hip=use_hip, form=streams_form)
    # the CPU form stays in the defined arithmetic to the end (streams_greedy_action's CPU form ends in torch's softmax)
    v, a = streams_logits(x, xg, stream_weights, use_hip=False)
    _q_out_arg(q_out, int(x.shape[0]), k, x.device, "state")
    return _dueling_act_cpu(v, a, support, q_out)


def _dueling_act_cpu(v: torch.Tensor, a: torch.Tensor, support: torch.Tensor, q_out: Optional[torch.Tensor]) -> torch.Tensor:
    """irbpp_dueling_act's arithmetic (csrc/irbpp_dueling.hip) without a mask, in numpy: x = (v + a) - dueling_mean(a), the
    softmax over the atoms with dueling_dexp and a left-to-right denominator, q = ((p0 z0 + p1 z1) + p2 z2) + .., the first
    maximum wins."""
    import numpy as np
    v, a, z = (t.detach().to(torch.float32).cpu().numpy() for t in (v, a, support))
    xs = (v[:, None, :] + a) - _mean_rows_np(a)[:, None, :]
    e = _dexp_np(xs - xs.max(-1, keepdims=True))
    den = e[..., 0]
    for j in range(1, e.shape[-1]):
        den = den + e[..., j]
    p = e / den[..., None]
    q = p[..., 0] * z[0]
    for j in range(1, p.shape[-1]):
        q = q + p[..., j] * z[j]
    if q_out is not None:
        q_out.copy_(torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)))
    return torch.from_numpy(q.argmax(1).astype(np.int64))


def actor_step(envs, policy, memory: VectorReplayMemory, state: torch.Tensor, reward_clip: float = 0.0):
    """One iteration of the trainer's acting loop (trainer.py:160-186) without per-env Python:
    mask -> policy -> envs.step -> clip -> append.  ``envs`` is a GpuPackingEnv (device-tensor
    API); ``policy(state, mask) -> int64[N]`` stands for Agent.act.  Returns the next state and
    (reward, done) device tensors.  The trainer's logged episode metrics (trainer.py:168-178, 215-222) stay on the device
    too when an irbpp_amd.metrics.EpisodeMetrics window is attached to ``envs``: read its rows every few hundred steps."""
    mask = mask_from_state(state, envs.S)
    action = policy(state, mask)
    next_state, reward, done = envs.step(action if action.dtype == torch.int32 else action.to(torch.int32))
    if reward_clip > 0:
        reward = reward.to(torch.float32).clamp(-reward_clip, reward_clip)           # trainer.py:181-182
    # every sample is Valid without physics.  (On a HIP device the append is one launch that takes the environment's own
    # float64 rewards and one-byte done flags: `reward` / `done` are then the step's views, overwritten by the next step.)
    memory.append(state, action, reward, done)
    return next_state, reward, done
