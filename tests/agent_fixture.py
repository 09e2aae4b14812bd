"""What the agent golden (tests/golden/agent_ref.npz) and its tests share: every number both sides start from, computed from
an integer hash so that it is the same bits on every machine, and `Net`, DQNBPP as plain torch layers.

`fill(name, shape, scale)` is float32 [shape] in (-scale, scale): element i is a splitmix64 hash of (FNV-1a of `name`, i), its
top 24 bits mapped to ((u + 0.5) / 2^23 - 1) * scale in float64 and rounded to float32 once.  No numpy or torch random stream
enters.  `fill_parameters(net)` and `fill_noise(net, salt)` write every parameter and every `*_epsilon` buffer of a network
by a name that does not depend on how its Sequentials label their members (`tensor_names`), so they fill the reference's
DQNBPP and `Net` alike: the golden stores no weights and no noise, both sides regenerate them.  The observations, the shape
tables and the learn batch come from here too.

`Net` is written against the layer shapes of the reference's model.py:258-299 (heightEncoder: Conv2d(1, 16, 4, 2, 1),
Conv2d(16, 32, 4, 2, 1), Conv2d(32, 4, 3, 1, 1); shapeEncoder: Linear(3, 128), Linear(128, 128); init_candidate_embed:
Linear(4, 32), Linear(32, 128); project_layer: Linear(512, 256), Linear(256, 128); for bufferSize > 1 an embedder of one
attention layer with one head and gat_project_layer: Linear(384, 256), Linear(256, 128); four noisy layers), LeakyReLU(0.01)
between them.  Its forward is the one that carries the gradient in `learn`, which stays with torch; for
bufferSize > 1 it only holds the parameters."""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

MASK64 = (1 << 64) - 1
GAIN = 1.7                                               # weights: uniform in +-GAIN / sqrt(fan_in), about unit variance kept
BIAS, NOISE, SIGMA = 0.1, 1.0, 0.5                       # biases +-0.1, epsilons +-1, sigmas +-0.5 / sqrt(fan_in)
POSITIONS = 512                                          # sampled positions per parameter tensor

# the scenarios (the smallest sizes the hard-coded layer widths allow; S and B below every wave and tile multiple)
S, B, ATOMS, HIDDEN, POINTS, L = 5, 6, 31, 128, 64, 32
N_SHAPES, TABLE_POINTS = 6, 200
K_ORDER, ORDER_TABLE_POINTS = 3, 10000                   # the order network resamples its table to 10000 points
V_MIN, V_MAX = -1.0, 8.0
# the reference's defaults (arguments.py)
LEARNING_RATE, ADAM_EPS, DISCOUNT, MULTI_STEP = 0.0000625, 1.5e-4, 0.99, 3
NORM_CLIP = 0.4475                                         # between the two steps' gradient norms: the clip is active in one
NOISY = ("fc_h_v", "fc_h_a", "fc_z_v", "fc_z_a")
# a gradient of zero in exact arithmetic: the advantage stream's bias is the same in every row and leaves with a - a.mean(1)
ZERO_GRADIENT = ("fc_z_a.bias_mu", "fc_z_a.bias_sigma")


def _name_seed(name: str) -> int:
    h = 0xcbf29ce484222325
    for c in name.encode("utf-8"):
        h = ((h ^ c) * 0x100000001b3) & MASK64
    return h


def _hash(name: str, n: int) -> np.ndarray:
    """uint64 [n]: splitmix64 of (seed of `name`) + (i + 1) * the golden-ratio increment."""
    with np.errstate(over="ignore"):
        x = np.uint64(_name_seed(name)) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def fill(name: str, shape, scale: float) -> np.ndarray:
    shape = tuple(int(d) for d in shape)
    u = (_hash(name, int(np.prod(shape, dtype=np.int64))) >> np.uint64(40)).astype(np.float64)
    return (((u + 0.5) / 2.0 ** 23 - 1.0) * float(scale)).astype(np.float32).reshape(shape)


def integers(name: str, shape, high: int) -> np.ndarray:
    """int64 [shape] in [0, high)."""
    shape = tuple(int(d) for d in shape)
    return ((_hash(name, int(np.prod(shape, dtype=np.int64))) >> np.uint64(33)) % np.uint64(high)).astype(np.int64).reshape(shape)


def positions(name: str, numel: int) -> np.ndarray:
    """The flat positions of a parameter tensor at which the golden keeps gradients and updates: every index 0 .. numel - 1
    of a tensor of at most POSITIONS elements, else POSITIONS hashed indices, drawn with replacement (a position may repeat)."""
    return np.arange(numel, dtype=np.int64) if numel <= POSITIONS else integers("positions/" + name, (POSITIONS,), numel)


# ---- the networks' numbers ---------------------------------------------------------------------------------------------------
def tensor_names(net):
    """[(name, parameter)] in the network's own order.  A name is the top-level member and the parameter's ordinal within it
    (`project_layer.2`), for a noisy layer the attribute (`fc_h_v.weight_sigma`): the same for every way of labelling the
    members of a Sequential."""
    out, count = [], {}
    for full, p in net.named_parameters():
        child, leaf = full.split(".")[0], full.split(".")[-1]
        if child in NOISY:
            out.append((f"{child}.{leaf}", p))
        else:
            out.append((f"{child}.{count.get(child, 0)}", p))
            count[child] = count.get(child, 0) + 1
    return out


def _scale(name: str, p, net) -> float:
    child, leaf = name.split(".")
    if child in NOISY:
        fan_in = int(getattr(net, child).weight_mu.shape[1])
        return {"weight_mu": GAIN / math.sqrt(fan_in), "bias_mu": BIAS}.get(leaf, SIGMA / math.sqrt(fan_in))
    return GAIN / math.sqrt(int(np.prod(p.shape[1:]))) if p.dim() >= 2 else BIAS


@torch.no_grad()
def fill_parameters(net) -> None:
    for name, p in tensor_names(net):
        p.copy_(torch.from_numpy(fill(name, p.shape, _scale(name, p, net))).to(device=p.device, dtype=p.dtype))


@torch.no_grad()
def fill_noise(net, salt: str) -> None:
    """Every `*_epsilon` buffer of the four noisy layers; `salt`: "online", "target/1", "target/2"."""
    for child in NOISY:
        layer = getattr(net, child)
        for leaf in ("weight_epsilon", "bias_epsilon"):
            t = getattr(layer, leaf)
            t.copy_(torch.from_numpy(fill(f"{salt}/{child}.{leaf}", t.shape, NOISE)).to(device=t.device, dtype=t.dtype))


# ---- the scenarios' inputs -----------------------------------------------------------------------------------------------------
def shape_table(name: str, n_points: int) -> np.ndarray:
    """float32 [N_SHAPES, n_points, 3]: shape s fills a box of (0.05 + 0.05 s) m a side, so the shapes' features differ."""
    half = (0.025 + 0.025 * np.arange(N_SHAPES, dtype=np.float64)).astype(np.float32)[:, None, None]
    return (fill("table/" + name, (N_SHAPES, n_points, 3), 1.0) * half + half).astype(np.float32)


ACT_MASKS = [[1, 0, 1, 1, 0], [0, 0, 0, 0, 0], [1, 1, 0, 1, 1], [1, 1, 1, 1, 1], [0, 1, 0, 0, 0], [0, 1, 1, 0, 1]]   # one bin all invalid
STATE_MASKS = [[1, 1, 0, 1, 1], [0, 1, 1, 0, 0], [1, 1, 1, 1, 1], [1, 0, 0, 0, 1], [0, 0, 1, 1, 1], [1, 1, 1, 0, 0]]
NEXT_MASKS = [[0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [1, 0, 1, 0, 1], [0, 0, 0, 1, 1], [1, 1, 0, 1, 0], [1, 0, 1, 1, 1]]


ORDER_IDS = [[4, 0, 2], [1, 3, 5], [3, 5, 0], [2, 4, 1], [0, 1, 2], [5, 2, 3]]


def item_observations(name: str, masks) -> np.ndarray:
    """float32 [B, 5 S + 9 + L^2]: S candidate rows (four values and the validity flag), the item id and eight more
    next-item values, the heightmap in centimetres of a 0.3 m bin."""
    masks = np.asarray(masks, dtype=np.float32)
    n = masks.shape[0]
    obs = np.zeros((n, 5 * S + 9 + L * L), dtype=np.float32)
    rows = obs[:, :5 * S].reshape(n, S, 5)
    rows[:, :, :4] = fill(name + "/rows", (n, S, 4), 0.16) + np.float32(0.16)
    rows[:, :, 4] = masks
    obs[:, 5 * S] = integers(name + "/ids", (n,), N_SHAPES)
    obs[:, 5 * S + 1:5 * S + 9] = fill(name + "/item", (n, 8), 0.5) + np.float32(0.5)
    obs[:, 5 * S + 9:] = np.round(fill(name + "/map", (n, L * L), 0.15).astype(np.float64) + 0.15, 2)
    return obs


def order_observations(name: str) -> np.ndarray:
    """float32 [B, K_ORDER + L^2]: the buffered item ids, then the heightmap.  The ids of a bin are distinct: two slots with
    one item have one value by construction."""
    obs = np.zeros((B, K_ORDER + L * L), dtype=np.float32)
    obs[:, :K_ORDER] = ORDER_IDS
    obs[:, K_ORDER:] = np.round(fill(name + "/map", (B, L * L), 0.15).astype(np.float64) + 0.15, 2)
    return obs


def learn_batch():
    """The sampled batch of both learn calls as numpy arrays: (states, actions, returns, next_states, nonterminals, weights).
    Sample 1 is terminal with a return below V_min, sample 2 has every Tz above V_max, sample 3 is terminal with Tz = 2.0,
    the atom of index 10; sample 5's lowest atoms clamp at V_min.  Every action is a valid row of its state."""
    states, next_states = item_observations("learn/states", STATE_MASKS), item_observations("learn/next_states", NEXT_MASKS)
    actions = np.array([3, 2, 0, 4, 2, 1], dtype=np.int64)
    returns = np.array([0.37, -1.5, 9.5, 2.0, 1.21, -0.4], dtype=np.float32)
    nonterminals = np.array([1, 0, 1, 0, 1, 1], dtype=np.float32).reshape(B, 1)
    weights = np.array([1.0, 0.31, 0.77, 0.52, 0.9, 0.64], dtype=np.float32)
    assert all(STATE_MASKS[i][a] == 1 for i, a in enumerate(actions))
    return states, actions, returns, next_states, nonterminals, weights


# ---- DQNBPP as plain layers ------------------------------------------------------------------------------------------------
class NoisyLayer(nn.Module):
    """mu + sigma * epsilon in training mode, mu alone in eval mode; the epsilons are buffers."""

    def __init__(self, fan_in: int, fan_out: int):
        super().__init__()
        self.weight_mu = nn.Parameter(torch.zeros(fan_out, fan_in))
        self.weight_sigma = nn.Parameter(torch.zeros(fan_out, fan_in))
        self.register_buffer("weight_epsilon", torch.zeros(fan_out, fan_in))
        self.bias_mu = nn.Parameter(torch.zeros(fan_out))
        self.bias_sigma = nn.Parameter(torch.zeros(fan_out))
        self.register_buffer("bias_epsilon", torch.zeros(fan_out))

    def forward(self, x):
        if self.training:
            return F.linear(x, self.weight_mu + self.weight_sigma * self.weight_epsilon, self.bias_mu + self.bias_sigma * self.bias_epsilon)
        return F.linear(x, self.weight_mu, self.bias_mu)


class _Wrapped(nn.Module):
    def __init__(self, module):
        super().__init__()
        self.module = module


class _Attention(nn.Module):
    n_heads = 1

    def __init__(self, dim: int):
        super().__init__()
        self.W_query, self.W_key, self.W_val = (nn.Linear(dim, dim, bias=False) for _ in range(3))
        self.W_out = nn.Linear(dim, dim)


class _Embedder(nn.Module):
    init_embed = None

    def __init__(self, dim: int, hidden: int):
        super().__init__()
        ff = nn.Sequential(nn.Linear(dim, hidden), nn.ReLU(), nn.Linear(hidden, dim))
        self.layers = nn.Sequential(nn.Sequential(_Wrapped(_Attention(dim)), _Wrapped(ff)))


class Net(nn.Module):
    def __init__(self, rows: int = S, atoms: int = ATOMS, hidden: int = HIDDEN, buffer_size: int = 1, map_len: int = L):
        super().__init__()
        self.rows, self.atoms, self.buffer_size, self.map_len = rows, atoms, buffer_size, map_len
        act = nn.LeakyReLU
        self.heightEncoder = nn.Sequential(nn.Conv2d(1, 16, 4, 2, 1), act(), nn.Conv2d(16, 32, 4, 2, 1), act(), nn.Conv2d(32, 4, 3, 1, 1), act())
        self.shapeEncoder = nn.Sequential(nn.Linear(3, 128), act(), nn.Linear(128, 128), act())
        self.init_candidate_embed = nn.Sequential(nn.Linear(4, 32), act(), nn.Linear(32, 128))
        self.project_layer = nn.Sequential(nn.Linear(512, 256), act(), nn.Linear(256, 128))
        if buffer_size > 1:
            self.embedder = _Embedder(128, 128)
            self.gat_project_layer = nn.Sequential(nn.Linear(384, 256), act(), nn.Linear(256, 128))
        self.fc_h_v, self.fc_h_a = NoisyLayer(128, hidden), NoisyLayer(128, hidden)
        self.fc_z_v, self.fc_z_a = NoisyLayer(hidden, atoms), NoisyLayer(hidden, atoms)

    def embeddings(self, x, points, indices):
        """-> (x [N, S, 128], x_global [N, 128]) with autograd; `points` is a replay.ShapePoints, whose gather stays on the
        device ("The shape branch")."""
        if self.buffer_size > 1:
            raise NotImplementedError("the order network is only acted with: its forward with a gradient is not needed")
        n, s, side = x.shape[0], self.rows, self.map_len
        rows = x[:, :5 * s].reshape(n, s, 5)
        fmap = self.heightEncoder(x[:, 5 * s + 9:].reshape(n, 1, side, side)).reshape(n, -1)
        shape_feature = torch.max(self.shapeEncoder(points.gather(x[:, 5 * s], indices)), dim=1)[0]
        cand = self.init_candidate_embed(rows[:, :, :4])
        joined = torch.cat((shape_feature[:, None, :].expand(n, s, -1), fmap[:, None, :].expand(n, s, -1), cand), dim=2)
        e = self.project_layer(joined)
        e = torch.where(rows[:, :, 4:5] == 1, e, torch.zeros((), dtype=e.dtype, device=e.device))
        return e, e.mean(1)

    def forward(self, x, points, indices):
        """-> the logits (v [N, atoms], a [N, S, atoms]) with autograd."""
        e, e_global = self.embeddings(x, points, indices)
        return self.fc_z_v(F.relu(self.fc_h_v(e_global))), self.fc_z_a(F.relu(self.fc_h_a(e)))


def make_nets(buffer_size: int = 1, device="cpu"):
    """(online, target) as Agent.__init__ leaves them: the online net filled, its noise drawn with the salt "online", the
    target a copy of all of it, both in training mode, the target without gradients."""
    rows = S if buffer_size == 1 else buffer_size
    online, target = Net(rows, buffer_size=buffer_size), Net(rows, buffer_size=buffer_size)
    fill_parameters(online)
    fill_noise(online, "online")
    target.load_state_dict(online.state_dict())
    for p in target.parameters():
        p.requires_grad = False
    return online.to(device).train(), target.to(device).train()
