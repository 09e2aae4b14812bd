"""The noisy dueling streams (csrc/irbpp_streams.hip, replay.StreamWeights / streams_greedy_action / streams_logits) without a
GPU.

The kernels' arithmetic is defined (the header of irbpp_streams.hip); this file carries that definition as numpy code
(``fmaf_np``, ``lin_np``, ``streams_logits_np``, ``streams_act_np``: tests/test_gpu_streams.py and
tests/test_streams_kernel_on_host.py hold the kernels to it bit for bit) and checks the definition itself:

* ``fmaf_np`` (float64 product, TwoSum, round-to-odd) against exact rational arithmetic, midpoint cases included;
* the effective weights against torch's ``mu + sigma * eps``;
* the definition against the reference's torch lines in float64 within the bound derived in ``stream_bounds``;
* the wrappers' CPU form and the IRBPP_ERR_ARG limits of the two entry points (checked before any HIP call)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_c51_cpu import act_torch
from test_dueling_cpu import DEXP_MAX_ULP, PARTS, U, dueling_act_np, f32, gap64, head_torch

f64 = np.float64


# ------------------------------------------------------------------ the definition, in numpy ------------
def fmaf_np(a, b, c):
    """fmaf(a, b, c) on float32 arrays -> float32, one rounding.  a * b is exact in float64 (48 bits); s = fl64(p + c) with its
    TwoSum error e; where e != 0 and s is even, the neighbour of s on e's side is taken instead (round-to-odd: the float64 then
    never sits on a float32 midpoint or grid point it is not exactly on), and the rounding to float32 is the single one."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    p = a.astype(f64) * b.astype(f64)
    c = c.astype(f64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    bits = s.view(np.int64).copy()
    even = (bits & 1) == 0
    up = (e > 0) == (s > 0)                                # away from zero in the bit pattern
    bits = np.where((e != 0) & even, np.where(up, bits + 1, bits - 1), bits)
    return bits.view(f64).astype(f32)


def lin_np(w, b, x):
    """x [..., K], w [J, K], b [J] -> [..., J]: acc = b[j]; acc = fmaf(x[k], w[j][k], acc), k ascending."""
    acc = np.broadcast_to(np.asarray(b, f32), x.shape[:-1] + (w.shape[0],))
    for k in range(w.shape[1]):
        acc = fmaf_np(x[..., k:k + 1], w[:, k], acc)
    return acc


def relu_np(t):
    return np.where(t > 0, t, f32(0)).astype(f32)


def streams_logits_np(W, xg, x):
    """W: dict of the eight effective arrays -> (v [N, atoms], a [N, S, atoms])."""
    v = lin_np(W["w_zv"], W["b_zv"], relu_np(lin_np(W["w_hv"], W["b_hv"], np.asarray(xg, f32))))
    a = lin_np(W["w_za"], W["b_za"], relu_np(lin_np(W["w_ha"], W["b_ha"], np.asarray(x, f32))))
    return v, a


def streams_act_np(W, xg, x, z, flags=None):
    """-> (action int64 [N], q float32 [N, S], v, a)."""
    v, a = streams_logits_np(W, xg, x)
    act, q, _ = dueling_act_np(v, a, z, flags)
    return act, q, v, a


NAMES = ("w_hv", "b_hv", "w_zv", "b_zv", "w_ha", "b_ha", "w_za", "b_za")


class Layer(object):
    """What StreamWeights.from_layers asks of a layer, and nothing else."""

    def __init__(self, rng, out, inp, scale=1.0):
        t = lambda *s: torch.from_numpy((rng.standard_normal(s) * scale).astype(f32))      # noqa: E731
        self.weight_mu, self.weight_sigma, self.weight_epsilon = t(out, inp) / np.sqrt(inp), t(out, inp) * 0.1, t(out, inp)
        self.bias_mu, self.bias_sigma, self.bias_epsilon = t(out) * 0.3, t(out) * 0.1, t(out)

    def to(self, dev):
        for n in ("weight_mu", "weight_sigma", "weight_epsilon", "bias_mu", "bias_sigma", "bias_epsilon"):
            setattr(self, n, getattr(self, n).to(dev))
        return self


def make_layers(rng, E, H, atoms, scale=1.0):
    return [Layer(rng, H, E, scale), Layer(rng, atoms, H, scale), Layer(rng, H, E, scale), Layer(rng, atoms, H, scale)]


def effective_np(layers, training=True):
    """the definition of the effective weights: two float32 ops, or mu in eval mode"""
    out = {}
    for (wn, bn), l in zip((("w_hv", "b_hv"), ("w_zv", "b_zv"), ("w_ha", "b_ha"), ("w_za", "b_za")), layers):
        n = lambda t: t.cpu().numpy()                      # noqa: E731
        out[wn] = n(l.weight_mu) + n(l.weight_sigma) * n(l.weight_epsilon) if training else n(l.weight_mu).copy()
        out[bn] = n(l.bias_mu) + n(l.bias_sigma) * n(l.bias_epsilon) if training else n(l.bias_mu).copy()
        assert out[wn].dtype == f32 and out[bn].dtype == f32
    return out


# ------------------------------------------------------------------ fmaf ------------
def round_f32(fr):
    """Fraction -> the nearest float32, ties to even (normal and subnormal range)."""
    if fr == 0:
        return f32(0)
    sign, fr = (-1, -fr) if fr < 0 else (1, fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    e = max(e, -126)
    q = fr / Fraction(2) ** (e - 23)
    n, r = divmod(q.numerator, q.denominator)
    half = Fraction(r, q.denominator)
    if half > Fraction(1, 2) or (half == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return f32(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))


def midpoint_triples():
    """a b + c within a float64 ulp of a float32 midpoint but not on it: a b = 2^(e-24) (1 - i^2 2^-46) is short of half an ulp
    of c = +-2^e (1 + k 2^-23) by i^2 2^(e-70), far below the float64 ulp 2^(e-52) of the sum: fl64(a b + c) IS the midpoint,
    and rounding that to float32 goes to even, the wrong side for half of the k."""
    out = []
    for e in (-20, 0, 10, 30):
        for i in range(1, 40):
            for k in range(8):
                for sgn in (1.0, -1.0):
                    out.append((f32(2.0 ** (e - 24) * (1 + i * 2.0 ** -23)), f32(1 - i * 2.0 ** -23), f32(sgn * 2.0 ** e * (1 + k * 2.0 ** -23))))
    return np.array(out, dtype=f32)


@pytest.mark.parametrize("fma", [fmaf_np, replay._fmaf_np], ids=["definition", "replay"])
def test_fmaf_is_exact(fma):
    rng = np.random.default_rng(5)
    n = 3000
    rand = np.stack([rng.standard_normal(n), rng.standard_normal(n),
                     rng.standard_normal(n) * 2.0 ** rng.integers(-30, 6, n)], 1).astype(f32)
    cancel = rand.copy()
    cancel[:, 2] = -(cancel[:, 0].astype(f64) * cancel[:, 1].astype(f64)).astype(f32)       # a b + c cancels to the product's tail
    tiny = (rand * np.array([2.0 ** -70, 2.0 ** -65, 2.0 ** -140], dtype=f64)).astype(f32)   # subnormal results
    mid = midpoint_triples()
    trip = np.concatenate([rand, cancel, tiny, mid])
    got = fma(trip[:, 0], trip[:, 1], trip[:, 2])
    want = np.array([round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))) for a, b, c in trip], dtype=f32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    naive = (mid[:, 0].astype(f64) * mid[:, 1].astype(f64) + mid[:, 2].astype(f64)).astype(f32)
    assert (naive != want[-len(mid):]).sum() > len(mid) // 4, "the midpoint cases are meant to defeat a float64 emulation"


def test_lin_is_the_ascending_chain():
    """The order is observable: 1e8, 1, -1e8 sums to 0 in this order with one rounding per step, and to 1 in another."""
    x = np.array([[1.0, 1.0, 1.0]], dtype=f32)
    w = np.array([[1e8, 1.0, -1e8], [1e8, -1e8, 1.0]], dtype=f32)
    np.testing.assert_array_equal(lin_np(w, np.zeros(2, f32), x), [[0.0, 1.0]])
    assert relu_np(np.array([-0.0, -1.0, 2.0], dtype=f32)).view(np.uint32).tolist() == [0, 0, 0x40000000]


# ------------------------------------------------------------------ effective weights ------------
@pytest.mark.parametrize("training", [True, False])
def test_effective_weights_are_torchs(training):
    rng = np.random.default_rng(6)
    layers = make_layers(rng, 37, 19, 31)
    w = replay.StreamWeights.from_layers(*layers, training=training)
    assert (w.embed, w.hidden, w.atoms) == (37, 19, 31)
    want = effective_np(layers, training)
    for (wn, bn), l in zip((("w_hv", "b_hv"), ("w_zv", "b_zv"), ("w_ha", "b_ha"), ("w_za", "b_za")), layers):
        tw = l.weight_mu + l.weight_sigma * l.weight_epsilon if training else l.weight_mu
        tb = l.bias_mu + l.bias_sigma * l.bias_epsilon if training else l.bias_mu
        assert torch.equal(getattr(w, wn), tw) and torch.equal(getattr(w, bn), tb)
        np.testing.assert_array_equal(want[wn], tw.numpy())
        np.testing.assert_array_equal(want[bn], tb.numpy())
    layers[2].weight_epsilon = layers[2].weight_epsilon + 1          # a reset_noise
    old = w.w_ha.clone()
    w.refresh()
    assert torch.equal(w.w_ha, old) != training
    with pytest.raises(ValueError):
        replay.StreamWeights.from_layers(layers[0], layers[1], layers[1], layers[3])
    with pytest.raises(ValueError):
        replay.StreamWeights.from_layers(*make_layers(rng, 257, 8, 31))
    with pytest.raises(ValueError):
        replay.StreamWeights.from_layers(*make_layers(rng, 8, 8, 129))


# ------------------------------------------------------------------ the definition against the reference ------------
def stream_bounds(W, xg, x, z):
    """Bounds on |definition - exact| for v, a and q (the float64 torch lines stand for exact; u = 2^-24; first-order terms
    times 1.02 for the higher orders).

    A chain of K fused multiply-adds rounds K times, each within u of a partial sum that is at most T = |b| + sum_k |x_k| |w_k|
    in magnitude: |chain - exact| <= 1.02 K u T.  T is evaluated in float64 from the absolute values, per output.
    h: dh = 1.02 E u (|b_h| + |x| |W_h|^T); relu moves nothing further (1-Lipschitz, exact).
    logits: the hidden errors pass through |W_z| and the second chain rounds H times:
       da = dh |W_z|^T + 1.02 H u (|b_z| + h |W_z|^T), with h the exact hidden row (plus dh); likewise dv.
    From there the bounds of test_dueling_cpu.bounds with the input errors added: x there (the combined logit) carries
       dx = (ceil(S / 16) + 19) u (V + A) + dv + 2 da    (a and the column mean both carry da),
    t = x - mx: dt = 2 dx + 80 u; e: ee = dt + 2 DEXP_MAX_ULP u; p: ep = 2 ee + atoms u;
    q: dq = (1.02 ep + 2e-35 atoms + atoms u) Z, Z = max |z|."""
    d = lambda t: np.abs(np.asarray(t, f64))               # noqa: E731

    def stream(wh, bh, wz, bz, inp):
        E, H = wh.shape[1], wh.shape[0]
        dh = 1.02 * E * U * (d(bh) + d(inp) @ d(wh).T)
        h = np.maximum(np.asarray(inp, f64) @ np.asarray(wh, f64).T + np.asarray(bh, f64), 0) + dh
        return float((dh @ d(wz).T + 1.02 * H * U * (d(bz) + h @ d(wz).T)).max())
    dv = stream(W["w_hv"], W["b_hv"], W["w_zv"], W["b_zv"], xg)
    da = stream(W["w_ha"], W["b_ha"], W["w_za"], W["b_za"], x)
    v, a = streams_logits_np(W, xg, x)
    s, atoms = a.shape[1], a.shape[2]
    V, A, Z = float(np.abs(v).max()), float(np.abs(a).max()), float(np.abs(z).max())
    dx = (-(-s // PARTS) + 19) * U * (V + A) + dv + 2 * da
    ee = 2 * dx + 80 * U + 2 * DEXP_MAX_ULP * U
    ep = 2 * ee + atoms * U
    return dv, da, (1.02 * ep + 2e-35 * atoms + atoms * U) * Z


def planted_case(rng, n, s, E, H, atoms, lead=12.0):
    """Layers, xg [n, E], x [n, s, E] with a planted leader per env: hidden unit 0 of the advantage stream reads x[.., 0] alone
    (and no other unit reads it) and feeds the last atom alone, and the leader's x[.., 0] is `lead`: its distribution sits on
    z[-1], the largest value."""
    layers = make_layers(rng, E, H, atoms, 0.5)
    ha, za = layers[2], layers[3]
    for t in (ha.weight_mu, ha.weight_sigma):
        t[0] = 0
        t[:, 0] = 0
    ha.weight_mu[0, 0] = 1
    ha.bias_mu[0], ha.bias_sigma[0] = 0, 0
    for t in (za.weight_mu, za.weight_sigma):
        t[:, 0] = 0
    za.weight_mu[-1, 0] = 1
    xg = (rng.standard_normal((n, E)) * 0.25).astype(f32)
    x = (rng.standard_normal((n, s, E)) * 0.25).astype(f32)
    leader = rng.integers(0, s, n)
    x[np.arange(n), leader, 0] = lead
    return layers, xg, x, leader


def streams_torch(W, xg, x):
    """model.py:393-394 on float64 tensors"""
    t = lambda k: torch.from_numpy(W[k]).double()           # noqa: E731
    v = F.linear(F.relu(F.linear(xg, t("w_hv"), t("b_hv"))), t("w_zv"), t("b_zv"))
    a = F.linear(F.relu(F.linear(x, t("w_ha"), t("b_ha"))), t("w_za"), t("b_za"))
    return v, a


CONFIGS = [(3, 50, 128, 128, 31, -1.0, 8.0), (2, 500, 16, 24, 31, -1.0, 8.0), (3, 33, 130, 67, 51, -10.0, 10.0), (4, 7, 5, 3, 2, 0.0, 1.0),
           (2, 20, 256, 256, 128, -1.0, 4.0), (3, 1, 9, 9, 31, -1.0, 8.0)]


@pytest.mark.parametrize("n,s,E,H,atoms,v_min,v_max", CONFIGS)
def test_definition_against_the_reference(n, s, E, H, atoms, v_min, v_max):
    rng = np.random.default_rng(500 + s)
    z = torch.linspace(v_min, v_max, atoms).numpy()
    layers, xg, x, leader = planted_case(rng, n, s, E, H, atoms)
    W = effective_np(layers)
    flags = (rng.random((n, s)) < 0.7).astype(f32)
    flags[np.arange(n), leader] = 1
    dv, da, dq = stream_bounds(W, xg, x, z)
    v64, a64 = streams_torch(W, torch.from_numpy(xg).double(), torch.from_numpy(x).double())
    p64 = head_torch(v64, a64)
    support64 = torch.from_numpy(z).double()
    for fl in (None, flags):
        want, q64 = act_torch(p64, support64, None if fl is None else torch.from_numpy(fl).double())
        got, q, v, a = streams_act_np(W, xg, x, z, fl)
        ev, ea, eq = np.abs(v - v64.numpy()).max(), np.abs(a - a64.numpy()).max(), np.abs(q.astype(f64) - q64.numpy()).max()
        print(f"v {ev:.3g} <= {dv:.3g}, a {ea:.3g} <= {da:.3g}, q {eq:.3g} <= {dq:.3g}, gap {gap64(q64.numpy(), fl).min():.3g}")
        assert ev <= dv and ea <= da and eq <= dq
        assert (gap64(q64.numpy(), fl) > 100 * dq).all(), "the planted leader does not lead by 100 bounds"
        np.testing.assert_array_equal(want.numpy(), leader)
        np.testing.assert_array_equal(got, want.numpy())


# ------------------------------------------------------------------ the wrappers on the CPU ------------
def test_wrappers_follow_the_definition_on_the_cpu():
    rng = np.random.default_rng(11)
    n, s, E, H, atoms = 4, 9, 12, 7, 31
    layers, xg, x, leader = planted_case(rng, n, s, E, H, atoms)
    W = effective_np(layers)
    w = replay.StreamWeights.from_layers(*layers)
    support = torch.linspace(-1.0, 8.0, atoms)
    wide = torch.full((n, s + 2, E + 5), 1e30)
    wide[:, 1:1 + s, 2:2 + E] = torch.from_numpy(x)
    wide_g = torch.full((n, E + 3), 1e30)
    wide_g[:, 1:1 + E] = torch.from_numpy(xg)
    want_v, want_a = streams_logits_np(W, xg, x)
    for xs, gs in ((torch.from_numpy(x), torch.from_numpy(xg)), (wide[:, 1:1 + s, 2:2 + E], wide_g[:, 1:1 + E].unsqueeze(1))):
        v, a = replay.streams_logits(xs, gs, w)
        assert v.dtype == torch.float32 and not v.requires_grad
        np.testing.assert_array_equal(v.numpy(), want_v)
        np.testing.assert_array_equal(a.numpy(), want_a)
        state = torch.zeros((n, s * 5 + 3))
        mask = torch.ones((n, s))
        mask[np.arange(n), leader] = 0
        mask[2] = 0
        state[:, :s * 5].view(n, s, 5)[:, :, 4] = mask
        q_out = torch.full((n, s), 7.0)
        act = replay.streams_greedy_action(xs, gs, w, support, q_out=q_out)
        assert act.dtype == torch.int64 and act.tolist() == leader.tolist()
        want_act = replay.dueling_greedy_action(v, a, support, state, use_hip=False)
        got = replay.streams_greedy_action(xs, gs, w, support, state)
        assert torch.equal(got, want_act) and got[2] == 0 and (got.numpy() != leader)[[0, 1, 3]].all()
        assert np.abs(q_out.numpy() - streams_act_np(W, xg, x, support.numpy())[1]).max() < 1e-4
    with pytest.raises(ValueError):
        replay.streams_logits(torch.zeros((n, s, E + 1)), torch.zeros((n, E)), w)
    with pytest.raises(ValueError):
        replay.streams_logits(torch.zeros((n, s, E)), torch.zeros((n + 1, E)), w)
    with pytest.raises(ValueError):
        replay.streams_logits(torch.zeros((1, 1025, E)), torch.zeros((1, E)), w)
    with pytest.raises(RuntimeError, match="HIP device"):
        replay.streams_greedy_action(torch.from_numpy(x), torch.from_numpy(xg), w, support, use_hip=True)
    assert replay.STREAMS_HIP_DEFAULT in (False, True)


# ------------------------------------------------------------------ limits of the entry points ------------
@pytest.fixture(scope="module")
def lib():
    from irbpp_amd import _lib, build
    build.build()
    return _lib.load()


NULL = C.c_void_p(0)
BUF = np.zeros(4096, dtype=f32)
PTR = C.c_void_p(BUF.ctypes.data)


def _call(lib, **kw):
    d = dict(w=dict(), embed=8, hidden=8, atoms=31, xg=PTR, xg_stride=8, x=PTR, env_stride=32, row_stride=8, support=PTR, obs=PTR,
             obs_stride=20, s_rows=4, n_env=1, action=PTR, q_out=PTR, q_stride=4, v_out=PTR, a_out=PTR, no_struct=False)
    d.update(kw)
    ptrs = {n: PTR.value for n in NAMES}
    ptrs.update(d["w"])
    ws = replay._IrbppStreamWeights(*(ptrs[n] for n in NAMES), d["embed"], d["hidden"], d["atoms"])
    return lib.irbpp_streams_act(None if d["no_struct"] else C.byref(ws), d["xg"], d["xg_stride"], d["x"], d["env_stride"],
                                 d["row_stride"], d["support"], d["obs"], d["obs_stride"], d["s_rows"], d["n_env"], d["action"], d["q_out"],
                                 d["q_stride"], d["v_out"], d["a_out"], None)


BAD = [dict(embed=0), dict(embed=257, xg_stride=257, row_stride=257, env_stride=2000), dict(hidden=0), dict(hidden=257), dict(atoms=1),
       dict(atoms=129), dict(s_rows=0), dict(s_rows=1025, env_stride=1 << 20, obs_stride=1 << 20, q_stride=1 << 20), dict(n_env=0),
       dict(n_env=-2), dict(xg_stride=7), dict(row_stride=7), dict(env_stride=31), dict(obs_stride=19), dict(q_stride=3), dict(xg=NULL),
       dict(x=NULL), dict(support=NULL), dict(no_struct=True), dict(action=NULL, q_out=NULL, v_out=NULL, a_out=NULL),
       dict(s_rows=1024, atoms=128, env_stride=1 << 20, obs_stride=1 << 20, q_stride=1 << 20, a_out=NULL)] + \
      [dict(w={n: None}) for n in NAMES]
ids = lambda d: ",".join(f"{k}={getattr(v, 'value', v)}" for k, v in d.items())      # noqa: E731


@pytest.mark.parametrize("bad", BAD, ids=ids)
def test_streams_act_rejects_what_is_outside_its_limits(lib, bad):
    assert _call(lib, **bad) == -1                          # IRBPP_ERR_ARG before any HIP call


@pytest.mark.parametrize("bad", [dict(out=0), dict(out=257), dict(inp=0), dict(inp=257)] + [dict(null=i) for i in range(8)], ids=ids)
def test_noisy_weights_rejects_what_is_outside_its_limits(lib, bad):
    args = [PTR] * 6 + [bad.get("out", 4), bad.get("inp", 4), PTR, PTR]
    if "null" in bad:
        args[bad["null"] if bad["null"] < 6 else bad["null"] + 2] = NULL
    assert lib.irbpp_noisy_weights(*args, None) == -1
