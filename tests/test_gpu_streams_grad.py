"""irbpp_streams_backward on the device (csrc/irbpp_streams_grad.hip) against the numpy definition
(replay._streams_grad_backward_np, held to explicit loops in tests/test_streams_grad_cpu.py), bit for bit: through
replay.streams_logits_grad and through the C ABI with NaN-poisoned workspaces and outputs and inputs that are strided slices of
wider tensors.  Shapes: S around one staging trip of 32 rows, around 64, past 128 and past 512; widths below, off and on the
multiple of four, the workload's and the widest; atoms 2, 31 and 33; one and three samples -- every (S, widths) pair once, the
atoms and the batch rotating through them -- and the workload's row shape at a batch of five.  Two calls give the same bits;
both forms of the forward give the same bits; NULL outputs leave the others' bits alone; the limits are refused; one float64
comparison against torch's autograd at (8, 500, 128, 128, 31) with the CPU suite's bound."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, replay
from test_streams_grad_cpu import LAYERS, NAMES, PARAMS, check_against_reference, effective, f32, make_case, reference, run_wrapper, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IRBPP_ERR_ARG = -1

S_LIST = (1, 63, 64, 65, 129, 513)
WIDTHS = ((4, 4), (12, 36), (33, 17), (128, 128), (256, 256))
ATOMS = (2, 31, 33)
CASES = [((3, 1)[(i + j) % 2], s, e, h, ATOMS[(i + 2 * j) % 3]) for i, s in enumerate(S_LIST) for j, (e, h) in enumerate(WIDTHS)]
CASES.append((5, 500, 128, 128, 31))

_WANT = {}


def want_for(case):
    """the definition's result for a case, computed once"""
    if case not in _WANT:
        B, S, E, H, A = case
        layers, x, xg, gv, ga = make_case(1000 + S + E + A, B, S, E, H, A)
        w, eps = effective(layers)
        _WANT[case] = (layers, x, xg, gv, ga, w, eps,
                       replay._streams_grad_backward_np(x.numpy(), xg.numpy(), w, eps, ga.numpy(), gv.numpy()))
    return _WANT[case]


def to_dev(layers, *tensors):
    return [copy.deepcopy(layer).to(DEV) for layer in layers], [t.to(DEV) for t in tensors]


def check(got, want):
    same(got["dx"], want[0], "dx")
    same(got["dxg"], want[1], "dxg")
    for n in NAMES:
        same(got[n], want[2][n], n)


def capi(layers, x, xg, ga, gv, *, training=True, skip=()):
    """irbpp_streams_backward itself: x and xg strided slices of wider poisoned tensors, the workspace and every output NaN;
    `skip`: the outputs passed as NULL -> {name: numpy array}"""
    lib = _lib.load()
    B, S, E = x.shape
    sw = replay.StreamWeights(*layers, training=training)
    H, A = sw.hidden, sw.atoms
    nan = float("nan")
    wide = torch.full((B, S + 1, E + 3), nan, device=DEV)
    wide[:, :S, 2:2 + E] = x
    xs = wide[:, :S, 2:2 + E]
    gwide = torch.full((B, E + 5), nan, device=DEV)
    gwide[:, 1:1 + E] = xg
    xgs = gwide[:, 1:1 + E]
    n_ws = lib.irbpp_streams_backward_workspace(E, H, A, S, B)
    assert n_ws == 4 * B * (H * E + A * H + H + A + 2 * H)
    ws = torch.full((n_ws // 4,), nan, device=DEV)
    outs = {"dx": torch.full((B, S, E), nan, device=DEV), "dxg": torch.full((B, E), nan, device=DEV)}
    shapes = {"hv": ((H, E), (H,)), "zv": ((A, H), (A,)), "ha": ((H, E), (H,)), "za": ((A, H), (A,))}
    for layer in LAYERS:
        for p in PARAMS:
            outs[f"{layer}_{p}"] = torch.full(shapes[layer][p.startswith("bias")], nan, device=DEV)
    ptr = lambda n: None if n in skip else outs[n].data_ptr()                                  # noqa: E731
    eps = [getattr(layer, n).detach() for layer in layers for n in ("weight_epsilon", "bias_epsilon")]
    noise = replay._IrbppStreamNoise(*(t.data_ptr() for t in eps))
    grads = replay._IrbppStreamGrads(*(ptr(n) for n in NAMES))
    wst = sw._struct()
    p = lambda t: None if t is None else t.data_ptr()        # noqa: E731
    rc = lib.irbpp_streams_backward(C.byref(wst), C.byref(noise) if training else None, xgs.data_ptr(), xgs.stride(0), xs.data_ptr(),
                                    xs.stride(0), xs.stride(1), p(ga), p(gv), S, B, ws.data_ptr(), ptr("dx"), ptr("dxg"), C.byref(grads),
                                    None)
    assert rc == 0
    torch.cuda.synchronize()
    wide[:, :S, 2:2 + E] = nan
    gwide[:, 1:1 + E] = nan
    assert torch.isnan(wide).all() and torch.isnan(gwide).all()
    return {n: t.cpu().numpy() for n, t in outs.items()}


@pytest.mark.parametrize("B,S,E,H,A", CASES)
def test_bit_equal_to_the_definition(B, S, E, H, A):
    layers, x, xg, gv, ga, w, eps, want = want_for((B, S, E, H, A))
    dl, (dx_, dxg_, dgv, dga) = to_dev(layers, x, xg, gv, ga)
    v, a, got = run_wrapper(dl, dx_, dxg_, dgv, dga, use_hip=True)
    check(got, want)
    v0, a0 = replay.streams_logits(dx_, dxg_, replay.StreamWeights(*dl, training=True), use_hip=True)     # the forward: streams_logits' bits
    same(v, v0.cpu().numpy(), "v"), same(a, a0.cpu().numpy(), "a")
    _, _, again = run_wrapper(dl, dx_, dxg_, dgv, dga, use_hip=True)
    for n in ["dx", "dxg"] + NAMES:                          # all 18 outputs, run to run
        same(again[n], got[n], n)
    if E % 4 == 0 and H % 4 == 0:                            # every form that exists: the forward's two, one backward
        vm, am, mf = run_wrapper(dl, dx_, dxg_, dgv, dga, use_hip=True, form="mfma")
        same(vm, v, "v mfma"), same(am, a, "a mfma")
        for n in ["dx", "dxg"] + NAMES:
            same(mf[n], got[n], n)
    through = capi(dl, dx_, dxg_, dga.contiguous(), dgv.contiguous())
    check(through, want)


def test_null_outputs_missing_gradients_and_eval_mode():
    case = (3, 65, 12, 36, 31)
    layers, x, xg, gv, ga, w, eps, want = want_for(case)
    dl, (dx_, dxg_, dgv, dga) = to_dev(layers, x, xg, gv, ga)
    full = capi(dl, dx_, dxg_, dga, dgv)
    check(full, want)
    for skip in (("dx",), ("dxg",), ("dx", "dxg"), tuple(n for n in NAMES if n.endswith("sigma")), tuple(NAMES),
                 ("ha_weight_mu", "zv_bias_sigma", "za_weight_sigma", "hv_bias_mu")):
        got = capi(dl, dx_, dxg_, dga, dgv, skip=skip)
        for n in ["dx", "dxg"] + NAMES:
            if n in skip:
                assert np.isnan(got[n]).all(), n
            else:
                same(got[n], full[n], f"{n} without {skip}")
    n = lambda t: t.numpy()                                  # noqa: E731
    for a_, v_ in ((dga, None), (None, dgv), (None, None)):
        got = capi(dl, dx_, dxg_, a_, v_)
        check(got, replay._streams_grad_backward_np(n(x), n(xg), w, eps, None if a_ is None else n(ga), None if v_ is None else n(gv)))
    we, _ = effective(layers, training=False)
    got = capi(dl, dx_, dxg_, dga, dgv, training=False)
    ev = replay._streams_grad_backward_np(n(x), n(xg), we, None, n(ga), n(gv))
    same(got["dx"], ev[0]), same(got["dxg"], ev[1])
    for name in NAMES:
        if name.endswith("sigma"):
            assert np.isnan(got[name]).all(), name
        else:
            same(got[name], ev[2][name], name)
    # the wrapper: a detached x, eval mode
    _, _, det = run_wrapper(dl, dx_, dxg_, dgv, dga, use_hip=True, detach_x=True)
    assert det["dx"] is None
    for name in ["dxg"] + NAMES:
        same(det[name], full[name], name)
    _, _, evw = run_wrapper(dl, dx_, dxg_, dgv, dga, use_hip=True, training=False)
    for name in NAMES:
        if name.endswith("sigma"):
            assert evw[name] is None
        else:
            same(evw[name], ev[2][name], name)


def test_limits_are_refused():
    lib = _lib.load()
    layers, x, xg, gv, ga = make_case(5, 2, 3, 4, 4, 3, device=DEV)
    sw = replay.StreamWeights(*layers, training=True)
    ws = torch.zeros(4096, device=DEV)
    grads = replay._IrbppStreamGrads(*([None] * 16))

    def call(S=3, B=2, embed=4, hidden=4, atoms=3, ws_ptr=None, row_stride=4):
        wst = sw._struct()
        wst.embed, wst.hidden, wst.atoms = embed, hidden, atoms
        return lib.irbpp_streams_backward(C.byref(wst), None, xg.data_ptr(), 4, x.data_ptr(), 12, row_stride, ga.data_ptr(), gv.data_ptr(), S, B,
                                          ws.data_ptr() if ws_ptr is None else ws_ptr, None, None, C.byref(grads), None)

    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(S=0), dict(S=1025), dict(B=0), dict(B=1025), dict(embed=0), dict(embed=257), dict(hidden=0), dict(hidden=257),
               dict(atoms=1), dict(atoms=129), dict(ws_ptr=0), dict(row_stride=3)):
        assert call(**kw) == IRBPP_ERR_ARG, kw
    for args in ((4, 4, 3, 3, 1025), (4, 4, 3, 1025, 2), (257, 4, 3, 3, 2), (4, 0, 3, 3, 2), (4, 4, 129, 3, 2), (4, 4, 3, 3, 0)):
        assert lib.irbpp_streams_backward_workspace(*args) == 0, args
    with pytest.raises(ValueError):
        replay.streams_logits_grad(torch.zeros(1025, 1, 4, device=DEV), torch.zeros(1025, 4, device=DEV), *layers, use_hip=True)
    with pytest.raises(ValueError):
        replay.streams_logits_grad(torch.zeros(2, 1025, 4, device=DEV), torch.zeros(2, 4, device=DEV), *layers, use_hip=True)
    with pytest.raises(ValueError):
        replay.streams_logits_grad(x, xg, *layers, use_hip=True, form="other")


def clear_of_the_corner(layers, x, xg, seed):
    """Rows of x (and of xg) whose float64 pre-activations come within 2^-18 max|p| of the relu's corner are drawn again, until
    none does: the choice of inputs that check_against_reference then asserts, with no entry excluded."""
    rng = np.random.default_rng(seed)
    d = lambda t: t.detach().double()                        # noqa: E731
    for xin, layer in ((x, layers[2]), (xg, layers[0])):
        w, b = d(layer.weight_mu) + d(layer.weight_sigma) * d(layer.weight_epsilon), d(layer.bias_mu) + d(layer.bias_sigma) * d(layer.bias_epsilon)
        flat = xin.view(-1, xin.shape[-1])
        for _ in range(100):
            p = torch.nn.functional.linear(flat.double(), w, b).abs()
            bad = (p <= 2.0 ** -17 * p.max()).any(dim=1)     # twice the asserted margin: the maximum may move
            if not bad.any():
                break
            flat[bad] = torch.from_numpy(rng.standard_normal((int(bad.sum()), flat.shape[1])).astype(f32))
        else:
            raise AssertionError("no rows clear of the corner")


def test_float64_comparison_on_the_device():
    """torch's autograd in float64 on the device beside the kernels at (8, 500, 128, 128, 31): the CPU suite's bound,
    4 max(e_ref, 2^-24 max|ref64|) per tensor.  Largest error / scale measured on an MI355X: DESIGN.md section 3."""
    B, S, E, H, A = 8, 500, 128, 128, 31
    layers, x, xg, gv, ga = make_case(77, B, S, E, H, A)
    clear_of_the_corner(layers, x, xg, 78)
    dl, (dx_, dxg_, dgv, dga) = to_dev(layers, x, xg, gv, ga)
    _, _, got = run_wrapper(dl, dx_, dxg_, dgv, dga, use_hip=True)
    check_against_reference(got, dl, dx_, dxg_, dgv, dga, "device (8,500,128,128,31)")
