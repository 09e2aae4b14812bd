"""The three autograd Functions with a HIP backward as autograd nodes on the device (``use_hip=True``): _StreamsLogitsGrad,
_ShapeFeaturesGrad and _DuelingLossFunction held to the items of tests/test_autograd_contract_cpu.py by that file's own
helpers -- a tensor written in place before the backward raises, the target network's tensors do not count, the effective
weights belong to the call, backward twice, expanded / non-contiguous / float64 gradients, one output unused, frozen
parameter groups -- and, on the device only:

5. the batch edges, bit for bit against the numpy definitions: streams_logits_grad at B = 64, 512 and 1024 (the workload's
   two batch sizes and the limit; B = 1025 is refused) with E = H = 4, A = 2 and S of 1 and 33 (one staging trip, and one more
   row: both sides of the ``s0 > 0`` carry), through the wrapper and through the C ABI with a NaN-poisoned workspace;
   shape_features_grad at 100003 rows of a k = 4, 4 x 4 encoder (its wrapper sets no row limit of its own; the suite's
   largest was 640); dueling_c51_loss at B = 1024, S = 2, 2 atoms (the suite's largest batch was 65);
6. the backward under ``torch.cuda.stream(side)``: the bits of the single-stream run;
7. the three chained into two learn steps with optim.ClippedAdam: run to run the same bits, and the CPU form's.

Every assertion is equality of bits or a raised exception."""
import functools

import numpy as np
import pytest
import torch

import irbpp_amd  # noqa: F401
from irbpp_amd import replay
from test_autograd_contract_cpu import (CASES, LOSS_READ, SHAPE_GROUPS, SHAPE_READ, STREAMS_GROUPS, STREAMS_READ, LossCase, ShapeCase,
                                        StreamsCase, chain_run, check_backward_twice, check_bystanders, check_frozen, check_layouts,
                                        check_one_output, check_private_effective_weights, check_stale, same)
from test_dueling_loss_cpu import dueling_loss_backward_np, dueling_loss_np
from test_gpu_dueling_loss import loss_case
from test_gpu_shape_grad import definition as shape_definition
from test_gpu_streams_grad import capi
from test_streams_grad_cpu import NAMES, effective, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ON = dict(dev=DEV, use_hip=True)


# ---- 1. stale state ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
@pytest.mark.parametrize("name", STREAMS_READ)
def test_streams_backward_refuses_a_tensor_written_in_place(name, training):
    check_stale(StreamsCase(training=training, **ON), name)


@pytest.mark.parametrize("name", SHAPE_READ)
def test_shape_backward_refuses_a_tensor_written_in_place(name):
    check_stale(ShapeCase(**ON), name)


@pytest.mark.parametrize("name", LOSS_READ)
def test_loss_backward_refuses_a_tensor_written_in_place(name):
    case = LossCase(**ON)
    assert case.unread == ()
    check_stale(case, name)


def test_converted_copies_do_not_hide_the_callers_tensor():
    case = StreamsCase(**ON)
    case.x = case.x.detach().double().requires_grad_()
    check_stale(case, "x")
    for name in ("ids", "indices"):
        case = ShapeCase(**ON)
        case.ids, case.indices = case.ids.double(), case.indices.long()
        check_stale(case, name)
    for name in ("v", "a", "actions", "m"):
        case = LossCase(**ON)
        case.v, case.a = case.v.detach().double().requires_grad_(), case.a.detach().double().requires_grad_()
        case.actions, case.m = case.actions.int(), case.m.double()
        check_stale(case, name)


@pytest.mark.parametrize("which", list(CASES))
def test_writing_the_target_networks_tensors_changes_nothing(which):
    check_bystanders(CASES[which](**ON))


def test_streams_effective_weights_belong_to_the_call():
    check_private_effective_weights(StreamsCase(**ON))


# ---- 2, 3, 4 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(CASES))
def test_backward_twice(which):
    check_backward_twice(CASES[which](**ON))


@pytest.mark.parametrize("which", list(CASES))
def test_gradient_layouts(which):
    check_layouts(CASES[which](**ON))


@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
def test_streams_one_output_unused(training):
    check_one_output(StreamsCase(training=training, **ON))


@pytest.mark.parametrize("layer,kind", STREAMS_GROUPS)
def test_streams_frozen_group(layer, kind):
    check_frozen(StreamsCase(**ON), ["x"] if layer == "x" else [f"{layer}.weight_{kind}", f"{layer}.bias_{kind}"])


@pytest.mark.parametrize("frozen", SHAPE_GROUPS)
def test_shape_frozen_group(frozen):
    check_frozen(ShapeCase(**ON), list(frozen))


# ---- 5. batch edges ---------------------------------------------------------------------------------------------------------

def streams_want(case):
    """{name: array} of the numpy definition for a StreamsCase"""
    n = lambda t: t.detach().cpu().numpy()                   # noqa: E731
    w, eps = effective(case.layers)
    gv, ga = case.gout
    dx, dxg, grads = replay._streams_grad_backward_np(n(case.x), n(case.xg), w, eps, n(ga), n(gv))
    keys = list(case.leaves())
    assert len(keys) == 2 + len(NAMES)
    return dict(zip(keys, [dx, dxg] + [grads[name] for name in NAMES]))


@pytest.mark.parametrize("S", [1, 33])
@pytest.mark.parametrize("B", [64, 512, 1024])
def test_streams_batch_edges(B, S):
    case = StreamsCase(dims=(500 + B + S, B, S, 4, 4, 2), **ON)
    want = streams_want(case)
    same(case.run(), want, "the wrapper")
    gv, ga = case.gout
    through = capi(case.layers, case.x.detach(), case.xg.detach(), ga.contiguous(), gv.contiguous())
    same(dict(zip(want, [through["dx"], through["dxg"]] + [through[name] for name in NAMES])), want, "the C ABI")


def test_streams_batch_beyond_the_limit_is_refused():
    layers = make_case(5, 1, 1, 4, 4, 2, device=DEV)[0]
    for S in (1, 33):
        with pytest.raises(ValueError):
            replay.streams_logits_grad(torch.zeros(1025, S, 4, device=DEV), torch.zeros(1025, 4, device=DEV), *layers, use_hip=True)


def test_shape_rows_far_beyond_the_suites():
    case = ShapeCase(dims=(61, 5, 40, 4, 4, 4, 100003), **ON)
    n = lambda t: t.detach().cpu().numpy()                   # noqa: E731
    _, _, grads = shape_definition(n(case.points.points), n(case.indices), n(case.ids), case.W, n(case.gout[0]))
    same(case.run(), grads, "100003 rows")


def test_loss_at_the_streams_batch_limit():
    b, s, atoms = 1024, 2, 2
    v, a, actions, m, w = loss_case(b, s, atoms)
    _, g = dueling_loss_np(v, a, actions, m)
    want_v, want_a = dueling_loss_backward_np(g, w, actions, s)
    case = LossCase(dims=(b, s, atoms), **ON)
    t = lambda arr: torch.from_numpy(arr).to(DEV)             # noqa: E731
    case.v, case.a, case.actions, case.m, case.gout = t(v).requires_grad_(), t(a).requires_grad_(), t(actions), t(m), [t(w)]
    same(case.run(), {"v": want_v, "a": want_a}, "B = 1024")


# ---- 6. a side stream -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(CASES))
def test_backward_on_a_side_stream(which):
    case = CASES[which](**ON)
    want = case.run()
    case.clear()
    outs = case.forward()
    main, side = torch.cuda.current_stream(DEV), torch.cuda.Stream(device=DEV)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        torch.autograd.backward(outs, case.gout)
    main.wait_stream(side)
    side.synchronize()
    same(case.grads(), want, "backward on a side stream")


# ---- 7. the three chained ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def chain_on_the_cpu():
    return chain_run()


def test_chain_of_the_three_and_the_optimiser():
    first, again = chain_run(**ON), chain_run(**ON)
    same(first, again, "run to run on the device")
    same(first, chain_on_the_cpu(), "the device beside the CPU form")
