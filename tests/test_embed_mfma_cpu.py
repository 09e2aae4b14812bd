"""The second form of the embedding stage's row launch (csrc/irbpp_embed_mfma.hip, ``form="mfma"``) without a GPU: the
wrapper's argument rules -- an unknown form, widths that are no multiple of 4, the form ignored on CPU tensors -- and
irbpp_embed_mfma's refusals through the C ABI, which are answered before any device call: everything irbpp_embed refuses (the
BAD list of tests/test_embed_cpu.py) with the same status, and the three widths that are the K of its products.

Also the configurations, (N, S) lists and inputs that tests/test_embed_mfma_kernel_on_host.py and tests/test_gpu_embed_mfma.py
share, and the layers of the definition one by one (for the check that the inputs tell the order of a chain)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from irbpp_amd import replay
from test_embed_cpu import BAD, NAMES, PTR, REFERENCE, SMALL, embed_cpu, ids, lib, make_layers, make_obs, same_bits, weights_of  # noqa: F401

f32 = np.float32


def widths(base, cand_hidden, cand_embed, proj_hidden, embed, **kw):
    return dict(base, cand_hidden=cand_hidden, cand_embed=cand_embed, proj_hidden=proj_hidden, embed=embed, **kw)


# (L, convs) of SMALL or REFERENCE.  small4: one partial feature block everywhere, embed no multiple of 4; blocks: several
# feature blocks, the last partial; the reference's widths; widest: the LDS bound; small4u: weight rows of project_layer[0]
# that are not 16-byte aligned (feat + M = 49)
CONFIGS = {"small4": widths(SMALL, 12, 36, 44, 33), "blocks": widths(SMALL, 36, 68, 100, 70), "reference": dict(REFERENCE),
           "widest": widths(SMALL, 64, 256, 256, 256, feat=256), "small4u": widths(SMALL, 12, 36, 44, 33, feat=41)}
ROWS = [(1, 1), (3, 17), (2, 33), (2, 64), (2, 65), (2, 130)]
CASES = [(name, N, S) for name in ("small4", "blocks") for N, S in ROWS] + [("reference", 3, 65), ("widest", 1, 65)]
UNALIGNED = ("small4u", 2, 65)


@functools.lru_cache(maxsize=None)
def case(name, N, S):
    """-> W, obs, sf and the CPU form's result: computed once and shared (treat as read-only)."""
    cfg = CONFIGS[name]
    rng = np.random.default_rng([sorted(CONFIGS).index(name), N, S])
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, N, S, cfg["L"], cfg["feat"])
    return W, obs, sf, embed_cpu(obs, sf, W)


def layers_np(W, obs, sf):
    """The three per-row layers of the definition with their inputs, as replay._embed_cpu runs them:
    -> [(name, start [N, S, J] or [J], weights [J, K], input [N, S, K])] for e2, h (before leaky) and x (before the mask)."""
    w = weights_of(W)
    N, S, L, F_, M = obs.shape[0], (obs.shape[1] - 9 - W["L"] ** 2) // 5, W["L"], w.feat, w.map_feat
    leaky = lambda s: np.where(s > 0, s, f32(W["slope"]) * s).astype(f32)  # noqa: E731
    with np.errstate(all="ignore"):
        rows = obs[:, :5 * S].reshape(N, S, 5)
        fmap = replay._height_map_np(obs[:, 5 * S + 9:5 * S + 9 + L * L].reshape(N, 1, L, L), w, leaky)
        base = np.broadcast_to(W["b_p1"], (N, w.proj_hidden)).astype(f32)
        base = replay._chain_np(replay._chain_np(base, W["w_p1"][:, :F_], sf), W["w_p1"][:, F_:F_ + M], fmap)
        e1 = leaky(replay._lin_np(W["w_c1"], W["b_c1"], rows[:, :, :4]))
        e2 = replay._lin_np(W["w_c2"], W["b_c2"], e1)
        start_h = np.broadcast_to(base[:, None, :], (N, S, w.proj_hidden)).astype(f32)
        h = leaky(replay._chain_np(start_h, W["w_p1"][:, F_ + M:], e2))
    return [("e2", np.broadcast_to(W["b_c2"], e2.shape).astype(f32), W["w_c2"], e1), ("h", start_h, W["w_p1"][:, F_ + M:], e2),
            ("x", np.broadcast_to(W["b_p2"], (N, S, w.embed)).astype(f32), W["w_p2"], h)]


def moved_by_descending_order(W, obs, sf):
    """Per layer, the number of output elements of valid rows in which the chain summed with k DESCENDING differs from the
    definition's, and the number of such elements."""
    S = (obs.shape[1] - 9 - W["L"] ** 2) // 5
    valid = obs[:, :5 * S].reshape(obs.shape[0], S, 5)[:, :, 4] == 1
    res = {}
    with np.errstate(all="ignore"):
        for name, start, w, x in layers_np(W, obs, sf):
            up = replay._chain_np(start, w, x)[valid]
            down = replay._chain_np(start, w[:, ::-1], x[..., ::-1])[valid]
            res[name] = int((up.view(np.uint32) != down.view(np.uint32)).sum()), up.size
    return res


# ------------------------------------------------------------------ the wrapper's argument rules ------------
def test_forms_are_named():
    assert replay.EMBED_FORMS == ("chain", "mfma") and replay.EMBED_HIP_DEFAULT is False


def test_an_unknown_form_is_refused():
    W, obs, sf, _ = case("small4", 1, 1)
    with pytest.raises(ValueError, match="form"):
        replay.embed(torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W), form="matrix")
    with pytest.raises(ValueError, match="form"):
        replay.embed(torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W), use_hip=False, form="")


@pytest.mark.parametrize("bad", [dict(cand_hidden=7), dict(cand_embed=34), dict(proj_hidden=45)], ids=ids)
def test_mfma_with_a_width_that_is_no_multiple_of_four_is_refused(bad):
    rng = np.random.default_rng(3)
    cfg = dict(CONFIGS["small4"], **bad)
    W = make_layers(rng, **cfg)
    obs, sf = make_obs(rng, 2, 3, cfg["L"], cfg["feat"])
    t_obs, t_sf, w = torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W)
    with pytest.raises(ValueError, match="multiples of 4"):
        replay.embed(t_obs, t_sf, w, form="mfma")
    x, _ = replay.embed(t_obs, t_sf, w, form="chain")        # the chain form takes them
    assert x.shape == (2, 3, cfg["embed"])


def test_the_form_changes_nothing_on_cpu_tensors():
    W, obs, sf, (want_x, want_xg) = case("small4", 3, 17)
    t_obs, t_sf, w = torch.from_numpy(obs), torch.from_numpy(sf), weights_of(W)
    for use_hip in (None, False):
        x, xg = replay.embed(t_obs, t_sf, w, use_hip=use_hip, form="mfma")
        same_bits(x.numpy(), want_x)
        same_bits(xg.numpy(), want_xg)
    with pytest.raises(RuntimeError):
        replay.embed(t_obs, t_sf, w, use_hip=True, form="mfma")              # no HIP device holds these tensors


def test_network_greedy_action_hands_the_form_on():
    import inspect
    p = inspect.signature(replay.network_greedy_action).parameters
    assert p["embed_form"].default == "chain" and p["streams_form"].default == "chain"
    assert inspect.signature(replay.embed).parameters["form"].default == "chain"


# ------------------------------------------------------------------ limits of the entry point ------------
def abi_call(lib, name="irbpp_embed_mfma", **kw):
    """test_embed_cpu.abi_call for either entry point: the same defaults (every width a multiple of 4)."""
    d = dict(w=dict(), map_len=8, c1=2, c2=2, c3=1, feat=4, cand_hidden=4, cand_embed=4, proj_hidden=8, embed=8, slope=0.01, obs=PTR,
             obs_stride=5 * 3 + 9 + 64, sf=PTR, feat_stride=4, s_rows=3, n_env=1, base=PTR, x=PTR, env_stride=24, row_stride=8, xg=PTR,
             xg_stride=8, no_struct=False)
    d.update(kw)
    ptrs = {n: PTR.value for n in NAMES}
    ptrs.update(d["w"])
    ws = replay._IrbppEmbedWeights(*(ptrs[n] for n in NAMES), *(d[n] for n in replay._EMBED_SIZES), d["slope"])
    return getattr(lib, name)(None if d["no_struct"] else C.byref(ws), d["obs"], d["obs_stride"], d["sf"], d["feat_stride"], d["s_rows"],
                              d["n_env"], d["base"], d["x"], d["env_stride"], d["row_stride"], d["xg"], d["xg_stride"], None)


@pytest.mark.parametrize("bad", BAD, ids=ids)
def test_irbpp_embed_mfma_rejects_what_irbpp_embed_rejects(lib, bad):
    assert abi_call(lib, **bad) == -1                       # IRBPP_ERR_ARG before any HIP call


@pytest.mark.parametrize("bad", [dict(cand_hidden=6), dict(cand_embed=6), dict(proj_hidden=6), dict(cand_hidden=1), dict(proj_hidden=255)],
                         ids=ids)
def test_irbpp_embed_mfma_rejects_widths_that_are_no_multiple_of_four(lib, bad):
    assert abi_call(lib, **bad) == -1
