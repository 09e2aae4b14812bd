"""CPU side of the cell step (irbpp_step_cells / irbpp_heuristic_step): the two entry points are declared and bound with the same
arity, and the oracle helper the GPU tests compare against (cell_step_helpers.OracleCellEnv) is deterministic and reaches the
conditions those tests rely on -- the heuristic's cell is often NOT one of the valid candidate rows (so irbpp_step could not have
played it), episodes end, and the all-invalid case (np.sum(naiveMask) == 0 -> argmin (0, 0, 0) -> refusal) occurs."""
import os
import re

import numpy as np
import pytest

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib, synthetic
from cell_step_helpers import OracleCellEnv, mix_cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "irbpp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/irbpp.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("irbpp_step_cells", 5), ("irbpp_heuristic_step", 6)])
def test_entry_points_declared_and_bound(name, arity):
    assert _header_arity(name) == arity
    assert name in _lib.SIGNATURES, f"{name} is not bound in irbpp_amd/_lib.py"
    assert len(_lib.SIGNATURES[name][1]) == arity
    # same outputs as irbpp_step: the irbpp_step_out pointer sits in front of the stream
    assert _lib.SIGNATURES[name][1][-2:] == _lib.SIGNATURES["irbpp_step"][1][-2:]


def test_python_surface_has_the_calls():
    from irbpp_amd import evaluate, vec_env
    import inspect
    for cls in (vec_env.GpuPackingEnv, vec_env.GroupedPackingEnv):
        assert hasattr(cls, "step_cells") and hasattr(cls, "heuristic_step")
    assert hasattr(vec_env.GroupedPackingEnv, "step_cells_group") and hasattr(vec_env.GroupedPackingEnv, "heuristic_step_group")
    assert hasattr(vec_env.GpuVecEnv, "step_cells")
    assert "heuristic" in inspect.signature(evaluate.evaluate).parameters


def _run(shapes, seqs, bins, steps, method, dir_idx, **kw):
    env = OracleCellEnv(range(bins), bins, shapes, seqs, **kw)
    obs = [env.reset()]
    cells_played, dones = [], []
    for _ in range(steps):
        cells = env.heuristic_cells(method, dir_idx)
        o, r, d, _ = env.step_cells(cells)
        obs.append(o)
        cells_played.append(cells)
        dones.append(d)
    return env, np.array(obs), np.array(cells_played), np.array(dones)


@pytest.mark.parametrize("method", ["MINZ", "DBLF", "FIRSTFIT", "HM"])
def test_blockout_heuristic_cells_leave_the_candidate_rows(method):
    """BlockOut shapes, 3 bins, 60 placements each, flip 0: in every method's run the chosen cell is absent from the valid
    candidate rows at least once (measured: 7 of 180 for MINZ at the lowest)."""
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.04, seed=0)
    seqs = synthetic.make_sequences(24, 32, 120, seed=5)
    env, _, _, _ = _run(sh, seqs, 3, 60, method, 0)
    assert env.in_rows + env.off_rows == 180
    assert env.off_rows >= 1, (method, env.off_rows)


@pytest.mark.parametrize("method,dir_idx,episodes", [("DBLF", 3, 6), ("MINZ", 1, 5)])
def test_free_form_runs_end_episodes_and_meet_the_all_invalid_case(method, dir_idx, episodes):
    sh = synthetic.general_shapes(n_shapes=16, n_rot=4, fmin=4, fmax=14, seed=3)
    seqs = synthetic.make_sequences(16, 32, 80, seed=2)
    env, obs, cells, dones = _run(sh, seqs, 3, 40, method, dir_idx)
    assert env.episodes == episodes and env.episodes >= 2
    assert env.off_rows >= 1 and env.all_invalid >= 1, (env.off_rows, env.all_invalid)
    # deterministic: a second run gives the same cells, observations and dones
    env2, obs2, cells2, dones2 = _run(sh, seqs, 3, 40, method, dir_idx)
    np.testing.assert_array_equal(cells, cells2)
    np.testing.assert_array_equal(obs, obs2)
    np.testing.assert_array_equal(dones, dones2)
    # an all-invalid placement chose (0, 0, 0) and was refused
    assert (cells[dones] == 0).all(axis=1).any()


def test_drawn_cells_reach_refusals_and_cells_outside_the_mask():
    """The every-fifth-placement uniform draw of the GPU comparison: it meets cells outside naiveMask and ends episodes."""
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    seqs = synthetic.make_sequences(24, 32, 120, seed=5)
    env = OracleCellEnv(range(3), 3, sh, seqs)
    env.reset()
    rng = np.random.RandomState(7)
    for t in range(20):
        env.step_cells(mix_cells(env.heuristic_cells("DBLF", 0), t, rng, 4, 16, 16))
    assert env.outside_mask >= 1 and env.episodes >= 1, (env.outside_mask, env.episodes)
