#!/usr/bin/env python
"""Golden vectors of configurations with more than 31 height levels, played by the REFERENCE'S OWN PackingGame.

Run from the repo root, where make_golden.py runs (its stubs, its kinematic interface, its MINZ policy and its recording loops
are reused as they are; only resolutionZ changes):

    python tests/golden/make_levels_golden.py

resolutionZ = 0.005 on the standard 0.32 x 0.32 x 0.30 m bin is 60 height levels (cvTools.py:78), beyond the 6-bit level
codes of the tuned pipeline: the library plays these configurations on the capacity path (csrc/irbpp_wide.hip).

Outputs (consumed by tests/test_height_levels_cpu.py and tests/test_gpu_height_levels.py):
    online_levels60.npz       online, 16 x 16, free-form solids at R = 4, S = 500 (recorded up to its first tied > S selection)
    hier_levels60_k3.npz      bufferSize = 3, 16 x 16, the small BlockOut set
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

from irbpp_amd import synthetic  # noqa: E402

RES_Z = 0.005
S = 500


def levels_scenario(name):
    """Shape set and sequences of a recording (the tests rebuild them from the same seeds)."""
    if name == "online_levels60":
        sh = synthetic.general_shapes(n_shapes=16, n_rot=4, fmin=4, fmax=14, seed=3)
        return sh, synthetic.make_sequences(sh.n_shapes, 16, 80, seed=2)
    sh = synthetic.blockout_shapes(n_shapes=24, n_rot=4, cube=0.06, seed=0)
    return sh, synthetic.make_sequences(sh.n_shapes, 16, 150, seed=5)


def _with_res_z(fn, *args, **kw):
    """make_golden's recording loops build their PackingGame through mg.make_reference_env: the same, at RES_Z."""
    orig = mg.make_reference_env
    mg.make_reference_env = functools.partial(orig, res_z=RES_Z)
    try:
        return fn(*args, **kw)
    finally:
        mg.make_reference_env = orig


def max_level(obs):
    """Highest level floor(H / resolutionZ) among the valid candidate rows of a stack of observations."""
    rows = np.asarray(obs)[:, :5 * S].reshape(-1, 5)
    h = rows[rows[:, 4] == 1, 3].astype(np.float64)
    return int(np.floor_divide(h, RES_Z).max()) if h.size else -1


def main():
    sh, seq = levels_scenario("online_levels60")
    rec = _with_res_z(mg.run_online, sh, seq, 60, S=S, tap=True)
    print("online_levels60: %d steps, %d episodes ended, highest candidate level %d" % (len(rec["act"]), int(rec["done"].sum()), max_level(rec["obs"])))
    assert max_level(rec["obs"]) > 31
    np.savez_compressed(os.path.join(mg.OUT, "online_levels60.npz"), seq=seq, **rec)

    sh, seq = levels_scenario("hier_levels60_k3")
    rec = _with_res_z(mg.run_hier, sh, seq, 70, 3)
    print("hier_levels60_k3: %d placements, %d episodes ended, highest candidate level %d" % (len(rec["act"]), int(rec["done"].sum()), max_level(rec["loc_obs"])))
    assert max_level(rec["loc_obs"]) > 31
    np.savez_compressed(os.path.join(mg.OUT, "hier_levels60_k3.npz"), seq=seq, **rec)
    for f in ("online_levels60.npz", "hier_levels60_k3.npz"):
        print(f, os.path.getsize(os.path.join(mg.OUT, f)))


if __name__ == "__main__":
    main()
