"""Generate tests/golden/kin_step_golden.npz: what the fused kinematic kernel (kin_ltv.hip)
returns for kinematic_batch(70, seed=31), recorded from the library built at the commit BEFORE
the serial-path restructuring of the rollout and the output sweep.  Such
changes perform the same operations on every value that reaches u*, so tests/test_gpu_kin_step.py
asks for bit-identical u*, iterations and status against these vectors.

Three runs, all on the same 70 problems (B = 70: ragged last XCD group; row 0 is the B = 1 case):
  (no prefix)  shipped settings
  p0_          qp.polish = 0: the interior-point iterate is returned
  nf_          problem NF_ROW's x0[ey] = NaN: that problem is VC_NONFINITE, the rest unchanged

Needs an MI355X and the built library.  Run from the repo root:
    python tests/golden/make_kin_step_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vehicle-control_amd"))

B, N, SEED, NF_ROW = 70, 20, 31, 35


def run(d, cfg):
    from vcmpc import Context
    from vcmpc.config import load_config
    with Context(N=N, max_batch=B, kin_car=load_config("kinematic_car"), kin_mpc=cfg) as c:
        u0, x, u, st, it = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy())
    return dict(u0=u0, x_star=x, u_star=u, status=st, iters=it)


def cases(cfg):
    """(prefix, inputs, config) of the three recorded runs."""
    from vcmpc.workload import kinematic_batch
    d = kinematic_batch(B, N=N, seed=SEED)
    nf = {k: v.copy() for k, v in d.items()}
    nf["x0"][NF_ROW, 3] = np.nan
    p0 = dict(cfg, qp=dict(cfg["qp"], polish=0))
    return [("", d, cfg), ("p0_", d, p0), ("nf_", nf, cfg)]


def main():
    from vcmpc.config import load_config
    out = {}
    for pre, d, cfg in cases(load_config("kinematic_mpc")):
        r = run(d, cfg)
        print(pre or "base", "status", np.unique(r["status"], return_counts=True), "iters max", r["iters"].max())
        out.update({pre + k: v for k, v in r.items()})
    assert (out["status"] == 0).all() and out["nf_status"][NF_ROW] == 2
    np.savez_compressed(os.path.join(HERE, "kin_step_golden.npz"), **out)


if __name__ == "__main__":
    main()
