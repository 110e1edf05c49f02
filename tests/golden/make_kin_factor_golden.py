"""Generate tests/golden/kin_factor_golden.npz: what the fused kinematic kernel (kin_ltv.hip)
returns on the problems that lean hardest on the blocked factorisation's outputs -- the factor's
row registers (zero on and above the diagonal) and its stored columns -- recorded from the library
built at the commit BEFORE the factorisation's lane-set bookkeeping moved to the scalar unit
(DESIGN 3.1, round 8).  That change performs the same floating-point operations in the same order,
so tests/test_gpu_kin_factor.py asks for bit-identical u*, u0, iterations and status.

Runs (the kernel exists for N = 20 only, and the lane sets do not depend on the batch size):
  (no prefix)  rows HARD of kinematic_batch(1024, N=20, seed=31) as one batch of 9, shipped settings:
               153, 260, 441, 532, 855 (failed early polish attempts, several polish rounds with
               rank-one updates and a drop) and 677, 689, 706, 868 (11 interior-point iterations)
  p0_          the same 9 rows with qp.polish = 0
  cf_          kinematic_batch(70, N=20, seed=31) with qp.tol lowered until the interior point
               leaves through the loss-of-definiteness exit (factor_blocked returns false:
               diag[2]'s lowest bit) on at least one problem with every output finite; recorded
               only if a tolerance of TOL_SCAN gets there (cf_tol is the one used)

Needs an MI355X and the library to record from (VCMPC_LIB selects it).  Run from the repo root:
    VCMPC_LIB=/path/to/parent/libvcmpc.so python tests/golden/make_kin_factor_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vehicle-control_amd"))

N, SEED = 20, 31
HARD = [153, 260, 441, 532, 855, 677, 689, 706, 868]
B_CF = 70
TOL_SCAN = [1e-11, 1e-12, 1e-13, 1e-14, 1e-15, 1e-16]  # shipped: 1e-10
KEYS = ("u0", "x_star", "u_star", "status", "iters", "diag")


def hard_batch():
    from vcmpc.workload import kinematic_batch
    d = kinematic_batch(1024, N=N, seed=SEED)
    return {k: np.ascontiguousarray(v[HARD]) for k, v in d.items()}


def run(d, cfg):
    from vcmpc import Context
    from vcmpc.config import load_config
    B = len(d["x0"])
    with Context(N=N, max_batch=B, kin_car=load_config("kinematic_car"), kin_mpc=cfg) as c:
        u0, x, u, st, it, dg = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
    return dict(u0=u0, x_star=x, u_star=u, status=st, iters=it, diag=dg)


def with_qp(cfg, **kw):
    return dict(cfg, qp=dict(cfg["qp"], **kw))


def chol_failed(diag):
    return (diag[:, 2].astype(np.int64) & 1) != 0


def main():
    from vcmpc.config import load_config
    from vcmpc.workload import kinematic_batch
    cfg = load_config("kinematic_mpc")
    out = {}
    d = hard_batch()
    for pre, c in (("", cfg), ("p0_", with_qp(cfg, polish=0))):
        r = run(d, c)
        print(pre or "base", "status", r["status"], "iters", r["iters"], "rounds", r["diag"][:, 3],
              "flags", r["diag"][:, 2])
        out.update({pre + k: v for k, v in r.items()})
    # the case must keep covering what it is for
    assert (out["status"] == 0).all()
    assert out["diag"][:, 3].max() >= 3, "no problem with three polish rounds"
    assert (out["iters"] == 11).any(), "no 11-iteration interior point"
    d70 = kinematic_batch(B_CF, N=N, seed=SEED)
    for tol in TOL_SCAN:
        r = run(d70, with_qp(cfg, tol=tol))
        cf = chol_failed(r["diag"])
        fin = all(np.isfinite(r[k]).all() for k in KEYS)
        print(f"tol {tol:g}: loss-of-definiteness exits {int(cf.sum())}, outputs finite {fin}, "
              f"status {np.unique(r['status'], return_counts=True)}, iters max {r['iters'].max()}")
        if cf.any() and fin:
            out.update({"cf_" + k: v for k, v in r.items()})
            out["cf_tol"] = np.float64(tol)
            break
    else:
        print("no tolerance of the scan reaches the loss-of-definiteness exit: cf_ case not recorded")
    np.savez_compressed(os.path.join(HERE, "kin_factor_golden.npz"), **out)


if __name__ == "__main__":
    main()
