"""Generate tests/golden/kin_shadow_golden.npz: what the fused kinematic kernel (kin_ltv.hip) returns
on the paths that the existing goldens do not run, recorded from the library built at the commit
BEFORE round 10 reordered the interior-point iteration (the panels' tiles
transposed in one LDS round trip, the passes' fused multiply-adds spelled out; the round also tried
the predictor's right-hand side in the shadow of the normal matrix's MFMAs, which these cases were
chosen for and which was left out).  That change performs the same floating-point operations in the
same order on every value that reaches u*, so tests/test_gpu_kin_shadow.py asks for bit-identical u*,
u0, iterations, status, solver flags and polish rounds.

Runs (the kernel exists for N = 20 only, and nothing here depends on the batch size):
  a_   kinematic_batch(70, N=20, seed=31), shipped settings
  b_   the same batch with qp.max_iter = MAX_ITER_LOW: most problems leave through the iteration
       limit, right after a step
  c_   the same batch with x0 of row NAN_ROW made NaN: that row is VC_NONFINITE (no interior point at
       all), the others are as in a_
  d_   the obstacle golden's problems (obs_golden.npz) with its obstacles set through set_obstacles on
       a context created without any
  e_   row 260 of kinematic_batch(1024, N=20, seed=31) alone (B = 1): its early polish attempt fails and
       the interior point resumes -- it factors again after a polish that used the broadcast
       vectors and the transposes' buffers

Needs an MI355X and the library to record from (VCMPC_LIB selects it).  Run from the repo root:
    VCMPC_LIB=/path/to/parent/libvcmpc.so python tests/golden/make_kin_shadow_golden.py
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
B_SMALL = 70
MAX_ITER_LOW = 4   # shipped: see config/kinematic_mpc.yaml; the C2 interior points take 7..11
NAN_ROW = 37
RESUMED = 260      # row of kinematic_batch(1024, N=20, seed=31)
VC_SOLVED, VC_MAX_ITER, VC_NONFINITE = 0, 1, 2
KEYS = ("u0", "x_star", "u_star", "status", "iters", "diag")


def run(d, cfg, obstacles=None):
    from vcmpc import Context
    from vcmpc.config import load_config
    B = len(d["x0"])
    with Context(N=N, max_batch=B, kin_car=load_config("kinematic_car"), kin_mpc=cfg) as c:
        if obstacles is not None:
            c.set_obstacles(obstacles)
        u0, x, u, st, it, dg = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
    return dict(u0=u0, x_star=x, u_star=u, status=st, iters=it, diag=dg)


def with_qp(cfg, **kw):
    return dict(cfg, qp=dict(cfg["qp"], **kw))


def nan_row_batch(d):
    d = {k: v.copy() for k, v in d.items()}
    d["x0"][NAN_ROW] = np.nan
    return d


def obstacle_case():
    g = dict(np.load(os.path.join(HERE, "obs_golden.npz")))
    d = {"x0": g["kin_x0"], "kappa": g["kin_kappa"], "ds": g["kin_ds"], "ubar": g["kin_ubar"]}
    return d, [tuple(float(v) for v in o) for o in g["obstacles"]]


def resumed_case():
    from vcmpc.workload import kinematic_batch
    d = kinematic_batch(1024, N=N, seed=SEED)
    return {k: np.ascontiguousarray(v[RESUMED:RESUMED + 1]) for k, v in d.items()}


def main():
    from vcmpc.config import load_config
    from vcmpc.workload import kinematic_batch
    cfg = load_config("kinematic_mpc")
    out = {}
    d70 = kinematic_batch(B_SMALL, N=N, seed=SEED)

    a = run(d70, cfg)
    print("a: status", np.unique(a["status"], return_counts=True), "iters", a["iters"].min(), a["iters"].max())
    assert (a["status"] == VC_SOLVED).all()
    out.update({"a_" + k: v for k, v in a.items()})

    b = run(d70, with_qp(cfg, max_iter=MAX_ITER_LOW))
    print("b: status", np.unique(b["status"], return_counts=True), "iters", b["iters"].min(), b["iters"].max())
    assert MAX_ITER_LOW < cfg["qp"]["max_iter"]
    assert (b["status"] == VC_MAX_ITER).mean() > 0.5, "most problems must leave through the iteration limit"
    assert (b["iters"][b["status"] == VC_MAX_ITER] == MAX_ITER_LOW).all()
    out.update({"b_" + k: v for k, v in b.items()})

    c = run(nan_row_batch(d70), cfg)
    others = np.arange(B_SMALL) != NAN_ROW
    print("c: status of the NaN row", c["status"][NAN_ROW])
    assert c["status"][NAN_ROW] == VC_NONFINITE and (c["status"][others] == VC_SOLVED).all()
    for k in ("u0", "u_star", "iters", "status"):
        assert np.array_equal(c[k][others], a[k][others]), k
    out.update({"c_" + k: v for k, v in c.items()})

    dobs, obstacles = obstacle_case()
    off = run(dobs, cfg)
    on = run(dobs, cfg, obstacles)
    print("d: status", np.unique(on["status"], return_counts=True), "max |u*_on - u*_off|",
          np.abs(on["u_star"] - off["u_star"]).max())
    assert np.abs(on["u_star"] - off["u_star"]).max() > 1e-3, "the obstacle terms must change the answer"
    out.update({"d_" + k: v for k, v in on.items()})

    e = run(resumed_case(), cfg)
    print("e: status", e["status"], "iters", e["iters"], "flags", e["diag"][:, 2], "rounds", e["diag"][:, 3])
    # more polish rounds than one attempt's early cap (KIN_EARLY_ROUNDS = 2): the early attempt
    # failed, the interior point resumed and the final attempt certified
    assert e["status"][0] == VC_SOLVED and e["diag"][0, 3] >= 3 and (int(e["diag"][0, 2]) & 4)
    out.update({"e_" + k: v for k, v in e.items()})

    np.savez_compressed(os.path.join(HERE, "kin_shadow_golden.npz"), **out)


if __name__ == "__main__":
    main()
