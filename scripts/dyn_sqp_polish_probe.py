"""The fp32 single-track kernel (dyn_sqp) on the row-family cases of tests/row_family_cases.py, under other
polish settings (needs an MI355X): per case the scaled |u* - u*_oracle|, status and diag flags (bit 1 every QP
converged, bit 2 every QP polish-certified, bits 4.. the number of certified QPs) for qp.polish 3 / 6 / 12 /
40 / 0 and tighter qp.tol, with 1 and 2 SQP iterations against the oracle stopped at the same count (first QP's
active rows and multipliers), and through st_sqp_kernel<40> in fp64 with the same parameters; then the
delta_max cases' x* against the bound, stage by stage; then the kernel's time on the C3 batch
(dynamic_batch(4096, seed 31), host pointers, 10 solves after 3) with qp.polish = 3 and 12.

    python scripts/dyn_sqp_polish_probe.py > profiles/row_families/dyn_sqp_polish_probe.log
"""
import copy
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vehicle-control_amd"), os.path.join(ROOT, "tests")]
warnings.filterwarnings("ignore")
import numpy as np
import row_family_cases as R
from oracle import dyn_sqp as D, models as M
from vcmpc import Context, _abi
from vcmpc.config import make_params

def run(case, tyre, qp=None, dtype=_abi.VC_F32):
    cfgs = copy.deepcopy(case["cfgs"])
    cfgs["mpc"]["qp"] = dict(cfgs["mpc"]["qp"], **(qp or {}))
    p = make_params(dyn_car=cfgs["car"], dyn_mpc=cfgs["mpc"], tyre=tyre)
    f = np.float32 if dtype == _abi.VC_F32 else np.float64
    a = {k: np.ascontiguousarray(v, f) for k, v in case["d"].items()}
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=40, max_batch=1, dtype=dtype, params=p) as c:
        r = c.solve(a["x0"], a["kappa"], a["ds"], a["ubar"].copy(), diag=True)
    return r, cfgs

def oracle(case, cfgs, tyre):
    d = case["d"]
    return D.dyn_sqp_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], M.dyn_params_from_config(cfgs["car"]), D.dyn_weights(cfgs["mpc"]), tyre)

S = np.array([1000.0, 1.0])
for fam, tyre in (("peng", "linear"), ("delta_max", "linear"), ("delta_max", "fiala"), ("tyre_f_up", "linear"), ("Ux_min", "linear")):
    case = R.st_case(fam, tyre, "dyn_sqp")
    print(f"== {fam} {tyre}", flush=True)
    for qp in ({"polish": 3}, {"polish": 6}, {"polish": 12}, {"polish": 40}, {"polish": 0}, {"tol": 1e-6}, {"tol": 1e-6, "polish": 12}, {"max_iter": 200, "tol": 3e-7, "polish": 0}):
        (u0, xs, us, st, it, dg), cfgs = run(case, tyre, qp)
        e = np.abs((us.astype(np.float64) - case["ref"]["u_star"]) / S)
        print(f"  fp32 {qp}: err_u {e.max():.3e} (Fx {e[..., 0].max():.3e} at k={e[0, :, 0].argmax()}, w {e[..., 1].max():.3e}), status {st.tolist()}, it {it.tolist()}, "
              f"diag res {dg[0, 0]:.2e} mu {dg[0, 1]:.2e} flags {int(dg[0, 2])} (polished QPs {int(dg[0, 2]) >> 4}) itmax {dg[0, 3]:.0f}", flush=True)
    for n_it in (1, 2):
        (u0, xs, us, st, it, dg), cfgs = run(case, tyre, {"sqp_iters": n_it})
        ref = oracle(case, cfgs, tyre)
        e = np.abs((us.astype(np.float64) - ref["u_star"]) / S)
        print(f"  fp32 sqp_iters={n_it}: err_u {e.max():.3e} (Fx {e[..., 0].max():.3e}, w {e[..., 1].max():.3e}) flags {int(dg[0, 2])}", flush=True)
        if n_it == 1:
            print("    Fx err by stage:", np.array2string(e[0, :, 0], precision=1, max_line_width=250))
            print("    w  err by stage:", np.array2string(e[0, :, 1], precision=1, max_line_width=250))
            lam = ref["hist"][0]["lam"][0]; fams = np.array([f for f, _ in ref["hist"][0]["rows"]]); stg = np.array([k for _, k in ref["hist"][0]["rows"]])
            for f in np.unique(fams[lam > 1e-6]):
                m = (fams == f) & (lam > 1e-6)
                print(f"    oracle QP0 {f}: stages {stg[m].tolist()} lam {np.array2string(lam[m], precision=2, max_line_width=250)}")
    (u0, xs, us, st, it, dg), cfgs = run(case, tyre, {}, _abi.VC_F64)
    e = np.abs((us - case["ref"]["u_star"]) / S)
    print(f"  fp64 st_sqp N=40 same config: err_u {e.max():.3e}, status {st.tolist()}", flush=True)

np.set_printoptions(linewidth=250, precision=2)
for tyre in ("linear", "fiala"):
    case = R.st_case("delta_max", tyre, "dyn_sqp")
    (u0, xs, us, st, it, dg), _ = run(case, tyre)
    ref = case["ref"]
    print(tyre, "flags", int(dg[0, 2]), "err", np.abs((us - ref["u_star"]) / case["scale"]).max())
    print(" kernel delta - 0.02:", (xs[0, :, 3].astype(np.float64) - 0.02))
    print(" oracle delta - 0.02:", ref["x_star"][0, :, 3] - 0.02)
    print(" w err:", us[0, :, 1] - ref["u_star"][0, :, 1])
    print(" oracle last QP lam delta_max:", [(k, round(float(l), 3)) for (f, k), l in zip(ref["hist"][-1]["rows"], ref["hist"][-1]["lam"][0]) if f == "delta_max" and l > 1e-6][:4], "...")
    print(" oracle QP slack of delta_max rows, last QP:", np.array([s for (f, k), s in zip(ref["hist"][-1]["rows"], ref["hist"][-1]["slack"][0]) if f == "delta_max"]))

import time
from vcmpc.config import load_config
from vcmpc.workload import dynamic_batch
d = dynamic_batch(4096, seed=31)
for polish in (3, 12):
    cfg = load_config("dynamic_mpc")
    cfg["qp"] = dict(cfg["qp"], polish=polish)
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=cfg, tyre="linear")
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=40, max_batch=4096, dtype=_abi.VC_F32, params=p) as c:
        ts = []
        for rep in range(13):
            t0 = time.perf_counter()
            r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
            ts.append(time.perf_counter() - t0)
    flags = r[5][:, 2].astype(int)
    print(f"C3 batch, qp.polish = {polish}: {1e3 * np.median(ts[3:]):.2f} ms per solve (median of 10, host pointers, copies included), "
          f"solved {(r[3] == 0).mean():.4f}, every QP certified on {((flags & 4) > 0).mean():.4f} of the problems")
