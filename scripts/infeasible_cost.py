"""Cost and payoff of the in-kernel infeasibility detection (vc_set_infeasibility):
kernel time (HIP events on the context stream) and iteration counts of the settings of one workload,
interleaved round by round in one process.

Stagewise kernel (kin_ric.hip, qp.solver = 1), settings off / on:
  feasible   the batch of bench.py's kinematic_n50 leg (B = 1024, N = 50, seed 31 + 50):
             every problem feasible, so `on` pays for the two wave sums per iteration and whatever
             sweeps d'lam < 0 starts
  p50        the test set P(50) of tests/test_gpu_infeasible.py (48 problems, delta box +-0.05,
             trust 1.0 / 0.1, max_iter 80), and the same set tiled to 1536 problems (a launch that
             fills the device): the infeasible problems stop at their certificate instead of max_iter

Condensed kernel (kin_ltv.hip, N = 20; --condensed), settings condensed_off (qp.solver = 2, detection
off: kin_ltv_kernel<20, false>), condensed_on (qp.solver = 2, detection on: kin_ltv_kernel<20, true>)
and stagewise_on (qp.solver = 0, detection on: the default routing, kin_ric_kernel<20, true>), with
stagewise_off (qp.solver = 1, detection off) beside them:
  c2         the batch of bench.py's C2 leg (B = 1024, seed 31, default config): every problem feasible
  p20        the test set P(20) of tests/test_gpu_kin_ltv_infeasible.py, and the same set tiled x32;
             the largest certificate value d'y + R |C'y|_inf of condensed_on is re-evaluated on the host
             with the oracle's rows

usage: python scripts/infeasible_cost.py [--rounds R] [--condensed | --stagewise]
       (prints one JSON line per workload; default: both groups)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vehicle-control_amd"))
sys.path.insert(0, ROOT)


def _stats(ms, s, i, inf):
    r = {"kernel_ms_median": float(np.median(ms)), "kernel_ms_min": float(np.min(ms)),
         "kernel_ms_max": float(np.max(ms)), "status_counts": np.bincount(s, minlength=5).tolist(),
         "iters_mean": float(i.mean()), "iters_max": int(i.max())}
    if inf.any():
        r["iters_mean_infeasible"] = float(i[inf].mean())
        r["iters_max_infeasible"] = int(i[inf].max())
    return r


def measure(name, data, cfg, rounds):
    import torch
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    dev = torch.device("cuda:0")
    B, N = data["ubar"].shape[:2]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in data.items()}
    p = make_params(kin_car=load_config("kinematic_car"), kin_mpc=cfg)
    stream = torch.cuda.Stream(dev)
    xbar = torch.empty((B, N + 1, 6), dtype=torch.float64, device=dev)
    u0 = torch.empty((B, 2), dtype=torch.float64, device=dev)
    u_out = torch.empty_like(t["ubar"])
    st = torch.empty((B,), dtype=torch.int32, device=dev)
    it = torch.empty((B,), dtype=torch.int32, device=dev)
    ms = {False: [], True: []}
    out = {}
    with Context(model=_abi.VC_MODEL_KINEMATIC, N=N, max_batch=B, params=p) as c:
        c.set_stream(stream.cuda_stream)
        for r in range(rounds + 2):  # two warm-up rounds
            for on in (False, True):
                c.set_infeasibility(on)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                c.solve_from(t["x0"], t["kappa"], t["ds"], t["ubar"], u_out, xbar, u0, st, it)
                e1.record(stream)
                torch.cuda.synchronize(dev)
                if r >= 2:
                    ms[on].append(e0.elapsed_time(e1))
                out[on] = (st.cpu().numpy().copy(), it.cpu().numpy().copy(), u_out.cpu().numpy().copy())
    res = {"workload": name, "B": B, "N": N, "rounds": rounds}
    inf = out[True][0] == _abi.VC_INFEASIBLE
    for on, key in ((False, "off"), (True, "on")):
        s, i, _ = out[on]
        res[key] = _stats(ms[on], s, i, inf)
    res["on_over_off_median"] = res["on"]["kernel_ms_median"] / res["off"]["kernel_ms_median"]
    res["solved_u_bit_identical"] = bool(np.array_equal(out[True][2][~inf], out[False][2][~inf]))
    res["solved_iters_equal"] = bool(np.array_equal(out[True][1][~inf], out[False][1][~inf]))
    print(json.dumps(res), flush=True)


# (stagewise_off, qp.solver = 1 without the detection, is there to tell the stagewise kernel's own time
# from what its detection adds)
SETTINGS = (("condensed_off", 2, False), ("condensed_on", 2, True), ("stagewise_on", 0, True),
            ("stagewise_off", 1, False))


def measure_condensed(name, data, cfg, rounds, rows=None):
    """The settings of an N = 20 workload, one context each (qp.solver is a context parameter), one
    solve of each per round.  rows = (C, d) of the oracle for the untiled problems: the certificates of
    condensed_on are re-evaluated with them."""
    import torch
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    dev = torch.device("cuda:0")
    B, N = data["ubar"].shape[:2]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in data.items()}
    stream = torch.cuda.Stream(dev)
    xbar = torch.empty((B, N + 1, 6), dtype=torch.float64, device=dev)
    u0 = torch.empty((B, 2), dtype=torch.float64, device=dev)
    u_out = torch.empty_like(t["ubar"])
    st = torch.empty((B,), dtype=torch.int32, device=dev)
    it = torch.empty((B,), dtype=torch.int32, device=dev)
    ctx, ms, out = {}, {}, {}
    try:
        for key, solver, on in SETTINGS:
            c = dict(cfg)
            c["qp"] = dict(cfg.get("qp") or {}, solver=solver)
            ctx[key] = Context(model=_abi.VC_MODEL_KINEMATIC, N=N, max_batch=B,
                               params=make_params(kin_car=load_config("kinematic_car"), kin_mpc=c),
                               detect_infeasible=on)
            ctx[key].set_stream(stream.cuda_stream)
            ms[key] = []
        y = None
        for r in range(rounds + 2):  # two warm-up rounds
            for key, _, on in SETTINGS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx[key].solve_from(t["x0"], t["kappa"], t["ds"], t["ubar"], u_out, xbar, u0, st, it)
                e1.record(stream)
                torch.cuda.synchronize(dev)
                if r >= 2:
                    ms[key].append(e0.elapsed_time(e1))
                out[key] = (st.cpu().numpy().copy(), it.cpu().numpy().copy(), u_out.cpu().numpy().copy())
                if key == "condensed_on" and r == rounds + 1:
                    y = ctx[key].farkas()  # copied on the context's stream: wait for it before reading
                    torch.cuda.synchronize(dev)
                    y = y.cpu().numpy()
    finally:
        for c in ctx.values():
            c.close()
    res = {"workload": name, "B": B, "N": N, "rounds": rounds}
    inf = out["condensed_on"][0] == _abi.VC_INFEASIBLE
    for key, _, _ in SETTINGS:
        s, i, _u = out[key]
        res[key] = _stats(ms[key], s, i, inf)
    med = {k: res[k]["kernel_ms_median"] for k in ms}
    res["condensed_on_over_off_median"] = med["condensed_on"] / med["condensed_off"]
    res["condensed_on_over_stagewise_on_median"] = med["condensed_on"] / med["stagewise_on"]
    # the acceptance margin: the slowest condensed_on round against the fastest stagewise_on round
    res["condensed_on_max_below_stagewise_on_min"] = bool(res["condensed_on"]["kernel_ms_max"] <
                                                          res["stagewise_on"]["kernel_ms_min"])
    on, off = out["condensed_on"], out["condensed_off"]
    res["noncertified_u_bit_identical"] = bool(np.array_equal(on[2][~inf], off[2][~inf]))
    res["noncertified_iters_equal"] = bool(np.array_equal(on[1][~inf], off[1][~inf]))
    res["status_equal_to_stagewise_on"] = bool(np.array_equal(on[0], out["stagewise_on"][0]))
    if rows is not None and inf.any():
        C, d = rows
        nb = len(C)
        worst = -np.inf
        for b in np.nonzero(inf)[0]:
            Cb, db, yb = C[b % nb], d[b % nb], y[b]
            box = db[:4 * N].reshape(N, 4)
            R = (np.maximum(box[:, 0], box[:, 1]) + np.maximum(box[:, 2], box[:, 3])).sum()
            worst = max(worst, float(db @ yb + R * np.abs(Cb.T @ yb).max()))
        res["largest_certificate_value"] = worst
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--condensed", action="store_true", help="the condensed workloads only")
    g.add_argument("--stagewise", action="store_true", help="the stagewise workloads only")
    a = ap.parse_args()
    from vcmpc.config import load_config
    from vcmpc.workload import kinematic_batch
    if not a.condensed:
        cfg = load_config("kinematic_mpc")
        cfg["qp"] = dict(cfg.get("qp") or {}, solver=1)
        measure("feasible: kinematic_n50 leg batch", kinematic_batch(1024, N=50, seed=31 + 50), cfg, a.rounds)
        cfg = load_config("kinematic_mpc")
        cfg["qp"] = dict(cfg.get("qp") or {}, solver=1, trust_a=1.0, trust_w=0.1, max_iter=80)
        cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
        d = kinematic_batch(48, N=50, seed=77)
        measure("P(50)", d, cfg, a.rounds)
        measure("P(50) tiled x32", {k: np.concatenate([v] * 32) for k, v in d.items()}, cfg, a.rounds)
    if not a.stagewise:
        from oracle import ltv_qp as Q
        cfg = load_config("kinematic_mpc")
        measure_condensed("feasible: C2 batch", kinematic_batch(1024, N=20, seed=31), cfg, a.rounds)
        cfg = load_config("kinematic_mpc")
        cfg["qp"] = dict(cfg.get("qp") or {}, trust_a=1.0, trust_w=0.1, max_iter=80)
        cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
        d = kinematic_batch(48, N=20, seed=77)
        Qd = Q.kin_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], 2.5, Q.kin_weights(cfg))
        rows = (Qd["C"], Qd["d"])
        measure_condensed("P(20)", d, cfg, a.rounds, rows)
        measure_condensed("P(20) tiled x32", {k: np.concatenate([v] * 32) for k, v in d.items()}, cfg, a.rounds, rows)


if __name__ == "__main__":
    main()
