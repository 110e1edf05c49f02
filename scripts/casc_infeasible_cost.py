"""Cost and payoff of the in-kernel infeasibility detection of the cascaded SQP
(vc_set_casc_infeasibility): kernel time (HIP events on the context stream) and
iteration counts of one context with the detection on and off, the two settings interleaved round
by round in one process.

  feasible   the batch of bench.py's cascaded leg (B = 4096, N = 20 + M = 40, seed 31,
             cascaded_mpc.yaml): `on` pays for the wave sums per interior-point iteration and
             whatever sweeps d'lam < 0 starts
  pv40       the test set PV(40) of tests/test_gpu_casc_infeasible.py (32 problems,
             state_pm_constraints.V_min = 14), and the same set tiled to 1536 problems: the
             infeasible problems stop at their certificate instead of applying a diverged iterate
             and going on

usage: python scripts/casc_infeasible_cost.py [--rounds R]     (prints one JSON line per workload)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vehicle-control_amd"))


def measure(name, data, cfg, rounds):
    import torch
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    dev = torch.device("cuda:0")
    B, H = data["ubar"].shape[:2]
    N = int(cfg["horizon"])
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev) for k, v in data.items()}
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=cfg, tyre="fiala")
    stream = torch.cuda.Stream(dev)
    xbar = torch.empty((B, H, 8), dtype=torch.float64, device=dev)
    u0 = torch.empty((B, 2), dtype=torch.float64, device=dev)
    u_out = torch.empty_like(t["ubar"])
    st = torch.empty((B,), dtype=torch.int32, device=dev)
    it = torch.empty((B,), dtype=torch.int32, device=dev)
    ms = {False: [], True: []}
    out = {}
    with Context(model=_abi.VC_MODEL_CASCADED, N=N, max_batch=B, dtype=_abi.VC_F64, params=p) as c:
        c.set_stream(stream.cuda_stream)
        for r in range(rounds + 2):  # two warm-up rounds
            for on in (False, True):
                c.set_casc_infeasibility(on)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                c.solve_from(t["x0"], t["kappa"], t["ds"], t["ubar"], u_out, xbar, u0, st, it)
                e1.record(stream)
                torch.cuda.synchronize(dev)
                if r >= 2:
                    ms[on].append(e0.elapsed_time(e1))
                out[on] = (st.cpu().numpy().copy(), it.cpu().numpy().copy(), u_out.cpu().numpy().copy())
                if on:
                    qi = c.casc_farkas()[1].cpu().numpy()
    res = {"workload": name, "B": B, "N": N, "M": H - N, "rounds": rounds}
    cert = qi >= 0
    inf = out[True][0] == _abi.VC_INFEASIBLE
    for on, key in ((False, "off"), (True, "on")):
        s, i, _ = out[on]
        res[key] = {"kernel_ms_median": float(np.median(ms[on])), "kernel_ms_min": float(np.min(ms[on])),
                    "kernel_ms_max": float(np.max(ms[on])), "status_counts": np.bincount(s, minlength=5).tolist(),
                    "iters_mean": float(i.mean()), "iters_max": int(i.max())}
        if cert.any():
            res[key]["iters_mean_certified"] = float(i[cert].mean())
            res[key]["iters_max_certified"] = int(i[cert].max())
    res["certified"] = int(cert.sum())
    res["qp_index_counts"] = np.bincount(qi[cert], minlength=1).tolist()
    res["on_over_off_median"] = res["on"]["kernel_ms_median"] / res["off"]["kernel_ms_median"]
    res["rest_u_bit_identical"] = bool(np.array_equal(out[True][2][~inf], out[False][2][~inf]))
    res["rest_status_equal"] = bool(np.array_equal(out[True][0][~inf], out[False][0][~inf]))
    res["uncertified_iters_equal"] = bool(np.array_equal(out[True][1][~cert], out[False][1][~cert]))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    from vcmpc.config import load_config
    from vcmpc.workload import cascaded_batch
    measure("feasible: cascaded leg batch", cascaded_batch(4096, seed=31), load_config("cascaded_mpc"), a.rounds)
    cfg = load_config("cascaded_mpc")
    cfg["state_pm_constraints"] = dict(cfg["state_pm_constraints"], V_min=14)
    d = cascaded_batch(32, M=40, seed=77)
    measure("PV(40)", d, cfg, a.rounds)
    measure("PV(40) tiled x48", {k: np.concatenate([v] * 48) for k, v in d.items()}, cfg, a.rounds)


if __name__ == "__main__":
    main()
