"""Cost and payoff of the in-kernel infeasibility detection (vc_set_infeasibility):
kernel time (HIP events on the context stream) and iteration counts of one context with the
detection on and off, the two settings interleaved round by round in one process.

  feasible   the batch of bench.py's kinematic_n50 leg (B = 1024, N = 50, seed 31 + 50, qp.solver = 1):
             every problem feasible, so `on` pays for the two wave sums per iteration and whatever
             sweeps d'lam < 0 starts
  p50        the test set P(50) of tests/test_gpu_infeasible.py (48 problems, delta box +-0.05,
             trust 1.0 / 0.1, max_iter 80), and the same set tiled to 1536 problems (a launch that
             fills the device): the infeasible problems stop at their certificate instead of max_iter

usage: python scripts/infeasible_cost.py [--rounds R]     (prints one JSON line per workload)"""
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
        res[key] = {"kernel_ms_median": float(np.median(ms[on])), "kernel_ms_min": float(np.min(ms[on])),
                    "kernel_ms_max": float(np.max(ms[on])), "status_counts": np.bincount(s, minlength=5).tolist(),
                    "iters_mean": float(i.mean()), "iters_max": int(i.max())}
        if inf.any():
            res[key]["iters_mean_infeasible"] = float(i[inf].mean())
            res[key]["iters_max_infeasible"] = int(i[inf].max())
    res["on_over_off_median"] = res["on"]["kernel_ms_median"] / res["off"]["kernel_ms_median"]
    res["solved_u_bit_identical"] = bool(np.array_equal(out[True][2][~inf], out[False][2][~inf]))
    res["solved_iters_equal"] = bool(np.array_equal(out[True][1][~inf], out[False][1][~inf]))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    from vcmpc.config import load_config
    from vcmpc.workload import kinematic_batch
    cfg = load_config("kinematic_mpc")
    cfg["qp"] = dict(cfg.get("qp") or {}, solver=1)
    measure("feasible: kinematic_n50 leg batch", kinematic_batch(1024, N=50, seed=31 + 50), cfg, a.rounds)
    cfg = load_config("kinematic_mpc")
    cfg["qp"] = dict(cfg.get("qp") or {}, solver=1, trust_a=1.0, trust_w=0.1, max_iter=80)
    cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
    d = kinematic_batch(48, N=50, seed=77)
    measure("P(50)", d, cfg, a.rounds)
    measure("P(50) tiled x32", {k: np.concatenate([v] * 32) for k, v in d.items()}, cfg, a.rounds)


if __name__ == "__main__":
    main()
