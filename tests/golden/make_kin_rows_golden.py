"""Generate tests/golden/kin_rows_golden.npz: what the fused kinematic kernel (kin_ltv.hip) returns on
every path that reads the factor's row `lane` -- the forward sweep of the triangular solves in the two
Mehrotra passes, the polish's first solve, the conjugate-gradient passes, and factor_update's
y = L^-1 z -- recorded from the library built at the commit BEFORE the row moved from vector registers
to accumulator registers.  That change performs the same floating-point
operations in the same order on every value that reaches u*, so tests/test_gpu_kin_rows.py asks for
bit-identical u*, u0, iterations, status, solver flags and polish rounds.

Runs, all on the 70 rows ROWS of kinematic_batch(1024, N=20, seed=31) as one batch (the kernel exists
for N = 20 only):
  (no prefix)  shipped settings.  ROWS holds 153, 260, 441, 855 (failed early polish attempts, rank-one
               update rounds, a dropped bound), 532, the 11-iteration row 677, and every 16th row
  pu_          qp.polish = POLISH_UPD, the smallest value that lets a final attempt run three rounds;
               pu_nupd is, per row, how many of its rounds took their factor from factor_update -- the
               timing build's diag slot T_NUPD, read from the parent's libvcmpc_timing.so
  p0_          qp.polish = 0: the interior point alone
  n_           x0 of batch position NAN_POS made NaN: that row is VC_NONFINITE, the others as without it

Needs an MI355X and the two libraries to record from.  Run from the repo root:
    VCMPC_LIB=/path/to/parent/libvcmpc.so VCMPC_TIMING_LIB=/path/to/parent/libvcmpc_timing.so \\
        python tests/golden/make_kin_rows_golden.py
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vehicle-control_amd"))

N, SEED = 20, 31
MUST = [153, 260, 441, 532, 677, 855]
ROWS = sorted(MUST + [r for r in range(0, 1024, 16) if r not in MUST])
POLISH_UPD = 3
NAN_POS = 37  # position in the batch of 70 (row ROWS[37] of the 1,024)
VC_SOLVED, VC_NONFINITE = 0, 2
T_NUPD, T_NSLOT = 14, 23  # kin_ltv.hip's timing slots: diag is [B][4 + T_NSLOT] in the timing build
KEYS = ("u0", "x_star", "u_star", "status", "iters", "diag")
assert len(ROWS) == 70


def rows_batch():
    from vcmpc.workload import kinematic_batch
    d = kinematic_batch(1024, N=N, seed=SEED)
    return {k: np.ascontiguousarray(v[ROWS]) for k, v in d.items()}


def with_qp(cfg, **kw):
    return dict(cfg, qp=dict(cfg["qp"], **kw))


def run(d, cfg):
    from vcmpc import Context
    from vcmpc.config import load_config
    B = len(d["x0"])
    with Context(N=N, max_batch=B, kin_car=load_config("kinematic_car"), kin_mpc=cfg) as c:
        u0, x, u, st, it, dg = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
    return dict(u0=u0, x_star=x, u_star=u, status=st, iters=it, diag=dg)


def nupd_child(out):
    """Runs under VCMPC_LIB = the timing library: the update rounds of the pu_ run, per row."""
    import ctypes as C

    import torch
    from vcmpc import Context, _abi, make_params
    from vcmpc.config import load_config
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(v).to(dev) for k, v in rows_batch().items()}
    B = len(ROWS)
    p = make_params(kin_car=load_config("kinematic_car"),
                    kin_mpc=with_qp(load_config("kinematic_mpc"), polish=POLISH_UPD))
    with Context(N=N, max_batch=B, params=p) as c:
        xbar = torch.empty((B, N + 1, 6), dtype=torch.float64, device=dev)
        u0 = torch.empty((B, 2), dtype=torch.float64, device=dev)
        st = torch.empty((B,), dtype=torch.int32, device=dev)
        it = torch.empty((B,), dtype=torch.int32, device=dev)
        diag = torch.zeros((B, 4 + T_NSLOT), dtype=torch.float64, device=dev)
        ub = t["ubar"].clone()
        rc = c.lib.vc_solve_diag(c._h, B, *[C.c_void_p(x.data_ptr()) for x in
                                            (t["x0"], t["kappa"], t["ds"], xbar, ub, u0, st, it, diag)],
                                 _abi.VC_DEVICE_PTRS)
        assert rc == 0
        c.synchronize()
        np.save(out, diag.cpu().numpy()[:, 4 + T_NUPD])


def main():
    from vcmpc.config import load_config
    cfg = load_config("kinematic_mpc")
    d = rows_batch()
    out = {"rows": np.array(ROWS)}

    a = run(d, cfg)
    print("base: iters", a["iters"], "rounds", a["diag"][:, 3])
    assert (a["status"] == VC_SOLVED).all()
    assert (a["iters"] == 11).any(), "no 11-iteration interior point"
    assert a["diag"][:, 3].max() >= 3, "no failed early attempt"
    out.update(a)

    pu = run(d, with_qp(cfg, polish=POLISH_UPD))
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "nupd.npy")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--nupd", f], check=True, timeout=300,
                       env=dict(os.environ, VCMPC_LIB=os.environ["VCMPC_TIMING_LIB"]))
        nupd = np.load(f)
    print("pu: rounds", pu["diag"][:, 3], "update rounds", nupd)
    assert ((pu["diag"][:, 3] >= 3) & (nupd >= 1)).any(), "no row with three rounds, one of them an update"
    out.update({"pu_" + k: v for k, v in pu.items()})
    out["pu_nupd"] = nupd

    p0 = run(d, with_qp(cfg, polish=0))
    assert (p0["diag"][:, 3] == 0).all()
    out.update({"p0_" + k: v for k, v in p0.items()})

    dn = {k: v.copy() for k, v in d.items()}
    dn["x0"][NAN_POS] = np.nan
    nn = run(dn, cfg)
    others = np.arange(len(ROWS)) != NAN_POS
    assert nn["status"][NAN_POS] == VC_NONFINITE and (nn["status"][others] == VC_SOLVED).all()
    for k in ("u0", "u_star", "iters", "status"):
        assert np.array_equal(nn[k][others], a[k][others]), k
    out.update({"n_" + k: v for k, v in nn.items()})

    np.savez_compressed(os.path.join(HERE, "kin_rows_golden.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--nupd":
        nupd_child(sys.argv[2])
    else:
        main()
