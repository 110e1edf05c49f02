"""The blocked factorisation's lane-set bookkeeping (kin_ltv.hip, factor_blocked: the row registers
zeroed on and above the diagonal, the branch-free column stores) against vectors recorded from the
kernel before that bookkeeping moved to the scalar unit (tests/golden/make_kin_factor_golden.py ->
kin_factor_golden.npz).

The change performs the same floating-point operations in the same order on every value that
reaches u*, so u*, u0, the iteration counts, the status, the solver flags and the polish rounds
must be BIT-IDENTICAL to the recorded ones; x* is held to the tolerance tests/test_gpu_parity.py
applies to the kernel's states (1e-4), as in tests/test_gpu_kin_step.py.

The problems are the ones that read most of what the factorisation leaves behind: nine rows of the
C2 batch with failed early polish attempts, polish rounds that update the factor by a rank-one term
or refactor after a drop, and 11-iteration interior points; the same rows without the polish; and a
run whose tolerance is low enough that one interior point leaves through the loss-of-definiteness
exit (factor_blocked returns false).  The kernel exists for N = 20 only, and the lane sets do not
depend on the batch size.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_TOL = 1e-4   # tests/test_gpu_parity.py: the kernel's states
N, SEED = 20, 31
HARD = [153, 260, 441, 532, 855, 677, 689, 706, 868]  # rows of kinematic_batch(1024, N=20, seed=31)
B_CF = 70


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "kin_factor_golden.npz")))


@pytest.fixture(scope="module")
def hard():
    from vcmpc.workload import kinematic_batch
    d = kinematic_batch(1024, N=N, seed=SEED)
    return {k: np.ascontiguousarray(v[HARD]) for k, v in d.items()}


def _solve(cfg, d):
    from vcmpc import Context
    from vcmpc.config import load_config
    B = len(d["x0"])
    with Context(N=N, max_batch=B, kin_car=load_config("kinematic_car"), kin_mpc=cfg) as c:
        u0, x, u, st, it, dg = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
    return dict(u0=u0, x_star=x, u_star=u, status=st, iters=it, diag=dg)


def _check(r, g, pre=""):
    for k in ("u_star", "u0", "iters", "status"):
        assert np.array_equal(r[k], g[pre + k]), k
    # diag[2]: solver flags (1 loss of definiteness, 2 converged, 4 polished, 8 the polish's factor
    # failed), diag[3]: polish rounds -- integers
    assert np.array_equal(r["diag"][:, 2:], g[pre + "diag"][:, 2:]), "flags / polish rounds"
    assert np.abs(r["x_star"] - g[pre + "x_star"]).max() < X_TOL


def test_hard_rows(kin_cfg, hard, gold):
    # what the case is for, on the recorded run
    assert gold["diag"][:, 3].max() >= 3 and (gold["iters"] == 11).any()
    r = _solve(kin_cfg, hard)
    _check(r, gold)
    assert (r["status"] == 0).all()


def test_hard_rows_polish_off(kin_cfg, hard, gold):
    """qp.polish = 0 returns the interior-point iterate: every digit of it went through the
    factor's rows (forward sweep) and stored columns (backward sweep)."""
    r = _solve(dict(kin_cfg, qp=dict(kin_cfg["qp"], polish=0)), hard)
    _check(r, gold, "p0_")
    assert (r["diag"][:, 3] == 0).all()


def test_loss_of_definiteness_exit(kin_cfg, gold):
    """qp.tol four orders below the shipped value on the 70-problem batch: one interior point runs
    on until a pivot of its normal matrix is not positive, leaves the loop there (a uniform early
    exit after factor_blocked returned false) and hands its iterate to the polish."""
    from vcmpc.workload import kinematic_batch
    tol = float(gold["cf_tol"])
    lost = (gold["cf_diag"][:, 2].astype(np.int64) & 1) != 0
    assert lost.any() and tol < kin_cfg["qp"]["tol"]
    r = _solve(dict(kin_cfg, qp=dict(kin_cfg["qp"], tol=tol)), kinematic_batch(B_CF, N=N, seed=SEED))
    _check(r, gold, "cf_")
    assert all(np.isfinite(r[k]).all() for k in ("u_star", "u0", "x_star", "diag"))
