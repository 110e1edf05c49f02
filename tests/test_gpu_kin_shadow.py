"""Round 10's reordering of kin_ltv.hip's interior-point iteration (the panels' tiles go to
rows in one LDS round trip per panel, through buffers that alias the factor storage, tb3 and the
broadcast vectors; the passes' fused multiply-adds are spelled out) against vectors recorded from
the kernel before it (tests/golden/make_kin_shadow_golden.py -> kin_shadow_golden.npz).  The round
also tried the predictor's right-hand side in the shadow of the normal matrix's MFMAs, which these
cases were chosen for; that part was measured and left out, the cases stay.

The change performs the same floating-point operations in the same order on every value that
reaches u*, so u*, u0, the iteration counts, the status, the solver flags and the polish rounds must
be BIT-IDENTICAL to the recorded ones; x* is held to the tolerance tests/test_gpu_parity.py applies
to the kernel's states (1e-4), as in tests/test_gpu_kin_step.py and tests/test_gpu_kin_factor.py.

The cases are the paths those two do not run: a plain small batch, the iteration limit (the loop is
left right after a step), a non-finite row among finite ones (no interior point at all), obstacles
set on a live context, and a single resumed interior point (B = 1: a factorisation after a polish
that used the same buffers).  The kernel exists for N = 20 only and nothing here depends on the
batch size.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_TOL = 1e-4   # tests/test_gpu_parity.py: the kernel's states
N, SEED = 20, 31
B_SMALL = 70
MAX_ITER_LOW = 4
NAN_ROW = 37
RESUMED = 260  # row of kinematic_batch(1024, N=20, seed=31)
VC_SOLVED, VC_MAX_ITER, VC_NONFINITE = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "kin_shadow_golden.npz")))


@pytest.fixture(scope="module")
def d70():
    from vcmpc.workload import kinematic_batch
    return kinematic_batch(B_SMALL, N=N, seed=SEED)


def _solve(cfg, d, obstacles=None):
    from vcmpc import Context
    from vcmpc.config import load_config
    B = len(d["x0"])
    with Context(N=N, max_batch=B, kin_car=load_config("kinematic_car"), kin_mpc=cfg) as c:
        if obstacles is not None:
            c.set_obstacles(obstacles)
        u0, x, u, st, it, dg = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
    return dict(u0=u0, x_star=x, u_star=u, status=st, iters=it, diag=dg)


def _check(r, g, pre, rows=slice(None)):
    for k in ("u_star", "u0", "iters", "status"):
        assert np.array_equal(r[k][rows], g[pre + k][rows]), k
    # diag[2]: solver flags (1 loss of definiteness, 2 converged, 4 polished, 8 the polish's factor
    # failed), diag[3]: polish rounds -- integers
    assert np.array_equal(r["diag"][rows, 2:], g[pre + "diag"][rows, 2:]), "flags / polish rounds"
    assert np.abs(r["x_star"][rows] - g[pre + "x_star"][rows]).max() < X_TOL


def test_small_batch(kin_cfg, d70, gold):
    r = _solve(kin_cfg, d70)
    _check(r, gold, "a_")
    assert (r["status"] == VC_SOLVED).all()


def test_iteration_limit(kin_cfg, d70, gold):
    """qp.max_iter below what any interior point of the batch needs: the loop is left right after a
    step, through the iteration limit."""
    assert (gold["b_status"] == VC_MAX_ITER).mean() > 0.5  # what the case is for, on the recorded run
    r = _solve(dict(kin_cfg, qp=dict(kin_cfg["qp"], max_iter=MAX_ITER_LOW)), d70)
    _check(r, gold, "b_")
    assert (r["iters"][r["status"] == VC_MAX_ITER] == MAX_ITER_LOW).all()


def test_nonfinite_row_among_finite(kin_cfg, d70, gold):
    """One row's x0 is NaN: that row never enters the interior point and reports VC_NONFINITE; every
    other row is what it is without it."""
    d = {k: v.copy() for k, v in d70.items()}
    d["x0"][NAN_ROW] = np.nan
    r = _solve(kin_cfg, d)
    others = np.arange(B_SMALL) != NAN_ROW
    assert r["status"][NAN_ROW] == VC_NONFINITE
    _check(r, gold, "c_", others)
    _check(r, gold, "a_", others)
    for k in ("u_star", "u0", "iters", "status"):
        assert np.array_equal(r[k][NAN_ROW], gold["c_" + k][NAN_ROW]), k
    assert np.array_equal(r["diag"][NAN_ROW, 2:], gold["c_diag"][NAN_ROW, 2:])
    assert np.array_equal(np.isfinite(r["x_star"][NAN_ROW]), np.isfinite(gold["c_x_star"][NAN_ROW]))


def test_obstacles_set_on_live_context(kin_cfg, gold):
    g = dict(np.load(os.path.join(GOLDEN, "obs_golden.npz")))
    d = {"x0": g["kin_x0"], "kappa": g["kin_kappa"], "ds": g["kin_ds"], "ubar": g["kin_ubar"]}
    r = _solve(kin_cfg, d, [tuple(float(v) for v in o) for o in g["obstacles"]])
    _check(r, gold, "d_")


def test_resumed_interior_point_alone(kin_cfg, gold):
    """B = 1, a problem whose early polish attempt fails: the interior point resumes and factors
    again after a polish that used the broadcast vectors and the transposes' buffers."""
    from vcmpc.workload import kinematic_batch
    assert gold["e_diag"][0, 3] >= 3 and (int(gold["e_diag"][0, 2]) & 4)  # on the recorded run
    d = kinematic_batch(1024, N=N, seed=SEED)
    r = _solve(kin_cfg, {k: np.ascontiguousarray(v[RESUMED:RESUMED + 1]) for k, v in d.items()})
    _check(r, gold, "e_")
    assert r["status"][0] == VC_SOLVED
