"""The fused kinematic kernel's serial path outside the factorisation (kin_ltv.hip: the rollout's
off-chain work -- stage weights, finiteness test, state scatter -- the lane-parallel output sweep,
and any restatement of the Mehrotra passes' step arithmetic) against vectors recorded from the kernel
before that restructuring (tests/golden/make_kin_step_golden.py -> kin_step_golden.npz).

Such changes perform the same operations on every value that reaches u*, so u*, the iteration
counts and the status must be BIT-IDENTICAL to the recorded ones; x* (the output sweep sums in
another order) may move at rounding level and is held to the tolerance tests/test_gpu_parity.py
applies to the kernel's states (1e-4), to the recorded x*, and to the oracle's xbar + G dz.

B = 70 is the smallest batch whose XCD placement has a ragged last group; row 0 is the B = 1 case.
The kernel exists for N = 20 only.

Not covered: a run whose early polish attempt cannot be taken.  The attempt's threshold is
max(tol, KIN_EARLY_F tol) with KIN_EARLY_F a compile-time constant of the kernel, so no qp.tol > 0
makes it equal tol and the ABI has no switch for it.
"""
import numpy as np
import pytest

from oracle import ltv_qp as Q

pytestmark = pytest.mark.gpu

U_TOL = 1e-5   # tests/test_gpu_parity.py: u* against the oracle
X_TOL = 1e-4   # tests/test_gpu_parity.py: the kernel's states
# x* against the oracle's linearisation applied to the kernel's own dz: both are fp64 evaluations of
# the same xbar and G (checked to 1e-12 relative elsewhere); |x| <= ~4e2 (s), <= 40 terms per entry
X_LIN_TOL = 1e-8
B, N, L, SEED, NF_ROW = 70, 20, 2.5, 31, 35


@pytest.fixture(scope="module")
def gold():
    import os
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "kin_step_golden.npz")))


@pytest.fixture(scope="module")
def batch():
    from vcmpc.workload import kinematic_batch
    return kinematic_batch(B, N=N, seed=SEED)


@pytest.fixture(scope="module")
def oracle(batch, kin_W):
    d = batch
    return Q.kin_ltv_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], L, kin_W)


def _solve(cfg, d, nb=None):
    from vcmpc import Context
    from vcmpc.config import load_config
    sl = slice(0, nb)
    with Context(N=N, max_batch=B, kin_car=load_config("kinematic_car"), kin_mpc=cfg) as c:
        u0, x, u, st, it = c.solve(*(np.ascontiguousarray(d[k][sl]) for k in ("x0", "kappa", "ds")),
                                   np.ascontiguousarray(d["ubar"][sl]).copy())
    return dict(u0=u0, x_star=x, u_star=u, status=st, iters=it)


def _bit_identical(r, g, pre="", rows=slice(None)):
    for k in ("u_star", "u0", "iters", "status"):
        assert np.array_equal(r[k][rows], g[pre + k][rows]), k


def _x_linearised(oracle, d, u_star, rows=slice(None)):
    dz = (u_star - d["ubar"][rows]).reshape(len(u_star), 2 * N)
    return oracle["xbar"][rows] + oracle["e"][rows] + np.einsum("bkin,bn->bki", oracle["G"][rows], dz)


@pytest.mark.parametrize("nb", [B, 1])
def test_golden(kin_cfg, batch, gold, oracle, nb):
    r = _solve(kin_cfg, batch, nb)
    rows = slice(0, nb)
    _bit_identical(r, gold, rows=rows)
    assert (r["status"] == 0).all()
    assert np.abs(r["x_star"] - gold["x_star"][rows]).max() < X_TOL
    assert np.abs(r["x_star"] - oracle["x_star"][rows]).max() < X_TOL
    assert np.abs(r["u_star"] - oracle["u_star"][rows]).max() < U_TOL
    assert np.abs(r["x_star"] - _x_linearised(oracle, batch, r["u_star"], rows)).max() < X_LIN_TOL


def test_polish_off(kin_cfg, batch, gold, oracle):
    """qp.polish = 0 returns the interior-point iterate: the output sweep must not lean on
    anything the polish computed."""
    cfg = dict(kin_cfg, qp=dict(kin_cfg["qp"], polish=0))
    r = _solve(cfg, batch)
    _bit_identical(r, gold, "p0_")
    assert np.abs(r["x_star"] - gold["p0_x_star"]).max() < X_TOL
    assert np.abs(r["x_star"] - _x_linearised(oracle, batch, r["u_star"])).max() < X_LIN_TOL


def test_nonfinite_in_the_middle(kin_cfg, batch, gold):
    """One problem with a non-finite x0 inside the batch: VC_NONFINITE and the recorded outputs
    for it (the rollout's single finiteness test, the sweep's z = 0 path), the other 69 untouched."""
    d = {k: v.copy() for k, v in batch.items()}
    d["x0"][NF_ROW, 3] = np.nan
    r = _solve(kin_cfg, d)
    assert r["status"][NF_ROW] == 2 and gold["nf_status"][NF_ROW] == 2
    for k in ("u_star", "u0", "iters", "status", "x_star"):
        np.testing.assert_array_equal(r[k][NF_ROW], gold["nf_" + k][NF_ROW], err_msg=k)  # NaN == NaN here
    rest = np.arange(B) != NF_ROW
    _bit_identical(r, gold, rows=rest)
    _bit_identical(r, gold, "nf_", rows=rest)
    assert np.abs(r["x_star"][rest] - gold["x_star"][rest]).max() < X_TOL


def test_trust_region_vs_oracle(kin_cfg, batch):
    """qp.trust_a / trust_w tighten the input boxes, which changes the bounds that bind."""
    cfg = dict(kin_cfg, qp=dict(kin_cfg["qp"], trust_a=0.8, trust_w=0.05))
    d = batch
    ref = Q.kin_ltv_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], L, Q.kin_weights(cfg))
    assert ref["polished"].all()
    r = _solve(cfg, d)
    assert (r["status"] == 0).all()
    assert np.abs(r["u_star"] - ref["u_star"]).max() < U_TOL
    assert np.abs(r["x_star"] - ref["x_star"]).max() < X_TOL
    du = np.abs(r["u_star"] - d["ubar"])
    assert du[..., 0].max() <= 0.8 + 1e-9 and du[..., 1].max() <= 0.05 + 1e-9
