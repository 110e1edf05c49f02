"""The parity-split G products (kin_ltv.hip grow_dot / gt_dot) inside the fused
kernel, against vectors recorded from the kernel with the 38-term products
(tests/golden/make_kin_gdots_rows_golden.py -> kin_gdots_rows_golden.npz).

The split drops only terms fma(+-0, v, acc) with v finite, so u*, x*, u0, the status, the iteration
counts, the solver flags and the polish rounds must be BIT-IDENTICAL to the recorded ones.

One batch of 14: twelve rows of kinematic_batch(1024, seed=31) -- 153, 260, 441, 855 (failed early
polish attempts, rank-one update rounds, a dropped bound) and the 11-iteration row 677 among them --
one problem whose inputs are finite and whose rollout overflows mid-horizon (a huge ds at stage 12: G
holds non-finite entries from there on, and the output product G z with z = 0 runs over them), and one
NaN row.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SEED = 20, 31
OVF_POS, OVF_STAGE, OVF_DS = 12, 12, 1e308
NAN_POS = 13
VC_SOLVED, VC_NONFINITE = 0, 2


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "kin_gdots_rows_golden.npz")))


@pytest.fixture(scope="module")
def result(gold, kin_cfg):
    from vcmpc import Context
    from vcmpc.config import load_config
    from vcmpc.workload import kinematic_batch
    rows = list(gold["rows"])
    assert len(rows) == 12 and all(r in rows for r in (260, 441, 677, 855))
    d = kinematic_batch(1024, N=N, seed=SEED)
    d = {k: np.ascontiguousarray(v[rows + [rows[0], rows[1]]]) for k, v in d.items()}
    d["ds"][OVF_POS, OVF_STAGE] = OVF_DS
    d["x0"][NAN_POS] = np.nan
    assert all(np.isfinite(d[k][OVF_POS]).all() for k in d)
    with Context(N=N, max_batch=14, kin_car=load_config("kinematic_car"), kin_mpc=kin_cfg) as c:
        u0, x, u, st, it, dg = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
    return dict(u0=u0, x_star=x, u_star=u, status=st, iters=it, diag=dg)


def test_recorded_run_is_what_the_cases_need(gold):
    assert (gold["status"][:12] == VC_SOLVED).all() and (gold["iters"][:12] == 11).any()
    assert gold["status"][OVF_POS] == VC_NONFINITE and gold["status"][NAN_POS] == VC_NONFINITE
    fin = np.isfinite(gold["x_star"][OVF_POS])
    assert fin[:OVF_STAGE + 1].all() and not fin[OVF_STAGE + 2:].all()


def test_c2_rows(result, gold):
    for k in ("u_star", "x_star", "u0", "status", "iters"):
        assert np.array_equal(result[k][:12], gold[k][:12]), k
    assert np.array_equal(result["diag"][:12, 2:], gold["diag"][:12, 2:]), "flags / polish rounds"


def test_rollout_overflows_mid_horizon(result, gold):
    """Finite inputs, non-finite G: every output as recorded (NaN where the record has NaN)."""
    for k in ("u_star", "x_star", "u0", "status", "iters"):
        assert np.array_equal(result[k][OVF_POS], gold[k][OVF_POS], equal_nan=k == "x_star"), k
    assert np.array_equal(result["diag"][OVF_POS, 2:], gold["diag"][OVF_POS, 2:])


def test_nan_row(result, gold):
    for k in ("u_star", "u0", "status", "iters"):
        assert np.array_equal(result[k][NAN_POS], gold[k][NAN_POS]), k
    assert np.array_equal(result["diag"][NAN_POS, 2:], gold["diag"][NAN_POS, 2:])
    assert np.array_equal(np.isfinite(result["x_star"][NAN_POS]), np.isfinite(gold["x_star"][NAN_POS]))
