"""The factor's row `lane` in accumulator registers (kin_ltv.hip, round 11: RowRegs, forward_sweep)
against vectors recorded from the kernel that kept it in vector registers
(tests/golden/make_kin_rows_golden.py -> kin_rows_golden.npz).

The change performs the same floating-point operations in the same order on every value that reaches
u*, so u*, u0, the iteration counts, the status, the solver flags and the polish rounds must be
BIT-IDENTICAL to the recorded ones; x* is held to the tolerance tests/test_gpu_parity.py applies to
the kernel's states (1e-4), as in tests/test_gpu_kin_factor.py.

Every caller of the forward sweep is run: the two Mehrotra passes, the polish's first solve and its
conjugate-gradient passes, factor_update's y = L^-1 z (a run whose recorded diag shows a row with three
polish rounds of which one took its factor from a rank-one update), the interior point alone, two
launches on one context, batches of 1, 3 and 65, and a non-finite row among finite ones.  One batch of
70 rows serves all of them; the kernel exists for N = 20 only.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_TOL = 1e-4   # tests/test_gpu_parity.py: the kernel's states
N, SEED = 20, 31
POLISH_UPD = 3
NAN_POS = 37
VC_SOLVED, VC_NONFINITE = 0, 2


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "kin_rows_golden.npz")))


@pytest.fixture(scope="module")
def d70(gold):
    from vcmpc.workload import kinematic_batch
    d = kinematic_batch(1024, N=N, seed=SEED)
    return {k: np.ascontiguousarray(v[gold["rows"]]) for k, v in d.items()}


def _take(d, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in d.items()}


def _launch(c, d):
    u0, x, u, st, it, dg = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
    return dict(u0=u0, x_star=x, u_star=u, status=st, iters=it, diag=dg)


def _solve(cfg, d):
    from vcmpc import Context
    from vcmpc.config import load_config
    with Context(N=N, max_batch=len(d["x0"]), kin_car=load_config("kinematic_car"), kin_mpc=cfg) as c:
        return _launch(c, d)


def _check(r, g, pre="", rows=slice(None), grows=None):
    """r[rows] against the recorded g[pre + .][grows] (grows: the same rows unless given)."""
    grows = rows if grows is None else grows
    for k in ("u_star", "u0", "iters", "status"):
        assert np.array_equal(r[k][rows], g[pre + k][grows]), k
    # diag[2]: solver flags, diag[3]: polish rounds -- integers
    assert np.array_equal(r["diag"][rows, 2:], g[pre + "diag"][grows, 2:]), "flags / polish rounds"
    assert np.abs(r["x_star"][rows] - g[pre + "x_star"][grows]).max() < X_TOL


def test_every_solve_call_site(kin_cfg, d70, gold):
    # what the case is for, on the recorded run
    rows = list(gold["rows"])
    assert len(rows) == 70 and all(r in rows for r in (153, 260, 441, 855))
    assert (gold["iters"] == 11).any() and gold["diag"][:, 3].max() >= 3
    r = _solve(kin_cfg, d70)
    _check(r, gold)
    assert (r["status"] == VC_SOLVED).all()


def test_factor_update(kin_cfg, d70, gold):
    """qp.polish = 3: a final attempt of three rounds.  On the recorded run some row has three rounds
    of which at least one took its factor from factor_update (pu_nupd: the timing build's count of
    update rounds), whose forward sweep reads the row it has just loaded into the accumulators."""
    assert ((gold["pu_diag"][:, 3] >= 3) & (gold["pu_nupd"] >= 1)).any()
    r = _solve(dict(kin_cfg, qp=dict(kin_cfg["qp"], polish=POLISH_UPD)), d70)
    _check(r, gold, "pu_")


def test_polish_off(kin_cfg, d70, gold):
    r = _solve(dict(kin_cfg, qp=dict(kin_cfg["qp"], polish=0)), d70)
    _check(r, gold, "p0_")
    assert (r["diag"][:, 3] == 0).all()


def test_two_launches_on_one_context(kin_cfg, d70, gold):
    """Different rows in the same batch positions, one launch after the other: nothing of the first
    launch's row registers reaches the second."""
    from vcmpc import Context
    from vcmpc.config import load_config
    first, second = np.arange(0, 35), np.arange(35, 70)
    with Context(N=N, max_batch=35, kin_car=load_config("kinematic_car"), kin_mpc=kin_cfg) as c:
        ra = _launch(c, _take(d70, first))
        rb = _launch(c, _take(d70, second))
    _check(ra, gold, grows=first)
    _check(rb, gold, grows=second)


@pytest.mark.parametrize("B", [1, 3, 65])
def test_batch_sizes(kin_cfg, d70, gold, B):
    """The same rows give the same bits in a batch of another size, at other positions."""
    start = {1: list(gold["rows"]).index(260), 3: 20, 65: 5}[B]
    idx = np.arange(start, start + B)
    _check(_solve(kin_cfg, _take(d70, idx)), gold, grows=idx)


def test_nonfinite_row_among_finite(kin_cfg, d70, gold):
    d = {k: v.copy() for k, v in d70.items()}
    d["x0"][NAN_POS] = np.nan
    r = _solve(kin_cfg, d)
    others = np.arange(70) != NAN_POS
    assert r["status"][NAN_POS] == VC_NONFINITE
    _check(r, gold, "n_", others)
    _check(r, gold, "", others)
    for k in ("u_star", "u0", "iters", "status"):
        assert np.array_equal(r[k][NAN_POS], gold["n_" + k][NAN_POS]), k
    assert np.array_equal(r["diag"][NAN_POS, 2:], gold["n_diag"][NAN_POS, 2:])
    assert np.array_equal(np.isfinite(r["x_star"][NAN_POS]), np.isfinite(gold["n_x_star"][NAN_POS]))
