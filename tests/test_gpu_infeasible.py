"""GPU: in-kernel infeasibility detection of the stagewise kinematic kernel (csrc/kin_ric.hip,
vc_set_infeasibility / vc_get_farkas), against the phase-1 LP certificates of
oracle/feasibility.py on the oracle's own rows (oracle/ltv_qp.py kin_qp).

Problem set P(N): kinematic_batch(48, N, seed=77) with the delta box at +-0.05 rad, the closed
loop's trust region (1.0 / 0.1) and max_iter = 80 -- the set of test_kin_ric_elastic_rows_vs_oracle,
where most hard-row QPs have no feasible point.

The criterion (y = lam / |lam|_1, R = sum over the stages of max(d_up, d_dn) for a and for w):
    d'y + R |C'y|_inf < 0   =>   no dz satisfies C dz <= d
is re-evaluated here in numpy with the oracle's C and d for every vector the kernel returns, with no
slack: the kernel's guard 1e-9 sits four orders above the fp64 roundoff of these sums.
"""
import functools

import numpy as np
import pytest

from oracle import ltv_qp as Q

pytestmark = pytest.mark.gpu

U_TOL = 1e-5
L = 2.5
B = 48
MAX_ITER = 80


def _cfg(solver=1, **qp):
    from vcmpc.config import load_config
    cfg = load_config("kinematic_mpc")
    cfg["qp"] = dict(cfg.get("qp") or {}, solver=solver, trust_a=1.0, trust_w=0.1, max_iter=MAX_ITER, **qp)
    cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
    return cfg


def _ctx(N, detect, solver=1, **qp):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(kin_car=load_config("kinematic_car"), kin_mpc=_cfg(solver, **qp))
    return Context(model=_abi.VC_MODEL_KINEMATIC, N=N, max_batch=B, dtype=_abi.VC_F64, params=p,
                   detect_infeasible=detect)


@functools.lru_cache(maxsize=None)
def _problems(N):
    """P(N) with the oracle's truth: rows C, d, the phase-1 verdicts and, on the feasible problems,
    the oracle's u*.  Computed once per horizon and shared (never modified) by the tests."""
    from oracle.feasibility import phase1
    from vcmpc.workload import kinematic_batch
    W = Q.kin_weights(_cfg())
    d = kinematic_batch(B, N=N, seed=77)
    Qd = Q.kin_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], L, W)
    cert = [phase1(Qd["C"][b], Qd["d"][b]) for b in range(B)]
    infeasible = np.array([not c["feasible"] for c in cert])
    assert all(c["farkas_ok"] for c, i in zip(cert, infeasible) if i)  # the truth is itself certified
    fe = np.nonzero(~infeasible)[0]
    ref = Q.kin_ltv_solve(d["x0"][fe], d["ubar"][fe], d["kappa"][fe], d["ds"][fe], L, W)
    return dict(d=d, C=Qd["C"], dvec=Qd["d"], xbar=Qd["xbar"], infeasible=infeasible, feasible_idx=fe,
                u_ref=ref["u_star"])


@functools.lru_cache(maxsize=None)
def _run(N, detect, solver=1):
    """One host-pointer solve of P(N); (u0, x*, u*, status, iters, diag, farkas or None)."""
    d = _problems(N)["d"]
    with _ctx(N, detect, solver) as c:
        r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        y = c.farkas() if detect else None
    return tuple(r) + (y,)


def _check_status_exact(P, st):
    inf = P["infeasible"]
    miss = np.nonzero(inf & (st != 4))[0]
    false_pos = np.nonzero(~inf & (st == 4))[0]
    assert len(false_pos) == 0, f"status 4 on feasible problems {false_pos.tolist()}"
    assert len(miss) == 0, f"oracle-infeasible problems not detected {miss.tolist()}: status {st[miss].tolist()}"


def _check_certificates(P, N, us, xs, st, it, y):
    d = P["d"]
    assert y.shape == (B, 7 * N - 3)
    worst = -np.inf
    for b in np.nonzero(st == 4)[0]:
        yb, C, dv = y[b], P["C"][b], P["dvec"][b]
        assert (yb >= 0.0).all()
        assert abs(yb.sum() - 1.0) <= 1e-12
        box = dv[:4 * N].reshape(N, 4)
        R = (np.maximum(box[:, 0], box[:, 1]) + np.maximum(box[:, 2], box[:, 3])).sum()
        val = float(dv @ yb + R * np.abs(C.T @ yb).max())
        worst = max(worst, val)
        assert val < 0.0, (int(b), val)
        assert it[b] < MAX_ITER
        np.testing.assert_array_equal(us[b], d["ubar"][b])
        assert np.isfinite(xs[b]).all()
    # rows of problems that did not end infeasible are exactly zero
    assert not y[st != 4].any()
    return worst


@pytest.mark.parametrize("N", [10, 20, 50])
def test_detection_matches_phase1_and_certifies(N):
    """Items 1-4: status 4 exactly on the oracle-infeasible problems (no miss, no false positive),
    every returned vector is a Farkas certificate by the host-side inequality, the output of an
    infeasible problem is its warm start; the feasible problems are solved to the oracle's u* with the
    status and iteration count of a detection-off run."""
    P = _problems(N)
    u0, xs, us, st, it, dg, y = _run(N, True)
    u0f, xsf, usf, stf, itf, dgf, _ = _run(N, False)
    inf, fe = P["infeasible"], P["feasible_idx"]
    print(f"N={N}: status on the {int(inf.sum())} oracle-infeasible {np.bincount(st[inf], minlength=5).tolist()}, "
          f"on the feasible {np.bincount(st[fe], minlength=5).tolist()} (counts of status 0..4); iterations of "
          f"the infeasible {sorted(it[inf].tolist())}")
    _check_status_exact(P, st)
    worst = _check_certificates(P, N, us, xs, st, it, y)
    assert ((dg[:, 2].astype(int) & 32) > 0).tolist() == (st == 4).tolist()
    err = np.abs(us[fe] - P["u_ref"]).max(axis=(1, 2))
    same_bits = np.array_equal(us[fe], usf[fe])
    print(f"N={N}: {int(inf.sum())} of {B} infeasible, all detected; iterations of the infeasible mean "
          f"{it[inf].mean():.1f} max {it[inf].max()} (detection off: {itf[inf].min()}..{itf[inf].max()}); "
          f"largest certificate value {worst:.3e}; feasible |u* - u*_oracle| max {err.max():.2e}, "
          f"iterations {it[fe].min()}..{it[fe].max()}; u* bit-identical to the detection-off run: {same_bits}")
    assert (st[fe] == 0).all(), st[fe]
    assert err.max() < U_TOL
    np.testing.assert_array_equal(st[fe], stf[fe])
    np.testing.assert_array_equal(it[fe], itf[fe])


@pytest.mark.parametrize("N", [10, 20, 50])
def test_detection_off_is_unchanged(N):
    """Item 5: the default context never reports status 4, leaves the oracle-infeasible problems
    non-solved, and has no certificates to return."""
    from vcmpc import _abi
    P = _problems(N)
    st = _run(N, False)[3]
    assert (st != 4).all()
    assert (st[P["infeasible"]] != 0).all()
    d = P["d"]
    with _ctx(N, False) as c:
        c.solve(d["x0"][:4], d["kappa"][:4], d["ds"][:4], d["ubar"][:4].copy())
        with pytest.raises(_abi.VcError):
            c.farkas()


def test_detection_routes_condensed_horizon_to_stagewise(kin_golden):
    """Item 6: N = 20 with vc_qp.solver = 0 (the condensed kernel's shape) and detection on is solved
    by the stagewise kernel -- the assertions of items 1 and 3 hold -- and a default solver = 0
    context whose detection was turned on and off again returns the condensed kernel's answer: the
    golden u* to 1e-5, bit-identical to a context that never had it on."""
    from vcmpc import Context
    from vcmpc.config import load_config
    N = 20
    P = _problems(N)
    u0, xs, us, st, it, dg, y = _run(N, True, solver=0)
    _check_status_exact(P, st)
    _check_certificates(P, N, us, xs, st, it, y)
    g = kin_golden
    kw = dict(N=N, max_batch=len(g["x0"]), kin_car=load_config("kinematic_car"), kin_mpc=load_config("kinematic_mpc"))
    with Context(**kw) as c:
        ref = c.solve(g["x0"], g["kappa"], g["ds"], g["ubar"].copy())
    with Context(detect_infeasible=True, **kw) as c:
        on = c.solve(g["x0"], g["kappa"], g["ds"], g["ubar"].copy())
        c.set_infeasibility(False)
        off = c.solve(g["x0"], g["kappa"], g["ds"], g["ubar"].copy())
    assert (on[3] == 0).all() and (off[3] == 0).all()
    assert np.abs(on[2] - g["u_star"]).max() < U_TOL
    assert np.abs(off[2] - g["u_star"]).max() < U_TOL
    np.testing.assert_array_equal(off[2], ref[2])
    np.testing.assert_array_equal(off[4], ref[4])


def test_elastic_rows_are_never_infeasible():
    """Item 7: with elastic state rows every QP has a solution; detection on changes nothing."""
    N = 20
    d = _problems(N)["d"]
    with _ctx(N, True, elastic=1e3) as c:
        st = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy())[3]
        y = c.farkas()
    assert (st == 0).all(), st
    assert not y.any()


def test_multiple_shooting_same_status():
    """Item 8: vc_qp.ms = 1 with the oracle rollout as state iterate is the same QP (zero defects):
    the same status vector as single shooting."""
    N = 20
    P = _problems(N)
    d = P["d"]
    with _ctx(N, True, ms=1) as c:
        st = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), xbar=P["xbar"].copy())[3]
    np.testing.assert_array_equal(st, _run(N, True)[3])
    _check_status_exact(P, st)


def test_kin_sqp_passes_status_through():
    """Item 9: vc_qp.kin_sqp = 1 with hard rows.  The step's status is its first QP's (kin_merit.hip
    only tests == VC_SOLVED and hands any other value on), and that QP is kin_qp of the same inputs
    (single shooting, the QP linearised at the rollout of ubar), so status 4 appears, and only on
    oracle-infeasible problems; the certificates of an SQP call are not retrievable."""
    from vcmpc import _abi
    N = 20
    P = _problems(N)
    d = P["d"]
    with _ctx(N, True, kin_sqp=1) as c:
        st = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy())[3]
        with pytest.raises(_abi.VcError) as e:
            c.farkas()
    assert e.value.code == _abi.VC_E_UNSUPPORTED
    assert (st == 4).any()
    assert not (st[~P["infeasible"]] == 4).any()


def test_device_pointers_equal_host_pointers():
    """Item 10: torch tensors on the device give the status and certificates of the host-array run."""
    import torch
    N = 20
    d = _problems(N)["d"]
    host = _run(N, True)
    with _ctx(N, True) as c:
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
        r = c.solve(t["x0"], t["kappa"], t["ds"], t["ubar"])
        y = c.farkas()
        torch.cuda.synchronize()
        assert isinstance(y, torch.Tensor) and y.is_cuda
        st, yh = r[3].cpu().numpy(), y.cpu().numpy()
    np.testing.assert_array_equal(st, host[3])
    np.testing.assert_array_equal(yh, host[6])


def test_dynamic_context_is_unsupported():
    """Item 11: a single-track context refuses the detection and still solves."""
    import os
    from conftest import GOLDEN
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    g = {k: v.astype(np.float64) for k, v in np.load(os.path.join(GOLDEN, "dyn_sqp_golden.npz")).items()}
    n = 4
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("dynamic_mpc"), tyre="linear")
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=40, max_batch=n, dtype=_abi.VC_F64, params=p) as c:
        with pytest.raises(_abi.VcError) as e:
            c.set_infeasibility(True)
        assert e.value.code == _abi.VC_E_UNSUPPORTED
        assert c.lib.vc_set_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
        st = c.solve(g["x0"][:n], g["kappa"][:n], g["ds"][:n], g["ubar"][:n].copy())[3]
    assert (st == 0).all(), st


def test_controller_config_key_enables_detection():
    """`qp.detect_infeasible` of the controller config turns the detection on (default off) and the
    controller counts the certified steps beside `status`.  Vehicles whose steering angle 0.25 rad is
    far outside a +-0.05 box have no feasible first stage (one step moves delta by ds w_max / s' ~ 0.05;
    phase-1 t* ~ 0.37 for every one of them), so the first solve is infeasible and the neutral retry
    takes over.  A count is only ever a certified problem, so counts are 0 or 1 here; that none is
    missed is asserted in the regime the zero-miss condition is stated for -- max_iter = 80 and a
    warm-start rollout inside the workload sampler's domain (v > 1 m/s along the horizon; the
    controller's first guess 1 + U[0, 1) rolls two of the eight vehicles out of it, one to v = -85 m/s,
    and that one's certificate needs 47 iterations: under the default cap of 40 it ends VC_MAX_ITER,
    as it does with the detection off)."""
    from vcmpc.config import load_config
    from vcmpc.controllers import kinematic_mpc as KM
    from vcmpc.environment import Track
    from vcmpc.models import KinematicCar
    track = Track.load("ippodromo")
    car = KinematicCar(load_config("kinematic_car"), track)
    n = 8
    x0 = np.zeros((n, 6))
    x0[:, 0] = 6.0
    x0[:, 1] = 0.25
    x0[:, 2] = np.linspace(1.0, 15.0, n)
    cfg = load_config("kinematic_mpc")
    cfg["horizon"] = 20
    cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
    cfg["qp"] = dict(cfg.get("qp") or {}, max_iter=MAX_ITER)
    off = KM.BatchedKinematicMPC(car, cfg, batch=n)
    assert not off.detect_infeasible and not off.ctx.detect_infeasible
    u_off = off.command(x0)
    assert (off.infeasible_steps == 0).all()
    cfg["qp"] = dict(cfg["qp"], detect_infeasible=True)
    on = KM.BatchedKinematicMPC(car, cfg, batch=n)
    assert on.detect_infeasible and on.ctx.detect_infeasible
    # the first solve's warm start, as command() builds it, and its rollout (CPU oracle)
    ds, kappa = KM.horizon_params(x0[:, 2], on.state_prediction[:, 0, :], on.dt, track.k)
    ubar = np.swapaxes(on.action_prediction, 1, 2).copy()
    ic = cfg["input_constraints"]
    np.clip(ubar[..., 0], ic["a_min"], ic["a_max"], out=ubar[..., 0])
    np.clip(ubar[..., 1], ic["w_min"], ic["w_max"], out=ubar[..., 1])
    in_domain = (Q.kin_predict(x0, ubar, kappa, ds, L)[:, :, 0] > 1.0).all(axis=1)
    u_on = on.command(x0)
    print(f"controller: infeasible first solves {on.infeasible_steps.tolist()}, rollout in the sampler's domain "
          f"{in_domain.tolist()}, status after the retry {on.status.tolist()}")
    assert on.infeasible_steps.shape == (n,) and ((on.infeasible_steps == 0) | (on.infeasible_steps == 1)).all()
    assert in_domain.sum() >= n // 2
    assert (on.infeasible_steps[in_domain] == 1).all()
    assert np.isfinite(u_on).all() and np.isfinite(u_off).all()
