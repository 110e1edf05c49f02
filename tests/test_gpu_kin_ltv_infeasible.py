"""GPU: in-kernel infeasibility detection of the condensed kinematic kernel (csrc/kin_ltv.hip,
kin_ltv_kernel<20, true>; vc_qp.solver = 2 with vc_set_infeasibility on), against the phase-1 LP
certificates of oracle/feasibility.py on the oracle's own rows (oracle/ltv_qp.py kin_qp).

Instantiation coverage (the table at the head of tests/test_gpu_instantiations.py gains this row):

    kernel      axis value                          test
    ----------  ----------------------------------  -------------------------------------------------------
    kin_ltv     N = 20, DET on                      test_gpu_kin_ltv_infeasible.py  (this file)

Problem set P(20), built exactly as tests/test_gpu_infeasible.py builds it: kinematic_batch(48, 20,
seed=77) with the delta box at +-0.05 rad, the closed loop's trust region (1.0 / 0.1) and max_iter = 80.

The criterion (y >= 0, |y|_1 = 1, R = sum over the stages of max(d_up, d_dn) for a and for w):
    d'y + R |C'y|_inf < 0   =>   no dz satisfies C dz <= d
is re-evaluated here in numpy with the oracle's C and d for every vector the kernel returns, with no
slack.  The kernel returns y = lam / |lam|_1 where that satisfies it, else -- from the same iteration's
row multipliers -- the y whose box multipliers cancel C'y (csrc/kin_ltv.hip); both are held
to the same inequality here.

Two properties carry the file: the detection finds exactly the phase-1-infeasible problems, and a
problem it does not certify is solved bit for bit as the condensed kernel solves it with the
detection off (vc_qp.solver = 0, the default context) -- u*, x*, u0, status, iterations, diagnostics.
"""
import functools

import numpy as np
import pytest

from oracle import ltv_qp as Q
from test_gpu_closed_loop import DT, MPC_DT, _kin_states, _warm

pytestmark = pytest.mark.gpu

U_TOL = 1e-5
L = 2.5
N = 20
B = 48
MAX_ITER = 80


def _cfg(solver, tight=True):
    from vcmpc.config import load_config
    cfg = load_config("kinematic_mpc")
    if tight:
        cfg["qp"] = dict(cfg.get("qp") or {}, solver=solver, trust_a=1.0, trust_w=0.1, max_iter=MAX_ITER)
        cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
    else:
        cfg["qp"] = dict(cfg.get("qp") or {}, solver=solver)
    return cfg


def _ctx(solver, detect, tight=True, max_batch=B):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(kin_car=load_config("kinematic_car"), kin_mpc=_cfg(solver, tight))
    assert p.qp.solver == solver
    return Context(model=_abi.VC_MODEL_KINEMATIC, N=N, max_batch=max_batch, dtype=_abi.VC_F64, params=p,
                   detect_infeasible=detect)


@functools.lru_cache(maxsize=None)
def _problems():
    """P(20) with the oracle's truth: rows C, d, the phase-1 verdicts and, on the feasible problems,
    the oracle's u*.  Computed once and shared (never modified) by the tests."""
    from oracle.feasibility import phase1
    from vcmpc.workload import kinematic_batch
    W = Q.kin_weights(_cfg(2))
    d = kinematic_batch(B, N=N, seed=77)
    Qd = Q.kin_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], L, W)
    cert = [phase1(Qd["C"][b], Qd["d"][b]) for b in range(B)]
    infeasible = np.array([not c["feasible"] for c in cert])
    assert all(c["farkas_ok"] for c, i in zip(cert, infeasible) if i)  # the truth is itself certified
    fe = np.nonzero(~infeasible)[0]
    ref = Q.kin_ltv_solve(d["x0"][fe], d["ubar"][fe], d["kappa"][fe], d["ds"][fe], L, W)
    return dict(d=d, C=Qd["C"], dvec=Qd["d"], infeasible=infeasible, feasible_idx=fe, u_ref=ref["u_star"])


@functools.lru_cache(maxsize=None)
def _run(solver, detect):
    """One host-pointer solve of P(20); (u0, x*, u*, status, iters, diag, farkas or None)."""
    d = _problems()["d"]
    with _ctx(solver, detect) as c:
        r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        y = c.farkas() if detect else None
    return tuple(r) + (y,)


def _assert_same_bits(got, want, idx=slice(None), what=""):
    for name, g, w in zip(("u0", "x*", "u*", "status", "iters", "diag"), got, want):
        np.testing.assert_array_equal(g[idx], w[idx], err_msg=f"{what}{name}")


def test_status_certificates_and_outputs():
    """Item 1: status 4 exactly on the phase-1-infeasible problems; every returned vector is a Farkas
    certificate by the host-side inequality; the output of a certified problem is its warm start.
    Measured on an MI355X: see profiles/infeasible/test_gpu_kin_ltv_infeasible.log."""
    P = _problems()
    u0, xs, us, st, it, dg, y = _run(2, True)
    inf, d = P["infeasible"], P["d"]
    print(f"status on the {int(inf.sum())} phase-1-infeasible {np.bincount(st[inf], minlength=5).tolist()}, on the "
          f"feasible {np.bincount(st[~inf], minlength=5).tolist()} (counts of status 0..4); iterations of the "
          f"infeasible {sorted(it[inf].tolist())}")
    false_pos = np.nonzero(~inf & (st == 4))[0]
    miss = np.nonzero(inf & (st != 4))[0]
    assert len(false_pos) == 0, f"status 4 on feasible problems {false_pos.tolist()}"
    assert len(miss) == 0, f"phase-1-infeasible problems not detected {miss.tolist()}: status {st[miss].tolist()}"
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
        np.testing.assert_array_equal(u0[b], d["ubar"][b, 0])
        assert np.isfinite(xs[b]).all()
    print(f"largest certificate value {worst:.3e}; iterations of the infeasible mean {it[inf].mean():.1f} "
          f"max {it[inf].max()}")
    assert ((dg[:, 2].astype(int) & 32) > 0).tolist() == (st == 4).tolist()
    assert not y[st != 4].any()  # rows of problems that did not end infeasible are exactly zero


def test_feasible_problems_solved_bit_for_bit():
    """Item 2: the feasible problems of P(20) are solved to the oracle's u*, and every output is
    bit-identical to the condensed kernel's without the detection (solver = 0, detection off).  On a
    library without the feature solver = 2 is the stagewise kernel: other iterations, other bits."""
    P = _problems()
    fe = P["feasible_idx"]
    on = _run(2, True)
    ref = _run(0, False)
    err = np.abs(on[2][fe] - P["u_ref"]).max(axis=(1, 2))
    print(f"feasible: |u* - u*_oracle| max {err.max():.2e}, iterations {on[4][fe].min()}..{on[4][fe].max()} "
          f"(detection off {ref[4][fe].min()}..{ref[4][fe].max()})")
    assert (on[3][fe] == 0).all(), on[3][fe]
    assert err.max() < U_TOL
    _assert_same_bits(on[:6], ref[:6], fe, "feasible problems of P(20): ")


@functools.lru_cache(maxsize=None)
def _c2_like():
    from vcmpc.workload import kinematic_batch
    return kinematic_batch(256, N=N, seed=31)


def test_feasible_c2_like_batch_is_untouched():
    """Item 3: 256 problems of the benchmark's sampler and config: no status 4, zero certificate
    rows, every output bit-identical to solver = 0 without the detection."""
    d = _c2_like()
    nb = len(d["x0"])
    with _ctx(2, True, tight=False, max_batch=nb) as c:
        on = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        y = c.farkas()
    with _ctx(0, False, tight=False, max_batch=nb) as c:
        ref = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
    print(f"C2-like: status counts {np.bincount(on[3], minlength=5).tolist()}, iterations {on[4].min()}..{on[4].max()}")
    assert (on[3] != 4).all()
    assert y.shape == (nb, 7 * N - 3) and not y.any()
    _assert_same_bits(on, ref, what="C2-like batch: ")


def test_toggling_restores_the_plain_kernel():
    """Item 4: on, then off, on one solver = 2 context: the off solve is bit-identical to a context
    that never had the detection on (and the on solve of the same context certifies)."""
    from vcmpc import _abi
    d = _problems()["d"]
    with _ctx(2, False) as c:
        never = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
    with _ctx(2, False) as c:
        c.set_infeasibility(True)
        on = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        c.set_infeasibility(False)
        off = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        with pytest.raises(_abi.VcError):
            c.farkas()
    np.testing.assert_array_equal(on[3], _run(2, True)[3])
    assert (off[3] != 4).all()
    _assert_same_bits(off, never, what="detection turned off again: ")
    # ... which is the condensed kernel: solver = 0 without the detection
    _assert_same_bits(never, _run(0, False)[:6], what="solver = 2 without the detection: ")


def test_device_pointers_and_solve_from():
    """Item 5: torch tensors on the device give the host-array results, certificates included;
    vc_solve_from leaves ubar_in untouched and returns it in u_out for the certified problems."""
    import torch
    d = _problems()["d"]
    host = _run(2, True)
    with _ctx(2, True) as c:
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
        r = c.solve(t["x0"], t["kappa"], t["ds"], t["ubar"].clone(), diag=True)
        y = c.farkas()
        torch.cuda.synchronize()
        assert isinstance(y, torch.Tensor) and y.is_cuda
        _assert_same_bits([a.cpu().numpy() for a in r], host[:6], what="device pointers: ")
        np.testing.assert_array_equal(y.cpu().numpy(), host[6])
        # vc_solve_from, device and host pointers
        u_out = torch.full_like(t["ubar"], -7.0)
        f = c.solve_from(t["x0"], t["kappa"], t["ds"], t["ubar"], u_out)
        yf = c.farkas()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(t["ubar"].cpu().numpy(), d["ubar"])
        _assert_same_bits([a.cpu().numpy() for a in f], host[:5], what="solve_from, device pointers: ")
        np.testing.assert_array_equal(yf.cpu().numpy(), host[6])
        ubar_in = d["ubar"].copy()
        u_host = np.full_like(ubar_in, -7.0)
        fh = c.solve_from(d["x0"], d["kappa"], d["ds"], ubar_in, u_host)
        yh = c.farkas()
    np.testing.assert_array_equal(ubar_in, d["ubar"])
    _assert_same_bits(fh, host[:5], what="solve_from, host pointers: ")
    np.testing.assert_array_equal(yh, host[6])
    cert = host[3] == 4
    assert cert.any()
    np.testing.assert_array_equal(u_host[cert], d["ubar"][cert])
    np.testing.assert_array_equal(u_out.cpu().numpy()[cert], d["ubar"][cert])


SIM_FAIL, SIM_GOOD, SIM_K = [6, 7], [0, 1, 2, 3, 4, 5], 4


@functools.lru_cache(maxsize=None)
def _simulate(max_iter):
    """vc_simulate (8 vehicles x 4 steps) on an N = 20 solver = 2 detection-on context -- the default
    config of tests/test_gpu_sim_bookkeeping.py's contexts, qp.max_iter as given (None: the config's
    own, 40) -- and the loop rebuilt on the host from the public calls:

        kap, ds        = ctx.horizon(x, xbar, MPC_DT)
        u0, xs, us, st = ctx.solve(x, kap, ds, ubar.copy())
        u_app          = where(st == 0, u0, 0)
        x_new          = ctx.drive(x.copy(), u_app, DT)
        solved         : ubar' = us,  xbar' = xs
        failed         : ubar' = 0,  xbar'[:, j] = x_new for every column j,  nfail += 1

    The vehicles: six from the closed-loop sampler on its warm start, one with v = 0 (the spatial ODE is
    singular: VC_NONFINITE) and one with delta0 = delta_max + 0.2, whose delta rows cannot be met; u = 0
    leaves both where they are, so they fail again at every step.  Computed once per setting and shared
    (never modified) by the tests."""
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    from vcmpc.environment import Track
    nv, K = 8, SIM_K
    track = Track.load("ippodromo")
    x0 = _kin_states(nv, track.length, 41)
    x0[6, 0] = 0.0                # v = 0
    x0[7, 1] = 0.3 + 0.2          # delta0 = delta_max + 0.2
    xbar0, ubar0 = _warm(nv, N, N + 1, 6, False, np.float64)
    cfg = load_config("kinematic_mpc")
    assert float(cfg["state_constraints"]["delta_max"]) == 0.3 and int(cfg["qp"]["max_iter"]) == 40
    cfg["qp"] = dict(cfg["qp"], solver=2, **({} if max_iter is None else {"max_iter": max_iter}))
    p = make_params(kin_car=load_config("kinematic_car"), kin_mpc=cfg)
    with Context(model=_abi.VC_MODEL_KINEMATIC, N=N, max_batch=nv, dtype=_abi.VC_F64, params=p,
                 detect_infeasible=True) as c:
        c.set_track(track)
        x, xbar, ubar = x0.copy(), xbar0.copy(), ubar0.copy()
        log_x, log_u, nfail = c.simulate(x, xbar, ubar, K, MPC_DT, DT, log=True)
        sim = dict(log_x=log_x, log_u=log_u, x=x, xbar=xbar, ubar=ubar, nfail=nfail)
        # the definition, step by step
        rx, rxbar, rubar = x0.copy(), xbar0.copy(), ubar0.copy()
        rnfail = np.zeros(nv, np.int32)
        rlog_x, rlog_u, stats, iters = [rx.copy()], [], [], []
        for _ in range(K):
            kap, ds = c.horizon(rx, rxbar, MPC_DT)
            u0, xs, us, st, it = c.solve(rx, kap, ds, rubar.copy())
            ok = st == 0
            u_app = np.ascontiguousarray(np.where(ok[:, None], u0, 0.0))
            x_new = c.drive(rx.copy(), u_app, DT)
            rubar, rxbar = us.copy(), xs.copy()
            rubar[~ok] = 0.0
            rxbar[~ok] = x_new[~ok, None, :]
            rnfail += (~ok).astype(np.int32)
            rlog_u.append(u_app)
            stats.append(st.copy())
            iters.append(it.copy())
            rx = x_new
            rlog_x.append(rx.copy())
    ref = dict(log_x=np.stack(rlog_x), log_u=np.stack(rlog_u), x=rx, xbar=rxbar, ubar=rubar, nfail=rnfail,
               status=np.stack(stats), iters=np.stack(iters))
    return sim, ref


SIM_CAPS = pytest.mark.parametrize("max_iter", [None, 80], ids=["max_iter_default", "max_iter_80"])


@SIM_CAPS
def test_simulate_equals_its_definition(max_iter):
    """Item 6, the bookkeeping: logs, final buffers and nfail of vc_simulate match the host loop bit
    for bit; the two failing vehicles fail at every step and are driven with u = 0."""
    sim, ref = _simulate(max_iter)
    print(f"status per step {ref['status'].tolist()}, nfail {sim['nfail'].tolist()}")
    assert (ref["status"][:, SIM_FAIL] != 0).all(), ref["status"]
    np.testing.assert_array_equal(sim["nfail"][SIM_FAIL], SIM_K)
    assert not sim["log_u"][:, SIM_FAIL].any()
    assert (sim["nfail"][SIM_GOOD] == 0).sum() >= 4, sim["nfail"]  # a condition of the test: the sampled vehicles solve
    for k in ("log_x", "log_u", "x", "xbar", "ubar", "nfail"):
        np.testing.assert_array_equal(sim[k], ref[k], err_msg=k)


@SIM_CAPS
def test_simulate_failing_vehicles_status(max_iter):
    """Item 6, the status: the failing vehicles end [2, 4] -- VC_NONFINITE, VC_INFEASIBLE -- at every
    step, under the config's own cap of 40 iterations and under 80.

    Measured on an MI355X: [2, 4] at every step, the delta vehicle certified at iterations 7, 19, 11,
    17 at either cap.  This is what the completed certificate is in the kernel for.  After the first step
    the failure restart puts the vehicle's own speed into the warm start (ds = 0.71 m per stage): with
    delta = 0.5 rad held the 20-stage prediction turns by about 3 rad and passes cos(epsi) = 0, where
    the spatial model is singular; the QP's residual starts at 1e7 .. 1e8, the interior point's box
    multipliers stay out of line with its row multipliers, and y = lam / |lam|_1 alone satisfies the
    criterion only at iterations 16, 58, 45, 59 -- past the cap on three of the four steps, which then
    ended VC_MAX_ITER ([2, 1]; the stagewise kernel, whose test has lam / |lam|_1 only, still gives
    [2, 4], [2, 1], [2, 1], [2, 1] on the same loop).  phase 1 of oracle/feasibility.py finds all four
    QPs infeasible (t* = 0.158, 0.142, 0.142, 0.142, Farkas-checked)."""
    sim, ref = _simulate(max_iter)
    print(f"status per step {ref['status'].tolist()}, iterations of vehicle 7 {ref['iters'][:, 7].tolist()}")
    assert (ref["status"][:, SIM_FAIL] == np.array([2, 4])).all(), ref["status"]


def test_controller_counts_certified_steps():
    """Item 7: BatchedKinematicMPC at horizon 20 with qp: {solver: 2, detect_infeasible: true}.
    Vehicles whose steering angle 0.25 rad is far outside a +-0.05 box have no feasible first stage, so
    the first solve is certified and counted in infeasible_steps, and the neutral retry takes over as
    for any other status != 0.  As in tests/test_gpu_infeasible.py the zero-miss assertion holds where
    the zero-miss condition is stated: max_iter = 80 and a warm-start rollout inside the workload
    sampler's domain (v > 1 m/s along the horizon)."""
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
    cfg["horizon"] = N
    cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
    cfg["qp"] = dict(cfg.get("qp") or {}, max_iter=MAX_ITER, solver=2, detect_infeasible=True)
    on = KM.BatchedKinematicMPC(car, cfg, batch=n)
    assert on.detect_infeasible and on.ctx.detect_infeasible and on.ctx.params.qp.solver == 2
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
    # the retry ran for them (status is the retry's) and left a finite command and a finite plan
    assert np.isfinite(u_on).all()
    assert np.isfinite(on.action_prediction).all() and np.isfinite(on.state_prediction).all()
    on.ctx.close()
