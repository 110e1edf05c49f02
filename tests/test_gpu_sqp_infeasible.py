"""GPU: in-kernel infeasibility detection of the fp64 single-track SQP (csrc/st_sqp.hip,
vc_set_sqp_infeasibility / vc_get_sqp_farkas), against the phase-1 LP certificates of
oracle/feasibility.py on the oracle's own rows (oracle/dyn_sqp.py dyn_qp).

Problem set P(N): dynamic_batch(32, N, seed=77) in fp64 under singletrack_mpc.yaml with the delta box
at +-0.05 rad and qp.max_iter = 80: more than half of the first QPs have no feasible point (20 of 32
at N = 20, 18 of 32 at N = 60 with the linear tyre; smallest phase-1 optimum t* 1.3e-3 / 2.5e-4).

The criterion (y = lam / |lam|_1, R = sum_k [trust_Fx / S + max(0, up_k, dn_k)] from the Fx trust
region and the trust-tightened w box):
    d'y + R |C'y|_inf < 0   =>   no dz satisfies C dz <= d
is re-evaluated here in numpy with the oracle's C and d for every vector the kernel returns, with no
slack.
"""
import functools

import numpy as np
import pytest

from oracle import dyn_sqp as D

pytestmark = pytest.mark.gpu

U_TOL = 1e-5
B = 32
MAX_ITER = 80


def _cfg(**qp):
    from vcmpc.config import load_config
    cfg = load_config("singletrack_mpc")
    cfg["qp"] = dict(cfg.get("qp") or {}, max_iter=MAX_ITER, **qp)
    cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
    return cfg


def _ctx(N, detect, tyre="linear", cfg=None, max_batch=B):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=cfg if cfg is not None else _cfg(), tyre=tyre)
    return Context(model=_abi.VC_MODEL_DYNAMIC, N=N, max_batch=max_batch, dtype=_abi.VC_F64, params=p,
                   detect_infeasible=detect)


@functools.lru_cache(maxsize=None)
def _dyn_params():
    from oracle import models as M
    from vcmpc.config import load_config
    return M.dyn_params_from_config(load_config("dynamic_car"))


def _box_radius(dvec, N):
    """R of the criterion from the oracle's right-hand sides: rows per stage [3 state rows (k >= 1),
    5 stage-function rows, w up, w dn, Fx up, Fx dn]."""
    R = 0.0
    for k in range(N):
        w_up = (12 * k - 3 if k >= 1 else 0) + (8 if k >= 1 else 5)
        R += dvec[w_up + 2] + max(0.0, dvec[w_up], dvec[w_up + 1])
    return R


@functools.lru_cache(maxsize=None)
def _problems(N, tyre="linear"):
    """P(N) with the oracle's truth: rows C, d of the first QP and their phase-1 verdicts.  Computed
    once per (horizon, tyre) and shared (never modified) by the tests."""
    from oracle.feasibility import phase1
    from vcmpc.workload import dynamic_batch
    W = D.dyn_weights(_cfg())
    d = {k: v.astype(np.float64) for k, v in dynamic_batch(B, N=N, seed=77).items()}
    Qd = D.dyn_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], _dyn_params(), W, tyre)
    assert Qd["C"].shape == (B, 12 * N - 3, 2 * N)
    cert = [phase1(Qd["C"][b], Qd["d"][b]) for b in range(B)]
    infeasible = np.array([not c["feasible"] for c in cert])
    assert all(c["farkas_ok"] for c, i in zip(cert, infeasible) if i)  # the truth is itself certified
    return dict(d=d, C=Qd["C"], dvec=Qd["d"], infeasible=infeasible, feasible_idx=np.nonzero(~infeasible)[0],
                t=np.array([c["t"] for c in cert]))


@functools.lru_cache(maxsize=None)
def _oracle_u(N):
    """u* of the oracle's SQP on the phase-1-feasible problems of P(N) (N = 20 only: 9 s)."""
    P = _problems(N)
    d, fe = P["d"], P["feasible_idx"]
    ref = D.dyn_sqp_solve(d["x0"][fe], d["ubar"][fe], d["kappa"][fe], d["ds"][fe], _dyn_params(),
                          D.dyn_weights(_cfg()), "linear")
    return ref["u_star"]


@functools.lru_cache(maxsize=None)
def _run(N, detect, tyre="linear"):
    """One host-pointer solve of P(N); (u0, x*, u*, status, iters, diag, y or None, qp_index or None)."""
    d = _problems(N, tyre)["d"]
    with _ctx(N, detect, tyre) as c:
        r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        y, qi = c.sqp_farkas() if detect else (None, None)
    return tuple(r) + (y, qi)


def _check_status_and_certificates(P, N, run):
    u0, xs, us, st, it, dg, y, qi = run
    d, inf = P["d"], P["infeasible"]
    print(f"N={N}: {int(inf.sum())} of {B} first QPs infeasible (smallest t* {P['t'][inf].min():.2e}); status on them "
          f"{np.bincount(st[inf], minlength=5).tolist()}, on the feasible {np.bincount(st[~inf], minlength=5).tolist()} "
          f"(counts of status 0..4); iterations of the infeasible {sorted(it[inf].tolist())}")
    false_pos = np.nonzero(~inf & (st == 4))[0]
    miss = np.nonzero(inf & (st != 4))[0]
    assert len(false_pos) == 0, f"status 4 on feasible problems {false_pos.tolist()}"
    assert len(miss) == 0, f"oracle-infeasible problems not detected {miss.tolist()}: status {st[miss].tolist()}"
    assert y.shape == (B, 12 * N - 3) and qi.shape == (B,)
    worst = -np.inf
    for b in np.nonzero(st == 4)[0]:
        yb, C, dv = y[b], P["C"][b], P["dvec"][b]
        assert (yb >= 0.0).all()
        assert abs(yb.sum() - 1.0) <= 1e-12
        val = float(dv @ yb + _box_radius(dv, N) * np.abs(C.T @ yb).max())
        worst = max(worst, val)
        assert val < 0.0, (int(b), val)
        assert qi[b] == 0
        assert it[b] < MAX_ITER
        np.testing.assert_array_equal(us[b], d["ubar"][b])   # u* is the warm start, bit for bit
        np.testing.assert_array_equal(u0[b], d["ubar"][b, 0])
        assert np.isfinite(xs[b]).all()
        assert int(dg[b, 2]) & 32
    rest = st != 4
    assert not y[rest].any()
    assert (qi[rest] == -1).all()
    print(f"N={N}: largest certificate value {worst:.3e}; iterations of the infeasible mean {it[inf].mean():.1f} "
          f"max {it[inf].max()}")


@pytest.mark.parametrize("N", [20, 60])
def test_status_and_certificates(N):
    """Test 1: status 4 exactly on the phase-1-infeasible problems (no miss, no false positive), every
    returned vector a Farkas certificate by the host-side inequality, the output the warm start."""
    P = _problems(N)
    assert int(P["infeasible"].sum()) == {20: 20, 60: 18}[N]
    _check_status_and_certificates(P, N, _run(N, True))


@pytest.mark.parametrize("N", [20, 60])
def test_feasible_problems_unchanged(N):
    """Test 2: on the phase-1-feasible problems u*, status and iters are those of a detection-off run,
    bit for bit; at N = 20 u* is the oracle's."""
    P = _problems(N)
    fe = P["feasible_idx"]
    on, off = _run(N, True), _run(N, False)
    np.testing.assert_array_equal(on[2][fe], off[2][fe])
    np.testing.assert_array_equal(on[3][fe], off[3][fe])
    np.testing.assert_array_equal(on[4][fe], off[4][fe])
    assert (off[3] != 4).all()
    if N == 20:
        err = np.abs(on[2][fe] - _oracle_u(N)).max()
        print(f"N={N}: feasible |u* - u*_oracle| max {err:.2e}, status {on[3][fe].tolist()}")
        assert err < U_TOL


def test_off_is_the_parent():
    """Test 3: detection turned on and off again: the next solve is bit-identical to a context that
    never had it on, and vc_get_sqp_farkas refuses while it is off."""
    from vcmpc import _abi
    N = 20
    d = _problems(N)["d"]
    ref = _run(N, False)
    with _ctx(N, False) as c:
        assert not c.detect_infeasible
        with pytest.raises(_abi.VcError) as e:
            c.sqp_farkas(0)
        assert e.value.code == _abi.VC_E_ARG
        c.set_sqp_infeasibility(True)
        c.set_sqp_infeasibility(False)
        r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        with pytest.raises(_abi.VcError) as e:
            c.sqp_farkas()
        assert e.value.code == _abi.VC_E_ARG
        y = np.empty((B, 12 * N - 3))
        assert c.lib.vc_get_sqp_farkas(c._h, B, y.ctypes.data, None, _abi.VC_HOST_PTRS) == _abi.VC_E_ARG
    for a, b in zip(r, ref[:6]):
        np.testing.assert_array_equal(a, b)


def test_later_qp_path_is_consistent_with_detection_off():
    """Test 4: the bench's N = 60 batch (4096 problems, singletrack_mpc.yaml as it is), detection off
    and on: every certified problem was non-solved before, everything else keeps its status and u*,
    and a certificate only ever shortens the interior point."""
    from vcmpc.config import load_config
    from vcmpc.workload import dynamic_batch
    Bn, N = 4096, 60
    cfg = load_config("singletrack_mpc")
    d = {k: v.astype(np.float64) for k, v in dynamic_batch(Bn, N=N, seed=31).items()}
    out = {}
    for on in (False, True):
        with _ctx(N, on, cfg=cfg, max_batch=Bn) as c:
            out[on] = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
            if on:
                y, qi = c.sqp_farkas()
    (_, _, us0, st0, it0, dg0), (_, _, us1, st1, it1, dg1) = out[False], out[True]
    s4 = st1 == 4
    b32 = (dg1[:, 2].astype(int) & 32) > 0
    b16 = (dg1[:, 2].astype(int) & 16) > 0
    print(f"N=60 B={Bn}: status off {np.bincount(st0, minlength=5).tolist()} on {np.bincount(st1, minlength=5).tolist()}; "
          f"certified {int(b32.sum())}, of them qp_index > 0: {int((qi > 0).sum())} (qp_index {qi[b32].tolist()}); "
          f"iterations of the certified off {it0[b32].tolist()} on {it1[b32].tolist()}")
    assert (st0[s4] != 0).all()
    np.testing.assert_array_equal(st1[~s4], st0[~s4])
    np.testing.assert_array_equal(us1[~s4], us0[~s4])
    assert (~b32 | b16 | s4).all()
    assert (it1 <= it0).all()
    assert (it1[b32] < it0[b32]).all()
    assert ((qi >= 0) == b32).all() and (qi[s4] == 0).all() and (qi[b32 & ~s4] > 0).all()
    assert not y[~b32].any()


def test_device_tensors_equal_host_arrays():
    """Test 5: torch tensors on the device give the status, y and qp_index of the host-array run."""
    import torch
    N = 20
    d = _problems(N)["d"]
    host = _run(N, True)
    with _ctx(N, True) as c:
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
        r = c.solve(t["x0"], t["kappa"], t["ds"], t["ubar"])
        y, qi = c.sqp_farkas()
        torch.cuda.synchronize()
        assert isinstance(y, torch.Tensor) and y.is_cuda and isinstance(qi, torch.Tensor) and qi.is_cuda
        st, yh, qh = r[3].cpu().numpy(), y.cpu().numpy(), qi.cpu().numpy()
    np.testing.assert_array_equal(st, host[3])
    np.testing.assert_array_equal(yh, host[6])
    np.testing.assert_array_equal(qh, host[7])


def test_refusals():
    """Test 6: kinematic and cascaded contexts are unsupported, trust_Fx = 0 is an argument error; the
    kinematic entry point keeps refusing a dynamic context."""
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    with Context(model=_abi.VC_MODEL_KINEMATIC, N=20, max_batch=4, kin_car=load_config("kinematic_car"),
                 kin_mpc=load_config("kinematic_mpc")) as c:
        assert c.lib.vc_set_sqp_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
        with pytest.raises(_abi.VcError) as e:
            c.set_sqp_infeasibility(True)
        assert e.value.code == _abi.VC_E_UNSUPPORTED
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("cascaded_mpc"), tyre="fiala")
    with Context(model=_abi.VC_MODEL_CASCADED, N=20, max_batch=4, dtype=_abi.VC_F64, params=p) as c:
        assert c.lib.vc_set_sqp_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
    with _ctx(20, False, cfg=_cfg(trust_Fx=0.0)) as c:
        assert c.lib.vc_set_sqp_infeasibility(c._h, 1, 0.0) == _abi.VC_E_ARG
        assert c.lib.vc_set_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
    with pytest.raises(_abi.VcError) as e:
        _ctx(20, True, cfg=_cfg(trust_Fx=0.0))
    assert e.value.code == _abi.VC_E_ARG


def test_fiala_tyre():
    """Test 7: test 1's checks with the Fiala tyre at N = 20, the truth recomputed by phase 1 on
    dyn_qp(..., "fiala")."""
    N = 20
    P = _problems(N, "fiala")
    assert int(P["infeasible"].sum()) >= 4
    _check_status_and_certificates(P, N, _run(N, True, "fiala"))


def test_detection_global_j_bit_identical():
    """Test 9: st_sqp_kernel<60, linear, JG = true, DET = true>.  P(60) tiled 32 times to B = 1024 is
    beyond the 768 problems the LDS-J kernel takes (csrc/st_sqp.hip st_jg_pick), so the launch runs the
    global-J kernel with the detection on.  J placement moves data, not arithmetic: every tile must
    equal the 32-problem LDS-J run of test 1 bit for bit -- status, iters, u*, x*, u0, diag, the Farkas
    vector and qp_index -- so a per-problem addressing error in the J or the Farkas workspace at any
    problem index shows as a mismatch (the pattern of test_gpu_st_sqp.py
    test_st_sqp_j_placement_bit_identical).  Measured on an MI355X: identical; 448 solved and 576
    certified (18 per tile) of 1024."""
    N, T = 60, 32
    small = _run(N, True)
    d = {k: np.ascontiguousarray(np.concatenate([v] * T)) for k, v in _problems(N)["d"].items()}
    assert len(d["x0"]) == T * B > 768
    with _ctx(N, True, max_batch=T * B) as c:
        big = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        y, qi = c.sqp_farkas()
    big = tuple(big) + (y, qi)
    print(f"N={N} B={T * B} global J + detection: status counts {np.bincount(big[3], minlength=5).tolist()}, "
          f"certified {int((qi >= 0).sum())}")
    assert (small[3] == 4).sum() == 18   # the tiles carry certificates to compare
    for a, s in zip(big, small):
        np.testing.assert_array_equal(a, np.concatenate([s] * T))


def test_controller_config_key_enables_detection():
    """Test 8: `qp.detect_infeasible` of the single-track controller config turns the detection on
    (default off); a step whose first QP is certified is counted and restarts neutrally like every
    other non-solved status.  Vehicles whose steering angle 0.25 rad is far outside a +-0.05 box have
    no feasible first QP (w moves delta by ~0.006 rad per stage); the truth is phase 1 on the oracle's
    rows of the very warm start command() builds."""
    from oracle.feasibility import phase1
    from vcmpc.config import load_config
    from vcmpc.controllers import cascaded_mpc as CM
    from vcmpc.environment import CurvatureTrack
    from vcmpc.models import DynamicCar
    n, N = 6, 20
    car = DynamicCar(load_config("dynamic_car"), CurvatureTrack(constant=1 / 60), tyre="linear")
    x0 = np.zeros((n, 8))
    x0[:, 0] = np.linspace(10.0, 18.0, n)
    x0[:, 3] = 0.25
    x0[:, 4] = 6.0
    cfg = _cfg()
    cfg["horizon"] = N
    off = CM.BatchedSingleTrackMPC(car, cfg, batch=n)
    assert not off.detect_infeasible and not off.ctx.detect_infeasible
    u_off = off.command(x0)
    assert (off.infeasible_steps == 0).all()
    cfg["qp"] = dict(cfg["qp"], detect_infeasible=True)
    on = CM.BatchedSingleTrackMPC(car, cfg, batch=n)
    assert on.detect_infeasible and on.ctx.detect_infeasible
    # the first solve's inputs as command() builds them, and the oracle's verdict on its first QP
    ds, kappa = CM.dyn_horizon_params(x0[:, 4], on.state_prediction[:, 0, :], on.dt, car.track.k)
    ubar = np.ascontiguousarray(np.swapaxes(on.action_prediction, 1, 2))
    ic = cfg["input_constraints"]
    np.clip(ubar[..., 1], ic["w_min"], ic["w_max"], out=ubar[..., 1])
    Qd = D.dyn_qp(x0, ubar, kappa, ds, _dyn_params(), D.dyn_weights(cfg), "linear")
    assert D.in_domain(Qd["xbar"], kappa).all()
    truth = np.array([not phase1(Qd["C"][b], Qd["d"][b])["feasible"] for b in range(n)])
    assert truth.all()
    u_on = on.command(x0)
    print(f"controller: infeasible first solves {on.infeasible_steps.tolist()}, status after the retry "
          f"{on.status.tolist()} (detection off: {off.status.tolist()})")
    np.testing.assert_array_equal(on.infeasible_steps, truth.astype(np.int64))
    # the neutral retry took over; where it is not solved either (the steering angle is still outside
    # its box), the step is the neutral restart: u = 0, the next warm start the current state
    bad = on.status != 0
    assert (u_on[bad] == 0.0).all() and (on.action_prediction[bad] == 0.0).all()
    np.testing.assert_array_equal(on.state_prediction[bad], np.repeat(x0[bad, :, None], N, axis=2))
    assert np.isfinite(u_on).all() and np.isfinite(u_off).all()
