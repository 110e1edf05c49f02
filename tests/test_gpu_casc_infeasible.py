"""GPU: in-kernel infeasibility detection of the stagewise cascaded SQP (csrc/casc_ric.hip,
vc_set_casc_infeasibility / vc_get_casc_farkas), against the phase-1 LP certificates of
oracle/feasibility.py on the oracle's own rows (oracle/casc_sqp.py casc_qp).

Problem sets, 32 problems each under cascaded_mpc.yaml (qp.max_iter = 80), N = 20:
    Pd(M, seed, tyre): cascaded_batch(32, M, seed, tyre) with the delta box at +-0.05 rad
    PV(M, tyre):       cascaded_batch(32, M, 77, tyre) with state_pm_constraints.V_min = 14
About half of the first QPs of each set have no feasible point (counts asserted in test 1; smallest
phase-1 optimum t* 1.3e-3 over all sets).  PV's infeasibility comes from the point-mass rows alone:
the same problems are phase-1 feasible under the default V_min, so a certificate must weigh the
V >= V_min rows, which pins the kernel's point-mass row mapping.

The criterion (y = lam / |lam|_1, S = fx_scale):
    R = sum_{k<N} [trust_Fx / S + max(0, up_k, dn_k)] + sum_{m<M} 2 trust_Fx / S
    d'y + R |C'y|_inf < 0   =>   no dz satisfies C dz <= d
is re-evaluated here in numpy with the oracle's C and d for every vector the kernel returns, with no
slack.  Rows (m = 12N - 3 + 6M): the single-track stages as oracle/dyn_sqp.py dyn_qp lays them out,
then per point-mass stage [V >= V_min, Fx <= Peng / V, Fx up, Fx dn, Fy up, Fy dn].

Instantiation coverage (casc_ric_kernel<20, M, tyre, JG, DET = true>; LDS J up to 768 problems,
global J beyond, M = 35 / 40 only):
    M   tyre    J       test
    15  fiala   LDS     test_status_and_certificates[Pd-15-77-fiala], [PV-15-77-fiala]
    15  linear  LDS     test_status_and_certificates[Pd-15-77-linear], [PV-15-77-linear]
    25  fiala   LDS     test_status_and_certificates[PV-25-77-fiala]
    25  linear  LDS     test_status_and_certificates[PV-25-77-linear]
    35  fiala   LDS     test_status_and_certificates[PV-35-77-fiala]
    35  linear  LDS     test_status_and_certificates[PV-35-77-linear]
    40  fiala   LDS     test_status_and_certificates[Pd-40-78-fiala], [PV-40-77-fiala]
    40  linear  LDS     test_status_and_certificates[PV-40-77-linear]
    35  fiala   global  test_detection_global_j_bit_identical[35-fiala]
    35  linear  global  test_detection_global_j_bit_identical[35-linear]
    40  fiala   global  test_detection_global_j_bit_identical[40-fiala], test_later_qp_path_...
    40  linear  global  test_detection_global_j_bit_identical[40-linear]
"""
import functools

import numpy as np
import pytest

from oracle import casc_sqp as CS

pytestmark = pytest.mark.gpu

U_TOL = 1e-5
B = 32
N = 20
MAX_ITER = 80

# (kind, M, seed, tyre) -> infeasible of 32 (None: at least 4, counted at test time)
SETS = {
    ("Pd", 15, 77, "fiala"): 16,
    ("Pd", 15, 77, "linear"): 17,
    ("Pd", 40, 78, "fiala"): 19,
    ("PV", 15, 77, "fiala"): 18,
    ("PV", 25, 77, "fiala"): 14,
    ("PV", 35, 77, "fiala"): 16,
    ("PV", 40, 77, "fiala"): 13,
    ("PV", 15, 77, "linear"): 17,
    ("PV", 25, 77, "linear"): None,
    ("PV", 35, 77, "linear"): None,
    ("PV", 40, 77, "linear"): None,
}
SET_IDS = ["-".join(str(v) for v in s) for s in SETS]


def _rows(M):
    return 12 * N - 3 + 6 * M


def _scale(M):
    s = np.ones((N + M, 2))
    s[:, 0] = 1000.0
    s[N:, 1] = 1000.0
    return s


def _cfg(kind, M, **qp):
    from vcmpc.config import load_config
    cfg = load_config("cascaded_mpc")
    cfg["horizon_pm"] = M
    assert cfg["qp"]["max_iter"] == MAX_ITER
    cfg["qp"] = dict(cfg["qp"], **qp)
    if kind == "Pd":
        cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
    elif kind == "PV":
        cfg["state_pm_constraints"] = dict(cfg["state_pm_constraints"], V_min=14)
    else:
        assert kind is None
    return cfg


def _ctx(kind, M, detect, tyre="fiala", cfg=None, max_batch=B):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=cfg if cfg is not None else _cfg(kind, M), tyre=tyre)
    return Context(model=_abi.VC_MODEL_CASCADED, N=N, max_batch=max_batch, dtype=_abi.VC_F64, params=p,
                   detect_infeasible=detect)


@functools.lru_cache(maxsize=None)
def _dyn_params():
    from oracle import models as M
    from vcmpc.config import load_config
    return M.dyn_params_from_config(load_config("dynamic_car"))


def _box_radius(dvec, M):
    """R of the criterion from the oracle's right-hand sides.  Single-track stage: [3 state rows
    (k >= 1), 5 stage-function rows, w up, w dn, Fx up, Fx dn]; point-mass stage: [V, Peng, Fx up,
    Fx dn, Fy up, Fy dn]."""
    R = 0.0
    for k in range(N):
        w_up = (12 * k - 3 if k >= 1 else 0) + (8 if k >= 1 else 5)
        R += dvec[w_up + 2] + max(0.0, dvec[w_up], dvec[w_up + 1])
    for m in range(M):
        base = 12 * N - 3 + 6 * m
        R += dvec[base + 2] + max(0.0, dvec[base + 4], dvec[base + 5])
    return R


def _certificate_value(C, dvec, y, M):
    return float(dvec @ y + _box_radius(dvec, M) * np.abs(C.T @ y).max())


@functools.lru_cache(maxsize=None)
def _problems(kind, M, seed, tyre):
    """One problem set with the oracle's truth: rows C, d of the first QP and their phase-1 verdicts
    (for PV also the verdicts under the default V_min).  Computed once per set and shared (never
    modified) by the tests."""
    from oracle.feasibility import phase1
    from vcmpc.workload import cascaded_batch
    d = cascaded_batch(B, M=M, seed=seed, tyre=tyre)
    Q = CS.casc_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], _dyn_params(), CS.casc_weights(_cfg(kind, M)), tyre)
    assert Q["C"].shape == (B, _rows(M), 2 * (N + M))
    cert = [phase1(Q["C"][b], Q["d"][b]) for b in range(B)]
    infeasible = np.array([not c["feasible"] for c in cert])
    assert all(c["farkas_ok"] for c, i in zip(cert, infeasible) if i)  # the truth is itself certified
    out = dict(d=d, C=Q["C"], dvec=Q["d"], infeasible=infeasible, feasible_idx=np.nonzero(~infeasible)[0],
               t=np.array([c["t"] for c in cert]))
    if kind == "PV":
        Q0 = CS.casc_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], _dyn_params(), CS.casc_weights(_cfg(None, M)), tyre)
        out["feasible_default"] = np.array([phase1(Q0["C"][b], Q0["d"][b])["feasible"] for b in range(B)])
    return out


@functools.lru_cache(maxsize=None)
def _oracle_u():
    """u* of the oracle's SQP on the phase-1-feasible problems of Pd(15, 77, fiala) (8 s), with the
    run's cleanliness asserted first: every QP polished, none stopped, x* inside the domain."""
    P = _problems("Pd", 15, 77, "fiala")
    d, fe = P["d"], P["feasible_idx"]
    ref = CS.casc_sqp_solve(d["x0"][fe], d["ubar"][fe], d["kappa"][fe], d["ds"][fe], _dyn_params(),
                            CS.casc_weights(_cfg("Pd", 15)), tyre="fiala")
    for rec in ref["hist"]:
        assert np.asarray(rec["polished"], bool).all()
        assert not np.asarray(rec["stopped"], bool).any()
    assert np.asarray(ref["in_domain"], bool).all()
    return ref["u_star"]


@functools.lru_cache(maxsize=None)
def _run(kind, M, seed, tyre, detect):
    """One host-pointer solve of a set; (u0, x*, u*, status, iters, diag, y or None, qp_index or None)."""
    d = _problems(kind, M, seed, tyre)["d"]
    with _ctx(kind, M, detect, tyre) as c:
        r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        y, qi = c.casc_farkas() if detect else (None, None)
    return tuple(r) + (y, qi)


@pytest.mark.parametrize("kind,M,seed,tyre", list(SETS), ids=SET_IDS)
def test_status_and_certificates(kind, M, seed, tyre):
    """Test 1: status 4 exactly on the phase-1-infeasible problems (no miss, no false positive), every
    returned vector a Farkas certificate by the host-side inequality, the output the warm start."""
    P = _problems(kind, M, seed, tyre)
    d, inf = P["d"], P["infeasible"]
    want = SETS[(kind, M, seed, tyre)]
    if want is None:
        assert int(inf.sum()) >= 4
    else:
        assert int(inf.sum()) == want
    u0, xs, us, st, it, dg, y, qi = _run(kind, M, seed, tyre, True)
    print(f"{kind}({M}, {seed}, {tyre}): {int(inf.sum())} of {B} first QPs infeasible (smallest t* "
          f"{P['t'][inf].min():.2e}); status on them {np.bincount(st[inf], minlength=5).tolist()}, on the feasible "
          f"{np.bincount(st[~inf], minlength=5).tolist()} (counts of status 0..4); iterations of the infeasible "
          f"{sorted(it[inf].tolist())}")
    false_pos = np.nonzero(~inf & (st == 4))[0]
    miss = np.nonzero(inf & (st != 4))[0]
    assert len(false_pos) == 0, f"status 4 on feasible problems {false_pos.tolist()}"
    assert len(miss) == 0, f"oracle-infeasible problems not detected {miss.tolist()}: status {st[miss].tolist()}"
    assert y.shape == (B, _rows(M)) and qi.shape == (B,)
    if kind == "PV":
        assert P["feasible_default"].all()   # only the point-mass V >= V_min rows make the set infeasible
    worst = -np.inf
    for b in np.nonzero(st == 4)[0]:
        yb = y[b]
        assert (yb >= 0.0).all()
        assert abs(yb.sum() - 1.0) <= 1e-12
        val = _certificate_value(P["C"][b], P["dvec"][b], yb, M)
        worst = max(worst, val)
        assert val < 0.0, (int(b), val)
        assert qi[b] == 0
        assert it[b] < MAX_ITER
        np.testing.assert_array_equal(us[b], d["ubar"][b])   # u* is the warm start, bit for bit
        np.testing.assert_array_equal(u0[b], d["ubar"][b, 0])
        assert np.isfinite(xs[b]).all()
        assert int(dg[b, 2]) & 32
        if kind == "PV":
            assert yb[12 * N - 3::6].sum() > 0.0   # weight on the point-mass V >= V_min rows
    rest = st != 4
    assert not y[rest].any()
    assert (qi[rest] == -1).all()
    print(f"{kind}({M}, {seed}, {tyre}): largest certificate value {worst:.3e}; iterations to the certificate mean "
          f"{it[inf].mean():.1f} max {it[inf].max()}")


@pytest.mark.parametrize("kind,M,seed,tyre", list(SETS), ids=SET_IDS)
def test_feasible_problems_unchanged(kind, M, seed, tyre):
    """Test 2: on the phase-1-feasible problems u*, status and iters are those of a detection-off run,
    bit for bit, and off never reports 4; on Pd(15, 77, fiala) u* is the oracle's."""
    P = _problems(kind, M, seed, tyre)
    fe = P["feasible_idx"]
    on, off = _run(kind, M, seed, tyre, True), _run(kind, M, seed, tyre, False)
    np.testing.assert_array_equal(on[2][fe], off[2][fe])
    np.testing.assert_array_equal(on[3][fe], off[3][fe])
    np.testing.assert_array_equal(on[4][fe], off[4][fe])
    assert (off[3] != 4).all()
    if (kind, M, seed, tyre) == ("Pd", 15, 77, "fiala"):
        assert len(fe) == 16
        err = np.abs((on[2][fe] - _oracle_u()) / _scale(M)).max()
        print(f"Pd(15, 77, fiala): feasible scaled |u* - u*_oracle| max {err:.2e}, status {on[3][fe].tolist()}")
        assert err < U_TOL


def test_off_is_the_parent():
    """Test 3: detection turned on and off again: the next solve is bit-identical to a context that
    never had it on, and vc_get_casc_farkas refuses while it is off."""
    from vcmpc import _abi
    s = ("Pd", 15, 77, "fiala")
    d = _problems(*s)["d"]
    ref = _run(*s, False)
    with _ctx("Pd", 15, False) as c:
        assert not c.detect_infeasible
        with pytest.raises(_abi.VcError) as e:
            c.casc_farkas(0)
        assert e.value.code == _abi.VC_E_ARG
        c.set_casc_infeasibility(True)
        assert c.detect_infeasible
        c.set_casc_infeasibility(False)
        r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        with pytest.raises(_abi.VcError) as e:
            c.casc_farkas()
        assert e.value.code == _abi.VC_E_ARG
        y = np.empty((B, _rows(15)))
        assert c.lib.vc_get_casc_farkas(c._h, B, y.ctypes.data, None, _abi.VC_HOST_PTRS) == _abi.VC_E_ARG
    for a, b in zip(r, ref[:6]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("M", [40, 15])
def test_later_qp_path_is_consistent_with_detection_off(M):
    """Test 4: the batch of test_gpu_casc_ric.py test_casc_ric_batch_properties (4096 problems, seed 9,
    cascaded_mpc.yaml as it is; M = 40 takes the global-J kernel, M = 15 the LDS-J one), detection off and on: every status-4 problem was non-solved before, everything
    else keeps its status and u*, a certificate only ever shortens the interior point, and where a
    later QP was refused the returned u* is the iterate that QP was linearised at: casc_qp rebuilt
    there is refuted by the returned vector."""
    from vcmpc.workload import cascaded_batch
    Bn = 4096
    cfg = _cfg(None, M)
    d = cascaded_batch(Bn, M=M, seed=9)
    out = {}
    for on in (False, True):
        with _ctx(None, M, on, cfg=cfg, max_batch=Bn) as c:
            out[on] = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
            if on:
                y, qi = c.casc_farkas()
    (_, _, us0, st0, it0, dg0), (_, _, us1, st1, it1, dg1) = out[False], out[True]
    s4 = st1 == 4
    b32 = (dg1[:, 2].astype(int) & 32) > 0
    b16 = (dg1[:, 2].astype(int) & 16) > 0
    later = np.nonzero(qi > 0)[0]
    print(f"M={M} B={Bn}: status off {np.bincount(st0, minlength=5).tolist()} on {np.bincount(st1, minlength=5).tolist()}; "
          f"certified {int(b32.sum())}, of them qp_index > 0: {len(later)} (qp_index {qi[b32].tolist()}); "
          f"iterations of the certified off {it0[b32].tolist()} on {it1[b32].tolist()}")
    assert (st0 != 0).sum() <= 8
    assert (st0[s4] != 0).all()
    np.testing.assert_array_equal(st1[~s4], st0[~s4])
    np.testing.assert_array_equal(us1[~s4], us0[~s4])
    assert (it1 <= it0).all()
    assert (it1[b32] < it0[b32]).all()
    assert ((qi >= 0) == b32).all() and (qi[s4] == 0).all() and b16[qi > 0].all()
    assert not y[~b32].any()
    W = CS.casc_weights(cfg)
    for b in np.nonzero(b32)[0]:
        # the refused QP's linearisation point: the warm start (status 4) or the returned iterate
        Q = CS.casc_qp(d["x0"][b:b + 1], us1[b:b + 1], d["kappa"][b:b + 1], d["ds"][b:b + 1], _dyn_params(), W, "fiala")
        val = _certificate_value(Q["C"][0], Q["d"][0], y[b], M)
        print(f"  problem {int(b)}: qp_index {int(qi[b])}, certificate value at the returned u* {val:.3e}")
        assert (y[b] >= 0.0).all() and abs(y[b].sum() - 1.0) <= 1e-12
        assert val < 0.0


@pytest.mark.parametrize("M,tyre", [(40, "fiala"), (35, "fiala"), (40, "linear"), (35, "linear")],
                         ids=["40-fiala", "35-fiala", "40-linear", "35-linear"])
def test_detection_global_j_bit_identical(M, tyre):
    """Test 5: casc_ric_kernel<20, M, tyre, JG = true, DET = true>.  PV(M) tiled 32 times to B = 1024
    is beyond the 768 problems the LDS-J kernel takes (csrc/casc_ric.hip cr_jg_pick), so the launch
    runs the global-J kernel with the detection on.  J placement moves data, not arithmetic: every
    tile must equal the 32-problem LDS-J run of test 1 bit for bit -- status, iters, u*, x*, u0, diag,
    the Farkas vector and qp_index."""
    T = 32
    s = ("PV", M, 77, tyre)
    small = _run(*s, True)
    d = {k: np.ascontiguousarray(np.concatenate([v] * T)) for k, v in _problems(*s)["d"].items()}
    assert len(d["x0"]) == T * B > 768
    with _ctx("PV", M, True, tyre, max_batch=T * B) as c:
        big = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        y, qi = c.casc_farkas()
    big = tuple(big) + (y, qi)
    print(f"M={M} {tyre} B={T * B} global J + detection: status counts {np.bincount(big[3], minlength=5).tolist()}, "
          f"certified {int((qi >= 0).sum())}")
    assert (small[3] == 4).sum() >= 4   # the tiles carry certificates to compare
    for a, sm in zip(big, small):
        np.testing.assert_array_equal(a, np.concatenate([sm] * T))


def test_device_tensors_equal_host_arrays():
    """Test 6: torch tensors on the device give the status, y and qp_index of the host-array run; a
    request for more rows than the last solve wrote is an argument error."""
    import torch
    from vcmpc import _abi
    s = ("PV", 15, 77, "fiala")
    d = _problems(*s)["d"]
    host = _run(*s, True)
    with _ctx("PV", 15, True, max_batch=2 * B) as c:
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
        r = c.solve(t["x0"], t["kappa"], t["ds"], t["ubar"])
        y, qi = c.casc_farkas()
        torch.cuda.synchronize()
        assert isinstance(y, torch.Tensor) and y.is_cuda and isinstance(qi, torch.Tensor) and qi.is_cuda
        st, yh, qh = r[3].cpu().numpy(), y.cpu().numpy(), qi.cpu().numpy()
        assert c.lib.vc_get_casc_farkas(c._h, B + 1, None, None, _abi.VC_DEVICE_PTRS) == _abi.VC_E_ARG
        yq = torch.empty((B, _rows(15)), dtype=torch.float64, device=y.device)   # qp_index may be NULL
        assert c.lib.vc_get_casc_farkas(c._h, B, yq.data_ptr(), None, _abi.VC_DEVICE_PTRS) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(yq.cpu().numpy(), yh)
    np.testing.assert_array_equal(st, host[3])
    np.testing.assert_array_equal(yh, host[6])
    np.testing.assert_array_equal(qh, host[7])


def test_refusals():
    """Test 7: kinematic and dynamic contexts, a tail the stagewise kernel is not built for and an
    explicit choice of the condensed kernel (qp.solver = 2) are unsupported; trust_Fx = 0 is an
    argument error, also through Context(detect_infeasible=True)."""
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    with Context(model=_abi.VC_MODEL_KINEMATIC, N=20, max_batch=4, kin_car=load_config("kinematic_car"),
                 kin_mpc=load_config("kinematic_mpc")) as c:
        assert c.lib.vc_set_casc_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
        with pytest.raises(_abi.VcError) as e:
            c.set_casc_infeasibility(True)
        assert e.value.code == _abi.VC_E_UNSUPPORTED
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("singletrack_mpc"), tyre="linear")
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=20, max_batch=4, dtype=_abi.VC_F64, params=p) as c:
        assert c.lib.vc_set_casc_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
    with _ctx(None, 20, False, max_batch=4) as c:    # M = 20: casc_ric.hip is not built for it
        assert c.lib.vc_set_casc_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
    with _ctx(None, 40, False, cfg=_cfg(None, 40, solver=2), max_batch=4) as c:
        assert c.lib.vc_set_casc_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
        # the setters of the other two controllers keep refusing a cascaded context
        assert c.lib.vc_set_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
        assert c.lib.vc_set_sqp_infeasibility(c._h, 1, 0.0) == _abi.VC_E_UNSUPPORTED
    with pytest.raises(_abi.VcError) as e:
        _ctx(None, 40, True, cfg=_cfg(None, 40, solver=2), max_batch=4)
    assert e.value.code == _abi.VC_E_UNSUPPORTED
    with _ctx(None, 40, False, cfg=_cfg(None, 40, trust_Fx=0.0), max_batch=4) as c:
        assert c.lib.vc_set_casc_infeasibility(c._h, 1, 0.0) == _abi.VC_E_ARG
    with pytest.raises(_abi.VcError) as e:
        _ctx(None, 40, True, cfg=_cfg(None, 40, trust_Fx=0.0), max_batch=4)
    assert e.value.code == _abi.VC_E_ARG


def _first_solve_inputs(ctl, x0):
    """(ds, kappa, ubar) of the first solve exactly as BatchedCascadedMPC.command() builds them."""
    from vcmpc.controllers import cascaded_mpc as CM
    ds, kappa = CM.casc_horizon_params(x0[:, 4], ctl.state_prediction[:, 0, :], ctl.dt, ctl.N, ctl.M, ctl.ds_pm,
                                       ctl.car.track.k)
    ubar = np.ascontiguousarray(np.swapaxes(ctl.action_prediction, 1, 2), dtype=np.float64)
    ubar[ctl._fresh, ctl.N:] = ctl._neutral(x0, kappa)[ctl._fresh, ctl.N:]
    ic = ctl.config["input_constraints"]
    np.clip(ubar[:, :ctl.N, 1], ic["w_min"], ic["w_max"], out=ubar[:, :ctl.N, 1])
    return ds, kappa, ubar


def test_controller_config_key_enables_detection():
    """Test 8: `qp.detect_infeasible` of the cascaded controller config turns the detection on
    (default off); a step whose first QP is certified is counted and restarts neutrally like every
    other non-solved status.  Vehicles whose steering angle 0.25 rad is far outside a +-0.05 box have
    no feasible first QP (w moves delta by ~0.006 rad per stage); the truth is phase 1 on the oracle's
    rows of the very warm start command() builds."""
    from oracle.feasibility import phase1
    from vcmpc.config import load_config
    from vcmpc.controllers import cascaded_mpc as CM
    from vcmpc.environment import CurvatureTrack
    from vcmpc.models import DynamicCar
    n, M = 6, 15
    car = DynamicCar(load_config("dynamic_car"), CurvatureTrack(constant=1 / 60), tyre="fiala")
    x0 = np.zeros((n, 8))
    x0[:, 0] = np.linspace(10.0, 18.0, n)
    x0[:, 3] = 0.25
    x0[:, 4] = 6.0
    cfg = _cfg("Pd", M)
    off = CM.BatchedCascadedMPC(car, cfg, batch=n)
    assert not off.detect_infeasible and not off.ctx.detect_infeasible
    u_off = off.command(x0)
    assert (off.infeasible_steps == 0).all()
    cfg["qp"] = dict(cfg["qp"], detect_infeasible=True)
    on = CM.BatchedCascadedMPC(car, cfg, batch=n)
    assert on.detect_infeasible and on.ctx.detect_infeasible
    ds, kappa, ubar = _first_solve_inputs(on, x0)
    Q = CS.casc_qp(x0, ubar, kappa, ds, _dyn_params(), CS.casc_weights(cfg), "fiala")
    assert CS.casc_in_domain(Q["xs"], Q["xp"], kappa).all()
    truth = np.array([not phase1(Q["C"][b], Q["d"][b])["feasible"] for b in range(n)])
    assert truth.all()
    u_on = on.command(x0)
    print(f"controller: infeasible first solves {on.infeasible_steps.tolist()}, status after the retry "
          f"{on.status.tolist()} (detection off: {off.status.tolist()})")
    np.testing.assert_array_equal(on.infeasible_steps, truth.astype(np.int64))
    # the neutral retry took over; where it is not solved either (the steering angle is still outside
    # its box), the step is the neutral restart: u = 0, the next warm start the current state on the
    # single-track stages with zero inputs there
    bad = on.status != 0
    assert (u_on[bad] == 0.0).all() and (on.action_prediction[bad][:, :, :N] == 0.0).all()
    np.testing.assert_array_equal(on.state_prediction[bad][:, :, :N], np.repeat(x0[bad, :, None], N, axis=2))
    assert np.isfinite(u_on).all() and np.isfinite(u_off).all()
    assert np.isfinite(on.state_prediction).all() and np.isfinite(on.action_prediction).all()
