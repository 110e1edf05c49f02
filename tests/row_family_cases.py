"""Problems on which one inequality-row family binds, for tests/test_row_families.py (CPU: the three
preconditions) and tests/test_gpu_row_families.py (GPU: the kernels against the same oracle solves).

A case is a straight-road problem (kappa = 0, warm start w = 0 and a flat Fx) plus the changes to the car
and controller configs that bring one family onto its bound.  Both sides read the same config dicts: the
kernels through make_params(dyn_car=..., dyn_mpc=...), the oracle through dyn_params_from_config /
dyn_weights (casc_weights, kin_weights).  A case runs the oracle twice -- as configured, and with
the family switched off through its parameters -- and `assert_preconditions` holds the pair to

  clean           every QP polished, no SQP stopped, x* in the domain
  binding         the family has a multiplier > 1e-6 in at least one QP
  discriminating  switching the family off moves u* by at least 100 x the bar of the kernel under test

so that a case on which the family is idle, or on which it hardly matters, cannot pass.
"""
import copy
import functools

import numpy as np

from oracle import casc_sqp as CS
from oracle import dyn_sqp as D
from oracle import families as F
from oracle import ltv_qp as Q
from oracle import models as M

MARGIN = 100.0          # discriminating: |u*_off - u*| >= MARGIN x the kernel's bar
N_ST = 20               # single-track stages of the fp64 and the cascaded cases

# family -> (config, path, value) that switches it off
OFF = {
    "peng": ("car", ("car", "Peng"), 1e12),
    "peng_pm": ("car", ("car", "Peng"), 1e12),
    "tyre_f_up": ("car", ("env", "mu", "f"), 1e3),
    "tyre_f_lo": ("car", ("env", "mu", "f"), 1e3),
    "tyre_r_up": ("car", ("env", "mu", "r"), 1e3),
    "tyre_r_lo": ("car", ("env", "mu", "r"), 1e3),
    "Ux_min": ("mpc", ("state_constraints", "Ux_min"), -1e9),
    "V_min": ("mpc", ("state_pm_constraints", "V_min"), -1e9),
    "v_min": ("mpc", ("state_constraints", "v_min"), -1e9),
    "delta_max": ("mpc", ("state_constraints", "delta_max"), 1e3),
    "delta_min": ("mpc", ("state_constraints", "delta_min"), -1e3),
}


def _set(cfg, path, value):
    for k in path[:-1]:
        cfg = cfg[k]
    cfg[path[-1]] = value


def _configs(car_name, mpc_name, changes):
    from vcmpc.config import load_config
    cfgs = {"car": load_config(car_name), "mpc": load_config(mpc_name)}
    for which, path, value in changes:
        _set(cfgs[which], path, value)
    return cfgs


def _off(cfgs, family):
    off = copy.deepcopy(cfgs)
    which, path, value = OFF[family]
    _set(off[which], path, value)
    return off


# -- single track ------------------------------------------------------------------------------------
# family -> (config changes, Ux, flat Fx warm start [N], delta0, ey0); see the coverage table of
# tests/test_gpu_row_families.py for what binds where
ST_CASES = {
    "tyre_f_lo": ((), 25.0, -10000.0, 0.0, 0.0),
    "tyre_r_lo": ((("car", ("car", "Xb", "f"), 0.5), ("car", ("car", "Xb", "r"), 0.5)), 25.0, -8000.0, 0.0, 0.0),
    "tyre_f_up": ((), 12.0, 6100.0, 0.0, 0.0),
    "tyre_r_up": ((("car", ("car", "Xd", "f"), 0.0), ("car", ("car", "Xd", "r"), 1.0)), 12.0, 7100.0, 0.0, 0.0),
    "peng": ((("car", ("car", "Peng"), 60000.0),), 15.0, 3800.0, 0.0, 0.0),
    "Ux_min": ((("mpc", ("state_constraints", "Ux_min"), 12.0),), 12.3, -2600.0, 0.0, 0.0),
    "delta_max": ((("mpc", ("state_constraints", "delta_max"), 0.02),), 12.0, 500.0, 0.01, -2.0),
    "delta_min": ((("mpc", ("state_constraints", "delta_min"), -0.02),), 12.0, 500.0, -0.01, 2.0),
}
ST_FAMILIES = tuple(ST_CASES)
# the fp32 kernel's, N = 40 (dynamic_mpc.yaml: prox 0.1, 3 SQP iterations).  Over 40 stages the optimum from
# 25 m/s brakes less than the tyres allow; from 35 - 40 m/s the terminal over-speed hinge (max_speed = 20) keeps
# it on the braking rows at every stage of every QP.  Ux_min: a warm start that QP 0 can bring back above 12
DYN_CASES = dict(ST_CASES, tyre_f_lo=((), 40.0, -11000.0, 0.0, 0.0),
                 tyre_r_lo=(ST_CASES["tyre_r_lo"][0], 35.0, -8500.0, 0.0, 0.0),
                 Ux_min=(ST_CASES["Ux_min"][0], 12.3, -1000.0, 0.0, 0.0))


def st_problem(N, Ux, Fx, delta0=0.0, ey0=0.0, dtype=np.float64):
    """One straight-road problem: x0 = [Ux, 0, 0, delta0, 50, ey0, 0, 0], ds = 0.03 Ux, warm start (Fx, 0);
    in float64, holding values that `dtype` (the kernel's input type) represents exactly."""
    x0 = np.array([[Ux, 0.0, 0.0, delta0, 50.0, ey0, 0.0, 0.0]])
    ubar = np.zeros((1, N, 2))
    ubar[..., 0] = Fx
    d = dict(x0=x0, kappa=np.zeros((1, N)), ds=np.full((1, N), 0.03 * Ux), ubar=ubar)
    return {k: v.astype(dtype).astype(np.float64) for k, v in d.items()}


def _st_solve(d, cfgs, tyre):
    return D.dyn_sqp_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], M.dyn_params_from_config(cfgs["car"]),
                           D.dyn_weights(cfgs["mpc"]), tyre)


@functools.lru_cache(maxsize=None)
def st_case(family, tyre, kernel="st_sqp", inputs=None):
    """The problem, its configs and the oracle's two answers; computed once and never modified.
    kernel "st_sqp": fp64, N = 20, singletrack_mpc.yaml, u* in (N, rad/s); "dyn_sqp": fp32, N = 40,
    dynamic_mpc.yaml, u* in the scaled variable (Fx / 1000, w) as tests/test_gpu_dyn_sqp.py states its bars."""
    N, mpc_name, scale, dtype = {"st_sqp": (N_ST, "singletrack_mpc", (1.0, 1.0), np.float64),
                                 "dyn_sqp": (40, "dynamic_mpc", (1000.0, 1.0), np.float32)}[kernel]
    changes, Ux, Fx, delta0, ey0 = (ST_CASES if kernel == "st_sqp" else DYN_CASES)[family] if inputs is None else inputs
    cfgs = _configs("dynamic_car", mpc_name, changes)
    d = st_problem(N, Ux, Fx, delta0, ey0, dtype)
    return dict(family=family, tyre=tyre, N=N, d=d, cfgs=cfgs, scale=np.array(scale),
                ref=_st_solve(d, cfgs, tyre), ref_off=_st_solve(d, _off(cfgs, family), tyre))


# -- cascaded: the single-track cases above on the first 20 stages, a straight point-mass tail behind ------
CASC_M = 15             # the smallest built tail


def casc_scale(Mh=CASC_M):
    s = np.ones((N_ST + Mh, 2))
    s[:, 0] = 1000.0
    s[N_ST:, 1] = 1000.0
    return s


def casc_problem(Ux, Fx, delta0=0.0, ey0=0.0, Fx_pm=None, Mh=CASC_M, ds_pm=3.0):
    """st_problem(20, ...) followed by Mh point-mass stages on the same straight road: ds = ds_pm, warm start
    Fy = 0 and a flat Fx_pm (default: the single-track part's Fx)."""
    d = st_problem(N_ST, Ux, Fx, delta0, ey0)
    u_pm = np.zeros((1, Mh, 2))
    u_pm[..., 0] = Fx if Fx_pm is None else Fx_pm
    return dict(x0=d["x0"], kappa=np.zeros((1, N_ST + Mh)), ds=np.concatenate([d["ds"], np.full((1, Mh), ds_pm)], 1),
                ubar=np.concatenate([d["ubar"], u_pm], 1))


def _casc_solve(d, cfgs, tyre):
    return CS.casc_sqp_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], M.dyn_params_from_config(cfgs["car"]),
                             CS.casc_weights(cfgs["mpc"]), tyre=tyre)


# family -> (config changes, Ux, Fx warm start of the single-track stages, delta0, ey0, Fx warm start of the tail).
# The tail takes over what the single-track cases' terminal cost did, so: braking rows from 35 - 40 m/s (terminal
# over-speed, as DYN_CASES); traction rows with a tail that keeps accelerating; the steering rows from outside
# the track boundary, whose cost is paid on the single-track stages; V_min a little under an entry speed above
# max_speed, where it stops the braking that the terminal over-speed hinge asks for.  The two power rows
# share one Peng and one switch, so each has a case on which the other is idle (asserted: IDLE): peng from just
# beyond the row with a tail held at 1500 N, peng_pm with the single-track part at half its limit
CASC_CASES = {
    "tyre_f_lo": ((), 40.0, -11000.0, 0.0, 0.0, -11000.0),
    "tyre_r_lo": (ST_CASES["tyre_r_lo"][0], 35.0, -8500.0, 0.0, 0.0, -8500.0),
    "tyre_f_up": ((), 12.0, 6100.0, 0.0, 0.0, 4000.0),
    "tyre_r_up": (ST_CASES["tyre_r_up"][0], 12.0, 7100.0, 0.0, 0.0, 4000.0),
    "peng": (ST_CASES["peng"][0], 15.0, 4100.0, 0.0, 0.0, 1500.0),
    "Ux_min": DYN_CASES["Ux_min"] + (None,),
    "delta_max": (ST_CASES["delta_max"][0], 12.0, 500.0, 0.01, -3.5, 500.0),
    "delta_min": (ST_CASES["delta_min"][0], 12.0, 500.0, -0.01, 3.5, 500.0),
    "V_min": ((("mpc", ("state_pm_constraints", "V_min"), 24.0),), 26.0, 500.0, 0.0, 0.0, 500.0),
    "peng_pm": (ST_CASES["peng"][0], 15.0, 2000.0, 0.0, 0.0, 3800.0),
}
CASC_FAMILIES = tuple(CASC_CASES)
# M = 40 (casc_sqp): over the 120 m tail the M = 15 warm starts stop the car (braking rows, Ux_min: first QP
# infeasible) or reach max_speed without the single-track stages' help (traction rows, peng: idle), so the tail
# starts nearer the drag level and Ux_min further under; the delta rows, V_min and peng_pm bind as at M = 15
CASC40_CASES = dict(
    CASC_CASES,
    tyre_f_lo=((), 40.0, -11000.0, 0.0, 0.0, -3000.0),
    tyre_r_lo=(ST_CASES["tyre_r_lo"][0], 35.0, -8500.0, 0.0, 0.0, -2000.0),
    tyre_f_up=((), 12.0, 6100.0, 0.0, 0.0, 1500.0),
    tyre_r_up=(ST_CASES["tyre_r_up"][0], 12.0, 7100.0, 0.0, 0.0, 1500.0),
    Ux_min=(ST_CASES["Ux_min"][0], 12.3, -1800.0, 0.0, 0.0, 300.0),
    peng_pm=ST_CASES["peng"] + (None,),
)
IDLE = {"peng": "peng_pm", "peng_pm": "peng"}   # cascaded: the family that must bind in no QP of the case


@functools.lru_cache(maxsize=None)
def casc_case(family, tyre, Mh=CASC_M, solver=0, inputs=None):
    """Mh = 15, qp.solver = 0: casc_ric_kernel<20, 15, tyre>; Mh = 40, qp.solver = 2: the condensed casc_sqp."""
    changes, Ux, Fx, delta0, ey0, Fx_pm = (CASC40_CASES if Mh == 40 else CASC_CASES)[family] if inputs is None else inputs
    cfgs = _configs("dynamic_car", "cascaded_mpc", tuple(changes) + (("mpc", ("horizon_pm",), Mh),
                                                                    ("mpc", ("qp", "solver"), solver)))
    d = casc_problem(Ux, Fx, delta0, ey0, Fx_pm, Mh, float(cfgs["mpc"]["ds_pm"]))
    return dict(family=family, tyre=tyre, M=Mh, d=d, cfgs=cfgs, scale=casc_scale(Mh), idle=IDLE.get(family),
                ref=_casc_solve(d, cfgs, tyre), ref_off=_casc_solve(d, _off(cfgs, family), tyre))


# -- kinematic: one LTV QP -------------------------------------------------------------------------------
# (config changes, v0, flat warm-start acceleration): v0 above v_max = 10, so the terminal over-speed hinge
# asks for braking, and the floor a little under v0 stops it at every stage but the unconstrained terminal one
KIN_CASES = {"v_min": ((("mpc", ("state_constraints", "v_min"), 11.5),), 12.0, 0.0)}


def kin_problem(N, v0, a, mpc_dt=0.03):
    x0 = np.array([[v0, 0.0, 50.0, 0.0, 0.0, 0.0]])
    ubar = np.zeros((1, N, 2))
    ubar[..., 0] = a
    return dict(x0=x0, kappa=np.zeros((1, N)), ds=np.full((1, N), mpc_dt * v0 + 0.5), ubar=ubar)


def _kin_solve(d, cfgs):
    """kin_ltv_solve's answer in the shape of an SQP history of one QP, so that the checks above apply."""
    r = Q.kin_ltv_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], float(cfgs["car"]["car"]["l"]), Q.kin_weights(cfgs["mpc"]))
    rec = dict(polished=r["polished"], stopped=~np.asarray(r["converged"], bool), alpha=np.ones(1), lam=r["lam"],
               rows=r["rows"], slack=r["d"] - np.einsum("bmn,bn->bm", r["C"], r["z"]))
    return dict(u_star=r["u_star"], x_star=r["x_star"], hist=[rec],
                in_domain=np.isfinite(r["x_star"]).all(axis=(1, 2)) & (r["x_star"][..., 0] > 0).all(axis=1))


@functools.lru_cache(maxsize=None)
def kin_case(family, solver=0, N=20, inputs=None):
    """qp.solver = 0: the condensed kin_ltv_kernel<20>; 1: the stagewise kin_ric_kernel<20>."""
    changes, v0, a = KIN_CASES[family] if inputs is None else inputs
    cfgs = _configs("kinematic_car", "kinematic_mpc", tuple(changes) + (("mpc", ("qp", "solver"), solver),))
    d = kin_problem(N, v0, a, float(cfgs["mpc"]["mpc_dt"]))
    return dict(family=family, N=N, d=d, cfgs=cfgs, scale=np.array([1.0, 1.0]),
                ref=_kin_solve(d, cfgs), ref_off=_kin_solve(d, _off(cfgs, family)))


# -- the preconditions -------------------------------------------------------------------------
def assert_clean(ref, what):
    """The oracle's own run is a clean one (the check of tests/test_gpu_instantiations.py): returns the smallest
    step length it took."""
    for i, rec in enumerate(ref["hist"]):
        assert np.asarray(rec["polished"], bool).all(), f"{what}: SQP iteration {i} has a QP that is not polished"
        assert not np.asarray(rec["stopped"], bool).any(), f"{what}: an SQP stopped at iteration {i}"
    assert np.asarray(ref["in_domain"], bool).all(), f"{what}: x* outside the domain"
    return min(float(np.min(rec["alpha"])) for rec in ref["hist"])


def assert_preconditions(case, bar, what):
    """Clean, binding, discriminating (module docstring).  bar: the u* bar of the kernel under test, in
    the units of u* / case["scale"].  Returns what the log prints."""
    ref, off = case["ref"], case["ref_off"]
    amin = assert_clean(ref, what)
    assert_clean(off, what + ", family off")
    qps, lam, rows = F.family_summary(ref["hist"], case["family"])
    assert qps and lam > F.LAM_BIND, f"{what}: {case['family']} binds in no QP"
    if case.get("idle"):
        assert not F.family_summary(ref["hist"], case["idle"])[0], f"{what}: {case['idle']} binds as well"
    moved = float(np.abs((off["u_star"] - ref["u_star"]) / case["scale"]).max())
    assert moved >= MARGIN * bar, f"{what}: switching {case['family']} off moves u* by {moved:.3e} < {MARGIN * bar:.1e}"
    return dict(qps=qps, lam=lam, rows=rows, moved=moved, alpha=amin)


# -- every kernel x family x tyre case ---------------------------------------------------------------
KERNELS = ("st_sqp", "dyn_sqp", "casc_ric", "casc_sqp", "kin_ltv", "kin_ric")
CASES = ([("st_sqp", f, t) for f in ST_CASES for t in ("fiala", "linear")]
         + [("dyn_sqp", f, t) for f in DYN_CASES for t in ("fiala", "linear")]
         + [("casc_ric", f, t) for f in CASC_CASES for t in ("fiala", "linear")]
         + [("casc_sqp", f, t) for f in CASC40_CASES for t in ("fiala", "linear")]
         + [("kin_ltv", "v_min", None), ("kin_ric", "v_min", None)])
CASE_IDS = ["-".join(x for x in c if x) for c in CASES]


def get_case(kernel, family, tyre):
    if kernel in ("st_sqp", "dyn_sqp"):
        return st_case(family, tyre, kernel)
    if kernel == "casc_ric":
        return casc_case(family, tyre, CASC_M, 0)
    if kernel == "casc_sqp":
        return casc_case(family, tyre, 40, 2)
    return kin_case(family, {"kin_ltv": 0, "kin_ric": 1}[kernel])


def bars(kernel, tyre):
    """(bar on u* / case["scale"], bar on x*): the project's existing ones, as tests/test_gpu_instantiations.py
    and, for the fp32 kernel, tests/test_gpu_dyn_sqp.py (U_TOL, U_TOL_FIALA, X_TOL) state them."""
    if kernel == "dyn_sqp":
        return (1e-4 if tyre == "linear" else 5e-4), 5e-3
    return 1e-5, 1e-6
