"""Configuration: YAML loading and packing of ``vc_params``.

The reference reads its YAML with ``yaml.safe_load`` (utils/common_utils.py:16-19)
and wraps it in OmegaConf for dot access (scripts/kinmain.py:6-11).  OmegaConf is
not available here, so :class:`AttrDict` provides the same dot access.
"""
from __future__ import annotations

import os

import yaml

from . import _abi

CONFIG_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config")

# The build's LTV-QP contract defaults (no reference counterpart).
QP_DEFAULTS = {"prox": 1e-4, "tol": 1e-10, "max_iter": 40, "polish": 10, "trust_a": 0.0, "trust_w": 0.0,
               "solver": 0, "kin_sqp": 0, "shift": 0, "ms": 0, "elastic": 0.0}
# The dynamic SQP contract defaults (config/dynamic_mpc.yaml `qp` block).
DYN_QP_DEFAULTS = {"prox": 0.1, "tol": 1e-5, "max_iter": 60, "polish": 12, "trust_a": 0.0, "trust_w": 0.2,
                   "fx_scale": 1000.0, "trust_Fx": 2000.0, "sqp_iters": 3, "solver": 0, "kin_sqp": 0, "shift": 0, "ms": 0,
                   "elastic": 0.0}


class AttrDict(dict):
    """dict with attribute access, recursively (a stand-in for OmegaConf.create)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        for k, v in list(self.items()):
            self[k] = _wrap(v)

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = _wrap(v)


def _wrap(v):
    if isinstance(v, dict) and not isinstance(v, AttrDict):
        return AttrDict(v)
    if isinstance(v, list):
        return [_wrap(x) for x in v]
    return v


def load_config(path: str) -> AttrDict:
    """``load_config`` of utils/common_utils.py:16-19, returning dot-accessible dicts.
    A bare name (``"kinematic_mpc"``) resolves to ``vehicle-control_amd/config/<name>.yaml``."""
    if not os.path.sep in path and not path.endswith(".yaml"):
        path = os.path.join(CONFIG_DIR, path + ".yaml")
    with open(path, "r") as f:
        return AttrDict(yaml.safe_load(f))


def kin_mpc_struct(cfg) -> _abi.vc_kin_mpc:
    """Weights and bounds of a kinematic controller config (reference schema
    config/controllers/kinematic.yaml:7-32)."""
    cw, ic, sc = cfg["cost_weights"], cfg["input_constraints"], cfg["state_constraints"]
    return _abi.vc_kin_mpc(
        w_time=float(cw["time"]), w_ey=float(cw["ey"]), w_epsi=float(cw["epsi"]), w_v=float(cw["v"]),
        w_w=float(cw["w"]), w_a=float(cw["a"]), w_dev=float(cw["deviation"]), w_b=float(cw["boundary"]),
        a_min=float(ic["a_min"]), a_max=float(ic["a_max"]), w_min=float(ic["w_min"]), w_max=float(ic["w_max"]),
        v_min=float(sc["v_min"]), v_max=float(sc["v_max"]), delta_min=float(sc["delta_min"]),
        delta_max=float(sc["delta_max"]), ey_min=float(sc["ey_min"]), ey_max=float(sc["ey_max"]),
        w_obs=float(cw.get("obstacles", 0.0)))


def obstacles_struct(obstacles=None, margin_min: float = _abi.OBS_MARGIN_MIN,
                     inside: bool = False) -> _abi.vc_obstacles:
    """Pack an obstacle list [(s, ey, radius), ...] (the `obstacle_data` rows of the
    reference's config/environment/*.yaml, read at environment/track.py:131-138).
    None / [] = no barrier terms (the controller's ``obstacles: False``).  inside: the
    reference's own barrier inside an obstacle beyond the margin floor (vc_obstacles.inside)."""
    o = _abi.vc_obstacles()
    o.inside = 1 if inside else 0
    rows = [tuple(float(v) for v in r) for r in (obstacles or [])]
    if len(rows) > _abi.VC_MAX_OBSTACLES:
        raise ValueError(f"{len(rows)} obstacles > VC_MAX_OBSTACLES = {_abi.VC_MAX_OBSTACLES}")
    o.n = len(rows)
    o.margin_min = float(margin_min)
    for j, (s, ey, r) in enumerate(rows):
        o.s[j], o.ey[j], o.radius[j] = s, ey, r
    return o


def obstacle_list(car_or_track, controller_config):
    """The obstacle rows the barrier terms use: the track's obstacles when the
    controller config says ``obstacles: True`` (kinematic_mpc.py:130-131,
    cascaded_mpc.py:173-174 loop over ``car.track.obstacles``), else []."""
    if not controller_config.get("obstacles", False):
        return []
    track = getattr(car_or_track, "track", car_or_track)
    return [(o.s, o.ey, o.radius) for o in getattr(track, "obstacles", [])]


def qp_struct(cfg=None, defaults=None) -> _abi.vc_qp:
    q = dict(QP_DEFAULTS if defaults is None else defaults)
    if cfg is not None and cfg.get("qp") is not None:
        q.update(cfg["qp"])
    return _abi.vc_qp(prox=float(q["prox"]), tol=float(q["tol"]), trust_a=float(q["trust_a"]),
                      trust_w=float(q["trust_w"]), max_iter=int(q["max_iter"]), polish=int(q["polish"]),
                      solver=int(q["solver"]), kin_sqp=int(q.get("kin_sqp", 0)), shift=int(q.get("shift", 0)),
                      ms=int(q.get("ms", 0)), elastic=float(q.get("elastic", 0.0)))


def dyn_car_struct(cfg, tyre: str = "fiala") -> _abi.vc_dyn_car:
    """Dynamic-car parameters (reference schema config/models/dynamic_car.yaml:4-32,
    consumed at models/dynamic_car.py:62-151)."""
    car, env = cfg["car"], cfg["env"]
    return _abi.vc_dyn_car(
        l=float(car["l"]), m=float(car["m"]), Izz=float(car["Izz"]), a=float(car["a"]), b=float(car["b"]),
        h=float(car["h"]), eps=float(car["eps"]), Peng=float(car["Peng"]),
        Xdf=float(car["Xd"]["f"]), Xdr=float(car["Xd"]["r"]), Xbf=float(car["Xb"]["f"]), Xbr=float(car["Xb"]["r"]),
        Caf=float(car["C_alpha"]["f"]), Car=float(car["C_alpha"]["r"]),
        Cd=float(env["Cd"]), muf=float(env["mu"]["f"]), mur=float(env["mu"]["r"]), theta=float(env["theta"]),
        phi=float(env["phi"]), Av2=float(env["Av2"]), Frr=float(env["Frr"]),
        tyre=_abi.VC_TYRE_LINEAR if tyre == "linear" else _abi.VC_TYRE_FIALA)


def dyn_mpc_struct(cfg) -> _abi.vc_dyn_mpc:
    """Weights and bounds of a single-track controller config (reference schema
    config/controllers/singletrack.yaml, read at cascaded_mpc.py:91-179,279-304)
    plus the SQP knobs of its `qp` block."""
    cw, ic, sc = cfg["cost_weights"], cfg["input_constraints"], cfg["state_constraints"]
    q = dict(DYN_QP_DEFAULTS)
    q.update(cfg.get("qp") or {})
    return _abi.vc_dyn_mpc(
        w_time=float(cw["time"]), w_speed=float(cw["speed"]), w_ey=float(cw["ey"]), w_epsi=float(cw["epsi"]),
        w_w=float(cw["w"]), w_Fx=float(cw["Fx"]), w_dev=float(cw["deviation_st"]), w_b=float(cw["boundary"]),
        w_slip=float(cw["slip"]), w_min=float(ic["w_min"]), w_max=float(ic["w_max"]),
        Ux_min=float(sc["Ux_min"]), max_speed=float(sc["max_speed"]), delta_min=float(sc["delta_min"]),
        delta_max=float(sc["delta_max"]), ey_min=float(sc["ey_min"]), ey_max=float(sc["ey_max"]),
        fx_scale=float(q["fx_scale"]), trust_Fx=float(q["trust_Fx"]), sqp_iters=int(q["sqp_iters"]),
        w_obs=float(cw.get("obstacles", 0.0)))


def casc_mpc_struct(cfg) -> _abi.vc_casc_mpc:
    """The point-mass tail of a cascaded controller config (reference schema
    config/controllers/cascaded.yaml, read at cascaded_mpc.py:41-52,181-277)."""
    cw, pc = cfg["cost_weights"], cfg["state_pm_constraints"]
    return _abi.vc_casc_mpc(horizon_pm=int(cfg["horizon_pm"]), ds_pm=float(cfg["ds_pm"]),
                            w_dev_pm=float(cw["deviation_pm"]), w_Fy=float(cw["Fy"]), w_switch=float(cw["switch_F"]),
                            V_min=float(pc["V_min"]), ey_min_pm=float(pc["ey_min"]), ey_max_pm=float(pc["ey_max"]))


def make_params(kin_car=None, dyn_car=None, kin_mpc=None, dyn_mpc=None, tyre: str = "fiala",
                obstacles=None, obstacle_inside: bool = False) -> _abi.vc_params:
    """Pack whichever configs are given into one ``vc_params`` (others zeroed).
    The QP knobs come from the controller config given (kinematic or dynamic);
    ``obstacles`` is the [(s, ey, radius), ...] list the barrier terms use."""
    p = _abi.vc_params()
    p.obs = obstacles_struct(obstacles, inside=obstacle_inside)
    if kin_car is not None:
        p.kin_car = _abi.vc_kin_car(l=float(kin_car["car"]["l"]))
    if dyn_car is not None:
        p.dyn_car = dyn_car_struct(dyn_car, tyre)
    if kin_mpc is not None:
        p.kin_mpc = kin_mpc_struct(kin_mpc)
    if dyn_mpc is not None:
        p.dyn_mpc = dyn_mpc_struct(dyn_mpc)
        p.qp = qp_struct(dyn_mpc, DYN_QP_DEFAULTS)
        if int(dyn_mpc.get("horizon_pm", 0) or 0) > 0:
            p.casc = casc_mpc_struct(dyn_mpc)
    else:
        p.qp = qp_struct(kin_mpc)
    return p
