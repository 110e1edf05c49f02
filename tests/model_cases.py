"""Inputs, oracle answers, bars and preconditions for the model kernels of csrc/models.hip, for
tests/test_model_cases.py (CPU: the builders, the preconditions, the mutation margins) and
tests/test_gpu_models.py (GPU: the kernels against the same oracle answers).  No GPU import here.

Every input number is rounded to float32 and stored as float64, so an fp32 and an fp64 context see
identical values.  A case is computed once (functools.lru_cache) and never modified; it holds

  d        the inputs
  ref      {F64, F32}: entry -> the oracle (oracle/models.py) evaluated in that precision, as float64
  unit     entry -> e_col = max over the case of |oracle in float32 - oracle in float64| per output column
  bar32    entry -> 32 x max(e_col, one float32 ulp of the column's largest magnitude)
  bound64  entry -> elementwise fp64 bound, the tolerances of tests/test_gpu_parity.py (TOL64 below)
  margins  mutation -> dtype -> entry -> largest (column's move) / (column's bar) over the columns
  facts    what `assert_preconditions` checks

The entries are "ode_t", "ode_s" (vc_ode, temporal / spatial), "plant" (vc_plant_step, dt = DT), "spatial"
(vc_spatial_step) on the point sets and "rollout" (vc_rollout) on the horizon sets.

Why 32 in bar32: vc_models.hpp puts the native sin / cos / exp forms of the dynamic fp32 path at about 1e-6
absolute, against about 6e-8 for a correctly rounded float at O(1), a factor of 16; doubled for FMA contraction
and the quotient tan.  The unit comes from the reference alone, never from the kernel.

A mutation is the same oracle on deliberately wrong inputs or parameters -- the stage index off by one, the
front and the rear coefficient swapped, the other tyre.  Each must move at least one output column by
MARGIN x that column's bar in each dtype, so a kernel with that defect cannot pass.
"""
import functools

import numpy as np

from oracle import models as M

F32, F64 = np.float32, np.float64
DTYPES = (F64, F32)
DT = 0.05               # vc_plant_step's dt in every test
MARGIN = 100.0
BAR32_FACTOR = 32.0
KIN_COLS = ("v", "delta", "s", "ey", "epsi", "t")
DYN_COLS = ("Ux", "Uy", "r", "delta", "s", "ey", "epsi", "t")
DYN_ODD = [1, 2, 3, 5, 6]     # Uy, r, delta, ey, epsi: the state columns a left/right mirror negates
POINT_ENTRIES = ("ode_t", "ode_s", "plant", "spatial")
TYRES = ("linear", "fiala")

B_POINTS = 130          # one thread per problem, blocks of 128: two blocks, the second with two live threads
KIN_SEED, KIN_HORIZON_SEED, KIN_N = 0, 5, 20
DYN_POINT_SEED, DYN_HORIZON_SEED, DYN_N = 4, 211, 40
MIN_BRANCH = 10         # Fiala: evaluations inside and outside alphamod, per axle

# fp64 bounds |got - ref| <= atol + rtol |ref| of tests/test_gpu_parity.py, per (model, entry); "floor": its
# plant-step form |got - ref| / max(|ref|, 1e-9) < rtol; "colmax": rtol x the column's largest magnitude (the
# dynamic rollout, which that file does not check)
TOL64 = {
    ("kin", "ode_t"): (1e-13, 1e-13), ("kin", "ode_s"): (1e-13, 1e-13), ("kin", "plant"): (1e-13, 1e-13),
    ("kin", "spatial"): (1e-13, 1e-13), ("kin", "rollout"): (1e-12, 1e-12), ("kin", "A"): (1e-12, 1e-12),
    ("kin", "Bm"): (1e-12, 1e-12),
    ("dyn", "ode_t"): (1e-12, 1e-9), ("dyn", "ode_s"): (1e-12, 1e-9), ("dyn", "plant"): (1e-11, "floor"),
    ("dyn", "spatial"): (1e-11, 1e-11), ("dyn", "rollout"): (1e-11, "colmax"),
}


def r32(a):
    """Rounded to float32, stored as float64."""
    return np.ascontiguousarray(np.asarray(a, F64).astype(F32).astype(F64))


def _cast(d, dtype):
    return {k: v.astype(dtype) for k, v in d.items()}


def _colmax(a):
    return np.abs(a).reshape(-1, a.shape[-1]).max(axis=0)


def bound64(model, entry, ref):
    rtol, atol = TOL64[(model, entry)]
    if atol == "floor":
        return rtol * np.maximum(np.abs(ref), 1e-9)
    if atol == "colmax":
        return np.broadcast_to(rtol * _colmax(ref), ref.shape)
    return atol + rtol * np.abs(ref)


def unit_and_bar32(ref64, ref32):
    e_col = _colmax(ref32 - ref64)
    ulp = np.spacing(_colmax(ref64).astype(F32)).astype(F64)
    return e_col, BAR32_FACTOR * np.maximum(e_col, ulp)


# -- the oracle in the precision under test ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kin_L():
    from vcmpc.config import load_config
    return float(load_config("kinematic_car")["car"]["l"])


@functools.lru_cache(maxsize=None)
def _dyn_cfg_params():
    from vcmpc.config import load_config
    return M.dyn_params_from_config(load_config("dynamic_car"))


def dyn_params(dtype=F64, swap=()):
    """The car's parameters as scalars of `dtype`; swap: pairs of keys exchanged (a mutation)."""
    p = dict(_dyn_cfg_params())
    for a, b in swap:
        p[a], p[b] = p[b], p[a]
    return {k: dtype(v) for k, v in p.items()}


def kin_point_eval(d, dtype):
    x, u, k, ds = (d[n].astype(dtype) for n in ("x", "u", "kappa", "ds"))
    L = dtype(kin_L())
    out = dict(ode_t=M.kin_temporal_ode(x, u, k, L), ode_s=M.kin_spatial_ode(x, u, k, L),
               plant=M.kin_transition(x, u, k, dtype(DT), L), spatial=M.kin_spatial_transition(x, u, k, ds, L))
    assert all(v.dtype == dtype for v in out.values())
    return {n: v.astype(F64) for n, v in out.items()}


def dyn_point_eval(d, tyre, dtype, swap=()):
    x, u, k, ds = (d[n].astype(dtype) for n in ("x", "u", "kappa", "ds"))
    p = dyn_params(dtype, swap)
    with np.errstate(invalid="ignore"):   # the linear tyre never reads Fymax; the preconditions check it
        out = dict(ode_t=M.dyn_temporal_ode(x, u, k, p, tyre), ode_s=M.dyn_spatial_ode(x, u, k, p, tyre),
                   plant=M.dyn_transition(x, u, k, dtype(DT), p, tyre),
                   spatial=M.dyn_spatial_transition(x, u, k, ds, p, tyre))
    assert all(v.dtype == dtype for v in out.values())
    return {n: v.astype(F64) for n, v in out.items()}


def _rollout(step, d, dtype):
    """xbar[B, N + 1, nx] in `dtype` (vc_rollout's shape), as float64."""
    x0, ubar, kappa, ds = (d[n].astype(dtype) for n in ("x0", "ubar", "kappa", "ds"))
    N = ubar.shape[1]
    xbar = np.empty((x0.shape[0], N + 1, x0.shape[1]), dtype)
    xbar[:, 0] = x0
    for k in range(N):
        xn = step(xbar[:, k], ubar[:, k], kappa[:, k], ds[:, k])
        assert xn.dtype == dtype
        xbar[:, k + 1] = xn
    return xbar.astype(F64)


def kin_rollout(d, dtype):
    L = dtype(kin_L())
    return _rollout(lambda x, u, k, h: M.kin_spatial_transition(x, u, k, h, L), d, dtype)


def dyn_rollout(d, tyre, dtype, swap=()):
    p = dyn_params(dtype, swap)
    with np.errstate(invalid="ignore"):
        return _rollout(lambda x, u, k, h: M.dyn_spatial_transition(x, u, k, h, p, tyre), d, dtype)


# -- assembling a case --------------------------------------------------------------------------------
def _case(model, d, evaluate, mutants, facts, **extra):
    """evaluate(d, dtype, **mutation) -> entry -> array; mutants: name -> (d', mutation kwargs)."""
    ref = {dt: evaluate(d, dt) for dt in DTYPES}
    unit, bar32, b64 = {}, {}, {}
    for e in ref[F64]:
        unit[e], bar32[e] = unit_and_bar32(ref[F64][e], ref[F32][e])
        b64[e] = bound64(model, e, ref[F64][e])
    margins = {}
    for name, (dm, kw) in mutants.items():
        mut = evaluate(dm, F64, **kw)
        margins[name] = {F64: {}, F32: {}}
        for e in ref[F64]:
            moved = _colmax(mut[e] - ref[F64][e])
            margins[name][F64][e] = float((moved / _colmax(b64[e])).max())
            margins[name][F32][e] = float((moved / bar32[e]).max())
    facts = dict(facts, finite=all(np.isfinite(v).all() for r in ref.values() for v in r.values()))
    case = dict(model=model, d=d, ref=ref, unit=unit, bar32=bar32, bound64=b64, margins=margins, facts=facts, **extra)
    assert_preconditions(case)
    return case


def assert_preconditions(case):
    """Finite, inside the models' domain, both Fiala branches taken, every mutation MARGIN x the bar away."""
    f = case["facts"]
    assert f["finite"], "an oracle output is not finite"
    assert f["rho_min"] >= 0.5, f"1 - kappa ey = {f['rho_min']:.3f} < 0.5"
    if case["model"] == "dyn":
        assert f["Ux_min"] >= 5.0, f"Ux = {f['Ux_min']:.3f} < 5"
        assert f["fymax_real"], "a friction ellipse is exceeded: Fymax is not real"
        assert f["mirror_ok"], "the oracle's output on a mirror image is not the mirror of its output"
        if case["tyre"] == "fiala":
            for axle in ("f", "r"):
                inside, outside = f["inside_" + axle], f["outside_" + axle]
                assert inside >= MIN_BRANCH and outside >= MIN_BRANCH, (axle, inside, outside)
                if "outside_pos_" + axle in f:
                    assert f["outside_pos_" + axle] >= 1 and f["outside_neg_" + axle] >= 1, axle
    else:
        assert f["v_min"] >= 1.0 and f["epsi_max"] <= 1.2
    if "distinct_stages" in f:
        assert f["distinct_stages"], "two stages of a problem share ds or kappa"
    for name, by_dtype in case["margins"].items():
        for dt, by_entry in by_dtype.items():
            for e, m in by_entry.items():
                assert m >= MARGIN, f"mutation {name} moves {e} by only {m:.3g} x the {np.dtype(dt).name} bar"


def describe(case, what):
    """The per-column units and the mutation margins, one line each."""
    cols = KIN_COLS if case["model"] == "kin" else DYN_COLS
    lines = []
    for e, u in case["unit"].items():
        lines.append(f"{what} {e}: e_col " + " ".join(f"{c} {v:.2e}" for c, v in zip(cols, u))
                     + " | fp32 bar " + " ".join(f"{v:.2e}" for v in case["bar32"][e]))
    for name, by_dtype in case["margins"].items():
        lines.append(f"{what} mutation {name}: x bar " + ", ".join(
            f"{np.dtype(dt).name} " + " ".join(f"{e} {m:.3g}" for e, m in by.items()) for dt, by in by_dtype.items()))
    facts = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in case["facts"].items()}
    lines.append(f"{what} facts: {facts}")
    return "\n".join(lines)


def _roll_mutants(d):
    return {name: (dict(d, **{key: np.ascontiguousarray(np.roll(d[key], 1, axis=1))}), {})
            for name, key in (("ds_rolled", "ds"), ("kappa_rolled", "kappa"), ("ubar_rolled", "ubar"))}


def _param_mutants(d, tyre):
    m = {"Caf_Car_swapped": (d, dict(swap=(("Caf", "Car"),))),
         "other_tyre": (d, dict(tyre="linear" if tyre == "fiala" else "fiala"))}
    if tyre == "fiala":                     # the linear tyre does not read mu
        m["muf_mur_swapped"] = (d, dict(swap=(("muf", "mur"),)))
    return m


# -- kinematic ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kin_points():
    """B = 130 points in the ranges of test_gpu_parity.py::test_kin_plant_and_spatial_step, kappa from +-0.05."""
    rng, B = np.random.default_rng(KIN_SEED), B_POINTS
    x = np.column_stack([rng.uniform(2, 10, B), rng.uniform(-.3, .3, B), rng.uniform(0, 300, B),
                         rng.uniform(-2, 2, B), rng.uniform(-.3, .3, B), rng.uniform(0, 5, B)])
    u = np.column_stack([rng.uniform(-3, 3, B), rng.uniform(-.4, .4, B)])
    d = dict(x=r32(x), u=r32(u), kappa=r32(rng.uniform(-.05, .05, B)), ds=r32(rng.uniform(.3, .9, B)))
    facts = dict(rho_min=float((1 - d["kappa"] * d["x"][:, 3]).min()), v_min=float(d["x"][:, 0].min()),
                 epsi_max=float(np.abs(d["x"][:, 4]).max()))
    return _case("kin", d, kin_point_eval, {}, facts)


@functools.lru_cache(maxsize=None)
def kin_horizons():
    """kinematic_batch(5, N = 20) with kappa scaled per stage by U(0.5, 1): no two stages of a problem share ds
    (the sampler's is per stage already) or kappa.  jac: (A, Bm) of the oracle at its own fp64 rollout."""
    from vcmpc.workload import kinematic_batch
    d = kinematic_batch(5, N=KIN_N, seed=KIN_HORIZON_SEED)
    rng = np.random.default_rng(KIN_HORIZON_SEED + 1)
    d["kappa"] = d["kappa"] * rng.uniform(0.5, 1.0, d["kappa"].shape)
    d = {k: r32(v) for k, v in d.items()}
    xbar = kin_rollout(d, F64)
    facts = dict(rho_min=float((1 - d["kappa"] * xbar[:, :-1, 3]).min()), v_min=float(xbar[..., 0].min()),
                 epsi_max=float(np.abs(xbar[..., 4]).max()),
                 distinct_stages=all(len(np.unique(d[k][b])) == KIN_N for k in ("ds", "kappa") for b in range(5)))
    A, Bm = M.kin_spatial_jacobians(xbar[:, :-1], d["ubar"], d["kappa"], d["ds"], kin_L())
    return _case("kin", d, lambda dd, dt: dict(rollout=kin_rollout(dd, dt)), _roll_mutants(d), facts,
                 jac=dict(A=A, Bm=Bm))


# -- dynamic ------------------------------------------------------------------------------------------
def mirror_points(d):
    """The left/right mirror image: Uy, r, delta, ey, epsi, w and kappa negated."""
    x, u = d["x"].copy(), d["u"].copy()
    x[:, DYN_ODD] *= -1
    u[:, 1] *= -1
    return dict(x=x, u=u, kappa=-d["kappa"], ds=d["ds"].copy())


def _fiala_branches(x, u, p):
    """Per axle: evaluations inside / outside alphamod at the points (x, u), and the signs of alpha outside."""
    F = M.dyn_forces(x, u, p)
    out = {}
    for axle, Ca in (("f", p["Caf"]), ("r", p["Car"])):
        alpha = F["alpha_" + axle]
        inside = np.abs(alpha) <= np.arctan(3 * F["Fymax_" + axle] * p["eps"] / Ca)
        out.update({"inside_" + axle: int(inside.sum()), "outside_" + axle: int((~inside).sum()),
                    "outside_pos_" + axle: int((~inside & (alpha > 0)).sum()),
                    "outside_neg_" + axle: int((~inside & (alpha < 0)).sum())})
    return out


def _dyn_facts(x, u, kappa, x_all):
    """x, u, kappa: where the model is evaluated; x_all: every state of the case, outputs included."""
    p = dyn_params()
    F = M.dyn_forces(x, u, p)
    return dict(rho_min=float((1 - kappa * x[..., 5]).min()), Ux_min=float(x_all[..., 0].min()),
                fymax_real=bool(np.isfinite(F["Fymax_f"]).all() and np.isfinite(F["Fymax_r"]).all()),
                **_fiala_branches(x, u, p))


@functools.lru_cache(maxsize=None)
def dyn_point_inputs():
    """65 points (x0, ubar[:, 0], kappa[:, 0], ds[:, 0]) of the survey-range sampler, their 65 mirror images,
    and four edge rows written over rows 0..3; the same points for both tyres.  Also returns whether the
    oracle's outputs on the mirror images are the mirrors of its outputs (before the edge rows go in)."""
    from vcmpc.workload import dynamic_batch
    s = dynamic_batch(B_POINTS // 2, N=4, seed=DYN_POINT_SEED, ranges="survey")
    half = dict(x=r32(s["x0"]), u=r32(s["ubar"][:, 0]), kappa=r32(s["kappa"][:, 0]), ds=r32(s["ds"][:, 0]))
    mir = mirror_points(half)
    mirror_ok = True
    for tyre in TYRES:
        a, b = dyn_point_eval(half, tyre, F64), dyn_point_eval(mir, tyre, F64)
        for e in POINT_ENTRIES:
            m = a[e].copy()
            m[:, DYN_ODD] *= -1
            # numpy's tan / arctan are odd to an ulp or two only; 1e-14 is three orders under the fp64 bars
            mirror_ok &= bool(np.allclose(m, b[e], rtol=1e-14, atol=1e-14))
    d = {k: np.concatenate([half[k], mir[k]]) for k in half}
    d["x"][0, [1, 2, 3]] = 0.0        # alpha_f = alpha_r = 0 exactly: sgn returns 0
    d["u"][1, 0] = -500.0             # the drive/brake split's tanh argument is 0
    d["u"][2, 0] = -4000.0            # hard braking, load transfer to the front
    d["u"][3, 0] = 4000.0
    return {k: np.ascontiguousarray(v) for k, v in d.items()}, mirror_ok


@functools.lru_cache(maxsize=None)
def dyn_points(tyre):
    d, mirror_ok = dyn_point_inputs()
    ref = dyn_point_eval(d, tyre, F64)
    facts = _dyn_facts(d["x"], d["u"], d["kappa"], np.stack([d["x"], ref["plant"], ref["spatial"]]))
    facts["mirror_ok"] = mirror_ok
    return _case("dyn", d, lambda dd, dt, tyre=tyre, swap=(): dyn_point_eval(dd, tyre, dt, swap),
                 _param_mutants(d, tyre), facts, tyre=tyre)


@functools.lru_cache(maxsize=None)
def dyn_horizons(tyre):
    """dynamic_batch(5, N = 40) with ds scaled per stage by U(0.6, 1) -- downward only: the sampler's docstring
    explains that larger steps leave RK4's stability region -- and kappa by U(0.5, 1), so that no two stages of
    a problem share either."""
    from vcmpc.workload import dynamic_batch
    s = dynamic_batch(5, N=DYN_N, seed=DYN_HORIZON_SEED, tyre=tyre)
    rng = np.random.default_rng(DYN_HORIZON_SEED + 1)
    d = dict(x0=s["x0"], ubar=s["ubar"], ds=s["ds"] * rng.uniform(0.6, 1.0, s["ds"].shape),
             kappa=s["kappa"] * rng.uniform(0.5, 1.0, s["kappa"].shape))
    d = {k: r32(v) for k, v in d.items()}
    xbar = dyn_rollout(d, tyre, F64)
    facts = _dyn_facts(xbar[:, :-1], d["ubar"], d["kappa"], xbar)
    facts = {k: v for k, v in facts.items() if "outside_pos" not in k and "outside_neg" not in k}
    facts.update(mirror_ok=True,   # the mirror check belongs to the point set
                 distinct_stages=all(len(np.unique(d[k][b])) == DYN_N for k in ("ds", "kappa") for b in range(5)))
    mutants = dict(_roll_mutants(d), **_param_mutants(d, tyre))
    return _case("dyn", d, lambda dd, dt, tyre=tyre, swap=(): dict(rollout=dyn_rollout(dd, tyre, dt, swap)),
                 mutants, facts, tyre=tyre)


def first_stage(d):
    """The N = 1 slice of a horizon set."""
    return {k: np.ascontiguousarray(v[:, :1]) if k != "x0" else v for k, v in d.items()}
