"""GPU: the model kernels of csrc/models.hip (vc_ode, vc_plant_step, vc_spatial_step, vc_rollout, vc_linearize)
in every built type against the oracle evaluated in the precision under test (tests/model_cases.py).

Coverage table -- the 17 kernels of models.hip, both tyres where the kernel reads one, and the cascaded route:

    kernel               NX      dtype  tyre            test
    -------------------  ------  -----  --------------  ---------------------------------------------------
    ode_kernel           KIN_NX  f64    -               test_kin_points_vs_oracle[f64]
    plant_step_kernel    KIN_NX  f64    -               test_kin_points_vs_oracle[f64]
    spatial_step_kernel  KIN_NX  f64    -               test_kin_points_vs_oracle[f64]
    rollout_kernel       KIN_NX  f64    -               test_kin_rollout_vs_oracle[f64]
    kin_linearize_kernel KIN_NX  f64    -               test_kin_rollout_vs_oracle[f64]  ([f32]: VC_E_UNSUPPORTED)
    ode_kernel           KIN_NX  f32    -               test_kin_points_vs_oracle[f32]
    plant_step_kernel    KIN_NX  f32    -               test_kin_points_vs_oracle[f32]
    spatial_step_kernel  KIN_NX  f32    -               test_kin_points_vs_oracle[f32]
    rollout_kernel       KIN_NX  f32    -               test_kin_rollout_vs_oracle[f32]
    ode_kernel           DYN_NX  f64    linear / fiala  test_dyn_points_vs_oracle[linear-f64 / fiala-f64]
    plant_step_kernel    DYN_NX  f64    linear / fiala  test_dyn_points_vs_oracle[linear-f64 / fiala-f64]
    spatial_step_kernel  DYN_NX  f64    linear / fiala  test_dyn_points_vs_oracle[linear-f64 / fiala-f64]
    rollout_kernel       DYN_NX  f64    linear / fiala  test_dyn_rollout_vs_oracle[linear-f64 / fiala-f64]
    ode_kernel           DYN_NX  f32    linear / fiala  test_dyn_points_vs_oracle[linear-f32 / fiala-f32]
    plant_step_kernel    DYN_NX  f32    linear / fiala  test_dyn_points_vs_oracle[linear-f32 / fiala-f32]
    spatial_step_kernel  DYN_NX  f32    linear / fiala  test_dyn_points_vs_oracle[linear-f32 / fiala-f32]
    rollout_kernel       DYN_NX  f32    linear / fiala  test_dyn_rollout_vs_oracle[linear-f32 / fiala-f32]
    the four DYN_NX f64 kernels through a VC_MODEL_CASCADED context (the `else` branches of
    m.model == VC_MODEL_KINEMATIC), fiala               test_cascaded_context_is_the_dynamic_model

Every point test runs B = 130 (two blocks of 128, two live threads in the second) and B = 1; every rollout test
has per-stage ds, kappa and inputs, and the dynamic ones an N = 1 context as well.

Bars.  fp64: the tolerances of tests/test_gpu_parity.py (model_cases.TOL64), and 1e-11 x the column's largest
magnitude for the dynamic rollout.  fp32: per output column 32 x max(e_col, one float32 ulp of the column's
largest magnitude), e_col = max |oracle in float32 - oracle in float64| on the same inputs -- from the reference
alone (model_cases.py says why 32).  Each check prints the largest error per column and, for fp32, its ratio to
the unit max(e_col, ulp); the log of an MI355X run is profiles/models/test_gpu_models.log.

Every test first asserts its case's preconditions (finite, inside the models' domain, both Fiala branches
taken on each axle, every mutation of the reference at least 100 x the bar away), checks that its inputs come
back unchanged and that a second call gives the same bits.
"""
import numpy as np
import pytest

import model_cases as C

pytestmark = pytest.mark.gpu

MAX_BATCH = 130
DTYPES = {"f64": C.F64, "f32": C.F32}


def _abi_dtype(dt):
    from vcmpc import _abi
    return _abi.VC_F64 if dt == C.F64 else _abi.VC_F32


def _kin_ctx(N, dt, kin_cfg):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config
    return Context(model=_abi.VC_MODEL_KINEMATIC, N=N, max_batch=MAX_BATCH, dtype=_abi_dtype(dt),
                   kin_car=load_config("kinematic_car"), kin_mpc=kin_cfg)


def _dyn_ctx(N, dt, tyre, horizon_pm=0):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    cfg = load_config("cascaded_mpc" if horizon_pm else "dynamic_mpc")
    if horizon_pm:
        cfg["horizon_pm"] = horizon_pm
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=cfg, tyre=tyre)
    model = _abi.VC_MODEL_CASCADED if horizon_pm else _abi.VC_MODEL_DYNAMIC
    return Context(model=model, N=N, max_batch=MAX_BATCH, dtype=_abi_dtype(dt), params=p)


def _inputs(d, dt, rows=slice(None)):
    return {k: np.ascontiguousarray(v[rows].astype(dt)) for k, v in d.items()}


def _twice(call, a):
    """call(a) on copies, twice: the same bits both times, the inputs unchanged; the first answer as float64."""
    b = {k: v.copy() for k, v in a.items()}
    first, second = call(b), call(b)
    for k in a:
        np.testing.assert_array_equal(b[k], a[k], err_msg=f"input {k} changed")
    for n in first:
        assert first[n].dtype == a[next(iter(a))].dtype
        np.testing.assert_array_equal(first[n], second[n], err_msg=f"{n} differs on a rerun")
    return {n: v.astype(np.float64) for n, v in first.items()}


def _check(what, case, entry, got, dt, rows=slice(None)):
    """|got - ref| against the case's bound for `dt`, per column; prints before it asserts."""
    ref = case["ref"][dt][entry][rows]
    cols = C.KIN_COLS if case["model"] == "kin" else C.DYN_COLS
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), f"{what} {entry}: not finite"
    err_col = err.reshape(-1, err.shape[-1]).max(axis=0)
    if dt == C.F64:
        bound = case["bound64"][entry][rows]
        used = (err / bound).reshape(-1, err.shape[-1]).max(axis=0)
        print(f"{what} {entry}: max err " + " ".join(f"{c} {e:.2e}" for c, e in zip(cols, err_col))
              + " | of the bound " + " ".join(f"{u:.3f}" for u in used))
    else:
        bound = np.broadcast_to(case["bar32"][entry], err.shape)
        unit = case["bar32"][entry] / C.BAR32_FACTOR
        print(f"{what} {entry}: max err " + " ".join(f"{c} {e:.2e}" for c, e in zip(cols, err_col))
              + " | unit " + " ".join(f"{u:.2e}" for u in unit)
              + " | err / unit " + " ".join(f"{r:.2f}" for r in err_col / unit))
    bad = err > bound
    assert not bad.any(), (f"{what} {entry}: {int(bad.sum())} values over the bar, worst {float((err / bound).max()):.3g} x "
                           f"the bar in column {cols[int(np.unravel_index(np.argmax(err / bound), err.shape)[-1])]}")


def _points(ctx, case, dt, what):
    for rows in (slice(None), slice(0, 1)):       # B = 130 and B = 1
        a = _inputs(case["d"], dt, rows)
        got = _twice(lambda b: dict(ode_t=ctx.ode(b["x"], b["u"], b["kappa"]),
                                    ode_s=ctx.ode(b["x"], b["u"], b["kappa"], space=True),
                                    plant=ctx.plant_step(b["x"], b["u"], b["kappa"], C.DT),
                                    spatial=ctx.spatial_step(b["x"], b["u"], b["kappa"], b["ds"])), a)
        for e in C.POINT_ENTRIES:
            assert got[e].shape == a["x"].shape
            _check(f"{what} B={len(a['x'])}", case, e, got[e], dt, rows)


def _rollout(ctx, d, dt):
    a = _inputs(d, dt)
    return _twice(lambda b: dict(rollout=ctx.rollout(b["x0"], b["ubar"], b["kappa"], b["ds"])), a)["rollout"]


# -- kinematic --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_kin_points_vs_oracle(dtype, kin_cfg):
    """ode_kernel / plant_step_kernel / spatial_step_kernel<T, KIN_NX>: vc_ode (temporal and spatial),
    vc_plant_step (dt = 0.05) and vc_spatial_step against the oracle in T, B = 130 and B = 1.  The fp32 kernels
    call the plain cos / sin / tan overloads, so the ratios to the unit stay near 1.
    Measured on an MI355X: fp64 at most 4.4e-16 (0.001 of the bound); fp32 err / unit at most 1.55 (ode_t, epsi)."""
    dt = DTYPES[dtype]
    case = C.kin_points()
    C.assert_preconditions(case)
    with _kin_ctx(C.KIN_N, dt, kin_cfg) as ctx:
        _points(ctx, case, dt, f"kin points {dtype}")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_kin_rollout_vs_oracle(dtype, kin_cfg):
    """rollout_kernel<T, KIN_NX> on N = 20 horizons whose stages all differ in ds, kappa and input, against the
    oracle in T; fp64: kin_linearize_kernel against the oracle's analytic Jacobians along its own rollout;
    fp32: vc_linearize answers VC_E_UNSUPPORTED.
    Measured on an MI355X: fp64 rollout at most 8.9e-16, A 2.2e-16, Bm 2.8e-17; fp32 err / unit at most 2.22 (epsi)."""
    from vcmpc import _abi
    dt = DTYPES[dtype]
    case = C.kin_horizons()
    C.assert_preconditions(case)
    d = case["d"]
    with _kin_ctx(C.KIN_N, dt, kin_cfg) as ctx:
        got = _rollout(ctx, d, dt)
        _check(f"kin rollout {dtype}", case, "rollout", got, dt)
        np.testing.assert_array_equal(got[:, 0], d["x0"])
        a = _inputs(dict(d, xbar=case["ref"][C.F64]["rollout"]), dt)
        if dt == C.F32:
            with pytest.raises(_abi.VcError) as e:
                ctx.linearize(a["xbar"], a["ubar"], a["kappa"], a["ds"])
            assert e.value.code == _abi.VC_E_UNSUPPORTED
            return
        jac = _twice(lambda b: dict(zip(("A", "Bm"), ctx.linearize(b["xbar"], b["ubar"], b["kappa"], b["ds"]))), a)
    for n in ("A", "Bm"):
        ref = case["jac"][n]
        err = np.abs(jac[n] - ref)
        bound = C.bound64("kin", n, ref)
        print(f"kin linearize {n}: max err {err.max():.2e}, {float((err / bound).max()):.3f} of the bound")
        assert jac[n].shape == ref.shape and (err <= bound).all()


# -- dynamic ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("tyre", C.TYRES)
def test_dyn_points_vs_oracle(tyre, dtype):
    """ode_kernel / plant_step_kernel / spatial_step_kernel<T, DYN_NX> with either tyre: vc_ode (temporal and
    spatial), vc_plant_step (dt = 0.05) and vc_spatial_step against the oracle in T on 65 survey-range points,
    their mirror images and the edge rows (alpha = 0, the split's tanh at 0, Fx = -4000 and +4000), B = 130 and
    B = 1 (the alpha = 0 row).
    Measured on an MI355X: fp64 at most 7.1e-15 on the vector fields and 3.6e-15 on the steps, 0.025 of the bound
    (plant, r, linear tyre); fp32 err / unit at most 4.64 (linear: plant, r) and 2.64 (fiala: ode_t, ey) -- the
    native sin / cos / exp forms stay well inside the factor 32 on these points."""
    dt = DTYPES[dtype]
    case = C.dyn_points(tyre)
    C.assert_preconditions(case)
    with _dyn_ctx(C.DYN_N, dt, tyre) as ctx:
        _points(ctx, case, dt, f"dyn points {tyre} {dtype}")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("tyre", C.TYRES)
def test_dyn_rollout_vs_oracle(tyre, dtype):
    """rollout_kernel<T, DYN_NX> on N = 40 horizons whose stages all differ in ds, kappa and input, against the
    oracle in T (fp64: 1e-11 x the column's largest magnitude); and on an N = 1 context, where xbar[:, 1] is bit
    for bit vc_spatial_step of stage 0 and xbar[:, 0] is x0.
    Measured on an MI355X: fp64 at most 4.4e-16 (linear) and 1.3e-15 (fiala, Uy), under 1e-3 of the bound; fp32
    err / unit at most 1.04 (linear, Uy) and 1.61 (fiala, Uy)."""
    dt = DTYPES[dtype]
    case = C.dyn_horizons(tyre)
    C.assert_preconditions(case)
    d = case["d"]
    with _dyn_ctx(C.DYN_N, dt, tyre) as ctx:
        got = _rollout(ctx, d, dt)
    _check(f"dyn rollout {tyre} {dtype}", case, "rollout", got, dt)
    one = C.first_stage(d)
    with _dyn_ctx(1, dt, tyre) as ctx:
        x1 = _rollout(ctx, one, dt)
        a = _inputs(one, dt)
        step = ctx.spatial_step(a["x0"], np.ascontiguousarray(a["ubar"][:, 0]), np.ascontiguousarray(a["kappa"][:, 0]),
                                np.ascontiguousarray(a["ds"][:, 0]))
    assert x1.shape == (5, 2, 8)
    np.testing.assert_array_equal(x1[:, 0], d["x0"])
    np.testing.assert_array_equal(x1[:, 1], step.astype(np.float64))
    np.testing.assert_array_equal(x1[:, 1], got[:, 1])


def test_cascaded_context_is_the_dynamic_model():
    """A VC_MODEL_CASCADED context (N = 20, horizon_pm = 15, Fiala, fp64) reaches the DYN_NX kernels through the
    `else` branches of m.model == VC_MODEL_KINEMATIC: vc_ode, vc_plant_step, vc_spatial_step and vc_rollout are bit
    for bit those of a dynamic fp64 N = 20 context on the same inputs (this axis moves data, not arithmetic, so it
    is compared with its sibling, which the tests above compare with the oracle)."""
    points, horizons = C.dyn_points("fiala"), C.dyn_horizons("fiala")
    C.assert_preconditions(points)
    C.assert_preconditions(horizons)
    a = _inputs(points["d"], C.F64)
    h = _inputs({k: (v if k == "x0" else v[:, :20]) for k, v in horizons["d"].items()}, C.F64)

    def run(ctx):
        out = _twice(lambda b: dict(ode_t=ctx.ode(b["x"], b["u"], b["kappa"]),
                                    ode_s=ctx.ode(b["x"], b["u"], b["kappa"], space=True),
                                    plant=ctx.plant_step(b["x"], b["u"], b["kappa"], C.DT),
                                    spatial=ctx.spatial_step(b["x"], b["u"], b["kappa"], b["ds"])), a)
        out["rollout"] = _twice(lambda b: dict(r=ctx.rollout(b["x0"], b["ubar"], b["kappa"], b["ds"])), h)["r"]
        return out

    with _dyn_ctx(20, C.F64, "fiala", horizon_pm=15) as ctx:
        casc = run(ctx)
    with _dyn_ctx(20, C.F64, "fiala") as ctx:
        dyn = run(ctx)
    assert casc["rollout"].shape == (5, 21, 8)
    for n in dyn:
        np.testing.assert_array_equal(casc[n], dyn[n], err_msg=n)
    # the sibling is the kernel the oracle tests hold: its first 21 columns are the N = 40 rollout's
    _check("dyn N=20 rollout fiala f64", horizons, "rollout", dyn["rollout"], C.F64, (slice(None), slice(0, 21)))
