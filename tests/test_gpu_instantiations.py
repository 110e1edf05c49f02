"""GPU: oracle parity for every built kernel instantiation that had none.

The launchers dispatch on template axes (horizon, tyre, J placement, detection); each compiled kernel
must be compared with the fp64 oracle (or, for an axis that moves data and not arithmetic, bit for bit
with a sibling that is).  Coverage table -- a new template axis gets a row here and a test:

    kernel      axis value                          test
    ----------  ----------------------------------  -------------------------------------------------------
    st_sqp      N = 20, linear / fiala              test_st_sqp_instantiations_vs_oracle[20-*]  (this file)
    st_sqp      N = 30, linear / fiala              test_st_sqp_instantiations_vs_oracle[30-*]  (this file)
    st_sqp      N = 40, linear                      test_gpu_st_sqp.py::test_st_sqp_vs_golden_n40
    st_sqp      N = 40, fiala                       test_gpu_st_sqp.py::test_st_sqp_reference_horizons_vs_oracle[40-fiala-*]
    st_sqp      N = 50, linear                      test_st_sqp_instantiations_vs_oracle[50-linear]  (this file)
    st_sqp      N = 50, fiala                       test_gpu_st_sqp.py::test_st_sqp_reference_horizons_vs_oracle[50-fiala-*]
    st_sqp      N = 60, linear / fiala              test_gpu_st_sqp.py::test_st_sqp_reference_horizons_vs_oracle[60-*]
    st_sqp      J global (B > 768), DET off         test_gpu_st_sqp.py::test_st_sqp_j_placement_bit_identical
    st_sqp      DET on, J in LDS                    test_gpu_sqp_infeasible.py::test_status_and_certificates, test_fiala_tyre
    st_sqp      DET on, J global                    test_gpu_sqp_infeasible.py::test_detection_global_j_bit_identical
    casc_ric    M = 15 / 25 / 35, fiala             test_gpu_casc_ric.py::test_casc_ric_recorded_tails_vs_oracle
    casc_ric    M = 40, fiala                       test_gpu_casc_ric.py::test_casc_ric_vs_golden_m40
    casc_ric    M = 15 / 25 / 35 / 40, linear       test_casc_ric_linear_vs_oracle  (this file)
    casc_ric    J global (M = 35 / 40), both tyres  test_gpu_casc_ric.py::test_casc_ric_j_placement_bit_identical[*-fiala / *-linear]
    casc_sqp    M = 40, fiala                       test_gpu_casc.py::test_first_qp_vs_golden, test_solve_vs_golden
    casc_sqp    M = 40, linear                      test_casc_sqp_linear_first_qp_vs_oracle,
                                                    test_casc_sqp_linear_matches_stagewise  (this file)
    kin_ltv     N = 20                              test_gpu_parity.py (golden vectors)
    kin_ric     N = 10 .. 60, DET off / on          test_gpu_kin_ric.py, test_gpu_infeasible.py
    drive / horizon kernels, every model            test_gpu_closed_loop.py, test_gpu_sim_bookkeeping.py
    models.hip  ode / plant_step / spatial_step,    test_gpu_models.py::test_kin_points_vs_oracle[f64 / f32],
                KIN_NX / DYN_NX, f64 / f32,         test_dyn_points_vs_oracle[linear / fiala - f64 / f32]
                linear / fiala
    models.hip  rollout, KIN_NX / DYN_NX,           test_gpu_models.py::test_kin_rollout_vs_oracle[f64 / f32],
                f64 / f32, linear / fiala           test_dyn_rollout_vs_oracle[linear / fiala - f64 / f32]
    models.hip  kin_linearize (f64 only)            test_gpu_models.py::test_kin_rollout_vs_oracle[f64]
    models.hip  DYN_NX kernels, cascaded context    test_gpu_models.py::test_cascaded_context_is_the_dynamic_model
                                                    (the kernel x NX x dtype x tyre table heads that file)

The template axes are one half; the other is which inequality rows bind on a test's problems -- the kernel x row
family table heads tests/test_gpu_row_families.py.

Bars (the project's own): single track 1e-5 on u* (Fx in N, w in rad/s) and 1e-6 on x*; cascaded 1e-5
on u* in the scaled variable (Fx / 1000, w, Fy / 1000) and 1e-6 on x*.

Every test first asserts that its oracle set is clean -- every QP of every SQP iteration polished, x*
in the models' domain, no SQP stopped early -- so that a degenerate set cannot hide a failure.
"""
import functools

import numpy as np
import pytest

from oracle import casc_sqp as CS
from oracle import dyn_sqp as D

pytestmark = pytest.mark.gpu

U_TOL = 1e-5
X_TOL = 1e-6
N_ST = 20   # single-track stages of the cascaded contexts


@functools.lru_cache(maxsize=None)
def _dyn_params():
    from oracle import models as M
    from vcmpc.config import load_config
    return M.dyn_params_from_config(load_config("dynamic_car"))


def _assert_clean(ref, what):
    """The oracle's own run is a clean one: returns the smallest step length it took."""
    for i, rec in enumerate(ref["hist"]):
        assert np.asarray(rec["polished"], bool).all(), f"{what}: SQP iteration {i} has a QP that is not polished"
        assert not np.asarray(rec["stopped"], bool).any(), f"{what}: an SQP stopped at iteration {i}"
    assert np.asarray(ref["in_domain"], bool).all(), f"{what}: x* outside the domain"
    return min(float(np.min(rec["alpha"])) for rec in ref["hist"])


# -- single track ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _st_case(N, tyre, B):
    """Problems and the oracle's answer, computed once per case and never modified."""
    from vcmpc.config import load_config
    from vcmpc.workload import dynamic_batch
    cfg = load_config("singletrack_mpc")
    d = {k: v.astype(np.float64) for k, v in dynamic_batch(B, N=N, seed=100 + N, tyre=tyre).items()}
    ref = D.dyn_sqp_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], _dyn_params(), D.dyn_weights(cfg), tyre)
    return d, ref


@pytest.mark.parametrize("N,tyre,B", [(20, "linear", 4), (20, "fiala", 4), (30, "linear", 4), (30, "fiala", 4),
                                      (50, "linear", 3)])
def test_st_sqp_instantiations_vs_oracle(N, tyre, B):
    """st_sqp_kernel<N, tyre> at the horizons no other oracle test reaches (singletrack_mpc.yaml, fp64).
    Measured on an MI355X, max |u* - u*_oracle| (Fx in N) and interior-point iterations:
    (20, linear) 2.6e-11, 40..55; (20, fiala) 3.0e-11, 40..72; (30, linear) 2.7e-11, 40..52;
    (30, fiala) 3.5e-11, 40..63; (50, linear) 3.0e-11, 40..53; |x* - x*_oracle| at most 7.5e-14."""
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    d, ref = _st_case(N, tyre, B)
    amin = _assert_clean(ref, f"N={N} {tyre}")
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("singletrack_mpc"), tyre=tyre)
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=N, max_batch=B, dtype=_abi.VC_F64, params=p) as c:
        u0, xs, us, st, it = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy())
    err_u = np.abs(us - ref["u_star"]).max()
    err_x = np.abs(xs - ref["x_star"]).max()
    print(f"st_sqp N={N} {tyre}: max |u* - u*_oracle| = {err_u:.3e}, |x* - x*_oracle| = {err_x:.3e}, status {st.tolist()}, "
          f"IPM iterations {it.min()}..{it.max()}, oracle's smallest alpha {amin:g}")
    assert (st == 0).all(), st
    assert err_u < U_TOL
    assert err_x < X_TOL
    np.testing.assert_array_equal(u0, us[:, 0])


# -- cascaded, linear tyre ---------------------------------------------------------------------------
def _scale(M):
    s = np.ones((N_ST + M, 2))
    s[:, 0] = 1000.0
    s[N_ST:, 1] = 1000.0
    return s


def _casc_cfg(M, solver=0):
    from vcmpc.config import load_config
    cfg = load_config("cascaded_mpc")
    cfg["horizon_pm"] = M
    cfg["qp"] = dict(cfg["qp"], solver=solver)
    return cfg


def _casc_ctx(M, B, solver=0):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=_casc_cfg(M, solver), tyre="linear")
    return Context(model=_abi.VC_MODEL_CASCADED, N=N_ST, max_batch=B, dtype=_abi.VC_F64, params=p)


@functools.lru_cache(maxsize=None)
def _casc_case(M, seed):
    from vcmpc.workload import cascaded_batch
    d = cascaded_batch(3, M=M, seed=seed, tyre="linear")
    ref = CS.casc_sqp_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], _dyn_params(), CS.casc_weights(_casc_cfg(M)),
                            tyre="linear")
    return d, ref


@pytest.mark.parametrize("M,seed", [(15, 415), (25, 425), (35, 435), (40, 440), (40, 441)])
def test_casc_ric_linear_vs_oracle(M, seed):
    """casc_ric_kernel<20, M, VC_TYRE_LINEAR, *> (switch-stage lateral force included) against the
    oracle with the linear tyre.  On these sets the linear and the Fiala optimum differ by 0.26 to 5 in
    the scaled variable, so a launcher that always ran the Fiala kernel fails by four orders.  Seed 440
    has a domain cut-back in the oracle (smallest alpha 1/64): the only coverage of the cut-back with
    this tyre; seed 441 is the same shape with alpha = 1 throughout.
    Measured on an MI355X, scaled max |u* - u*_oracle| and iterations: M = 15 4.8e-14, 24..33;
    25 1.7e-13, 25..28; 35 2.1e-13, 25..27; 40 (seed 440) 4.1e-12, 24..31; 40 (seed 441) 3.2e-12, 25..31;
    |x* - x*_oracle| at most 2.9e-11 (seed 440)."""
    d, ref = _casc_case(M, seed)
    amin = _assert_clean(ref, f"M={M} seed {seed}")
    assert (amin < 1.0) == (seed == 440)
    with _casc_ctx(M, 3) as c:
        u0, xs, us, st, it = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy())
    err_u = np.abs((us - ref["u_star"]) / _scale(M)).max()
    err_x = np.abs(xs - ref["x_star"]).max()
    print(f"casc_ric linear M={M} seed {seed}: scaled |u* - u*_oracle| = {err_u:.3e}, |x* - x*_oracle| = {err_x:.3e}, "
          f"status {st.tolist()}, iterations {it.min()}..{it.max()}, oracle's smallest alpha {amin:g}")
    assert (st == 0).all(), st
    assert err_u < U_TOL
    assert err_x < X_TOL
    np.testing.assert_array_equal(u0, us[:, 0])


@pytest.mark.parametrize("seed", [440, 441])
def test_casc_sqp_linear_first_qp_vs_oracle(seed):
    """casc_sqp_kernel<20, 40, VC_TYRE_LINEAR>: vc_condense's H and g of the first QP against
    oracle casc_qp(..., tyre="linear"), at the relative bars of test_gpu_casc.py::test_first_qp_vs_golden.
    Measured on an MI355X (seed 440 / 441): rel |H - H_oracle| 1.1e-15 / 1.1e-15, rel |g - g_oracle|
    1.8e-15 / 1.2e-15."""
    d, _ = _casc_case(40, seed)
    Q = CS.casc_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], _dyn_params(), CS.casc_weights(_casc_cfg(40)), tyre="linear")
    with _casc_ctx(40, 3, solver=2) as c:
        H, g = c.condense(d["x0"], d["ubar"].copy(), d["kappa"], d["ds"])
    errH = (np.abs(H - Q["H"]) / np.abs(Q["H"]).max(axis=(1, 2), keepdims=True)).max()
    errg = (np.abs(g - Q["g"]) / np.abs(Q["g"]).max(axis=1, keepdims=True)).max()
    print(f"casc_sqp linear seed {seed}: rel |H - H_oracle| {errH:.2e}, rel |g - g_oracle| {errg:.2e}")
    assert errH < 1e-9 and errg < 1e-9


def test_casc_sqp_linear_matches_stagewise():
    """M = 40, linear tyre: the stagewise kernel (oracle parity above) and the condensed
    casc_sqp.hip (qp.solver = 2) agree, with the asserts of
    test_gpu_casc_ric.py::test_casc_ric_matches_condensed_kernel.
    Measured on an MI355X: scaled |du*| 3.7e-9 on the 32 of 32 problems solved by both."""
    from vcmpc.workload import cascaded_batch
    B = 32
    d = cascaded_batch(B, seed=5, tyre="linear")
    with _casc_ctx(40, B, solver=0) as c:
        r0 = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy())
    with _casc_ctx(40, B, solver=2) as c:
        r2 = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy())
    ok = (r0[3] == 0) & (r2[3] == 0)
    assert ok.any()
    err = np.abs((r0[2] - r2[2]) / _scale(40))[ok].max()
    print(f"linear tyre, stagewise vs condensed on {ok.sum()} problems solved by both: scaled |du*| {err:.2e}; "
          f"solved {np.mean(r0[3] == 0):.3f} vs {np.mean(r2[3] == 0):.3f}")
    assert err < U_TOL
    assert (r0[3] == 0).mean() >= (r2[3] == 0).mean()
