"""GPU: every inequality-row family of the SQP / QP contracts on its bound, kernel against the fp64 oracle.

A row that binds at no optimum has no effect on a polished u*, so a kernel may linearise it wrongly -- sign,
stage index, a partial through cos(alpha) or the load transfer, the 1 / S scale -- and still pass every
parity test on the samplers' problems, on which most families are idle (counted with
oracle/families.py::binding on dynamic_batch, cascaded_batch, kinematic_batch and the golden sets: only the
w box, the trust rows and the kinematic a / w / delta boxes bind).  Each case here is a problem on which one
family binds (tests/row_family_cases.py, which documents the inputs); before a kernel runs, the oracle's own
solve must be clean, the family must carry a multiplier > 1e-6 in some QP, and switching the family off
through its parameters must move u* by at least 100 x the bar, so a kernel that ignored or mis-signed the row
fails by two orders.  tests/test_row_families.py runs the same three preconditions without a device.

Coverage table: kernel x row family -> test.  A new row family or cost branch gets a line here and a case.
[f] = test_row_family_vs_oracle[<kernel>-<family>-fiala / -linear] of this file.

    kernel     row family                                   test
    ---------  -------------------------------------------  ----------------------------------------------------
    st_sqp     Ux_min, delta_max, delta_min, peng,          [f] st_sqp_kernel<20, tyre>, fp64, singletrack_mpc.yaml
               tyre_f_up, tyre_f_lo, tyre_r_up, tyre_r_lo
    st_sqp     w_up, w_dn, trust_Fx_up, trust_Fx_dn         test_gpu_instantiations.py::test_st_sqp_instantiations_vs_oracle
    st_sqp     delta box tightened to +-0.05                test_gpu_sqp_infeasible.py::test_feasible_problems_unchanged
                                                            (u* of the feasible problems against the oracle, 1e-5)
    dyn_sqp    the same eight                               [f] dyn_sqp_kernel<40>, fp32, dynamic_mpc.yaml, at U_TOL /
                                                            U_TOL_FIALA / X_TOL of test_gpu_dyn_sqp.py
    dyn_sqp    w_up, w_dn, trust_Fx_up, trust_Fx_dn         test_gpu_dyn_sqp.py::test_sqp_vs_golden
    casc_ric   the same eight, V_min, peng_pm               [f] casc_ric_kernel<20, 15, tyre>, fp64; peng with peng_pm idle
                                                            and peng_pm with peng idle (asserted), since one Peng
                                                            switches both off
    casc_ric   w_up, w_dn, trust_Fx / trust_Fy up, dn       test_gpu_casc_ric.py::test_casc_ric_recorded_tails_vs_oracle,
                                                            test_gpu_instantiations.py::test_casc_ric_linear_vs_oracle
    casc_ric   delta box +-0.05, V_min = 14                 test_gpu_casc_infeasible.py::test_feasible_problems_unchanged
    casc_sqp   the same ten                                 [f] casc_sqp_kernel<20, 40, tyre> (qp.solver = 2), M = 40 inputs
                                                            (CASC40_CASES); peng / peng_pm separated as above
    casc_sqp   w, trust rows                                test_gpu_casc.py::test_solve_vs_golden
    kin_ltv    v_min                                        test_row_family_vs_oracle[kin_ltv-v_min]  (qp.solver = 0)
    kin_ric    v_min                                        test_row_family_vs_oracle[kin_ric-v_min]  (qp.solver = 1)
    kin_ltv    a, w, delta boxes                            test_gpu_parity.py (golden vectors);
                                                            test_gpu_kin_ltv_infeasible.py::test_feasible_problems_solved_bit_for_bit
    kin_ric    a, w, delta boxes                            test_gpu_kin_ric.py::test_kin_ric_horizons_vs_oracle;
                                                            test_gpu_infeasible.py::test_detection_matches_phase1_and_certifies

Inputs that did not work (oracle on the CPU), so that nobody tries them again:
  * tyre_f_up / tyre_r_up from a warm start 6 % beyond the row (6400 / 7300 N): the model's own
    Fymax = sqrt((mu Fz)^2 - (0.99 Fx)^2) is NaN from 1 % beyond; 6100 / 7100 N (0.7 % / 0.2 % beyond) are clean.
  * dyn_sqp (N = 40) braking rows from 25 m/s: the optimum brakes less than the tyres allow; from 35 - 40 m/s the
    terminal over-speed hinge holds it on the row.  The same on the cascaded tail.
  * cascaded V_min a little under the entry speed with a braking tail (V_min 14, 15 m/s, tail -1500 N): binds at
    M = 15 in QP 0 only, at M = 40 the first QP is infeasible or the row idle; an entry above max_speed with V_min
    under it (24 under 26 m/s) binds in every QP at both tails.
  * casc_sqp (M = 40) with the M = 15 inputs: braking rows and Ux_min -- the 120 m tail at the single-track warm
    start stops the car, first QP infeasible; traction rows and peng -- the tail reaches max_speed by itself, rows
    idle.  With the tail near the drag level (-3000 / -2000 N braking, 1500 N traction, 300 N for Ux_min from
    -1800 N) they bind; tails of -4500 / -3000 N (braking), 2500 / 2000 N (traction) leave them idle.
  * peng with the tail at the same warm start as the single-track part (3800 N): peng_pm binds too; from 4100 N
    (beyond the row) with the tail at 1500 N peng binds alone, from 2000 N with the tail at 3800 N peng_pm alone.
  * cascaded delta rows from ey0 = -+2 (the single-track inputs): idle, the tail corrects ey; from ey0 = -+3.5,
    outside the boundary, they bind in every QP.

Hinge branches of the cost, frozen at the prediction (stage-iterations on which the branch is active, counted
with the oracle over every SQP iterate):
    ey boundary low     st_sqp  test_gpu_instantiations.py::test_st_sqp_instantiations_vs_oracle[30-fiala] (118);
                        casc_ric [casc_ric-delta_max-*] (ey0 = -3.5); tail: test_casc_ric_recorded_tails_vs_oracle[35] (68);
                        kinematic: golden vectors (124)
    ey boundary high    casc_ric [casc_ric-delta_min-*] (ey0 = +3.5); tail: test_casc_ric_recorded_tails_vs_oracle[25] (33);
                        kinematic: golden vectors (44)
    front slip          st_sqp test_st_sqp_instantiations_vs_oracle[20-linear] (83), [20-fiala] (114);
                        casc_ric test_casc_ric_recorded_tails_vs_oracle[15] (60)
    rear slip           st_sqp test_st_sqp_instantiations_vs_oracle[20-linear] (34);
                        casc_ric test_casc_ric_recorded_tails_vs_oracle[35] (6)
    terminal over-speed dyn_sqp [dyn_sqp-tyre_f_lo-*], [dyn_sqp-tyre_r_lo-*]; casc_ric [casc_ric-tyre_f_lo-*],
                        [casc_ric-V_min-*], test_casc_ric_recorded_tails_vs_oracle[35] (3); casc_sqp [casc_sqp-V_min-*];
                        kinematic [kin_ltv-v_min], [kin_ric-v_min], golden vectors (2)

The fp32 kernel and its polish.  dyn_sqp stops its interior point at qp.tol = 1e-5 and gets the remaining digits
from an active-set polish of at most qp.polish rounds; a QP on which no round is certified keeps the interior-point
iterate and still reports status 0.  dynamic_mpc.yaml asked for 3 rounds, with which the families that bind on part
of the horizon were not certified (measured on an MI355X, scaled |u* - u*_oracle|): peng (rows 18 .. 39 bind) 1 QP
of 3 certified, 5.7e-2; delta_max / delta_min (rows 7 .. 39) none, 4.4e-3 linear, 3.7e-3 Fiala -- the interior
point's own accuracy (7.7e-2 with the polish off), not the rows: st_sqp_kernel<40> in fp64 with the same parameters
is at 3e-15 and 2e-9.  peng is certified from 6 rounds on, delta from 12, so dynamic_mpc.yaml (and the default of
vcmpc.config) now asks for 12; a QP certified earlier stops there.  The cases run the shipped config and assert the
certificate of every QP.
What the delta cases found in the kernel.  With every QP certified, [dyn_sqp-delta_max-linear] and
[dyn_sqp-delta_min-linear] measured 3.4e-4 against U_TOL = 1e-4, all of it in w (Fx at 3e-7): x* left delta 5.5e-6
over its bound at the first strongly active stage.  The polish's augmented-Lagrangian passes stopped at a residual
of eps_r = 5e-7 (1 + max |d|), and max |d| is Ux - Ux_min ~ 10 on every problem, so 5e-6 rad was "converged" on a
delta row -- 2e-4 rad/s in the neighbouring w (ds / Ux = 0.03 s).  The passes now stop at 5e-7 on the rows' own
O(1) scale (at most 12 passes as before; the certificate is unchanged): 6.4e-5 linear, 2.8e-5 Fiala.  Figures and
the runs behind them: profiles/row_families/.

Bars (the project's own): 1e-5 on u* (single track fp64: Fx in N, w in rad/s; cascaded: the scaled variable
Fx / 1000, w, Fy / 1000; kinematic: a, w) and 1e-6 on x*; the fp32 kernel at test_gpu_dyn_sqp.py's.
"""
import numpy as np
import pytest

import row_family_cases as R

pytestmark = pytest.mark.gpu


def _solve(kernel, case):
    """The case through vc_solve, the kernel's parameters packed from the case's own config dicts."""
    from vcmpc import Context, _abi
    from vcmpc.config import make_params
    cfgs, d = case["cfgs"], case["d"]
    if kernel in ("kin_ltv", "kin_ric"):
        p = make_params(kin_car=cfgs["car"], kin_mpc=cfgs["mpc"])
        model, N, dt = _abi.VC_MODEL_KINEMATIC, case["N"], _abi.VC_F64
    else:
        p = make_params(dyn_car=cfgs["car"], dyn_mpc=cfgs["mpc"], tyre=case["tyre"])
        model = _abi.VC_MODEL_DYNAMIC if kernel in ("st_sqp", "dyn_sqp") else _abi.VC_MODEL_CASCADED
        N = case.get("N", R.N_ST)
        dt = _abi.VC_F32 if kernel == "dyn_sqp" else _abi.VC_F64
    f = np.float32 if dt == _abi.VC_F32 else np.float64
    a = {k: np.ascontiguousarray(v, f) for k, v in d.items()}   # copies: the case is never modified
    with Context(model=model, N=N, max_batch=1, dtype=dt, params=p) as c:
        if kernel == "dyn_sqp":   # vc_solve_diag: the same solve, plus the polish certificates
            return c.solve(a["x0"], a["kappa"], a["ds"], a["ubar"].copy(), diag=True)
        return c.solve(a["x0"], a["kappa"], a["ds"], a["ubar"].copy()) + (None,)


@pytest.mark.parametrize("kernel,family,tyre", R.CASES, ids=R.CASE_IDS)
def test_row_family_vs_oracle(kernel, family, tyre):
    """One family on its bound.  Measured on an MI355X: profiles/row_families/test_gpu_row_families.log."""
    what = R.CASE_IDS[R.CASES.index((kernel, family, tyre))]
    u_bar, x_bar = R.bars(kernel, tyre)
    case = R.get_case(kernel, family, tyre)
    info = R.assert_preconditions(case, u_bar, what)
    ref = case["ref"]
    u0, xs, us, st, it, dg = _solve(kernel, case)
    err_u = np.abs((np.asarray(us, np.float64) - ref["u_star"]) / case["scale"]).max()
    err_x = np.abs(np.asarray(xs, np.float64) - ref["x_star"]).max()
    print(f"{what}: |u* - u*_oracle| = {err_u:.3e} (bar {u_bar:g}), |x* - x*_oracle| = {err_x:.3e} (bar {x_bar:g}), "
          f"status {st.tolist()}, iterations {it.tolist()}; {family} binds in QPs {info['qps']}, up to {info['rows']} rows, "
          f"largest multiplier {info['lam']:.3g}; family off moves u* by {info['moved']:.3g}; oracle's smallest alpha "
          f"{info['alpha']:g}")
    assert (st == 0).all(), st
    if kernel == "dyn_sqp":   # every QP converged and polish-certified, as test_gpu_dyn_sqp.py::test_sqp_vs_golden asks
        assert (int(dg[0, 2]) & 6) == 6, dg
    assert err_u < u_bar
    assert err_x < x_bar
    np.testing.assert_array_equal(u0, us[:, 0])
