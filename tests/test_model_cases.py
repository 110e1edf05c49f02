"""CPU: the case builders of tests/model_cases.py -- the preconditions and the mutation margins of every case
of tests/test_gpu_models.py, through the code that the GPU test runs before it calls a kernel -- and the
oracle's kinematic model in the precision of its inputs.  Prints the per-column units (pytest -s)."""
import numpy as np
import pytest

import model_cases as C
from oracle import models as M

CASES = {"kin_points": C.kin_points, "kin_horizons": C.kin_horizons}
for _t in C.TYRES:
    CASES[f"dyn_points-{_t}"] = lambda t=_t: C.dyn_points(t)
    CASES[f"dyn_horizons-{_t}"] = lambda t=_t: C.dyn_horizons(t)


@pytest.mark.parametrize("name", list(CASES))
def test_case_preconditions_and_margins(name):
    """Every precondition holds, every mutation moves some column by at least 100 x its bar in each dtype, the
    inputs are float32 numbers, and the fp32 bar is built from the reference's own error alone."""
    case = CASES[name]()
    C.assert_preconditions(case)
    print(C.describe(case, name))
    for k, v in case["d"].items():
        assert v.dtype == np.float64 and np.array_equal(v, v.astype(np.float32).astype(np.float64)), k
    for e, ref in case["ref"][C.F64].items():
        e_col, bar = C.unit_and_bar32(ref, case["ref"][C.F32][e])
        np.testing.assert_array_equal(bar, case["bar32"][e])
        assert (bar >= 32 * e_col).all() and (bar > 0).all() and np.isfinite(bar).all()
    want = {"kin_points": set(), "kin_horizons": {"ds_rolled", "kappa_rolled", "ubar_rolled"}}
    params = {"Caf_Car_swapped", "other_tyre"} | ({"muf_mur_swapped"} if name.endswith("fiala") else set())
    want.update({f"dyn_points-{t}": params for t in C.TYRES})
    want.update({f"dyn_horizons-{t}": params | want["kin_horizons"] for t in C.TYRES})
    assert set(case["margins"]) == want[name]
    smallest = min((m for by in case["margins"].values() for dt in by.values() for m in dt.values()), default=None)
    print(f"{name}: smallest mutation margin {smallest} x the bar")


def test_shapes_of_the_sets():
    """B = 130 is two blocks of 128 with two live threads in the second; the dynamic set is 65 points, their 65
    mirror images, and the four edge rows; the N = 1 slice is stage 0."""
    assert C.kin_points()["d"]["x"].shape == (130, 6) and C.kin_horizons()["d"]["ubar"].shape == (5, 20, 2)
    d, mirror_ok = C.dyn_point_inputs()
    assert mirror_ok and d["x"].shape == (130, 8)
    m = C.mirror_points({k: v[4:65] for k, v in d.items()})
    for k in d:
        np.testing.assert_array_equal(m[k], d[k][69:])
    assert not d["x"][0, [1, 2, 3]].any() and d["u"][1:4, 0].tolist() == [-500.0, -4000.0, 4000.0]
    F = M.dyn_forces(d["x"][:1], d["u"][:1], C.dyn_params())
    assert F["alpha_f"][0] == 0.0 and F["alpha_r"][0] == 0.0
    assert C.dyn_points("linear")["d"] is C.dyn_points("fiala")["d"]     # the same points for both tyres
    h = C.dyn_horizons("fiala")["d"]
    one = C.first_stage(h)
    assert one["ubar"].shape == (5, 1, 2) and one["ds"].shape == (5, 1) and one["x0"] is h["x0"]
    np.testing.assert_array_equal(C.dyn_horizons("fiala")["ref"][C.F64]["rollout"][:, 1],
                                  C.dyn_rollout(one, "fiala", C.F64)[:, 1])


def test_fp64_rollout_reference_noise():
    """The oracle's own fp64 rounding along the 40-stage dynamic rollouts, against an 80-bit longdouble
    evaluation, is orders under the 1e-11 x column-maximum bar given to the kernel (measured: at most 9.4e-15
    absolute, 1.7e-15 of the column's largest magnitude)."""
    for tyre in C.TYRES:
        case = C.dyn_horizons(tyre)
        ref = case["ref"][C.F64]["rollout"]
        d = case["d"]
        p = C.dyn_params(np.longdouble)
        x0, ubar, kappa, ds = (d[k].astype(np.longdouble) for k in ("x0", "ubar", "kappa", "ds"))
        x, worst_abs, worst_rel = x0, 0.0, 0.0
        colmax = np.abs(ref).reshape(-1, 8).max(axis=0)
        for k in range(C.DYN_N):
            x = M.dyn_spatial_transition(x, ubar[:, k], kappa[:, k], ds[:, k], p, tyre)
            assert x.dtype == np.longdouble
            err = np.abs(ref[:, k + 1] - x).astype(np.float64).max(axis=0)
            worst_abs, worst_rel = max(worst_abs, err.max()), max(worst_rel, (err / colmax).max())
        print(f"{tyre}: oracle fp64 vs longdouble along the rollout: {worst_abs:.2e} absolute, {worst_rel:.2e} of the "
              f"column maximum")
        assert worst_rel < 1e-13


def test_kinematic_oracle_keeps_its_inputs_dtype():
    """float32 in, float32 out (oracle/models.py's kinematic functions once forced kappa and the step to
    float64); float64 in gives what the forced form gave, bit for bit."""
    d = C.kin_points()["d"]
    L = C.kin_L()
    for dt in (np.float32, np.float64, np.longdouble):
        x, u, k, ds = (d[n].astype(dt) for n in ("x", "u", "kappa", "ds"))
        for out in (M.kin_temporal_ode(x, u, k, dt(L)), M.kin_spatial_ode(x, u, k, dt(L)),
                    M.kin_transition(x, u, k, dt(0.05), dt(L)), M.kin_spatial_transition(x, u, k, ds, dt(L))):
            assert out.dtype == dt
    x, u, k, ds = d["x"], d["u"], d["kappa"], d["ds"]
    forced = x + np.asarray(ds, dtype=np.float64)[..., None] * M.kin_spatial_ode(x, u, np.asarray(k, dtype=np.float64), L)
    np.testing.assert_array_equal(M.kin_spatial_transition(x, u, k, ds, L), forced)
    np.testing.assert_array_equal(M.kin_transition(x, u, k, 0.05, L), x + 0.05 * M.kin_temporal_ode(x, u, k, L))
    np.testing.assert_array_equal(M.kin_spatial_transition(x, u, list(k), list(ds), L), forced)
