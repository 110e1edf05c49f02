"""CPU: the oracle's row-family bookkeeping (oracle/families.py) and the three preconditions -- clean,
binding, discriminating -- of every case of tests/test_gpu_row_families.py, through the code that the GPU
test runs before it calls a kernel (tests/row_family_cases.py)."""
import numpy as np
import pytest

import row_family_cases as R
from oracle import casc_sqp as CS
from oracle import dyn_sqp as D
from oracle import families as F
from oracle import ltv_qp as Q


def _weights(kind, trust):
    from vcmpc.config import load_config
    if kind == "dyn":
        W = D.dyn_weights(load_config("singletrack_mpc"))
    elif kind == "casc":
        cfg = load_config("cascaded_mpc")
        cfg["horizon_pm"] = R.CASC_M
        W = CS.casc_weights(cfg)
    else:
        W = Q.kin_weights(load_config("kinematic_mpc"))
        W.update(trust_a=1.0 if trust else 0.0, trust_w=0.1 if trust else 0.0)
        return W
    W.update(trust_Fx=2000.0 if trust else 0.0, trust_w=0.2 if trust else 0.0)
    return W


@pytest.mark.parametrize("trust", [True, False], ids=["trust", "no-trust"])
@pytest.mark.parametrize("kind", ["dyn", "casc", "kin"])
def test_row_names_match_builder(kind, trust, dyn_params):
    """One name per row of C at the smallest horizons (N = 20; 20 + 15), trust region on and off; the rows
    whose content can be told from C alone sit where their name says."""
    N, Mh = R.N_ST, R.CASC_M
    W = _weights(kind, trust)
    if kind == "dyn":
        d = R.st_problem(N, 12.0, 500.0, 0.01, -1.0)
        qp = D.dyn_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], dyn_params, W, "fiala")
        per_stage = {f: N for f in F.DYN_FAMILIES}
        per_stage.update(Ux_min=N - 1, delta_max=N - 1, delta_min=N - 1)
        unit = {"w_up": (1, 1.0), "w_dn": (1, -1.0), "trust_Fx_up": (0, 1.0), "trust_Fx_dn": (0, -1.0)}
    elif kind == "casc":
        d = R.casc_problem(12.0, 500.0, 0.01, -1.0)
        qp = CS.casc_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], dyn_params, W, "fiala")
        per_stage = {f: N for f in F.DYN_FAMILIES}
        per_stage.update(Ux_min=N - 1, delta_max=N - 1, delta_min=N - 1, V_min=Mh, peng_pm=Mh,
                         trust_Fx_up=N + Mh, trust_Fx_dn=N + Mh, trust_Fy_up=Mh, trust_Fy_dn=Mh)
        unit = {"w_up": (1, 1.0), "w_dn": (1, -1.0), "trust_Fx_up": (0, 1.0), "trust_Fx_dn": (0, -1.0),
                "trust_Fy_up": (1, 1.0), "trust_Fy_dn": (1, -1.0)}
    else:
        d = R.kin_problem(N, 8.0, 0.5)
        qp = Q.kin_qp(d["x0"], d["ubar"], d["kappa"], d["ds"], 2.5, W)
        per_stage = dict(a_up=N, a_dn=N, w_up=N, w_dn=N, v_min=N - 1, delta_max=N - 1, delta_min=N - 1)
        unit = {"a_up": (0, 1.0), "a_dn": (0, -1.0), "w_up": (1, 1.0), "w_dn": (1, -1.0)}
    if not trust:
        per_stage = {f: n for f, n in per_stage.items() if not f.startswith("trust_")}
    fam, stg = F.row_families(qp), F.row_stages(qp)
    C = qp["C"][0]
    assert len(fam) == C.shape[0] == qp["d"].shape[1]
    assert {f: int((fam == f).sum()) for f in np.unique(fam)} == per_stage
    for f, (col, sign) in unit.items():
        if f not in per_stage:
            continue
        for i in np.nonzero(fam == f)[0]:
            e = np.zeros(C.shape[1])
            e[2 * stg[i] + col] = sign
            np.testing.assert_array_equal(C[i], e)
    # a state row of stage k depends on no input of stage k or later
    for f in ("Ux_min", "delta_max", "v_min", "V_min"):
        for i in np.nonzero(fam == f)[0]:
            assert not C[i, 2 * stg[i]:].any() and (stg[i] == 1 or C[i, :2 * stg[i]].any())


def test_binding_reports_what_the_multipliers_say():
    """binding() on a hand-made record: the family with a multiplier above the threshold, its largest
    multiplier, smallest slack and stages; nothing for the idle family."""
    rec = dict(rows=[("a", 0), ("a", 1), ("b", 0), ("b", 1)], lam=np.array([[0.0, 0.5, 1e-9, 0.0]]),
               slack=np.array([[0.3, 0.0, 0.2, 0.1]]))
    out = F.binding([rec])
    assert out == [[{"a": dict(lam=0.5, slack=0.0, rows=1, stages=[1])}]]
    assert F.family_summary([rec], "a") == ([0], 0.5, 1) and F.family_summary([rec], "b") == ([], 0.0, 0)


@pytest.mark.parametrize("kernel,family,tyre", R.CASES, ids=R.CASE_IDS)
def test_case_preconditions(kernel, family, tyre):
    """Clean, binding, discriminating (tests/row_family_cases.py), at 100 x the bar of the kernel under test."""
    case = R.get_case(kernel, family, tyre)
    info = R.assert_preconditions(case, R.bars(kernel, tyre)[0], R.CASE_IDS[R.CASES.index((kernel, family, tyre))])
    print(f"{kernel} {family} {tyre}: binds in QPs {info['qps']}, up to {info['rows']} rows, largest multiplier "
          f"{info['lam']:.3g}; family off moves u* by {info['moved']:.3g} (scaled)")
