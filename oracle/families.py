"""Row-family bookkeeping of the oracle's QPs (TEST INFRASTRUCTURE ONLY).

Every inequality row of dyn_qp, casc_qp and kin_qp belongs to a *family* -- one constraint of the
NLP, repeated over the stages.  The builders name each row as they append it (their ``rows`` entry:
a list of (family, stage) in the order of C's rows), so the names cannot drift from the loops that
build C.  This module turns a solved history into the answer to "which families bind, where, and how
hard", which is what decides whether a parity test can see a kernel that linearises a family wrongly:
a row that binds at no optimum has no effect on a polished u*.

A row *binds* in a QP when its multiplier exceeds LAM_BIND (its slack is then zero to the solver's
precision); SLACK_BIND is the alternative for a solver that reports no multipliers.
"""
from __future__ import annotations

import numpy as np

LAM_BIND = 1e-6
SLACK_BIND = 1e-9

DYN_FAMILIES = ("Ux_min", "delta_max", "delta_min", "peng", "tyre_f_up", "tyre_f_lo", "tyre_r_up", "tyre_r_lo",
                "w_up", "w_dn", "trust_Fx_up", "trust_Fx_dn")
CASC_FAMILIES = DYN_FAMILIES + ("V_min", "peng_pm", "trust_Fy_up", "trust_Fy_dn")
KIN_FAMILIES = ("a_up", "a_dn", "w_up", "w_dn", "v_min", "delta_max", "delta_min")


def row_families(Q):
    """Family name of every row of Q["C"] (Q from dyn_qp / casc_qp / kin_qp), as an array of str."""
    return np.array([f for f, _ in Q["rows"]])


def row_stages(Q):
    """Stage index of every row of Q["C"]."""
    return np.array([k for _, k in Q["rows"]])


def binding(hist, lam_bind=LAM_BIND):
    """Which families bind in a solved SQP history.

    hist: the ``hist`` list of dyn_sqp_solve / casc_sqp_solve, or [Q] with Q = kin_ltv_solve's result
    (a one-QP history); each record holds ``rows``, ``lam`` [B, m] and, where the solver kept them,
    ``slack`` [B, m] (otherwise C, d and z / dz, from which the slack is rebuilt).
    Returns out[b][q] = {family: dict(lam=largest multiplier, slack=smallest slack, rows=number of rows
    with multiplier > lam_bind, stages=their stage indices)} over the families that have a row with
    multiplier > lam_bind in QP q of problem b."""
    B = np.asarray(hist[0]["lam"]).shape[0]
    out = [[{} for _ in hist] for _ in range(B)]
    for q, rec in enumerate(hist):
        fam, stg = row_families(rec), row_stages(rec)
        lam = np.asarray(rec["lam"])
        if "slack" in rec:
            slack = np.asarray(rec["slack"])
        else:
            z = rec["z"] if "z" in rec else rec["dz"]
            slack = rec["d"] - np.einsum("bmn,bn->bm", rec["C"], z)
        assert lam.shape[1] == len(fam) == slack.shape[1]
        for b in range(B):
            act = lam[b] > lam_bind
            for f in np.unique(fam[act]):
                m = fam == f
                out[b][q][str(f)] = dict(lam=float(lam[b, m].max()), slack=float(slack[b, m].min()),
                                         rows=int((act & m).sum()), stages=stg[act & m].tolist())
    return out


def family_summary(hist, family, b=0, lam_bind=LAM_BIND):
    """(QPs in which `family` binds for problem b, its largest multiplier over them, the most rows bound
    in one QP).  ([], 0.0, 0) when it never binds."""
    per_qp = binding(hist, lam_bind)[b]
    qps = [q for q, fams in enumerate(per_qp) if family in fams]
    if not qps:
        return [], 0.0, 0
    return qps, max(per_qp[q][family]["lam"] for q in qps), max(per_qp[q][family]["rows"] for q in qps)
