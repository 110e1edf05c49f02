"""GPU: the merit line search of the kinematic SQP step (csrc/kin_merit.hip) on its own, branch by
branch, through the test hook vc_debug_kin_merit (Context.debug_kin_merit), against
oracle/kin_sqp.py merit / line_search / line_search_ms / noise_step on the same input bits.

Problem sets (no QP is solved on the CPU except in the natural-restart test): N = 20, the 44
problems of tests/golden/obs_golden.npz with its 7 obstacles (kin_ubar; kin_u_star as a QP
solution); N = 50, the 32 n50_* problems of kin_nlp_obs_golden.npz (n50_ubar; n50_u_nlp as a
target), where the kernel's 64-lane strided loops over 2N = 100 and (N+1)*6 = 306 elements wrap.
Directions are synthetic, u_qp = u_prev + t (target - u_prev); "restore" starts are ubar with
the steering rate 0.9 at every stage (outside the model's domain, phi0 = inf).

Merit parity, measured on an MI355X over every set below (profiles/merit/test_gpu_kin_merit.log):
max |phi_gpu - phi_ref| / max(1, |phi_ref|) = 2.134e-14 (single shooting 8.8e-15, multiple shooting
2.1e-14; MEASURED_PARITY rounds it up); BAR is ten times that (the kernel contracts to FMA and uses
the device's cos / tan), 2.2e-13, far below the 1e-9 at which a dropped
stage, obstacle or slew term (>= 1.7e-7 on the most sensitive problem) would still fail --
test_oracle_merit_terms_exceed_the_bar checks that on the oracle, without a GPU.  D is a one-sided
difference over EPS_FD = 1e-7, so its bar is 2 BAR max(1, |phi0|) / EPS_FD.

Step sizes are discrete: alpha must equal the oracle's exactly outside near-ties (_near_tie; at
most 2 per set, the sets here have none), and every answer, near-tie or not, must be
self-consistent with the kernel's own diagnostics (_self_consistent).
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import kin_sqp as KS
from oracle import ltv_qp as Q

gpu = pytest.mark.gpu

L = 2.5
MEASURED_PARITY = 2.2e-14     # largest seen over all sets (2.134e-14, a multiple-shooting merit)
BAR = 10 * MEASURED_PARITY
U_TOL = 1e-5
IW, IS = Q.IW, Q.IS
EPS_FD, LS = KS.EPS_FD, KS.LS_STEPS
ALPHAS = 0.5 ** np.arange(LS)


# -- problem sets, contexts ---------------------------------------------------------------------
def _cfg(N, ms=0, kin_sqp=1, **qp):
    from vcmpc.config import load_config
    cfg = load_config("kinematic_mpc")
    cfg["horizon"] = N
    cfg["qp"] = dict(cfg["qp"], kin_sqp=kin_sqp, solver=1, ms=ms, **qp)
    return cfg


def _ctx(cfg, obstacles, B, N):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(kin_car=load_config("kinematic_car"), kin_mpc=cfg, obstacles=obstacles)
    return Context(model=_abi.VC_MODEL_KINEMATIC, N=N, max_batch=B, dtype=_abi.VC_F64, params=p)


def _set(N):
    c = np.ascontiguousarray
    if N == 20:
        g = np.load(os.path.join(GOLDEN, "obs_golden.npz"))
        k = dict(x0="kin_x0", kap="kin_kappa", ds="kin_ds", ubar="kin_ubar", target="kin_u_star")
    else:
        g = np.load(os.path.join(GOLDEN, "kin_nlp_obs_golden.npz"))
        k = dict(x0="n50_x0", kap="n50_kappa", ds="n50_ds", ubar="n50_ubar", target="n50_u_nlp")
    P = SimpleNamespace(N=N, **{a: c(g[b].astype(np.float64)) for a, b in k.items()})
    P.obs = [tuple(float(v) for v in o) for o in g["obstacles"]]
    P.W = Q.kin_weights(_cfg(N))
    P.W["obstacles"] = P.obs
    P.B = len(P.x0)
    P.bad = P.ubar.copy()          # outside the model's domain: the steering angle runs away
    P.bad[:, :, IW] = 0.9
    return P


@pytest.fixture(scope="module")
def P20():
    return _set(20)


@pytest.fixture(scope="module")
def P50():
    return _set(50)


@pytest.fixture(scope="module")
def dev20(P20):
    """Device-side targets of the N = 20 set, computed once: the converged 8-iteration SQP
    solution, one more QP solution from it, and a 6-iteration solution for the multiple-shooting
    state iterate of test_kin_sqp_multiple_shooting_vs_oracle."""
    P = P20
    out = {}
    for S in (8, 6):
        with _ctx(_cfg(20, kin_sqp=S), P.obs, P.B, 20) as c:
            r = c.solve(P.x0, P.kap, P.ds, P.ubar.copy())
        assert (r[3] == 0).all()
        out[S] = r[2]
    with _ctx(_cfg(20, kin_sqp=0), P.obs, P.B, 20) as c:     # one plain QP step at the converged iterate
        r = c.solve(P.x0, P.kap, P.ds, out[8].copy())
    out["qp"] = r[2]
    return SimpleNamespace(conv=out[8], six=out[6], qp=out["qp"])


def _sub(P, idx):
    """The problems idx of a set."""
    return SimpleNamespace(N=P.N, B=len(idx), W=P.W, obs=P.obs,
                           **{k: np.ascontiguousarray(getattr(P, k)[idx]) for k in ("x0", "kap", "ds", "ubar", "target", "bad")})


# -- the device side ----------------------------------------------------------------------------
def _launch(c, P, up, uq, status=None, iters=None, st_acc=None, it_acc=None, first=True, restart=False,
            xp=None, xq=None):
    B = len(up)
    i32 = lambda a: np.zeros(B, np.int32) if a is None else np.array(a, np.int32)
    st, it, sa, ia = i32(status), i32(iters), i32(st_acc), i32(it_acc)
    u = np.array(uq, np.float64)
    kw = {} if xp is None else dict(x_prev=np.ascontiguousarray(xp), x=np.array(xq, np.float64))
    u0, x, u, st, it, d = c.debug_kin_merit(P.x0, P.kap, P.ds, np.ascontiguousarray(up), u, st, it, sa, ia,
                                            first=first, restart=restart, **kw)
    return SimpleNamespace(alpha=d[:, 0].copy(), phi0=d[:, 1].copy(), phia=d[:, 2].copy(), D=d[:, 3].copy(), u=u,
                           x=x, u0=u0, status=st, iters=it, st_acc=sa, it_acc=ia)


# -- the oracle side ----------------------------------------------------------------------------
def _rel(a, ref):
    """|a - ref| / max(1, |ref|), 0 where both are the same infinity."""
    with np.errstate(invalid="ignore"):
        e = np.abs(a - ref) / np.maximum(1.0, np.abs(ref))
    return np.where((a == ref) & ~np.isfinite(ref), 0.0, e)


def _candidates(P, up, dz, xp=None, dx=None):
    """phi of the 24 candidates [24, B] (the rollout's, or the state iterate's with xp / dx)."""
    if xp is None:
        return np.array([KS.merit(P.x0, up + a * dz, P.kap, P.ds, L, P.W) for a in ALPHAS])
    return np.array([KS.merit(P.x0, up + a * dz, P.kap, P.ds, L, P.W, x=xp + a * dx) for a in ALPHAS])


def _domain_gap(P, up, dz):
    """[24, B]: the smallest |v - V_DOM|, |EPSI_DOM - |epsi||, |rho| over stages 0..N-1 of each candidate."""
    out = []
    for a in ALPHAS:
        with np.errstate(all="ignore"):
            x = Q.kin_predict(P.x0, up + a * dz, P.kap, P.ds, L)[:, :P.N]
            q = np.stack([x[:, :, Q.IV] - KS.V_DOM, KS.EPSI_DOM - np.abs(x[:, :, Q.IEP]), 1.0 - x[:, :, Q.IEY] * P.kap])
        out.append(np.nanmin(np.abs(q), axis=(0, 2)))
    return np.array(out)


def _near_tie(alpha, phi0, D, cand, gap=None):
    """Problems whose step size the oracle itself decides within rounding: a candidate at or above
    the accepted size within 1e-9 max(1, |phi0|) of the Armijo threshold, |D| below
    4 BAR max(1, |phi0|) / EPS_FD, or (restore) a candidate's domain quantity within 1e-9 of zero."""
    fin = np.isfinite(phi0)
    sc = np.maximum(1.0, np.abs(np.where(fin, phi0, 0.0)))
    jacc = np.where(alpha > 0, np.round(-np.log2(np.where(alpha > 0, alpha, 1.0))), LS - 1).astype(int)
    seen = np.arange(LS)[:, None] <= jacc[None, :]
    with np.errstate(invalid="ignore"):
        thr = phi0[None, :] + KS.ARMIJO * ALPHAS[:, None] * D[None, :]
        t_a = (seen & np.isfinite(cand) & fin[None, :] & (np.abs(cand - thr) < 1e-9 * sc[None, :])).any(axis=0)
        t_b = fin & (np.abs(D) < 4 * BAR * sc / EPS_FD)
    t_c = np.zeros_like(t_a) if gap is None else (~fin & (seen & (gap < 1e-9)).any(axis=0))
    return t_a | t_b | t_c


def _self_consistent(r, phi_ret):
    """From the kernel's own diagnostics: an accepted step from a finite merit passed the Armijo
    test or the noise rule, and the oracle's merit of what came back is phi(accepted)."""
    acc = (r.alpha > 0) & np.isfinite(r.phi0)
    sc = np.maximum(1.0, np.abs(r.phi0))
    with np.errstate(invalid="ignore"):
        armijo = (r.D < 0) & (r.phia <= r.phi0 + KS.ARMIJO * r.alpha * r.D)
        noise = (r.alpha == 1.0) & (np.abs(r.D) <= KS.NOISE_D * sc) & (r.phia <= r.phi0 + KS.NOISE_PHI * sc)
    assert (armijo | noise)[acc].all(), np.nonzero(acc & ~(armijo | noise))[0]
    assert np.isfinite(r.phia[r.alpha > 0]).all()
    e = _rel(r.phia, phi_ret)
    assert e.max() <= BAR, (e.max(), e.argmax())
    return int((acc & ~armijo & noise).sum())


def _hist(alpha):
    v, n = np.unique(alpha, return_counts=True)
    return {float(a): int(k) for a, k in zip(v[::-1], n[::-1])}


def _check_ss(c, P, up, uq, name, restore=False, cap=2):
    """One single-shooting launch against line_search: every item of the issue's list.  Returns
    (device result, oracle (alpha, phi0, phia, D), candidates, near-tie mask)."""
    dz = uq - up
    ref = KS.line_search(P.x0, up, dz, P.kap, P.ds, L, P.W)
    cand = _candidates(P, up, dz)
    tie = _near_tie(ref[0], ref[1], ref[3], cand, _domain_gap(P, up, dz) if restore else None)
    r = _launch(c, P, up, uq)
    xr = c.rollout(P.x0, r.u, P.kap, P.ds)
    fin = np.isfinite(ref[1])
    e0, ea = _rel(r.phi0, ref[1]), _rel(r.phia, ref[2])
    sc = np.maximum(1.0, np.abs(np.where(fin, ref[1], 0.0)))
    eD = np.abs(r.D[fin] - ref[3][fin]) / (sc[fin] / EPS_FD) if fin.any() else np.zeros(1)
    ninf = int((~np.isfinite(cand)).any(axis=0).sum())
    print(f"{name}: B {P.B}; alpha {_hist(r.alpha)} (oracle {_hist(ref[0])}); near-ties {np.nonzero(tie)[0].tolist()}; "
          f"restore (phi0 = inf) {int((~fin).sum())}; problems with an infinite candidate {ninf}; "
          f"phi0 err {e0.max():.2e}, phi(acc) err {ea[~tie].max() if (~tie).any() else 0.0:.2e}, "
          f"D err x EPS_FD / max(1, |phi0|) {eD.max():.2e}")
    if cap is not None:
        assert tie.sum() <= cap, np.nonzero(tie)[0]
    np.testing.assert_array_equal(r.alpha[~tie], ref[0][~tie])
    assert e0.max() <= BAR and ea[~tie].max(initial=0.0) <= BAR
    assert eD.max() <= 2 * BAR
    assert not np.isfinite(r.D[~fin]).any()
    exp = np.where((r.alpha > 0)[:, None, None], up + r.alpha[:, None, None] * (uq - up), up)
    np.testing.assert_array_equal(r.u, exp)
    np.testing.assert_array_equal(r.u0, r.u[:, 0])
    assert np.abs(r.x - xr).max() <= 1e-12 * (1.0 + np.abs(xr).max())
    nz = _self_consistent(r, KS.merit(P.x0, r.u, P.kap, P.ds, L, P.W))
    return r, ref, cand, tie, nz


def _phi_gpu(c, P, u, x=None):
    """phi(u) from the kernel: the hook with u = u_prev, so dz = 0 and ls_diag[:, 1] = phi(u_prev)."""
    return _launch(c, P, u, u, xp=x, xq=x).phi0


# -- merit parity -------------------------------------------------------------------------------
SCALES = {20: (1.0, 8.0, 64.0, 200.0, 1000.0, -1.0), 50: (1.0, 8.0)}


def _merit_points(P):
    pts = [("ubar", P.ubar), ("target", P.target), ("out of domain", P.bad)]
    pts += [(f"ubar + {t:g} dz", P.ubar + t * (P.target - P.ubar)) for t in SCALES[P.N]]
    return pts


@gpu
@pytest.mark.parametrize("N", [20, 50])
def test_merit_parity(P20, P50, N):
    """phi from the kernel against oracle merit at ubar, the targets, the scaled steps and the
    out-of-domain starts (inf must equal inf).  Measured: see the module docstring."""
    P = P20 if N == 20 else P50
    worst, ninf, ext = 0.0, 0, 0
    with _ctx(_cfg(N), P.obs, P.B, N) as c:
        for name, u in _merit_points(P):
            ref = KS.merit(P.x0, u, P.kap, P.ds, L, P.W)
            e = _rel(_phi_gpu(c, P, np.ascontiguousarray(u)), ref)
            ninf += int((~np.isfinite(ref)).sum())
            worst = max(worst, e.max())
            print(f"N={N} {name}: inf {int((~np.isfinite(ref)).sum())}, max rel err {e.max():.3e}")
            assert e.max() <= BAR, (name, e.argmax())
        x = Q.kin_predict(P.x0, P.ubar, P.kap, P.ds, L)
        for so, eo, r in P.obs:
            d = np.sqrt((x[:, 1:N, IS] - so) ** 2 + (x[:, 1:N, Q.IEY] - eo) ** 2) - (r + 0.1)
            ext = max(ext, int((d < P.W["obs_margin_min"]).any(axis=1).sum()))
    print(f"N={N}: merit parity over all points {worst:.3e} (bar {BAR:.1e}); infinite merits {ninf}; problems on "
          f"the extended barrier at ubar, most of any obstacle {ext}")
    assert ninf >= P.B          # the out-of-domain starts at least
    assert ext >= 3


@gpu
def test_merit_parity_multiple_shooting(P20, dev20):
    """The multiple-shooting merit (state iterates with nonzero defects: the rollout of the mean of
    ubar and a converged solution, and that moved halfway towards the rollout of the target)."""
    P = P20
    xw = Q.kin_predict(P.x0, 0.5 * (P.ubar + dev20.six), P.kap, P.ds, L)
    xt = 0.5 * (xw + Q.kin_predict(P.x0, P.target, P.kap, P.ds, L))
    with _ctx(_cfg(20, ms=1), P.obs, P.B, 20) as c:
        for name, u, x in (("ubar at xw", P.ubar, xw), ("target at xw", P.target, xw), ("ubar at xt", P.ubar, xt)):
            pm = KS.merit(P.x0, u, P.kap, P.ds, L, P.W, x=x)
            ps = KS.merit(P.x0, u, P.kap, P.ds, L, P.W)
            roll = np.isfinite(ps) & (ps <= pm + KS.TIE * np.abs(pm))
            ref = np.where(roll, ps, pm)
            e = _rel(_phi_gpu(c, P, u, np.ascontiguousarray(x)), ref)
            print(f"ms {name}: state-iterate merit governs on {int((~roll).sum())} of {P.B}; max rel err {e.max():.3e}")
            assert e.max() <= BAR, e.argmax()
            if name == "ubar at xw":
                assert (~roll).sum() >= 10


def _without_one_term(P, u, which):
    """Oracle merit with one single term removed: what a dropped stage or obstacle would compute."""
    x = Q.kin_predict(P.x0, u, P.kap, P.ds, L)
    N, W = P.N, P.W
    if which == "w_dev, last stage":
        t = W["w_dev"] * P.ds[:, N - 1] * x[:, N - 1, Q.IEY] ** 2
    elif which == "w_dev, first stage":
        t = W["w_dev"] * P.ds[:, 1] * x[:, 1, Q.IEY] ** 2
    elif which == "w_w, last stage":
        t = W["w_w"] * u[:, N - 1, IW] ** 2
    elif which == "slew, last pair":
        t = W["w_a"] * (u[:, N - 1, Q.IA] - u[:, N - 2, Q.IA]) ** 2
    else:   # one obstacle at one stage: the largest such term of the problem
        t = np.zeros(P.B)
        for so, eo, r in P.obs:
            d = np.sqrt((x[:, 1:N, IS] - so) ** 2 + (x[:, 1:N, Q.IEY] - eo) ** 2)
            t = np.maximum(t, (W["w_obs"] * P.ds[:, 1:N] * KS.barrier_ext(d - (r + 0.1), W["obs_margin_min"])).max(axis=1))
    return t


@pytest.mark.parametrize("N", [20, 50])
def test_oracle_merit_terms_exceed_the_bar(N):
    """CPU: the bar resolves a single dropped term.  The oracle's merit without one stage's w_dev,
    w_w or slew term, or one obstacle at one stage, differs from itself by more than BAR (relative
    to max(1, |phi|)) on at least one problem of each set -- so an off-by-one in the kernel's stage
    range or obstacle loop fails test_merit_parity."""
    assert BAR <= 1e-9
    P = _set(N)
    worst = {}
    for u in (P.ubar, P.target):        # the points of test_merit_parity with a finite merit
        phi = KS.merit(P.x0, u, P.kap, P.ds, L, P.W)
        fin = np.isfinite(phi)          # (some targets leave the domain: no term to resolve there)
        assert fin.sum() >= P.B // 2
        for which in ("w_dev, last stage", "w_dev, first stage", "w_w, last stage", "slew, last pair", "obstacle"):
            rel = (_without_one_term(P, u, which) / np.maximum(1.0, np.abs(phi)))[fin]
            worst[which] = max(worst.get(which, 0.0), rel.max())
    for which, rel in worst.items():
        print(f"N={N} {which}: removed term / max(1, |phi|), largest of the set {rel:.2e}")
        assert rel > BAR, which


# -- line search, single shooting ---------------------------------------------------------------
@gpu
def test_line_search_n20(P20):
    """The N = 20 rows of the table: t = 1, 8 (Armijo picks down to 2^-6), 64 / 200 / 1000 (down to
    2^-13, every problem with an infinite candidate), -1 (D >= 0: no step)."""
    P = P20
    with _ctx(_cfg(20), P.obs, P.B, 20) as c:
        res = {t: _check_ss(c, P, P.ubar, P.ubar + t * (P.target - P.ubar), f"N=20 t={t:g}") for t in SCALES[20]}
        full = KS.merit(P.x0, P.target, P.kap, P.ds, L, P.W)
    h = _hist(res[1.0][0].alpha)
    assert h.get(1.0, 0) >= 31 and h.get(0.5, 0) >= 6 and h.get(0.25, 0) >= 5 and h.get(0.125, 0) >= 2, h
    assert (~np.isfinite(full)).sum() >= 3           # full-step merit infinite
    a8 = res[8.0][0].alpha
    assert len(np.unique(a8[a8 > 0])) >= 7 and a8[a8 > 0].min() <= 2.0 ** -6, _hist(a8)
    small = 1.0
    for t in (64.0, 200.0, 1000.0):
        r, _, cand, _, _ = res[t]
        assert (~np.isfinite(cand)).any(axis=0).all()       # domain left along the step, every problem
        small = min(small, r.alpha[r.alpha > 0].min())
    assert small <= 2.0 ** -13
    rm = res[-1.0]
    assert (rm[0].alpha == 0).all() and (rm[0].D >= 0).all()
    np.testing.assert_array_equal(rm[0].u, P.ubar)


@gpu
def test_line_search_n50(P50):
    """N = 50 (the strided loops over 2N and 6(N+1) elements wrap): t = 1 and 8, 1 down to 2^-8."""
    P = P50
    with _ctx(_cfg(50), P.obs, P.B, 50) as c:
        res = {t: _check_ss(c, P, P.ubar, P.ubar + t * (P.target - P.ubar), f"N=50 t={t:g}") for t in SCALES[50]}
    a = np.concatenate([res[t][0].alpha for t in SCALES[50]])
    assert a.max() == 1.0 and a[a > 0].min() <= 2.0 ** -8, _hist(a)


@gpu
def test_restore_n20(P20, dev20):
    """From outside the model's domain (phi0 = inf on all 44) the largest step back inside it:
    t = 1, 2, 4 restore with alpha = 1, 1/2, 1/4 on every problem; t = 1.5 with 1/2 on 7, none on 37."""
    P = P20
    with _ctx(_cfg(20), P.obs, P.B, 20) as c:
        res = {t: _check_ss(c, P, P.bad, P.bad + t * (dev20.conv - P.bad), f"N=20 restore t={t:g}", restore=True)
               for t in (1.0, 2.0, 4.0, 1.5)}
    for t in (1.0, 2.0, 4.0):
        r = res[t][0]
        assert np.isinf(r.phi0).all() and (r.alpha == 1.0 / t).all(), _hist(r.alpha)
    r = res[1.5][0]
    assert (r.alpha == 0.5).sum() >= 7 and (r.alpha == 0.0).sum() >= 37 - 2, _hist(r.alpha)
    np.testing.assert_array_equal(r.u[r.alpha == 0], P.bad[r.alpha == 0])


@gpu
def test_restore_n50(P50):
    """The same at N = 50 with the NLP optimum as target: 18 problems restore (1, 1/2, 1/4 for
    t = 1, 2, 4), 14 have no step -- their target is outside the domain too."""
    P = P50
    with _ctx(_cfg(50), P.obs, P.B, 50) as c:
        res = {t: _check_ss(c, P, P.bad, P.bad + t * (P.target - P.bad), f"N=50 restore t={t:g}", restore=True)
               for t in (1.0, 2.0, 4.0)}
    for t in (1.0, 2.0, 4.0):
        r = res[t][0]
        assert np.isinf(r.phi0).all()
        assert (r.alpha == 1.0 / t).sum() >= 18 and (r.alpha == 0).sum() >= 14 - 2, _hist(r.alpha)


@gpu
def test_noise_step(P20, dev20):
    """Near a KKT point: dz = 1e-9 (qp_solution - iterate) at the converged iterate, and dz = 0
    exactly.  Every answer self-consistent; dz = 0 is the noise rule's full step (alpha = 1, the
    iterate unchanged).  alpha parity outside near-ties only -- few problems here, by construction:
    the count is printed, not capped."""
    P = P20
    with _ctx(_cfg(20), P.obs, P.B, 20) as c:
        r, ref, _, tie, nz = _check_ss(c, P, dev20.conv, dev20.conv + 1e-9 * (dev20.qp - dev20.conv),
                                       "N=20 noise 1e-9", cap=None)
        r0, ref0, _, tie0, nz0 = _check_ss(c, P, dev20.conv, dev20.conv.copy(), "N=20 dz = 0", cap=None)
    print(f"noise: 1e-9 dz: {int((~tie).sum())} of {P.B} compared for alpha, noise steps {nz}, oracle noise-level "
          f"|D| on {int((np.abs(ref[3]) <= KS.NOISE_D * np.maximum(1, np.abs(ref[1]))).sum())}; dz = 0: noise steps {nz0}")
    assert (r0.alpha == 1.0).all() and (r0.D == 0.0).all() and nz0 == P.B
    np.testing.assert_array_equal(r0.u, dev20.conv)
    np.testing.assert_array_equal(r0.phia, r0.phi0)
    assert nz + int((r.alpha == 0).sum()) >= 1


# -- multiple shooting --------------------------------------------------------------------------
def _ms_case(P, dev20):
    xw = Q.kin_predict(P.x0, 0.5 * (P.ubar + dev20.six), P.kap, P.ds, L)
    # a "QP solution" in the states that is not the rollout of the inputs' (defects at every step
    # size): the rollout of the mean of the target and the converged solution
    return xw, Q.kin_predict(P.x0, 0.5 * (P.target + dev20.six), P.kap, P.ds, L)


def _expect_x(P, r, reset, xp, xq):
    """The state iterate out: the rollout where reset, else x_prev + alpha (x - x_prev) with
    x_0 = x0 and the s column as it came in with the QP's x -- or, where the step was refused
    (a failed QP's x may be NaN, its s column included), s0 + sum ds summed in stage order."""
    al = r.alpha[:, None, None]
    xe = np.where(al > 0, xp + al * (xq - xp), xp)
    xe[:, 0] = P.x0
    xe[:, 1:, IS] = np.where(r.alpha[:, None] > 0, xq[:, 1:, IS], _s_column(P))
    return xe


def _s_column(P):
    """s0 + ds_0 + ds_1 + ... added in this order (csrc/kin_ric.hip, kin_merit.hip): [B, N]."""
    return np.cumsum(np.concatenate([P.x0[:, IS:IS + 1], P.ds], axis=1), axis=1)[:, 1:]


def _check_ms(c, P, up, uq, xp, xq, name, status=None):
    ok = None if status is None else np.asarray(status) == 0
    dz, dx = uq - up, xq - xp
    ref = KS.line_search_ms(P.x0, up, dz, xp, dx, P.kap, P.ds, L, P.W, qp_ok=ok)
    gap = KS.line_search_ms.reset_gap
    pm0 = KS.merit(P.x0, up, P.kap, P.ds, L, P.W, x=xp)
    ps0 = KS.merit(P.x0, up, P.kap, P.ds, L, P.W)
    roll = np.isfinite(ps0) & (ps0 <= pm0 + KS.TIE * np.abs(pm0))
    cand = np.where(roll[None, :], _candidates(P, up, dz), _candidates(P, up, dz, xp, dx))
    tie = _near_tie(ref[0], ref[1], ref[3], cand)
    r = _launch(c, P, up, uq, status=status, xp=xp, xq=xq)
    xr = c.rollout(P.x0, r.u, P.kap, P.ds)
    with np.errstate(invalid="ignore"):
        rtie = np.abs(gap) < 1e-6
    reset = ref[4]
    print(f"{name}: alpha {_hist(r.alpha)} (oracle {_hist(ref[0])}); state-iterate mode {int((~roll).sum())}; "
          f"reset {int(reset.sum())} of {P.B}, reset near-ties {np.nonzero(rtie)[0].tolist()}; alpha near-ties "
          f"{np.nonzero(tie)[0].tolist()}; phi0 err {_rel(r.phi0, ref[1]).max():.2e}")
    assert tie.sum() <= 2
    np.testing.assert_array_equal(r.alpha[~tie], ref[0][~tie])
    assert _rel(r.phi0, ref[1]).max() <= BAR and _rel(r.phia, ref[2])[~tie].max() <= BAR
    fin = np.isfinite(ref[1]) & np.isfinite(ref[3])
    with np.errstate(invalid="ignore"):
        eD = np.abs(r.D - ref[3])
    assert (eD[fin] <= 2 * BAR * np.maximum(1.0, np.abs(ref[1][fin])) / EPS_FD).all()
    assert not np.isfinite(r.D[~fin]).any()
    exp = np.where((r.alpha > 0)[:, None, None], up + r.alpha[:, None, None] * dz, up)
    np.testing.assert_array_equal(r.u, exp)
    np.testing.assert_array_equal(r.u0, r.u[:, 0])
    xe = _expect_x(P, r, reset, xp, xq)
    is_roll = np.abs(r.x - xr).max(axis=(1, 2)) <= 1e-12 * (1.0 + np.abs(xr).max())
    is_iter = (r.x == xe).all(axis=(1, 2))
    sure = ~rtie & ~tie
    assert (is_roll | is_iter).all()
    assert is_roll[sure & reset].all() and is_iter[sure & ~reset].all(), np.nonzero(sure & (is_roll != reset))[0]
    # self-consistency: phi(accepted) is the governing merit of what the kernel took
    al = r.alpha[:, None, None]
    xa = np.where(al > 0, xp + al * dx, xp)
    phi_ret = np.where(roll, KS.merit(P.x0, r.u, P.kap, P.ds, L, P.W), KS.merit(P.x0, r.u, P.kap, P.ds, L, P.W, x=xa))
    _self_consistent(r, phi_ret)
    return r, ref, roll


@gpu
def test_line_search_multiple_shooting(P20, dev20):
    """line_search_ms on the 15-of-44 split of test_kin_sqp_multiple_shooting_vs_oracle, t in
    {1, 8, -1}: alpha exact, reset exact outside |reset_gap| < 1e-6, and the state iterate out."""
    P = P20
    xw, xt = _ms_case(P, dev20)
    nreset, nkeep = 0, 0
    with _ctx(_cfg(20, ms=1), P.obs, P.B, 20) as c:
        for t in (1.0, 8.0, -1.0):
            uq = P.ubar + t * (P.target - P.ubar)
            xq = xw + t * (xt - xw)
            r, ref, roll = _check_ms(c, P, P.ubar, uq, xw, xq, f"ms t={t:g}")
            assert (~roll).sum() >= 10
            nreset += int(ref[4].sum())
            nkeep += int((~ref[4]).sum())
            if t == -1.0:
                assert (r.alpha[roll] == 0).all()
    assert nreset >= 3 and nkeep >= 3, (nreset, nkeep)


# -- refused steps ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ms", [0, 1], ids=["single_shooting", "multiple_shooting"])
def test_refused_steps(P20, dev20, ms):
    """status != 0 on three problems (one with NaN u / x, two with a finite u): alpha = 0, the
    iterate bit-identical to u_prev, nothing non-finite in the outputs, u0 = u_prev[:, 0]; under
    multiple shooting the reset decision is the one of alpha = 0 (the rollout of u_prev against the
    state iterate), whatever step size the finite output would have earned."""
    P = P20
    from vcmpc import _abi
    xw, xt = _ms_case(P, dev20)
    st = np.zeros(P.B, np.int32)
    # refused: two problems whose state-iterate merit governs at alpha = 0 (no reset there; the first
    # gets the NaN output), and one whose reset answer at the step size its finite output would
    # have earned is the opposite of the one at alpha = 0 -- the case that tells the two rules apart
    pm0 = KS.merit(P.x0, P.ubar, P.kap, P.ds, L, P.W, x=xw)
    ps0 = KS.merit(P.x0, P.ubar, P.kap, P.ds, L, P.W)
    reset0 = np.isfinite(ps0) & (ps0 <= pm0 + KS.TIE * np.abs(pm0))
    free = KS.line_search_ms(P.x0, P.ubar, P.target - P.ubar, xw, xt - xw, P.kap, P.ds, L, P.W)
    flip = np.nonzero((free[4] != reset0) & (free[0] > 0) & (np.abs(KS.line_search_ms.reset_gap) > 1e-6)
                      & (np.abs(ps0 - pm0) > 1e-6 * np.abs(pm0)))[0]
    assert len(flip) >= 1
    keep = [b for b in np.nonzero(ps0 > pm0 * (1 + 1e-6))[0] if b != flip[0]]
    bad = [int(keep[0]), int(flip[0]), int(keep[1])]
    st[bad] = [_abi.VC_NONFINITE, _abi.VC_MAX_ITER, _abi.VC_INFEASIBLE]
    uq, xq = P.target.copy(), xt.copy()
    uq[bad[0]], xq[bad[0]] = np.nan, np.nan
    with _ctx(_cfg(20, ms=ms), P.obs, P.B, 20) as c:
        if ms:
            r, ref, _ = _check_ms(c, P, P.ubar, uq, xw, xq, "refused ms", status=st)
            np.testing.assert_array_equal(ref[4][bad], reset0[bad])
            xr = Q.kin_predict(P.x0, P.ubar, P.kap, P.ds, L)
            for b in bad:
                if reset0[b]:
                    assert np.abs(r.x[b] - xr[b]).max() < 1e-9
                else:       # the state iterate as it was, s = s0 + sum ds
                    cols = [i for i in range(6) if i != IS]
                    np.testing.assert_array_equal(r.x[b][1:, cols], xw[b][1:, cols])
                    np.testing.assert_array_equal(r.x[b][1:, IS], _s_column(P)[b])
            print(f"refused ms: problems {bad}, reset of alpha = 0 {reset0[bad].tolist()}; the finite output would "
                  f"have earned alpha {free[0][bad].tolist()} and reset {free[4][bad].tolist()}")
            assert reset0[bad].any() and not reset0[bad].all()
        else:
            r = _launch(c, P, P.ubar, uq, status=st)
            ref = KS.line_search(P.x0, P.ubar, P.target - P.ubar, P.kap, P.ds, L, P.W, qp_ok=st == 0)
            np.testing.assert_array_equal(r.alpha, ref[0])
            print(f"refused: problems {bad}: alpha {r.alpha[bad].tolist()}; the others {_hist(np.delete(r.alpha, bad))}")
    assert (r.alpha[bad] == 0).all()
    np.testing.assert_array_equal(r.u[bad], P.ubar[bad])
    np.testing.assert_array_equal(r.u0[bad], P.ubar[bad][:, 0])
    np.testing.assert_array_equal(r.phia[bad], r.phi0[bad])
    # D of the problem whose QP output is NaN is the derivative along a NaN direction: not finite
    # (the oracle's alike), in the diagnostics only; everything the step hands on is finite
    for a in (r.u, r.x, r.u0, r.phi0, r.phia, r.alpha, np.delete(r.D, bad[0])):
        assert np.isfinite(a).all()
    assert not np.isfinite(r.D[bad[0]])
    np.testing.assert_array_equal(r.status, st)     # first = 1: the step's status is the QP's


# -- status and iteration bookkeeping -----------------------------------------------------------
@gpu
@pytest.mark.parametrize("ms", [0, 1], ids=["single_shooting", "multiple_shooting"])
def test_status_bookkeeping(P20, dev20, ms):
    """Two launches in sequence on B = 9 with st_acc / it_acc carried over.  restart = 1: a failed
    first QP gives st_acc = RESTART_PENDING (-1), u = 0 and (ms) the state iterate x0 at every stage;
    the next launch's QP status is then the step's and iters the sum of both.  restart = 0 keeps the
    first status and the iterate.  A later failure after a solved first QP keeps status 0."""
    P = _sub(P20, np.arange(9))
    xw, xt = (a[:9] for a in _ms_case(P20, dev20))
    s1 = np.array([0, 0, 1, 2, 4, 0, 3, 0, 1], np.int32)
    s2 = np.array([0, 2, 0, 4, 0, 1, 3, 0, 0], np.int32)
    i1 = np.arange(5, 14, dtype=np.int32)
    i2 = np.arange(20, 29, dtype=np.int32)
    f1 = s1 != 0
    kw1 = dict(xp=xw, xq=xt) if ms else {}
    with _ctx(_cfg(20, ms=ms), P.obs, 9, 20) as c:
        for restart in (True, False):
            a = _launch(c, P, P.ubar, P.target, status=s1, iters=i1, first=True, restart=restart, **kw1)
            np.testing.assert_array_equal(a.status, s1)
            np.testing.assert_array_equal(a.iters, i1)
            np.testing.assert_array_equal(a.it_acc, i1)
            np.testing.assert_array_equal(a.st_acc, np.where(f1, -1, s1) if restart else s1)
            assert (a.alpha[f1] == 0).all() and (a.alpha[~f1] > 0).all()
            if restart:
                assert (a.u[f1] == 0).all()
                if ms:
                    np.testing.assert_array_equal(a.x[f1], np.repeat(P.x0[f1][:, None, :], 21, axis=1))
            else:
                np.testing.assert_array_equal(a.u[f1], P.ubar[f1])
            assert np.isfinite(a.u).all() and np.isfinite(a.x).all()
            kw2 = dict(xp=a.x, xq=xt) if ms else {}
            b = _launch(c, P, a.u, P.target, status=s2, iters=i2, st_acc=a.st_acc, it_acc=a.it_acc, first=False,
                        restart=restart, **kw2)
            exp = np.where(f1, s2, 0) if restart else s1
            np.testing.assert_array_equal(b.status, exp)
            np.testing.assert_array_equal(b.st_acc, exp)
            np.testing.assert_array_equal(b.iters, i1 + i2)
            np.testing.assert_array_equal(b.it_acc, i1 + i2)
            assert (b.alpha[s2 != 0] == 0).all()
            np.testing.assert_array_equal(b.u[s2 != 0], a.u[s2 != 0])
            later = ~f1 & (s2 != 0)          # solved first QP, failed later one: the step stays solved
            assert later.sum() >= 2 and (b.status[later] == 0).all()
            print(f"bookkeeping ms={ms} restart={int(restart)}: first failed {int(f1.sum())} of 9 (restarted "
                  f"{int(f1.sum()) if restart else 0}), status after two launches {b.status.tolist()}, iters {b.iters.tolist()}")


# -- restart end to end -------------------------------------------------------------------------
RESTART_B = 7


@gpu
@pytest.mark.parametrize("ms", [0, 1], ids=["single_shooting", "multiple_shooting"])
def test_restart_end_to_end(P20, ms):
    """vc_solve with kin_sqp = 3 and problem b's first QP failed (vc_debug_qp_fault at SQP iteration
    0): b restarts from the neutral guess, so its u*, x*, u0 and status are bit for bit those of a
    kin_sqp = 2 solve of b from ubar = 0 (xbar = x0 tiled), its iters that run's plus the first
    QP's; every other problem is bit-identical to the run without the fault."""
    P = P20
    b = RESTART_B
    xw = Q.kin_predict(P.x0, P.ubar, P.kap, P.ds, L)
    run = lambda c, sl=slice(None), ub=P.ubar, xb=xw: c.solve(
        P.x0[sl], P.kap[sl], P.ds[sl], np.ascontiguousarray(ub[sl]).copy(), xbar=np.ascontiguousarray(xb[sl]).copy())
    with _ctx(_cfg(20, ms=ms, kin_sqp=3), P.obs, P.B, 20) as c:
        clean = run(c)
        c._check(c.lib.vc_debug_qp_fault(c._h, 0, b))
        hit = run(c)
    with _ctx(_cfg(20, ms=ms, kin_sqp=1), P.obs, P.B, 20) as c:
        it_first = run(c)[4]
    one = slice(b, b + 1)
    with _ctx(_cfg(20, ms=ms, kin_sqp=2), P.obs, P.B, 20) as c:
        neutral = run(c, one, np.zeros_like(P.ubar), np.repeat(P.x0[:, None, :], 21, axis=1))
    print(f"restart end to end ms={ms}: problem {b}: status {int(hit[3][b])} (neutral run {int(neutral[3][0])}), iters "
          f"{int(hit[4][b])} = {int(neutral[4][0])} + {int(it_first[b])}; |u* - clean u*| {np.abs(hit[2][b] - clean[2][b]).max():.2e}")
    assert neutral[3][0] == 0
    for k in (0, 1, 2, 3):      # u0, x*, u*, status
        np.testing.assert_array_equal(hit[k][b], neutral[k][0])
    assert hit[4][b] == neutral[4][0] + it_first[b]
    others = np.arange(P.B) != b
    for k in range(5):
        np.testing.assert_array_equal(hit[k][others], clean[k][others])
    assert not np.array_equal(hit[2][b], clean[2][b])       # the restart was taken


# -- natural restarts ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ms", [0, 1], ids=["single_shooting", "multiple_shooting"])
def test_natural_restarts_vs_oracle(P20, ms):
    """The tightened-delta-box problems of test_kin_sqp_elastic_on_failure_vs_oracle with hard rows
    only (elastic = 0) and kin_sqp = 2: at least half the first QPs fail and restart; the kernel's
    solved / non-solved split is the oracle's qp_ok of the deciding QP (the second where the first
    failed) and u* matches to 1e-5 where solved.  Multiple shooting gets the obstacle list, so the
    restarted state iterate's s column matters to a merit that would read it."""
    from vcmpc.workload import kinematic_batch
    cfg = _cfg(20, ms=ms, kin_sqp=2, trust_a=1.0, trust_w=0.1, elastic=0.0, max_iter=80)
    cfg["state_constraints"] = dict(cfg["state_constraints"], delta_max=0.05, delta_min=-0.05)
    obs = P20.obs if ms else []
    W = Q.kin_weights(cfg)
    W["obstacles"] = obs
    d = kinematic_batch(32, N=20, seed=91)
    xw = Q.kin_predict(d["x0"], d["ubar"], d["kappa"], d["ds"], L) if ms else None
    ref = KS.kin_sqp_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], L, W, 2, x_ws=xw)
    with _ctx(cfg, obs, 32, 20) as c:
        u0, xs, us, st, it = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(),
                                     xbar=None if xw is None else xw.copy())
    ok0, ok1 = ref["hist"][0]["qp_ok"], ref["hist"][1]["qp_ok"]
    deciding = np.where(ok0, ok0, ok1)
    solved = st == 0
    err = np.abs(us - ref["u_star"]).max(axis=(1, 2))
    print(f"natural restarts ms={ms}: oracle first QP failed {int((~ok0).sum())} of 32, deciding QP solved "
          f"{int(deciding.sum())}; device solved {int(solved.sum())}; oracle alphas after restart "
          f"{_hist(ref['hist'][1]['alpha'][~ok0])}; |u* - u*_oracle| max where solved {err[solved].max():.2e}")
    assert (~ok0).sum() >= 16
    np.testing.assert_array_equal(solved, deciding)
    assert np.isfinite(us).all() and np.isfinite(xs).all()
    assert err[solved].max() < U_TOL, np.nonzero(solved & (err >= U_TOL))[0]


# -- batch independence, pointer modes ----------------------------------------------------------
@gpu
def test_batch_independence(P20):
    """The t = 8 row at B = 1, 7 and 44: the same bits for the same problems (44 = 5 * 8 + 4 puts
    four problems on the identity tail of the kernel's problem-to-workgroup map, 7 is all tail)."""
    P = P20
    outs = {}
    with _ctx(_cfg(20), P.obs, P.B, 20) as c:
        for B in (44, 7, 1):
            S = _sub(P, np.arange(B))
            r = _launch(c, S, S.ubar, S.ubar + 8.0 * (S.target - S.ubar))
            outs[B] = [r.alpha, r.phi0, r.phia, r.D, r.u, r.x, r.u0]
    for B in (7, 1):
        for a, full in zip(outs[B], outs[44]):
            np.testing.assert_array_equal(a, full[:B])


@gpu
@pytest.mark.parametrize("ms", [0, 1], ids=["single_shooting", "multiple_shooting"])
def test_pointer_modes(P20, dev20, ms):
    """Host arrays (staged through the arena) and device tensors give the same bits at B = 9."""
    import torch
    P = _sub(P20, np.arange(9))
    xw, xt = (np.ascontiguousarray(a[:9]) for a in _ms_case(P20, dev20))
    st = np.array([0, 0, 2, 0, 0, 0, 0, 0, 1], np.int32)
    it = np.arange(9, dtype=np.int32)
    uq = P.ubar + 8.0 * (P.target - P.ubar)
    kw = dict(xp=xw, xq=xt) if ms else {}
    with torch.cuda.stream(torch.cuda.Stream()):
        with _ctx(_cfg(20, ms=ms), P.obs, 9, 20) as c:
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            h = _launch(c, P, P.ubar, uq, status=st, iters=it, first=True, restart=True, **kw)
            dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            bufs = dict(u=dv(uq), status=dv(st), iters=dv(it), st_acc=dv(np.zeros(9, np.int32)),
                        it_acc=dv(np.zeros(9, np.int32)))
            xk = dict(x_prev=dv(xw), x=dv(xt)) if ms else {}
            u0, x, u, s, i, d = c.debug_kin_merit(dv(P.x0), dv(P.kap), dv(P.ds), dv(P.ubar), bufs["u"], bufs["status"],
                                                  bufs["iters"], bufs["st_acc"], bufs["it_acc"], first=True,
                                                  restart=True, **xk)
            torch.cuda.current_stream().synchronize()
            got = [t.cpu().numpy() for t in (u0, x, u, s, i, d, bufs["st_acc"], bufs["it_acc"])]
        torch.cuda.synchronize()
    want = [h.u0, h.x, h.u, h.status, h.iters, np.stack([h.alpha, h.phi0, h.phia, h.D], axis=1), h.st_acc, h.it_acc]
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert (h.st_acc[[2, 8]] == -1).all() and (h.u[[2, 8]] == 0).all()


@gpu
def test_hook_is_kinematic_fp64_only():
    """Every other context answers VC_E_UNSUPPORTED."""
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("dynamic_mpc"))
    z = np.zeros(8)
    i = np.zeros(1, np.int32)
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=20, max_batch=1, dtype=_abi.VC_F64, params=p) as c:
        v = lambda a: a.ctypes.data
        code = c.lib.vc_debug_kin_merit(c._h, 1, v(z), v(z), v(z), v(z), v(z), None, v(z), v(i), v(i), v(i), v(i), 1, 0,
                                        v(z), v(z), _abi.VC_HOST_PTRS)
    assert code == _abi.VC_E_UNSUPPORTED
