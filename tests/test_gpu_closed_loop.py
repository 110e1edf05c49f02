"""GPU: curvature table, horizon parameters, plant and the batched closed loop
(vc_track_k / vc_horizon / vc_drive / vc_simulate) against
the oracle.

Checks, per layer:
* k(s) on the device == the package's host evaluation of the same table (fp64,
  1e-13) and the scipy restatement (oracle/track.py, 1e-9), and reproduces the
  curvature the reference's plant used in its recorded runs (2e-9);
* horizon parameters: ds bit-exact, kappa to the table tolerance (kinematic fp64;
  dynamic fp32 within one fp32 ulp);
* plant: x+ == the oracle's fp64 transition with k(s) (1e-12 relative);
* closed loop: every logged step satisfies the plant relation, a sample of the
  per-step solves matches the oracle SQP / LTV-QP on the exact inputs the kernel
  saw, K steps in one call == K one-step calls bit for bit, host == device pointers.
"""
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import dyn_sqp as D
from oracle import ltv_qp as Q
from oracle import models as M
from oracle import track as OT

pytestmark = pytest.mark.gpu

TRACK_DIR = os.path.join(ROOT, "vehicle-control_amd", "config", "tracks")
DT = 0.05
MPC_DT = 0.03
SCALE = np.array([1000.0, 1.0])
U_TOL_FIALA = 5e-4     # tests/test_gpu_dyn_sqp.py (scaled u*, Fiala tyre)
U_TOL_KIN = 1e-5       # north star bar, kinematic fp64
# closed-loop runs use the reference's 1.8 s preview (singletrack.yaml: 60 x 0.03 s) at
# BASELINE's N = 40, i.e. mpc_dt = 0.045; at 40 x 0.03 s the contract (oracle included)
# brakes too late for ippodromo's 21 m corners from 18 m/s
C5_MPC_DT = 0.045


@pytest.fixture(scope="module")
def tracks():
    from vcmpc.environment import Track
    return Track.load("ippodromo"), OT.load_track(os.path.join(TRACK_DIR, "ippodromo.yaml"))


def _dyn_ctx(track, tyre="fiala", B=256, N=40, f64=False):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("dynamic_mpc"), tyre=tyre)
    c = Context(model=_abi.VC_MODEL_DYNAMIC, N=N, max_batch=B, dtype=_abi.VC_F64 if f64 else _abi.VC_F32, params=p)
    c.set_track(track)
    return c


def _kin_ctx(track, B=256, N=20):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(kin_car=load_config("kinematic_car"), kin_mpc=load_config("kinematic_mpc"))
    c = Context(model=_abi.VC_MODEL_KINEMATIC, N=N, max_batch=B, dtype=_abi.VC_F64, params=p)
    c.set_track(track)
    return c


def _dyn_states(B, L, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 8))
    x[:, 0] = rng.uniform(8, 14, B)
    x[:, 1] = rng.uniform(-0.1, 0.1, B)
    x[:, 2] = rng.uniform(-0.05, 0.2, B)
    x[:, 3] = rng.uniform(-0.03, 0.1, B)
    x[:, 4] = rng.uniform(0, L, B)
    x[:, 5] = rng.uniform(-1.5, 1.5, B)
    x[:, 6] = rng.uniform(-0.1, 0.1, B)
    return x


def _kin_states(B, L, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 6))
    x[:, 0] = rng.uniform(4, 9, B)
    x[:, 1] = rng.uniform(-0.05, 0.1, B)
    x[:, 2] = rng.uniform(0, L, B)
    x[:, 3] = rng.uniform(-1.5, 1.5, B)
    x[:, 4] = rng.uniform(-0.1, 0.1, B)
    return x


def _dyn_p():
    from vcmpc.config import load_config
    return M.dyn_params_from_config(load_config("dynamic_car"))


# -- curvature table ---------------------------------------------------------------------
def test_track_k_device(tracks, dyn_kat):
    pt, ot = tracks
    L = pt.length
    h = 0.05
    edges = np.array([0.0, h, 2 * h, 1000 * h, L - 0.1, L - 0.05, L - 1e-9, L, L + 1e-9, 2 * L - 1e-6, 3.5 * L])
    s = np.concatenate([edges, np.random.default_rng(0).uniform(0, 2 * L, 4000), dyn_kat["x"][:431, 4]])
    with _kin_ctx(pt, B=len(s)) as c:
        k = c.track_k(s)
    assert np.abs(k - pt.k(s)).max() < 1e-13
    assert np.abs(k - ot.k_periodic(s)).max() < 1e-9
    # the reference's plant curvature over its recorded ippodromo run (KAT)
    assert np.abs(k[len(edges) + 4000:] - dyn_kat["kappa"][:431]).max() < 2e-9
    s32 = s.astype(np.float32)
    with _dyn_ctx(pt, B=len(s)) as c:
        k32 = c.track_k(s32)
    ref = pt.k(s32.astype(np.float64)).astype(np.float32)
    assert np.abs(k32.view(np.int32) - ref.view(np.int32)).max() <= 1


def test_track_set_rejects_bad_tables(tracks):
    from vcmpc import _abi
    pt, _ = tracks
    with _kin_ctx(pt, B=4) as c:
        bad = np.full((4, 4), np.nan)
        rc = c.lib.vc_track_set(c._h, 4, 0.05, 1.0, bad.ctypes.data)
        assert rc == _abi.VC_E_ARG and b"not finite" in c.lib.vc_last_error(c._h)
        assert c.lib.vc_track_set(c._h, 0, 0.05, 1.0, bad.ctypes.data) == _abi.VC_E_ARG
        # the previous table is untouched by a rejected call
        np.testing.assert_allclose(c.track_k(np.array([10.0])), pt.k(np.array([10.0])), atol=1e-13)


# -- horizon parameters ----------------------------------------------------------------------
def test_horizon_kinematic_fp64(tracks):
    pt, ot = tracks
    B, N = 128, 20
    rng = np.random.default_rng(5)
    x0 = _kin_states(B, pt.length, 5)
    x0[:4, 2] = pt.length - rng.uniform(0, 2, 4)        # horizons that run over the lap end
    xbar = np.zeros((B, N + 1, 6))
    xbar[..., 0] = rng.uniform(2, 12, (B, N + 1))
    with _kin_ctx(pt, B=B) as c:
        kap, ds = c.horizon(x0, xbar, MPC_DT)
    for b in range(B):
        ds_r, k_r = Q.kin_horizon_params(x0[b], xbar[b].T, MPC_DT, N, pt.k)
        np.testing.assert_array_equal(ds[b], ds_r)
        assert np.abs(kap[b] - k_r).max() < 1e-13
        _, k_o = Q.kin_horizon_params(x0[b], xbar[b].T, MPC_DT, N, ot.k_periodic)
        assert np.abs(kap[b] - k_o).max() < 1e-9


def test_horizon_dynamic_fp32(tracks):
    pt, _ = tracks
    B, N = 128, 40
    rng = np.random.default_rng(6)
    x0 = _dyn_states(B, pt.length, 6).astype(np.float32)
    xbar = np.ones((B, N, 8), np.float32)
    xbar[..., 0] = rng.uniform(3, 20, (B, N))
    with _dyn_ctx(pt, B=B) as c:
        kap, ds = c.horizon(x0, xbar, MPC_DT)
    for b in range(B):
        ds_r, k_r = D.dyn_horizon_params(x0[b].astype(np.float64), xbar[b].T.astype(np.float64), MPC_DT, N, pt.k)
        np.testing.assert_array_equal(ds[b], ds_r.astype(np.float32))
        d = np.abs(kap[b].view(np.int32) - k_r.astype(np.float32).view(np.int32))
        assert d.max() <= 1


def test_horizon_dynamic_fp64(tracks):
    """horizon_kernel<double, double, DYNAMIC>: ds bit-exact, kappa to the table tolerance (the
    bars of test_horizon_kinematic_fp64), four starts whose horizon runs over the lap end.
    Measured on an MI355X: max |kappa - kappa_oracle| = 0."""
    pt, _ = tracks
    B, N = 128, 20
    rng = np.random.default_rng(16)
    x0 = _dyn_states(B, pt.length, 16)
    x0[:4, 4] = pt.length - rng.uniform(0, 2, 4)
    xbar = np.ones((B, N, 8))
    xbar[..., 0] = rng.uniform(3, 20, (B, N))
    with _dyn_ctx(pt, B=B, N=N, f64=True) as c:
        kap, ds = c.horizon(x0, xbar, MPC_DT)
    worst = 0.0
    for b in range(B):
        ds_r, k_r = D.dyn_horizon_params(x0[b], xbar[b].T, MPC_DT, N, pt.k)
        np.testing.assert_array_equal(ds[b], ds_r)
        worst = max(worst, np.abs(kap[b] - k_r).max())
    print(f"dynamic fp64 horizon: max |kappa - kappa_oracle| = {worst:.2e}")
    assert worst < 1e-13
    assert (x0[:4, 4] + ds[:4].sum(1) - ds[:4, -1] > pt.length).all()   # they do cross the lap end


@pytest.mark.parametrize("Mh", [15, 40])
def test_horizon_cascaded_fp64(tracks, Mh):
    """horizon_kernel<double, double, CASCADED>: the single-track stages as above, then the
    point-mass tail ds = ds_pm, s = cumsum(ds_pm) - ds[N-1] + s_traj[N-1] (cascaded_mpc.py:332-338)
    against oracle/casc_sqp.py casc_horizon_params.  Four starts within 2 m of the lap end, so
    that the tail's s wraps.  Measured on an MI355X: max |kappa - kappa_oracle| = 0, both tails."""
    from oracle import casc_sqp as CS
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    pt, _ = tracks
    B, N = 64, 20
    cfg = load_config("cascaded_mpc")
    cfg["horizon_pm"] = Mh
    ds_pm = float(cfg["ds_pm"])
    rng = np.random.default_rng(17 + Mh)
    x0 = _dyn_states(B, pt.length, 17 + Mh)
    x0[:4, 4] = pt.length - rng.uniform(0, 2, 4)
    xbar = np.ones((B, N + Mh, 8))
    xbar[:, :N, 0] = rng.uniform(3, 20, (B, N))
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=cfg, tyre="fiala")
    with Context(model=_abi.VC_MODEL_CASCADED, N=N, max_batch=B, dtype=_abi.VC_F64, params=p) as c:
        c.set_track(pt)
        kap, ds = c.horizon(x0, xbar, MPC_DT)
    assert kap.shape == ds.shape == (B, N + Mh)
    worst = 0.0
    for b in range(B):
        ds_r, k_r = CS.casc_horizon_params(x0[b], xbar[b].T, MPC_DT, N, Mh, ds_pm, pt.k)
        np.testing.assert_array_equal(ds[b], ds_r)
        worst = max(worst, np.abs(kap[b] - k_r).max())
    print(f"cascaded fp64 horizon M={Mh}: max |kappa - kappa_oracle| = {worst:.2e}")
    assert worst < 1e-13


# -- plant --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tyre", ["fiala", "linear"])
def test_drive_dynamic_fp64_plant(tracks, tyre):
    pt, _ = tracks
    B = 512
    x = _dyn_states(B, pt.length, 7)
    u = np.stack([np.random.default_rng(7).uniform(-5000, 3000, B), np.random.default_rng(8).uniform(-.4, .4, B)], 1)
    ref = M.dyn_transition(x, u, pt.k(x[:, 4]), DT, _dyn_p(), tyre)
    with _dyn_ctx(pt, tyre=tyre, B=B) as c:
        x64 = x.copy()
        xc = np.empty((B, 8), np.float32)
        c.drive(x64, u.astype(np.float32), DT, x_ctx=xc)
    ref32 = M.dyn_transition(x, u.astype(np.float32).astype(np.float64), pt.k(x[:, 4]), DT, _dyn_p(), tyre)
    rel = np.abs(x64 - ref32) / np.maximum(np.abs(ref32), 1e-9)
    assert rel.max() < 1e-12
    np.testing.assert_array_equal(xc, x64.astype(np.float32))
    assert np.abs(ref - ref32).max() > 0   # u really went through fp32


def test_drive_reproduces_reference_runs(tracks, dyn_kat):
    """Plant + track table together reproduce the reference's recorded ippodromo run
    (racing_car.py:34-46): x[n+1] from x[n], u[n+1] with k(s_n) from the table."""
    pt, _ = tracks
    m = np.array(["ippodromo" in r for r in dyn_kat["run"]])
    x, u, xn = dyn_kat["x"][m], dyn_kat["u"][m], dyn_kat["x_next"][m]
    B = len(x)
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("dynamic_mpc"), tyre="fiala")
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=40, max_batch=B, dtype=_abi.VC_F64, params=p) as c:
        c.set_track(pt)
        x64 = np.ascontiguousarray(x)
        c.drive(x64, np.ascontiguousarray(u), DT)
    err = np.abs(x64 - xn)
    assert err[:, :4].max() < 1e-11 * max(1.0, np.abs(xn[:, :4]).max())   # kappa-independent block
    assert err.max() < 1e-8                                               # table vs CasADi bspline


def test_drive_kinematic(tracks):
    pt, _ = tracks
    B = 256
    x = _kin_states(B, pt.length, 9)
    u = np.stack([np.random.default_rng(1).uniform(-3, 3, B), np.random.default_rng(2).uniform(-.4, .4, B)], 1)
    with _kin_ctx(pt, B=B) as c:
        x64 = x.copy()
        c.drive(x64, u, DT)
    ref = M.kin_transition(x, u, pt.k(x[:, 2]), DT, 2.5)
    assert (np.abs(x64 - ref) / np.maximum(np.abs(ref), 1e-9)).max() < 1e-13


# -- closed loop --------------------------------------------------------------------------------
def _warm(B, N, ns, nx, dynamic, dtype):
    xbar = np.ones((B, ns, nx)) if dynamic else np.zeros((B, ns, nx))
    xbar[..., 0] += 3 if dynamic else 0.1
    ubar = np.zeros((B, N, 2))
    return xbar.astype(dtype), ubar.astype(dtype)


def _check_plant_log(log_x, log_u, pt, step_fn):
    for k in range(log_u.shape[0]):
        xk = log_x[k]
        ref = step_fn(xk, log_u[k].astype(np.float64), pt.k(xk[:, IS_OF[xk.shape[1]]]))
        rel = np.abs(log_x[k + 1] - ref) / np.maximum(np.abs(ref), 1e-9)
        assert rel.max() < 1e-12, (k, rel.max())


IS_OF = {8: 4, 6: 2}


@pytest.mark.parametrize("f64", [False, True], ids=["fp32", "fp64"])
def test_simulate_dynamic_matches_stepwise_oracle(tracks, f64):
    """fp32 (dyn_sqp.hip) at the scaled fp32 bar; fp64 (st_sqp.hip) at the north star's
    1e-5 in the reference's units (Fx in N, w in rad/s)."""
    pt, _ = tracks
    from vcmpc.config import load_config
    B, N, K = 24, 40, 12
    p, W = _dyn_p(), D.dyn_weights(load_config("dynamic_mpc"))
    x0 = _dyn_states(B, pt.length, 11)
    ft = np.float64 if f64 else np.float32
    with _dyn_ctx(pt, B=B, f64=f64) as c:
        xbar, ubar = _warm(B, N, N, 8, True, ft)
        x64 = x0.copy()
        log_x, log_u, nfail = c.simulate(x64, xbar, ubar, K, MPC_DT, DT, log=True)
        # the same loop as K one-step calls, capturing each step's warm start
        xb1, ub1 = _warm(B, N, N, 8, True, ft)
        x1 = x0.copy()
        warm = []
        nf1 = np.zeros(B, np.int32)
        for k in range(K):
            warm.append((x1.copy(), xb1.copy(), ub1.copy()))
            c.simulate(x1, xb1, ub1, 1, MPC_DT, DT, nfail=nf1)
    np.testing.assert_array_equal(x1, x64)
    np.testing.assert_array_equal(xb1, xbar)
    np.testing.assert_array_equal(ub1, ubar)
    np.testing.assert_array_equal(nf1, nfail)
    np.testing.assert_array_equal(log_x[0], x0)
    np.testing.assert_array_equal(log_x[-1], x64)
    _check_plant_log(log_x, log_u, pt, lambda x, u, k: M.dyn_transition(x, u, k, DT, p, "fiala"))
    assert nfail.sum() <= 1
    # per-step solve parity on the exact fp32 inputs the kernel received
    ok = np.nonzero(nfail == 0)[0][:4]
    for k in (0, 5, K - 1):
        xk, xbk, ubk = warm[k]
        x0_32 = xk[ok].astype(ft)
        kap = np.empty((len(ok), N), ft)
        ds = np.empty((len(ok), N), ft)
        for i, b in enumerate(ok):
            d, kk = D.dyn_horizon_params(x0_32[i].astype(np.float64), xbk[b].T.astype(np.float64), MPC_DT, N, pt.k)
            ds[i], kap[i] = d.astype(ft), kk.astype(ft)
        f = lambda a: np.asarray(a, np.float64)
        ref = D.dyn_sqp_solve(f(x0_32), f(ubk[ok]), f(kap), f(ds), p, W, "fiala")
        if f64:  # kappa from the device table vs the host table: 1e-13 apart (test_track_k_device)
            err = np.abs(log_u[k][ok] - ref["u0"])
            assert err.max() < 1e-5, (k, err.max())
        else:
            err = np.abs(log_u[k][ok].astype(np.float64) - ref["u0"]) / SCALE
            assert err.max() < U_TOL_FIALA, (k, err.max())


def test_simulate_kinematic_matches_stepwise_oracle(tracks, kin_W):
    pt, _ = tracks
    B, N, K = 32, 20, 10
    x0 = _kin_states(B, pt.length, 12)
    with _kin_ctx(pt, B=B) as c:
        xbar, ubar = _warm(B, N, N + 1, 6, False, np.float64)
        x64 = x0.copy()
        xb0, ub0 = xbar.copy(), ubar.copy()
        log_x, log_u, nfail = c.simulate(x64, xbar, ubar, K, MPC_DT, DT, log=True)
        # step 0 and a later step, re-run one step at a time
        xs, xbs, ubs = x0.copy(), xb0.copy(), ub0.copy()
        captured = {}
        for k in range(K):
            if k in (0, 6):
                captured[k] = (xs.copy(), xbs.copy(), ubs.copy())
            c.simulate(xs, xbs, ubs, 1, MPC_DT, DT)
    np.testing.assert_array_equal(xs, x64)
    _check_plant_log(log_x, log_u, pt, lambda x, u, k: M.kin_transition(x, u, k, DT, 2.5))
    assert nfail.sum() <= 0.02 * B * K, nfail.sum()
    for k, (xk, xbk, ubk) in captured.items():
        for b in [b for b in range(0, B, 4) if nfail[b] == 0][:6]:
            ds, kap = Q.kin_horizon_params(xk[b], xbk[b].T, MPC_DT, N, pt.k)
            ref = Q.kin_ltv_solve(xk[b][None], ubk[b][None], kap[None], ds[None], 2.5, kin_W)
            assert np.abs(log_u[k][b] - ref["u_star"][0, 0]).max() < U_TOL_KIN, (k, b)


def test_simulate_host_and_device_pointers_agree(tracks):
    import torch
    pt, _ = tracks
    B, N, K = 64, 40, 4
    x0 = _dyn_states(B, pt.length, 13)
    with _dyn_ctx(pt, B=B) as c:
        xbar, ubar = _warm(B, N, N, 8, True, np.float32)
        xh, xbh, ubh = x0.copy(), xbar.copy(), ubar.copy()
        lxh, luh, nfh = c.simulate(xh, xbh, ubh, K, MPC_DT, DT, log=True)
        dev = lambda a: torch.from_numpy(a.copy()).cuda()
        xd, xbd, ubd = dev(x0), dev(xbar), dev(ubar)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        lxd, lud, nfd = c.simulate(xd, xbd, ubd, K, MPC_DT, DT, log=True)
        torch.cuda.synchronize()
    np.testing.assert_array_equal(xd.cpu().numpy(), xh)
    np.testing.assert_array_equal(ubd.cpu().numpy(), ubh)
    np.testing.assert_array_equal(lxd.cpu().numpy(), lxh)
    np.testing.assert_array_equal(lud.cpu().numpy(), luh)
    np.testing.assert_array_equal(nfd.cpu().numpy(), nfh)


def test_simulate_argument_errors(tracks):
    from vcmpc import Context, _abi
    from vcmpc._abi import VcError
    from vcmpc.config import load_config, make_params
    pt, _ = tracks
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("dynamic_mpc"))
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=40, max_batch=4, dtype=_abi.VC_F32, params=p) as c:
        x = np.zeros((4, 8))
        xb, ub = np.zeros((4, 40, 8), np.float32), np.zeros((4, 40, 2), np.float32)
        with pytest.raises(VcError, match="no track table"):
            c.simulate(x, xb, ub, 1, MPC_DT, DT)
        c.set_track(pt)
        with pytest.raises(VcError, match="steps"):
            c.simulate(x, xb, ub, -1, MPC_DT, DT)
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=12, max_batch=4, dtype=_abi.VC_F32, params=p) as c:
        c.set_track(pt)
        with pytest.raises(VcError, match="no built vc_solve"):
            c.simulate(np.zeros((4, 8)), np.zeros((4, 12, 8), np.float32), np.zeros((4, 12, 2), np.float32), 1,
                       MPC_DT, DT)


def test_batched_simulator_laps_ippodromo(tracks):
    """BatchedRacingSimulator (racing.py:217-242 for B cars): 256 dynamic-bicycle NMPC
    vehicles, 200 steps (10 s) from spread-out starts, all on the device."""
    from vcmpc.config import load_config
    from vcmpc.models import DynamicCar
    from vcmpc.simulation import BatchedRacingSimulator
    pt, _ = tracks
    B, K = 256, 200
    car = DynamicCar(load_config("dynamic_car"), pt, tyre="fiala")
    cfg = load_config("dynamic_mpc")
    cfg["mpc_dt"] = C5_MPC_DT
    sim = BatchedRacingSimulator(car, cfg, pt, batch=B)
    x0 = _dyn_states(B, pt.length, 21)
    out = sim.reset(x0).run(K)
    X, U = out["state_traj"], out["action_traj"]
    assert X.shape == (K + 1, B, 8) and U.shape == (K, B, 2)
    assert np.isfinite(X).all() and np.isfinite(U).all()
    assert out["nfail"].sum() <= 0.01 * B * K, out["nfail"].sum()
    on_track = (np.abs(X[:, :, 5]) < pt.width / 2).all(axis=0)
    assert on_track.all(), on_track.mean()   # fp64 solve (st_sqp): every vehicle (round 1 fp32: >= 99 %)
    progress = X[-1, :, 4] - X[0, :, 4]
    assert np.median(progress) > K * DT * 8.0
    assert np.abs(U[..., 1]).max() <= 0.4 + 1e-4
    # a second run continues from the stored state and warm starts
    out2 = sim.run(5)
    np.testing.assert_array_equal(out2["state_traj"][0], X[-1])


def test_c5_divergent_vehicles_stay_on_track(tracks):
    """Regression for round 1's C5 divergence: the four vehicles (ids 801, 2640, 5936, 5986
    of the bench's 8,192) that left the track at |ey| ~ 240 m under the fp32 solve (non-finite
    solves from their first step, scripts/c5_divergence.py, fixture c5_divergent_x0.npz).
    The full 500-step C5 job for them, through the fp64 closed loop: on track throughout,
    max |ey| < 4.5 m (the bench criterion), and lap progress."""
    import os
    from conftest import GOLDEN
    from vcmpc.config import load_config
    from vcmpc.models import DynamicCar
    from vcmpc.simulation import BatchedRacingSimulator
    pt, _ = tracks
    x0 = np.load(os.path.join(GOLDEN, "c5_divergent_x0.npz"))["x0"]
    car = DynamicCar(load_config("dynamic_car"), pt, tyre="fiala")
    cfg = load_config("dynamic_mpc")
    cfg["mpc_dt"] = C5_MPC_DT
    sim = BatchedRacingSimulator(car, cfg, pt, batch=len(x0))
    out = sim.reset(x0.copy()).run(500)
    X = out["state_traj"]
    ey = np.abs(X[:, :, 5]).max(axis=0)
    print("max |ey| per vehicle:", ey, "non-solved steps:", out["nfail"].sum(axis=0) if out["nfail"].ndim > 1
          else out["nfail"])
    assert np.isfinite(X).all()
    assert (ey < 4.5).all(), ey
    assert (X[-1, :, 4] - X[0, :, 4] > 250.0).all()
