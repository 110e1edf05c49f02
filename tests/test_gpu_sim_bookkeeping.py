"""GPU: vc_simulate against its own definition (include/vcmpc.h): one step is
vc_horizon -> vc_solve -> vc_drive plus the stated policy, rebuilt here on the host from the public
calls and compared with vc_simulate(steps = K, log = True) step by step.

Reference for step k (numpy; `ctx.*` are the public entry points, which run the same kernels on the same
bits as the loop inside vc_simulate, so every comparison is bit for bit):

    kap, ds        = ctx.horizon(x, xbar, MPC_DT)
    u0, xs, us, st = ctx.solve(x, kap, ds, ubar.copy())
    u_app          = where(st == 0, u0, 0)
    x_new          = ctx.drive(x.copy(), u_app, DT)           # public vc_drive: no status, no bookkeeping
    solved, no shift : ubar' = us,  xbar' = xs
    solved, shift    : ubar'[k] = us[k+1], last kept;  xbar'[k] = xs[k+1], last kept
    failed           : ubar' = 0,  xbar'[:, j] = x_new for every column j,  nfail += 1
    failed, cascaded : tail k >= N:  ubar'[k] = (Frr + Cd V^2,  m V^2 kap[k]),
                       V = max(hypot(Ux, Uy), 3) of the state *before* the step

The one restated formula is the cascaded neutral tail, compared at 1e-12 relative (the project's bar for an
fp64 restatement of one formula, tests/test_gpu_parity.py) with this file's numpy and with
BatchedCascadedMPC._neutral (vcmpc/controllers/cascaded_mpc.py), which the kernel names as its mirror.  Both
take V from the state before the step, as the kernel does.

Every batch: six vehicles from the closed-loop samplers of test_gpu_closed_loop.py on its `_warm` warm start
and two that fail every step through per-problem status only -- kinematic: v = 0 (VC_NONFINITE) and
delta0 = delta_max + 0.2; single track / cascaded: delta0 = delta_max + 0.1 (|w| <= 0.4 rad/s moves delta by
about 0.012 rad per stage, so the delta rows of the first stages cannot be met: phase 1 of
oracle/feasibility.py on kin_qp / dyn_qp of these starts gives t* = 0.154 / 0.096 with a valid Farkas
certificate).  u = 0 leaves delta where it is, so they fail again at every step.

What would fail here: the shift loop reading stage k instead of k + 1 (ubar / xbar of every solved vehicle
of a shift = 1 context); the failed branch not filling xbar (xbar of the failing vehicles, and through
vc_horizon their next step); a wrong restart input, nfail count or log slot.
"""
import functools

import numpy as np
import pytest

from test_gpu_closed_loop import DT, MPC_DT, _dyn_states, _kin_states, _warm

pytestmark = pytest.mark.gpu

B, K = 8, 4
FAIL = [6, 7]          # the vehicles made to fail
GOOD = [0, 1, 2, 3, 4, 5]
CASES = {
    # name: model, N, M, vc_qp.solver, detection, vc_qp.shift
    "kin_ltv": ("kin", 20, 0, 0, False, 0),
    "kin_ric-shift": ("kin", 10, 0, 1, False, 1),
    "kin_ric-det-shift": ("kin", 10, 0, 1, True, 1),
    "st_sqp": ("dyn", 20, 0, 0, False, 0),
    "st_sqp-shift": ("dyn", 20, 0, 0, False, 1),
    "st_sqp-det-shift": ("dyn", 20, 0, 0, True, 1),
    "casc_ric-shift-ignored": ("casc", 20, 15, 0, False, 1),
}


@functools.lru_cache(maxsize=None)
def _track():
    from vcmpc.environment import Track
    return Track.load("ippodromo")


def _ctx(case):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    model, N, M, solver, detect, shift = CASES[case]
    if model == "kin":
        cfg = load_config("kinematic_mpc")
        cfg["qp"] = dict(cfg["qp"], solver=solver, shift=shift)
        p = make_params(kin_car=load_config("kinematic_car"), kin_mpc=cfg)
        mid = _abi.VC_MODEL_KINEMATIC
    else:
        cfg = load_config("cascaded_mpc" if model == "casc" else "dynamic_mpc")
        if model == "casc":
            cfg["horizon_pm"] = M
        cfg["qp"] = dict(cfg["qp"], solver=solver, shift=shift)
        p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=cfg, tyre="fiala")
        mid = _abi.VC_MODEL_CASCADED if model == "casc" else _abi.VC_MODEL_DYNAMIC
    assert p.qp.shift == shift
    c = Context(model=mid, N=N, max_batch=B, dtype=_abi.VC_F64, params=p, detect_infeasible=detect)
    c.set_track(_track())
    return c


def _start(case):
    model, N, M = CASES[case][:3]
    L = _track().length
    if model == "kin":
        x = _kin_states(B, L, 41)
        x[6, 0] = 0.0                # v = 0: the spatial ODE is singular, VC_NONFINITE
        x[7, 1] = 0.3 + 0.2          # delta0 = delta_max + 0.2
        xbar, ubar = _warm(B, N, N + 1, 6, False, np.float64)
    else:
        x = _dyn_states(B, L, 42)
        x[FAIL, 3] = 0.45 + 0.1      # delta0 = delta_max + 0.1
        xbar, ubar = _warm(B, N + M, N + M, 8, True, np.float64)
    return x, xbar, ubar


def _neutral_tail(x_prev, kap, N):
    """The cascaded failure restart's point-mass inputs [B, M, 2] from the state before the step."""
    from vcmpc.config import load_config
    car = load_config("dynamic_car")
    m, Frr, Cd = float(car["car"]["m"]), float(car["env"]["Frr"]), float(car["env"]["Cd"])
    V = np.maximum(np.hypot(x_prev[:, 0], x_prev[:, 1]), 3.0)[:, None]
    return np.stack([np.broadcast_to(Frr + Cd * (V * V), kap[:, N:].shape), m * (V * V) * kap[:, N:]], -1)


def _reference(c, case, x0, xbar0, ubar0):
    """K steps of the definition on the host.  Returns the logs, the final buffers, and per step the
    status and (cascaded) the inputs of the neutral tail."""
    model, N, M, _, _, shift = CASES[case]
    x, xbar, ubar = x0.copy(), xbar0.copy(), ubar0.copy()
    nfail = np.zeros(B, np.int32)
    log_x, log_u, stats, tails, ubar_steps = [x.copy()], [], [], [], []
    for _ in range(K):
        kap, ds = c.horizon(x, xbar, MPC_DT)
        u0, xs, us, st, it = c.solve(x, kap, ds, ubar.copy())
        ok = st == 0
        u_app = np.ascontiguousarray(np.where(ok[:, None], u0, 0.0))
        x_new = c.drive(x.copy(), u_app, DT)
        ubar, xbar = us.copy(), xs.copy()
        if shift and model != "casc":
            ubar[:, :-1] = us[:, 1:]
            xbar[:, :-1] = xs[:, 1:]
        ubar[~ok] = 0.0
        xbar[~ok] = x_new[~ok, None, :]
        nfail += (~ok).astype(np.int32)
        if model == "casc":
            tail = _neutral_tail(x, kap, N)
            ubar[~ok, N:] = tail[~ok]
            tails.append((x.copy(), kap.copy()))
        log_u.append(u_app)
        stats.append(st.copy())
        ubar_steps.append(ubar.copy())
        x = x_new
        log_x.append(x.copy())
    return dict(log_x=np.stack(log_x), log_u=np.stack(log_u), x=x, xbar=xbar, ubar=ubar, nfail=nfail,
                status=np.stack(stats), tails=tails, ubar_steps=ubar_steps)


@functools.lru_cache(maxsize=None)
def _run(case):
    """One vc_simulate(K) run and the reference of the same start; computed once per case and shared
    (never modified) by the tests."""
    x0, xbar0, ubar0 = _start(case)
    with _ctx(case) as c:
        x, xbar, ubar = x0.copy(), xbar0.copy(), ubar0.copy()
        log_x, log_u, nfail = c.simulate(x, xbar, ubar, K, MPC_DT, DT, log=True)
        sim = dict(log_x=log_x, log_u=log_u, x=x, xbar=xbar, ubar=ubar, nfail=nfail)
        ref = _reference(c, case, x0, xbar0, ubar0)
        # the buffers after one step, for the shift = 0 / shift = 1 comparison
        x1, xbar1, ubar1 = x0.copy(), xbar0.copy(), ubar0.copy()
        c.simulate(x1, xbar1, ubar1, 1, MPC_DT, DT)
        sim["ubar_step1"] = ubar1
    return sim, ref


@pytest.mark.parametrize("case", list(CASES))
def test_simulate_equals_its_definition(case):
    """Measured on an MI355X: every case bit-identical; cascaded neutral tail against this file's
    numpy and against BatchedCascadedMPC._neutral: relative error 0 / 0 (V 12.18 and 12.33 m/s before
    the last step, 12.06 and 12.21 after it); status of the failing vehicles at every step: kinematic
    [2, 1] ([2, 4] with detection), single track [1, 1] ([4, 4] with detection), cascaded [1, 1];
    nfail of the six sampled vehicles 0 in every case."""
    model, N, M, _, detect, shift = CASES[case]
    sim, ref = _run(case)
    print(f"{case}: status per step {ref['status'].tolist()}, nfail {sim['nfail'].tolist()}")
    # the set is what the docstring says: the failing vehicles fail at every step ...
    assert (ref["status"][:, FAIL] != 0).all(), ref["status"]
    if detect:   # the delta vehicles are certified: VC_INFEASIBLE takes the failure path in the loop
        certified = [7] if model == "kin" else FAIL
        assert (ref["status"][:, certified] == 4).all(), ref["status"]
    np.testing.assert_array_equal(sim["nfail"][FAIL], K)
    assert not sim["log_u"][:, FAIL].any()
    # ... and the sampled vehicles solve (a condition of the test, not a property under test)
    assert (sim["nfail"][GOOD] == 0).sum() >= 4, sim["nfail"]
    # the comparison
    np.testing.assert_array_equal(sim["log_x"], ref["log_x"])
    np.testing.assert_array_equal(sim["log_u"], ref["log_u"])
    np.testing.assert_array_equal(sim["x"], ref["x"])
    np.testing.assert_array_equal(sim["nfail"], ref["nfail"])
    np.testing.assert_array_equal(sim["xbar"], ref["xbar"])
    if model != "casc":
        np.testing.assert_array_equal(sim["ubar"], ref["ubar"])
    else:
        failed = ref["status"][-1] != 0
        exact = np.ones(sim["ubar"].shape, bool)
        exact[failed, N:] = False
        np.testing.assert_array_equal(sim["ubar"][exact], ref["ubar"][exact])
        got, want = sim["ubar"][failed, N:], ref["ubar"][failed, N:]
        assert np.abs(want).max() > 100.0   # forces in N, not a tail of zeros
        rel = (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max()
        # the controller's neutral guess, the kernel's stated mirror
        from vcmpc.config import load_config
        from vcmpc.controllers.cascaded_mpc import BatchedCascadedMPC
        from vcmpc.models import DynamicCar
        cfg = load_config("cascaded_mpc")
        cfg["horizon_pm"] = M
        ctl = BatchedCascadedMPC(DynamicCar(load_config("dynamic_car"), _track(), tyre="fiala"), cfg, batch=B)
        x_prev, kap = ref["tails"][-1]
        mirror = ctl._neutral(x_prev, kap)[failed, N:]
        ctl.ctx.close()
        rel_m = (np.abs(got - mirror) / np.maximum(np.abs(mirror), 1e-300)).max()
        print(f"{case}: neutral tail relative error {rel:.2e} (numpy), {rel_m:.2e} (BatchedCascadedMPC._neutral); "
              f"V before / after the step {np.hypot(*x_prev[failed, :2].T).tolist()} / "
              f"{np.hypot(*ref['x'][failed, :2].T).tolist()}")
        assert rel < 1e-12
        assert rel_m < 1e-12
        # the state before the step is not the state after it, so the comparison tells the two apart
        after = _neutral_tail(ref["x"], kap, N)[failed]
        assert (np.abs(after - want) / np.maximum(np.abs(want), 1e-300)).max() > 1e-9


@pytest.mark.parametrize("plain,shifted", [("kin_ltv", "kin_ric-shift"), ("st_sqp", "st_sqp-shift")])
def test_public_drive_is_the_plant_whatever_shift_says(plain, shifted):
    """vc_drive is the plant alone: it takes no status and no warm starts, so vc_qp.shift -- a
    vc_simulate policy -- must not act in it.  (Before this test the drive kernel entered its shift
    branch whenever the flag was set and the vehicle had not failed, also from vc_drive, where the
    warm-start pointers are null: the reference loop above could not run on a shift = 1 context.)"""
    x0 = _start(plain)[0]
    u = np.random.default_rng(3).uniform(-0.3, 0.3, (B, 2))
    out = []
    for case in (plain, shifted):
        with _ctx(case) as c:
            out.append(c.drive(x0.copy(), u, DT))
    assert (out[0] != x0).any()
    np.testing.assert_array_equal(out[0], out[1])


def test_shift_flag_reaches_the_kernel():
    """The shift = 1 and shift = 0 runs of the same single-track start differ in ubar after step 1 on
    a solved vehicle (the first solve is the same: the flag only acts after it), and the shifted plan is
    the unshifted one moved one stage, the last stage kept.  A cascaded context ignores the flag."""
    s0, r0 = _run("st_sqp")
    s1, r1 = _run("st_sqp-shift")
    solved = np.nonzero((r0["status"][0] == 0) & (r1["status"][0] == 0))[0]
    assert len(solved) >= 4
    np.testing.assert_array_equal(r0["status"][0], r1["status"][0])
    u_plain, u_shift = s0["ubar_step1"], s1["ubar_step1"]
    assert all((u_plain[b] != u_shift[b]).any() for b in solved)
    np.testing.assert_array_equal(u_shift[solved, :-1], u_plain[solved, 1:])
    np.testing.assert_array_equal(u_shift[solved, -1], u_plain[solved, -1])
    # cascaded, shift = 1 in the config: the warm start after step 1 is u* itself (no stage moved)
    sc, rc = _run("casc_ric-shift-ignored")
    ok = np.nonzero(rc["status"][0] == 0)[0]
    assert len(ok) >= 4
    np.testing.assert_array_equal(sc["ubar_step1"][ok], rc["ubar_steps"][0][ok])
    assert all((rc["ubar_steps"][0][b, :-1] != rc["ubar_steps"][0][b, 1:]).any() for b in ok)
