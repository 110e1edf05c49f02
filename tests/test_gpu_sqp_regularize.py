"""GPU: the regularised retry of the fp64 single-track SQP's QPs (csrc/st_sqp.hip REG instantiations,
vc_set_sqp_regularization / vc_get_sqp_regularization / vc_debug_sqp_breakdown).

A QP whose interior point breaks down is solved again with the proximal weight prox f^j, j = 1..J.
The reference is oracle/dyn_sqp.py dyn_sqp_solve's loop with a level per problem and SQP iteration
(`_ref_sqp` below: the oracle itself does not change): every QP is dyn_qp with prox f^level, solved
exactly by oracle/qp.py, under the same `stopped` rule and domain step.  At all-zero levels it is
dyn_sqp_solve.  The breakdowns of tests 1-6 are forced by the test hook on well-scaled problems
(dynamic_batch(6, N, seed=5)), those of test 7 are the natural ones of the survey-range C3 set.
"""
import functools

import numpy as np
import pytest

from oracle import dyn_sqp as D

pytestmark = pytest.mark.gpu

U_TOL = 1e-5    # the project's bar: ||u* - u*_ref||_inf in N and rad/s
X_TOL = 1e-9    # x* = rollout(u*), relative to 1 + |x| (tests/test_gpu_st_sqp.py's measure)
B, J, F = 6, 3, 10.0
# name -> (N, tyre, controller config)
CASES = {"n20_linear": (20, "linear", "dynamic_mpc"), "n20_fiala": (20, "fiala", "dynamic_mpc"),
         "n60_linear": (60, "linear", "singletrack_mpc")}


@functools.lru_cache(maxsize=None)
def _dyn_params():
    from oracle import models as M
    from vcmpc.config import load_config
    return M.dyn_params_from_config(load_config("dynamic_car"))


def _cfg(name):
    from vcmpc.config import load_config
    return load_config(name)


def _K(case):
    return int(_cfg(CASES[case][2])["qp"]["sqp_iters"])


def _hooks(case):
    """(sqp_iter, problem, levels) of the forced breakdowns."""
    return [(1, 1, 1), (0, 3, 2), (_K(case) - 1, 4, 3)]


@functools.lru_cache(maxsize=None)
def _data(case):
    from vcmpc.workload import dynamic_batch
    return {k: v.astype(np.float64) for k, v in dynamic_batch(B, N=CASES[case][0], seed=5).items()}


def _ctx(N, tyre, cfg, max_batch=B, **kw):
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=cfg, tyre=tyre)
    return Context(model=_abi.VC_MODEL_DYNAMIC, N=N, max_batch=max_batch, dtype=_abi.VC_F64, params=p, **kw)


@functools.lru_cache(maxsize=None)
def _run(case, levels, hook=None):
    """One host-pointer solve of the case's six problems: (u0, x*, u*, status, iters, diag, level or
    None, rollout(u*)).  Shared by the tests, never modified."""
    N, tyre, cname = CASES[case]
    d = _data(case)
    with _ctx(N, tyre, _cfg(cname), regularize_levels=levels, regularize_factor=F if levels else 0.0) as c:
        if hook is not None:
            c.debug_sqp_breakdown(*hook)
        r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        lev = c.sqp_regularization() if levels else None
        xr = c.rollout(d["x0"], r[2], d["kappa"], d["ds"])[:, :N]
    return tuple(r) + (lev, xr)


def _ref_sqp(d, W, tyre, levels, f):
    """oracle.dyn_sqp.dyn_sqp_solve's loop with the QP of SQP iteration i of problem b built at the
    proximal weight prox f^levels[b, i] (entries below 0 count as 0).  Returns u*[B, N, 2], the
    convergence flags [K, B] and the QP scales 1 + max(|g|, |d|) [K, B]."""
    from oracle.qp import solve_qp_batch
    p = _dyn_params()
    x0, kappa, ds = (np.asarray(d[k], np.float64) for k in ("x0", "kappa", "ds"))
    u = np.array(d["ubar"], np.float64, copy=True)
    nb, N = u.shape[:2]
    S = W["fx_scale"]
    stopped = np.zeros(nb, bool)
    convs, scales = [], []
    for it in range(W["sqp_iters"]):
        lev = np.maximum(levels[:, it], 0)
        z, conv, scale = np.zeros((nb, 2 * N)), np.zeros(nb, bool), np.zeros(nb)
        for j in np.unique(lev):
            idx = np.nonzero(lev == j)[0]
            Q = D.dyn_qp(x0[idx], u[idx], kappa[idx], ds[idx], p, dict(W, prox=W["prox"] * f ** int(j)), tyre)
            sol = solve_qp_batch(Q["H"], Q["g"], Q["C"], Q["d"])
            z[idx], conv[idx] = sol["z"], np.asarray(sol["converged"], bool)
            scale[idx] = 1.0 + np.maximum(np.abs(Q["g"]).max(axis=1), np.abs(Q["d"]).max(axis=1))
        if it > 0:
            stopped |= ~conv
        dz = np.where(stopped[:, None], 0.0, z)
        du = dz.reshape(nb, N, 2) * np.array([S, 1.0])
        alpha = D.domain_step(x0, u, du, kappa, ds, p, tyre, D.dyn_predict)
        u = np.where(((alpha > 0) & ~stopped)[:, None, None], u + alpha[:, None, None] * du, u)
        convs.append(conv)
        scales.append(scale)
    return u, np.stack(convs), np.stack(scales)


def _sub(d, idx):
    return {k: v[idx] for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _ref(case, hook):
    """The reference for the hooked problem alone (the problems of a batch are independent), at the
    levels the hook implies; hook None: all six problems at level 0."""
    N, tyre, cname = CASES[case]
    W = D.dyn_weights(_cfg(cname))
    if hook is None:
        return _ref_sqp(_data(case), W, tyre, np.zeros((B, _K(case)), int), F)
    q, b, n = hook
    lev = np.zeros((1, _K(case)), int)
    lev[0, q] = n
    return _ref_sqp(_sub(_data(case), [b]), W, tyre, lev, F)


def test_reference_at_level_zero_is_the_oracle():
    """The reference of this module at all-zero levels is oracle.dyn_sqp.dyn_sqp_solve (CPU only)."""
    case = "n20_linear"
    N, tyre, cname = CASES[case]
    d = _data(case)
    W = D.dyn_weights(_cfg(cname))
    ref = D.dyn_sqp_solve(d["x0"], d["ubar"], d["kappa"], d["ds"], _dyn_params(), W, tyre)
    np.testing.assert_array_equal(_ref(case, None)[0], ref["u_star"])


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_forced_breakdown_parity(case, which):
    """Test 1: the hook breaks rungs 0..n-1 of one QP of one problem; that QP's step comes from level
    n, the level array says so, bit 128 marks the problem, u* is the reference's at those levels and
    the other problems are those of a run with the feature off, bit for bit."""
    hook = _hooks(case)[which]
    q, b, n = hook
    K = _K(case)
    u0, xs, us, st, it, dg, lev, xr = _run(case, J, hook)
    off = _run(case, 0)
    want = np.zeros((B, K), np.int32)
    want[b, q] = n
    np.testing.assert_array_equal(lev, want)
    bits = dg[:, 2].astype(int)
    np.testing.assert_array_equal((bits & 128) > 0, np.arange(B) == b)
    assert not (bits & 64).any()
    uref, conv, _ = _ref(case, hook)
    assert conv.all()
    err = float(np.abs(us[b] - uref[0]).max())
    moved = float(np.abs(uref[0] - off[2][b]).max())   # against the level-0 answer (the run with the feature off)
    rel = np.abs(xs - xr).max(axis=(1, 2)) / (1.0 + np.abs(xr).max(axis=(1, 2)))
    print(f"{case} hook {hook}: |u* - u*_ref(levels)| {err:.3e}; the level moves u*_ref by {moved:.3e}; "
          f"status {st.tolist()}, iters {it.tolist()} (off {off[4].tolist()}); |x* - rollout(u*)| rel {rel.max():.2e}")
    assert st[b] == 0
    assert err < U_TOL
    assert moved > 100 * U_TOL   # a kernel that ignored the level could not pass
    assert rel.max() < X_TOL
    rest = np.arange(B) != b
    for a, o in zip((u0, xs, us, st, it, dg), off[:6]):
        np.testing.assert_array_equal(a[rest], o[rest])


@pytest.mark.parametrize("case", ["n20_linear", "n60_linear"])
def test_exhausted_ladder(case):
    """Test 2: the hook breaks all J + 1 rungs.  At a later QP the problem ends as the same hook ends it
    with the feature off (u*, status, bit 16), with bit 64, level -2 there and -1 after; at QP 0 the
    status is VC_MAX_ITER with bit 64 and level -2."""
    K = _K(case)
    for q, b in ((1, 2), (0, 5)):
        hook = (q, b, J + 1)
        on, off = _run(case, J, hook), _run(case, 0, hook)
        bits_on, bits_off = on[5][:, 2].astype(int), off[5][:, 2].astype(int)
        print(f"{case} hook {hook}: status on {on[3].tolist()} off {off[3].tolist()}; diag[2] on {bits_on.tolist()} "
              f"off {bits_off.tolist()}; levels of the problem {on[6][b].tolist()}")
        for i in (0, 1, 2, 3):   # u0, x*, u*, status: the whole batch
            np.testing.assert_array_equal(on[i], off[i])
        np.testing.assert_array_equal((bits_on & 64) > 0, np.arange(B) == b)
        assert not (bits_on & 128).any() and not (bits_off & (64 | 128)).any()
        np.testing.assert_array_equal(bits_on & ~64, bits_off)
        want = np.zeros((B, K), np.int32)
        want[b, q] = -2
        if q > 0:
            want[b, q + 1:] = -1
            assert bits_on[b] & 16 and bits_off[b] & 16
        else:
            assert on[3][b] == 1 and off[3][b] == 1   # VC_MAX_ITER
        np.testing.assert_array_equal(on[6], want)


def test_off_is_off():
    """Test 3: never set, set to 0, and on then off again are bit-identical to a fresh context in
    outputs, status, iters and diag; on without a breakdown has every level 0 and the same bits."""
    from vcmpc import _abi
    case = "n60_linear"
    N, tyre, cname = CASES[case]
    d = _data(case)
    ref = _run(case, 0)
    for prep in ("zero", "on_off"):
        with _ctx(N, tyre, _cfg(cname)) as c:
            if prep == "on_off":
                c.set_sqp_regularization(J, F)
            c.set_sqp_regularization(0)
            r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
            with pytest.raises(_abi.VcError) as e:
                c.sqp_regularization()
            assert e.value.code == _abi.VC_E_ARG
        for a, o in zip(r, ref[:6]):
            np.testing.assert_array_equal(a, o)
    for cs in CASES:
        on, off = _run(cs, J), _run(cs, 0)
        assert (on[6] == 0).all(), on[6]
        for a, o in zip(on[:6], off[:6]):
            np.testing.assert_array_equal(a, o)


def test_global_j_placement_bit_identical():
    """Test 4: the six N = 60 problems tiled to a batch just above the threshold at which the launch
    takes the global-J kernel (st_sqp_jws_doubles(N, B) > 0: the context then allocates the J
    workspace, which the B = 6 launch does not); the hooked row equals the B = 6 LDS-J run bit for bit,
    and so does every other row equal the unhooked B = 6 run."""
    case = "n60_linear"
    N, tyre, cname = CASES[case]
    hook = _hooks(case)[2]
    q, b, n = hook
    T = 768 // B + 1   # 774 problems: beyond the 768 the LDS-J kernel holds (csrc/st_sqp.hip st_jg_pick)
    row = (T - 1) * B + b
    small, plain = _run(case, J, hook), _run(case, J)
    d = {k: np.ascontiguousarray(np.concatenate([v] * T)) for k, v in _data(case).items()}
    with _ctx(N, tyre, _cfg(cname), max_batch=T * B, regularize_levels=J, regularize_factor=F) as c:
        c.debug_sqp_breakdown(q, row, n)
        big = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        big = tuple(big) + (c.sqp_regularization(),)
    print(f"N={N} B={T * B}: hooked row {row} level {big[6][row].tolist()}, diag[2] {int(big[5][row, 2])}")
    assert big[6][row, q] == n
    for a, s, p in zip(big, small[:7], plain[:7]):
        want = np.concatenate([p] * T)
        want[row] = s[b]
        np.testing.assert_array_equal(a, want)


def test_with_farkas_detection():
    """Test 5: both features on, on the infeasible problems of tests/test_gpu_sqp_infeasible.py: a
    certified problem ends VC_INFEASIBLE with the same Farkas vector and qp_index as with the
    regularisation off and spends no rung (equal iters, level 0 at QP 0, -1 after)."""
    import test_gpu_sqp_infeasible as TI
    N = 20
    P = TI._problems(N)
    d = P["d"]
    off = TI._run(N, True)
    with TI._ctx(N, True) as c:
        c.set_sqp_regularization(J, F)
        r = c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True)
        y, qi = c.sqp_farkas()
        lev = c.sqp_regularization()
    inf = off[3] == 4
    print(f"N={N}: certified {int(inf.sum())} of {TI.B}; levels used on the rest {np.unique(lev[~inf]).tolist()}")
    assert inf.sum() == P["infeasible"].sum() > 0
    np.testing.assert_array_equal(r[3], off[3])
    np.testing.assert_array_equal(r[4][inf], off[4][inf])
    np.testing.assert_array_equal(y, off[6])
    np.testing.assert_array_equal(qi, off[7])
    np.testing.assert_array_equal(r[2][inf], off[2][inf])
    assert (lev[inf, 0] == 0).all() and (lev[inf, 1:] == -1).all()
    assert ((r[5][inf, 2].astype(int) & (64 | 128)) == 0).all()


def test_device_tensors_equal_host_arrays():
    """Test 6: setter, solve and getter with device tensors give the bits of the host-array run."""
    import torch
    case = "n20_linear"
    N, tyre, cname = CASES[case]
    hook = _hooks(case)[1]
    host = _run(case, J, hook)
    with _ctx(N, tyre, _cfg(cname)) as c:
        c.set_sqp_regularization(J, F)
        c.debug_sqp_breakdown(*hook)
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in _data(case).items()}
        r = c.solve(t["x0"], t["kappa"], t["ds"], t["ubar"], diag=True)
        lev = c.sqp_regularization()
        torch.cuda.synchronize()
        assert isinstance(lev, torch.Tensor) and lev.is_cuda and lev.dtype == torch.int32
        got = [a.cpu().numpy() for a in r] + [lev.cpu().numpy()]
    for a, h in zip(got, host[:7]):
        np.testing.assert_array_equal(a, h)


SURVEY_IDX = [610, 1371, 1802, 0, 1, 2, 3, 4]


@functools.lru_cache(maxsize=None)
def _survey():
    from vcmpc.workload import dynamic_batch
    d = dynamic_batch(4096, N=40, seed=31, ranges="survey")
    return {k: np.ascontiguousarray(v[SURVEY_IDX].astype(np.float64)) for k, v in d.items()}


def test_natural_breakdowns():
    """Test 7: problems 610, 1371, 1802 of the survey-range C3 set (the breakdowns of
    tests/test_gpu_certify.py's allowances) and five ordinary ones, J = 3.  Levels, bits 64 / 128 and
    status are consistent with the contract; a problem whose step came from a level above 0 and whose
    ladder was never exhausted meets the reference at the kernel's own levels to 1e-5.

    Measured on an MI355X (J = 3, f = 10): 1371 keeps the step of its second QP at level
    1, 7.6e-6 N from the reference at levels [0, 1, 0]; 1802 that of its third QP at level 3, 5.1e-8 N
    from the reference at [0, 0, 3]; both VC_SOLVED with bit 128.  610 breaks down at every level of
    its first and of its second QP (levels [-2, -2, -1], bits 1 | 16 | 64, VC_MAX_ITER as before): a
    finding the contract labels, not a failure of this test."""
    cfg = _cfg("dynamic_mpc")
    N, tyre, K, nb = 40, "linear", int(cfg["qp"]["sqp_iters"]), len(SURVEY_IDX)
    d = _survey()
    out = {}
    for lv in (0, J):
        with _ctx(N, tyre, cfg, max_batch=nb, regularize_levels=lv, regularize_factor=F if lv else 0.0) as c:
            out[lv] = tuple(c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy(), diag=True))
            if lv:
                lev = c.sqp_regularization()
    off, on = out[0], out[J]
    b_off, b_on = off[5][:, 2].astype(int), on[5][:, 2].astype(int)
    st = on[3]
    print(f"survey {SURVEY_IDX}: off status {off[3].tolist()} diag[2] {b_off.tolist()} iters {off[4].tolist()}")
    print(f"  on (J={J}, f={F:g}) status {st.tolist()} diag[2] {b_on.tolist()} iters {on[4].tolist()} levels {lev.tolist()}")
    # precondition: these are still the breakdown cases
    assert b_off[1] & 16 and b_off[2] & 16 and b_off[0] & 1, b_off[:3].tolist()
    # consistency under the contract
    for b in range(nb):
        lv = lev[b]
        assert ((lv >= -2) & (lv <= J)).all()
        assert bool(b_on[b] & 64) == bool((lv == -2).any())
        ended = np.nonzero(lv == -1)[0]
        if len(ended):   # -1 from the QP after the one that ended the SQP, to the end
            assert (lv[ended[0]:] == -1).all()
            # the SQP ends early at a refused later step (bit 16) or at a non-finite first rollout
            assert (ended[0] >= 2 and b_on[b] & 16) or (ended[0] == 0 and st[b] == 2)
        if b_on[b] & 16:   # stopped at a later QP: the last QP run is not QP 0, nothing after it ran
            assert len(lv) - len(ended) >= 2
        if b_on[b] & 128:
            assert (lv > 0).any()
        if (lv > 0).any() and not (b_on[b] & 16):
            assert b_on[b] & 128   # every such QP's step was applied
        if lv[0] == -2:           # the first QP's failure: its iterate applied, never VC_SOLVED
            assert st[b] != 0 and b_on[b] & 1
        if (lv[1:] == -2).any():  # a later QP's failure: the step refused, the SQP stopped
            assert b_on[b] & 16
    # problems the ladder never touched are those of the run with the feature off
    same = (lev <= 0).all(axis=1) & ((b_on & 64) == 0)
    for a, o in zip(on[:4], off[:4]):
        np.testing.assert_array_equal(a[same], o[same])
    # parity at the kernel's own levels
    cmp_idx = [b for b in range(nb) if b_on[b] & 128 and not (lev[b] == -2).any()]
    W = D.dyn_weights(cfg)
    for b in cmp_idx:
        uref, conv, scale = _ref_sqp(_sub(d, [b]), W, tyre, lev[b:b + 1], F)
        err = float(np.abs(on[2][b] - uref[0]).max())
        print(f"  problem {SURVEY_IDX[b]}: levels {lev[b].tolist()}, status {int(st[b])}, |u* - u*_ref(levels)| {err:.3e}; "
              f"reference QPs converged {conv[:, 0].tolist()}, scales {np.array2string(scale[:, 0], precision=2)}")
        assert err < U_TOL, (SURVEY_IDX[b], err)
    for b in range(3):
        if b not in cmp_idx:
            print(f"  problem {SURVEY_IDX[b]}: levels {lev[b].tolist()}, status {int(st[b])}, diag[2] {int(b_on[b])}: "
                  f"not compared (ladder exhausted or no level above 0)")


def test_refusals():
    """VC_E_UNSUPPORTED on kinematic, cascaded, fp32 and N = 45 contexts; VC_E_ARG for levels -1 / 7,
    factor 0.5 / 1.0, and for the getter with the feature off or a B beyond the last solve's."""
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    with Context(model=_abi.VC_MODEL_KINEMATIC, N=20, max_batch=4, kin_car=load_config("kinematic_car"),
                 kin_mpc=load_config("kinematic_mpc")) as c:
        assert c.lib.vc_set_sqp_regularization(c._h, 3, 10.0) == _abi.VC_E_UNSUPPORTED
        with pytest.raises(_abi.VcError) as e:
            c.set_sqp_regularization(3)
        assert e.value.code == _abi.VC_E_UNSUPPORTED
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("cascaded_mpc"), tyre="fiala")
    with Context(model=_abi.VC_MODEL_CASCADED, N=20, max_batch=4, dtype=_abi.VC_F64, params=p) as c:
        assert c.lib.vc_set_sqp_regularization(c._h, 3, 10.0) == _abi.VC_E_UNSUPPORTED
    p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("dynamic_mpc"), tyre="linear")
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=40, max_batch=4, dtype=_abi.VC_F32, params=p) as c:
        assert c.lib.vc_set_sqp_regularization(c._h, 3, 10.0) == _abi.VC_E_UNSUPPORTED
    with Context(model=_abi.VC_MODEL_DYNAMIC, N=45, max_batch=4, dtype=_abi.VC_F64, params=p) as c:
        assert c.lib.vc_set_sqp_regularization(c._h, 3, 10.0) == _abi.VC_E_UNSUPPORTED
    with pytest.raises(_abi.VcError) as e:
        Context(model=_abi.VC_MODEL_DYNAMIC, N=45, max_batch=4, dtype=_abi.VC_F64, params=p, regularize_levels=3)
    assert e.value.code == _abi.VC_E_UNSUPPORTED
    case = "n20_linear"
    N, tyre, cname = CASES[case]
    d = _data(case)
    with _ctx(N, tyre, _cfg(cname)) as c:
        lev = np.empty((B, _K(case)), np.int32)
        for levels, factor in ((-1, 10.0), (7, 10.0), (3, 0.5), (3, 1.0)):
            assert c.lib.vc_set_sqp_regularization(c._h, levels, factor) == _abi.VC_E_ARG
        assert c.lib.vc_get_sqp_regularization(c._h, B, lev.ctypes.data, _abi.VC_HOST_PTRS) == _abi.VC_E_ARG  # off
        assert c.lib.vc_set_sqp_regularization(c._h, 6, 0.0) == 0   # factor <= 0 keeps the default
        assert c.lib.vc_get_sqp_regularization(c._h, 1, lev.ctypes.data, _abi.VC_HOST_PTRS) == _abi.VC_E_ARG  # no solve yet
        c.solve(d["x0"][:4], d["kappa"][:4], d["ds"][:4], d["ubar"][:4].copy())
        assert c.lib.vc_get_sqp_regularization(c._h, 4, lev.ctypes.data, _abi.VC_HOST_PTRS) == 0
        assert c.lib.vc_get_sqp_regularization(c._h, 5, lev.ctypes.data, _abi.VC_HOST_PTRS) == _abi.VC_E_ARG
        assert c.lib.vc_get_sqp_regularization(c._h, B + 1, lev.ctypes.data, _abi.VC_HOST_PTRS) == _abi.VC_E_ARG


def test_controller_config_keys():
    """`qp.regularize_levels` / `qp.regularize_factor` of the single-track controller config turn the
    feature on (default off), and a kept solve that used a level above 0 is counted per vehicle."""
    from vcmpc.config import load_config
    from vcmpc.controllers import cascaded_mpc as CM
    from vcmpc.environment import CurvatureTrack
    from vcmpc.models import DynamicCar
    n, N = 4, 20
    car = DynamicCar(load_config("dynamic_car"), CurvatureTrack(constant=1 / 60), tyre="linear")
    x0 = np.zeros((n, 8))
    x0[:, 0] = np.linspace(10.0, 16.0, n)
    x0[:, 4] = 6.0
    cfg = _cfg("singletrack_mpc")
    cfg["horizon"] = N
    off = CM.BatchedSingleTrackMPC(car, cfg, batch=n)
    assert off.regularize_levels == 0 and off.ctx.regularize_levels == 0
    u_off = off.command(x0)
    assert (off.regularized_steps == 0).all()
    cfg["qp"] = dict(cfg["qp"], regularize_levels=2, regularize_factor=100.0)
    on = CM.BatchedSingleTrackMPC(car, cfg, batch=n)
    assert on.regularize_levels == 2 and on.ctx.regularize_levels == 2 and on.regularize_factor == 100.0
    on.ctx.debug_sqp_breakdown(1, 2, 1)
    u_on = on.command(x0)
    print(f"controller: regularized steps {on.regularized_steps.tolist()}, status {on.status.tolist()}")
    assert (on.status == 0).all()
    np.testing.assert_array_equal(on.regularized_steps, [0, 0, 1, 0])
    rest = np.arange(n) != 2
    np.testing.assert_array_equal(u_on[rest], u_off[rest])
    assert np.abs(u_on[2] - u_off[2]).max() > 0.0
