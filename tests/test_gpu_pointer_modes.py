"""GPU: every entry point that takes VC_HOST_PTRS or VC_DEVICE_PTRS, called both ways on identical
inputs through the public ``Context`` API: host numpy arrays (staged through the context's arena) and
device tensors (``torch.from_numpy(...).cuda()``).  Both run the same kernel on the same bits, so

* every output agrees bit for bit (``np.testing.assert_array_equal``);
* the read-only inputs are unchanged after the call (``ubar_in`` of ``solve_from`` among them);
* a NULL optional buffer (diag, x_ctx, log_x, log_u) is NULL in both modes: the calls with and
  without it agree on everything else.

B = 9 throughout: one full group of eight plus the tail of the kernels' problem-to-workgroup mapping
(``xcd_problem``), the smallest batch that takes both of its branches.  Shapes are the smallest built
ones, data from ``vcmpc.workload``.  The batches are feasible, so with the detection on every
certificate must come back zero with ``qp_index == -1``: the kernels write them for every problem.
Infeasible problems are the business of tests/test_gpu_*infeasible.py.

Not covered: cascaded ``qp.solver = 2`` (condensed, M = 40 only; tests/test_gpu_casc.py).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 9
DT, MPC_DT = 0.05, 0.03


# -- contexts and data ---------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _side_stream():
    """Every test runs inside a torch side stream that its contexts share (``_ctx``), so torch's own
    work on the device tensors (uploads, ``torch.zeros``, ``.cpu()``) is ordered with the library's.
    torch's default stream will not do: its handle is 0, which ``vc_set_stream`` reads as "the
    context's own stream"."""
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        yield
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _track():
    from vcmpc.environment import Track
    return Track.load("ippodromo")


def _ctx(kind, N, detect=False, track=False, M=15):
    """A context on torch's current stream (``_side_stream``)."""
    import torch
    from vcmpc import Context, _abi
    from vcmpc.config import load_config, make_params
    if kind == "kin":
        p = make_params(kin_car=load_config("kinematic_car"), kin_mpc=load_config("kinematic_mpc"))
        model, dtype = _abi.VC_MODEL_KINEMATIC, _abi.VC_F64
    elif kind == "casc":
        cfg = load_config("cascaded_mpc")
        cfg["horizon_pm"] = M
        p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=cfg)
        model, dtype = _abi.VC_MODEL_CASCADED, _abi.VC_F64
    else:
        p = make_params(dyn_car=load_config("dynamic_car"), dyn_mpc=load_config("dynamic_mpc"))
        model, dtype = _abi.VC_MODEL_DYNAMIC, _abi.VC_F64 if kind == "dyn64" else _abi.VC_F32
    c = Context(model=model, N=N, max_batch=B, dtype=dtype, params=p, detect_infeasible=detect)
    assert torch.cuda.current_stream().cuda_stream != 0
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    if track:
        c.set_track(_track())
    return c


@functools.lru_cache(maxsize=None)
def _data(kind, N):
    """The batch of a context kind; shared by the tests, which copy what they pass on."""
    from vcmpc import workload as W
    if kind == "kin":
        return W.kinematic_batch(B, N)
    if kind == "casc":
        return W.cascaded_batch(B, M=15)
    d = W.dynamic_batch(B, N)
    return {k: v.astype(np.float64) for k, v in d.items()} if kind == "dyn64" else d


def _dev(a):
    import torch
    return torch.from_numpy(a.copy()).cuda()


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _both(call, ro, rw=None):
    """``call(**arrays)`` on host copies of ``ro`` / ``rw`` (read-only / updated in place) and on device
    copies.  Asserts that ``ro`` is unchanged in both modes and that every returned array and every
    ``rw`` array agrees bit for bit; returns the host call's (outputs, rw arrays)."""
    import torch
    rw = rw or {}
    res = []
    for to in (np.copy, _dev):
        a_ro, a_rw = {k: to(v) for k, v in ro.items()}, {k: to(v) for k, v in rw.items()}
        out = call(**a_ro, **a_rw)
        torch.cuda.synchronize()
        for k, v in ro.items():
            np.testing.assert_array_equal(_np(a_ro[k]), v, err_msg=f"read-only input {k} changed")
        out = out if isinstance(out, tuple) else (out,)
        res.append(([_np(o) for o in out if o is not None], {k: _np(v) for k, v in a_rw.items()}))
    (out_h, rw_h), (out_d, rw_d) = res
    assert len(out_h) == len(out_d)
    for i, (h, d) in enumerate(zip(out_h, out_d)):
        np.testing.assert_array_equal(d, h, err_msg=f"output {i}")
    for k in rw:
        np.testing.assert_array_equal(rw_d[k], rw_h[k], err_msg=f"in/out buffer {k}")
    return out_h, rw_h


def _solve_args(d):
    return dict(x0=d["x0"], kappa=d["kappa"], ds=d["ds"]), dict(ubar=d["ubar"])


# -- kinematic fp64 N = 20 -----------------------------------------------------------------
def test_kinematic_solve_with_and_without_diag():
    ro, rw = _solve_args(_data("kin", 20))
    with _ctx("kin", 20) as c:
        plain, u_plain = _both(c.solve, ro, rw)
        diag, u_diag = _both(functools.partial(c.solve, diag=True), ro, rw)
    assert len(plain) == 5 and len(diag) == 6 and diag[5].shape == (B, 4)
    for a, b in zip(plain, diag):  # diag = NULL changes nothing else
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(u_plain["ubar"], u_diag["ubar"])
    np.testing.assert_array_equal(plain[2], u_plain["ubar"])  # u* is written through ubar
    assert (plain[3] == 0).all()


def test_kinematic_solve_from_leaves_ubar_in():
    d = _data("kin", 20)
    ro = dict(x0=d["x0"], kappa=d["kappa"], ds=d["ds"], ubar_in=d["ubar"])
    with _ctx("kin", 20) as c:
        out, rw = _both(c.solve_from, ro, dict(u_out=np.zeros_like(d["ubar"])))
        ref, _ = _both(c.solve, *_solve_args(d))
    np.testing.assert_array_equal(out[2], rw["u_out"])
    for a, b in zip(out, ref):  # the same step as vc_solve on a copy of the warm start
        np.testing.assert_array_equal(a, b)


def test_kinematic_model_calls():
    d = _data("kin", 20)
    x, u, k, s = d["x0"], np.ascontiguousarray(d["ubar"][:, 0]), np.ascontiguousarray(d["kappa"][:, 0]), \
        np.ascontiguousarray(d["ds"][:, 0])
    horizon = dict(x0=d["x0"], ubar=d["ubar"], kappa=d["kappa"], ds=d["ds"])
    with _ctx("kin", 20) as c:
        _both(c.condense, horizon)
        (xbar,), _ = _both(c.rollout, horizon)
        _both(c.linearize, dict(xbar=xbar, ubar=d["ubar"], kappa=d["kappa"], ds=d["ds"]))
        _both(functools.partial(c.plant_step, dt=DT), dict(x=x, u=u, kappa=k))
        f_t, _ = _both(functools.partial(c.ode, space=False), dict(x=x, u=u, kappa=k))
        f_s, _ = _both(functools.partial(c.ode, space=True), dict(x=x, u=u, kappa=k))
        _both(c.spatial_step, dict(x=x, u=u, kappa=k, ds=s))
    assert not np.array_equal(f_t[0], f_s[0])


def test_kinematic_track_calls():
    d = _data("kin", 20)
    u0 = np.ascontiguousarray(d["ubar"][:, 0])
    with _ctx("kin", 20, track=True) as c:
        xbar = c.rollout(d["x0"], d["ubar"], d["kappa"], d["ds"])
        _both(c.track_k, dict(s=np.ascontiguousarray(d["x0"][:, 2])))
        _both(functools.partial(c.horizon, mpc_dt=MPC_DT), dict(x0=d["x0"], xbar=xbar))
        _, x_plain = _both(functools.partial(c.drive, dt=DT), dict(u0=u0), dict(x64=d["x0"]))
        _, x_ctx = _both(functools.partial(c.drive, dt=DT), dict(u0=u0), dict(x64=d["x0"], x_ctx=np.zeros((B, 6))))
        np.testing.assert_array_equal(x_plain["x64"], x_ctx["x64"])  # x_ctx = NULL changes nothing else
        np.testing.assert_array_equal(x_ctx["x_ctx"], x_ctx["x64"])  # fp64 context: the same state

        state = dict(x64=d["x0"], xbar=xbar, ubar=d["ubar"])
        sim = functools.partial(c.simulate, steps=2, mpc_dt=MPC_DT, dt=DT)
        logs, logged = _both(functools.partial(sim, log=True), {}, dict(state, nfail=np.zeros(B, np.int32)))
        quiet, unlogged = _both(functools.partial(sim, log=False, nfail=None), {}, state)
    assert logs[0].shape == (3, B, 6) and logs[1].shape == (2, B, 2)
    np.testing.assert_array_equal(logs[0][0], d["x0"])
    np.testing.assert_array_equal(logs[0][2], logged["x64"])
    for k in state:  # log_x = log_u = NULL changes nothing else
        np.testing.assert_array_equal(unlogged[k], logged[k])
    np.testing.assert_array_equal(quiet[0], logged["nfail"])


# -- infeasibility detection: certificates and getter errors ----------------------------------
def _certificates(c, getter):
    """The getter's arrays of the last solve as numpy, and whether it returned host arrays (it
    answers in the kind of that solve's buffers)."""
    out = getattr(c, getter)()
    out = out if isinstance(out, tuple) else (out,)
    return tuple(_np(o) for o in out), isinstance(out[0], np.ndarray)


DETECT = {"kin": ("kin", 10, "farkas", 7 * 10 - 3), "dyn64": ("dyn64", 20, "sqp_farkas", 12 * 20 - 3),
          "casc": ("casc", 20, "casc_farkas", 12 * 20 - 3 + 6 * 15)}


@pytest.mark.parametrize("kind", list(DETECT))
def test_certificates_of_feasible_batches(kind):
    import torch
    kind, N, getter, rows = DETECT[kind]
    d = _data(kind, N)
    got = []
    with _ctx(kind, N, detect=True) as c:
        for to in (np.copy, _dev):
            out = c.solve(to(d["x0"]), to(d["kappa"]), to(d["ds"]), to(d["ubar"]), diag=True)
            cert, host = _certificates(c, getter)
            torch.cuda.synchronize()
            assert host == (to is np.copy)
            got.append(([_np(o) for o in out], cert))
    (out_h, cert_h), (out_d, cert_d) = got
    for h, dv in zip(out_h + list(cert_h), out_d + list(cert_d)):
        np.testing.assert_array_equal(dv, h)
    print(kind, "status", out_h[3], "|y|max", np.abs(cert_h[0]).max(), "qp_index", cert_h[1:])
    assert cert_h[0].shape == (B, rows) and not cert_h[0].any()
    assert (out_h[3] != 4).all()  # no VC_INFEASIBLE
    if getter != "farkas":
        assert cert_h[1].shape == (B,) and (cert_h[1] == -1).all()


def _get_raises(c, getter, rows):
    """The getter for B problems fails in both pointer modes (the device-pointer call through the
    library: ``Context`` picks the mode from the last solve, and there is none to go by)."""
    import torch
    from vcmpc import _abi
    with pytest.raises(_abi.VcError) as e:
        getattr(c, getter)(B)
    assert e.value.code == _abi.VC_E_ARG and f"vc_get_{getter}" in str(e.value)
    y = torch.zeros((B, rows), dtype=torch.float64, device="cuda")
    qi = torch.zeros((B,), dtype=torch.int32, device="cuda")
    ptrs = [y.data_ptr()] + ([qi.data_ptr()] if getter != "farkas" else [])
    with pytest.raises(_abi.VcError) as e:
        c._check(getattr(c.lib, f"vc_get_{getter}")(c._h, B, *ptrs, _abi.VC_DEVICE_PTRS))
    assert e.value.code == _abi.VC_E_ARG and f"vc_get_{getter}" in str(e.value)
    torch.cuda.synchronize()
    assert not y.any() and not qi.any()  # nothing was copied


@pytest.mark.parametrize("kind", list(DETECT))
def test_getter_before_any_solve_and_with_detection_off(kind):
    kind, N, getter, rows = DETECT[kind]
    d = _data(kind, N)
    setter = {"farkas": "set_infeasibility", "sqp_farkas": "set_sqp_infeasibility",
              "casc_farkas": "set_casc_infeasibility"}[getter]
    with _ctx(kind, N, detect=True) as c:
        _get_raises(c, getter, rows)            # on, but no solve yet
        c.solve(_dev(d["x0"]), _dev(d["kappa"]), _dev(d["ds"]), _dev(d["ubar"]))
        assert _certificates(c, getter)[0][0].shape == (B, rows)
        getattr(c, setter)(True)
        _get_raises(c, getter, rows)            # set again: the last solve no longer counts
        c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy())
        getattr(c, setter)(False)
        _get_raises(c, getter, rows)            # off
        getattr(c, setter)(True)                # the buffers were kept
        c.solve(d["x0"], d["kappa"], d["ds"], d["ubar"].copy())
        assert not _certificates(c, getter)[0][0].any()


# -- dynamic and cascaded contexts ---------------------------------------------------------
def test_dynamic_fp32_calls():
    d = _data("dyn32", 40)
    x, u, k, s = d["x0"], np.ascontiguousarray(d["ubar"][:, 0]), np.ascontiguousarray(d["kappa"][:, 0]), \
        np.ascontiguousarray(d["ds"][:, 0])
    with _ctx("dyn32", 40) as c:
        out, _ = _both(c.solve, *_solve_args(d))
        _both(functools.partial(c.plant_step, dt=DT), dict(x=x, u=u, kappa=k))
        _both(c.spatial_step, dict(x=x, u=u, kappa=k, ds=s))
    assert out[0].dtype == np.float32 and out[1].shape == (B, 40, 8)


def test_cascaded_solve_and_simulate():
    d = _data("casc", 20)
    with _ctx("casc", 20, detect=True, track=True) as c:
        out, rw = _both(c.solve, *_solve_args(d))
        state = dict(x64=d["x0"], xbar=out[1], ubar=rw["ubar"], nfail=np.zeros(B, np.int32))
        logs, _ = _both(functools.partial(c.simulate, steps=2, mpc_dt=MPC_DT, dt=DT, log=True), {}, state)
    assert out[1].shape == (B, 35, 8) and logs[0].shape == (3, B, 8) and logs[1].shape == (2, B, 2)
