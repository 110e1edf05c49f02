"""Batched solve context: the Python face of ``vc_ctx`` (include/vcmpc.h).

Every method takes either host numpy arrays (the call stages them through the
context's device arena and returns when results are back in the caller's arrays)
or device-resident ``torch`` tensors on the context's GPU (the call only enqueues
work on the context stream -- the fast path, used by ``bench.py``).

Shapes (batch-outermost, C-contiguous, state/action orders of the reference
FancyVector keys, see include/vcmpc.h):

    x0[B, nx]  kappa[B, N]  ds[B, N]  ubar[B, N, nu]  xbar[B, NS, nx]  u0[B, nu]

NS = N + 1 state columns for the kinematic model (kinematic_mpc.py:59), N for the
dynamic single-track model (cascaded_mpc.py:70); vc_rollout / vc_linearize use N + 1.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .config import make_params

NX = {_abi.VC_MODEL_KINEMATIC: 6, _abi.VC_MODEL_DYNAMIC: 8, _abi.VC_MODEL_CASCADED: 8}
NU = 2
_NP_DT = {_abi.VC_F64: np.float64, _abi.VC_F32: np.float32}


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


class Context:
    """One solve context (one device, one model, one horizon, one stream).

    ``detect_infeasible`` turns the model's in-kernel infeasibility detection on at creation.  On a
    kinematic N = 20 context the params' ``qp.solver`` decides where it runs: 0 hands the solve to
    the stagewise kernel while it is on, 2 keeps the condensed kernel and tests there."""

    def __init__(self, model: int = _abi.VC_MODEL_KINEMATIC, N: int = 20, max_batch: int = 1024,
                 dtype: int = _abi.VC_F64, device: int = 0, params: _abi.vc_params | None = None,
                 detect_infeasible: bool = False, infeasible_eps: float = 0.0,
                 regularize_levels: int = 0, regularize_factor: float = 0.0, **cfgs):
        self.lib = _abi.load_library()
        self.model, self.N, self.max_batch, self.dtype, self.device = model, int(N), int(max_batch), dtype, device
        self.nx = NX[model]
        self.params = params if params is not None else make_params(**cfgs)
        # stages of the solve arrays: N + 1 states (kinematic), N (single track), or
        # H = N + horizon_pm (cascaded: kappa, ds, ubar, xbar span the point-mass tail too)
        self.NH = self.N + (int(self.params.casc.horizon_pm) if model == _abi.VC_MODEL_CASCADED else 0)
        self.ns_solve = self.N + 1 if model == _abi.VC_MODEL_KINEMATIC else self.NH
        h = self.lib.vc_create(device, model, self.N, self.max_batch, dtype, C.byref(self.params))
        if not h:
            raise _abi.VcError(_abi.VC_E_HIP, self.lib.vc_last_error(None).decode())
        self._h = C.c_void_p(h)
        self.detect_infeasible = False
        self._last = None  # (B, device or None) of the last solve: what farkas() returns
        self.regularize_levels = 0
        if regularize_levels:
            try:
                self.set_sqp_regularization(regularize_levels, regularize_factor)
            except Exception:
                self.close()
                raise
        if detect_infeasible:
            try:
                # the single-track fp64 SQP has its own entry point (vc_set_sqp_infeasibility)
                if model == _abi.VC_MODEL_DYNAMIC and dtype == _abi.VC_F64:
                    self.set_sqp_infeasibility(True, infeasible_eps)
                # ... and so has the cascaded fp64 SQP (vc_set_casc_infeasibility)
                elif model == _abi.VC_MODEL_CASCADED and dtype == _abi.VC_F64:
                    self.set_casc_infeasibility(True, infeasible_eps)
                else:
                    self.set_infeasibility(True, infeasible_eps)
            except Exception:
                self.close()
                raise

    # -- lifetime ---------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.vc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, code):
        _abi.check(self.lib, self._h, code)

    def set_stream(self, stream_handle: int | None):
        """Run on an external HIP stream (e.g. ``torch.cuda.current_stream().cuda_stream``)."""
        self._check(self.lib.vc_set_stream(self._h, C.c_void_p(stream_handle or 0)))

    def set_obstacles(self, obstacles, margin_min: float = 0.0):
        """``vc_set_obstacles``: replace the obstacle list [(s, ey, radius), ...] the
        barrier terms use (Track._construct_obstacles, track.py:131-138); [] = off."""
        rows = np.asarray([tuple(r) for r in (obstacles or [])], np.float64).reshape(-1, 3)
        cols = [np.ascontiguousarray(rows[:, i]) for i in range(3)]
        self._check(self.lib.vc_set_obstacles(self._h, len(rows), *[C.c_void_p(c.ctypes.data) for c in cols],
                                              float(margin_min)))

    def set_infeasibility(self, on: bool, eps: float = 0.0):
        """``vc_set_infeasibility``: in-kernel infeasibility detection of the kinematic kernels.
        On: a QP whose linearised rows have no feasible point ends with status
        ``VC_INFEASIBLE`` (4), proved by the Farkas vector ``farkas()`` returns; ``eps <= 0`` keeps
        the default roundoff guard 1e-9.  An N = 20 ``qp.solver = 0`` context is solved by the
        stagewise kernel while the detection is on; with ``qp.solver = 2`` it keeps the condensed
        kernel, which runs the same test (the problems it does not certify come out bit for bit
        as with the detection off).  Raises ``VcError`` (VC_E_UNSUPPORTED) on dynamic / cascaded
        contexts."""
        self._set_detection(self.lib.vc_set_infeasibility, on, eps)

    def farkas(self, B: int | None = None):
        """``vc_get_farkas``: y[B, 7N - 3] of the last solve (rows in the order of
        oracle/ltv_qp.py ``kin_qp``; zero for problems that did not end ``VC_INFEASIBLE``), a
        numpy array after a host-array solve, a torch tensor on the context's device after a
        device-tensor one.  The stagewise kernel and the condensed one (``qp.solver = 2``) write the
        same rows in the same order; the condensed one may return the row multipliers with the box
        weights that cancel C'y instead of the interior point's own (the same inequality holds).  Raises ``VcError`` when the detection is off."""
        return self._certificates(self.lib.vc_get_farkas, B, 7 * self.N - 3, False)[0]

    def set_sqp_infeasibility(self, on: bool, eps: float = 0.0):
        """``vc_set_sqp_infeasibility``: in-kernel infeasibility detection of the single-track fp64
        SQP (csrc/st_sqp.hip).  On: a problem whose first QP has no feasible point ends with status
        ``VC_INFEASIBLE`` (4); a later infeasible QP ends the SQP at the current iterate as before,
        only sooner.  Either way ``sqp_farkas()`` returns the proof.  ``eps <= 0`` keeps the default
        guard 1e-9.  Raises ``VcError``: VC_E_UNSUPPORTED on kinematic / cascaded / fp32 contexts,
        VC_E_ARG when ``trust_Fx <= 0``."""
        self._set_detection(self.lib.vc_set_sqp_infeasibility, on, eps)

    def sqp_farkas(self, B: int | None = None):
        """``vc_get_sqp_farkas``: ``(y[B, 12N - 3], qp_index[B])`` of the last solve -- rows in the
        order of oracle/dyn_sqp.py ``dyn_qp``, ``qp_index`` the SQP iteration whose QP was certified
        infeasible or -1 (``y``'s row is then zero).  Numpy arrays after a host-array solve, torch
        tensors on the context's device after a device-tensor one.  Raises ``VcError`` when the
        detection is off."""
        return self._certificates(self.lib.vc_get_sqp_farkas, B, 12 * self.N - 3, True)

    def set_sqp_regularization(self, levels: int, factor: float = 0.0):
        """``vc_set_sqp_regularization``: the regularised retry of the single-track fp64 SQP
        (csrc/st_sqp.hip).  ``levels = J`` in 1..6: a QP whose interior point breaks down is solved
        again with the proximal weight ``prox * factor**j``, j = 1..J, until a rung does not break
        down (``factor <= 0`` keeps 10); ``levels = 0`` turns it off.  ``sqp_regularization()``
        returns the level of every QP; diag[2] bit 64 marks an exhausted ladder, bit 128 a step from
        a level above 0.  Raises ``VcError``: VC_E_UNSUPPORTED on kinematic / cascaded / fp32
        contexts, VC_E_ARG for ``levels`` outside 0..6 or ``0 < factor <= 1``."""
        self._check(self.lib.vc_set_sqp_regularization(self._h, int(levels), float(factor)))
        self.regularize_levels = int(levels)
        self._last = None

    def sqp_regularization(self, B: int | None = None):
        """``vc_get_sqp_regularization``: ``level[B, sqp_iters]`` (int32) of the last solve -- per QP
        the level 0..J its answer came from, -1 where the QP was not run (the SQP had ended), -2
        where its ladder was exhausted.  A numpy array after a host-array solve, a torch tensor on
        the context's device after a device-tensor one.  Raises ``VcError`` when the feature is off."""
        last_B, dev = self._last if self._last is not None else (0, None)
        B = last_B if B is None else int(B)
        K = int(self.params.dyn_mpc.sqp_iters)
        if dev is not None:
            import torch
            out = torch.empty((B, K), dtype=torch.int32, device=dev)
            ptr, flags = C.c_void_p(out.data_ptr()), _abi.VC_DEVICE_PTRS
        else:
            out = np.empty((B, K), np.int32)
            ptr, flags = C.c_void_p(out.ctypes.data), _abi.VC_HOST_PTRS
        self._check(self.lib.vc_get_sqp_regularization(self._h, B, ptr, flags))
        return out

    def debug_sqp_breakdown(self, sqp_iter: int, problem: int = 0, levels: int = 1):
        """``vc_debug_sqp_breakdown`` (test hook): in the QP of SQP iteration ``sqp_iter`` of problem
        ``problem`` the rungs 0..levels-1 report a failed factorisation at their first
        interior-point iteration; ``sqp_iter < 0`` turns it off."""
        self._check(self.lib.vc_debug_sqp_breakdown(self._h, int(sqp_iter), int(problem), int(levels)))

    def set_casc_infeasibility(self, on: bool, eps: float = 0.0):
        """``vc_set_casc_infeasibility``: in-kernel infeasibility detection of the stagewise cascaded
        fp64 SQP (csrc/casc_ric.hip).  On: a problem whose first QP has no feasible point ends with
        status ``VC_INFEASIBLE`` (4); a later infeasible QP ends the SQP at the current iterate as
        before, only sooner.  Either way ``casc_farkas()`` returns the proof.  ``eps <= 0`` keeps the
        default guard 1e-9.  Raises ``VcError``: VC_E_UNSUPPORTED on kinematic / dynamic / fp32
        contexts, on tails the stagewise kernel is not built for and with ``qp.solver = 2``;
        VC_E_ARG when ``trust_Fx <= 0``."""
        self._set_detection(self.lib.vc_set_casc_infeasibility, on, eps)

    def casc_farkas(self, B: int | None = None):
        """``vc_get_casc_farkas``: ``(y[B, 12N - 3 + 6M], qp_index[B])`` of the last solve -- rows in
        the order of oracle/casc_sqp.py ``casc_qp`` (M = horizon_pm), ``qp_index`` the SQP iteration
        whose QP was certified infeasible or -1 (``y``'s row is then zero).  Numpy arrays after a
        host-array solve, torch tensors on the context's device after a device-tensor one.  Raises
        ``VcError`` when the detection is off."""
        return self._certificates(self.lib.vc_get_casc_farkas, B, 12 * self.N - 3 + 6 * (self.NH - self.N), True)

    def _set_detection(self, fn, on, eps):
        self._check(fn(self._h, int(bool(on)), float(eps)))
        self.detect_infeasible = bool(on)
        self._last = None

    def _certificates(self, fn, B, rows, with_index):
        """``fn`` (a ``vc_get_*_farkas``) into fresh buffers of the last solve's kind: ``(y[B, rows],)``
        or, ``with_index``, ``(y, qp_index[B])``."""
        last_B, dev = self._last if self._last is not None else (0, None)
        B = last_B if B is None else int(B)
        if dev is not None:
            import torch
            out = (torch.empty((B, rows), dtype=torch.float64, device=dev),
                   torch.empty((B,), dtype=torch.int32, device=dev))[:1 + with_index]
            ptrs, flags = [C.c_void_p(a.data_ptr()) for a in out], _abi.VC_DEVICE_PTRS
        else:
            out = (np.empty((B, rows), np.float64), np.empty((B,), np.int32))[:1 + with_index]
            ptrs, flags = [C.c_void_p(a.ctypes.data) for a in out], _abi.VC_HOST_PTRS
        self._check(fn(self._h, B, *ptrs, flags))
        return out

    def synchronize(self):
        self._check(self.lib.vc_synchronize(self._h))

    # -- argument marshalling -----------------------------------------------------
    def _marshal(self, arrays, shapes, dtypes):
        """Validate a set of buffers; all host numpy or all device torch.
        Returns (pointers, flags)."""
        dev = [_is_torch(a) for a in arrays]
        if any(dev) and not all(dev):
            raise TypeError("mix of host and device buffers in one call")
        ptrs = []
        for a, shp, dt in zip(arrays, shapes, dtypes):
            if dev[0]:
                import torch
                tdt = {np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32}[dt]
                if a.dtype != tdt or not a.is_contiguous() or tuple(a.shape) != tuple(shp):
                    raise ValueError(f"device buffer must be contiguous {tdt}{tuple(shp)}, got {a.dtype}{tuple(a.shape)}")
                if not a.is_cuda or a.device.index != self.device:
                    raise ValueError(f"device buffer must live on cuda:{self.device}")
                ptrs.append(C.c_void_p(a.data_ptr()))
            else:
                if not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous or a.shape != tuple(shp):
                    got = f"{getattr(a, 'dtype', type(a))}{getattr(a, 'shape', '')}"
                    raise ValueError(f"host buffer must be C-contiguous {np.dtype(dt)}{tuple(shp)}, got {got}")
                ptrs.append(C.c_void_p(a.ctypes.data))
        return ptrs, (_abi.VC_DEVICE_PTRS if dev[0] else _abi.VC_HOST_PTRS)

    def _batch(self, x):
        B = int(x.shape[0])
        if B > self.max_batch:
            raise ValueError(f"batch {B} > max_batch {self.max_batch}")
        return B

    # -- entry points -------------------------------------------------------------
    def solve(self, x0, kappa, ds, ubar, xbar=None, u0=None, status=None, iters=None, diag=None):
        """One MPC step (``vc_solve``: LTV-QP for the kinematic model, SQP for the
        dynamic one).  ``ubar`` is the warm start and is
        overwritten with u*; returns (u0, xbar, ubar, status, iters).  With
        ``diag=True`` (or a [B, 4] buffer) it calls ``vc_solve_diag`` and returns
        the per-problem solver diagnostics as a sixth element."""
        B, N, nx, f = self._batch(x0), self.NH, self.nx, _NP_DT[self.dtype]
        NS = self.ns_solve
        xbar, u0, status, iters = self._solve_outputs(x0, B, xbar, u0, status, iters)
        bufs = [x0, kappa, ds, xbar, ubar, u0, status, iters]
        shapes = [(B, nx), (B, N), (B, N), (B, NS, nx), (B, N, NU), (B, NU), (B,), (B,)]
        dts = [f, f, f, f, f, f, np.int32, np.int32]
        self._last = (B, x0.device if _is_torch(x0) else None)
        if diag is not None and diag is not False:
            if diag is True:
                diag = self._like(x0, (B, 4))
            # [B, 4]; timing builds (libvcmpc_timing.so) append section-cycle columns
            ptrs, flags = self._marshal(bufs + [diag], shapes + [(B, int(diag.shape[1]))], dts + [f])
            self._check(self.lib.vc_solve_diag(self._h, B, *ptrs, flags))
            return u0, xbar, ubar, status, iters, diag
        ptrs, flags = self._marshal(bufs, shapes, dts)
        self._check(self.lib.vc_solve(self._h, B, *ptrs, flags))
        return u0, xbar, ubar, status, iters

    def _solve_outputs(self, x0, B, xbar, u0, status, iters):
        """The caller's xbar, u0, status, iters, or fresh ones of x0's kind where None."""
        NS, nx, f = self.ns_solve, self.nx, _NP_DT[self.dtype]
        if xbar is None and self.model == _abi.VC_MODEL_KINEMATIC and self.params.qp.ms:
            raise ValueError("vc_qp.ms: multiple shooting linearises at the state iterate; pass xbar")
        if _is_torch(x0):
            import torch
            kw = dict(device=x0.device)
            xbar = torch.empty((B, NS, nx), dtype=x0.dtype, **kw) if xbar is None else xbar
            u0 = torch.empty((B, NU), dtype=x0.dtype, **kw) if u0 is None else u0
            status = torch.empty((B,), dtype=torch.int32, **kw) if status is None else status
            iters = torch.empty((B,), dtype=torch.int32, **kw) if iters is None else iters
        else:
            xbar = np.empty((B, NS, nx), f) if xbar is None else xbar
            u0 = np.empty((B, NU), f) if u0 is None else u0
            status = np.empty((B,), np.int32) if status is None else status
            iters = np.empty((B,), np.int32) if iters is None else iters
        return xbar, u0, status, iters

    def solve_from(self, x0, kappa, ds, ubar_in, u_out, xbar=None, u0=None, status=None, iters=None):
        """``vc_solve_from``: ``solve`` with the warm start read from ``ubar_in``, which is left
        unchanged, and u* written to ``u_out``; returns (u0, xbar, u_out, status, iters)."""
        B, N, nx, f = self._batch(x0), self.NH, self.nx, _NP_DT[self.dtype]
        NS = self.ns_solve
        xbar, u0, status, iters = self._solve_outputs(x0, B, xbar, u0, status, iters)
        bufs = [x0, kappa, ds, ubar_in, xbar, u_out, u0, status, iters]
        self._last = (B, x0.device if _is_torch(x0) else None)
        shapes = [(B, nx), (B, N), (B, N), (B, N, NU), (B, NS, nx), (B, N, NU), (B, NU), (B,), (B,)]
        dts = [f, f, f, f, f, f, f, np.int32, np.int32]
        ptrs, flags = self._marshal(bufs, shapes, dts)
        self._check(self.lib.vc_solve_from(self._h, B, *ptrs, flags))
        return u0, xbar, u_out, status, iters

    def solve_debug(self, x0, kappa, ds, ubar):
        """``vc_solve_debug`` (dynamic contexts): the solve plus a dump of the first
        QP's internals (g, normal matrix, factor storage, predictor rhs and step)."""
        B, N, nx, f = self._batch(x0), self.N, self.nx, np.float32
        stride = self.lib.vc_debug_stride()
        xbar, u0 = np.empty((B, self.ns_solve, nx), f), np.empty((B, NU), f)
        status, iters, dbg = np.empty(B, np.int32), np.empty(B, np.int32), np.empty((B, stride), f)
        ptrs, flags = self._marshal([x0, kappa, ds, xbar, ubar, u0, status, iters, dbg],
                                    [(B, nx), (B, N), (B, N), (B, self.ns_solve, nx), (B, N, NU), (B, NU), (B,),
                                     (B,), (B, stride)], [f] * 6 + [np.int32, np.int32, f])
        self._check(self.lib.vc_solve_debug(self._h, B, *ptrs, flags))
        n = 2 * N
        return dict(u0=u0, xbar=xbar, ubar=ubar, status=status, iters=iters, g=dbg[:, :n],
                    M=dbg[:, n:n + n * n].reshape(B, n, n), Y=dbg[:, n + n * n:n + 2 * n * n].reshape(B, n, n),
                    rhs=dbg[:, n + 2 * n * n:2 * n + 2 * n * n], dz=dbg[:, 2 * n + 2 * n * n:3 * n + 2 * n * n])

    def debug_kin_merit(self, x0, kappa, ds, u_prev, u, status, iters, st_acc, it_acc, first=True, restart=False,
                        x_prev=None, x=None):
        """``vc_debug_kin_merit`` (test hook, kinematic fp64): one launch of the merit line search
        of the kinematic SQP step on its own.  ``u`` (the QP's u*), ``status`` / ``iters`` (the
        QP's), ``st_acc`` / ``it_acc`` and, under ``vc_qp.ms``, ``x`` (the QP's x*) are overwritten
        with the step's; ``x_prev`` is read under ``vc_qp.ms`` only.  Returns
        (u0, x, u, status, iters, ls_diag[B, 4] = alpha, phi(u_prev), phi(accepted), D)."""
        B, N, nx, f = self._batch(x0), self.N, self.nx, np.float64
        ms = bool(self.params.qp.ms)
        if ms and (x is None or x_prev is None):
            raise ValueError("vc_qp.ms: pass the state iterate x_prev and the QP's x")
        x = self._like(x0, (B, N + 1, nx)) if x is None else x
        u0, diag = self._like(x0, (B, NU)), self._like(x0, (B, 4))
        bufs = [x0, kappa, ds, u_prev, u] + ([x_prev] if ms else []) + [x, status, iters, st_acc, it_acc, u0, diag]
        xs = [(B, N + 1, nx)]
        shapes = [(B, nx), (B, N), (B, N), (B, N, NU), (B, N, NU)] + xs * ms + xs + [(B,)] * 4 + [(B, NU), (B, 4)]
        dts = [f] * (6 + ms) + [np.int32] * 4 + [f, f]
        p, flags = self._marshal(bufs, shapes, dts)
        if not ms:
            p.insert(5, C.c_void_p(0))
        self._check(self.lib.vc_debug_kin_merit(self._h, B, *p[:11], int(bool(first)), int(bool(restart)), *p[11:],
                                                flags))
        return u0, x, u, status, iters, diag

    def debug_kin_trisolve(self, L, dinv, b):
        """``vc_debug_kin_trisolve`` (test hook, kinematic fp64, N = 20): the fused kernel's
        triangular solves (``chol_solve``) on the factor ``L[B, 2N, 2N]`` (whole rows, the entries on
        and above the diagonal as given), the inverse pivots ``dinv[B, 2N]`` and the right-hand
        sides ``b[B, 64]``.  Returns all 64 lanes of the result, ``[B, 64]``."""
        B, n, f = self._batch(L), 2 * self.N, np.float64
        out = self._like(L, (B, 64))
        ptrs, flags = self._marshal([L, dinv, b, out], [(B, n, n), (B, n), (B, 64), (B, 64)], [f] * 4)
        self._check(self.lib.vc_debug_kin_trisolve(self._h, B, *ptrs, flags))
        return out

    def rollout(self, x0, ubar, kappa, ds):
        B, N, nx, f = self._batch(x0), self.N, self.nx, _NP_DT[self.dtype]
        xbar = self._like(x0, (B, N + 1, nx))
        ptrs, flags = self._marshal([x0, ubar, kappa, ds, xbar],
                                    [(B, nx), (B, N, NU), (B, N), (B, N), (B, N + 1, nx)], [f] * 5)
        self._check(self.lib.vc_rollout(self._h, B, *ptrs, flags))
        return xbar

    def linearize(self, xbar, ubar, kappa, ds):
        B, N, nx, f = self._batch(xbar), self.N, self.nx, _NP_DT[self.dtype]
        A = self._like(xbar, (B, N, nx, nx))
        Bm = self._like(xbar, (B, N, nx, NU))
        ptrs, flags = self._marshal([xbar, ubar, kappa, ds, A, Bm],
                                    [(B, N + 1, nx), (B, N, NU), (B, N), (B, N), (B, N, nx, nx), (B, N, nx, NU)],
                                    [f] * 6)
        self._check(self.lib.vc_linearize(self._h, B, *ptrs, flags))
        return A, Bm

    def condense(self, x0, ubar, kappa, ds):
        B, N, nx, f = self._batch(x0), self.NH, self.nx, _NP_DT[self.dtype]
        n = NU * N
        H = self._like(x0, (B, n, n))
        g = self._like(x0, (B, n))
        ptrs, flags = self._marshal([x0, ubar, kappa, ds, H, g],
                                    [(B, nx), (B, N, NU), (B, N), (B, N), (B, n, n), (B, n)], [f] * 6)
        self._check(self.lib.vc_condense(self._h, B, *ptrs, flags))
        return H, g

    def plant_step(self, x, u, kappa, dt):
        B, nx, f = self._batch(x), self.nx, _NP_DT[self.dtype]
        xn = self._like(x, (B, nx))
        px, pu, pk, pxn = self._marshal([x, u, kappa, xn], [(B, nx), (B, NU), (B,), (B, nx)], [f] * 4)[0]
        flags = _abi.VC_DEVICE_PTRS if _is_torch(x) else _abi.VC_HOST_PTRS
        self._check(self.lib.vc_plant_step(self._h, B, px, pu, pk, float(dt), pxn, flags))
        return xn

    def ode(self, x, u, kappa, space=False):
        """``vc_ode``: the model's vector field f(x, u, kappa) (temporal, or spatial with
        ``space=True``) for B points."""
        B, nx, f = self._batch(x), self.nx, _NP_DT[self.dtype]
        fo = self._like(x, (B, nx))
        ptrs, flags = self._marshal([x, u, kappa, fo], [(B, nx), (B, NU), (B,), (B, nx)], [f] * 4)
        p = ptrs
        self._check(self.lib.vc_ode(self._h, B, p[0], p[1], p[2], int(bool(space)), p[3], flags))
        return fo

    def spatial_step(self, x, u, kappa, ds):
        B, nx, f = self._batch(x), self.nx, _NP_DT[self.dtype]
        xn = self._like(x, (B, nx))
        ptrs, flags = self._marshal([x, u, kappa, ds, xn], [(B, nx), (B, NU), (B,), (B,), (B, nx)], [f] * 5)
        self._check(self.lib.vc_spatial_step(self._h, B, *ptrs, flags))
        return xn

    # -- track table and closed loop ----------------------------
    def set_track(self, track):
        """Upload ``track``'s curvature table (``vc_track_set``); ``track`` is a
        ``vcmpc.environment.Track`` (or anything with ``kappa_table()``)."""
        coef, h, length = track.kappa_table()
        coef = np.ascontiguousarray(coef, np.float64)
        self._check(self.lib.vc_track_set(self._h, int(coef.shape[0]), float(h), float(length),
                                          C.c_void_p(coef.ctypes.data)))
        self.track = track

    def track_k(self, s):
        B, f = self._batch(s), _NP_DT[self.dtype]
        k = self._like(s, (B,))
        ptrs, flags = self._marshal([s, k], [(B,), (B,)], [f, f])
        self._check(self.lib.vc_track_k(self._h, B, *ptrs, flags))
        return k

    def horizon(self, x0, xbar, mpc_dt):
        """``_init_horizon`` on the device: (kappa[B, N], ds[B, N]) from the state and
        the unshifted warm start xbar[B, NS, nx]."""
        B, N, nx, f = self._batch(x0), self.NH, self.nx, _NP_DT[self.dtype]
        kappa, ds = self._like(x0, (B, N)), self._like(x0, (B, N))
        ptrs, flags = self._marshal([x0, xbar, kappa, ds], [(B, nx), (B, self.ns_solve, nx), (B, N), (B, N)], [f] * 4)
        self._check(self.lib.vc_horizon(self._h, B, ptrs[0], ptrs[1], float(mpc_dt), ptrs[2], ptrs[3], flags))
        return kappa, ds

    def drive(self, x64, u0, dt, x_ctx=None):
        """``RacingCar.drive`` for B vehicles: x64[B, nx] (fp64) is advanced in place
        with k(s) from the track table; returns x64 (and fills x_ctx if given)."""
        B, nx, f = self._batch(x64), self.nx, _NP_DT[self.dtype]
        arrs, shapes, dts = [x64, u0], [(B, nx), (B, NU)], [np.float64, f]
        if x_ctx is not None:
            arrs, shapes, dts = arrs + [x_ctx], shapes + [(B, nx)], dts + [f]
        ptrs, flags = self._marshal(arrs, shapes, dts)
        xc = ptrs[2] if x_ctx is not None else None
        self._check(self.lib.vc_drive(self._h, B, ptrs[0], ptrs[1], float(dt), xc, flags))
        return x64

    def simulate(self, x64, xbar, ubar, steps, mpc_dt, dt, log=False, nfail=None):
        """``vc_simulate``: ``steps`` closed-loop steps (horizon -> solve -> drive) on the
        device.  x64, xbar, ubar are updated in place.  With ``log=True`` returns
        (log_x[steps+1, B, nx] fp64, log_u[steps, B, nu], nfail[B]); else (None, None, nfail)."""
        B, N, nx, f = self._batch(x64), self.NH, self.nx, _NP_DT[self.dtype]
        steps = int(steps)
        dev = _is_torch(x64)
        if nfail is None:
            if dev:
                import torch
                nfail = torch.zeros((B,), dtype=torch.int32, device=x64.device)
            else:
                nfail = np.zeros((B,), np.int32)
        arrs = [x64, xbar, ubar, nfail]
        shapes = [(B, nx), (B, self.ns_solve, nx), (B, N, NU), (B,)]
        dts = [np.float64, f, f, np.int32]
        log_x = log_u = None
        if log:
            if dev:
                import torch
                log_x = torch.empty((steps + 1, B, nx), dtype=torch.float64, device=x64.device)
                log_u = torch.empty((steps, B, NU), dtype=xbar.dtype, device=x64.device)
            else:
                log_x, log_u = np.empty((steps + 1, B, nx)), np.empty((steps, B, NU), f)
            arrs, shapes, dts = arrs + [log_x, log_u], shapes + [(steps + 1, B, nx), (steps, B, NU)], dts + [np.float64, f]
        ptrs, flags = self._marshal(arrs, shapes, dts)
        lx, lu = (ptrs[4], ptrs[5]) if log else (None, None)
        self._check(self.lib.vc_simulate(self._h, B, steps, float(mpc_dt), float(dt), ptrs[0], ptrs[1], ptrs[2],
                                         lx, lu, ptrs[3], flags))
        return log_x, log_u, nfail

    def _like(self, ref, shape):
        if _is_torch(ref):
            import torch
            return torch.empty(shape, dtype=ref.dtype, device=ref.device)
        return np.empty(shape, _NP_DT[self.dtype])
