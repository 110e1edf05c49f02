"""GPU: the fused kinematic kernel's triangular solves (kin_ltv.hip chol_solve), called through
vc_debug_kin_trisolve on factors built here, against an exact restatement of their operation sequence.

Lane j holds b_j and row j of L in registers, the LDS holds the columns, dj = dinv_j.

  forward, k = 0..n-1:   p = RN(acc_k dj_k), then acc_i = fma(-L[i][k], p, acc_i) for i > k
  between:               acc = RN(acc dj)                                  (y)
  backward, k = n-1..0:  x_k = RN(acc_k dj_k), then acc_i = fma(-L[k][i], x_k, acc_i) for i < k

Every fma is exact arithmetic rounded once (fractions.Fraction, float()).  The device result must be
BIT-IDENTICAL in lanes 0..n-1, the sign of a zero included, and +0 in lanes n..63.  Non-finite values are
compared by class (NaN, +inf, -inf).

Since round 13 both sweeps keep a lane's accumulator from changing after its unknown is taken
by the EXEC mask, not by zeros in the factor's storage, so every case POISONS what a finished lane could
still read: the row registers (and the LDS column slot of the diagonal) hold a mix of 1e300 and NaN on and
above the diagonal.  Neither sweep may let them act.
"""
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 20
n = 2 * N


# ---- the reference ---------------------------------------------------------------------------
def _neg(x):
    return bool(np.signbit(x))


def _round(e):
    try:
        return float(e)
    except OverflowError:
        return float("inf") if e > 0 else float("-inf")


def _fma(a, b, c):
    """fma(a, b, c), correctly rounded, with IEEE's sign of an exact zero and IEEE's non-finite classes."""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))  # the class is all that is compared
    e = Fraction(a) * Fraction(b) + Fraction(c)
    if e != 0:
        return _round(e)
    if (a == 0 or b == 0) and c == 0:  # (+-0) + (+-0): -0 only if both are
        return -0.0 if (_neg(a) != _neg(b)) and _neg(c) else 0.0
    return 0.0  # exact cancellation, round to nearest


def _mul(a, b):
    if not (np.isfinite(a) and np.isfinite(b)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b))
    e = Fraction(a) * Fraction(b)
    if e != 0:
        return _round(e)
    return -0.0 if _neg(a) != _neg(b) else 0.0


def _reference(L, dinv, b):
    """x[64]: the documented sequence on lanes 0..n-1 (only entries strictly below the diagonal are read)."""
    acc = [float(v) for v in b[:n]]
    dj = [float(v) for v in dinv]
    for k in range(n):
        p = _mul(acc[k], dj[k])
        for i in range(k + 1, n):
            acc[i] = _fma(-float(L[i, k]), p, acc[i])
    acc = [_mul(acc[i], dj[i]) for i in range(n)]
    x = np.zeros(64)
    for k in range(n - 1, -1, -1):
        x[k] = _mul(acc[k], dj[k])
        for i in range(k):
            acc[i] = _fma(-float(L[k, i]), x[k], acc[i])
    return x


# ---- the device ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from vcmpc import Context
    with Context(N=N, max_batch=4) as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check(c, L, dinv, b):
    L, dinv, b = (np.ascontiguousarray(a, np.float64) for a in (L, dinv, b))
    out = c.debug_kin_trisolve(L, dinv, b)
    assert out.shape == (len(L), 64)
    for q in range(len(L)):
        ref = _reference(L[q], dinv[q], b[q])
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(out[q]), np.isnan(ref)), (q, np.nonzero(np.isnan(out[q]) != np.isnan(ref))[0])
        inf = np.isinf(ref)
        assert np.array_equal(out[q][inf], ref[inf]), q
        bad = np.nonzero(_bits(out[q])[fin] != _bits(ref)[fin])[0]
        assert bad.size == 0, (q, np.nonzero(fin)[0][bad], out[q][fin][bad], ref[fin][bad])
    assert (_bits(out[:, n:]) == 0).all()  # lanes that own no unknown: +0


# ---- the cases -------------------------------------------------------------------------------
def _poison(L, rng):
    """1e300 and NaN, mixed, on and above the diagonal"""
    up = np.triu(np.ones((n, n), bool))
    L = L.copy()
    L[up] = np.where(rng.random(up.sum()) < 0.5, 1e300, np.nan)
    return L


def _factor(rng):
    """a well-conditioned lower-triangular factor: unit-size diagonal, small entries below it"""
    M = np.tril(rng.standard_normal((n, n)) * 0.2, -1)
    d = rng.uniform(0.5, 2.0, n)
    return M + np.diag(d), 1.0 / d


def _rhs(rng):
    return np.concatenate([rng.standard_normal(n), rng.standard_normal(64 - n)])  # lanes >= n: anything


def _random(rng):
    L, dinv = _factor(rng)
    return _poison(L, rng), dinv, _rhs(rng)


def _wide(rng):
    """entries from 1e-8 to 1e8: L = S M S^-1 with S = diag(1e-4 .. 1e4), so the solve itself stays tame"""
    M, dinv = _factor(rng)
    s = 10.0 ** rng.permutation(np.linspace(-4.0, 4.0, n))
    L = M * s[:, None] / s[None, :]
    return _poison(L, rng), dinv, _rhs(rng) * np.concatenate([s, np.ones(64 - n)])


def _nonfinite(rng):
    L, dinv, b = _random(rng)
    b[3] = np.inf
    b[17] = np.nan
    return L, dinv, b


def _zero(rng):
    L, dinv, _ = _random(rng)
    return L, dinv, np.zeros(64)


CASES = {"random": _random, "wide": _wide, "nonfinite": _nonfinite, "zero": _zero}


@pytest.mark.parametrize("B", [4, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_trisolve_bit_identical(ctx, case, B):
    rng = np.random.default_rng([sorted(CASES).index(case), B])
    L, dinv, b = (np.stack(a) for a in zip(*(CASES[case](rng) for _ in range(B))))
    _check(ctx, L, dinv, b)


def test_reference_against_numpy():
    """The reference itself (no device): it solves L L' x = b to rounding on a tame factor."""
    rng = np.random.default_rng(5)
    L, dinv = _factor(rng)
    b = _rhs(rng)
    x = _reference(_poison(L, rng), dinv, b)
    want = np.linalg.solve(L @ L.T, b[:n])
    assert np.allclose(x[:n], want, rtol=1e-9, atol=1e-12) and (_bits(x[n:]) == 0).all()
