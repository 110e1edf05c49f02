"""GPU: the fused kinematic kernel's two G products (kin_ltv.hip grow_dot, gt_dot), called through
vc_debug_kin_gdots on operands built here, against an exact reference.

Since round 12 the products run each row's / column's two parity chains in two lanes, or
one after the other in one lane, and skip the entries of G the condensing leaves structurally zero.
The reference is the 38-term form they replaced, in exact rational arithmetic: two chains, a0 over the
even indices and a1 over the odd ones, ascending, every term one fma (float() of the exact a*b + c is
its one rounding) and the first one onto +0, then a0 + a1.  The results must be BIT-IDENTICAL, the
sign of a zero included, in every lane; the lanes that own no row / column return +0.

Row r of G has stage k = r + 1 (v rows, r < N - 1) or r - N + 2 (delta rows) and is zero from column
2k on; the inputs keep to that pattern (with -0.0 as a zero where a case says so), and v is finite:
the precondition under which a skipped term fma(+-0, v, acc) is acc.
"""
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 20
n, NC = 2 * N, 2 * (N - 1)


def _stage(r):
    return r + 1 if r < N - 1 else r - (N - 1) + 1


PATTERN = np.array([[i < 2 * _stage(r) for i in range(n)] for r in range(NC)])


# ---- the reference ---------------------------------------------------------------------------
def _neg(x):
    return np.signbit(x)


def _fma(a, b, c):
    """fma(a, b, c) of finite doubles, correctly rounded, with IEEE's sign of an exact zero."""
    e = Fraction(a) * Fraction(b) + Fraction(c)
    if e != 0:
        return float(e)
    if (a == 0 or b == 0) and c == 0:  # (+-0) + (+-0): -0 only if both are
        return -0.0 if (_neg(a) != _neg(b)) and _neg(c) else 0.0
    return 0.0  # exact cancellation, round to nearest


def _add(a, b):
    e = Fraction(a) + Fraction(b)
    if e != 0:
        return float(e)
    return -0.0 if (a == 0 and b == 0 and _neg(a) and _neg(b)) else 0.0


def _dot(a, b):
    a0 = a1 = 0.0
    for i in range(0, len(a), 2):
        a0 = _fma(float(a[i]), float(b[i]), a0)
    for i in range(1, len(a), 2):
        a1 = _fma(float(a[i]), float(b[i]), a1)
    return _add(a0, a1)


def _reference(G, vz, vc):
    grow = np.zeros(64)
    gt = np.zeros(64)
    for r in range(NC):
        grow[r] = _dot(G[r, :NC], vz[:NC])  # the 38-term form reads columns 0..37
    for j in range(n):
        gt[j] = _dot(G[:, j], vc)
    return grow, gt


# ---- the device ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from vcmpc import Context
    with Context(N=N, max_batch=3) as c:
        yield c


def _device(c, G, vz, vc):
    from vcmpc import _abi
    B = len(G)
    G, vz, vc = (np.ascontiguousarray(a, np.float64) for a in (G, vz, vc))
    assert G.shape == (B, NC, n) and vz.shape == (B, n) and vc.shape == (B, NC)
    grow = np.full((B, 64), np.nan)
    gt = np.full((B, 64), np.nan)
    c._check(c.lib.vc_debug_kin_gdots(c._h, B, G.ctypes.data, vz.ctypes.data, vc.ctypes.data,
                                      grow.ctypes.data, gt.ctypes.data, _abi.VC_HOST_PTRS))
    return grow, gt


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check(c, G, vz, vc):
    grow, gt = _device(c, G, vz, vc)
    for b in range(len(G)):
        rg, rt = _reference(G[b], vz[b], vc[b])
        assert np.array_equal(_bits(grow[b]), _bits(rg)), (b, np.nonzero(_bits(grow[b]) != _bits(rg))[0])
        assert np.array_equal(_bits(gt[b]), _bits(rt)), (b, np.nonzero(_bits(gt[b]) != _bits(rt))[0])
    # lanes that own no row / column: +0 (the reference arrays hold +0 there, bits compared above)
    assert (_bits(grow[:, NC:]) == 0).all() and (_bits(gt[:, n:]) == 0).all()


# ---- the cases -------------------------------------------------------------------------------
def _pow2(count, rng):
    """distinct powers of two in a random order: every subset sum is exact and names its terms"""
    return 2.0 ** rng.permutation(count).astype(np.float64)


def _random(rng):
    return np.where(PATTERN, rng.standard_normal((NC, n)), 0.0), rng.standard_normal(n), rng.standard_normal(NC)


def _pattern_pow2(rng):
    vz = np.zeros(n)
    vz[:NC] = _pow2(NC, rng)
    return PATTERN.astype(np.float64), vz, _pow2(NC, rng)


def _huge(rng):
    G = np.where(PATTERN, rng.standard_normal((NC, n)), 0.0)
    return (G, 1e300 * rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n),
            1e300 * rng.uniform(0.5, 2.0, NC) * rng.choice([-1.0, 1.0], NC))


def _neg_zero(rng):
    G = np.where(PATTERN, rng.standard_normal((NC, n)), 0.0)
    G[rng.random((NC, n)) < 0.3] = -0.0  # inside the pattern and in the structural zeros
    G[4, :] = -0.0    # a short and a long row, a long and a short column of nothing but -0
    G[30, :] = -0.0
    G[:, 3] = -0.0
    G[:, 33] = -0.0
    vz, vc = rng.standard_normal(n), rng.standard_normal(NC)
    vz[rng.random(n) < 0.3] = -0.0
    vc[rng.random(NC) < 0.3] = -0.0
    return G, vz, vc


def _one_row(r):
    def make(rng):
        G = np.zeros((NC, n))
        G[r, PATTERN[r]] = rng.choice([-1.0, 1.0], PATTERN[r].sum()) * rng.integers(1, 8, PATTERN[r].sum())
        vz = np.zeros(n)
        vz[:NC] = _pow2(NC, rng)
        return G, vz, _pow2(NC, rng)
    return make


def _one_col(j):
    def make(rng):
        G = np.zeros((NC, n))
        G[PATTERN[:, j], j] = rng.choice([-1.0, 1.0], PATTERN[:, j].sum()) * rng.integers(1, 8, PATTERN[:, j].sum())
        vz = np.zeros(n)
        vz[:NC] = _pow2(NC, rng)
        return G, vz, _pow2(NC, rng)
    return make


CASES = {"random": _random, "pattern_pow2": _pattern_pow2, "huge": _huge, "neg_zero": _neg_zero,
         # the last short and first long row of each half, the last long and first short column
         "row8": _one_row(8), "row9": _one_row(9), "row27": _one_row(27), "row28": _one_row(28),
         "col19": _one_col(19), "col20": _one_col(20)}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_gdots_bit_identical(ctx, case, B):
    rng = np.random.default_rng([sorted(CASES).index(case), B])
    G, vz, vc = (np.stack(a) for a in zip(*(CASES[case](rng) for _ in range(B))))
    _check(ctx, G, vz, vc)


def test_reference_signs_of_zero():
    """The reference's own zero rules (no device): what IEEE round-to-nearest gives."""
    assert _bits(_fma(-0.0, 3.0, 0.0)) == 0 and _bits(_fma(-0.0, 3.0, -0.0)) == _bits(-0.0)
    assert _bits(_fma(2.0, 3.0, -6.0)) == 0 and _bits(_add(-0.0, -0.0)) == _bits(-0.0)
    assert _bits(_add(-0.0, 0.0)) == 0 and _bits(_dot([-0.0, -0.0], [1.0, 1.0])) == 0
