"""The operator form of -Jl^-1(e) [jl; ja] (tests/jlinv_apply_mirror.py restates se3_jlinv_coef5 / se3_jlinv_apply5 of
csrc/gmr_device_math.h) against the multiprecision Jl^-1 of tests/mp_lie.py times the vector.  CPU only.

Scale and bound.  top = -(A jl + B ja), bot = -A ja.  An error is measured in ulp of  max|entry of the block| * max|vector
entry|, summed over the blocks a row multiplies: max|A| max|ja| for bot, max|A| max|jl| + max|B| max|ja| for top.  The
bound is the one tests/test_device_math.py asserts for the blocks of se3_jlinv_col5, _jl_bound(32, t) (imported), plus
8 ulp for the six-term sums: the operator form evaluates the same coefficient expressions and replaces a rounded matrix
and a rounded matrix-vector product by one rounded product.  In the identity zone (|w|^2 < 1e-10) the result is
[-jl; -ja] exactly, up to the sign of zeros.
"""
import numpy as np
import pytest

import jlinv_apply_mirror as mirror
import math_fixture as F
import mp_lie
from test_device_math import BOUND, _jl_bound

SUM_ULP = 8.0


def truth_mp(e, ident, jl, ja):
    """(hi[n, 6], lo[n, 6], scale[n, 6]) of [top; bot] = -Jl^-1(e) [jl; ja] in multiprecision (`branch` mode: the
    identity where the caller's float64 predicate says so) and the scale of each row as the module docstring defines it."""
    M = mp_lie.M
    n = len(e)
    hi, lo, scale = np.empty((n, 6)), np.empty((n, 6)), np.empty((n, 6))
    for i in range(n):
        A, B = mp_lie.se3_jlinv(e[i], "branch", bool(ident[i]))
        l, a = [M(x) for x in jl[i]], [M(x) for x in ja[i]]
        rows = [-(sum(A[r][c] * l[c] for c in range(3)) + sum(B[r][c] * a[c] for c in range(3))) for r in range(3)]
        rows += [-sum(A[r][c] * a[c] for c in range(3)) for r in range(3)]
        for r, x in enumerate(rows):
            hi[i, r], lo[i, r] = mp_lie.split(x)
        ma, mb = float(max(abs(c) for row in A for c in row)), float(max(abs(c) for row in B for c in row))
        scale[i, :3] = ma * np.abs(jl[i]).max() + mb * np.abs(ja[i]).max()
        scale[i, 3:] = ma * np.abs(ja[i]).max()
    return hi, lo, scale


def allowed(e):
    t = np.linalg.norm(e[:, 3:], axis=1)
    return _jl_bound(BOUND["se3_jlinv_col5 / zone"], t) + SUM_ULP


def check(out, e, ident, jl, ja, truth):
    """out[n, 6] = [top; bot] of an implementation; returns the largest error / allowed outside the identity zone"""
    hi, lo, scale = truth
    idz = ident == 1
    t2 = (e[:, 3:] ** 2).sum(1)
    assert idz.sum() >= 9 and ((t2 >= 1e-10) & (t2 < 1e-2)).sum() >= 60 and (t2 >= 1e-2).sum() >= 20      # all three zones
    assert np.array_equal(idz, t2 < 1e-10)
    assert np.array_equal(out[idz] + 0.0, np.concatenate([-jl[idz], -ja[idz]], 1) + 0.0)
    err = F.err_ulp(out, hi, lo, scale).max(1)
    ratio = err[~idz] / allowed(e)[~idz]
    assert not np.isnan(ratio).any()
    return float(err[~idz].max()), float(ratio.max())


@pytest.fixture(scope="module")
def inputs():
    e, aux, ident, jl, ja = mirror.cases()
    return e, aux, ident, jl, ja, truth_mp(e, ident, jl, ja)


def test_mirror_against_multiprecision(inputs):
    e, aux, ident, jl, ja, truth = inputs
    out = np.empty((len(e), 6))
    for i in range(len(e)):
        cf = mirror.coef5(e[i], aux[i])
        if ident[i] == 1:
            assert np.array_equal(cf, [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        out[i, :3], out[i, 3:] = mirror.apply5(e[i], cf, jl[i], ja[i])
    worst, ratio = check(out, e, ident, jl, ja, truth)
    print(f"mirror: max error {worst:.2f} ulp, max error / allowed {ratio:.3f}")
    assert ratio <= 1.0, (worst, ratio)


def test_magnitudes_cover_the_stated_range(inputs):
    _, _, _, jl, ja, _ = inputs
    for v in (jl, ja):
        m = np.abs(v).max(1)
        assert m.min() < 1e-2 and m.max() > 5.0
