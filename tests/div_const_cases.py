"""Inputs and host mirror of div_const (csrc/gmr_device_math.h): x / c for a literal c as q = x rc, r = fma(-q, c, x),
fma(r, rc, q).  Shared by tests/test_div_const.py (host, exact) and tests/test_row_bcast_fma.py (device).

Two engines for the fused multiply-add: `fma_exact` (rationals, rounded once) and `fma_np` (vectorised: an error-free
product and sum, the two error terms added with rounding to odd, one final rounding to nearest -- Boldo and Melquiond,
"Emulation of a FMA and correctly rounded sums: proved algorithms using rounding to odd", 2008; exact while neither the
splitting overflows nor the product's low part underflows, which the ranges below keep far away).
"""
from fractions import Fraction

import numpy as np

# every literal the series and closed forms of gmr_device_math.h divide a variable by
LITERALS = [6.0, 120.0, 720.0, 5040.0, 40320.0, 362880.0, 3628800.0, 39916800.0, 47900160.0]

N_RANDOM = 1 << 20
N_MIDPOINT = 15000


def fma_exact(a, b, c):
    """round(a * b + c), one rounding (finite operands, result not an exact zero of interest for its sign)."""
    e = Fraction(a) * Fraction(b) + Fraction(c)
    return 0.0 if e == 0 else float(e)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = 134217729.0 * a                                    # 2^27 + 1
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma_np(a, b, c):
    a, b, c = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    s, e = _two_sum(tl, ul)
    # round tl + ul to odd: where the sum was inexact and its last bit is even, step to the neighbour on the error's side
    bits = s.view(np.int64)
    fix = (e != 0.0) & ((bits & 1) == 0)
    v = np.where(fix, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
    return th + v


def div_const_np(x, c):
    rc = 1.0 / c
    q = x * rc
    r = fma_np(-q, c, x)
    return fma_np(r, rc, q)


def div_const_exact(x, c):
    rc = 1.0 / c
    q = x * rc
    r = fma_exact(-q, c, x)
    return fma_exact(r, rc, q)


def random_numerators():
    """2^20 normal-range numerators: signs mixed, binary exponents -110 .. +5 (t^2 in [0, 1e-2] and its powers)."""
    rng = np.random.default_rng(20)
    mant = 1.0 + rng.random(N_RANDOM)
    x = np.ldexp(mant, rng.integers(-110, 6, size=N_RANDOM))
    x = np.where(rng.random(N_RANDOM) < 0.5, -x, x)
    x.setflags(write=False)
    return x


def midpoint_numerators(c):
    """For 15 000 random odd m = 2 k + 1, k in [2^52, 2^53) -- the quotient's rounding midpoints, in half ulps -- the three
    53-bit integers nearest c m / 2^t (t puts them into [2^52, 2^53]); signs mixed.  45 000 numerators whose quotients
    are as close to a midpoint as a 53-bit numerator allows."""
    ci = int(c)
    assert float(ci) == c
    rng = np.random.default_rng(ci % (1 << 31))
    ks = rng.integers(1 << 52, 1 << 53, size=N_MIDPOINT, dtype=np.int64)
    sign = rng.random(3 * N_MIDPOINT) < 0.5
    out = np.empty(3 * N_MIDPOINT)
    for i, k in enumerate(ks.tolist()):
        p = ci * (2 * k + 1)
        t = p.bit_length() - 53
        n0 = (p + (1 << (t - 1))) >> t                    # nearest integer to p / 2^t
        for j, n in enumerate((n0 - 1, n0, n0 + 1)):
            n = min(n, 1 << 53)                           # (the one integer above that a double cannot hold)
            assert n >= (1 << 52) - 1 and int(float(n)) == n
            out[3 * i + j] = float(n)
    out = np.where(sign, -out, out)
    out.setflags(write=False)
    return out
