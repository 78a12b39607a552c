"""NumPy restatement of se3_jlinv_coef5 / se3_jlinv_apply5 (csrc/gmr_device_math.h): -Jl^-1(e) applied to a body-frame
Jacobian column [jl; ja] as cross and dot products, no 3 x 3 matrix formed.  The same expressions in the same order as
the header (NumPy does not contract multiply-adds, the device does: values agree to rounding, not bit for bit).

Also the shared inputs of tests/test_jlinv_apply_host.py (CPU, against mpmath) and tests/test_jlinv_apply.py (GPU).
"""
import numpy as np

import math_fixture as F


def coef5(e, aux):
    """{a, da, c1, kw, dq, sq.x, sq.y, sq.z} of one tangent e[6]; aux = {a, sin t, cos t, t, 1 / t} as se3_log_rel5 hands over."""
    rho, w = np.asarray(e[:3], dtype=np.float64), np.asarray(e[3:], dtype=np.float64)
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if t2 < 1e-10:
        return np.array([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    a = aux[0]
    if t2 < 1e-2:
        c1 = 1.0 / 6.0 - t2 / 120.0 + t2 * t2 / 5040.0 - t2 * t2 * t2 / 362880.0
        c2 = -1.0 / 24.0 + t2 / 720.0 - t2 * t2 / 40320.0 + t2 * t2 * t2 / 3628800.0
        c3 = -1.0 / 120.0 + t2 / 5040.0 - t2 * t2 / 362880.0 + t2 * t2 * t2 / 39916800.0
    else:
        sn, cs, t, it = aux[1], aux[2], aux[3], aux[4]
        it2 = it * it
        c1 = (t - sn) * it2 * it
        c2 = (1.0 - 0.5 * t2 - cs) * it2 * it2
        c3 = (t - sn - t2 * t / 6.0) * it2 * it2 * it
    c4 = -0.5 * (c2 - 3.0 * c3)
    s = w[0] * rho[0] + w[1] * rho[1] + w[2] * rho[2]
    m = np.cross(w, np.cross(w, rho))
    k1 = (c1 + c2) * s
    sq = 0.5 * rho - k1 * w - c2 * m
    dq = -2.0 * c1 * s + 2.0 * c4 * s * t2
    kw = -2.0 * c4 * s
    da = 1.0 - a * t2
    return np.array([a, da, c1, kw, dq, sq[0], sq[1], sq[2]])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def op_a(w, hw, a, da, x):
    """A x = hw x x + (a (w . x)) w + da x"""
    return np.cross(hw, x) + (a * _dot(w, x)) * w + da * x


def op_q(w, rho, sq, c1, kw, dq, v):
    """Q v = sq x v + (c1 (w . v)) rho + (c1 (rho . v) + kw (w . v)) w + dq v"""
    wv, rv = _dot(w, v), _dot(rho, v)
    return np.cross(sq, v) + (c1 * wv) * rho + (c1 * rv + kw * wv) * w + dq * v


def apply5(e, coef, jl, ja):
    """(top, bot) = -Jl^-1(e) [jl; ja]: three applications of A and one of Q.  a == 0 marks the identity zone (a is
    1 / 12 or more everywhere else): there hw is zero as well, so that A = I and Q = 0 exactly."""
    rho, w = np.asarray(e[:3], dtype=np.float64), np.asarray(e[3:], dtype=np.float64)
    a, da, c1, kw, dq = coef[:5]
    sq = np.asarray(coef[5:8])
    hw = (-0.5 if a != 0.0 else 0.0) * w
    v1 = op_a(w, hw, a, da, ja)
    top = op_a(w, hw, a, da, op_q(w, rho, sq, c1, kw, dq, v1)) - op_a(w, hw, a, da, jl)
    return top, -v1


def aux5_of(e):
    """What se3_log_rel5 hands over for the tangent e, evaluated in float64: {a, sin t, cos t, t, 1 / t}; below
    t^2 = 1e-2 the series of `a` and the sentinels 0, 1, 0, 0, above it the closed forms from the half angle."""
    w = np.asarray(e[3:], dtype=np.float64)
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if t2 < 1e-2:
        a = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0 + t2 / 47900160.0)))
        return np.array([a, 0.0, 1.0, 0.0, 0.0])
    t = np.sqrt(t2)
    half, it = 0.5 * t, 1.0 / t
    sh, ch = np.sin(half), np.cos(half)
    return np.array([(sh - half * ch) / sh * (it * it), 2.0 * sh * ch, 1.0 - 2.0 * sh * sh, t, it])


def cases():
    """(e[n, 6], aux5[n, 5], ident[n], jl[n, 3], ja[n, 3]).  The jle_e rows of the multiprecision fixture (identity zone
    and series zone: the fixture stops at t^2 = 1e-2) and, for the closed forms, 24 seeded tangents with t from just
    above the switch to 3.1; each row with seeded random columns jl, ja of magnitudes 1e-3 ... 10."""
    g = F.load()
    rng = np.random.default_rng(17)
    t = np.concatenate([0.1 * (1.0 + np.array([1e-9, 1e-6, 1e-3])), np.geomspace(0.11, 3.1, 21)])
    d = rng.normal(size=(len(t), 3))
    w = d / np.linalg.norm(d, axis=1, keepdims=True) * t[:, None]
    rho = rng.normal(size=(len(t), 3)) * 10.0 ** rng.uniform(-2.0, 0.5, size=(len(t), 1))
    e = np.concatenate([g["jle_e"], np.concatenate([rho, w], 1)])
    ident = np.concatenate([g["jle_ident"], np.zeros(len(t), dtype=g["jle_ident"].dtype)])
    n = len(e)
    mag = 10.0 ** rng.uniform(-3.0, 1.0, size=(2, n, 1))
    v = rng.normal(size=(2, n, 3)) * mag
    return e, np.array([aux5_of(r) for r in e]), ident, v[0], v[1]
