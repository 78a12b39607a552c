"""The CPU oracle's Lie-group functions against the multiprecision fixture (tests/golden/g_math_mp.npz), in ulp of the
true value, on the same grid the device-math tests use -- this is what makes "kernel == oracle at 1e-9" mean something:
the oracle is held to an independent reference first.  Also: the committed fixture is what its generator produces.

Which mode the oracle is held to (tests/mp_lie.py): `branch` everywhere.  It differs from `exact` only inside the pi
snap (|q.w| < 1e-10: by at most 2e-10 rad as a rotation) and where Jl^-1 is replaced by the identity (|w|^2 < 1e-10:
by |w| / 2 <= 5e-6 in A); the series below their switches are approximations of the exact function.

Every bound is twice the maximum observed on this grid, rounded up.  The scale of an error is the norm of the true
3-vector (rotation part |w|, translation part |v|) for `direct` cases; `composed` cases form q_b^-1 q_t and
R_b^T (p_t - p_b) in float64 first, which costs an ABSOLUTE 1e-16 whatever the angle, so there the scale is
max(|w|, 1) and max(|v|, |p_t - p_b|).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import math_fixture as F   # noqa: E402

SO3_ULP = 5          # observed 2.02
E_ROT_ULP = {0: 3, 1: 8}      # observed 1.25 (direct), 3.0 (composed)
E_TRA_ULP = {0: 6, 1: 12}     # observed 2.6, 5.1
JL_ULP_SERIES, JL_ULP_MAIN, JL_ZONE_K = 6, 15, 22      # of the largest entry of the block; observed 2.7, 7.2, 10.6 / t


def _jl_bound(t):
    """Just above t = 0.1 the closed forms (t - sin t - t^3 / 6) / t^5 and (1 - t^2 / 2 - cos t) / t^4 of Q's coefficients
    round sin t and cos t to eps / 2 and divide by t^4: relative to |B| ~ |rho| / 2 that is ~ eps / t (106 ulp observed
    at the switch).  The same formulas, hence the same zone, as in the kernels (tests/test_device_math.py)."""
    with np.errstate(divide="ignore"):
        return np.where(t >= 0.1 * (1 - 1e-12), np.maximum(JL_ULP_MAIN, JL_ZONE_K / t), JL_ULP_SERIES)


def _rot(q):
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_so3_log_against_multiprecision(oracle):
    g = F.load()
    hi, lo = g["so3_hi"][:, :3], g["so3_lo"][:, :3]
    w = np.array([oracle.so3_log(q) for q in g["so3_q"]])
    err = F.err_ulp(w, hi, lo, np.broadcast_to(F.norm3(hi), hi.shape))
    for name, m in (("main", g["so3_flag"] == 0), ("pi snap", g["so3_flag"] == 1), ("small series", g["so3_flag"] == 2)):
        assert m.sum() >= 30, name
        assert np.nanmax(err[m]) <= SO3_ULP, (name, np.nanmax(err[m]))
    assert np.array_equal(w[np.all(hi == 0, axis=1)], hi[np.all(hi == 0, axis=1)])      # angle 0: exactly 0


def test_branch_mode_is_close_to_exact():
    """How far mink's switches move the result from the true log: nothing outside the pi snap, <= 2e-10 rad inside
    (as a rotation: +pi about v and -pi about v are the same turn, so the distance is taken modulo 2 pi)."""
    g = F.load()
    b, e, fl = g["so3_hi"][:, :3], g["so3_hi"][:, 3:], g["so3_flag"]
    d = np.linalg.norm(b - e, axis=1)
    d = np.minimum(d, np.abs(d - 2 * np.pi))
    assert d[fl == 0].max() == 0.0
    assert d[fl == 2].max() <= 1e-25          # truncation of the two-term series, |v|^4 / 5
    assert 1e-11 < d[fl == 1].max() <= 2.0001e-10


def test_se3_log_rel_against_multiprecision(oracle):
    g = F.load()
    P, H, Lo, cls = g["se3_in"], g["se3_hi"], g["se3_lo"], g["se3_class"]
    E = np.array([oracle.se3_log_rel(p[:3], p[3:7], _rot(p[3:7]), p[7:10], p[10:14]) for p in P])
    sr, sv = F.se3_scales(g)
    er = F.err_ulp(E[:, 3:], H[:, 3:6], Lo[:, 3:6], np.broadcast_to(sr, (len(P), 3)))
    ev = F.err_ulp(E[:, :3], H[:, 0:3], Lo[:, 0:3], np.broadcast_to(sv, (len(P), 3)))
    for c in (0, 1):
        m = cls == c
        assert m.sum() > 150
        assert np.nanmax(er[m]) <= E_ROT_ULP[c], (c, np.nanmax(er[m]))
        assert np.nanmax(ev[m]) <= E_TRA_ULP[c], (c, np.nanmax(ev[m]))


def test_se3_jlinv_against_multiprecision(oracle):
    """Jl^-1 at the TRUE tangent (rounded to float64): the LU inverse of sum ad(e)^n / (n + 1)!."""
    g = F.load()
    for e, hi, lo, ident in ((g["se3_hi"][:, :6], g["se3_hi"][:, 11:29], g["se3_lo"][:, 11:29], g["se3_ident"]),
                             (g["jle_e"], g["jle_hi"], g["jle_lo"], g["jle_ident"])):
        t = np.linalg.norm(e[:, 3:], axis=1)
        J = np.array([oracle.se3_jlinv(r) for r in e])
        J = np.concatenate([J[:, :3, :3].reshape(-1, 9), J[:, :3, 3:].reshape(-1, 9)], 1)
        err = F.jl_err(J, hi, lo)
        ok = ident != 2                       # on the |w|^2 = 1e-10 switch either side is right
        assert ok.sum() >= 90 and (ident == 1).sum() >= 9
        assert (err[ok] <= _jl_bound(t[ok])).all(), (err[ok] / _jl_bound(t[ok])).max()
        eye = np.concatenate([np.eye(3).ravel(), np.zeros(9)])
        assert np.array_equal(J[ident == 1], np.broadcast_to(eye, J[ident == 1].shape))


def test_fixture_is_current():
    """The committed fixture is what golden/make_math_golden.py writes: same grid, and a sample of every family
    re-evaluated with mpmath gives the stored (hi, lo) pairs (lo: an int16 count of 2^-16 ulp)."""
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_math_golden as mk
    g = F.load()
    assert os.path.getsize(F.PATH) < 4e5
    fresh = mk.grid()
    for k, v in fresh.items():
        assert g[k].shape == v.shape and g[k].dtype == v.dtype, k
        assert np.allclose(g[k], v, rtol=1e-12, atol=0, equal_nan=True), k      # (libm may differ in the last bit of an input)
    rng = np.random.default_rng(1)
    for fam, (_, names) in mk.FAMILIES.items():
        n = len(g[names[0]])
        idx = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 40 if fam in ("se3", "jle") else 200)]))
        hi, lo = mk.expect(g, fam, idx)
        assert np.array_equal(hi, g[fam + "_hi"][idx], equal_nan=True), fam
        assert np.abs(lo.astype(np.int32) - g[fam + "_lo_counts"][idx]).max() <= 1, fam
