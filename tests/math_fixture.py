"""NumPy-only access to tests/golden/g_math_mp.npz (the multiprecision fixture written by golden/make_math_golden.py)
and the error measure of the device-math and oracle-math tests: ulp of the TRUE value, from its (hi, lo) pair."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_math_mp.npz")
_cache = {}


LO_UNIT = 2.0 ** -16        # *_lo is stored as an int16 count of this fraction of ulp(hi)


def lo_from_counts(hi, k):
    with np.errstate(invalid="ignore"):
        lo = k.astype(np.float64) * LO_UNIT * np.spacing(np.abs(hi))
    return np.where(np.isfinite(lo), lo, 0.0)


def load():
    """every array of the fixture; the *_lo arrays rebuilt as float64 (true value = hi + lo to 2^-17 ulp)"""
    if not _cache:
        with np.load(PATH) as z:
            _cache.update({k: z[k] for k in z.files})
        for k in [k for k in _cache if k.endswith("_lo")]:
            _cache[k + "_counts"] = _cache[k]
            _cache[k] = lo_from_counts(_cache[k[:-3] + "_hi"], _cache[k])
    return _cache


def ulp_of(scale):
    """the float64 spacing at |scale| (of the binade below it for an exact power of two is NOT taken: np.spacing)"""
    return np.spacing(np.abs(np.asarray(scale, dtype=np.float64)))


def err_ulp(val, hi, lo, scale=None):
    """|val - (hi + lo)| in ulp of `scale` (default: of the true value itself).  val - hi is exact near the truth."""
    val = np.asarray(val, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs((val - hi) - lo)
        return d / ulp_of(hi if scale is None else scale)


def norm3(hi):
    return np.sqrt((np.asarray(hi) ** 2).sum(-1, keepdims=True))


def se3_scales(g):
    """(rotation scale, translation scale) per case, as the module docstring defines them."""
    H, P, cls = g["se3_hi"], g["se3_in"], g["se3_class"]
    nw, nv = norm3(H[:, 3:6]), norm3(H[:, 0:3])
    d = norm3(P[:, 7:10] - P[:, 0:3])
    comp = (cls == 1)[:, None]
    return np.where(comp, np.maximum(nw, 1.0), nw), np.where(comp, np.maximum(nv, d), nv)


def jl_err(J, hi, lo):
    """error of a stack of A | B (18 numbers) in ulp of the largest true entry of each block"""
    out = []
    for k in (0, 9):
        s = np.abs(hi[:, k:k + 9]).max(1, keepdims=True)
        out.append(err_ulp(J[:, k:k + 9], hi[:, k:k + 9], lo[:, k:k + 9], np.broadcast_to(np.maximum(s, 1e-300), (len(hi), 9))))
    return np.concatenate(out, 1).max(1)
