"""Writes tests/golden/g_math_mp.npz: the deterministic input grid of the device-math tests and, for every input, the
value of the multiprecision reference (tests/mp_lie.py) as a (hi, lo) pair: hi the nearest double, lo the rest of the true
value as an int16 count of 2^-16 ulp(hi) -- the truth to 2^-17 ulp at 10 bytes a number (tests/math_fixture.py rebuilds lo).

    python tests/golden/make_math_golden.py            # rewrite the fixture (needs mpmath)

Inputs are stored as the exact float64 the kernels are fed.  `*_flag` arrays say on which side of mink's switches a
case lies, decided here in float64 on inputs whose predicate has one possible value (edge cases are single-axis, with
an identity base orientation, so that no rounding or FMA contraction of the kernel can move them across):

    so3_flag / se3_flag   bit 0: pi snap (|q.w| < 1e-10)   bit 1: small series (|v|^2 < 1e-10)
    se3_ident / jle_ident 0: Jl^-1 is the full expression   1: identity (|w|^2 < 1e-10)   2: on the switch, either
    se3_class             0: direct (identity base, p_b = 0)   1: composed (random base pose)   2: off unit length

tests/test_oracle_math_mp.py re-evaluates a sample with mpmath and fails if the committed file is stale.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "g_math_mp.npz")

PI = np.pi
TAN_PI_8 = 0.41421356237309503          # the literal of atan2_q1's second reduction
ANGLES = ([0.0] + [10.0 ** k for k in range(-12, -2)] + [0.1 - 1e-9, 0.1, 0.1 + 1e-9, 0.5, 1.0, PI / 2, 2.0, 3.0,
          PI - 1e-3, PI - 1e-6, PI - 1e-9, PI - 1e-11, PI])
SINCOS_DOMAIN = 320.0                   # "a few hundred"


def ulps(x, ks):
    """x moved by k float64 steps for every k of ks."""
    out = []
    for k in ks:
        y = np.float64(x)
        for _ in range(abs(k)):
            y = np.nextafter(y, np.inf if k > 0 else -np.inf)
        out.append(y)
    return out


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _qnorm(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def _quat(axis, ang):
    return _qnorm(np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * np.asarray(axis)]))


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _sq_edge(target):
    """single-axis lengths x whose float64 square lies just below, (as near as possible) at and just above target."""
    x0 = np.sqrt(np.float64(target))
    return [x for x in ulps(x0, range(-3, 4))]


def _so3_flags(q):
    n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if n2 < 1e-10:
        return 2
    return 1 if abs(q[0]) < 1e-10 else 0


def _edge_quats(rng):
    """unit-length-ish quaternions on and next to every switch of the SO(3) log (single axis where a sum would round)."""
    out = []
    for x in _sq_edge(1e-10):                                   # |v|^2 = 1e-10, both hemispheres
        for s in (1.0, -1.0):
            out.append([s * np.sqrt(1.0 - x * x), x, 0.0, 0.0])
            out.append([s * np.sqrt(1.0 - x * x), 0.0, 0.0, -x])
    v = _unit(rng, 1)
    for w in ulps(1e-10, range(-2, 3)) + [0.0, 1e-11, 5e-11, 2e-10, 1e-9]:   # |q.w| = 1e-10, +0 / -0, -+1e-11
        for s in (1.0, -1.0):
            for a in v:
                out.append([s * w, a[0], a[1], a[2]])
            out.append([s * w, 0.0, 1.0, 0.0])
    return np.array(out, dtype=np.float64)


def grid():
    """Every input array of the fixture (float64) and the switch flags.  Deterministic."""
    rng = np.random.default_rng(20240707)
    g = {}
    # ---- fast_rcp / fast_rsqrt: powers of two, 1 -+ ulp, pivots of H (1e-8 .. 1e8), squared norms (1e-10 .. 1)
    x = [2.0 ** k for k in range(-200, 201, 16)] + [2.0 ** k for k in range(-30, 31, 2)] + ulps(1.0, range(-4, 5)) + ulps(2.0, range(-2, 3)) \
        + ulps(4.0, range(-2, 3)) + ulps(1e-10, range(-2, 3)) + [3.0, 1.0 / 3.0, 0.1, 10.0]
    x += list(10.0 ** rng.uniform(-8, 8, 400)) + list(10.0 ** rng.uniform(-10, 0, 250)) + list(rng.uniform(0.5, 2.0, 250))
    g["rr_x"] = np.array(x, dtype=np.float64)
    g["rr_special"] = np.array([np.nan, 0.0, -0.0, -1.0, -1e-300, -np.inf], dtype=np.float64)
    # ---- sincos_small: multiples of pi/4 -+ ulps (the even ones are the doubles closest to multiples of pi/2), joint / half angles
    x = []
    for k in range(-int(SINCOS_DOMAIN / (PI / 4)), int(SINCOS_DOMAIN / (PI / 4)) + 1):
        # every multiple; its neighbours at the multiples of pi/2 (where the reduced argument nearly cancels); further out now and then
        x += ulps(k * (PI / 4), range(-3, 4) if k % 16 == 0 else range(-1, 2) if k % 2 == 0 else [0])
    x += list(rng.uniform(-PI, PI, 500)) + list(rng.uniform(-SINCOS_DOMAIN, SINCOS_DOMAIN, 400))
    x += list(rng.choice([-1.0, 1.0], 60) * 10.0 ** rng.uniform(-300, 0, 60)) + [0.0, -0.0, 5e-324, 1e-310]
    g["sc_x"] = np.array(x, dtype=np.float64)
    # ---- atan2_q1(y, x), y, x >= 0: the two switches a = tan(pi/8) b and a = b at and around the value, a = 0, random
    yx = []
    for b in [1.0, 0.75, 3.0, 1e-5, 0.9999999] + list(rng.uniform(0.0, 1.0, 5)):
        for a in ulps(TAN_PI_8 * b, range(-2, 3)) + ulps(b, range(-2, 3)) + [0.0, 5e-324, 1e-300 * b, 1e-17 * b]:
            yx += [[a, b], [b, a]]
    r = rng.uniform(0.0, 1.0, (400, 2))
    yx += list(r) + [[p[0] * 10.0 ** s, p[1]] for p, s in zip(rng.uniform(0.1, 1.0, (300, 2)), rng.uniform(-12, 0, 300))]
    h = rng.uniform(0.0, PI / 2, 500)
    yx += list(np.stack([np.sin(h), np.cos(h)], 1))                       # (sin h, cos h) as se3_log_rel5 feeds it
    yx += [[1.0, v] for v in ulps(1e-10, range(-1, 2))] + [[np.sin(t / 2), np.cos(t / 2)] for t in ANGLES[1:]]
    # the worst inputs found so far (2.2 .. 2.5 ulp on an MI355X), all just above the tan(pi/8) switch
    yx += [[float.fromhex(a), float.fromhex(b)] for a, b in (
        ("0x1.f0187723ff451p-6", "0x1.2b6b8fbe20ee0p-4"), ("0x1.d8f56b017da45p-4", "0x1.1d74afa7b9e2cp-2"),
        ("0x1.8af57b6a042bfp-2", "0x1.d86217c10bd87p-1"), ("0x1.9afe0bdad2567p-2", "0x1.d4f3882725825p-1"),
        ("0x1.9cc9a0cf64b8dp-2", "0x1.d48e9301b3696p-1"))]
    g["at_yx"] = np.array(yx, dtype=np.float64)
    # ---- so3_log: angle list x axes x {q, -q}, float64-normalised, the edge quaternions, random
    axes = np.concatenate([_unit(rng, 2), np.eye(3)[:2]])
    q = [s * _quat(a, t) for t in ANGLES for a in axes for s in (1.0, -1.0)]
    q += list(_edge_quats(rng)) + list(_qnorm(rng.normal(size=(250, 4))))
    q += [s * _quat(a, t) for t, a in zip(10.0 ** rng.uniform(-12, 0, 100), _unit(rng, 100)) for s in (1.0, -1.0)]
    g["so3_q"] = np.array(q, dtype=np.float64)
    g["so3_flag"] = np.array([_so3_flags(c) for c in g["so3_q"]], dtype=np.int8)
    # ---- se3_log / Jl^-1 from poses
    poses, cls, flag, ident = [], [], [], []
    ID = np.array([1.0, 0.0, 0.0, 0.0])

    def add(pb, qb, pt, qt, c):
        qr = qt if c != 1 else _qmul(qb * [1, -1, -1, -1], qt)
        f = _so3_flags(qr)
        n = np.sqrt(qr[1] ** 2 + qr[2] ** 2 + qr[3] ** 2)
        t = PI if f & 1 else 2.0 * np.arctan2(n, abs(qr[0]))
        poses.append(np.concatenate([pb, qb, pt, qt]))
        cls.append(c)
        flag.append(f)
        ident.append(2 if abs(t * t - 1e-10) < 1e-15 else int(t * t < 1e-10))

    tlen = [1e-6, 1e-3, 0.05, 0.7, 10.0]
    for i, t in enumerate(ANGLES):
        for j, a in enumerate(axes[[0, 2]]):
            for s in (1.0, -1.0):
                p = _unit(rng, 1)[0] * tlen[(i + j) % 5]
                add(np.zeros(3), ID, p, s * _quat(a, t), 0)
                if t != PI and j == 0:          # composed at exactly pi: the sign of q.w is rounding noise
                    qb = _qnorm(rng.normal(size=4))
                    pb = rng.normal(size=3)
                    add(pb, qb, pb + _unit(rng, 1)[0] * tlen[(i + j + 2) % 5], _qnorm(_qmul(qb, s * _quat(a, t))), 1)
    for qe in _edge_quats(rng):
        add(np.zeros(3), ID, _unit(rng, 1)[0] * 0.3, qe, 0)
    for x in _sq_edge(1e-2 / 4):                 # |w|^2 = 1e-2 from the quaternion side: sin(h) about h = 0.05
        add(np.zeros(3), ID, np.array([0.2, -0.1, 0.4]), _qnorm([np.cos(np.arcsin(x)), 0.0, x, 0.0]), 0)
    for _ in range(60):
        qb, pb = _qnorm(rng.normal(size=4)), rng.normal(size=3)
        add(pb, qb, pb + rng.normal(size=3) * 10.0 ** rng.uniform(-3, 0.5), _qnorm(rng.normal(size=4)), 1)
    for t, a in zip(10.0 ** rng.uniform(-4.5, 0.4, 60), _unit(rng, 60)):     # residual sizes the solver really sees
        qb, pb = _qnorm(rng.normal(size=4)), rng.normal(size=3)
        add(pb, qb, pb + rng.normal(size=3) * 0.1, _qnorm(_qmul(qb, _quat(a, t))), 1)
    for scale in (1.0 + 1e-15, 1.0 - 1e-15):    # off unit length: by 1e-15, and float32-normalised (6e-8)
        for t in (1e-3, 0.5, 2.0, PI - 1e-3):
            add(np.zeros(3), ID, np.array([0.3, 0.1, -0.2]), scale * _quat(axes[0], t), 2)
    for t in (1e-3, 0.5, 2.0, PI - 1e-3):
        q32 = _quat(axes[1], t).astype(np.float32)
        q32 = (q32 / np.sqrt((q32 * q32).sum(dtype=np.float32))).astype(np.float64)
        add(np.zeros(3), ID, np.array([0.3, 0.1, -0.2]), q32, 2)
    g["se3_in"] = np.array(poses, dtype=np.float64)
    g["se3_class"] = np.array(cls, dtype=np.int8)
    g["se3_flag"] = np.array(flag, dtype=np.int8)
    g["se3_ident"] = np.array(ident, dtype=np.int8)
    # ---- Jl^-1 at given tangents with |w|^2 < 1e-2: the identity switch at |w|^2 = 1e-10 and the series region
    e = []
    for x in _sq_edge(1e-10) + _sq_edge(1e-2)[:3] + [1e-12, 1e-8, 3e-6, 1e-4, 1e-3, 0.03, 0.09]:
        for k in range(3):
            w = np.zeros(3)
            w[k] = x if k != 1 else -x
            e.append(np.concatenate([_unit(rng, 1)[0] * tlen[(k + len(e)) % 5], w]))
    for t, a in zip(10.0 ** rng.uniform(-4.9, -1.01, 40), _unit(rng, 40)):
        e.append(np.concatenate([rng.normal(size=3) * 10.0 ** rng.uniform(-3, 0.5), t * a]))
    g["jle_e"] = np.array(e, dtype=np.float64)
    t2 = (g["jle_e"][:, 3:] ** 2).sum(1)
    g["jle_ident"] = (t2 < 1e-10).astype(np.int8)
    # ---- vinv_coef / vinv_coef_sc: both switches of t^2 at and around the value, the cancellation zone, up to pi^2
    t2 = ulps(1e-2, range(-2, 3)) + ulps(1e-10, range(-2, 3)) + [0.0, 1e-300, 1e-24, 1e-16, 1e-6, 9.9e-3, 1.01e-2, PI * PI, np.nextafter(PI * PI, 0)]
    t2 += [t * t for t in ANGLES] + list(10.0 ** rng.uniform(-12, -2, 150)) + list(10.0 ** rng.uniform(-2, np.log10(PI * PI), 500))
    g["vc_t2"] = np.array(t2, dtype=np.float64)
    # ---- quaternion helpers: qa[4] qb[4] v[3] axis[3] angle
    n = 120
    qa = rng.normal(size=(n, 4)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    g["qt_in"] = np.concatenate([qa, _qnorm(rng.normal(size=(n, 4))), rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-6, 1, (n, 1)),
                                 _unit(rng, n), rng.uniform(-2 * PI, 2 * PI, (n, 1))], axis=1)
    return g


# ---- the reference on rows of each family: lists of multiprecision numbers, one list per row -------------------
def ref_rr(x):
    import mp_lie as L
    return [[L.rcp(v), L.rsqrt(v)] for v in x]


def ref_sc(x):
    import mp_lie as L
    return [[L.sin(v), L.cos(v)] for v in x]


def ref_at(yx):
    import mp_lie as L
    return [[L.atan2(y, x)] for y, x in yx]


def ref_so3(q, flag):
    import mp_lie as L
    return [L.so3_log(c, "branch", bool(f & 1), bool(f & 2)) + L.so3_log(c, "exact") for c, f in zip(q, flag)]


def ref_se3(poses, flag, ident):
    """per row: e[6], a, sin t, cos t, t, 1/t, A[9], B[9] of the branch mode: 29 numbers"""
    import mp_lie as L
    out = []
    for p, f, idn in zip(poses, flag, ident):
        e = L.se3_log_rel(p[0:3], p[3:7], p[7:10], p[10:14], "branch", bool(f & 1), bool(f & 2))
        t2 = e[3] * e[3] + e[4] * e[4] + e[5] * e[5]
        t = L.mp.sqrt(t2)
        A, B = L.se3_jlinv(e, "branch", idn == 1)
        out.append(e + [L.vinv_coef(t2), L.mp.sin(t), L.mp.cos(t), t, (1 / t if t != 0 else L.M(0))] + sum(A, []) + sum(B, []))
    return out


def ref_jle(e, ident):
    import mp_lie as L
    out = []
    for r, idn in zip(e, ident):
        A, B = L.se3_jlinv(r, "branch", idn == 1)
        out.append(sum(A, []) + sum(B, []))
    return out


def ref_vc(t2):
    import mp_lie as L
    return [[L.vinv_coef(v), L.mp.sin(L.mp.sqrt(L.M(v))), L.mp.cos(L.mp.sqrt(L.M(v)))] for v in t2]


def ref_qt(rows):
    import mp_lie as L
    out = []
    for r in rows:
        qn = L.qnormalize(r[0:4])
        out.append(qn + L.qrot(qn, r[8:11]) + L.qrot(qn, r[8:11], inverse=True) + L.qmul([L.M(c) for c in r[0:4]], [L.M(c) for c in r[4:8]])
                   + L.axis_angle(r[11:14], r[14]))
    return out


# family -> (reference function, names of its input arrays); the expectation is stored as <family>_hi / <family>_lo
FAMILIES = {"rr": (ref_rr, ["rr_x"]), "sc": (ref_sc, ["sc_x"]), "at": (ref_at, ["at_yx"]), "so3": (ref_so3, ["so3_q", "so3_flag"]),
            "se3": (ref_se3, ["se3_in", "se3_flag", "se3_ident"]), "jle": (ref_jle, ["jle_e", "jle_ident"]), "vc": (ref_vc, ["vc_t2"]),
            "qt": (ref_qt, ["qt_in"])}


LO_UNIT = 2.0 ** -16        # `lo` is stored as an int16 count of this fraction of ulp(hi): the truth to 2^-17 ulp in 2 bytes


def hilo(rows):
    """true values -> (hi float64, lo int16): hi the nearest double, lo = (true - hi) / (LO_UNIT ulp(hi)) rounded"""
    import mp_lie as L
    pairs = [[L.split(v) for v in r] for r in rows]
    hi = np.array([[p[0] for p in r] for r in pairs], dtype=np.float64)
    lo = np.array([[p[1] for p in r] for r in pairs], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        k = np.rint(lo / (np.spacing(np.abs(hi)) * LO_UNIT))
    return hi, np.clip(np.where(np.isfinite(k), k, 0.0), -32767, 32767).astype(np.int16)


def expect(g, fam, idx=None):
    fn, names = FAMILIES[fam]
    args = [g[n] if idx is None else g[n][idx] for n in names]
    return hilo(fn(*args))


def main():
    g = grid()
    for fam in FAMILIES:
        g[fam + "_hi"], g[fam + "_lo"] = expect(g, fam)
        print(fam, g[fam + "_hi"].shape, flush=True)
    np.savez_compressed(OUT, **g)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
