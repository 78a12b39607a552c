"""Multiprecision reference for the FP64 device math (csrc/gmr_device_math.h) and the oracle's Lie-group functions.

Written from the definitions on mpmath, not from the kernel's formulas:

* the SO(3) log of a quaternion is  angle * axis  with  angle = 2 atan2(|v|, w)  folded into (-pi, pi];
* V(w) = sum_n K^n / (n + 1)!  is summed term by term and inverted by LU, so V^-1 never sees a closed form;
* Jl(e) = sum_n ad(e)^n / (n + 1)!  likewise (the series is entire: it converges for every angle), Jl^-1 by LU.

Two modes.  ``exact`` is the true function.  ``branch`` is the switch structure the reference project (mink) and
therefore the kernels follow, evaluated in multiprecision:

* ``snap``   |q.w| < 1e-10:  the angle is pi exactly, about +v if q.w > 0 and about -v otherwise (+0 and -0 included);
* ``small``  |v|^2 < 1e-10:  the two-term series  2 / w - 2 |v|^2 / (3 w^3)  of the log;
* ``ident``  |w|^2 < 1e-10:  Jl^-1 is the 6 x 6 identity.

WHICH side of a switch a case is on is decided by the caller, in float64, exactly as the kernel decides it (the grid
in tests/golden/make_math_golden.py puts its edge cases on inputs whose float64 predicate has one possible value);
this module only evaluates the chosen side.  Below t^2 = 1e-2 the kernels use Taylor series of `a` and of the Q
coefficients: those are approximations OF the exact function (truncation < 1e-19), so ``branch`` holds them to it.

Needs mpmath; only the fixture generator and the CPU freshness test import this module.
"""
import mpmath as mp

mp.mp.dps = 80
M = mp.mpf


def rcp(x):
    return 1 / M(x)


def rsqrt(x):
    return 1 / mp.sqrt(M(x))


def sin(x):
    return mp.sin(M(x))


def cos(x):
    return mp.cos(M(x))


def atan2(y, x):
    return mp.atan2(M(y), M(x))


# ---- 3-vectors and 3 x 3 matrices as plain lists ---------------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _skew(w):
    z = M(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _mv(A, v):
    return [_dot(A[i], v) for i in range(3)]


def _madd(A, B):
    return [[A[i][j] + B[i][j] for j in range(3)] for i in range(3)]


def _eye():
    return [[M(int(i == j)) for j in range(3)] for i in range(3)]


def qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def qnormalize(q):
    q = [M(c) for c in q]
    n = mp.sqrt(sum(c * c for c in q))
    return [c / n for c in q]


def qrot(q, v, inverse=False):
    """v turned by the rotation the (not necessarily unit) quaternion q stands for: q v q^-1."""
    q = [M(c) for c in q]
    v = [M(c) for c in v]
    n2 = sum(c * c for c in q)
    if inverse:
        q = [q[0], -q[1], -q[2], -q[3]]
    r = qmul(qmul(q, [M(0)] + v), [q[0], -q[1], -q[2], -q[3]])
    return [r[1] / n2, r[2] / n2, r[3] / n2]


def axis_angle(axis, angle):
    h = M(angle) / 2
    s = mp.sin(h)
    return [mp.cos(h)] + [M(a) * s for a in axis]


def so3_log(q, mode="exact", snap=False, small=False):
    """Rotation vector of the rotation q stands for.  `snap` / `small` select mink's branches (mode == 'branch')."""
    q = [M(c) for c in q]
    w, v = q[0], q[1:]
    n = mp.sqrt(_dot(v, v))
    if n == 0:
        return [M(0)] * 3
    if mode == "branch" and snap:
        f = (mp.pi if w > 0 else -mp.pi) / n
    elif mode == "branch" and small:
        f = 2 / w - 2 * n * n / (3 * w ** 3)
    else:
        ang = 2 * mp.atan2(n, w)            # [0, 2 pi]
        if ang > mp.pi:
            ang -= 2 * mp.pi                # q and -q are the same rotation: the short way round
        f = ang / n
    return [f * c for c in v]


def _phi1(K, kn):
    """sum_n K^n / (n + 1)!  for a 3 x 3 matrix of norm about kn, to working precision."""
    S, T = _eye(), _eye()
    tol = M(10) ** (-(mp.mp.dps + 5))
    for n in range(1, 400):
        T = [[c / (n + 1) for c in row] for row in _mm(T, K)]
        S = _madd(S, T)
        if n > kn and max(abs(c) for row in T for c in row) < tol:
            break
    return S


def _inv3(A):
    return (mp.matrix(A) ** -1).tolist()


def vinv(w):
    """V(w)^-1, V = sum K^n / (n + 1)!, by LU."""
    w = [M(c) for c in w]
    return _inv3(_phi1(_skew(w), float(mp.sqrt(_dot(w, w)))))


def vinv_coef(t2):
    """the coefficient a of K^2 in  V^-1 = I - K / 2 + a K^2:  (1 - (t/2) cot(t/2)) / t^2,  1/12 at t = 0."""
    t2 = M(t2)
    if t2 < M(10) ** -20:        # 1 - h cot h ~ h^2 / 3 would cancel below the working precision: its series instead
        return M(1) / 12 + t2 / 720 + t2 * t2 / 30240
    h = mp.sqrt(t2) / 2
    return (1 - h * mp.cos(h) / mp.sin(h)) / t2


def se3_log_rel(pb, qb, pt, qt, mode="exact", snap=False, small=False):
    """e = log(T_wb^-1 T_wt) = [V^-1(w) p_bt ; w]  and  t = |w|."""
    qb = [M(c) for c in qb]
    qt = [M(c) for c in qt]
    q = qmul([qb[0], -qb[1], -qb[2], -qb[3]], qt)
    pbt = qrot(qb, [M(b) - M(a) for a, b in zip(pb, pt)], inverse=True)
    w = so3_log(q, mode, snap, small)
    v = _mv(vinv(w), pbt)
    return v + w


def se3_jlinv(e, mode="exact", ident=False):
    """Jl^-1(e) = [[A, B], [0, A]] as (A, B): LU inverse of sum ad(e)^n / (n + 1)!, ad(e) = [[W, V], [0, W]]."""
    e = [M(c) for c in e]
    if mode == "branch" and ident:
        z = [[M(0)] * 3 for _ in range(3)]
        return _eye(), z
    W, V = _skew(e[3:]), _skew(e[:3])
    kn = float(mp.sqrt(_dot(e, e)))
    # powers of the block-triangular ad(e): ad^n = [[P, X], [0, P]],  ad^(n+1) = [[P W, P V + X W], [0, P W]]
    P, X = _eye(), [[M(0)] * 3 for _ in range(3)]
    SP, SX = _eye(), [[M(0)] * 3 for _ in range(3)]
    tol = M(10) ** (-(mp.mp.dps + 5))
    for n in range(1, 400):
        X = [[c / (n + 1) for c in row] for row in _madd(_mm(P, V), _mm(X, W))]
        P = [[c / (n + 1) for c in row] for row in _mm(P, W)]
        SP, SX = _madd(SP, P), _madd(SX, X)
        if n > kn and max(abs(c) for row in P + X for c in row) < tol:
            break
    J = mp.zeros(6)
    for i in range(3):
        for j in range(3):
            J[i, j] = SP[i][j]
            J[i + 3, j + 3] = SP[i][j]
            J[i, j + 3] = SX[i][j]
    Ji = (J ** -1).tolist()
    return [r[:3] for r in Ji[:3]], [r[3:] for r in Ji[:3]]


# ---- (hi, lo) double pairs: a value to ~106 bits, so that errors can be measured in ulp of the TRUE value ------
def split(x):
    x = M(x)
    hi = float(x)
    if hi != hi or hi in (float("inf"), float("-inf")):
        return hi, 0.0
    return hi, float(x - M(hi))
