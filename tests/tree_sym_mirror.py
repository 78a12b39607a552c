"""Mirror of ONE local elimination of the tree QP (csrc/gmr_ik_tree.h): lane i holds row i of the local matrix (limb
rows, then trunk rows), the pivots run right-looking with every column of every lane updated by a fused multiply-add,
exactly as the kernel issues them.  Two forms of the rows:

  lower   limb row a keeps its columns m <= a, trunk row t its trunk columns u <= t; the columns of the lower factor
          are what the lanes BELOW the pivot hold (the form that needed a transpose to hand lane a column a)
  full    every free row keeps all its free columns; lane p's own row, untouched after pivot p - 1, times its own
          1 / sqrt(d_p) is column p of the lower factor

The fused multiply-adds are emulated exactly (rationals, rounded once), so "equal" below means bit for bit.
"""
import math
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    """round(a * b + c), one rounding, IEEE signs of zero."""
    if a == 0.0 or b == 0.0:
        return a * b + c                                  # the product is an exact (signed) zero: the sum is exact
    e = Fraction(a) * Fraction(b) + Fraction(c)
    return 0.0 if e == 0 else float(e)                    # exact cancellation gives +0 (round to nearest); float(): correctly rounded


def spd_symmetric(rng, nv):
    """A random SPD matrix whose (i, j) and (j, i) cells hold the same bits."""
    g = rng.normal(size=(nv, nv + 3))
    m = g @ g.T + nv * np.eye(nv)
    return np.tril(m) + np.tril(m, -1).T


def _factor(rows, first, count):
    """`count` pivots starting at column / lane `first`, on every lane's row.  Returns (lower factor columns as the lanes
    below each pivot see them: col[p][lane], each lane's 1 / sqrt(d) at its own pivot)."""
    nv = len(rows)
    cols, dinv_of = [], [1.0] * nv
    for p in range(first, first + count):
        dp = rows[p][p]
        assert dp > 0.0
        dinv = 1.0 / math.sqrt(dp)                         # any function of d_p: every lane is given the same value
        dinv_of[p] = dinv
        l = [rows[i][p] * dinv if i > p else 0.0 for i in range(nv)]
        cols.append([rows[i][p] * dinv if i >= p else 0.0 for i in range(nv)])
        for i in range(nv):
            for k in range(p + 1, len(rows[i])):
                rows[i][k] = fma(-l[i], l[k], rows[i][k])
    return cols, dinv_of


def eliminate(A, nl, nt, fixed, full):
    """The local elimination of one limb (nl rows) and the trunk (nt rows) on the (nl + nt)-square matrix A.
    `fixed`: rows / columns replaced by identity (variables on a bound, padding rows).  Returns a dict:
      L_l [m][a]   column a of the limb factor below its diagonal, as lane m > a sees it at pivot a
      Y_l [u][a]   column a of Y_l, as trunk lane u sees it at pivot a
      L_t [q][t]   column t of the trunk factor below its diagonal, as trunk lane q > t sees it
      ltl, yl, lt  the same three taken from the pivot lane's own row times its own 1 / sqrt(d)   (full rows only)
    """
    nv = nl + nt
    free = [i not in fixed for i in range(nv)]
    rows = []
    for i in range(nv):
        limb = i < nl
        r = [0.0] * nv
        for m in range(nl):
            if free[i] and free[m] and (full or not limb or m <= i):
                r[m] = float(A[i, m])
            if limb and m == i and not free[i]:
                r[m] = 1.0
        if limb and full and free[i]:
            for u in range(nt):
                if free[nl + u]:
                    r[nl + u] = float(A[i, nl + u])
        rows.append(r)
    cols, dinv_l = _factor(rows, 0, nl)
    out = {"L_l": [[cols[a][m] if m > a else 0.0 for a in range(nl)] for m in range(nl)],
           "Y_l": [[cols[a][nl + u] for a in range(nl)] for u in range(nt)]}
    if full:
        out["ltl"] = [[rows[a][m] * dinv_l[a] if m > a else 0.0 for a in range(nl)] for m in range(nl)]
        out["yl"] = [[rows[a][nl + u] * dinv_l[a] for a in range(nl)] for u in range(nt)]
    # trunk: H's trunk block plus this limb's Schur part, which the trunk lanes' trunk columns have collected
    srows = [[0.0] * nv for _ in range(nv)]                # (lanes and columns keep their local numbers; limb lanes hold zeros)
    for t in range(nt):
        i = nl + t
        for u in range(nt):
            live = free[i] and free[nl + u]
            srows[i][nl + u] = float(A[i, nl + u]) + rows[i][nl + u] if live and (full or u <= t) else 0.0
            if u == t and not live:
                srows[i][nl + u] = 1.0
    tcols, dinv_t = _factor(srows, nl, nt)
    out["L_t"] = [[tcols[t][nl + q] if q > t else 0.0 for t in range(nt)] for q in range(nt)]
    if full:
        out["lt"] = [[srows[nl + t][nl + q] * dinv_t[nl + t] if q > t else 0.0 for t in range(nt)] for q in range(nt)]
    return out


def bits(x):
    """The bit patterns of a nested list of doubles, -0.0 folded onto +0.0 (a finished row adds signed zeros to its
    entries: an exact zero may change sign, nothing else can change)."""
    a = np.asarray(x, dtype=np.float64) + 0.0
    return a.view(np.uint64)
