"""NumPy mirror of how the tree QP (csrc/gmr_ik_tree.h) forms the right-hand side of a pivoting round with fixed
variables: by the owner of each row, from the columns of the owner's local matrix alone.

Row i of H is zero outside its own limb and the trunk, so  -c_i - sum over fixed j of H_ij x_j  needs only those
columns.  The kernel sums them in a fixed order that does not depend on the bound set: the limb columns' products in
two FMA chains by column parity (even + odd), the trunk columns' likewise.  A free limb row subtracts both sums from
-c_i.  A free trunk row keeps the trunk columns' sum and receives minus each limb's sum as that limb's share, the four
shares added as (0 + 1) + (2 + 3).  `rhs_by_owner` does exactly that; `capture_rounds` replays a stream with the block
principal pivoting of tests/bpp_mirror.py (same rounds, same bound sets) and records the QP of every round.
"""
import numpy as np

import bpp_mirror


def _two_chains(h, xf):
    """sum of h[m] * xf[m] as the kernel orders it: even columns in one chain, odd columns in the other, then even + odd."""
    s = [0.0, 0.0]
    for m in range(len(h)):
        s[m & 1] += float(h[m]) * float(xf[m])
    return s[0] + s[1]


def rhs_by_owner(H, c, xfix, free, limbs, trunk):
    """(rhs, products) of the free rows (0.0 elsewhere): the right-hand side as the kernel forms it, and the sum of the
    products H_ij x_j alone, in the kernel's grouping.  xfix: the bound value of every fixed variable, 0.0 for a free one;
    limbs: four lists of dofs (empty ones allowed), trunk: list of dofs."""
    rhs = np.zeros(len(c))
    products = np.zeros(len(c))
    shares = []                                      # per limb: what it sends to every trunk row
    for limb in limbs:
        for i in limb:
            if free[i]:
                st = _two_chains(H[i, trunk], xfix[trunk])
                sl = _two_chains(H[i, limb], xfix[limb])
                rhs[i] = (-c[i] - st) - sl
                products[i] = st + sl
        shares.append({t: -_two_chains(H[t, limb], xfix[limb]) for t in trunk})
    for t in trunk:
        if free[t]:
            st = _two_chains(H[t, trunk], xfix[trunk])
            sent = (shares[0][t] + shares[1][t]) + (shares[2][t] + shares[3][t])
            rhs[t] = (-c[t] - st) + sent
            products[t] = st - sent
    return rhs, products


def bound_values(lo, hi, lower, upper):
    """(xfix, free) of the bound sets: xfix is selected, never multiplied -- lo / hi of an unlimited dof are infinite."""
    idx = np.arange(len(lo))
    at_lo = ((lower >> idx) & 1).astype(bool)
    at_up = ((upper >> idx) & 1).astype(bool)
    xfix = np.where(at_lo, lo, np.where(at_up, hi, 0.0))
    xfix[~(at_lo | at_up)] = 0.0
    return xfix, ~(at_lo | at_up)


def capture_rounds(oracle, model, ts, q0, human):
    """One stream through bpp_mirror.retarget_stream; returns (q, nsolve, rounds) with one (H, c, lo, hi, lower, upper)
    per pivoting round.  bpp_solve logs only the union of the bound sets of a round, so every solve is run by bpp_solve
    (result, number of rounds) and its bound sets are walked forward beside it with the same update; the walk must see
    bpp_solve's fixed set in every round and end in the sets bpp_solve returns."""
    rounds = []
    solve = bpp_mirror.bpp_solve

    def capturing(H, c, lo, hi, lower, upper, log=None):
        own = []
        x, lower_end, upper_end = solve(H, c, lo, hi, lower, upper, own)
        lw, up = lower, upper
        pcount, ninf_best = 3, 65
        idx = np.arange(len(c))
        dual_tol = 1e-13 * (1.0 + np.abs(c).max())
        ptol_lo, ptol_hi = 1e-12 * (1.0 + np.abs(lo)), 1e-12 * (1.0 + np.abs(hi))
        for fixed_mask, _ in own:
            assert fixed_mask == lw | up
            rounds.append((H, c, lo, hi, lw, up))
            xfix, free = bound_values(lo, hi, lw, up)
            xx = xfix.copy()
            if free.any():
                xx[free] = np.linalg.solve(H[np.ix_(free, free)], -c[free] - H[np.ix_(free, ~free)] @ xfix[~free])
            g = c + H @ xx
            at_lo = ((lw >> idx) & 1).astype(bool)
            at_up = ((up >> idx) & 1).astype(bool)
            to_lo = free & (xx < lo - ptol_lo)
            to_up = free & ~to_lo & (xx > hi + ptol_hi)
            rel = (at_lo & (g < -dual_tol)) | (at_up & ~at_lo & (g > dual_tol))
            m_lo, m_up, m_rel = (int(sum(1 << int(i) for i in idx[m])) for m in (to_lo, to_up, rel))
            every = m_lo | m_up | m_rel
            if every == 0:
                break
            total = bin(every).count("1")
            sel = every
            if total < ninf_best:
                ninf_best, pcount = total, 3
            elif pcount > 0:
                pcount -= 1
            else:
                sel = 1 << (every.bit_length() - 1)
            lw = (lw & ~(m_rel & sel)) | (m_lo & sel)
            up = (up & ~(m_rel & sel)) | (m_up & sel)
        assert (lw, up) == (lower_end, upper_end), "the replayed bound sets left bpp_solve's"
        if log is not None:
            log.extend(own)
        return x, lower_end, upper_end

    bpp_mirror.bpp_solve = capturing
    try:
        q, ns = bpp_mirror.retarget_stream(oracle, model, ts, q0, human)
    finally:
        bpp_mirror.bpp_solve = solve
    return q, ns, rounds
