"""NumPy mirror of the latency IK kernel's box-QP (csrc/gmr_ik_tree.h): block principal pivoting over the bound sets,
warm-started from the previous solve of the stream, inside the reference's retarget loop built from the oracle's
preprocess / stage_error / build_qp / integrate.  It computes what the kernel computes, round for round, so the rounds
of a test input can be classified on the host: which ones fix a trunk (waist) variable, which only limb variables, and
how many multipliers release a variable of either kind.

The dense solve of a round stands for the kernel's limb / trunk elimination: same system, same solution up to rounding.
"""
import numpy as np

MAX_ROUNDS = 100


def bpp_solve(H, c, lo, hi, lower, upper, log=None):
    """One QP.  lower / upper: integer bit masks of the variables on their bounds (the warm start; returned updated).
    log, if given, receives one (fixed mask, released mask) pair per pivoting round.  Returns (x, lower, upper)."""
    n = len(c)
    idx = np.arange(n)
    dual_tol = 1e-13 * (1.0 + np.abs(c).max())
    ptol_lo, ptol_hi = 1e-12 * (1.0 + np.abs(lo)), 1e-12 * (1.0 + np.abs(hi))
    pcount, ninf_best = 3, 65
    for _ in range(MAX_ROUNDS):
        at_lo = ((lower >> idx) & 1).astype(bool)
        at_up = ((upper >> idx) & 1).astype(bool)
        fixed = at_lo | at_up
        xfix = np.where(at_lo, lo, np.where(at_up, hi, 0.0))
        xfix[~fixed] = 0.0
        free = ~fixed
        x = xfix.copy()
        if free.any():
            rhs = -c[free] - H[np.ix_(free, fixed)] @ xfix[fixed]
            x[free] = np.linalg.solve(H[np.ix_(free, free)], rhs)
        g = c + H @ x
        to_lo = free & (x < lo - ptol_lo)
        to_up = free & ~to_lo & (x > hi + ptol_hi)
        rel = (at_lo & (g < -dual_tol)) | (at_up & ~at_lo & (g > dual_tol))
        m_lo, m_up, m_rel = (int(sum(1 << int(i) for i in idx[m])) for m in (to_lo, to_up, rel))
        every = m_lo | m_up | m_rel
        if every == 0:
            if log is not None:
                log.append((lower | upper, 0))
            return np.minimum(np.maximum(x, lo), hi), lower, upper
        total = bin(every).count("1")
        sel = every                                   # exchange all violating variables ...
        if total < ninf_best:
            ninf_best, pcount = total, 3
        elif pcount > 0:
            pcount -= 1
        else:
            sel = 1 << (every.bit_length() - 1)       # ... or, after three rounds without progress, the highest one only
        if log is not None:
            log.append((lower | upper, m_rel & sel))
        lower = (lower & ~(m_rel & sel)) | (m_lo & sel)
        upper = (upper & ~(m_rel & sel)) | (m_up & sel)
    raise RuntimeError("block principal pivoting did not terminate")


def retarget_stream(oracle, model, ts, q0, human, log=None):
    """One stream through the reference's loop with bpp_solve as the QP solver: (q[T, nq], nsolve[T, 2])."""
    T = human.shape[0]
    tol, max_iter = float(ts["tol"][0]), int(ts["max_iter"][0])
    q = np.array(q0, dtype=np.float64)
    lower = upper = 0
    q_out = np.empty((T, len(q)))
    ns = np.zeros((T, 2), dtype=np.int32)
    for t in range(T):
        tgt = oracle.preprocess(ts, human[t])
        for stage in range(2):
            if not int(ts["use_stage"][0][stage]):
                continue
            curr = oracle.stage_error(model, ts, stage, q, tgt)[1]
            num_iter = 0
            while True:
                H, c, lo, hi = oracle.build_qp(model, ts, stage, q, tgt)
                x, lower, upper = bpp_solve(H, c, lo, hi, lower, upper, log)
                q = oracle.integrate(model, q, x)
                nxt = oracle.stage_error(model, ts, stage, q, tgt)[1]
                ns[t, stage] += 1
                if ns[t, stage] > 1:
                    num_iter += 1
                if not (curr - nxt > tol and num_iter < max_iter):
                    break
                curr = nxt
        q_out[t] = q
    return q_out, ns


def classify_rounds(log, trunk_mask):
    """(rounds with a trunk variable fixed, rounds with only limb variables fixed, trunk releases, limb releases)."""
    n_trunk = sum(1 for fixed, _ in log if fixed & trunk_mask)
    n_limb = sum(1 for fixed, _ in log if fixed and not fixed & trunk_mask)
    rel_trunk = sum(bin(rel & trunk_mask).count("1") for _, rel in log)
    rel_limb = sum(bin(rel & ~trunk_mask).count("1") for _, rel in log)
    return n_trunk, n_limb, rel_trunk, rel_limb
