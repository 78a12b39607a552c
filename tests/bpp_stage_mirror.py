"""NumPy mirror of the latency IK kernel's retarget loop with the per-stage start of the QP's bound sets (StageStart,
csrc/gmr_ik.hip): the loop of bpp_mirror.retarget_stream around the same bpp_solve, except that a frame's first solve of
stage s starts from the sets that the first solve of stage s ended with in the previous frame; every other solve
carries on from its predecessor, and a stream starts with nothing remembered.  tests/bpp_mirror.py stays the mirror of
the carried start (-DGMR_QP_CARRIED_START).

A round computes x from (H, c, sets) alone and both starts end at the same sets, so q equals the carried mirror's bit
for bit; only the number of pivoting rounds differs.
"""
import numpy as np

from bpp_mirror import bpp_solve


def retarget_stream(oracle, model, ts, q0, human, log=None, stats=None):
    """One stream: (q[T, nq], nsolve[T, 2]).  log: as in bpp_solve (one entry per pivoting round).  stats, if given (a
    dict), counts `restores` (first solves that had a remembered set) and `replaced` (... that differed from the carried
    one)."""
    T = human.shape[0]
    tol, max_iter = float(ts["tol"][0]), int(ts["max_iter"][0])
    q = np.array(q0, dtype=np.float64)
    lower = upper = 0
    remembered = [None, None]
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
                first = ns[t, stage] == 0
                if first and remembered[stage] is not None:
                    if stats is not None:
                        stats["restores"] = stats.get("restores", 0) + 1
                        stats["replaced"] = stats.get("replaced", 0) + int(remembered[stage] != (lower, upper))
                    lower, upper = remembered[stage]
                H, c, lo, hi = oracle.build_qp(model, ts, stage, q, tgt)
                x, lower, upper = bpp_solve(H, c, lo, hi, lower, upper, log)
                if first:
                    remembered[stage] = (lower, upper)
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
