"""NumPy mirror of the chunked-retargeting steps (``csrc/gmr_chunk.hip``): plan, gather, stitch, seams and the pass loop around
any IK callable -- the CPU oracle in the host tests and in ``tools/chunk_probe.py --oracle``, the HIP launch in the GPU tests.
Test infrastructure: nothing in the product package imports this."""
from __future__ import annotations

import numpy as np

PASS0, REPAIR = 0, 1


def plan_np(lens, L, W):
    """(chunk i32[nchunk,4] = clip, first source frame, warm, owned; clip_first i32[nclip+1]; Tc)"""
    rows, first = [], [0]
    for c, n in enumerate(int(x) for x in lens):
        K = max(1, -(-n // L))
        for i in range(K):
            a, b = i * n // K, (i + 1) * n // K
            warm = min(W, a) if i > 0 else 0
            rows.append((c, a - warm, warm, b - a))
        first.append(len(rows))
    chunk = np.array(rows, dtype=np.int32).reshape(-1, 4)
    Tc = max(1, int((chunk[:, 2] + chunk[:, 3]).max())) if len(rows) else 1
    return chunk, np.array(first, dtype=np.int32), Tc


def _clamp(rec, S, T, Tc):
    clip, src0, warm, owned = (int(x) for x in rec)
    ok = 0 <= clip < S
    src0 = min(max(src0, 0), T)
    warm = min(max(warm, 0), min(Tc, T - src0))
    owned = min(max(owned, 0), min(Tc - warm, T - src0 - warm))
    return ok, clip, src0, warm, owned


def gather_np(chunk, Tc, slots, mode, human, q0, q_out, human_c, len_c, q0_c, q_seam):
    """``slots``: chunk index per slot (``range(nchunk)`` in pass 0).  Writes into the given arrays, like the kernel."""
    S, T = human.shape[:2]
    for s, k in enumerate(slots):
        ok = 0 <= k < len(chunk)
        if ok:
            ok, clip, src0, warm, owned = _clamp(chunk[k], S, T, Tc)
        if not ok:
            len_c[s] = 0
            q0_c[s] = q0[0]
            continue
        first, frames = (src0 + warm, owned) if mode == REPAIR else (src0, warm + owned)
        len_c[s] = frames
        row = q_out[clip, first - 1] if (mode == REPAIR and first > 0) else q0[clip]
        q0_c[s] = row
        if mode == REPAIR:
            q_seam[k] = row
        human_c[s, :frames] = human[clip, first:first + frames]


def stitch_np(chunk, clip_first, Tc, slots, mode, q_out_c, nsolve_c, status_c, q_out, nsolve, chunk_status, status, q_seam, warm_solves):
    S, T = q_out.shape[:2]
    for s, k in enumerate(slots):
        if not 0 <= k < len(chunk):
            continue
        ok, clip, src0, warm, owned = _clamp(chunk[k], S, T, Tc)
        if not ok:
            continue
        skip, o0 = (0 if mode == REPAIR else warm), src0 + warm
        chunk_status[k] = status_c[s]
        if mode == PASS0:
            q_seam[k] = q_out_c[s, warm - 1] if warm > 0 else np.nan
        q_out[clip, o0:o0 + owned] = q_out_c[s, skip:skip + owned]
        nsolve[clip, o0:o0 + owned] = nsolve_c[s, skip:skip + owned]
    for c in range(S):
        a, b = int(clip_first[c]), int(clip_first[c + 1])
        bad = [k for k in range(a, b) if chunk_status[k] != 0]
        status[c] = chunk_status[bad[0]] if bad else 0
        if mode == PASS0:
            warm_solves[c] = sum(int(nsolve_c[k, :_clamp(chunk[k], S, T, Tc)[3]].sum()) for k in range(a, b))


def seams_np(chunk, clip_first, Tc, q_out, q_seam, chunk_status, tol):
    """(resid f64[nchunk,3], bad list i32[nbad] ascending, seam_max f64[S,3])"""
    S, T = q_out.shape[:2]
    n = len(chunk)
    resid = np.zeros((n, 3))
    bad = []
    for k in range(n):
        ok, clip, src0, warm, owned = _clamp(chunk[k], S, T, Tc)
        if not (k > 0 and ok and src0 + warm > 0 and int(clip_first[clip]) != k):
            continue
        a, b = q_out[clip, src0 + warm - 1], q_seam[k]
        with np.errstate(invalid="ignore"):
            resid[k, 0] = np.nan if np.isnan(b[7:] - a[7:]).any() else (np.abs(b[7:] - a[7:]).max() if len(a) > 7 else 0.0)
            resid[k, 1] = np.nan if np.isnan(b[:3] - a[:3]).any() else np.abs(b[:3] - a[:3]).max()
            aw, ax, ay, az = a[3], -a[4], -a[5], -a[6]
            bw, bx, by, bz = b[3:7]
            d = np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                          aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])
            nv, w = np.sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]), abs(d[0])
            resid[k, 2] = 2.0 * np.arctan2(nv, w) if (nv > 0 or w > 0) else np.nan
        if chunk_status[k - 1] == 0 and not np.all(resid[k] <= tol):
            bad.append(k)
    seam_max = np.zeros((S, 3))
    for c in range(S):
        r = resid[int(clip_first[c]):int(clip_first[c + 1])]
        for i in range(3):
            seam_max[c, i] = np.nan if np.isnan(r[:, i]).any() else (r[:, i].max() if len(r) else 0.0)
    return resid, np.array(bad, dtype=np.int32), seam_max


def run_chunked_np(ik, human, q0, lens, L, W, tol, max_passes):
    """The pass loop with ``ik(q0_c[n,nq], human_c[n,Tc,nh,7], len_c[n]) -> (q_out_c, nsolve_c, status_c)``.
    Returns a dict: q_out, nsolve, status, resid0, resid, warm_solves, passes, chunk, clip_first, Tc, bad (after the last pass)."""
    S, T = human.shape[:2]
    nq = q0.shape[1]
    chunk, first, Tc = plan_np(lens, L, W)
    n = len(chunk)
    q_out, nsolve, status = np.zeros((S, T, nq)), np.zeros((S, T, 2), np.int32), np.zeros(S, np.int32)
    chunk_status, q_seam, warm_solves = np.zeros(n, np.int32), np.zeros((n, nq)), np.zeros(S, np.int32)

    def one_pass(slots, mode):
        m = len(slots)
        human_c = np.zeros((m, Tc) + human.shape[2:])
        human_c[..., 3] = 1.0
        len_c, q0_c = np.zeros(m, np.int32), np.zeros((m, nq))
        gather_np(chunk, Tc, slots, mode, human, q0, q_out, human_c, len_c, q0_c, q_seam)
        q_c, ns_c, st_c = ik(q0_c, human_c, len_c)
        stitch_np(chunk, first, Tc, slots, mode, q_c, ns_c, st_c, q_out, nsolve, chunk_status, status, q_seam, warm_solves)
        return seams_np(chunk, first, Tc, q_out, q_seam, chunk_status, tol)

    resid0, bad, _ = one_pass(list(range(n)), PASS0)
    resid, passes = resid0, 0
    while len(bad) and (max_passes is None or passes < max_passes):
        resid, bad, _ = one_pass(bad.tolist(), REPAIR)
        passes += 1
    return {"q_out": q_out, "nsolve": nsolve, "status": status, "resid0": resid0, "resid": resid, "warm_solves": warm_solves,
            "passes": passes, "chunk": chunk, "clip_first": first, "Tc": Tc, "bad": bad}


def oracle_ik(model_blob, taskset_blob, nthreads=1):
    """the CPU oracle as the ``ik`` of :func:`run_chunked_np`.  It has no per-stream lengths: rows beyond ``len_c`` repeat the
    stream's last frame (so that they solve), and the stitch ignores them."""
    from oracle import oracle

    def ik(q0_c, human_c, len_c):
        human_c = human_c.copy()
        for s, n in enumerate(len_c):
            if 0 < n < human_c.shape[1]:
                human_c[s, n:] = human_c[s, n - 1]
        return oracle.retarget_streams(model_blob, taskset_blob, q0_c, human_c, nthreads=nthreads)
    return ik
