#!/usr/bin/env python3
"""Diagnostic: per-phase cycle shares of the IK kernel (GMR_IK_PROFILE build, s_memtime stamps).
Not part of the product or of the bench; read SHARES, not absolute time (stamps forbid overlap).

    python tools/phase_profile.py [S] [T]

GMR_PROF_LIBRARY=/path/to/libgmrhip_prof.so profiles that build instead (A/B of two trees' profile builds).
The tree QP counts its pivoting rounds (one factorisation each) in NFACT: "rounds/solve".
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from general_motion_retargeting_amd import _lib, params, synth  # noqa: E402
from general_motion_retargeting_amd.ik_config import build_task_tables, pack_model, pack_taskset  # noqa: E402
from general_motion_retargeting_amd.models import load_ik_config, load_robot  # noqa: E402

# csrc/gmr_ik_prof.h.  QWALK, ROT, K2, POS: the latency kernel's split evaluation after a solve (main wavefront): rotation
# walk, rotation halves of residuals and series, wait at the barrier behind helper 1's walk, position halves.
PH = ["PRE", "FK", "ERR", "JLOG", "PAIRS", "CVEC", "HACC", "KBUILD", "CHOL", "SUBST", "RATIO", "MULT", "INTEG", "IO",
      "QWALK", "ROT", "K2", "POS", "NFACT", "NSOLVE", "TICKS", "REALTIME"]
# a library from before the split has no QWALK .. POS (GMR_PROF_LEGACY=1: A/B against such a build)
if os.environ.get("GMR_PROF_LEGACY"):
    PH = [n for n in PH if n not in ("QWALK", "ROT", "K2", "POS")]
NT = PH.index("NFACT")          # the stamped phases come first, then the counters
NFACT, NSOLVE, TICKS, REALTIME = (PH.index(n) for n in ("NFACT", "NSOLVE", "TICKS", "REALTIME"))


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    pkg = os.path.join(ROOT, "general_motion_retargeting_amd")
    so = os.environ.get("GMR_PROF_LIBRARY") or os.path.join(pkg, "libgmrhip_prof.so")
    if not os.path.exists(so) or os.environ.get("REBUILD"):
        from general_motion_retargeting_amd import build
        build.build_variant("prof", ["-DGMR_IK_PROFILE"])
    _lib.LIB_PATH = so
    L = _lib.lib()
    model = load_robot(params.ROBOT_XML_DICT["unitree_g1"])
    tt = build_task_tables(load_ik_config(params.IK_CONFIG_DICT["smplx"]["unitree_g1"]), None)
    sol = _lib.Solver(pack_model(model), pack_taskset(model, tt))
    human, q0 = synth.make_streams(model, tt, S, T, seed=0)
    d_q0 = _lib.DeviceBuffer.from_host(q0)
    d_h = _lib.DeviceBuffer.from_host(human)
    d_qo = _lib.DeviceBuffer(S * T * sol.nq * 8)
    d_ns = _lib.DeviceBuffer(S * T * 8)
    d_st = _lib.DeviceBuffer(S * 4)
    d_pr = _lib.DeviceBuffer(2 * S * len(PH) * 8)
    _lib.check(L.gmr_memset(d_pr.ptr, 0, 2 * S * len(PH) * 8, None))
    fn = L.gmr_retarget_streams_prof
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 4
    for _ in range(2):
        _lib.check(fn(sol.handle, S, T, d_q0.ptr, d_h.ptr, 0, d_qo.ptr, d_ns.ptr, d_st.ptr, d_pr.ptr))
    _lib.check(L.gmr_stream_sync(None))
    both = d_pr.to_host((2, S, len(PH)), np.uint64).astype(np.float64)
    pr, hp = both[0], both[1]
    tot = pr[:, :NT].sum(axis=1).mean()
    nsolve = pr[:, NSOLVE].mean()
    nfact = pr[:, NFACT].mean()
    print(f"S={S} T={T}  solves/stream={nsolve:.0f}  rounds/solve={nfact / nsolve:.3f}  "
          f"stamped cycles/solve={tot / nsolve:.0f} (100 MHz ticks if s_memtime is the constant clock)")
    clk = pr[:, TICKS].mean() / pr[:, REALTIME].mean() * 100.0
    print(f"  kernel ticks/stream={pr[:, TICKS].mean():.3e}  realtime(100MHz)={pr[:, REALTIME].mean():.3e}  => in-kernel clock {clk:.0f} MHz; "
          f"stream wall {pr[:, REALTIME].mean() / 100.0:.0f} us")
    rt = pr[:, REALTIME] / 100.0
    print("  per-stream wall us: min %.0f median %.0f max %.0f ; rounds/solve per stream: min %.3f max %.3f" % (
        rt.min(), np.median(rt), rt.max(), (pr[:, NFACT] / pr[:, NSOLVE]).min(), (pr[:, NFACT] / pr[:, NSOLVE]).max()))
    for i, n in enumerate(PH[:NT]):
        print(f"  {n:7s} {pr[:, i].mean() / tot * 100:6.2f} %   {pr[:, i].mean() / nsolve:10.0f} /solve")
    if S <= 512:     # latency shape: the batch's time is its slowest stream's -- the same breakdown for that stream alone
        k = int(np.argmax(pr[:, REALTIME]))
        med = int(np.argsort(pr[:, REALTIME])[S // 2])
        for name, i in (("slowest", k), ("median", med)):
            ns_i, tot_i = pr[i, NSOLVE], pr[i, :NT].sum()
            print(f"  {name} stream {i}: wall {pr[i, REALTIME] / 100.0:.0f} us, {ns_i:.0f} solves, {pr[i, NFACT] / ns_i:.3f} rounds/solve, "
                  f"{tot_i / ns_i:.0f} stamped cycles/solve: " +
                  " ".join(f"{n}={pr[i, j] / ns_i:.0f}" for j, n in enumerate(PH[:NT])))
    if hp.sum() > 0:
        print("  helper wavefront 1 (cycles/solve): idle at B1 %.0f, FK walk %.0f, wait K2 %.0f, Jacobian share %.0f, wait B2 %.0f, "
              "H share %.0f, wait B3 %.0f, tree-QP %.0f" % (
            hp[:, 0].mean() / nsolve, hp[:, 1].mean() / nsolve, hp[:, 2].mean() / nsolve, hp[:, 4].mean() / nsolve,
            hp[:, 5].mean() / nsolve, hp[:, 6].mean() / nsolve, hp[:, 3].mean() / nsolve, hp[:, 7:14].sum(axis=1).mean() / nsolve))
        if "INTEG" in PH and hp[:, PH.index("INTEG")].sum() > 0:   # the helpers never integrate: the slot holds the other half of B1
            ij = PH.index("INTEG")
            print("  helper wavefront 1: 'idle at B1' above is the wait behind a QP only (%.0f); the wait behind jbody_phase is %.0f cycles/solve"
                  % (hp[:, 0].mean() / nsolve, hp[:, ij].mean() / nsolve)
                  + ("; slowest stream %.0f behind jbody_phase / %.0f behind the QP, median stream %.0f / %.0f"
                     % (hp[k, ij] / pr[k, NSOLVE], hp[k, 0] / pr[k, NSOLVE], hp[med, ij] / pr[med, NSOLVE], hp[med, 0] / pr[med, NSOLVE])
                     if S <= 512 else ""))
        if S <= 512:
            for name, i in (("slowest", k), ("median", med)):
                ns_i = pr[i, NSOLVE]
                print(f"  helper wavefront 1 of the {name} stream {i} (cycles/solve): idle at B1 {hp[i, 0] / ns_i:.0f}, "
                      f"FK walk {hp[i, 1] / ns_i:.0f}, wait K2 {hp[i, 2] / ns_i:.0f}")


if __name__ == "__main__":
    main()
