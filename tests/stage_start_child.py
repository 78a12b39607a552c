"""Child process of tests/test_ik_stage_start.py: one launch of the IK kernel through the library that GMR_HIP_LIBRARY
names (a process loads one library), results into an .npz.

    python stage_start_child.py run  <in.npz> <out.npz> <waves>     q, nsolve, status of Solver.retarget_streams
    python stage_start_child.py prof <in.npz> <out.npz> <waves>     per-stream NFACT / NSOLVE of a GMR_IK_PROFILE build

in.npz: mb, ts (packed blobs), q0, human.  GMR_IK_NO_WIDE, if wanted, is set by the parent.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PH_NFACT, PH_NSOLVE, PH_COUNT = 18, 19, 22          # csrc/gmr_ik_prof.h


def main():
    mode, src, dst, waves = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
    from general_motion_retargeting_amd import _lib
    assert os.environ.get("GMR_HIP_LIBRARY") and _lib.LIB_PATH == os.environ["GMR_HIP_LIBRARY"]
    _lib.require_gpu()
    d = np.load(src)
    q0, human = d["q0"], d["human"]
    sol = _lib.Solver(np.frombuffer(d["mb"].tobytes(), dtype=_lib.MODEL_DTYPE),
                      np.frombuffer(d["ts"].tobytes(), dtype=_lib.TASKSET_DTYPE))
    sol.set_waves(waves)
    if mode == "run":
        q, ns, st = sol.retarget_streams(q0, human)
        np.savez(dst, q=q, ns=ns, st=st)
        return
    S, T = human.shape[:2]
    L = _lib.lib()
    d_q0, d_h = _lib.DeviceBuffer.from_host(q0), _lib.DeviceBuffer.from_host(human)
    d_qo, d_ns, d_st = _lib.DeviceBuffer(S * T * sol.nq * 8), _lib.DeviceBuffer(S * T * 8), _lib.DeviceBuffer(S * 4)
    d_pr = _lib.DeviceBuffer(2 * S * PH_COUNT * 8)
    _lib.check(L.gmr_memset(d_pr.ptr, 0, 2 * S * PH_COUNT * 8, None))
    fn = L.gmr_retarget_streams_prof
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 4
    _lib.check(fn(sol.handle, S, T, d_q0.ptr, d_h.ptr, 0, d_qo.ptr, d_ns.ptr, d_st.ptr, d_pr.ptr))
    _lib.check(L.gmr_stream_sync(None))
    pr = d_pr.to_host((2, S, PH_COUNT), np.uint64)[0]
    np.savez(dst, nfact=pr[:, PH_NFACT].astype(np.int64), nsolve=pr[:, PH_NSOLVE].astype(np.int64),
             st=d_st.to_host((S,), np.int32), ns=d_ns.to_host((S, T, 2), np.int32))


if __name__ == "__main__":
    main()
