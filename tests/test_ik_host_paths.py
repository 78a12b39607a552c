"""The host-buffer IK entry points with every array of a job in play: ``tgt_out`` and ``err_out`` (which the Python wrapper of
the group entry point never passes), ``len`` and ``scale``, through slices of streams, windows of frames, two jobs, and the
pinned staging of a small call.

The contract is bitwise: all five outputs equal those of ``Solver.retarget_streams`` on the whole batch.  Every output array
is pre-filled with 0xFF before a call, so a row the library forgets to write -- or to zero: the rows at and beyond
``lens[s]`` -- shows.  Streams of three heights, each generated with the task tables of its own height, so that targets are
reachable and every status is OK (asserted on both sides).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import get_setup

pytestmark = pytest.mark.gpu

S, T = 12, 8
LENS = np.array([8, 1, 5, 8, 4, 7, 8, 2, 8, 3, 6, 8], dtype=np.int32)
HEIGHTS = np.array([1.60, 1.75, 1.83])
NAMES = ("q_out", "nsolve", "status", "tgt_out", "err_out")


def _inputs():
    from general_motion_retargeting_amd import synth
    from general_motion_retargeting_amd.ik_config import scale_rows
    base = get_setup("smplx", "unitree_g1")
    hidx = np.arange(S) % 3
    human = np.empty((S, T, len(base.tt.human_names), 7))
    for k in range(3):
        su = get_setup("smplx", "unitree_g1", float(HEIGHTS[k]))
        ids = np.nonzero(hidx == k)[0]
        human[ids] = synth.make_streams_ids(su.model, su.tt, ids, T, seed=33)[0]
    q0 = np.broadcast_to(base.model.qpos0, (S, base.model.nq)).copy()
    return base, q0, human, scale_rows(base.cfg, HEIGHTS[hidx])


def _fresh(sol, n):
    """the five output arrays of n streams, every byte 0xFF"""
    shapes = ((n, T, sol.nq), (n, T, 2), (n,), (n, T, sol.nhuman, 7), (n, T, 2))
    dtypes = (np.float64, np.int32, np.int32, np.float64, np.float64)
    outs = [np.empty(s, d) for s, d in zip(shapes, dtypes)]
    for o in outs:
        o.view(np.uint8)[...] = 0xFF
    return outs


def _check(got, ref, lens, what):
    for name, a, b in zip(NAMES, got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name)
    assert (got[2] == 0).all(), (what, got[2])
    for s, n in enumerate(lens):
        for name, a in zip(NAMES, got):
            if a.ndim > 1:
                assert not a[s, n:].view(np.uint8).any(), (what, name, s)


def test_every_array_of_a_job_through_slices_windows_and_pinned_staging():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    L = _lib.lib()
    su, q0, human, scales = _inputs()
    sol = _lib.Solver(su.mb, su.ts)
    sol.set_waves(1)
    try:
        ref = sol.retarget_streams(q0, human, lens=LENS, scales=scales, want_targets=True, want_errors=True)
        assert (ref[2] == _lib.STATUS_OK).all(), ref[2]
        for s, n in enumerate(LENS):
            assert not any(a[s, n:].view(np.uint8).any() for a in ref if a.ndim > 1), s

        def group(parts, slices):
            """the batch as one job per (first, count) part"""
            outs = _fresh(sol, S)
            arr = (_lib.Job * len(parts))()
            for i, (a, n) in enumerate(parts):
                b = a + n
                arr[i] = _lib.Job(sol.handle.value, n, T, q0[a:b].ctypes.data, human[a:b].ctypes.data, LENS[a:b].ctypes.data,
                                  outs[0][a:b].ctypes.data, outs[1][a:b].ctypes.data, outs[2][a:b].ctypes.data,
                                  outs[3][a:b].ctypes.data, outs[4][a:b].ctypes.data, scales[a:b].ctypes.data)
            _lib.check(L.gmr_retarget_group(C.cast(arr, C.c_void_p), len(parts), 0, slices))
            _check(outs, ref, LENS, (parts, slices))

        for slices in (1, 3, -2):
            group([(0, S)], slices)
        for slices in (2, -2):
            group([(0, 5), (5, 7)], slices)
        # the pinned path (two streams are far less than 1 MiB), after the reference call left the solver's grow-only workspace
        # full of the bytes of twelve streams
        outs = _fresh(sol, 2)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(L.gmr_retarget_streams_scaled(sol.handle, 2, T, p(q0[:2]), p(human[:2]), p(LENS[:2]), p(scales[:2]), 0, *(p(o) for o in outs)))
        _check(outs, [a[:2] for a in ref], LENS[:2], "pinned")
    finally:
        sol.set_waves(0)
