"""The refusals of the IK group entry points that come before any device call (csrc/gmr_ik_host.hip: one check of a job list
for all of them), through the built library, without a GPU."""
import ctypes as C

import pytest

from general_motion_retargeting_amd import _lib

GMR_ERR_ARG = -1


def _jobs(*jobs):
    return C.cast((_lib.Job * max(len(jobs), 1))(*jobs), C.c_void_p)


@pytest.mark.parametrize("entry", ["gmr_retarget_group_dev", "gmr_retarget_group"])
def test_a_bad_job_list_and_a_null_solver_are_refused(entry):
    L = _lib.lib()
    call = getattr(L, entry)
    last = None if entry.endswith("_dev") else 0         # the stream / the slice count
    assert call(_jobs(), -1, 0, last) == GMR_ERR_ARG and L.gmr_last_error() == b"bad job list"
    assert call(None, 1, 0, last) == GMR_ERR_ARG and L.gmr_last_error() == b"bad job list"
    job = _lib.Job(None, 1, 1, None, None, None, None, None, None, None, None, None)
    assert call(_jobs(job), 1, 0, last) == GMR_ERR_ARG and L.gmr_last_error() == b"job 0: null solver"
    assert call(_jobs(), 0, 0, last) == 0


def test_an_empty_window_is_refused():
    L = _lib.lib()
    job = _lib.Job(None, 1, 1, None, None, None, None, None, None, None, None, None)
    for t_begin, t_end in ((4, 4), (4, 2), (-1, 3)):
        assert L.gmr_retarget_group_window_dev(_jobs(job), 1, 0, t_begin, t_end, None) == GMR_ERR_ARG
        assert L.gmr_last_error() == f"bad window [{t_begin}, {t_end})".encode()
    assert L.gmr_retarget_group_window_dev(_jobs(), -1, 0, 4, 4, None) == GMR_ERR_ARG and L.gmr_last_error() == b"bad job list"
    assert L.gmr_retarget_group_window_dev(_jobs(job), 1, 0, 0, 4, None) == GMR_ERR_ARG and L.gmr_last_error() == b"job 0: null solver"
