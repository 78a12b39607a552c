"""Per-stream human scale tables, the part that needs no GPU: the packed table of a height, the C ABI's new symbols and job
field, the argument checks of the Python layers (all raised before any device call) and the rule that keeps height groups
under chunking.  tests/test_ik_stream_scales.py runs the kernels."""
import ctypes as C

import numpy as np
import pytest

from conftest import ALL_CONFIGS, get_setup
from general_motion_retargeting_amd import _lib, dataset
from general_motion_retargeting_amd.ik_config import build_task_tables, scale_row, scale_rows


@pytest.mark.parametrize("src,robot", ALL_CONFIGS)
def test_packed_table_of_a_height_is_the_task_tables_scale_table(src, robot):
    su = get_setup(src, robot)
    for h in (1.52, 1.95):
        tt = build_task_tables(su.cfg, h)
        want = np.array([tt.scale_table[n] for n in tt.human_names], dtype=np.float64)
        got = scale_row(su.cfg, h)
        assert got.dtype == np.float64 and got.shape == (len(tt.human_names),) and got.tobytes() == want.tobytes()
        from general_motion_retargeting_amd.ik_config import pack_taskset
        assert pack_taskset(su.model, tt)["scale"][0][: len(want)].astype(np.float64).tobytes() == want.tobytes()
    rows = scale_rows(su.cfg, [1.95, None, 1.52])
    assert rows.shape == (3, len(su.tt.human_names)) and rows.flags.c_contiguous
    assert rows[0].tobytes() == scale_row(su.cfg, 1.95).tobytes() and rows[2].tobytes() == scale_row(su.cfg, 1.52).tobytes()
    assert rows[1].tobytes() == np.array([su.tt.scale_table[n] for n in su.tt.human_names]).tobytes()      # no height: ratio 1
    for bad in (0.0, -1.7, np.inf):
        with pytest.raises(ValueError):
            scale_rows(su.cfg, [1.7, bad])


def test_library_exports_the_new_symbols():
    L = C.CDLL(_lib.LIB_PATH)
    for sym in ("gmr_retarget_streams_scaled", "gmr_retarget_streams_scaled_dev", "gmr_retarget_streams", "gmr_retarget_streams_dev"):
        assert hasattr(L, sym), sym
        assert sym in _lib._SIGS, sym
    assert len(_lib._SIGS["gmr_retarget_streams_scaled"][1]) == len(_lib._SIGS["gmr_retarget_streams"][1]) + 1
    assert len(_lib._SIGS["gmr_retarget_streams_scaled_dev"][1]) == len(_lib._SIGS["gmr_retarget_streams_dev"][1]) + 1


def test_job_has_twelve_fields_and_scale_is_last():
    names = [f[0] for f in _lib.Job._fields_]
    assert len(names) == 12 and names[-1] == "scale" and names[:11] == ["solver", "S", "T", "q0", "human", "len", "q_out", "nsolve", "status",
                                                                        "tgt_out", "err_out"]
    assert C.sizeof(_lib.Job) == 88 and _lib.Job.scale.offset == 80          # include/gmr_hip.h: gmr_job_t
    j = _lib.Job(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)            # eleven values, as every caller of today fills it
    assert j.scale is None and j.err_out == 11


class _NoDevice:
    """stands in for the library: any call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def _fake_solver(nq=36, nhuman=14):
    sol = _lib.Solver.__new__(_lib.Solver)
    sol.handle, sol.nq, sol.nhuman = None, nq, nhuman
    return sol


def test_scales_are_checked_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())
    sol = _fake_solver()
    human, q0 = np.zeros((3, 2, 14, 7)), np.zeros((3, 36))
    with pytest.raises(ValueError, match=r"\[3,14\]"):
        sol.retarget_streams(q0, human, scales=np.ones((2, 14)))
    with pytest.raises(ValueError, match=r"\[3,14\]"):
        sol.retarget_streams(q0, human, scales=np.ones((3, 13)))
    with pytest.raises(ValueError, match=r"\[3,14\]"):
        sol.retarget_streams(q0, human, scales=np.ones(42))
    with pytest.raises(TypeError, match="numbers"):
        sol.retarget_streams(q0, human, scales=np.full((3, 14), "1.0"))
    with pytest.raises(ValueError, match=r"job 0: scales must be \[3,14\]"):
        _lib.retarget_group([{"solver": sol, "human": human, "q0": q0, "scales": np.ones((3, 15))}])
    with pytest.raises(ValueError, match="9 or 10"):
        _lib.retarget_group_dev([(sol, 3, 2, None, None, None, None, None)])
    ok = _lib.check_scales(np.ones((3, 14), dtype=np.float32)[:, ::1], 3, 14)
    assert ok.dtype == np.float64 and ok.flags.c_contiguous and _lib.check_scales(None, 3, 14) is None


def test_dev_job_names_the_nine_or_ten_elements(monkeypatch):
    """a plain 9- or 10-sequence and a DevJob are the same job; any other length is refused before a device call"""
    assert _lib.DevJob._fields == ("solver", "S", "T", "q0", "human", "len", "q_out", "nsolve", "status", "scale")
    nine = ("sol", 3, 2, "q0", "human", "len", "q_out", "nsolve", "status")
    a, b = _lib.dev_job(nine), _lib.dev_job(list(nine) + ["scale"])
    assert a[:9] == b[:9] == nine and a.scale is None and b.scale == "scale" and (b.len, b.q_out, b.nsolve) == ("len", "q_out", "nsolve")
    assert _lib.dev_job(b) is b and _lib.DevJob(*nine) == a and len(a) == 10

    seen = []

    class _Records:
        def gmr_retarget_group_dev(self, arr, n, flags, stream):
            jobs = C.cast(arr, C.POINTER(_lib.Job))
            seen.append([(jobs[i].S, jobs[i].T, jobs[i].q0, jobs[i].status, jobs[i].scale) for i in range(n)])
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: _Records())
    sol = _fake_solver()
    sol.handle = C.c_void_p(0x42)
    q0, status, scale = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)
    _lib.retarget_group_dev([(sol, 3, 2, q0, None, None, None, None, status), (sol, 3, 2, q0, None, None, None, None, status, scale),
                             _lib.DevJob(sol, 3, 2, q0, None, None, None, None, status, scale)])
    assert seen == [[(3, 2, 0x1000, 0x2000, None), (3, 2, 0x1000, 0x2000, 0x3000), (3, 2, 0x1000, 0x2000, 0x3000)]]
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())
    for n in (8, 11):
        with pytest.raises(ValueError, match="9 or 10"):
            _lib.retarget_group_dev([(sol, 3, 2) + (None,) * (n - 3)])


def test_heights_and_scales_exclude_each_other(monkeypatch):
    from general_motion_retargeting_amd import GeneralMotionRetargeting
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())
    g = GeneralMotionRetargeting("smplx", "unitree_g1", actual_human_height=1.8)
    nh = len(g.human_body_names)
    human = np.zeros((2, 3, nh, 7))
    with pytest.raises(ValueError, match="not both"):
        g.retarget_streams(human, heights=[1.6, 1.7], scales=np.ones((2, nh)))
    with pytest.raises(ValueError, match=r"heights must be \[2\]"):
        g.retarget_streams(human, heights=[1.6, 1.7, 1.8])
    with pytest.raises(ValueError, match="finite and positive"):
        g.retarget_streams(human, heights=[1.6, -1.0])
    with pytest.raises(ValueError, match=rf"\[2,{nh}\]"):
        g.retarget_streams(human, scales=np.ones((2, nh + 1)))
    # the rows of a height do not depend on the height the object was built for
    rows = g.stream_scales(2, heights=[1.6, 1.8])
    cfg = get_setup("smplx", "unitree_g1").cfg
    assert rows.tobytes() == scale_rows(cfg, [1.6, 1.8]).tobytes()
    assert rows[1].tobytes() == np.array(list(g.human_scale_table.values())).tobytes()
    assert g.stream_scales(2) is None
    with pytest.raises(ValueError, match="3 heights for 2 clips"):
        dataset.retarget_clips("smplx", "unitree_g1", [human[0], human[1]], [30, 30], actual_human_height=[1.6, 1.7, 1.8])


def test_chunking_keeps_height_groups(monkeypatch):
    """Scale rows are not gathered into chunk jobs: a chunk spec that takes effect keeps one job per height; one that does not
    (no clip longer than its frames) leaves the merged job."""
    from general_motion_retargeting_amd import chunking
    spec = chunking.ChunkSpec(64)
    assert dataset.heights_groups_needed(spec, [10, 65, 3]) and not dataset.heights_groups_needed(spec, [10, 64, 3])
    assert not dataset.heights_groups_needed(None, [10, 6500, 3])
    assert dataset.heights_path() == "merged"
    monkeypatch.setenv("GMR_DATASET_HEIGHTS", "groups")
    assert dataset.heights_path() == "groups"
    monkeypatch.delenv("GMR_DATASET_HEIGHTS")
    # retarget_clips with per-clip heights and such a spec: one call per height, each with that height as a number
    calls = []

    class Stub:
        chunk_report = None
        library = None

        def __init__(self, src, robot, height, *a, **k):
            calls.append(height)

        def __call__(self, clips, fps):
            return [len(c) for c in clips]
    monkeypatch.setattr(dataset, "ClipRetargeter", Stub)
    clips = [np.zeros((n, 14, 7)) for n in (70, 5, 9, 66)]
    out = dataset.retarget_clips("smplx", "unitree_g1", clips, [30] * 4, actual_human_height=[1.6, 1.7, 1.6, 1.7], chunk=spec)
    assert calls == [1.6, 1.7] and out == [70, 5, 9, 66]
    calls.clear()
    out = dataset.retarget_clips("smplx", "unitree_g1", clips[1:3], [30] * 2, actual_human_height=[1.6, 1.7], chunk=spec)
    assert len(calls) == 1 and list(calls[0]) == [1.6, 1.7] and out == [5, 9]
    with pytest.raises(ValueError, match="one job"):
        dataset.retarget_clips("smplx", "unitree_g1", clips, [30] * 4, actual_human_height=[1.6, 1.7, 1.6, 1.7], chunk=spec, library=True)
