"""Per-stream human scale tables: ONE solver (built from the unscaled config) and ONE launch serve subjects of every height.

The contract is bitwise: a stream retargeted with scale row r gives the bytes of today's kernel with a task set whose table
is r.  So every test builds eight solvers the old way, one per ``actual_human_height``, launches each on its own streams
(same ``lens``, same forced launch shape where shapes differ by rounding) and compares ``q_out``, ``nsolve``, ``status``,
``tgt_out`` and ``err_out`` of the merged launch byte for byte.

Heights: 1.40 ... 1.95 (eight); stream s gets height (5 s) mod 8, so neighbouring streams never share a row.  Inputs come
from ``synth.make_streams_ids`` with the task tables OF THAT STREAM'S HEIGHT (stream s uses seed + s whatever set it is
generated in), so targets are reachable and every status is OK -- asserted on both sides.  The one exception is the
stream that test 1 gives an absent body (``pos[0] = NaN``): every human body of smplx -> unitree_g1 carries a task, so that
stream's status is whatever today's kernel says about it, and must be the same on both sides.
"""
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import get_setup

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smplx_synth as sx  # noqa: E402

pytestmark = pytest.mark.gpu

HEIGHTS = np.array([1.40, 1.52, 1.60, 1.66, 1.71, 1.75, 1.83, 1.95])
TOL_RAD = TOL_POS = 1e-9          # tests/test_gpu_parity.py's own: FP64 kernel vs FP64 oracle


def height_index(S):
    return (5 * np.arange(S)) % 8


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


_batches = {}


def batch(src, robot, S, T, seed, period=None):
    """(human, q0, scales, hidx) of S streams; stream s is generated with the tables of its own height.  ``period``: only that
    many distinct streams, repeated (period a multiple of 8, so a stream's height still is (5 s) mod 8)."""
    key = (src, robot, S, T, seed, period)
    if key not in _batches:
        from general_motion_retargeting_amd import synth
        from general_motion_retargeting_amd.ik_config import scale_rows
        base = get_setup(src, robot)
        n = S if period is None else period
        assert n % 8 == 0 or period is None
        hidx = height_index(n)
        human = np.empty((n, T, len(base.tt.human_names), 7))
        for k in range(8):
            ids = np.nonzero(hidx == k)[0]
            if len(ids):
                su = get_setup(src, robot, float(HEIGHTS[k]))
                human[ids] = synth.make_streams_ids(su.model, su.tt, ids, T, seed)[0]
        pick = np.arange(S) % n
        human, hidx = np.ascontiguousarray(human[pick]), hidx[pick]
        q0 = np.broadcast_to(base.model.qpos0, (S, base.model.nq)).copy()
        _batches[key] = (human, q0, scale_rows(base.cfg, HEIGHTS[hidx]), hidx)
    return _batches[key]


_solvers = {}


def solver(hip, src, robot, height=None, waves=0, dispatch=None):
    key = (src, robot, height, waves, dispatch)
    if key not in _solvers:
        su = get_setup(src, robot, height)
        sol = hip.Solver(su.mb, su.ts)
        sol.set_waves(waves)
        if dispatch is not None:
            sol.set_dispatch(dispatch)
        _solvers[key] = sol
    return _solvers[key]


def per_height(hip, src, robot, human, q0, hidx, lens=None, flags=0, waves=0, dispatch=None):
    """the old way: one solver per height, each launched on its own streams"""
    S, T = human.shape[:2]
    su = get_setup(src, robot)
    nq, nh = su.model.nq, len(su.tt.human_names)
    out = (np.zeros((S, T, nq)), np.zeros((S, T, 2), np.int32), np.zeros(S, np.int32), np.zeros((S, T, nh, 7)), np.zeros((S, T, 2)))
    for k in np.unique(hidx):
        ids = np.nonzero(hidx == k)[0]
        sol = solver(hip, src, robot, float(HEIGHTS[k]), waves, dispatch)
        r = sol.retarget_streams(q0[ids], human[ids], lens=None if lens is None else lens[ids], flags=flags, want_targets=True,
                                 want_errors=True)
        for o, x in zip(out, r):
            o[ids] = x
    return out


def same(got, ref, what=""):
    for name, a, b in zip(("q_out", "nsolve", "status", "tgt_out", "err_out"), got, ref):
        assert _bits(a, b), (what, name)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ground", [False, True])
def test_latency_shape(hip, ground):
    """S = 8 (four wavefronts per stream), T = 5, lens 5 and 3 alternating, one stream with an absent body."""
    human, q0, scales, hidx = batch("smplx", "unitree_g1", 8, 5, seed=21)
    human = human.copy()
    human[6, :, 9, 0] = np.nan                          # stream 6 never saw body 9
    lens = np.array([5, 3] * 4, dtype=np.int32)
    flags = hip.FLAG_OFFSET_TO_GROUND if ground else 0
    ref = per_height(hip, "smplx", "unitree_g1", human, q0, hidx, lens, flags)
    got = solver(hip, "smplx", "unitree_g1").retarget_streams(q0, human, lens=lens, flags=flags, want_targets=True, want_errors=True,
                                                              scales=scales)
    print("status", got[2].tolist(), ref[2].tolist())
    assert not np.delete(got[2], 6).any() and not np.delete(ref[2], 6).any()
    same(got, ref, ground)
    # the rows differ between the heights, so the comparison could fail: stream 0 under stream 1's row is another result
    wrong = solver(hip, "smplx", "unitree_g1").retarget_streams(q0[:1], human[:1], scales=scales[1:2])
    assert not _bits(wrong[0], ref[0][:1])


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------------
def test_one_wavefront_per_stream_direct(hip):
    human, q0, scales, hidx = batch("smplx", "unitree_g1", 16, 5, seed=33)
    ref = per_height(hip, "smplx", "unitree_g1", human, q0, hidx, waves=1, dispatch=0)
    got = solver(hip, "smplx", "unitree_g1", None, 1, 0).retarget_streams(q0, human, want_targets=True, want_errors=True, scales=scales)
    assert not got[2].any() and not ref[2].any()
    same(got, ref)


def test_one_wavefront_per_stream_queued(hip):
    """set_dispatch(2), T = 5: items of 2 + 2 + 1 frames, so a wavefront changes stream (and scale row) between items.  The
    launch of S = 16 that the case names never reaches the queue (it engages when streams outnumber the resident wavefronts,
    about 2 300), so the same sixteen streams are ALSO launched repeated to S = 2 608, where it does."""
    import ctypes as C
    for S in (16, 2608):
        human, q0, scales, hidx = batch("smplx", "unitree_g1", S, 5, seed=33, period=16)
        ref = per_height(hip, "smplx", "unitree_g1", human[:16], q0[:16], hidx[:16], waves=1, dispatch=0)
        sol = solver(hip, "smplx", "unitree_g1", None, 1, 2)
        got = sol.retarget_streams(q0, human, want_targets=True, want_errors=True, scales=scales)
        assert not got[2].any() and not ref[2].any()
        pick = np.arange(S) % 16
        same(got, tuple(r[pick] for r in ref), S)
        # today's path: scales=None is the launch without the argument (the entry point that has no scale parameter)
        none = sol.retarget_streams(q0, human, want_targets=True, want_errors=True, scales=None)
        old = (np.zeros_like(none[0]), np.zeros_like(none[1]), np.zeros_like(none[2]), np.zeros_like(none[3]), np.zeros_like(none[4]))
        p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
        hip.check(hip.lib().gmr_retarget_streams(sol.handle, S, 5, p(q0), p(human), None, 0, *(p(a) for a in old)))
        same(none, old, S)
        assert not _bits(none[0], got[0])                   # (and the base table is not what the heights give)


# ---- 4, 5 ---------------------------------------------------------------------------------------------------------------------
_groups = {}


def group(hip, T):
    """three jobs, 304 streams: unitree_g1 160 with scales, booster_t1 120 with scales, a unitree_g1 solver of height 1.75 with
    24 streams and no scales; and each job's own separate launches (one wavefront per stream: the shape of the group)"""
    if T not in _groups:
        from general_motion_retargeting_amd import synth
        jobs, ref = [], []
        for robot, S, seed in (("unitree_g1", 160, 5), ("booster_t1", 120, 6)):
            human, q0, scales, hidx = batch("smplx", robot, S, T, seed)
            jobs.append({"solver": solver(hip, "smplx", robot), "human": human, "q0": q0, "scales": scales})
            ref.append(per_height(hip, "smplx", robot, human, q0, hidx, waves=1)[:3])
        su = get_setup("smplx", "unitree_g1", 1.75)
        human, q0 = synth.make_streams(su.model, su.tt, 24, T, seed=7)
        jobs.append({"solver": solver(hip, "smplx", "unitree_g1", 1.75), "human": human, "q0": q0})
        ref.append(solver(hip, "smplx", "unitree_g1", 1.75, 1).retarget_streams(q0, human))
        assert not any(r[2].any() for r in ref)
        _groups[T] = (jobs, ref)
    return _groups[T]


def _same_group(out, ref, what):
    for j, (a, b) in enumerate(zip(out, ref)):
        for name, x, y in zip(("q_out", "nsolve", "status"), a, b):
            assert _bits(x, y), (what, j, name)


def test_group_launch_as_one_scheduling_domain(hip):
    jobs, ref = group(hip, 3)
    assert sum(j["human"].shape[0] for j in jobs) == 304          # more than 300: the group takes the throughput shape by itself
    _same_group(hip.retarget_group(jobs, 0, 1), ref, "group")


def _window_launch(hip, jobs, T, windows):
    st = hip.Stream()
    dev, bufs = [], []
    for j in jobs:
        sol, S = j["solver"], j["human"].shape[0]
        b = [hip.DeviceBuffer.from_host(j["q0"]), hip.DeviceBuffer.from_host(j["human"]), hip.DeviceBuffer(S * T * sol.nq * 8),
             hip.DeviceBuffer(S * T * 8), hip.DeviceBuffer(S * 4)]
        if j.get("scales") is not None:
            b.append(hip.DeviceBuffer.from_host(j["scales"]))
        bufs.append(b)
        dev.append((sol, S, T, b[0], b[1], None, b[2], b[3], b[4]) + tuple(b[5:]))
    for w in windows:
        hip.retarget_group_dev(dev, 0, st, window=w)
    st.sync()
    out = [(b[2].to_host((d[1], T, d[0].nq), np.float64), b[3].to_host((d[1], T, 2), np.int32), b[4].to_host((d[1],), np.int32))
           for d, b in zip(dev, bufs)]
    for b in bufs:
        for x in b:
            x.free()
    return out


def test_windows(hip):
    """The group of test 4 in windows [0, 1), [1, 3) through the device entry point: every window reads the same scale rows.
    The host entry point with slices = 2 (a slice copies its rows of scale) and slices = -2.  A slice of 152 streams would
    take the latency shape by itself, whose bits are not the throughput shape's, so the solvers are told one wavefront per
    stream here; and the host pipeline cuts in time only from 4 frames on, so slices = -2 also runs on the same group with
    T = 5, where it does cut."""
    for T, windows in ((3, ((0, 1), (1, 3))), (5, ((0, 1), (1, 3), (3, 5)))):
        jobs, ref = group(hip, T)
        try:
            for j in jobs:
                j["solver"].set_waves(1)
            _same_group(_window_launch(hip, jobs, T, windows), ref, ("windows", T))
            one = hip.retarget_group(jobs, 0, 1)
            _same_group(one, ref, ("slices=1", T))
            for slices in (2, -2):
                _same_group(hip.retarget_group(jobs, 0, slices), one, (slices, T))
        finally:
            for j in jobs:
                j["solver"].set_waves(0)


def test_host_entry_points_name_a_bad_scale(hip):
    human, q0, scales, _ = batch("smplx", "unitree_g1", 8, 5, seed=21)
    sol = solver(hip, "smplx", "unitree_g1")
    for bad in (0.0, -1.0, np.nan, np.inf):
        s = scales.copy()
        s[5, 3] = bad
        with pytest.raises(hip.GmrHipError, match="stream 5, body 3"):
            sol.retarget_streams(q0, human, scales=s)
        with pytest.raises(hip.GmrHipError, match="job 0: scale of stream 5, body 3"):
            hip.retarget_group([{"solver": sol, "human": human, "q0": q0, "scales": s}])


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_cpu_oracle(hip, oracle):
    """three heights, S = 3, T = 4, one merged launch, against one oracle per height"""
    human, q0, scales, hidx = batch("smplx", "unitree_g1", 3, 4, seed=44)
    assert len(set(hidx.tolist())) == 3
    q, ns, st = solver(hip, "smplx", "unitree_g1").retarget_streams(q0, human, scales=scales)
    assert not st.any()
    for s in range(3):
        su = get_setup("smplx", "unitree_g1", float(HEIGHTS[hidx[s]]))
        q_o, ns_o, st_o = oracle.retarget_streams(su.mb, su.ts, q0[s:s + 1], human[s:s + 1])
        assert not st_o.any() and np.array_equal(ns[s:s + 1], ns_o), s
        joint = np.abs(q[s, :, 7:] - q_o[0, :, 7:]).max()
        pos = np.abs(q[s, :, :3] - q_o[0, :, :3]).max()
        qa, qb = q[s, :, 3:7], q_o[0, :, 3:7]
        rot = np.abs(qa - np.sign(np.sum(qa * qb, axis=-1, keepdims=True)) * qb).max()
        print(s, joint, pos, rot)
        assert joint <= TOL_RAD and pos <= TOL_POS and rot <= TOL_RAD, (s, joint, pos, rot)


def test_shim_heights_and_scales(hip):
    """GeneralMotionRetargeting.retarget_streams(heights=) is the launch with scale_rows of those heights, targets and errors
    included; scales= takes the rows themselves."""
    from general_motion_retargeting_amd import GeneralMotionRetargeting
    human, q0, scales, hidx = batch("smplx", "unitree_g1", 8, 5, seed=21)
    g = GeneralMotionRetargeting("smplx", "unitree_g1", actual_human_height=1.8)      # (whatever it was built for)
    ref = per_height(hip, "smplx", "unitree_g1", human, q0, hidx)
    same(g.retarget_streams(human, heights=HEIGHTS[hidx], want_targets=True, want_errors=True), ref)
    same(g.retarget_streams(human, scales=scales, want_targets=True, want_errors=True), ref)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_dataset_one_job_for_all_heights(hip, tmp_path, monkeypatch):
    """Six clips of three subjects and two genders, 2 to 90 frames: GMR_DATASET_HEIGHTS=groups (one solver and job per height)
    and the default (one solver, one job, scale rows) write the same bytes; with library= the merged run hands over one job."""
    from general_motion_retargeting_amd import dataset
    models = sx.write_models(tmp_path / "models")
    betas = np.random.default_rng(8).normal(0, 0.5, size=(3, 16))
    spec = [(90, 120.0, 0, "neutral"), (2, 30.0, 1, "female"), (47, 59.94, 2, "neutral"), (33, 30.0, 0, "neutral"), (61, 100.0, 1, "female"),
            (18, 30.0, 2, "neutral")]
    raws = [sx.clip(N, fps, 60 + i, g, betas[b]) for i, (N, fps, b, g) in enumerate(spec)]
    seen = []
    orig = dataset.DevicePost.run
    monkeypatch.setattr(dataset.DevicePost, "run", lambda self, jobs, *a, **k: (seen.append(len(jobs)), orig(self, jobs, *a, **k))[1])
    merged, library = dataset.retarget_smplx_loaded(raws, models, "unitree_g1", library=True)
    assert seen == [1] and library is not None and library.num_clips == 6
    monkeypatch.setenv("GMR_DATASET_HEIGHTS", "groups")
    groups = dataset.retarget_smplx_loaded(raws, models, "unitree_g1")
    assert seen == [1, 3]
    lens = [len(m["dof_pos"]) for m in merged]
    print("frames", lens)
    assert min(lens) >= 1 and max(lens) <= 90
    for i, (a, b) in enumerate(zip(merged, groups)):
        assert set(a) == set(b)
        for key in a:
            assert pickle.dumps(a[key]) == pickle.dumps(b[key]), (i, key)
    with pytest.raises(ValueError, match="one job"):
        dataset.retarget_smplx_loaded(raws, models, "unitree_g1", library=True)


def test_retarget_clips_with_one_height_per_clip(hip):
    from general_motion_retargeting_amd import dataset
    human, _, _, hidx = batch("smplx", "unitree_g1", 8, 5, seed=21)
    clips = [human[s, : 5 - s % 3] for s in range(8)]
    fps = [30.0] * 8
    heights = HEIGHTS[hidx]
    got = dataset.retarget_clips("smplx", "unitree_g1", clips, fps, actual_human_height=list(heights))
    for h in np.unique(heights):
        ids = np.nonzero(heights == h)[0]
        ref = dataset.retarget_clips("smplx", "unitree_g1", [clips[i] for i in ids], [30.0] * len(ids), actual_human_height=float(h))
        for i, r in zip(ids, ref):
            for key in r:
                assert pickle.dumps(got[i][key]) == pickle.dumps(r[key]), (i, key)
    # retarget_mixed: per-stream heights in a group
    q, ns, st = dataset.retarget_mixed([{"src_human": "smplx", "tgt_robot": "unitree_g1", "human": human, "actual_human_height": heights}])[0]
    ref = per_height(hip, "smplx", "unitree_g1", human, np.broadcast_to(get_setup().model.qpos0, (8, q.shape[2])).copy(), hidx)
    assert not st.any() and _bits(q, ref[0]) and _bits(ns, ref[1])
