"""-m gpu: per-frame joint velocity limits in the QP box (gmr_solver_set_frame_velocity_limits), on every launch path.

The reference is tests/frame_limit_mirror.py -- vel_limit_mirror's loop with the frame window applied last to build_qp's box,
theta0 taken at the top of each frame; tests/test_ik_frame_limits_host.py shows on the CPU that every case here is fit for
the comparison (the two CPU solvers agree to 1e-12, at most 20 pivoting rounds, no stop decision within 1e-6 of its tolerance,
a variable on a frame bound in every bounded frame).  The bound on max |q - q_mirror| is the one of the per-solve tests for
bound-heavy input, 1e-8 (vel_limit_mirror.TOL), with the mirror's solve counts.

What the feature promises is checked without a mirror as well: |theta_t - theta_{t-1}| <= w_h (1 + 1e-12) on the device's
qpos for every bounded frame, and the same input without the limit exceeds it by far.
"""
import pickle

import numpy as np
import pytest

import frame_limit_mirror as fm
import vel_limit_mirror as vm

pytestmark = pytest.mark.gpu

TOL = fm.TOL
QUEUED_S = 2600                  # more streams than the throughput kernel's resident wavefronts: the queued dispatch takes over


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _solver(hip, monkeypatch, su, shape, vmax, vmax_solve=None):
    """A solver that serves `shape` (as tests/test_ik_variants.py forces them) with the frame table `vmax` at 30 fps (None:
    never set) and the per-solve limit `vmax_solve` (None: never set)."""
    if shape == "onewave":
        monkeypatch.setenv("GMR_IK_NO_WIDE", "1")
    try:
        sol = hip.Solver(su.mb, su.ts)
    finally:
        monkeypatch.delenv("GMR_IK_NO_WIDE", raising=False)
    sol.set_waves(4 if shape == "latency" else 1)
    if vmax is not None:
        sol.set_frame_velocity_limit(vmax, fm.FRAME_DT)
    if vmax_solve is not None:
        sol.set_velocity_limit(np.full(sol.nv - 6, vmax_solve))
    return sol


def _flags(hip, case):
    return hip.FLAG_FRAME_LIMIT_FIRST if case.first_bounded else 0


def _check(tag, out, ref, tol=TOL):
    q_h, ns_h, st_h = out[:3]
    q_m, ns_m = ref
    assert (st_h == 0).all(), (tag, st_h)
    same = np.array_equal(ns_h, ns_m)
    err = float(np.abs(q_h - q_m).max())
    print(f"{tag}: max |q - q_mirror| = {err:.3e} (tolerance {tol:g}), solves/frame {ns_h.sum() / ns_h[..., 0].size:.2f}, counts equal: {same}")
    assert same, f"{tag}: solve counts differ from the mirror's"
    assert err <= tol, (tag, err)


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _holds(tag, case, q, q0):
    """the invariant on the device's qpos, every bounded frame"""
    w = fm.window_of(fm.setup_of(case.robot).mb, case.vmax())
    worst = float(fm.excess(q, q0, w, case.first_bounded).max())
    print(f"{tag}: largest |theta_t - theta_(t-1)| - w (1 + 1e-12) = {worst:.3e}")
    assert worst <= 0.0, (tag, worst)


# ---- 1: every instance a launch can end in ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["latency", "onewave", "throughput"])
@pytest.mark.parametrize("name", ["f_g1", "f_t1"])
def test_uniform_limit_matches_mirror(hip, oracle, monkeypatch, name, shape):
    """0.6 rad/s at 30 fps on every hinge, frame 0 free.  G1: <36, 4, TREE_SMALL>, <36, 1, TREE_SMALL> and the throughput
    kernel, one workgroup per stream; bvh -> booster_t1 likewise in its class."""
    case = fm.CASES[name]
    su = fm.setup_of(case.robot)
    human, q0 = fm.make_input(case)
    sol = _solver(hip, monkeypatch, su, shape, case.vmax())
    table, dt = sol.frame_velocity_limit()
    assert np.array_equal(table, case.vmax()) and dt == fm.FRAME_DT
    out = sol.retarget_streams(q0, human)
    sol.close()
    _check(f"{name} {shape}", out, fm.stacked(fm.mirror_runs(oracle, case)))
    _holds(f"{name} {shape}", case, out[0], q0)


@pytest.mark.parametrize("frames_per_item", [1, 2])
def test_queued_dispatch(hip, oracle, frames_per_item):
    """The throughput kernel serving (stream, 1 or 2 frames) items from its queue: item boundaries fall inside every stream, so
    theta0 of an item's first frame is the q_out row ANOTHER item wrote.  The bits of one workgroup per stream, and the
    mirror's result on the last copy of the four generated streams."""
    case = fm.CASES["f_g1"]
    su = fm.setup_of(case.robot)
    bh, bq = fm.make_input(case)
    pick = np.arange(QUEUED_S) % case.S
    human, q0 = bh[pick].copy(), bq[pick].copy()
    sol = hip.Solver(su.mb, su.ts)
    sol.set_waves(1)
    sol.set_frame_velocity_limit(case.vmax(), fm.FRAME_DT)
    sol.set_dispatch(0)
    q_d, ns_d, st_d = sol.retarget_streams(q0, human)
    sol.set_dispatch(frames_per_item)
    q_q, ns_q, st_q = sol.retarget_streams(q0, human)
    sol.close()
    assert (st_d == 0).all() and _bits(st_d, st_q) and _bits(ns_d, ns_q) and _bits(q_d, q_q)
    n = case.S
    assert (pick[-n:] == np.arange(n)).all()
    _check(f"f_g1 queued x{frames_per_item}", (q_q[-n:], ns_q[-n:], st_q[-n:]), fm.stacked(fm.mirror_runs(oracle, case)))
    _holds(f"f_g1 queued x{frames_per_item}", case, q_q, q0)


# ---- 2: the invariant, and that the bound is what holds it ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["latency", "onewave", "throughput"])
def test_bound_holds_between_frames_and_only_with_the_limit(hip, monkeypatch, shape):
    """|theta_t - theta_(t-1)| <= w_h (1 + 1e-12) for every frame t >= 1 of the device's qpos under the mixed table; the same
    input without the limit exceeds w by more than 0.1 rad."""
    case = fm.CASES["f_g1_mixed"]
    su = fm.setup_of(case.robot)
    human, q0 = fm.make_input(case)
    w = fm.window_of(su.mb, case.vmax())
    sol = _solver(hip, monkeypatch, su, shape, case.vmax())
    q, ns, st = sol.retarget_streams(q0, human)
    sol.set_frame_velocity_limit(None)
    q_off, ns_off, st_off = sol.retarget_streams(q0, human)
    sol.close()
    assert (st == 0).all() and (st_off == 0).all()
    worst, worst_off = float(fm.excess(q, q0, w).max()), float(fm.excess(q_off, q0, w).max())
    print(f"{shape}: largest step - w: {worst:.3e} with the limit, {worst_off:.3e} without")
    assert worst <= 0.0, worst
    assert worst_off > 0.1, "the input does not exceed the bound without the limit: the case tests nothing"


# ---- 3: a table that differs from hinge to hinge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shapes", [("f_g1_mixed", ("latency", "onewave", "throughput")),
                                         ("f_t1_mixed", ("latency", "onewave", "throughput")),
                                         ("f_dense_mixed", ("latency", "throughput"))])
def test_mixed_table_matches_mirror(hip, oracle, monkeypatch, name, shapes):
    """0.6 / 12 / none in turn by hinge: a table read at the wrong lane fails here.  The dense robot's three hinges without a
    range have the window as their only bound -- set_waves(4) is its <36, 4, TREE> instance, set_waves(1) its <36, 1, DENSE>
    one (it does not fit the throughput kernel)."""
    case = fm.CASES[name]
    su = fm.setup_of(case.robot)
    human, q0 = fm.make_input(case)
    ref = fm.stacked(fm.mirror_runs(oracle, case))
    for shape in shapes:
        sol = _solver(hip, monkeypatch, su, shape, case.vmax())
        out = sol.retarget_streams(q0, human)
        sol.close()
        _check(f"{name} {shape}", out, ref)
        _holds(f"{name} {shape}", case, out[0], q0)


# ---- 4: off is off ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["latency", "onewave", "throughput"])
def test_no_limit_is_byte_equal(hip, monkeypatch, shape):
    """Never set, set to inf everywhere, set to 0.6 and cleared with NULL: the same bytes in qpos, nsolve, tgt_out, err_out --
    also with GMR_FLAG_FRAME_LIMIT_FIRST, which means nothing without a limit."""
    case = fm.CASES["f_g1"]
    su = fm.setup_of(case.robot)
    human, q0 = fm.make_input(case)
    nh = len(su.model.joint_names)
    outs = {}
    for how in ("never", "inf", "cleared"):
        sol = _solver(hip, monkeypatch, su, shape, {"never": None, "inf": np.full(nh, np.inf), "cleared": case.vmax()}[how])
        if how == "cleared":
            limited = sol.retarget_streams(q0, human)
            sol.set_frame_velocity_limit(None)
        table, dt = sol.frame_velocity_limit()
        assert np.isinf(table).all() and dt == 0.0
        outs[how] = sol.retarget_streams(q0, human, want_targets=True, want_errors=True)
        if how == "inf":
            outs["flag"] = sol.retarget_streams(q0, human, flags=hip.FLAG_FRAME_LIMIT_FIRST, want_targets=True, want_errors=True)
        sol.close()
    for how in ("inf", "cleared", "flag"):
        for a, b in zip(outs["never"], outs[how]):
            assert _bits(a, b), (shape, how)
    assert (outs["never"][2] == 0).all()
    assert np.abs(limited[0] - outs["never"][0]).max() > 1e-3        # (and the limit was on in between)


# ---- 5: frame 0 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["latency", "onewave", "throughput"])
def test_first_frame_is_free_without_the_flag_and_bounded_with_it(hip, oracle, monkeypatch, shape):
    case, first = fm.CASES["f_g1"], fm.CASES["f_g1_first"]
    su = fm.setup_of(case.robot)
    human, q0 = fm.make_input(case)
    sol = _solver(hip, monkeypatch, su, shape, case.vmax())
    free = sol.retarget_streams(q0, human)
    bounded = sol.retarget_streams(q0, human, flags=hip.FLAG_FRAME_LIMIT_FIRST)
    sol.set_frame_velocity_limit(None)
    off = sol.retarget_streams(q0, human)
    sol.close()
    assert _bits(free[0][:, 0], off[0][:, 0]) and _bits(free[1][:, 0], off[1][:, 0])       # frame 0 of the free run IS the unlimited one
    assert not _bits(free[0][:, 1], off[0][:, 1])
    _check(f"f_g1_first {shape}", bounded, fm.stacked(fm.mirror_runs(oracle, first)))
    _holds(f"f_g1_first {shape}", first, bounded[0], q0)
    w = fm.window_of(su.mb, case.vmax())
    assert float(fm.excess(free[0], q0, w, True)[:, 0].max()) > 0.1                        # (frame 0 of the free run is far outside)


@pytest.mark.parametrize("shape", ["latency", "throughput"])
def test_start_outside_range_walks_back_by_w_per_frame(hip, oracle, monkeypatch, shape):
    """Left knee 0.1 rad above, right ankle pitch 0.07 below its range, q0 declared the previous frame: the window is the bound
    that always holds, so each of the two comes back by exactly w = 0.02 per frame until it is inside."""
    case = fm.CASES["f_g1_outside"]
    su = fm.setup_of(case.robot)
    human, q0 = fm.make_input(case)
    sol = _solver(hip, monkeypatch, su, shape, case.vmax())
    out = sol.retarget_streams(q0, human, flags=_flags(hip, case))
    sol.close()
    _check(f"f_g1_outside {shape}", out, fm.stacked(fm.mirror_runs(oracle, case)))
    _holds(f"f_g1_outside {shape}", case, out[0], q0)
    for h, d in vm.outside_hinges(su.model):
        assert fm.walk_back_error(out[0], q0, h, d) <= 1e-12, (h, d)


# ---- 6: the per-frame API ----------------------------------------------------------------------------------------------------------------
def test_retarget_per_frame_equals_clip_and_mirror(hip, oracle):
    """retarget() passes GMR_FLAG_FRAME_LIMIT_FIRST from its second call on: a per-frame loop, retarget_clip and the mirror
    agree on the same frames, and so does a clip continued after a first retarget() call."""
    from general_motion_retargeting_amd import GeneralMotionRetargeting, synth
    case = fm.CASES["f_g1"]
    su = fm.setup_of(case.robot)
    human, q0 = fm.make_input(case)
    assert np.array_equal(q0[0], su.model.qpos0)
    frames = synth.streams_to_dicts(su.tt, human[0, :4])
    make = lambda: GeneralMotionRetargeting(*fm.G1[:2], actual_human_height=fm.G1[2], frame_velocity_limit=fm.VMAX, fps=fm.FPS)   # noqa: E731
    g = make()
    per_frame = np.stack([g.retarget(f) for f in frames])
    counts = g.last_num_solves
    gc = make()
    clip = gc.retarget_clip(frames)
    g2 = make()
    mixed = np.concatenate([g2.retarget(frames[0])[None], g2.retarget_clip(frames[1:])])
    g2.setup_retarget_configuration()                                  # a fresh configuration: the next frame is free again
    assert _bits(g2.retarget(frames[0]), per_frame[0])
    # (a launch per frame starts the pivoting cold, a clip carries the bound sets from frame to frame: the same QPs by another
    #  pivot sequence, so the three agree to rounding, not in their bits)
    ref = fm.mirror_runs(oracle, case)[0]
    for tag, q in (("retarget() x 4", per_frame), ("retarget_clip", clip), ("retarget() + retarget_clip", mixed)):
        err = float(np.abs(q - ref.q[:4]).max())
        print(f"{tag}: max |q - q_mirror| = {err:.3e}, against the per-frame loop {np.abs(q - per_frame).max():.3e}")
        assert err <= TOL, (tag, err)
    assert np.array_equal(counts, ref.nsolve[3]) and np.array_equal(gc.last_num_solves, ref.nsolve[:4])
    w = fm.window_of(su.mb, case.vmax())
    assert float(fm.excess(per_frame[None], q0[:1], w).max()) <= 0.0


# ---- 7: windows of frames ----------------------------------------------------------------------------------------------------------------
def test_two_windows_equal_one_launch(hip):
    """gmr_retarget_group_window_dev, frames [0, 2) then [2, 6): the second window continues from q_out[1] under the bound,
    with no flag; the bytes of one launch."""
    case = fm.CASES["f_g1"]
    su = fm.setup_of(case.robot)
    bh, bq = fm.make_input(case)
    pick = np.arange(8) % case.S
    human, q0 = bh[pick].copy(), bq[pick].copy()
    S, T = human.shape[:2]
    sol = hip.Solver(su.mb, su.ts)
    sol.set_waves(1)
    sol.set_frame_velocity_limit(case.vmax(), fm.FRAME_DT)
    q1, ns1, st1 = sol.retarget_streams(q0, human)
    st = hip.Stream()
    b = [hip.DeviceBuffer.from_host(q0), hip.DeviceBuffer.from_host(human), hip.DeviceBuffer(S * T * sol.nq * 8), hip.DeviceBuffer(S * T * 8),
         hip.DeviceBuffer(S * 4)]
    job = [(sol, S, T, b[0], b[1], None, b[2], b[3], b[4])]
    for win in ((0, 2), (2, T)):
        hip.retarget_group_dev(job, 0, st, window=win)
    st.sync()
    q2, ns2, st2 = b[2].to_host((S, T, sol.nq), np.float64), b[3].to_host((S, T, 2), np.int32), b[4].to_host((S,), np.int32)
    for x in b:
        x.free()
    sol.close()
    assert (st1 == 0).all() and _bits(q1, q2) and _bits(ns1, ns2) and _bits(st1, st2)
    _holds("windows", case, q2, q0)


# ---- 8: a group of two jobs with two tables --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [0, 1])
def test_group_jobs_keep_their_own_tables(hip, waves):
    """G1 under the uniform and T1 under the mixed frame table in one gmr_retarget_group: every job's rows are the bytes of its
    solver's own launch.  waves = 0: two launches of the latency shape; waves = 1: ONE launch of the throughput kernel's group
    instance, whose job table names each solver's image."""
    jobs, own = [], []
    for name in ("f_g1", "f_t1_mixed"):
        case = fm.CASES[name]
        su = fm.setup_of(case.robot)
        human, q0 = fm.make_input(case)
        sol = hip.Solver(su.mb, su.ts)
        sol.set_waves(waves)
        sol.set_frame_velocity_limit(case.vmax(), fm.FRAME_DT)
        own.append(sol.retarget_streams(q0, human))
        jobs.append({"solver": sol, "human": human, "q0": q0})
    outs = hip.retarget_group(jobs)
    for (q, ns, st), (q1, ns1, st1), name in zip(outs, own, ("f_g1", "f_t1_mixed")):
        assert (st == 0).all() and _bits(q, q1) and _bits(ns, ns1) and _bits(st, st1)
        _holds(f"group waves={waves} {name}", fm.CASES[name], q, fm.make_input(fm.CASES[name])[1])
    # T1 under G1's uniform table is something else: the tables did not leak into each other
    case = fm.CASES["f_t1"]
    other = hip.Solver(fm.setup_of(case.robot).mb, fm.setup_of(case.robot).ts)
    other.set_waves(waves)
    other.set_frame_velocity_limit(case.vmax(), fm.FRAME_DT)
    assert not _bits(other.retarget_streams(*fm.make_input(case)[::-1])[0], outs[1][0])
    other.close()
    for j in jobs:
        j["solver"].close()


def test_group_job_without_a_limit_is_not_changed_by_a_neighbour_with_one(hip):
    """G1 under the frame limit and T1 with none in ONE launch of the group instance that applies windows: T1's window is +inf
    there, and its rows are the bytes of its own launch, which runs the instance without windows."""
    jobs, own = [], []
    for name, limited in (("f_g1", True), ("f_t1", False)):
        case = fm.CASES[name]
        su = fm.setup_of(case.robot)
        human, q0 = fm.make_input(case)
        sol = hip.Solver(su.mb, su.ts)
        sol.set_waves(1)
        if limited:
            sol.set_frame_velocity_limit(case.vmax(), fm.FRAME_DT)
        own.append(sol.retarget_streams(q0, human))
        jobs.append({"solver": sol, "human": human, "q0": q0})
    outs = hip.retarget_group(jobs)
    for (q, ns, st), (q1, ns1, st1) in zip(outs, own):
        assert (st == 0).all() and _bits(q, q1) and _bits(ns, ns1) and _bits(st, st1)
    for j in jobs:
        j["solver"].close()


# ---- 9: the scaled path, both limits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [4, 1])
def test_scaled_streams_with_limit(hip, oracle, waves):
    """retarget_streams(heights=): one height per stream as scale rows; the mirror runs stream s under the task set of an
    object built for heights[s]."""
    from general_motion_retargeting_amd import GeneralMotionRetargeting
    case = fm.CASES["f_g1_scaled"]
    human, q0 = fm.make_input(case)
    g = GeneralMotionRetargeting(*fm.G1[:2], frame_velocity_limit=fm.VMAX, fps=fm.FPS)
    g.hip_solver.set_waves(waves)
    out = g.retarget_streams(human, q0=q0, heights=np.array(case.heights))
    g.hip_solver.close()
    _check(f"f_g1_scaled waves={waves}", out, fm.stacked(fm.mirror_runs(oracle, case)))
    _holds(f"f_g1_scaled waves={waves}", case, out[0], q0)


@pytest.mark.parametrize("shape", ["latency", "onewave", "throughput"])
def test_both_limits_together(hip, oracle, monkeypatch, shape):
    """3 pi per solve and 0.6 rad/s per frame: the per-solve clamp first, the frame window last."""
    case = fm.CASES["f_g1_both"]
    su = fm.setup_of(case.robot)
    human, q0 = fm.make_input(case)
    sol = _solver(hip, monkeypatch, su, shape, case.vmax(), case.vmax_solve)
    out = sol.retarget_streams(q0, human)
    sol.close()
    _check(f"f_g1_both {shape}", out, fm.stacked(fm.mirror_runs(oracle, case)))
    _holds(f"f_g1_both {shape}", case, out[0], q0)


# ---- 10: the dataset path ---------------------------------------------------------------------------------------------------------------
def test_dataset_clips_take_the_limit(hip):
    from general_motion_retargeting_amd import dataset
    case = fm.CASES["f_g1"]
    su = fm.setup_of(case.robot)
    human, _ = fm.make_input(case)
    clips = [human[0, :5], human[1, :6]]
    motions = dataset.retarget_clips(*fm.G1[:2], clips, [fm.FPS, fm.FPS], actual_human_height=fm.G1[2], frame_velocity_limit=fm.VMAX)
    sol = hip.Solver(su.mb, su.ts)
    sol.set_frame_velocity_limit(case.vmax(), fm.FRAME_DT)
    plain = hip.Solver(su.mb, su.ts)
    for clip, md in zip(clips, motions):
        q, ns, st = sol.retarget_streams(su.model.qpos0[None], clip[None])
        assert st[0] == 0
        want = q[0][:, 7:].astype(md["dof_pos"].dtype)
        assert pickle.dumps(np.ascontiguousarray(md["dof_pos"])) == pickle.dumps(np.ascontiguousarray(want))
        q_off = plain.retarget_streams(su.model.qpos0[None], clip[None])[0]
        assert np.abs(q_off[0] - q[0]).max() > 1e-3
    sol.close()
    plain.close()


def test_dataset_refuses_mixed_fps_and_chunks(hip):
    from general_motion_retargeting_amd import GeneralMotionRetargeting, chunking, dataset
    case = fm.CASES["f_g1"]
    human, _ = fm.make_input(case)
    clips = [human[0, :5], human[1, :6]]
    with pytest.raises(ValueError, match="share one fps"):
        dataset.retarget_clips(*fm.G1[:2], clips, [30.0, 60.0], actual_human_height=fm.G1[2], frame_velocity_limit=fm.VMAX)
    assert len(dataset.retarget_clips(*fm.G1[:2], clips, [30.0, 60.0], actual_human_height=fm.G1[2])) == 2      # (fine without the limit)
    spec = chunking.ChunkSpec(frames=3, warmup=1)
    with pytest.raises(ValueError, match="chunk"):
        dataset.retarget_clips(*fm.G1[:2], clips, [30.0, 30.0], actual_human_height=fm.G1[2], frame_velocity_limit=fm.VMAX, chunk=spec)
    g = GeneralMotionRetargeting(*fm.G1[:2], actual_human_height=fm.G1[2], frame_velocity_limit=fm.VMAX, fps=fm.FPS)
    with pytest.raises(ValueError, match="chunk"):
        g.retarget_clip(np.asarray(human[0]), chunk=spec)
    with pytest.raises(ValueError, match="chunk"):                     # and below the Python front doors: the runner itself
        chunking.retarget_chunked_host(g.hip_solver, np.asarray(human[:1]), np.asarray(g.model.qpos0)[None], None, 0, spec)
    g.set_frame_velocity_limit(None)
    assert g.retarget_clip(np.asarray(human[0]), chunk=spec).shape == (case.T, g.model.nq)


# ---- host-side argument checks (the only failures provoked on purpose) --------------------------------------------------------------------
def test_setter_rejects_bad_arguments(hip):
    su = fm.setup_of(fm.G1)
    nh = len(su.model.joint_names)
    sol = hip.Solver(su.mb, su.ts)
    good = np.full(nh, 5.0)
    good[2] = np.inf
    sol.set_frame_velocity_limit(good, 0.01)
    for bad in (np.full(nh + 1, 5.0), np.full(nh - 1, 5.0)):
        with pytest.raises(hip.GmrHipError, match="hinges"):
            sol.set_frame_velocity_limit(bad, 0.01)
    for v in (0.0, -2.0, np.nan):
        bad = good.copy()
        bad[7] = v
        with pytest.raises(hip.GmrHipError, match="hinge 7"):
            sol.set_frame_velocity_limit(bad, 0.01)
    for dt in (0.0, -0.01, np.inf, np.nan):
        with pytest.raises(hip.GmrHipError, match="frame_dt"):
            sol.set_frame_velocity_limit(good, dt)
    table, dt = sol.frame_velocity_limit()
    assert np.array_equal(table, good) and dt == 0.01                 # a rejected call changes nothing
    sol.set_frame_velocity_limit(np.full(nh, np.inf), np.nan)         # no finite entry: frame_dt is not looked at
    assert sol.frame_velocity_limit()[1] == 0.0
    assert sol.lds_bytes == hip.Solver(su.mb, su.ts).lds_bytes
    sol.close()
