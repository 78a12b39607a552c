"""-m gpu: per-frame body weights and missing bodies (gmr_retarget_streams_weighted, gmr_retarget_group_weighted*), on every
launch path.

The reference is tests/body_weight_mirror.py -- vel_limit_mirror's loop with the task weights of each frame multiplied by the
multiplier of the task's human body, missing bodies (multiplier 0) out of the targets and out of the residual norm;
tests/test_ik_body_weights_host.py shows on the CPU that every case here is fit for the comparison (the two CPU solvers agree to
1e-12, no stop decision within 1e-6 of its tolerance, the weights move the result by up to 3 rad and most solve counts).  The
bound on max |q - q_mirror| is vel_limit_mirror.TOL, 1e-8, with the mirror's solve counts.

Without a mirror: missing rows are never read (NaN, zeros and 1e300 there give the same bytes), the neutral forms (no array,
weights of ones) are the bytes of the entry points without weights, constant positive weights are the bytes of a solver packed
with the products, and windows, slices and group launches are the bytes of one launch.
"""
import ctypes as C
import pickle

import numpy as np
import pytest

import body_weight_mirror as bw
import frame_limit_mirror as fm

pytestmark = pytest.mark.gpu

TOL = bw.TOL
ERR_TOL = 1e-10
GMR_ERR_ARG = -1
QUEUED_S = 2600                  # more streams than the throughput kernel's resident wavefronts: the queued dispatch takes over
SHAPES = ["latency", "onewave", "throughput"]


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _solver(hip, monkeypatch, su, shape, ts=None, vmax_solve=None, vmax_frame=None):
    """A solver that serves `shape` (as tests/test_ik_frame_limits.py forces them), of `ts` in place of the setup's task set."""
    if shape == "onewave":
        monkeypatch.setenv("GMR_IK_NO_WIDE", "1")
    try:
        sol = hip.Solver(su.mb, su.ts if ts is None else ts)
    finally:
        monkeypatch.delenv("GMR_IK_NO_WIDE", raising=False)
    sol.set_waves(4 if shape == "latency" else 1)
    if vmax_frame is not None:
        sol.set_frame_velocity_limit(vmax_frame, fm.FRAME_DT)
    if vmax_solve is not None:
        sol.set_velocity_limit(vmax_solve)
    return sol


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


def _all_bits(tag, a, b):
    for name, x, y in zip(("qpos", "nsolve", "status", "tgt_out", "err_out"), a, b):
        assert _bits(x, y), (tag, name)


def _missing(case, w):
    su = bw.setup_of(case.robot)
    return np.stack([[bw.missing_rows(su.ts, w[s, t]) for t in range(w.shape[1])] for s in range(w.shape[0])])


def _flags(hip, ground):
    return hip.FLAG_OFFSET_TO_GROUND if ground else 0


# ---- 1: every instance a launch can end in, against the mirror ---------------------------------------------------------------------------
@pytest.mark.parametrize("ground", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["w_g1", "w_t1"])
def test_weights_match_mirror(hip, oracle, monkeypatch, name, shape, ground):
    case = bw.CASES[name]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    w = bw.make_weights(case, ground)
    sol = _solver(hip, monkeypatch, su, shape)
    out = sol.retarget_streams(q0, human, flags=_flags(hip, ground), weights=w, want_targets=True, want_errors=True)
    sol.close()
    runs = bw.mirror_runs(oracle, case, ground=ground)
    _check(f"{name} {shape} ground={ground}", out, bw.stacked(runs))
    miss = _missing(case, w)
    assert miss.any() and np.isnan(out[3][miss]).all() and np.isfinite(out[3][~miss & ~np.isnan(human[..., 0])]).all()
    derr = float(np.abs(out[4] - np.stack([r.err for r in runs])).max())
    print(f"{name} {shape} ground={ground}: max |err_out - masked norm| = {derr:.3e}")
    assert derr <= ERR_TOL, derr


def test_dense_robot_on_one_wavefront(hip, oracle, monkeypatch):
    """the <36, 1, QP_DENSE> instance: a robot that does not decompose"""
    case = bw.CASES["w_dense"]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    sol = _solver(hip, monkeypatch, su, "onewave")
    out = sol.retarget_streams(q0, human, weights=bw.make_weights(case))
    sol.close()
    _check("w_dense onewave", out, bw.stacked(bw.mirror_runs(oracle, case)))


# ---- 2: the throughput kernel's queue ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames_per_item", [1, 2])
def test_queued_dispatch(hip, oracle, frames_per_item):
    """(stream, 1 or 2 frames) items: the row of a frame is found by its index in the stream, whichever item serves it.  The
    bytes of one workgroup per stream, and the mirror's result on the last copy of the four generated streams."""
    case = bw.CASES["w_g1"]
    su = bw.setup_of(case.robot)
    bh, bq = bw.make_input(case)
    pick = np.arange(QUEUED_S) % case.S
    human, q0, w = bh[pick].copy(), bq[pick].copy(), bw.make_weights(case)[pick].copy()
    sol = hip.Solver(su.mb, su.ts)
    sol.set_waves(1)
    sol.set_dispatch(0)
    q_d, ns_d, st_d = sol.retarget_streams(q0, human, weights=w)
    sol.set_dispatch(frames_per_item)
    q_q, ns_q, st_q = sol.retarget_streams(q0, human, weights=w)
    sol.close()
    assert (st_d == 0).all() and _bits(st_d, st_q) and _bits(ns_d, ns_q) and _bits(q_d, q_q)
    n = case.S
    assert (pick[-n:] == np.arange(n)).all()
    _check(f"w_g1 queued x{frames_per_item}", (q_q[-n:], ns_q[-n:], st_q[-n:]), bw.stacked(bw.mirror_runs(oracle, case)))


# ---- 3: missing rows are never read --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ground", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_missing_rows_are_never_read(hip, monkeypatch, shape, ground):
    case = bw.CASES["w_g1"]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    w = bw.make_weights(case, ground)
    miss = _missing(case, w)
    sol = _solver(hip, monkeypatch, su, shape)
    outs = [sol.retarget_streams(q0, bw.with_missing_rows(case, human, w, fill), flags=_flags(hip, ground), weights=w, want_targets=True,
                                 want_errors=True) for fill in (np.nan, 0.0, 1e300)]
    plain = sol.retarget_streams(q0, bw.with_missing_rows(case, human, w, np.nan), flags=_flags(hip, ground))
    sol.close()
    assert (outs[0][2] == 0).all()
    for o in outs[1:]:
        for k in (0, 1, 2, 4):
            assert _bits(o[k], outs[0][k]), (shape, k)
    for o in outs:
        assert np.isnan(o[3][miss]).all() and np.isfinite(o[3][~miss & ~np.isnan(human[..., 0])]).all()
    assert (plain[2] != 0).any(), "NaN rows without weights fail the stream, as ever"


# ---- 4: the neutral forms are the bytes of the entry points without weights ----------------------------------------------------------------
def _weighted_entry(hip, sol, q0, human, weights, flags):
    """gmr_retarget_streams_weighted itself, with a null or a given weight array (Solver.retarget_streams takes the entry point
    without weights when it has none)"""
    S, T = human.shape[:2]
    q0, human = np.ascontiguousarray(q0), np.ascontiguousarray(human)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    out = (np.zeros((S, T, sol.nq)), np.zeros((S, T, 2), np.int32), np.zeros(S, np.int32), np.zeros((S, T, sol.nhuman, 7)), np.zeros((S, T, 2)))
    hip.check(hip.lib().gmr_retarget_streams_weighted(sol.handle, S, T, p(q0), p(human), None, None, p(weights), int(flags), *(p(o) for o in out)))
    return out


@pytest.mark.parametrize("limit", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_neutral_forms_are_byte_equal(hip, monkeypatch, shape, limit):
    case = bw.CASES["w_g1"]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    nh = len(su.model.joint_names)
    sol = _solver(hip, monkeypatch, su, shape, vmax_frame=np.full(nh, fm.VMAX) if limit else None)
    for ground in (False, True):
        old = sol.retarget_streams(q0, human, flags=_flags(hip, ground), want_targets=True, want_errors=True)
        assert (old[2] == 0).all()
        _all_bits(f"{shape} null", _weighted_entry(hip, sol, q0, human, None, _flags(hip, ground)), old)
        ones = np.ones(human.shape[:3])
        _all_bits(f"{shape} ones", sol.retarget_streams(q0, human, flags=_flags(hip, ground), weights=ones, want_targets=True, want_errors=True), old)
    sol.close()


# ---- 5: without a mirror: constant weights are a solver packed with the products ------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["w_g1", "w_t1"])
def test_constant_weights_are_a_solver_packed_with_the_products(hip, monkeypatch, name, shape):
    case = bw.CASES[name]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    nhum = int(su.ts["nhuman"][0])
    m = np.array([(0.25, 2.5, 1.0)[b % 3] for b in range(nhum)])      # (a table indexed by the wrong lane shows)
    sol = _solver(hip, monkeypatch, su, shape)
    got = sol.retarget_streams(q0, human, weights=np.broadcast_to(m, human.shape[:3]), want_targets=True, want_errors=True)
    plain = sol.retarget_streams(q0, human)
    sol.close()
    folded = _solver(hip, monkeypatch, su, shape, ts=bw.weighted_taskset(su.ts, m))
    want = folded.retarget_streams(q0, human, want_targets=True, want_errors=True)
    folded.close()
    assert (want[2] == 0).all()
    _all_bits(f"{name} {shape}", got, want)
    assert not _bits(got[0], plain[0])


# ---- 6: windows, slices, groups ---------------------------------------------------------------------------------------------------------------
def test_two_windows_equal_one_launch(hip):
    case = bw.CASES["w_g1"]
    su = bw.setup_of(case.robot)
    bh, bq = bw.make_input(case)
    pick = np.arange(8) % case.S
    human, q0, w = bh[pick].copy(), bq[pick].copy(), bw.make_weights(case)[pick].copy()
    S, T = human.shape[:2]
    sol = hip.Solver(su.mb, su.ts)
    sol.set_waves(1)
    q1, ns1, st1 = sol.retarget_streams(q0, human, weights=w)
    st = hip.Stream()
    b = [hip.DeviceBuffer.from_host(q0), hip.DeviceBuffer.from_host(human), hip.DeviceBuffer(S * T * sol.nq * 8), hip.DeviceBuffer(S * T * 8),
         hip.DeviceBuffer(S * 4), hip.DeviceBuffer.from_host(w)]
    job = [(sol, S, T, b[0], b[1], None, b[2], b[3], b[4])]
    for win in ((0, 2), (2, T)):
        hip.retarget_group_dev(job, 0, st, window=win, weights=[b[5]])
    st.sync()
    q2, ns2, st2 = b[2].to_host((S, T, sol.nq), np.float64), b[3].to_host((S, T, 2), np.int32), b[4].to_host((S,), np.int32)
    for x in b:
        x.free()
    sol.close()
    assert (st1 == 0).all() and _bits(q1, q2) and _bits(ns1, ns2) and _bits(st1, st2)


@pytest.mark.parametrize("slices", [3, -2])
def test_sliced_and_windowed_host_paths_equal_one_launch(hip, slices):
    """gmr_retarget_group_weighted cutting the weight rows with the streams (3 slices) and with the frames (2 windows)"""
    case = bw.CASES["w_g1"]
    su = bw.setup_of(case.robot)
    bh, bq = bw.make_input(case)
    pick = np.arange(7) % case.S
    human, q0, w = bh[pick].copy(), bq[pick].copy(), bw.make_weights(case)[pick].copy()
    sol = hip.Solver(su.mb, su.ts)
    sol.set_waves(1)
    one = sol.retarget_streams(q0, human, weights=w)
    cut = hip.retarget_group([{"solver": sol, "human": human, "q0": q0, "weights": w}], 0, slices)[0]
    sol.close()
    assert (one[2] == 0).all()
    for a, c in zip(one, cut):
        assert _bits(a, c)


@pytest.mark.parametrize("waves", [4, 1])
def test_a_job_with_weights_next_to_one_without(hip, waves):
    """G1 with weights and T1 without in one gmr_retarget_group_weighted: every job's rows are the bytes of its own launch.
    waves = 4: two launches of the latency shape; waves = 1: ONE launch of the throughput kernel's weighted group instance,
    in which T1's multipliers are 1."""
    jobs, own = [], []
    for name, weighted in (("w_g1", True), ("w_t1", False)):
        case = bw.CASES[name]
        su = bw.setup_of(case.robot)
        human, q0 = bw.make_input(case)
        w = bw.make_weights(case) if weighted else None
        sol = hip.Solver(su.mb, su.ts)
        sol.set_waves(waves)
        own.append(sol.retarget_streams(q0, human, weights=w))
        jobs.append({"solver": sol, "human": human, "q0": q0, "weights": w})
    outs = hip.retarget_group(jobs)
    for (q, ns, st), (q1, ns1, st1) in zip(outs, own):
        assert (st == 0).all() and _bits(q, q1) and _bits(ns, ns1) and _bits(st, st1)
    unweighted = jobs[0]["solver"].retarget_streams(jobs[0]["q0"], jobs[0]["human"])
    assert not _bits(unweighted[0], outs[0][0])
    for j in jobs:
        j["solver"].close()


# ---- 7: scale rows and both velocity limits on top ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["latency", "throughput"])
def test_heights_case(hip, oracle, monkeypatch, shape):
    """one height per stream as scale rows next to the weights; the mirror runs stream s under the task set built for heights[s]"""
    from general_motion_retargeting_amd.ik_config import scale_rows
    from general_motion_retargeting_amd import GeneralMotionRetargeting
    case = bw.CASES["w_g1_heights"]
    human, q0 = bw.make_input(case)
    g = GeneralMotionRetargeting(*bw.G1[:2])
    g.hip_solver.set_waves(4 if shape == "latency" else 1)
    out = g.retarget_streams(human, q0=q0, heights=np.array(case.heights), weights=bw.make_weights(case))
    g.hip_solver.close()
    assert scale_rows(g._ik_config, np.array(case.heights)).shape == (case.S, human.shape[2])
    _check(f"w_g1_heights {shape}", out, bw.stacked(bw.mirror_runs(oracle, case)))


@pytest.mark.parametrize("shape", ["latency", "throughput"])
def test_both_limits_case(hip, oracle, monkeypatch, shape):
    case = bw.CASES["w_g1_both"]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    vs, vf = bw.limits_of(case)
    sol = _solver(hip, monkeypatch, su, shape, vmax_solve=vs, vmax_frame=vf)
    out = sol.retarget_streams(q0, human, weights=bw.make_weights(case))
    sol.close()
    _check(f"w_g1_both {shape}", out, bw.stacked(bw.mirror_runs(oracle, case)))


# ---- 8: evaluation only -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_eval_only_applies_the_weights(hip, oracle, monkeypatch, shape):
    case = bw.CASES["w_g1"]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    w = bw.make_weights(case)
    sol = _solver(hip, monkeypatch, su, shape)
    q, ns, st, tg, er = sol.retarget_streams(q0, human[:, :1], flags=hip.FLAG_EVAL_ONLY, weights=w[:, :1], want_targets=True, want_errors=True)
    sol.close()
    assert (st == 0).all() and (ns == 0).all() and _bits(q[:, 0], np.ascontiguousarray(q0))
    want = np.stack([bw.masked_errors(oracle, su.mb, su.ts, q0[s], human[s, 0], w[s, 0]) for s in range(case.S)])
    unmasked = np.stack([bw.masked_errors(oracle, su.mb, su.ts, q0[s], human[s, 0], np.where(w[s, 0] == 0, 1.0, w[s, 0])) for s in range(case.S)])
    d = float(np.abs(er[:, 0] - want).max())
    print(f"eval only {shape}: max |err_out - masked norm| = {d:.3e}; the unmasked norm is {np.abs(unmasked - want).max():.2f} away")
    assert d <= ERR_TOL and np.abs(unmasked - want).max() > 1e-3
    miss = _missing(case, w[:, :1])
    assert np.isnan(tg[miss]).all() and np.isfinite(tg[~miss & ~np.isnan(human[:, :1, :, 0])]).all()


# ---- 9: Python ----------------------------------------------------------------------------------------------------------------------------------
def test_retarget_per_frame_clip_and_mirror(hip, oracle):
    from general_motion_retargeting_amd import GeneralMotionRetargeting, synth
    case = bw.CASES["w_g1"]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    w = bw.make_weights(case)
    assert np.array_equal(q0[0], su.model.qpos0)
    names = GeneralMotionRetargeting(*bw.G1[:2], actual_human_height=bw.G1[2]).human_body_names
    frames = synth.streams_to_dicts(su.tt, human[0, :4])
    dicts = [{n: float(w[0, t, i]) for i, n in enumerate(names) if w[0, t, i] != 1.0} for t in range(4)]
    # a missing body may be absent from the frame altogether (the root never is)
    lacking = [{n: v for n, v in f.items() if d.get(n, 1.0) != 0.0 or n == su.tt.human_root_name} for f, d in zip(frames, dicts)]
    assert any(len(a) < len(b) for a, b in zip(lacking, frames))
    g = GeneralMotionRetargeting(*bw.G1[:2], actual_human_height=bw.G1[2])
    per_frame = np.stack([g.retarget(dict(f), body_weights=d) for f, d in zip(lacking, dicts)])
    counts = g.last_num_solves
    shd = g.scaled_human_data
    gone = [n for i, n in enumerate(names) if w[0, 3, i] == 0.0 and n != su.tt.human_root_name]
    assert gone and all(n not in shd for n in gone) and su.tt.human_root_name in shd
    e1 = g.error1()
    gc = GeneralMotionRetargeting(*bw.G1[:2], actual_human_height=bw.G1[2])
    clip = gc.retarget_clip([dict(f) for f in frames], body_weights=dicts)
    ga = GeneralMotionRetargeting(*bw.G1[:2], actual_human_height=bw.G1[2])
    arr = ga.retarget_clip(np.ascontiguousarray(human[0, :4]), body_weights=w[0, :4])
    ref = bw.mirror_runs(oracle, case)[0]
    for tag, q in (("retarget() x 4", per_frame), ("retarget_clip, dicts", clip), ("retarget_clip, array", arr)):
        err = float(np.abs(q - ref.q[:4]).max())
        print(f"{tag}: max |q - q_mirror| = {err:.3e}")
        assert err <= TOL, (tag, err)          # (a launch per frame starts the pivoting cold: rounding, not bits)
    assert _bits(clip, arr)
    assert np.array_equal(counts, ref.nsolve[3]) and np.array_equal(gc.last_num_solves, ref.nsolve[:4])
    assert abs(e1 - ref.err[3, 0]) <= 1e-8
    with pytest.raises(ValueError, match="chunk"):
        gc.retarget_clip(np.ascontiguousarray(human[0, :4]), chunk="auto", body_weights=w[0, :4])


def test_streaming_drop_equals_explicit_weights(hip):
    from general_motion_retargeting_amd import GeneralMotionRetargeting, synth
    from general_motion_retargeting_amd.utils.optitrack import StreamingRetargeter, rigid_body_id_map
    g1, g2, g3 = (GeneralMotionRetargeting("fbx", "unitree_g1", actual_human_height=1.6) for _ in range(3))
    human, _ = synth.make_streams(g1.model, g1._tables, 1, 6, seed=5)
    names = g1.human_body_names
    id_of = {n: i for i, n in rigid_body_id_map().items()}
    wrist = next(n for n in g1._tables.stages[0].human_names if "Hand" in n and n != g1.human_root_name)
    st, strict = StreamingRetargeter(g2, missing="drop"), StreamingRetargeter(g3)
    for t in range(human.shape[1]):
        fr = human[0, t]
        dropped = t in (2, 3)
        keep = np.array([not (dropped and n == wrist) for n in names])
        ids = np.array([id_of[n] for n in names])
        wts = keep.astype(np.float64)
        q_ref = g1.retarget_packed(fr, weights=wts) if dropped else g1.retarget_packed(fr)
        q = st.step(ids[keep], fr[keep, :3], fr[keep][:, [4, 5, 6, 3]])
        assert np.array_equal(q, q_ref), t
        if dropped:
            with pytest.raises(KeyError, match=wrist):
                strict.step(ids[keep], fr[keep, :3], fr[keep][:, [4, 5, 6, 3]])
            assert wrist not in g2.scaled_human_data


def test_dataset_clips_take_the_weights(hip):
    from general_motion_retargeting_amd import chunking, dataset
    case = bw.CASES["w_g1"]
    su = bw.setup_of(case.robot)
    human, _ = bw.make_input(case)
    w = bw.make_weights(case)
    clips, wts = [human[0, :5], human[1, :6], human[2, :4]], [w[0, :5], None, w[2, :4]]
    motions = dataset.retarget_clips(*bw.G1[:2], clips, [30.0] * 3, actual_human_height=bw.G1[2], body_weights=wts)
    sol = hip.Solver(su.mb, su.ts)
    for clip, wt, md in zip(clips, wts, motions):
        q, ns, st = sol.retarget_streams(su.model.qpos0[None], clip[None], weights=None if wt is None else wt[None])
        assert st[0] == 0
        want = q[0][:, 7:].astype(md["dof_pos"].dtype)
        assert pickle.dumps(np.ascontiguousarray(md["dof_pos"])) == pickle.dumps(np.ascontiguousarray(want))
    q_off = sol.retarget_streams(su.model.qpos0[None], clips[0][None])[0]
    assert np.abs(q_off[0][:, 7:] - motions[0]["dof_pos"]).max() > 1e-3
    sol.close()
    with pytest.raises(ValueError, match="chunk"):
        dataset.retarget_clips(*bw.G1[:2], clips, [30.0] * 3, actual_human_height=bw.G1[2], body_weights=wts, chunk=chunking.ChunkSpec(frames=100))
    mixed = dataset.retarget_mixed([{"src_human": bw.G1[0], "tgt_robot": bw.G1[1], "actual_human_height": bw.G1[2], "human": human, "weights": w}])
    sol = hip.Solver(su.mb, su.ts)
    one = sol.retarget_streams(np.broadcast_to(su.model.qpos0, (case.S, sol.nq)), human, weights=w)
    sol.close()
    assert _bits(mixed[0][0], one[0]) and _bits(mixed[0][1], one[1])


# ---- 10: the host entry points look at the values -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1.0, np.nan, np.inf])
def test_host_entry_points_reject_bad_weights(hip, bad):
    case = bw.CASES["w_t1"]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    human, q0 = np.ascontiguousarray(human), np.ascontiguousarray(q0)
    S, T = human.shape[:2]
    sol = hip.Solver(su.mb, su.ts)
    w = np.ones((S, T, sol.nhuman))
    w[1, 2, 3] = bad
    L = hip.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    q, ns, st = np.full((S, T, sol.nq), 7.0), np.zeros((S, T, 2), np.int32), np.full(S, 5, np.int32)
    rc = L.gmr_retarget_streams_weighted(sol.handle, S, T, p(q0), p(human), None, None, p(w), 0, p(q), p(ns), p(st), None, None)
    msg = L.gmr_last_error().decode()
    assert rc == GMR_ERR_ARG and "stream 1, frame 2, body 3" in msg, (rc, msg)
    job = (hip.Job * 1)(hip.Job(sol.handle.value, S, T, q0.ctypes.data, human.ctypes.data, None, q.ctypes.data, ns.ctypes.data, st.ctypes.data,
                                None, None, None))
    wl = (C.c_void_p * 1)(w.ctypes.data)
    rc = L.gmr_retarget_group_weighted(C.cast(job, C.c_void_p), 1, C.cast(wl, C.c_void_p), 0, 0)
    msg = L.gmr_last_error().decode()
    assert rc == GMR_ERR_ARG and "job 0: " in msg and "stream 1, frame 2, body 3" in msg, (rc, msg)
    assert (q == 7.0).all() and (st == 5).all(), "nothing reached the device"
    # the same entry in a frame beyond its stream's length is padding: the launch runs, and equals the launch with ones there
    lens = np.array([T, 2], np.int32)
    good = sol.retarget_streams(q0, human, lens=lens, weights=np.ones((S, T, sol.nhuman)))
    rc = L.gmr_retarget_streams_weighted(sol.handle, S, T, p(q0), p(human), p(lens), None, p(w), 0, p(q), p(ns), p(st), None, None)
    assert rc == 0 and (st == 0).all() and _bits(q[:, :2], good[0][:, :2]) and _bits(q[0], good[0][0])
    sol.close()
