"""-m gpu: per-joint velocity limits in the QP box (gmr_solver_set_velocity_limits), on every launch path.

The reference is tests/vel_limit_mirror.py -- the reference's loop from the oracle's pieces, the clamp on build_qp's box, the
kernels' pivoting behind it; tests/test_ik_velocity_limits_host.py shows on the CPU that every case here is fit for the
comparison (the two CPU solvers agree to 1e-12, the limit bites in every solve, no stop decision is within 1e-6 of its
tolerance).  The bound on max |q - q_mirror| is the project's established one for bound-heavy input, 1e-8
(ik_variants.BASE_TOL["scatter"]); the solve counts must be the mirror's.

The limit bounds ONE solve (|dq_h| <= vmax_h * timestep), as mink's VelocityLimit does: the invariant checked without a
mirror is therefore |dtheta| <= (solves of the frame) * vmax_h * timestep, not a velocity between frames.
"""
import pickle

import numpy as np
import pytest

import ik_variants as iv
import vel_limit_mirror as vm

pytestmark = pytest.mark.gpu

TOL = iv.BASE_TOL["scatter"]
QUEUED_S = 2600                  # more streams than the throughput kernel's resident wavefronts: the queued dispatch takes over


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _solver(hip, monkeypatch, su, shape, vmax):
    """A solver that serves `shape` (as tests/test_ik_variants.py forces them) with the table `vmax` (None: never set)."""
    if shape == "onewave":
        monkeypatch.setenv("GMR_IK_NO_WIDE", "1")
    try:
        sol = hip.Solver(su.mb, su.ts)
    finally:
        monkeypatch.delenv("GMR_IK_NO_WIDE", raising=False)
    sol.set_waves(4 if shape == "latency" else 1)
    if vmax is not None:
        sol.set_velocity_limit(vmax)
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


# ---- 1: every instance a launch can end in ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["latency", "onewave", "throughput"])
def test_uniform_limit_matches_mirror(hip, oracle, monkeypatch, shape):
    """G1, 3 pi on every hinge: <36, 4, TREE_SMALL>, <36, 1, TREE_SMALL> and the throughput kernel, one workgroup per stream."""
    case = vm.CASES["g1_uniform"]
    su = vm.setup_of(case.robot)
    human, q0 = vm.make_input(case)
    sol = _solver(hip, monkeypatch, su, shape, case.vmax())
    assert np.array_equal(sol.velocity_limit, case.vmax())
    out = sol.retarget_streams(q0, human)
    sol.close()
    _check(f"g1_uniform {shape}", out, vm.stacked(vm.mirror_runs(oracle, case)))


def test_uniform_limit_queued_dispatch(hip, oracle):
    """The throughput kernel serving (stream, 2 frames) items from its queue: the bits of one workgroup per stream, and the
    mirror's result on the last copy of the four generated streams."""
    case = vm.CASES["g1_uniform"]
    su = vm.setup_of(case.robot)
    bh, bq = vm.make_input(case)
    pick = np.arange(QUEUED_S) % case.S
    human, q0 = bh[pick].copy(), bq[pick].copy()
    sol = hip.Solver(su.mb, su.ts)
    sol.set_waves(1)
    sol.set_velocity_limit(case.vmax())
    sol.set_dispatch(0)
    q_d, ns_d, st_d = sol.retarget_streams(q0, human)
    sol.set_dispatch(2)
    q_q, ns_q, st_q = sol.retarget_streams(q0, human)
    sol.close()
    assert (st_d == 0).all() and _bits(st_d, st_q) and _bits(ns_d, ns_q) and _bits(q_d, q_q)
    n = case.S
    assert (pick[-n:] == np.arange(n)).all()
    _check("g1_uniform queued", (q_q[-n:], ns_q[-n:], st_q[-n:]), vm.stacked(vm.mirror_runs(oracle, case)))


# ---- 2: a table that differs from hinge to hinge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shapes", [("g1_mixed", ("latency", "onewave", "throughput")),
                                         ("t1_mixed", ("latency", "onewave", "throughput")),
                                         ("dense_mixed", ("latency", "throughput"))])
def test_mixed_table_matches_mirror(hip, oracle, monkeypatch, name, shapes):
    """2.0 / 40 / none in turn: a table read at the wrong lane fails here.  G1; bvh -> booster_t1 (27 dofs, one-sided ranges,
    qpos0 on a bound); the dense robot, three of whose hinges have no range -- set_waves(4) is its <36, 4, TREE> instance,
    set_waves(1) its <36, 1, DENSE> one (it does not fit the throughput kernel)."""
    case = vm.CASES[name]
    su = vm.setup_of(case.robot)
    human, q0 = vm.make_input(case)
    ref = vm.stacked(vm.mirror_runs(oracle, case))
    for shape in shapes:
        sol = _solver(hip, monkeypatch, su, shape, case.vmax())
        out = sol.retarget_streams(q0, human)
        sol.close()
        _check(f"{name} {shape}", out, ref)


# ---- 3: off is off ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["latency", "onewave", "throughput"])
def test_no_limit_is_byte_equal(hip, monkeypatch, shape):
    """Never set, set to inf everywhere, set to 3 pi and cleared with NULL: the same bytes in qpos, nsolve, tgt_out, err_out."""
    case = vm.CASES["g1_uniform"]
    su = vm.setup_of(case.robot)
    human, q0 = vm.make_input(case)
    nh = len(su.model.joint_names)
    outs = {}
    for how in ("never", "inf", "cleared"):
        sol = _solver(hip, monkeypatch, su, shape, {"never": None, "inf": np.full(nh, np.inf), "cleared": case.vmax()}[how])
        if how == "cleared":
            limited = sol.retarget_streams(q0, human)
            sol.set_velocity_limit(None)
        assert np.isinf(sol.velocity_limit).all()
        outs[how] = sol.retarget_streams(q0, human, want_targets=True, want_errors=True)
        sol.close()
    for how in ("inf", "cleared"):
        for a, b in zip(outs["never"], outs[how]):
            assert _bits(a, b), (shape, how)
    assert (outs["never"][2] == 0).all()
    assert np.abs(limited[0] - outs["never"][0]).max() > 1e-3        # (and the limit was on in between)


# ---- 4: the invariant, without a mirror ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["latency", "throughput"])
def test_per_solve_bound_holds_per_frame(hip, monkeypatch, shape):
    """|dtheta_h| of a frame <= (its solves) * vmax_h * timestep * (1 + 1e-12); without the limit the same input breaks it."""
    case = vm.CASES["g1_mixed"]
    su = vm.setup_of(case.robot)
    human, q0 = vm.make_input(case)
    vdt = vm.vdt_of(su.mb, case.vmax())[6:]

    def excess(q, ns):
        th = np.concatenate([q0[:, None, 7:], q[..., 7:]], axis=1)
        step = np.abs(np.diff(th, axis=1))
        with np.errstate(invalid="ignore"):
            allowed = ns.sum(axis=2)[..., None] * vdt * (1.0 + 1e-12)
        return step - allowed

    sol = _solver(hip, monkeypatch, su, shape, case.vmax())
    q, ns, st = sol.retarget_streams(q0, human)
    sol.set_velocity_limit(None)
    q_off, ns_off, st_off = sol.retarget_streams(q0, human)
    sol.close()
    assert (st == 0).all() and (st_off == 0).all()
    worst, worst_off = float(excess(q, ns).max()), float(excess(q_off, ns_off).max())
    print(f"{shape}: largest |dtheta| - allowed: {worst:.3e} with the limit, {worst_off:.3e} without")
    assert worst <= 0.0, worst
    assert worst_off > 0.0, "the input does not exceed the bound without the limit: the case tests nothing"


# ---- 5: a start outside the joint ranges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["latency", "onewave", "throughput"])
def test_start_outside_range_walks_back(hip, oracle, monkeypatch, shape):
    """Left knee 0.1 rad above, right ankle pitch 0.07 below its range, 3 pi: the box of those joints collapses to -vdt / +vdt
    until they are back; status 0, the mirror's result, both inside their ranges at the end."""
    case = vm.CASES["g1_outside"]
    su = vm.setup_of(case.robot)
    human, q0 = vm.make_input(case)
    sol = _solver(hip, monkeypatch, su, shape, case.vmax())
    out = sol.retarget_streams(q0, human)
    sol.close()
    _check(f"g1_outside {shape}", out, vm.stacked(vm.mirror_runs(oracle, case)))
    for h, _ in vm.outside_hinges(su.model):
        end = out[0][:, -1, 7 + h]
        assert (end >= su.model.range_lo[h] - 1e-9).all() and (end <= su.model.range_hi[h] + 1e-9).all(), (h, end)


# ---- 6: a group of two jobs, one limited -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [0, 1])
def test_group_jobs_keep_their_own_tables(hip, waves):
    """G1 at 3 pi and T1 without a limit in one gmr_retarget_group: every job's rows are the bytes of its solver's own launch.
    waves = 1: both jobs in ONE launch of the throughput kernel's group instance, whose job table names each solver's image."""
    jobs, own = [], []
    for name, limited in (("g1_uniform", True), ("t1_mixed", False)):
        case = vm.CASES[name]
        su = vm.setup_of(case.robot)
        human, q0 = vm.make_input(case)
        sol = hip.Solver(su.mb, su.ts)
        sol.set_waves(waves)
        if limited:
            sol.set_velocity_limit(case.vmax())
        own.append(sol.retarget_streams(q0, human))
        jobs.append({"solver": sol, "human": human, "q0": q0})
    outs = hip.retarget_group(jobs)
    for (q, ns, st), (q1, ns1, st1) in zip(outs, own):
        assert (st == 0).all() and _bits(q, q1) and _bits(ns, ns1) and _bits(st, st1)
    # the unlimited job is the unlimited result: T1's table was never set, and G1's did not leak into it
    su = vm.setup_of(vm.T1)
    plain = hip.Solver(su.mb, su.ts)
    plain.set_waves(waves)
    human, q0 = vm.make_input(vm.CASES["t1_mixed"])
    assert _bits(plain.retarget_streams(q0, human)[0], outs[1][0])
    plain.close()
    for j in jobs:
        j["solver"].close()


# ---- 7: the scaled path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [4, 1])
def test_scaled_streams_with_limit(hip, oracle, waves):
    """retarget_streams(heights=): one height per stream as scale rows, 3 pi; the mirror runs stream s under the task set of
    an object built for heights[s]."""
    from general_motion_retargeting_amd import GeneralMotionRetargeting
    case = vm.CASES["g1_scaled"]
    human, q0 = vm.make_input(case)
    g = GeneralMotionRetargeting(*vm.G1[:2], use_velocity_limit=True)
    g.hip_solver.set_waves(waves)
    out = g.retarget_streams(human, q0=q0, heights=np.array(case.heights))
    _check(f"g1_scaled waves={waves}", out, vm.stacked(vm.mirror_runs(oracle, case)))
    g.hip_solver.close()


# ---- 8: the per-frame API ----------------------------------------------------------------------------------------------------------------
def test_retarget_per_frame_equals_clip_and_mirror(hip, oracle):
    from general_motion_retargeting_amd import GeneralMotionRetargeting, synth
    case = vm.CASES["g1_uniform"]
    su = vm.setup_of(case.robot)
    human, q0 = vm.make_input(case)
    assert np.array_equal(q0[0], su.model.qpos0)
    frames = synth.streams_to_dicts(su.tt, human[0, :3])
    g = GeneralMotionRetargeting(*vm.G1[:2], actual_human_height=vm.G1[2], use_velocity_limit=True)
    per_frame = np.stack([g.retarget(f) for f in frames])
    counts = g.last_num_solves
    clip = GeneralMotionRetargeting(*vm.G1[:2], actual_human_height=vm.G1[2], use_velocity_limit=True).retarget_clip(frames)
    assert _bits(per_frame, clip)
    ref = vm.mirror_runs(oracle, case)[0]
    err = float(np.abs(per_frame - ref.q[:3]).max())
    print(f"retarget() x 3: max |q - q_mirror| = {err:.3e}")
    assert err <= TOL and np.array_equal(counts, ref.nsolve[2])


# ---- 9: the dataset path -----------------------------------------------------------------------------------------------------------------
def test_dataset_clips_take_the_limit(hip):
    from general_motion_retargeting_amd import dataset
    case = vm.CASES["g1_uniform"]
    su = vm.setup_of(case.robot)
    human, _ = vm.make_input(case)
    clips = [human[0, :5], human[1, :6]]
    motions = dataset.retarget_clips(*vm.G1[:2], clips, [30.0, 30.0], actual_human_height=vm.G1[2], velocity_limit=vm.THREE_PI)
    sol = hip.Solver(su.mb, su.ts)
    sol.set_velocity_limit(case.vmax())
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


# ---- host-side argument checks (the only failures provoked on purpose) --------------------------------------------------------------------
def test_setter_rejects_bad_tables(hip):
    su = vm.setup_of(vm.G1)
    nh = len(su.model.joint_names)
    sol = hip.Solver(su.mb, su.ts)
    good = np.full(nh, 5.0)
    sol.set_velocity_limit(good)
    for bad in (np.full(nh + 1, 5.0), np.full(nh - 1, 5.0)):
        with pytest.raises(hip.GmrHipError, match="hinges"):
            sol.set_velocity_limit(bad)
    for v in (0.0, -2.0, np.nan):
        bad = good.copy()
        bad[7] = v
        with pytest.raises(hip.GmrHipError, match="hinge 7"):
            sol.set_velocity_limit(bad)
    assert np.array_equal(sol.velocity_limit, good)              # a rejected table changes nothing
    assert sol.lds_bytes == hip.Solver(su.mb, su.ts).lds_bytes
    sol.close()
