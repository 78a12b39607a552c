"""CPU: the reference of the frame-velocity-limit tests is fit for its job, and the Python side parses the limit as documented.

tests/frame_limit_mirror.py is vel_limit_mirror's loop with the frame window clamped last onto build_qp's box.  Shown here:
with an infinite window that loop IS oracle.retarget_streams; on every case of tests/test_ik_frame_limits.py the oracle's
active-set solver and the kernels' pivoting (bpp_mirror.bpp_solve) agree to 1e-12 with equal solve counts, the pivoting needs
at most 20 rounds in any solve, every bounded frame has a solve with a variable on a frame bound, no stop decision is closer
than 1e-6 to its tolerance (device and mirror differ by about 1e-14, so equal solve counts on the device are a fair demand),
and the invariant |theta_t - theta_(t-1)| <= w (1 + 1e-12) holds on the mirror's own result for every bounded frame.

Figures of the cases (bpp solver; seeds fixed after this check, none had to be dropped -- G1 seed 9, the seed of the
per-solve tests, was never a candidate: its margin at w = 0.02 is 3.4e-7):

    case            rounds  margin   on a frame bound (mean)  unbounded step - w
    f_g1               7    9.5e-5        25.2                    0.43
    f_t1               4    8.3e-4        17.9                    0.39
    f_g1_mixed         5    3.6e-5         9.1                    0.34
    f_t1_mixed         4    4.5e-5         6.1                    0.30
    f_dense_mixed      4    2.2e-5        10.5                    0.83
    f_g1_first         4    5.4e-6        24.9                    2.09
    f_g1_outside       3    2.0e-5        22.0                    2.06
    f_g1_scaled        6    5.2e-5        25.2                    0.43
    f_g1_both          6    4.3e-5        20.7                    0.40
"""
import inspect

import numpy as np
import pytest

import frame_limit_mirror as fm
import vel_limit_mirror as vm

SOLVERS_AGREE = 1e-12
MAX_ROUNDS = 20
MIN_MARGIN = 1e-6


@pytest.mark.parametrize("name", ["f_g1", "f_t1_mixed", "f_dense_mixed", "f_g1_scaled", "f_g1_first"])
def test_mirror_without_limit_is_the_oracle(oracle, name):
    """w = inf on every hinge: min(max(lo, -inf), inf) is lo itself, and the composed loop with the oracle's solver returns
    oracle.retarget_streams bit for bit (qpos and solve counts), stream by stream with its own task set, frame 0 bounded or not."""
    case = fm.CASES[name]
    su = fm.setup_of(case.robot)
    human, q0 = fm.make_input(case)
    runs = fm.mirror_runs(oracle, case, "oracle", vmax=np.full(len(su.model.joint_names), np.inf))
    for s, ts in enumerate(fm.stream_tasksets(case)):
        q_o, ns_o, st_o = oracle.retarget_streams(su.mb, ts, q0[s:s + 1], human[s:s + 1])
        assert st_o[0] == 0
        assert np.array_equal(runs[s].nsolve, ns_o[0]) and np.array_equal(runs[s].q, q_o[0]), (name, s)
        assert max(n for _, n in runs[s].on_frame) == 0


def test_infinite_window_returns_the_box_bit_for_bit():
    rng = np.random.default_rng(3)
    lo, hi = -rng.random(40), rng.random(40)
    lo[::5], hi[::7] = -np.inf, np.inf
    lo[3], hi[4] = -0.0, 0.0
    th0, th = rng.normal(size=40), rng.normal(size=40)
    a, b, lf, hf = fm.clamp_window(lo, hi, th0, th, np.full(40, np.inf))
    assert a.tobytes() == lo.tobytes() and b.tobytes() == hi.tobytes()
    assert np.isneginf(lf).all() and np.isposinf(hf).all()


@pytest.mark.parametrize("name", list(fm.CASES))
def test_case_is_fit_for_the_device_comparison(oracle, name):
    case = fm.CASES[name]
    su = fm.setup_of(case.robot)
    _, q0 = fm.make_input(case)
    bpp, act = fm.mirror_runs(oracle, case, "bpp"), fm.mirror_runs(oracle, case, "oracle")
    (q_b, ns_b), (q_a, ns_a) = fm.stacked(bpp), fm.stacked(act)
    d = float(np.abs(q_b - q_a).max())
    rounds = max(max(r.rounds) for r in bpp)
    margin = min(min(r.margin for r in bpp), min(r.margin for r in act))
    bounded = [t for t in range(case.T) if t > 0 or case.first_bounded]
    on = [n for r in bpp for t, n in r.on_frame if t in bounded]
    w = fm.window_of(su.mb, case.vmax())
    worst = max(float(fm.excess(q, q0, w, case.first_bounded).max()) for q in (q_b, q_a))
    free = fm.stacked(fm.mirror_runs(oracle, case, "bpp", vmax=np.full(len(su.model.joint_names), np.inf)))[0]
    print(f"{name}: |q_bpp - q_active_set| = {d:.2e}, at most {rounds} rounds, smallest stop margin {margin:.2e}, {np.mean(on):.1f} variables "
          f"on a frame bound per solve, largest step - w (1 + 1e-12) = {worst:.2e} (without the limit {fm.excess(free, q0, w, case.first_bounded).max():.2f})")
    assert np.array_equal(ns_b, ns_a)
    assert d <= SOLVERS_AGREE, d
    assert rounds <= MAX_ROUNDS, rounds
    assert margin >= MIN_MARGIN, margin
    for r in bpp + act:
        assert (r.nsolve > 0).all()
        for t in bounded:
            assert any(n > 0 for tt, n in r.on_frame if tt == t), (name, t)
    assert worst <= 0.0, worst
    assert fm.excess(free, q0, w, case.first_bounded).max() > 0.1          # the limit is what holds the invariant


def test_free_first_frame_is_the_unlimited_one(oracle):
    case = fm.CASES["f_g1"]
    su = fm.setup_of(case.robot)
    lim = fm.stacked(fm.mirror_runs(oracle, case))[0]
    off = fm.stacked(fm.mirror_runs(oracle, case, vmax=np.full(len(su.model.joint_names), np.inf)))[0]
    assert lim[:, 0].tobytes() == off[:, 0].tobytes() and np.abs(lim[:, 1] - off[:, 1]).max() > 1e-3


def test_mixed_tables_are_not_uniform():
    """Every mixed table holds 0.6, 12 and inf; the dense robot's hinges without a range are limited."""
    for name in ("f_g1_mixed", "f_t1_mixed", "f_dense_mixed"):
        assert {fm.VMAX, fm.VMAX_LARGE, np.inf} <= set(fm.CASES[name].vmax().tolist()), name
    su = fm.setup_of("dense")
    free = [h for h, l in enumerate(su.model.limited) if not l]
    assert len(free) == 3 and (fm.CASES["f_dense_mixed"].vmax()[free] == fm.VMAX).all()


def test_outside_start_walks_back_by_w_per_frame(oracle):
    """The window is applied last, so it holds against a joint range that asks for more: both hinges of the outside start
    come back by exactly w per frame while the range's own bound lies beyond the window."""
    case = fm.CASES["f_g1_outside"]
    su = fm.setup_of(case.robot)
    _, q0 = fm.make_input(case)
    w = fm.VMAX * fm.FRAME_DT
    gain = float(su.ts["limit_gain"][0])
    q = fm.stacked(fm.mirror_runs(oracle, case))[0]
    for h, d in vm.outside_hinges(su.model):
        assert gain <= 1.0 and gain * (abs(d) - (fm.WALK_FRAMES - 1) * w) >= w, (gain, d)
        assert fm.walk_back_error(q, q0, h, d) <= 1e-12, (h, d)


# ---- Python-side parsing and argument errors that need no device ----------------------------------------------------------------------
def test_constructor_and_setter_hold_the_table_until_a_solver_exists():
    from general_motion_retargeting_amd import GeneralMotionRetargeting
    g = GeneralMotionRetargeting(*fm.G1[:2], actual_human_height=fm.G1[2])
    nh = len(g.model.joint_names)
    assert g.frame_velocity_limit is None and not g._frame_limit_on()
    g = GeneralMotionRetargeting(*fm.G1[:2], actual_human_height=fm.G1[2], frame_velocity_limit=fm.VMAX, fps=30)
    assert np.array_equal(g.frame_velocity_limit, np.full(nh, fm.VMAX)) and g._frame_fps == 30.0 and g._frame_limit_on()
    g.set_frame_velocity_limit({"left_knee_joint": 2.0}, fps=60)
    k = g.model.joint_names.index("left_knee_joint")
    assert g.frame_velocity_limit[k] == 2.0 and np.isinf(g.frame_velocity_limit).sum() == nh - 1 and g._frame_fps == 60.0
    g.set_frame_velocity_limit(np.full(nh, np.inf), fps=60)
    assert not g._frame_limit_on()                   # a table without a finite entry limits nothing (and refuses no chunk)
    g.set_frame_velocity_limit(None)
    assert g.frame_velocity_limit is None and g._frame_fps is None
    assert g._solver is None                         # nothing above needed a device


def test_bad_arguments_raise_before_anything_reaches_a_device():
    from general_motion_retargeting_amd import GeneralMotionRetargeting, chunking, dataset
    with pytest.raises(ValueError, match="fps"):
        GeneralMotionRetargeting(*fm.G1[:2], frame_velocity_limit=fm.VMAX)
    g = GeneralMotionRetargeting(*fm.G1[:2], actual_human_height=fm.G1[2])
    nh = len(g.model.joint_names)
    for fps in (None, 0, -30.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="fps"):
            g.set_frame_velocity_limit(fm.VMAX, fps)
    for bad in (0.0, -1.0, np.nan, np.ones(nh + 1), {g.model.joint_names[0]: -2.0}):
        with pytest.raises(ValueError):
            g.set_frame_velocity_limit(bad, 30)
    with pytest.raises(KeyError):
        g.set_frame_velocity_limit({"no_such_joint": 2.0}, 30)
    assert g.frame_velocity_limit is None and g._solver is None
    # chunk= under a finite limit, refused where the two arguments meet; mixed fps, where the batch is known
    g.set_frame_velocity_limit(fm.VMAX, 30)
    with pytest.raises(ValueError, match="chunk"):
        g.retarget_clip(np.zeros((4, len(g.human_body_names), 7)), chunk="auto")
    with pytest.raises(ValueError, match="chunk"):
        dataset.ClipRetargeter(*fm.G1[:2], chunk=chunking.ChunkSpec(frames=100), frame_velocity_limit=fm.VMAX)
    with pytest.raises(ValueError, match="share one fps"):
        dataset._set_batch_frame_limit([g], fm.VMAX, [30.0, 30.0, 60.0])
    assert g._solver is None


def test_every_driver_takes_the_argument_and_the_cli_passes_it():
    from general_motion_retargeting_amd import GeneralMotionRetargeting, dataset
    for f in (dataset.ClipRetargeter.__init__, dataset.retarget_clips, dataset.retarget_bvh_files, dataset.retarget_smplx_files,
              dataset.retarget_smplx_loaded, dataset.run_bvh_dataset, dataset.run_smplx_dataset, GeneralMotionRetargeting.__init__):
        assert inspect.signature(f).parameters["frame_velocity_limit"].default is None, f
    assert inspect.signature(GeneralMotionRetargeting.__init__).parameters["fps"].default is None
    assert inspect.signature(GeneralMotionRetargeting.retarget_streams).parameters["q0_is_previous_frame"].default is False
    src = inspect.getsource(dataset.main)
    assert '"--frame_velocity_limit", type=float, default=None' in src and src.count("frame_velocity_limit=a.frame_velocity_limit") == 2
    assert 'frame_velocity_limit=g.get("frame_velocity_limit"), fps=g.get("fps")' in inspect.getsource(dataset.retarget_mixed)


def test_flag_value_and_signatures():
    from general_motion_retargeting_amd import _lib
    assert _lib.FLAG_FRAME_LIMIT_FIRST == 4
    assert {"gmr_solver_set_frame_velocity_limits", "gmr_solver_frame_velocity_limits"} <= set(_lib._SIGS)
    header = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "gmr_hip.h")).read()
    assert "#define GMR_FLAG_FRAME_LIMIT_FIRST 4" in header
    assert "int gmr_solver_set_frame_velocity_limits(gmr_solver_t* solver, const double* vmax, int n, double frame_dt);" in header
    assert "int gmr_solver_frame_velocity_limits(const gmr_solver_t* solver, double* vmax_out, int n, double* frame_dt_out);" in header
