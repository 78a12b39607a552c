"""CPU: the reference of the velocity-limit tests is fit for its job, and the Python side parses the limit as documented.

tests/vel_limit_mirror.py composes the reference's loop from the oracle's pieces and clamps build_qp's box.  Shown here:
with an infinite limit that loop IS oracle.retarget_streams; on every case of tests/test_ik_velocity_limits.py the oracle's
active-set solver and the kernels' pivoting (bpp_mirror.bpp_solve) agree, the pivoting stays far below its cap of 100
rounds, the limit bites in at least half of the solves, and no stop decision is closer than 1e-6 to its tolerance, so
that equal solve counts on the device are a fair demand.
"""
import numpy as np
import pytest

import vel_limit_mirror as vm

SOLVERS_AGREE = 1e-12
MAX_ROUNDS = 20
MIN_MARGIN = 1e-6


@pytest.mark.parametrize("name", ["g1_uniform", "t1_mixed", "dense_mixed", "g1_scaled"])
def test_mirror_without_limit_is_the_oracle(oracle, name):
    """vmax = inf on every hinge: min(max(lo, -inf), inf) is lo itself, and the composed loop with the oracle's solver
    returns oracle.retarget_streams bit for bit (qpos and solve counts), stream by stream with its own task set."""
    case = vm.CASES[name]
    su = vm.setup_of(case.robot)
    human, q0 = vm.make_input(case)
    runs = vm.mirror_runs(oracle, case, "oracle", vmax=np.full(len(su.model.joint_names), np.inf))
    for s, ts in enumerate(vm.stream_tasksets(case)):
        q_o, ns_o, st_o = oracle.retarget_streams(su.mb, ts, q0[s:s + 1], human[s:s + 1])
        assert st_o[0] == 0
        assert np.array_equal(runs[s].nsolve, ns_o[0]) and np.array_equal(runs[s].q, q_o[0]), (name, s)
        assert max(runs[s].on_bound) == 0


@pytest.mark.parametrize("name", list(vm.CASES))
def test_case_is_fit_for_the_device_comparison(oracle, name):
    case = vm.CASES[name]
    bpp, act = vm.mirror_runs(oracle, case, "bpp"), vm.mirror_runs(oracle, case, "oracle")
    (q_b, ns_b), (q_a, ns_a) = vm.stacked(bpp), vm.stacked(act)
    d = float(np.abs(q_b - q_a).max())
    rounds = max(max(r.rounds) for r in bpp)
    on = np.concatenate([r.on_bound for r in bpp])
    margin = min(min(r.margin for r in bpp), min(r.margin for r in act))
    print(f"{name}: |q_bpp - q_active_set| = {d:.2e}, {len(on)} solves, at most {rounds} rounds, a velocity bound active in "
          f"{(on > 0).mean():.2f} of them ({on.mean():.1f} variables on average), smallest stop margin {margin:.2e}")
    assert np.array_equal(ns_b, ns_a)
    assert d <= SOLVERS_AGREE, d
    assert rounds < MAX_ROUNDS, rounds
    assert (on > 0).mean() >= 0.5
    assert margin >= MIN_MARGIN, margin
    assert [r.on_bound for r in bpp] == [r.on_bound for r in act]


def test_mixed_tables_are_not_uniform():
    """Every mixed table holds 2.0, 40 and inf; the dense robot's hinges without a range are limited."""
    for name in ("g1_mixed", "t1_mixed", "dense_mixed"):
        case = vm.CASES[name]
        v = case.vmax()
        assert {2.0, 40.0, np.inf} <= set(v.tolist()), name
    su = vm.setup_of("dense")
    free = [h for h, l in enumerate(su.model.limited) if not l]
    assert len(free) == 3 and (vm.CASES["dense_mixed"].vmax()[free] == 2.0).all()


def test_outside_start_lies_outside_by_more_than_one_solve():
    case = vm.CASES["g1_outside"]
    su = vm.setup_of(case.robot)
    _, q0 = vm.make_input(case)
    vdt = vm.THREE_PI * su.model.timestep
    (h_up, d_up), (h_dn, d_dn) = vm.outside_hinges(su.model)
    assert np.allclose(q0[:, 7 + h_up] - su.model.range_hi[h_up], 0.1) and np.allclose(q0[:, 7 + h_dn] - su.model.range_lo[h_dn], -0.07)
    assert min(d_up, -d_dn) > 2 * vdt        # the joint-range box alone is empty against the velocity box: the clamp form matters


# ---- Python-side parsing -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return vm.setup_of(vm.G1).model


def test_table_from_scalar_array_dict(model):
    from general_motion_retargeting_amd.ik_config import velocity_limit_table
    nh = len(model.joint_names)
    assert velocity_limit_table(model) is None and velocity_limit_table(model, False, None) is None
    assert np.array_equal(velocity_limit_table(model, True), np.full(nh, 3.0 * np.pi))
    assert np.array_equal(velocity_limit_table(model, False, 40.0), np.full(nh, 40.0))
    assert np.array_equal(velocity_limit_table(model, True, 40.0), np.full(nh, 40.0))       # a given table wins over the default
    arr = np.linspace(1.0, 5.0, nh)
    arr[3] = np.inf
    out = velocity_limit_table(model, False, arr)
    assert np.array_equal(out, arr) and out is not arr
    d = velocity_limit_table(model, False, {model.joint_names[3]: 2.0, model.joint_names[-1]: 7.5})
    want = np.full(nh, np.inf)
    want[3], want[-1] = 2.0, 7.5
    assert np.array_equal(d, want)


def test_table_rejects_bad_input(model):
    from general_motion_retargeting_amd.ik_config import velocity_limit_table
    nh = len(model.joint_names)
    with pytest.raises(KeyError):
        velocity_limit_table(model, False, {"no_such_joint": 2.0})
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            velocity_limit_table(model, False, bad)
        arr = np.full(nh, 3.0)
        arr[5] = bad
        with pytest.raises(ValueError):
            velocity_limit_table(model, False, arr)
        with pytest.raises(ValueError):
            velocity_limit_table(model, False, {model.joint_names[0]: bad})
    with pytest.raises(ValueError):
        velocity_limit_table(model, False, np.ones(nh + 1))


def test_retargeter_arguments():
    """use_velocity_limit=True alone is upstream's 3 pi on every motor joint; the table is held until a solver exists."""
    from general_motion_retargeting_amd import GeneralMotionRetargeting
    g = GeneralMotionRetargeting(*vm.G1[:2], actual_human_height=vm.G1[2])
    assert g.velocity_limit is None and g.use_velocity_limit is False
    g = GeneralMotionRetargeting(*vm.G1[:2], actual_human_height=vm.G1[2], use_velocity_limit=True)
    assert g.use_velocity_limit and np.array_equal(g.velocity_limit, np.full(len(g.model.joint_names), 3.0 * np.pi))
    g.set_velocity_limit({"left_knee_joint": 2.0})
    assert g.velocity_limit[g.model.joint_names.index("left_knee_joint")] == 2.0 and np.isinf(g.velocity_limit).sum() == len(g.model.joint_names) - 1
    g.set_velocity_limit()
    assert g.velocity_limit is None and not g.use_velocity_limit
    with pytest.raises(ValueError):
        GeneralMotionRetargeting(*vm.G1[:2], velocity_limit=-3.0)


def test_cli_takes_the_limit():
    """--velocity_limit is absent by default and reaches the drivers as a number."""
    import inspect
    from general_motion_retargeting_amd import dataset
    for f in (dataset.retarget_clips, dataset.retarget_smplx_files, dataset.retarget_bvh_files, dataset.retarget_smplx_loaded,
              dataset.run_bvh_dataset, dataset.run_smplx_dataset, dataset.ClipRetargeter.__init__):
        assert inspect.signature(f).parameters["velocity_limit"].default is None, f
    src = inspect.getsource(dataset.main)
    assert '"--velocity_limit", type=float, default=None' in src and src.count("velocity_limit=a.velocity_limit") == 2
