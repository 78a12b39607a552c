"""-m gpu: the latency shape applies -Jl^-1(e_k) to every (task, dof) column in operator form (se3_jlinv_coef5 on one lane
per task, se3_jlinv_apply5 in the pair lanes); the one-wavefront shape still forms the matrix.  Both launch shapes against
the oracle on inputs where the operator path can go wrong: the bound-path input, a zero residual (the identity zone of
Jl^-1) followed by 1e-3 perturbations (its series zone), other task lists (bvh, fbx; the second table repeats the first
one's tasks, so its first solve reuses the first stage's residuals), the <8, 10> instance, and the per-frame errors.

On every input: status 0, solve counts equal to the oracle's and to each other, |q - q_oracle| <= 1e-8, |q_4 - q_1| <= 1e-12.
The oracle solves every input with status 0 (asserted where the input is built, on the CPU).
"""
import numpy as np
import pytest

from conftest import get_setup
from test_ik_bound_path import _Synthetic, _scatter

Q_ORACLE_TOL = 1e-8
Q_SHAPES_TOL = 1e-12


def _repeats_first_table(ts):
    n = int(ts["ntask"][0][0])
    return (n == int(ts["ntask"][0][1]) and np.array_equal(ts["task_body"][0][0][:n], ts["task_body"][0][1][:n])
            and np.array_equal(ts["task_human"][0][0][:n], ts["task_human"][0][1][:n]))


def _zero_then_perturbed(su, S, T):
    """Frame 0: the targets are the FK poses of q0 (no noise, q0 = the pose the frame was generated from).  Frames 1..:
    the same human frame moved by N(0, 1e-3 m) and turned by N(0, 1e-3 rad) per body."""
    from general_motion_retargeting_amd import synth
    clean, _, truth = synth.make_streams(su.model, su.tt, S, 1, seed=33, pos_noise=0.0, rot_noise_deg=0.0, return_truth=True)
    q0 = truth[:, 0].copy()
    human = np.repeat(clean, T, axis=1)
    rng = np.random.default_rng(4)
    human[:, 1:, :, :3] += rng.normal(0.0, 1e-3, size=human[:, 1:, :, :3].shape)
    rv = rng.normal(0.0, 1e-3, size=human[:, 1:, :, :3].shape)
    human[:, 1:, :, 3:] = synth.quat_mul(human[:, 1:, :, 3:], synth.rotvec_quat(rv))
    return q0, human


@pytest.fixture(scope="module")
def inputs(oracle, g1, tmp_path_factory):
    """name -> (setup, q0, human, oracle q, oracle solve counts).  Shared, never modified."""
    from general_motion_retargeting_amd import synth
    out = {}

    def add(name, su, q0, human):
        q_o, ns_o, st_o = oracle.retarget_streams(su.mb, su.ts, q0, human)
        assert (st_o == 0).all(), name
        for a in (q0, human, q_o, ns_o):
            a.setflags(write=False)
        out[name] = (su, q0, human, q_o, ns_o)

    human, q0 = synth.make_streams(g1.model, g1.tt, 6, 10, seed=21)
    add("bound_path", g1, q0, _scatter(human))
    q0, human = _zero_then_perturbed(g1, 3, 6)
    add("zero_residual", g1, q0, human)
    for src, robot in (("bvh", "booster_t1"), ("fbx", "unitree_g1")):
        su = get_setup(src, robot, 1.7)
        human, q0 = synth.make_streams(su.model, su.tt, 3, 8, seed=5)
        add(src, su, q0, _scatter(human))
    su = _Synthetic(tmp_path_factory.mktemp("robot"))
    human, q0 = synth.make_streams(su.model, su.tt, 3, 8, seed=5)
    add("wide_trunk", su, q0, _scatter(human))
    return out


def test_inputs_reach_the_zones_and_the_reuse_path(oracle, inputs):
    """CPU: what each input is there for."""
    for name in ("bound_path", "bvh", "fbx", "wide_trunk"):
        assert _repeats_first_table(inputs[name][0].ts), name     # stage 1's first solve starts from stage 0's residuals
    lists = {tuple(zip(inputs[n][0].tt.stages[0].frame_names, inputs[n][0].tt.stages[0].human_names))
             for n in ("bound_path", "bvh", "fbx", "wide_trunk")}
    assert len(lists) == 4                                         # four different task lists
    su, q0, human, q_o, ns_o = inputs["zero_residual"]
    # frame 0: every task's residual at q0 is in the identity zone of Jl^-1 (|w|^2 < 1e-10) and the frame leaves q alone
    tgt = oracle.preprocess(su.ts, human[:, 0])
    for s in range(len(q0)):
        for stage in (0, 1):
            _, E = oracle.stage_error(su.mb, su.ts, stage, q0[s], tgt[s])
            assert E < 1e-9, (s, stage, E)
    assert np.abs(q_o[:, 0] - q0).max() <= 1e-12
    # frames 1..: the first residual of a frame is ~ 1e-3 rad per task: the series zone (1e-10 <= |w|^2 < 1e-2)
    tgt = oracle.preprocess(su.ts, human[:, 1])
    _, E = oracle.stage_error(su.mb, su.ts, 0, q_o[0, 0], tgt[0])
    assert 1e-4 < E < 1e-1, E


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bound_path", "zero_residual", "bvh", "fbx", "wide_trunk"])
def test_both_shapes_match_the_oracle(hip, inputs, name):
    su, q0, human, q_o, ns_o = inputs[name]
    sol = hip.Solver(su.mb, su.ts)
    out = {}
    for waves in (4, 1):
        sol.set_waves(waves)
        q_h, ns_h, st_h = sol.retarget_streams(q0, human)
        assert (st_h == 0).all(), waves
        assert np.array_equal(ns_h, ns_o), f"{name}, {waves} wavefront(s): solve counts differ from the oracle's"
        err = np.abs(q_h - q_o).max()
        print(f"{name}, {waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
        assert err <= Q_ORACLE_TOL, (waves, err)
        out[waves] = (q_h, ns_h)
    sol.close()
    assert np.array_equal(out[4][1], out[1][1])
    d = np.abs(out[4][0] - out[1][0]).max()
    print(f"{name}: max |q_4 - q_1| = {d:.3e}")
    assert d <= Q_SHAPES_TOL, d
    if name == "zero_residual":     # the identity zone: the frame's solves leave q where it is
        for waves in (4, 1):
            assert np.abs(out[waves][0][:, 0] - q0).max() <= 1e-12, waves


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bound_path", "zero_residual"])
def test_per_frame_errors_match_the_oracle(hip, oracle, inputs, name):
    """error1 / error2 (the residual norms at the configuration every frame ends with) through the per-frame output of both
    shapes against the oracle's stage error at that configuration, to 1e-12: the residual path is untouched."""
    su, q0, human, q_o, ns_o = inputs[name]
    tgt = oracle.preprocess(su.ts, human)
    sol = hip.Solver(su.mb, su.ts)
    for waves in (4, 1):
        sol.set_waves(waves)
        q_h, _, st, _, err = sol.retarget_streams(q0, human, want_errors=True)
        assert (st == 0).all()
        exp = np.array([[[oracle.stage_error(su.mb, su.ts, stage, q_h[s, t], tgt[s, t])[1] for stage in (0, 1)]
                         for t in range(human.shape[1])] for s in range(human.shape[0])])
        d = np.abs(err - exp).max()
        print(f"{name}, {waves} wavefront(s): max |error - oracle error| = {d:.3e}")
        assert d <= 1e-12, (waves, d)
    sol.close()
