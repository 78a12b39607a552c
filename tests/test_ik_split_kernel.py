"""-m gpu: the latency kernel with its evaluation after a solve split over two wavefronts (helper 1 walks the tree, the main
wavefront the rotations; csrc/gmr_ik.hip), both launch shapes against the oracle.  Pass conditions as in
tests/test_ik_bound_path.py: status 0, solve counts equal, |q - q_oracle| <= 1e-8, four wavefronts against one <= 1e-12.

Cases: the joint-limit input of test_ik_bound_path (G1, S=6, T=10, seed 21, scattered: many solves per frame), every shipped
configuration at S=3, T=8, a ragged batch with a zero-length and a one-frame stream, and the per-frame output (T=1) of both
error norms against the oracle's stage errors.
"""
import numpy as np
import pytest

from conftest import ALL_CONFIGS, get_setup
from test_ik_bound_path import _both_shapes, _scatter

pytestmark = pytest.mark.gpu

Q_ORACLE_TOL = 1e-8
Q_SHAPES_TOL = 1e-12


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _check(out, q_o, ns_o, what, lens=None):
    T = q_o.shape[1]
    live = np.ones(q_o.shape[:2], dtype=bool) if lens is None else (np.arange(T)[None, :] < np.asarray(lens)[:, None])
    for waves, (q_h, ns_h, st_h) in out.items():
        assert (st_h == 0).all(), (what, waves)
        assert np.array_equal(ns_h[live], ns_o[live]), f"{what}, {waves} wavefront(s): solve counts differ from the oracle's"
        err = np.abs(q_h[live] - q_o[live]).max() if live.any() else 0.0
        print(f"{what}, {waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
        assert err <= Q_ORACLE_TOL, (what, waves, err)
    assert np.array_equal(out[4][1][live], out[1][1][live])
    d = np.abs(out[4][0][live] - out[1][0][live]).max() if live.any() else 0.0
    print(f"{what}: max |q_4 - q_1| = {d:.3e}")
    assert d <= Q_SHAPES_TOL, (what, d)


@pytest.fixture(scope="module")
def limits_input(oracle, g1):
    """G1, S=6, T=10, seed 21, scattered, and the oracle's answer.  Shared, never modified."""
    from general_motion_retargeting_amd import synth
    human, q0 = synth.make_streams(g1.model, g1.tt, 6, 10, seed=21)
    human = _scatter(human)
    q_o, ns_o, st_o = oracle.retarget_streams(g1.mb, g1.ts, q0, human)
    assert (st_o == 0).all()
    for a in (q0, human, q_o, ns_o):
        a.setflags(write=False)
    return q0, human, q_o, ns_o


def test_joint_limit_input(hip, g1, limits_input):
    q0, human, q_o, ns_o = limits_input
    assert ns_o.sum() >= 4 * ns_o[..., 0].size, "the input must take many solves per frame"
    _check(_both_shapes(hip, g1.mb, g1.ts, q0, human), q_o, ns_o, "G1 on its joint limits")


@pytest.mark.parametrize("src,robot", ALL_CONFIGS)
def test_all_configs(hip, oracle, src, robot):
    from general_motion_retargeting_amd import synth
    su = get_setup(src, robot, 1.7)
    human, q0 = synth.make_streams(su.model, su.tt, 3, 8, seed=5)
    human = _scatter(human)
    q_o, ns_o, st_o = oracle.retarget_streams(su.mb, su.ts, q0, human)
    assert (st_o == 0).all()
    _check(_both_shapes(hip, su.mb, su.ts, q0, human), q_o, ns_o, f"{src}/{robot}")


def test_ragged_lengths(hip, oracle, g1, limits_input):
    """lens = (10, 0, 1, 7, 10, 3): a stream without a frame never posts a command to its helpers, a one-frame stream posts
    its last one in its first frame.  Every stream's live frames equal the oracle's (frames of a stream depend on its
    earlier frames only)."""
    q0, human, q_o, ns_o = limits_input
    lens = np.array([10, 0, 1, 7, 10, 3], dtype=np.int32)
    sol = hip.Solver(g1.mb, g1.ts)
    out = {}
    for waves in (4, 1):
        sol.set_waves(waves)
        out[waves] = sol.retarget_streams(q0, human, lens=lens)
    sol.close()
    _check(out, q_o, ns_o, "ragged", lens)


def test_per_frame_errors(hip, oracle, g1, limits_input):
    """T = 1 with the error output, as the per-frame API launches it: error1 / error2 at the configuration the frame ends with
    against the oracle's stage errors there, to 1e-12 (the bound of tests/test_ik_jlinv_apply.py: norms of O(1) residuals)."""
    q0, human, _, _ = limits_input
    human = np.ascontiguousarray(human[:, :1])
    tgt = oracle.preprocess(g1.ts, human)
    q_o, ns_o, _ = oracle.retarget_streams(g1.mb, g1.ts, q0, human)
    sol = hip.Solver(g1.mb, g1.ts)
    for waves in (4, 1):
        sol.set_waves(waves)
        q_h, ns_h, st, _, err = sol.retarget_streams(q0, human, want_errors=True)
        assert (st == 0).all()
        assert np.array_equal(ns_h, ns_o)
        assert np.abs(q_h - q_o).max() <= Q_ORACLE_TOL
        exp = np.array([[[oracle.stage_error(g1.mb, g1.ts, stage, q_h[s, 0], tgt[s, 0])[1] for stage in (0, 1)]]
                        for s in range(human.shape[0])])
        d = np.abs(err - exp).max()
        print(f"{waves} wavefront(s): max |error - oracle error| = {d:.3e}")
        assert d <= 1e-12, (waves, d)
    sol.close()
