"""Per-body state of the motion library, host side: the exports of the library built here, the NumPy mirror
(tests/body_state_mirror.py) against itself on clips of constant rates and against the reference FK fixture
(tests/golden/g_fk.npz), and the argument handling of ``MotionLibrary.body_state`` that needs no device.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_state_mirror as bm  # noqa: E402
import motion_mirror as mm  # noqa: E402
from test_motion_library_host import constant_rate_clip  # noqa: E402

ROBOTS = ["unitree_g1", "booster_t1", "booster_t1_4dof", "stanford_toddy", "fourier_n1", "kuavo_s45", "hightorque_hi"]


def kinematics(robot):
    from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT
    return KinematicsModel(ROBOT_XML_DICT[robot])


def constant_rates(ndof, T=20, fps=50.0, yaw=1.7, seed=0):
    """``constant_rate_clip`` (constant yaw rate) with a linear root track and linear joint angles on top"""
    rng = np.random.default_rng(seed)
    m = constant_rate_clip((0, 0, 1), yaw, T, fps)
    i = np.arange(T)[:, None] / fps
    m["root_pos"] = np.array([0.3, -0.2, 0.8]) + i * np.array([0.7, -0.4, 0.1])
    m["dof_pos"] = rng.uniform(-0.5, 0.5, size=ndof) + i * rng.uniform(-1.0, 1.0, size=ndof)
    m["local_body_pos"] = None
    return m


def test_the_library_exports_the_body_state_entry_points():
    from general_motion_retargeting_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for sym in ("gmr_motion_body_state_dev", "gmr_motion_body_state"):
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
    assert C.sizeof(_lib.BodyStateOut) == 11 * C.sizeof(C.c_void_p)


def rotvec_between(qa, qb):
    """log of qb qa^-1 for xyzw quaternion arrays [..., 4] (normalised first)"""
    shp = qa.shape[:-1]
    qa, qb = qa.reshape(-1, 4), qb.reshape(-1, 4)
    qa = qa / np.linalg.norm(qa, axis=1, keepdims=True)
    qb = qb / np.linalg.norm(qb, axis=1, keepdims=True)
    return mm.rotvec(mm.qmul_xyzw(qb, qa * np.array([-1.0, -1.0, -1.0, 1.0]))).reshape(shp + (3,))


@pytest.mark.parametrize("robot", ROBOTS)
def test_mirror_velocities_are_the_derivatives_of_its_own_pose_on_constant_rates(robot):
    km = kinematics(robot)
    tree = bm.tree_of(km)
    # (the stored local rotations are float32 and 1e-7 off unit length; the walk, like the device, does not normalise them, which
    #  scales R_b a_b by as much per level: 1.5e-6 on the G1.  Unit rotations make the identity exact.)
    tree["r"] = tree["r"] / np.linalg.norm(tree["r"], axis=1, keepdims=True)
    m = constant_rates(km.num_dof, seed=ROBOTS.index(robot))
    dt, yaw = 1.0 / 50.0, 1.7
    rv, dv = (m["root_pos"][1] - m["root_pos"][0]) / dt, (m["dof_pos"][1] - m["dof_pos"][0]) / dt
    h = 2e-5                                    # (the quotient's own error is O(h^2 |w|^3): 6e-8 here)
    t = (np.arange(1, 18) + 0.5) * dt           # mid-interval: t +- h stays inside one frame interval
    n = len(t)

    def state(tt):
        # the clip at time tt, exactly and in float64 (linear tracks, the yaw analytically): a float32 rounding anywhere would
        # show in a difference quotient over 2h
        a = yaw * tt
        step = np.stack([0 * a, 0 * a, np.sin(a / 2), np.cos(a / 2)], axis=1)
        rot = mm.qmul_xyzw(step, np.tile(m["root_rot"][0], (n, 1)))
        return bm.walk(tree, m["root_pos"][0] + tt[:, None] * rv, rot, np.tile(rv, (n, 1)), np.tile([0.0, 0.0, yaw], (n, 1)),
                       m["dof_pos"][0] + tt[:, None] * dv, np.tile(dv, (n, 1)), half_f32=False)

    p0, q0, v, w = state(t)
    pm, qm, _, _ = state(t - h)
    pp, qp, _, _ = state(t + h)
    assert np.abs(v - (pp - pm) / (2 * h)).max() <= 1e-6
    assert np.abs(w - rotvec_between(qm, qp) / (2 * h)).max() <= 1e-6
    assert np.abs(v).max() > 0.5 and np.abs(w[:, 1:] - w[:, :1]).max() > 0.1      # the joints do move the links


@pytest.mark.parametrize("robot", ROBOTS)
def test_mirror_pose_at_frame_times_is_the_reference_fk(robot):
    g = np.load(os.path.join(GOLDEN, "g_fk.npz"))
    km = kinematics(robot)
    tree = bm.tree_of(km)
    rp, rr, dof = g[robot + "__root_pos"], g[robot + "__root_rot"], g[robot + "__dof"]
    m = {"fps": 30.0, "root_pos": rp, "root_rot": rr, "dof_pos": dof}
    lib = mm.Library([m])
    T = len(rp)
    out = bm.body_state(lib, tree, np.zeros(T, int), np.arange(T) / 30.0 + 1e-9, loop=True)
    assert not out["status"].any()
    assert np.abs(out["body_pos"] - g[robot + "__body_pos"]).max() <= 2e-6
    assert np.abs(out["body_rot"] - g[robot + "__body_rot"]).max() <= 2e-6
    assert np.array_equal(out["body_pos"][:, 0], out["root_pos"].astype(np.float64)) and np.array_equal(out["body_vel"][:, 0], out["root_vel"].astype(np.float64))
    sub = bm.body_state(lib, tree, np.zeros(T, int), np.arange(T) / 30.0 + 1e-9, bodies=[5, 2])
    assert np.array_equal(sub["body_vel"], out["body_vel"][:, [5, 2]])
    bad = bm.body_state(lib, tree, [0, 3], [0.1, 0.1])
    assert bad["status"].tolist() == [0, 1] and np.isnan(bad["body_rot"][1]).all() and np.isfinite(bad["body_rot"][0]).all()


class _OfflineLibrary:
    """a ``MotionLibrary`` without a device handle: what the checks in front of the library call look at"""

    def __new__(cls, ndof, ang_vel="world"):
        from general_motion_retargeting_amd.motion_library import MotionLibrary
        lib = MotionLibrary.__new__(MotionLibrary)
        lib.ndof, lib.ang_vel, lib._kinematics, lib.handle = ndof, ang_vel, None, None
        return lib


def test_python_argument_handling_without_a_device():
    km = kinematics("unitree_g1")
    lib = _OfflineLibrary(km.num_dof)
    with pytest.raises(ValueError, match="attach_kinematics"):
        lib.body_state([0], [0.0])
    with pytest.raises(KeyError, match="no_such_link"):
        lib.body_state([0], [0.0], kinematics=km, bodies=["pelvis", "no_such_link"])
    with pytest.raises(ValueError, match="1 to 64"):
        lib.body_state([0], [0.0], kinematics=km, bodies=[])
    with pytest.raises(ValueError, match="1 to 64"):
        lib.body_state([0], [0.0], kinematics=km, bodies=list(range(38)) * 2)
    with pytest.raises(ValueError, match="outside"):
        lib.body_state([0], [0.0], kinematics=km, bodies=[0, 38])
    with pytest.raises(ValueError, match="once"):
        lib.body_state([0], [0.0], kinematics=km, bodies=[3, 3])
    with pytest.raises(ValueError, match="dofs"):
        _OfflineLibrary(12).body_state([0], [0.0], kinematics=km)
    with pytest.raises(ValueError, match="dofs"):
        _OfflineLibrary(12).attach_kinematics(km)
    ref = _OfflineLibrary(km.num_dof, "reference")
    with pytest.raises(ValueError, match='ang_vel="world"'):
        ref.body_state([0], [0.0], kinematics=km)
    with pytest.raises(ValueError, match='ang_vel="world"'):
        ref.body_state_dev(1, 256, 256, kinematics=km)
    assert lib.attach_kinematics(km) is lib and lib._kinematics is km
    names = km.body_names
    sel, nsel = lib._body_selection([names[7], 2], names, len(names))
    assert sel.tolist() == [7, 2] and sel.dtype == np.int32 and nsel == 2
    assert lib._body_selection(None, names, len(names)) == (None, len(names))
