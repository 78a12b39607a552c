"""The motion library on a real MI355X (csrc/gmr_motion.hip, csrc/gmr_motion_sample.h) at the widths, clips and rotations no robot
reaches: every group width and column sweep of motion_stats_kernel, empty clips, the NaN carry, the quaternion log at its edges
and the float32 slerp at its switches -- against mpmath and float64 evaluations (tests/motion_cases.py).  The bounds and the
constants in them are stated and re-measured on the CPU in tests/test_motion_edges_host.py; nothing here is measured from the device.
Each test makes one pass; the largest library has 327 frames."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_cases as mc  # noqa: E402
import motion_mirror as mm  # noqa: E402
from test_motion_edges_host import ANGVEL_C, ANGVEL_MAX_NEAR_PI, SLERP_BOUND, SLERP_F32_DEV  # noqa: E402
from test_motion_library import _bits, device_library  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- A. fill and stats at every width ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndof", mc.WIDTH_NDOF)
def test_fill_and_stats_at_every_width_with_empty_clips(hip, ndof):
    motions = mc.width_motions(ndof)
    lib = device_library(hip, motions)                       # (NaN rows behind row B of every input)
    mirror = mm.Library(motions)
    nbody = 0 if motions[0]["local_body_pos"] is None else motions[0]["local_body_pos"].shape[1]
    assert (lib.num_clips, lib.num_frames, lib.ndof, lib.nbody) == (len(mc.WIDTH_LENS), sum(mc.WIDTH_LENS), ndof, nbody)
    for k in ("root_pos", "root_rot", "dof_pos", "root_vel", "dof_vel") + (("local_body_pos",) if nbody else ()):
        assert same_bits(lib.array(k), getattr(mirror, k)), k
    assert lib.has_local_body_pos == (nbody > 0)
    stats = lib.array("stats")
    assert stats.shape == (len(mc.WIDTH_LENS), 4, 3 + ndof)
    mean, std = mc.library_stats_reference(ndof)
    u_mean, u_std = float(mc.spacings_off(stats[:, 0], mean).max()), float(mc.spacings_off(stats[:, 1], std).max())
    print(f"\nndof {ndof} (G, sweeps = {mc.group_width(3 + ndof)}): mean {u_mean:.3f}, std {u_std:.3f} float32 spacings from mpmath")
    assert u_mean <= 1.0 and u_std <= 1.0
    rv, rw, dv = lib.array("root_vel"), lib.array("root_ang_vel"), lib.array("dof_vel")
    for c, n in enumerate(mc.WIDTH_LENS):
        s = slice(int(lib.seg_start[c]), int(lib.seg_start[c + 1]))
        v = lib.clip(c)
        assert v.num_frames == n
        if n == 0:                                            # an empty clip: NaN in all four rows, and its view does not raise
            assert np.isnan(stats[c]).all() and np.isnan(v.root_pos_std).all() and np.isnan(v.dof_pos_min).all() and v.root_pos.shape == (0, 3)
            continue
        x = np.concatenate([mirror.root_pos[s], mirror.dof_pos[s]], axis=1)
        assert same_bits(stats[c, 2], x.min(axis=0)) and same_bits(stats[c, 3], x.max(axis=0)), c
        assert np.isnan(stats[c, 1]).all() == (n == 1)
        # the rows next to an empty clip belong to their own clip: no velocity differences across a boundary, every clip has its own dt
        if n == 1:
            assert not rv[s].any() and not rw[s].any() and not dv[s].any()
        else:
            want = (mirror.root_pos[s][1] - mirror.root_pos[s][0]) / F(1.0 / motions[c]["fps"])
            assert same_bits(rv[s][0], want) and same_bits(rv[s][1], want) and same_bits(rw[s][0], rw[s][1]), c
    # root_ang_vel of these clips: the mirror's value to a float32 spacing or the floor (pinned against mpmath below)
    tol = np.maximum(np.spacing(np.abs(mirror.root_ang_vel)).astype(np.float64), 2 * ANGVEL_C * 2.0 ** -52 * 120.0)
    assert (np.abs(rw.astype(np.float64) - mirror.root_ang_vel) <= tol).all()
    # queries: an empty clip is refused, its neighbours answer with their own rows
    empty = [c for c, n in enumerate(mc.WIDTH_LENS) if n == 0]
    got = lib.sample(empty + [0, 1, 3, 8], [0.0] * len(empty) + [0.0, 0.0, 0.0, 0.0], loop=False, local_body_pos=nbody > 0)
    assert got["status"].tolist() == [1] * len(empty) + [0, 0, 0, 0]
    for k in ("root_pos", "root_rot", "dof_pos", "dof_vel"):
        assert np.isnan(got[k][:len(empty)]).all(), k
    rows = [int(lib.seg_start[c]) for c in (0, 1, 3, 8)]
    assert same_bits(got["root_pos"][len(empty):], mirror.root_pos[rows]) and same_bits(got["dof_pos"][len(empty):], mirror.dof_pos[rows])


def test_stats_far_from_zero_and_the_nan_carry(hip):
    """300 frames, 66 columns, root_pos at 1000 +- 1e-3 and one dof column at -500 +- 1e-3: a one-pass or float32 variance is thousands
    of spacings off here (asserted on the CPU).  Then four fills with one NaN each: that column's four values are NaN, every other
    column keeps the bits of the NaN-free fill."""
    clean = device_library(hip, [mc.offset_motion()])
    stats = clean.array("stats")
    mean, std = mc.library_stats_reference("offset")
    u_mean, u_std = float(mc.spacings_off(stats[:, 0], mean).max()), float(mc.spacings_off(stats[:, 1], std).max())
    print(f"\noffset clip: mean {u_mean:.3f}, std {u_std:.3f} float32 spacings from mpmath")
    assert u_mean <= 1.0 and u_std <= 1.0
    mirror = mm.Library([mc.offset_motion()])
    x = np.concatenate([mirror.root_pos, mirror.dof_pos], axis=1)
    assert same_bits(stats[0, 2], x.min(axis=0)) and same_bits(stats[0, 3], x.max(axis=0))
    for place in mc.NAN_PLACES:
        bad = device_library(hip, [mc.offset_motion(place)]).array("stats")
        col = place[1]
        assert np.isnan(bad[0, :, col]).all(), place
        keep = np.arange(stats.shape[2]) != col
        assert same_bits(bad[0][:, keep], stats[0][:, keep]), place


# ---- B. angular velocity and slerp against high precision ----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["world", "reference"])
def test_angular_velocity_against_mpmath(hip, mode):
    """per component one float32 spacing of mpmath's rotvec(q_i q_{i-1}^-1) / dt or ANGVEL_C 2^-52 / dt; the rows within 1e-6 of a half
    turn up to the sign of the whole vector"""
    lib = device_library(hip, [mc.angvel_clip()], mode)
    got = lib.array("root_ang_vel")
    c, n = mc.angvel_floor_needed(got, mode)
    print(f"\n{mode}: the device needs c = {c:.3f} (bound {ANGVEL_C}), {n} of {len(got)} rows compared up to sign")
    assert n <= ANGVEL_MAX_NEAR_PI * len(got)
    assert c <= ANGVEL_C
    assert np.isfinite(got).all() and same_bits(got[0], got[1])


@pytest.mark.parametrize("loop", [True, False])
def test_slerp_at_its_switches_against_float64(hip, loop):
    """dot within 1e-6 of 0.9995, of 0 and of 1 on both sides, q2 = -q1, each in both hemispheres; blends 0, 2^-1074, 1/2, 1 - 2^-24"""
    motions = mc.slerp_motions()
    lib = device_library(hip, motions)
    mirror = mm.Library(motions)
    mirror.root_ang_vel = lib.array("root_ang_vel").copy()    # (pinned above; from here on the lerp is bit for bit)
    clip, time = mc.slerp_queries()
    got = lib.sample(clip, time, loop)
    want = mirror.sample(clip, time, loop)
    assert not got["status"].any() and set(want["branch"].tolist()) == {1, 2, 5, 6}
    for k in ("root_pos", "root_vel", "root_ang_vel", "dof_pos", "dof_vel"):
        assert same_bits(got[k], want[k]), k
    dev = float(np.abs(got["root_rot"] - mc.slerp_f64(mirror, clip, time, loop)).max())
    print(f"\nloop {loop}: device root_rot at most {dev:.3e} from float64 (float32 mirror {SLERP_F32_DEV:.3e}, bound {SLERP_BOUND:.3e})")
    assert dev <= SLERP_BOUND
    # a blend whose float32 image is 0 is answered as the blend 0 is
    assert same_bits(got["root_rot"][time == 5e-324], got["root_rot"][time == 0.0])
