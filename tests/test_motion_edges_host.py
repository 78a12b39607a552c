"""Motion library at the edges of its kernels, host side: the cases of tests/motion_cases.py are what they claim, the NumPy mirror
(tests/motion_mirror.py) stays inside the bounds the GPU tests (tests/test_motion_edges.py) hold the device to, and the constants
of those bounds are what the float32 mirror measures.  No GPU.

The bounds, and where each comes from:

* stats min and max: the bits of the float32 data's min and max (nothing is computed);
* stats mean and std: one float32 spacing of an mpmath evaluation on the float32 data.  The kernel accumulates in FP64 in two passes
  and rounds once: its FP64 result is some 1e-13 relative off, the rounding half a spacing.  The float64 mirror measures 0.50;
* root_ang_vel: per component one float32 spacing of mpmath's value or, where that is smaller, ANGVEL_C 2^-52 / dt (below);
* sampled root_rot: SLERP_BOUND (below)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_cases as mc  # noqa: E402
import motion_mirror as mm  # noqa: E402

F = np.float32

# The absolute floor of the root_ang_vel bound, c 2^-52 / dt.  The kernel forms d = q_i q_{i-1}^-1 in FP64 from two quaternions it
# normalised itself: a normalised component is 2.5 half-spacings off (sum of squares, square root, division), a product of two of
# them 6 with its own rounding, and the four products of a component of d have absolute values that sum to at most |q_i| |q_{i-1}| = 1;
# three additions of partial sums below 1 add 3.  That is 9 half-spacings of 1 = 4.5 x 2^-52 on the vector part, and the log of a
# small rotation doubles it: c = 9.  Where the rotation is not small the error is relative and far below the float32 spacing.
# Needed by the float64 NumPy mirror on the CPU over angvel_clip(): c = 0.89 (world mode), 0.69 (reference mode).
ANGVEL_C = 9.0
ANGVEL_MAX_NEAR_PI = 0.03                                     # of the clip's rows: compared up to the sign of the whole vector

# The largest |float32 NumPy mirror - float64 evaluation of the same statement| over slerp_queries(), both loop modes, any component
# of root_rot: measured on the CPU by test_the_float32_slerp_mirror_stays_within_what_was_measured, never from the device.  The
# device may deviate by twice that plus one float32 spacing at 1 (the rule of fk_trees.bound: its sinf, cosf and acosf are not
# libm's, and a unit quaternion's components are rounded at the spacing of 1 at most).
SLERP_F32_DEV = 1.0202994249475239e-07
SLERP_BOUND = 2.0 * SLERP_F32_DEV + float(np.spacing(F(1.0)))


def test_the_widths_reach_every_group_and_sweep_of_the_stats_kernel():
    ncol = [3 + n for n in mc.WIDTH_NDOF]
    G = [mc.group_width(n) for n in ncol]
    assert {g for g, _ in G} == {4, 8, 16, 32, 64} and {s for _, s in G} == {1, 2, 3}
    assert {4, 8, 16, 32, 64} <= set(ncol) and {5, 9, 65} <= set(ncol)    # ncol == G, and one more column than a group holds
    lens = list(mc.WIDTH_LENS)
    assert lens[-1] == 0 and lens[lens.index(1) + 2] == 0 and 0 in lens[1:-1] and {63, 64, 65, 129} <= set(lens)
    for ndof in mc.WIDTH_NDOF:
        ms = mc.width_motions(ndof)
        assert [len(m["root_pos"]) for m in ms] == lens and all(m["dof_pos"].shape == (n, ndof) for m, n in zip(ms, lens))
        assert all(a["fps"] != b["fps"] for a, b in zip(ms, ms[1:]))
    assert {0 if mc.width_motions(n)[0]["local_body_pos"] is None else mc.width_motions(n)[0]["local_body_pos"].shape[1]
            for n in mc.WIDTH_NDOF} == {0, 1, 3}
    # the NaN places: wavefront 0 lane 0, the last row, a wavefront other than 0 in the first sweep, the second sweep
    assert mc.group_width(3 + mc.OFFSET_NDOF) == (64, 2)
    (r0, c0), (r1, c1), (r2, c2), (r3, c3) = mc.NAN_PLACES
    assert (r0, c0) == (0, 0) and (r1, c1) == (mc.OFFSET_FRAMES - 1, 2) and r2 % 4 != 0 and c2 < 64 and c3 == 65


@pytest.mark.parametrize("ndof", mc.WIDTH_NDOF)
def test_mirror_stats_against_mpmath_and_empty_clips(ndof):
    motions = mc.width_motions(ndof)
    lib = mm.Library(motions)
    mean, std = mc.library_stats_reference(ndof)
    worst = max(float(mc.spacings_off(lib.stats[:, 0], mean).max()), float(mc.spacings_off(lib.stats[:, 1], std).max()))
    print(f"ndof {ndof}: mean / std of the float64 mirror at most {worst:.3f} float32 spacings from mpmath")
    assert worst <= 1.0
    for c, n in enumerate(mc.WIDTH_LENS):
        s = slice(lib.seg[c], lib.seg[c + 1])
        x = np.concatenate([lib.root_pos[s], lib.dof_pos[s]], axis=1)
        if n == 0:                                            # an empty clip has no statistics: NaN in all four rows
            assert np.isnan(lib.stats[c]).all()
            continue
        assert np.array_equal(lib.stats[c, 2], x.min(axis=0)) and np.array_equal(lib.stats[c, 3], x.max(axis=0))
        assert np.isnan(lib.stats[c, 1]).all() == (n == 1) and np.isfinite(lib.stats[c, 0]).all()
        # the rows next to an empty clip belong to their own clip: no difference crosses a boundary, each clip divides by its own dt
        if n == 1:
            assert not lib.root_vel[s].any() and not lib.root_ang_vel[s].any() and not lib.dof_vel[s].any()
        else:
            want = (lib.root_pos[s][1] - lib.root_pos[s][0]) / F(1.0 / motions[c]["fps"])
            assert np.array_equal(lib.root_vel[s][0], want) and np.array_equal(lib.root_vel[s][1], want)
    # a query into an empty clip is refused, its neighbours answer
    empty = [c for c, n in enumerate(mc.WIDTH_LENS) if n == 0]
    out = lib.sample(empty + [0, 1, 8], [0.0] * len(empty) + [0.0, 0.01, 0.02])
    assert out["status"].tolist() == [1] * len(empty) + [0, 0, 0] and np.isnan(out["root_pos"][:len(empty)]).all()
    assert np.array_equal(out["root_pos"][len(empty)], lib.root_pos[0])


def test_mirror_stats_far_from_zero_and_with_a_nan():
    lib = mm.Library([mc.offset_motion()])
    mean, std = mc.library_stats_reference("offset")
    assert mc.spacings_off(lib.stats[:, 0], mean).max() <= 1.0 and mc.spacings_off(lib.stats[:, 1], std).max() <= 1.0
    # what the bound is for: a float32 accumulation and a one-pass variance in FP64 are thousands of spacings off here
    x = np.concatenate([lib.root_pos, lib.dof_pos], axis=1)
    cols = [0, 1, 2, mc.OFFSET_COLUMN]
    assert np.abs(x[:, :3] - 1000).max() <= 1.1e-3 and np.abs(x[:, mc.OFFSET_COLUMN] + 500).max() <= 1.1e-3
    x64 = x.astype(np.float64)
    one_pass = np.sqrt((np.sum(x64 * x64, axis=0) - np.sum(x64, axis=0) ** 2 / len(x)) / (len(x) - 1))
    assert mc.spacings_off(one_pass.astype(F), std[0])[cols].min() > 100
    assert mc.spacings_off(x.std(axis=0, ddof=1, dtype=F), std[0])[cols].min() > 100
    for place in mc.NAN_PLACES:
        bad = mm.Library([mc.offset_motion(place)])
        col = place[1]
        assert np.isnan(bad.stats[0, :, col]).all()
        keep = np.arange(x.shape[1]) != col
        assert np.array_equal(bad.stats[0][:, keep], lib.stats[0][:, keep])


@pytest.mark.parametrize("mode", ["world", "reference"])
def test_mirror_angular_velocity_against_mpmath(mode):
    m = mc.angvel_clip()
    assert len(m["root_rot"]) == mc.ANGVEL_PAIRS + 1
    q = m["root_rot"].astype(F)
    assert (q[1:] == q[:-1]).all(axis=1).any() and (q[1:] == -q[:-1]).all(axis=1).any()            # identical, and its negated twin
    norms = np.linalg.norm(q.astype(np.float64), axis=1)
    assert (np.abs(norms - 0.5) < 1e-6).any() and (np.abs(norms - 2.0) < 1e-6).any()
    assert ((q[1:] != q[:-1]).sum(axis=1) == 1).any()                                             # float32 neighbours
    ref, near, side = mc.angvel_reference(mode)
    ang = np.linalg.norm(ref[1:], axis=1) / mc.ANGVEL_FPS
    for a in (1e-6, 1e-3, 0.2):
        assert (np.abs(ang / a - 1) < 0.2).any(), a
    assert 6 <= near.sum() <= ANGVEL_MAX_NEAR_PI * len(ref)
    if mode == "world":                                       # both sides of the half turn, and the half turn itself
        assert (side[near] < -1e-7).any() and (side[near] > 1e-7).any() and (side[near] == 0).any()
    lib = mm.Library([m], mode)
    c, n = mc.angvel_floor_needed(lib.root_ang_vel, mode)
    print(f"{mode}: the float64 mirror needs c = {c:.3f} (bound {ANGVEL_C}), {n} rows compared up to sign")
    assert c <= ANGVEL_C


def test_the_float32_slerp_mirror_stays_within_what_was_measured():
    pairs = mc.slerp_pairs().astype(np.float64)
    dot = (pairs[:, 0] * pairs[:, 1]).sum(axis=1)
    for d0 in (0.9995, 0.0, 1.0, -0.9995, -1.0):
        near = dot[np.abs(dot - d0) <= 1.2e-6]
        assert len(near) >= 8 and (d0 in (1.0, -1.0) or ((near < d0).any() and (near > d0).any())), d0
    assert (pairs[:, 1] == -pairs[:, 0]).all(axis=1).any() and (pairs[:, 1] == pairs[:, 0]).all(axis=1).any()
    lib = mm.Library(mc.slerp_motions())
    clip, time = mc.slerp_queries()
    worst, seen = 0.0, set()
    for loop in (True, False):
        ok, lo, hi, blend = lib.frames(clip, time, loop)
        assert ok.all() and (hi == lo + 1).all()
        w1 = blend.astype(F)
        assert set(w1.tolist()) == {0.0, 0.5, float(F(1.0) - F(2.0 ** -24))} and (blend > 0).sum() == 3 * len(blend) // 4
        out = lib.sample(clip, time, loop)
        seen |= set(out["branch"].tolist())
        worst = max(worst, float(np.abs(out["root_rot"] - mc.slerp_f64(lib, clip, time, loop)).max()))
    assert seen == {1, 2, 5, 6}                               # normalised lerp and slerp, each also with a flipped hemisphere
    print(f"float32 slerp mirror: largest deviation from float64 {worst!r} (measured {SLERP_F32_DEV!r}, device bound {SLERP_BOUND!r})")
    assert worst <= SLERP_F32_DEV


def test_clip_view_of_an_empty_clip():
    """``ClipView`` slices whatever the library holds: an empty clip gives empty arrays and the NaN stats row, and does not raise"""
    from general_motion_retargeting_amd.motion_library import ClipView

    class Lib:
        num_clips, seg_start, fps_list, link_body_lists, has_local_body_pos = 3, np.array([0, 2, 2, 5]), [30.0, 50.0, 30.0], [[], [], []], False
        mirror = mm.Library([{"fps": 30.0, "root_pos": np.ones((n, 3)), "root_rot": np.tile([0, 0, 0, 1.0], (n, 1)), "dof_pos": np.zeros((n, 2))}
                             for n in (2, 0, 3)])

        def array(self, name):
            return getattr(self.mirror, name)

    v = ClipView(Lib(), 1)
    assert v.num_frames == 0 and v.motion_duration == 0.0 and v.root_pos.shape == (0, 3) and v.dof_vel.shape == (0, 2)
    for s in ("mean", "std", "min", "max"):
        assert np.isnan(getattr(v, f"root_pos_{s}")).all() and np.isnan(getattr(v, f"dof_pos_{s}")).all()
    assert np.array_equal(ClipView(Lib(), 2).root_pos_mean, F([1, 1, 1]))
