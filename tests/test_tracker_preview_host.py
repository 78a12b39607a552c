"""The tracker's preview without a GPU: exports and constants against the header, the NumPy mirror
(tests/preview_mirror.py) against the sampler's mirror, the valid mask on a hand-made clip, the invariances of the anchored frames, the
layout arithmetic, and every argument check that must fire before a device is touched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_mirror as mm  # noqa: E402
import preview_mirror as pm  # noqa: E402
import tracker_mirror as tm  # noqa: E402
from test_motion_body_state_host import _OfflineLibrary  # noqa: E402
from test_motion_library import _bits, make_motions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREVIEW_SYMBOLS = ("gmr_motion_tracker_set_preview", "gmr_motion_tracker_preview_dev", "gmr_motion_tracker_preview")
F = np.float32


def test_the_library_exports_the_preview_entry_points():
    from general_motion_retargeting_amd import _lib
    from general_motion_retargeting_amd import motion_tracker as mt
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmr_hip.h")).read()
    for sym in PREVIEW_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
    for name, bit in _lib.PREVIEW_BLOCKS.items():
        assert f"#define GMR_PREVIEW_{name.upper()} {bit}\n" in hdr
    assert tuple(_lib.PREVIEW_BLOCKS) == mt.PREVIEW_BLOCKS == pm.BLOCKS and _lib.PREVIEW_BLOCKS == pm.BITS
    for k, v in (("FRAME_RAW", _lib.PREVIEW_FRAME_RAW), ("FRAME_REFERENCE", _lib.PREVIEW_FRAME_REFERENCE), ("FRAME_SIM", _lib.PREVIEW_FRAME_SIM),
                 ("MAX_OFFSETS", _lib.PREVIEW_MAX_OFFSETS), ("MAX_BODIES", _lib.PREVIEW_MAX_BODIES)):
        assert f"#define GMR_PREVIEW_{k} {v}\n" in hdr
    assert mt.PREVIEW_FRAMES == {"raw": 0, "reference": 1, "sim": 2} == {f: i for i, f in enumerate(pm.FRAMES)}
    assert (mt.PREVIEW_MAX_OFFSETS, mt.PREVIEW_MAX_BODIES) == (16, 32) == (_lib.PREVIEW_MAX_OFFSETS, _lib.PREVIEW_MAX_BODIES)


def mirror_tracker(rng, N=60, loop=True, ndof=9, nbody=7, **kw):
    motions = make_motions(rng, [1, 2, 40, 90], ndof, nbody)
    t = tm.Tracker(mm.Library(motions, "world"), N, 0.02, loop=loop, seed=5, **kw)
    t.assign(rng.integers(0, 4, size=N), rng.uniform(0.0, 2.0, size=N).astype(F))
    return t


@pytest.mark.parametrize("loop", [True, False])
def test_raw_frame_is_the_sampler_at_the_float64_sum_of_clock_and_offset(loop):
    rng = np.random.default_rng(21 + loop)
    dmap = np.array([3, -1, 0, 8, 8, -1, 5], dtype=np.int64)
    default = rng.uniform(-1, 1, size=7).astype(F)
    t = mirror_tracker(rng, loop=loop, dof_map=dmap, dof_default=default)
    before = t.state()
    offsets = np.array([0.0, 0.02, -0.7, 1e-3, 250.0], dtype=F)          # a negative one, a far-future one
    bodies = [6, 0, 3]
    out = pm.preview(t, offsets, pm.BLOCKS, "raw", bodies)
    lay = out["layout"]
    assert lay["row_width"] == 3 + 4 + 6 + 3 + 3 + 7 + 7 + 9 and out["obs"].shape == (60, 5, 42)
    on = dmap >= 0
    for k, off in enumerate(offsets):
        s = t.lib.sample(t.clip, t.time.astype(np.float64) + np.float64(off), loop, local_body_pos=True)
        assert not s["status"].any()
        row = out["obs"][:, k]
        for b, key in (("root_pos", "root_pos"), ("root_quat", "root_rot"), ("root_vel", "root_vel"), ("root_ang_vel", "root_ang_vel")):
            assert np.array_equal(row[:, lay[b]].astype(F), s[key]), (b, k)
        assert np.array_equal(row[:, lay["dof_pos"]][:, on].astype(F), s["dof_pos"][:, dmap[on]])
        assert np.array_equal(row[:, lay["dof_vel"]][:, on].astype(F), s["dof_vel"][:, dmap[on]])
        assert np.array_equal(row[:, lay["dof_pos"]][:, ~on].astype(F), np.tile(default[~on], (60, 1)))
        assert not row[:, lay["dof_vel"]][:, ~on].any()
        assert np.array_equal(row[:, lay["body_pos"]].astype(F), s["local_body_pos"][:, bodies].reshape(60, 9))
        assert np.allclose(row[:, lay["root_rot6"]], pm.rot6(s["root_rot"].astype(np.float64)), rtol=0, atol=1e-15)
    # without the rot6 block the rows are float32, the sampler's bits; nothing of the tracker has moved
    six = pm.preview(t, offsets, ("root_pos", "root_quat", "dof_vel"), "raw")
    assert six["obs"].dtype == F and np.array_equal(_bits(six["obs"][:, :, :3]), _bits(out["obs"][:, :, lay["root_pos"]].astype(F)))
    after = t.state()
    assert all(np.array_equal(before[k], after[k]) for k in ("clip", "time", "length", "draws"))
    # a bad assignment: NaN rows, valid 0, status 1
    t.assign([4, 1], [0.5, np.nan], env_ids=[7, 9])
    bad = pm.preview(t, offsets, pm.BLOCKS, "raw", bodies)
    assert bad["status"].tolist() == [int(e in (7, 9)) for e in range(60)]
    assert np.isnan(bad["obs"][[7, 9]]).all() and not np.isnan(bad["obs"][8]).any() and not bad["valid"][[7, 9]].any()


def test_valid_marks_the_queries_inside_the_clip():
    T, fps = 9, 64.0                       # duration 9 / 64, the last frame at 8 / 64 = 0.125: all exact in float32
    z = np.zeros((T, 3))
    clip = {"fps": fps, "root_pos": z, "root_rot": np.tile([0.0, 0.0, 0.0, 1.0], (T, 1)), "dof_pos": z, "local_body_pos": None}
    one = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in clip.items()}
    lib = mm.Library([clip, one], "world")
    last = F(0.125)
    times = np.array([0.0625, last, np.nextafter(last, F(1)), 0.0, 0.0, 0.0, 0.0], dtype=F)
    clips = np.array([0, 0, 0, 0, 1, 1, 2])
    offsets = np.array([0.0, -0.0625, 0.0625, 1.0], dtype=F)
    for loop in (True, False):
        t = tm.Tracker(lib, len(times), 0.02, loop=loop)
        t.assign(clips, times)
        v = pm.preview(t, offsets, ("root_pos",))["valid"]
        assert v.tolist() == [[1, 1, 1, 0],        # inside; 0 exactly; the last frame exactly; past the end
                              [1, 1, 0, 0],        # the last frame exactly; inside; past
                              [0, 1, 0, 0],        # one ulp past the last frame
                              [1, 0, 1, 0],        # a negative query
                              [1, 0, 0, 0],        # T = 1: only tq = 0
                              [1, 0, 0, 0],
                              [0, 0, 0, 0]]        # a clip id outside the library
    assert np.array_equal(pm.valid_mask(lib, [0], [np.nan], [0.0]), [[0]])


def qz(a):
    return np.array([0.0, 0.0, np.sin(a / 2), np.cos(a / 2)])


def qmul(a, b):
    return mm.qmul_xyzw(np.atleast_2d(a).reshape(-1, 4), np.atleast_2d(b).reshape(-1, 4))


def test_anchored_frames_are_blind_to_a_common_translation_and_yaw_but_not_to_a_roll():
    rng = np.random.default_rng(31)
    t = mirror_tracker(rng, N=25)
    offsets = np.array([0.04, 0.0, 0.1, -0.05], dtype=F)
    bodies = [2, 5]
    blocks = ("root_pos", "root_quat", "root_rot6", "root_vel", "root_ang_vel", "body_pos", "dof_pos")
    ref = pm.preview(t, offsets, blocks, "reference", bodies)
    lay = ref["layout"]
    # At offset 0 the reference frame sees its own anchor: no displacement and a q_rel without yaw.  The heading frame of 6l takes the
    # twist of q about z out, so "without yaw" is q_rel.z = 0 for every root; the heading of column 0, atan2(col0.y, col0.x) =
    # atan2(2 x y, ..) of q_rel, is zero as well only where the root is not tilted about both x and y (checked on pure yaws below).
    at0 = ref["obs"][:, 1]
    assert np.abs(at0[:, lay["root_pos"]]).max() < 1e-12
    q_rel = at0[:, lay["root_quat"]]
    assert np.abs(np.arctan2(q_rel[:, 2], q_rel[:, 3])).max() < 1e-12
    yaws = np.stack([qz(a) for a in rng.uniform(-3.0, 3.0, size=25)])
    flat = pm.transform({"root_quat": yaws[:, None, :]}, np.zeros((25, 3)), yaws)
    col0 = flat["root_rot6"][:, 0, :3]
    assert np.abs(np.arctan2(col0[:, 1], col0[:, 0])).max() < 1e-12 and np.abs(flat["root_quat"][:, 0] - [0, 0, 0, 1]).max() < 1e-12
    # the sim frame with the anchor on the reference root is the reference frame
    a = pm.raw_rows(t, [0.0])
    sim = {"base_pos": a["root_pos"][:, 0], "base_quat": a["root_quat"][:, 0]}
    same = pm.preview(t, offsets, blocks, "sim", bodies, sim)
    assert np.array_equal(same["obs"], ref["obs"]) and np.array_equal(same["valid"], ref["valid"])
    # the dofs are the raw ones in every frame
    raw = pm.preview(t, offsets, blocks, "raw", bodies)
    assert np.array_equal(ref["obs"][:, :, lay["dof_pos"]].astype(F), raw["obs"][:, :, lay["dof_pos"]].astype(F))
    # sampled rows and anchor moved alike, in float64.  R(q) takes q as it is, and the float32 slerp leaves |q| = 1 +- 1e-7, for which
    # R(a q) = R(a) R(q) holds to 1e-7 only: the invariance is a property of rotations, so the rows are normalised in float64 first.
    rows = {k: v.astype(np.float64) for k, v in pm.raw_rows(t, offsets, bodies).items() if k in ("root_pos", "root_quat", "root_vel", "root_ang_vel", "body_pos")}
    rows["root_quat"] /= np.linalg.norm(rows["root_quat"], axis=-1, keepdims=True)
    anchor_p = rng.normal(0, 1, (25, 3))
    anchor_q = rng.normal(size=(25, 4))
    anchor_q /= np.linalg.norm(anchor_q, axis=1, keepdims=True)
    base = pm.transform(rows, anchor_p, anchor_q)

    def moved(q, shift):
        N, K = rows["root_pos"].shape[:2]
        qq = np.broadcast_to(q, (N, K, 4))
        out = {"root_pos": pm.qrot(qq, rows["root_pos"]) + shift, "root_quat": qmul(qq, rows["root_quat"]).reshape(N, K, 4),
               "root_vel": pm.qrot(qq, rows["root_vel"]), "root_ang_vel": pm.qrot(qq, rows["root_ang_vel"]), "body_pos": rows["body_pos"]}
        return pm.transform(out, pm.qrot(np.broadcast_to(q, (N, 4)), anchor_p) + shift, qmul(np.broadcast_to(q, (N, 4)), anchor_q))

    drift = moved(qz(1.1), np.array([3.0, -2.0, 0.0]))
    for k in base:
        d = np.abs(drift[k] - base[k])
        if k in ("root_quat",):            # q and -q are one rotation
            d = np.minimum(d, np.abs(drift[k] + base[k]))
        assert d.max() < 1e-9, k
    roll = moved(np.array([np.sin(0.2), 0.0, 0.0, np.cos(0.2)]), np.zeros(3))
    for k in ("root_pos", "root_rot6", "root_vel", "body_pos"):
        assert np.abs(roll[k] - base[k]).max() > 1e-3, k


def offline_tracker(ndof=29, ang_vel="world", nbody=12, has_body=True, link_body_lists=None):
    from general_motion_retargeting_amd import MotionTracker
    t = MotionTracker.__new__(MotionTracker)
    lib = _OfflineLibrary(ndof, ang_vel)
    lib.nbody, lib.has_local_body_pos, lib.num_clips = nbody, has_body, 3
    lib.link_body_lists = link_body_lists if link_body_lists is not None else [[] for _ in range(3)]
    t._init_state(lib, 8, ndof)
    return t


def test_layout_arithmetic():
    t = offline_tracker()
    assert t.preview_layout is None
    t._preview = (3, ("root_pos", "root_rot6", "dof_pos", "dof_vel", "body_pos"), "reference", 4)
    lay = t.preview_layout
    assert lay == {"root_pos": slice(0, 3), "root_rot6": slice(3, 9), "dof_pos": slice(9, 38), "dof_vel": slice(38, 67), "body_pos": slice(67, 79),
                   "row_width": 79}
    assert lay == pm.layout(t._preview[1], 29, 4)
    t.nrobot_dof = 23                     # what set_dof_map leaves behind: R, and with it D, has changed
    assert t.preview_layout["row_width"] == 67 and t.preview_layout["body_pos"] == slice(55, 67)
    assert pm.layout(pm.BLOCKS, 64, 32)["row_width"] == 243               # the widest row: 16 of them are 15 552 bytes of LDS
    # the checks hand the library the blocks in row order whatever order they were named in
    off, names, bits, sel = t._preview_setup([0.0, 0.02], ("dof_vel", "root_pos", "body_pos"), "sim", [5, 1])
    assert names == ("root_pos", "dof_vel", "body_pos") and bits == 1 + 64 + 128 and sel.tolist() == [5, 1] and off.dtype == F
    lists = [["pelvis", "left_foot", "right_foot"]] * 3
    assert offline_tracker(link_body_lists=lists)._preview_setup([0.0], ("body_pos",), "raw", ["right_foot", 0])[3].tolist() == [2, 0]


def test_preview_arguments_are_refused_before_anything_touches_a_device(monkeypatch):
    from general_motion_retargeting_amd import _lib

    def no_device():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    t = offline_tracker()
    for kw, exc, match in ((dict(offsets=[0.0] * 17), ValueError, "1 to 16"),
                           (dict(offsets=[0.0, np.inf]), ValueError, "finite"),
                           (dict(offsets=[0.0, np.nan]), ValueError, "finite"),
                           (dict(offsets=[0.0], blocks=("root_pos", "root_height")), ValueError, "root_height"),
                           (dict(offsets=[0.0], blocks=()), ValueError, "at least one block"),
                           (dict(offsets=[0.0], frame="heading"), ValueError, "frame"),
                           (dict(offsets=[0.0], blocks=("body_pos",)), ValueError, "bodies"),
                           (dict(offsets=[0.0], blocks=("body_pos",), bodies=[]), ValueError, "bodies"),
                           (dict(offsets=[0.0], blocks=("body_pos",), bodies=[0, 12]), ValueError, "outside"),
                           (dict(offsets=[0.0], blocks=("body_pos",), bodies=[-1]), ValueError, "outside"),
                           (dict(offsets=[0.0], blocks=("body_pos",), bodies=[3, 3]), ValueError, "once"),
                           (dict(offsets=[0.0], blocks=("body_pos",), bodies=["pelvis"]), ValueError, "link_body_list"),
                           (dict(offsets=[0.0], blocks=("root_pos",), bodies=[1]), ValueError, "body_pos")):
        with pytest.raises(exc, match=match):
            t.set_preview(**kw)
    with pytest.raises(ValueError, match="1 to 32"):
        offline_tracker(nbody=40).set_preview([0.0], blocks=("body_pos",), bodies=list(range(33)))
    with pytest.raises(ValueError, match="local_body_pos"):
        offline_tracker(has_body=False).set_preview([0.0], blocks=("body_pos",), bodies=[0])
    lists = [["pelvis", "left_foot"], ["pelvis", "left_foot"], ["pelvis"]]
    with pytest.raises(ValueError, match="link_body_list"):
        offline_tracker(link_body_lists=lists).set_preview([0.0], blocks=("body_pos",), bodies=["pelvis"])
    with pytest.raises(KeyError, match="no_such_link"):
        offline_tracker(link_body_lists=[["pelvis"]] * 3).set_preview([0.0], blocks=("body_pos",), bodies=["no_such_link"])
    for frame in ("reference", "sim"):
        with pytest.raises(ValueError, match='ang_vel="world"'):
            offline_tracker(ang_vel="reference").set_preview([0.0], frame=frame)
    offline_tracker(ang_vel="reference")._preview_setup([0.0], ("root_pos", "root_ang_vel"), "raw", None)      # as sampled: allowed
    offline_tracker(ang_vel="reference")._preview_setup([0.0], ("root_pos", "root_vel"), "reference", None)
    # a preview: none configured; the sim frame without the simulator's root; an unknown array
    for call in (t.preview, t.preview_dev):
        with pytest.raises(ValueError, match="set_preview"):
            call()
    t._preview = (2, ("root_pos",), "sim", 0)
    for call in (t.preview, t.preview_dev):
        with pytest.raises(ValueError, match="base_pos"):
            call()
        with pytest.raises(ValueError, match="base_pos"):
            call({"base_pos": np.zeros((8, 3), F)})
        with pytest.raises(TypeError, match="unknown"):
            call({"base_height": np.zeros(8, F)})
    with pytest.raises(ValueError, match="shape"):
        t.preview({"base_pos": np.zeros((8, 3), F), "base_quat": np.zeros((7, 4), F)})
    with pytest.raises(TypeError, match="device address"):
        t.preview_dev({"base_pos": np.zeros((8, 3), F), "base_quat": np.zeros((8, 4), F)})
