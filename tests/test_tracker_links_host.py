"""The tracker's link step without a GPU: exports and struct layouts against the header, the float64 mirror
(tests/links_mirror.py) against body_state_mirror, hand-computed terms, the heading frame's invariances, and every argument check
that must fire before a device is touched."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_state_mirror as bm  # noqa: E402
import links_mirror as lm  # noqa: E402
import motion_mirror as mm  # noqa: E402
import tracker_mirror as tm  # noqa: E402
from test_motion_body_state_host import _OfflineLibrary, kinematics  # noqa: E402
from test_motion_library import make_motions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK_SYMBOLS = ("gmr_motion_tracker_set_links", "gmr_motion_tracker_set_link_terms", "gmr_motion_tracker_step_links_dev",
                "gmr_motion_tracker_step_links")


def test_the_library_exports_the_link_entry_points():
    from general_motion_retargeting_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for sym in LINK_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "gmr_hip.h")).read()
    for name, struct in (("gmr_tracker_links_out_t", _lib.TrackerLinksOut), ("gmr_tracker_links_sim_t", _lib.TrackerLinksSim)):
        body = re.search(r"typedef struct \{([^}]*)\} " + name, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"[\*\s,](\w+)\s*[,;]", body) == [f for f, _ in struct._fields_], name      # the same fields in the same order
    assert C.sizeof(_lib.TrackerLinksOut) == 8 * C.sizeof(C.c_void_p) and C.sizeof(_lib.TrackerLinksSim) == 4 * C.sizeof(C.c_void_p) + 16
    for k, v in (("GMR_TRACKER_FRAME_WORLD", _lib.TRACKER_FRAME_WORLD), ("GMR_TRACKER_FRAME_HEADING", _lib.TRACKER_FRAME_HEADING),
                 ("GMR_TRACKER_NO_ADVANCE", _lib.TRACKER_NO_ADVANCE), ("GMR_TRACKER_LINK_TERMS", _lib.TRACKER_LINK_TERMS)):
        assert f"#define {k} {v}" in hdr
    # the tracker's own two structs stay as they were
    assert C.sizeof(_lib.TrackerOut) == 11 * C.sizeof(C.c_void_p) and C.sizeof(_lib.TrackerSim) == 6 * C.sizeof(C.c_void_p)


def test_the_link_plan_holds_every_tree_the_fk_handle_accepts(tmp_path):
    """tests/cpp/link_plan_check.cpp replays csrc/gmr_link_plan.h as the kernel walks it.  Every wavefront re-walks its trunk, so a long
    trunk in front of the branching needs up to four walks of the whole tree: more than the 128 records of the FK split."""
    exe = str(tmp_path / "link_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "link_plan_check.cpp")])

    def run(parent, sel=()):
        text = f"{len(parent)} " + " ".join(map(str, parent)) + f" {len(sel)} " + " ".join(map(str, sel))
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (parent, sel, out.stdout, out.stderr)
        return {k: int(v) for k, v in (f.split("=") for f in out.stdout.split()[:3])}

    def trunk(n, leaves, limb=1):
        par = [-1] + list(range(n - 1))
        for _ in range(leaves):
            par += [n - 1] + [len(par) + i for i in range(limb - 1)]
        return par

    rng = np.random.default_rng(0)
    for robot in ("unitree_g1", "booster_t1", "stanford_toddy"):
        par = [int(x) for x in kinematics(robot)._tree["parent"]]
        assert run(par)["steps"] <= 64
        for _ in range(6):
            run(par, rng.permutation(len(par))[:int(rng.integers(1, 9))].tolist())
    assert run(trunk(22, 42)) == {"steps": 130, "waves": 4, "slots": 4}      # 23 levels, which gmr_fk_create takes: 4 x 22 + 42, past 2 x 64
    assert run(trunk(40, 4))["steps"] == 164                      # (deeper than an FK handle goes; the plan holds it all the same)
    assert run(trunk(59, 4))["steps"] == 240
    assert run(trunk(33, 4, limb=6))["steps"] > 128
    assert run(trunk(40, 4), [43, 5, 40]) == {"steps": 82, "waves": 2, "slots": 0}
    assert run([-1] + [(b - 1) // 2 for b in range(1, 63)])["waves"] == 4
    assert run([-1]) == {"steps": 1, "waves": 1, "slots": 0} and run([-1] + list(range(19)))["waves"] == 1
    assert run([int(x) for x in kinematics("unitree_g1")._tree["parent"]], [37])["waves"] == 1
    from general_motion_retargeting_amd import _lib
    assert _lib.FK_MAX_BODIES == 64


def mirror_tracker(km, rng, N=40, loop=True):
    motions = make_motions(rng, [1, 2, 40, 90], km.num_dof, 0)
    t = tm.Tracker(mm.Library(motions, "world"), N, 0.02, loop=loop, seed=5)
    t.assign(rng.integers(0, 4, size=N), rng.uniform(0.0, 2.0, size=N).astype(np.float32))
    return t


def test_world_frame_references_are_body_state_at_the_trackers_clocks():
    km = kinematics("unitree_g1")
    tree, rng = bm.tree_of(km), np.random.default_rng(3)
    t = mirror_tracker(km, rng)
    t.assign([9], [0.5], env_ids=[4])                                   # a bad assignment: NaN rows
    sel = [30, 2, 17, 0, 9, 22]
    ref = lm.references(t, tree, sel)
    want = bm.body_state(t.lib, tree, t.clip, t.time.astype(np.float64), True, sel)
    for k in lm.FIELDS:
        assert np.array_equal(ref["ref_" + k], want[k], equal_nan=True), k
    assert np.isnan(ref["ref_body_pos"][4]).all() and not np.isnan(ref["ref_body_pos"][5]).any()
    # the dof_map does not enter the link targets
    t.set_dof_map(np.full(km.num_dof, -1))
    again = lm.references(t, tree, sel)
    assert all(np.array_equal(again[k], ref[k], equal_nan=True) for k in ref)


def test_terms_on_a_hand_computed_case():
    ref = {"ref_body_pos": np.zeros((2, 3, 3), np.float32), "ref_body_rot": np.tile(np.array([0, 0, 0, 1], np.float32), (2, 3, 1)),
           "ref_body_vel": np.zeros((2, 3, 3), np.float32), "ref_body_ang_vel": np.zeros((2, 3, 3), np.float32)}
    pos = np.zeros((2, 3, 3), np.float32)
    pos[0, 0, 0], pos[0, 1, 1], pos[0, 2, 2] = 3.0, 4.0, 12.0        # distances 3, 4, 12
    pos[1, 1, 0] = np.nan
    rot = np.tile(np.array([0, 0, 0, 1], np.float32), (2, 3, 1))
    rot[0, 0] = [1, 0, 0, 0]                                         # half a turn: theta = pi
    vel = np.zeros((2, 3, 3), np.float32)
    vel[0, :, 0] = 2.0
    err, term, md, fail, total = lm.link_terms(ref, {"body_pos": pos, "body_rot": rot, "body_vel": vel}, link_weight=[1.0, 2.0, 0.0],
                                                scales=(0.3, 0.8, 2.0, 4.0), weights=(1.0, 0.0, 2.0, 1.0), fail_dist=3.5)
    assert np.isclose(err[0, 0], np.sqrt((9.0 + 2 * 16.0) / 3.0)) and np.isclose(err[0, 1], np.pi * np.sqrt(1.0 / 3.0))
    assert np.isclose(err[0, 2], 2.0) and err[0, 3] == 0.0 and term[0, 3] == 0.0       # not given: err = term = 0
    assert md[0] == 4.0 and fail[0] == 1                                                # the link of weight zero (12 m away) is not looked at
    assert np.isclose(total[0], np.exp(-err[0, 0] / 0.3) + 2.0 * np.exp(-1.0))          # weight 0 and the array not given stay out
    assert np.isnan(md[1]) and fail[1] == 1                                             # a NaN distance fails
    _, _, md, fail, _ = lm.link_terms(ref, {"body_pos": pos}, link_weight=[1.0, 2.0, 0.0])
    assert fail.tolist() == [0, 1]                                                      # fail_dist = inf: only the non-finite distance
    _, _, md, fail, _ = lm.link_terms(ref, {"body_vel": vel})
    assert md.tolist() == [0.0, 0.0] and fail.tolist() == [0, 0]


def qz(a):
    return np.array([0.0, 0.0, np.sin(a / 2), np.cos(a / 2)])


def test_heading_frame_is_blind_to_drift_in_x_y_and_yaw_but_not_to_a_roll():
    km = kinematics("booster_t1")
    tree, rng = bm.tree_of(km), np.random.default_rng(8)
    t = mirror_tracker(km, rng, N=12)
    sel = [1, 5, 9, 12]
    ref = lm.references(t, tree, sel, frame="heading")
    world = lm.references(t, tree, sel, frame="world")
    s = t.lib.sample(t.clip, t.time.astype(np.float64), True)
    # a simulator that is the reference plus noise, in the world
    sim = {k: world["ref_" + k] + rng.normal(0, 0.05, world["ref_" + k].shape) for k in lm.FIELDS}
    base = (s["root_pos"].astype(np.float64), s["root_rot"].astype(np.float64))
    e0 = lm.link_terms(ref, sim, base=base)[0]
    assert (e0 > 1e-3).all()

    def moved(q, shift):
        N, n = sim["body_pos"].shape[:2]
        qq = np.broadcast_to(q, (N, n, 4))
        out = {"body_pos": bm.qrot(qq, sim["body_pos"]) + shift, "body_rot": bm.qmul(qq, sim["body_rot"]),
               "body_vel": bm.qrot(qq, sim["body_vel"]), "body_ang_vel": bm.qrot(qq, sim["body_ang_vel"])}
        b = (bm.qrot(np.broadcast_to(q, (N, 4)), base[0]) + shift, bm.qmul(np.broadcast_to(q, (N, 4)), base[1]))
        return out, b

    drift, b = moved(qz(1.1), np.array([3.0, -2.0, 0.0]))
    e1 = lm.link_terms(ref, drift, base=b)[0]
    assert np.abs(e1 - e0).max() < 1e-5          # (float32 storage of the moved rows)
    roll, b = moved(np.array([np.sin(0.2), 0.0, 0.0, np.cos(0.2)]), np.zeros(3))
    e2 = lm.link_terms(ref, roll, base=b)[0]
    assert (np.abs(e2 - e0)[:, 0] > 1e-3).any()
    # a perfect tracker in the world frame
    e = lm.link_terms(world, {k: world["ref_" + k] for k in lm.FIELDS})[0]
    assert np.abs(e[:, [0, 2, 3]]).max() < 1e-5 and np.abs(e[:, 1]).max() < 1e-3


def offline_tracker(ndof, ang_vel="world"):
    from general_motion_retargeting_amd import MotionTracker
    t = MotionTracker.__new__(MotionTracker)
    t._init_state(_OfflineLibrary(ndof, ang_vel), 8, ndof)
    return t


def test_link_arguments_are_refused_before_anything_touches_a_device(monkeypatch):
    from general_motion_retargeting_amd import _lib
    from general_motion_retargeting_amd import motion_tracker as mt
    km = kinematics("unitree_g1")

    def no_device():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    t = offline_tracker(km.num_dof)
    for kw, exc, match in ((dict(bodies=[3, 3]), ValueError, "once"), (dict(bodies=list(range(38)) * 2), ValueError, "1 to 64"),
                           (dict(bodies=[0, 38]), ValueError, "outside"), (dict(bodies=["no_such_link"]), KeyError, "no_such_link"),
                           (dict(bodies=[1, 2], sim_bodies=[0, -1]), ValueError, "sim_bodies"),
                           (dict(bodies=[1, 2], sim_bodies=[0]), ValueError, "sim_bodies"),
                           (dict(bodies=[1, 2], link_weight=[1.0, -1.0]), ValueError, "link_weight"),
                           (dict(bodies=[1, 2], link_weight=[0.0, 0.0]), ValueError, "link_weight"),
                           (dict(bodies=[1, 2], link_weight=[1.0, np.nan]), ValueError, "link_weight"),
                           (dict(bodies=[1, 2], frame="local"), ValueError, "frame")):
        with pytest.raises(exc, match=match):
            t.set_links(km, **kw)
    with pytest.raises(ValueError, match='ang_vel="world"'):
        offline_tracker(km.num_dof, "reference").set_links(km, bodies=[1])
    with pytest.raises(ValueError, match="dofs"):
        offline_tracker(12).set_links(km, bodies=[1])
    for kw in (dict(scales=[1.0] * 3), dict(scales=[0.3, 0.0, 1, 1]), dict(weights={"link_height": 1.0}), dict(fail_dist=0.0),
               dict(fail_dist=float("nan"))):
        with pytest.raises((ValueError, KeyError)):
            t.set_link_terms(**kw)
    # a step: no links attached; heading without the simulator's root; a packed tensor that sim_bodies overruns
    with pytest.raises(ValueError, match="set_links"):
        t.step_links(links={"body_pos": np.zeros((8, 2, 3))})
    t._links = (types.SimpleNamespace(handle=None), 2, np.array([0, 5], np.int32), "heading")
    with pytest.raises(ValueError, match="base_pos"):
        t.step_links(sim={"base_pos": np.zeros((8, 3))}, links={"body_state": np.zeros((8, 6, 13))})
    t._links = (types.SimpleNamespace(handle=None), 2, np.array([0, 5], np.int32), "world")
    with pytest.raises(ValueError, match="reaches body 5"):
        t.step_links(links={"body_state": np.zeros((8, 5, 13))})
    with pytest.raises(ValueError, match="identity"):
        t.step_links(links={"body_pos": np.zeros((8, 2, 3))})
    with pytest.raises(TypeError, match="unknown"):
        t.step_links(links={"body_height": np.zeros((8, 2, 3))})
    assert mt.LINK_TERMS == lm.LINK_TERMS and mt.DEFAULT_LINK_SCALES == lm.DEFAULT_LINK_SCALES
