"""The motion tracker, host side: the exports of the library built here, the Philox4x32-10 of the mirror and of the product header
against known-answer vectors, the float32 clock against a torch tensor, the NumPy mirror (tests/tracker_mirror.py) against the
fixture generated from the reference's loader (tests/golden/g_tracker.npz), and the argument handling of ``MotionTracker`` that
needs no device.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_mirror as mm  # noqa: E402
import tracker_mirror as tm  # noqa: E402
from test_motion_library_host import close  # noqa: E402

F = np.float32
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                 ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                 ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
TRACKER_SYMBOLS = ("gmr_motion_tracker_create", "gmr_motion_tracker_destroy", "gmr_motion_tracker_set_dof_map", "gmr_motion_tracker_set_terms",
                   "gmr_motion_tracker_assign_dev", "gmr_motion_tracker_assign", "gmr_motion_tracker_reset_dev", "gmr_motion_tracker_reset",
                   "gmr_motion_tracker_step_dev", "gmr_motion_tracker_step", "gmr_motion_tracker_state")


def golden():
    return np.load(os.path.join(GOLDEN, "g_tracker.npz"), allow_pickle=False)


def golden_library(g, ang_vel="reference"):
    return mm.Library([{k: g[f"c{c}_{k}"] for k in ("root_pos", "root_rot", "dof_pos")} | {"fps": float(g[f"c{c}_fps"])}
                       for c in range(int(g["nclip"]))], ang_vel)


def test_the_library_exports_the_tracker_entry_points():
    from general_motion_retargeting_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for sym in TRACKER_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
    assert C.sizeof(_lib.TrackerOut) == 11 * C.sizeof(C.c_void_p) and C.sizeof(_lib.TrackerSim) == 6 * C.sizeof(C.c_void_p)
    hdr = open(os.path.join(ROOT, "include", "gmr_hip.h")).read()
    for name, struct in (("gmr_tracker_out_t", _lib.TrackerOut), ("gmr_tracker_sim_t", _lib.TrackerSim)):
        body = re.search(r"typedef struct \{([^}]*)\} " + name, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"\*(\w+)", body) == [f for f, _ in struct._fields_], name       # the same fields in the same order
    assert f"#define GMR_TRACKER_MAX_DOF {_lib.TRACKER_MAX_DOF}" in hdr


def test_philox_of_the_mirror_gives_the_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        assert " ".join("%08x" % w for w in tm.philox4x32(ctr, key)) == want


def test_philox_of_the_product_header_gives_the_known_answers(tmp_path):
    exe = str(tmp_path / "philox_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "philox_check.cpp")])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[:3] == [want for _, _, want in KNOWN_ANSWERS]
    u0, u1, b0, b1 = lines[3].split()
    assert float(u0) == 0.0 and F(float(u1)) == F(1) - F(2.0 ** -24) and (int(b0), int(b1)) == (0, 6)


def test_draws_depend_on_the_environment_and_the_draw_number_alone():
    lib = mm.Library([{"fps": 30.0, "root_pos": np.zeros((5, 3)), "root_rot": np.tile([0, 0, 0, 1.0], (5, 1)), "dof_pos": np.zeros((5, 2))}] * 7)
    a, b = tm.Tracker(lib, 64, 0.02, seed=11), tm.Tracker(lib, 5000, 0.02, seed=11)
    b.reset([4999, 3, 7])                      # other environments first: no effect on environment 7's sequence
    seq = []
    for t in (a, b):
        t.reset([7], time_offset_range=(0.5, 2.0))
        t.reset([7], resample=False, time_offset_range=(0.0, 1.0))
        seq.append((t.clip[7], t.time[7], t.draws[7] - (t is b)))
    assert seq[0][0] != 0 or seq[0][1] != 0
    assert a.draws[7] == 2 and b.draws[7] == 3 and a.clip[3] == 0 and b.draws[3] == 1
    # the first draw of environment 0 under seed 0 is the first known answer
    t = tm.Tracker(lib, 1, 0.02, seed=0)
    t.reset(time_offset_range=(0.0, 1.0))
    assert t.clip[0] == (0x6627E8D5 * 7) >> 32 and t.time[0] == F(0xE169C58D >> 8) * F(2.0 ** -24)


def test_weighted_draws_never_take_a_clip_of_weight_zero():
    w = np.array([0.0, 3.0, 0.0, 0.0, 1.0, 0.0])
    cdf = tm.clip_cdf(w)
    assert cdf[0] == 0.0 and cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all()
    for x in (0.0, 0.75 - 2.0 ** -32, 0.75, 1.0 - 2.0 ** -32):
        k = int(np.searchsorted(cdf, x, side="right")) - 1
        assert w[k] > 0 and k == (1 if x < 0.75 else 4)


def test_the_float32_clock_is_the_reference_tensor_incremented_in_place():
    import torch
    for dt in (0.02, 1.0 / 60.0, 0.001):
        times = torch.tensor([0.0, 0.333, 17.123, 4096.5], dtype=torch.float32)
        mine = times.numpy().copy()
        dtf = F(dt)
        for _ in range(3000):
            times += dt                         # t1_imitation.py:198
            mine = (mine + dtf).astype(F)
        assert np.array_equal(times.numpy().view(np.uint32), mine.view(np.uint32)), dt


def test_mirror_reproduces_the_reference_loop():
    g = golden()
    lib = golden_library(g)
    steps, envs = g["s_time"].shape
    t = tm.Tracker(lib, envs, float(g["dt"]), dof_map=g["map_stage1"], dof_default=g["dof_default"], scales=g["scales"])
    seen_maps = set()
    for s in range(steps):
        for s_, e, c, tt in g["script"]:
            if int(s_) == s:
                t.assign([int(c)], [tt], [int(e)])
        if s == int(g["stage2_from"]):
            t.set_dof_map(g["map_full"], g["dof_default"])
        seen_maps.add(tuple(t.map))
        assert np.array_equal(t.clip, g["s_clip"][s])
        assert np.array_equal(t.time.view(np.uint32), g["s_time"][s].view(np.uint32)), s      # the clocks: bit for bit
        out = t.step({k: g[f"s_{k}"][s] for k in tm.SIM})
        assert not out["status"].any() and not out["finished"].any()
        # the bounds under which the sampler's mirror reproduces the loader (test_motion_library_host.check_against_golden)
        for k in ("ref_root_pos", "ref_root_vel", "ref_dof_pos", "ref_dof_vel"):
            close(out[k], g[f"s_{k}"][s], rel=1e-6, abs_=1e-7)
        close(out["ref_root_rot"], g["s_ref_root_rot"][s], abs_=1e-6)
        close(out["ref_root_ang_vel"], g["s_ref_root_ang_vel"][s], rel=1e-6, abs_=1e-5)
        # where the map says -1 the rows are the defaults and zero, exactly
        off = t.map < 0
        assert np.array_equal(out["ref_dof_pos"][:, off], np.tile(t.default[off], (envs, 1))) and not out["ref_dof_vel"][:, off].any()
        # the terms hang on rows that agree to 1e-6 .. 1e-5; the reference's float32 formulas on ITS rows are within:
        close(out["err"], g["s_err"][s], rel=2e-5, abs_=2e-5)
        close(out["term"], g["s_term"][s], rel=1e-4, abs_=2e-5)
        # ... and the formulas themselves, on the reference's own rows: 1e-6
        err64 = formulas(g, s)
        rest = [0, 2, 3, 4, 5]
        close(err64[:, rest], g["s_err"][s][:, rest], rel=1e-6, abs_=1e-6)
        close(np.exp(-err64 / g["scales"])[:, rest], g["s_term"][s][:, rest], rel=1e-6, abs_=1e-6)
        # (the angle: 2 acos(x) turns the float32 rounding of x, 6e-8, into 1.2e-7 / sin(angle / 2))
        room = 1e-6 + 4e-7 / np.sin(err64[:, 1] / 2)
        assert (np.abs(err64[:, 1] - g["s_err"][s][:, 1]) < room).all()
        assert (np.abs(np.exp(-err64[:, 1] / g["scales"][1]) - g["s_term"][s][:, 1]) < room / g["scales"][1]).all()
    assert len(seen_maps) == 2
    assert np.array_equal(t.time.view(np.uint32), g["final_time"].view(np.uint32))


def formulas(g, s):
    """the six errors in float64 on the fixture's own reference rows"""
    d = np.float64
    pairs = (("base_pos", "ref_root_pos"), None, ("base_lin_vel", "ref_root_vel"), ("base_ang_vel", "ref_root_ang_vel"), ("dof_pos", "ref_dof_pos"),
             ("dof_vel", "ref_dof_vel"))
    err = np.zeros(g["s_err"][s].shape)
    for k, p in enumerate(pairs):
        if p:
            err[:, k] = np.linalg.norm(g[f"s_{p[0]}"][s].astype(d) - g[f"s_{p[1]}"][s].astype(d), axis=1)
    dot = np.abs((g["s_base_quat"][s].astype(d) * g["s_ref_root_rot"][s].astype(d)).sum(axis=1))
    err[:, 1] = 2.0 * np.arccos(np.minimum(dot, 1.0))
    return err


def test_mirror_terms_of_a_perfect_tracker_and_of_a_skipped_term():
    g = golden()
    lib = golden_library(g, "world")
    t = tm.Tracker(lib, 4, 0.02, dof_map=g["map_full"], weights=[1, 2, 0, 0.5, 1, 1])
    t.assign([0, 1, 2, 1], [0.1, 0.2, 0.05, 1.0])
    ref = t.step()
    t.assign([0, 1, 2, 1], [0.1, 0.2, 0.05, 1.0])
    sim = {"base_pos": ref["ref_root_pos"], "base_quat": -ref["ref_root_rot"], "base_lin_vel": ref["ref_root_vel"] + F(1),
           "base_ang_vel": ref["ref_root_ang_vel"], "dof_pos": ref["ref_dof_pos"], "dof_vel": ref["ref_dof_vel"]}
    out = t.step(sim)
    close(out["term"][:, [0, 1, 3, 4, 5]], 1.0, abs_=1e-3)          # (acos near 1 amplifies the float32 norm of the quaternion)
    close(out["term"][:, 2], np.exp(-np.sqrt(3.0) / 2.0), rel=1e-6)
    close(out["total"], out["term"][:, [0, 1, 3, 4, 5]] @ np.array([1, 2, 0.5, 1, 1.0]), rel=1e-12)


# ---- arguments that need no device ----------------------------------------------------------------------------------------------
def stub_library(ndof=21, num_clips=3):
    return types.SimpleNamespace(ndof=ndof, num_clips=num_clips, handle=None)


@pytest.mark.parametrize("kw, exc", [
    (dict(dof_map=[0, 1, 21]), ValueError), (dict(dof_map=[0, -2]), ValueError), (dict(dof_map=list(range(21)) * 4), ValueError),
    (dict(dof_map=[]), ValueError), (dict(dof_default=np.zeros(20)), ValueError), (dict(dof_map=[0, 1], dof_weight=[1.0, np.nan]), ValueError),
    (dict(clip_weights=[1.0, 2.0]), ValueError), (dict(clip_weights=[0.0, 0.0, 0.0]), ValueError), (dict(clip_weights=[1.0, -1.0, 1.0]), ValueError),
    (dict(clip_weights=[1.0, np.inf, 1.0]), ValueError), (dict(scales=[1.0] * 5), ValueError), (dict(scales=[0.5, 0.5, 0.0, 1, 1, 1]), ValueError),
    (dict(weights={"root_height": 1.0}), KeyError), (dict(weights=[1, 1, 1, 1, 1, np.nan]), ValueError), (dict(seed=-1), ValueError),
])
def test_bad_arguments_are_refused_before_anything_touches_a_device(kw, exc):
    from general_motion_retargeting_amd import MotionTracker
    with pytest.raises(exc):
        MotionTracker(stub_library(), 16, 0.02, **kw)


def test_the_tracker_needs_a_device_and_says_so():
    from general_motion_retargeting_amd import MotionTracker, _lib
    if _lib.lib().gmr_device_count() > 0:
        lib = stub_library()
        with pytest.raises(ValueError):
            MotionTracker(lib, 0, 0.02)
        return
    with pytest.raises(_lib.GmrHipError):
        MotionTracker(stub_library(), 16, 0.02)


def test_term_names_resolve_to_six_numbers():
    from general_motion_retargeting_amd import motion_tracker as mt
    sc, wt = mt._terms({"dof_vel": 0.2}, {"root_rot": 0.0})
    assert sc.tolist() == [F(x) for x in (0.5, 0.5, 2.0, 1.0, 1.0, 0.2)] and wt.tolist() == [1, 0, 1, 1, 1, 1]
    assert mt.TERMS == tm.TERMS and mt.DEFAULT_SCALES == tm.DEFAULT_SCALES
