"""The motion tracker on a real MI355X (csrc/gmr_tracker.hip through motion_tracker.py) against the sampler it shares its code with,
against the NumPy mirror (tests/tracker_mirror.py) and against the fixture generated from the reference's loader
(tests/golden/g_tracker.npz).  Every test makes one pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_mirror as mm  # noqa: E402
import tracker_mirror as tm  # noqa: E402
from test_motion_library import _bits, device_library, make_motions  # noqa: E402
from test_motion_library_host import close  # noqa: E402
from test_motion_tracker_host import golden, golden_library  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
REFS = ("ref_root_pos", "ref_root_rot", "ref_root_vel", "ref_root_ang_vel", "ref_dof_pos", "ref_dof_vel")
STATE = ("clip", "time", "length", "draws")
ROOT_ROT_BOUND = 1e-6                    # ref_root_rot against the mirror (sin / cos / acos of the device's and NumPy's float32 libraries)
TERM_BOUND = 2e-6                        # x max(1, |w|): err / term / total against the float64 formulas


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def tracker(lib, *a, **k):
    from general_motion_retargeting_amd import MotionTracker
    return MotionTracker(lib, *a, **k)


def mirror_library(lib, motions, ang_vel="world"):
    """the NumPy library of ``motions`` with the device's root_ang_vel (pinned to 1e-5 by test_motion_library; from there on the lerp
    is bit for bit)"""
    m = mm.Library(motions, ang_vel)
    m.root_ang_vel = lib.array("root_ang_vel").copy()
    return m


def assert_refs_equal(got, want, rows=slice(None)):
    for k in REFS:
        if k == "ref_root_rot":          # (sin / cos / acos of the device's and NumPy's float32 libraries)
            close(got[k][rows], want[k][rows], abs_=ROOT_ROT_BOUND)
        else:
            assert np.array_equal(_bits(got[k][rows]), _bits(want[k][rows])), k


def assert_state_equal(t, m):
    got, want = t.state(), m.state()
    for k in STATE:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert got["ignored"] == want["ignored"]


def random_sim(rng, ref, amp=0.3):
    q = ref["ref_root_rot"] + rng.normal(0, 0.5, size=ref["ref_root_rot"].shape)          # tens of degrees away: acos well conditioned
    sim = {"base_pos": ref["ref_root_pos"] + rng.normal(0, amp, ref["ref_root_pos"].shape), "base_quat": q / np.linalg.norm(q, axis=1, keepdims=True),
           "base_lin_vel": ref["ref_root_vel"] + rng.normal(0, amp, ref["ref_root_vel"].shape),
           "base_ang_vel": ref["ref_root_ang_vel"] + rng.normal(0, amp, ref["ref_root_ang_vel"].shape),
           "dof_pos": ref["ref_dof_pos"] + rng.normal(0, 0.2 * amp, ref["ref_dof_pos"].shape),
           "dof_vel": ref["ref_dof_vel"] + rng.normal(0, 0.1 * amp, ref["ref_dof_vel"].shape)}
    return {k: np.ascontiguousarray(v, dtype=F) for k, v in sim.items()}


def close_terms(out, sim, m):
    """err / term / total of the device against the float64 formulas on the device's own reference rows"""
    want = dict(zip(("err", "term", "total"), tm.tracking_terms(out, sim, m.dof_weight, m.scale, m.weight)))
    for k in ("err", "term", "total"):
        w = np.asarray(want[k], dtype=np.float64)
        assert out[k].dtype == F and out[k].shape == w.shape
        tol = TERM_BOUND * np.maximum(1.0, np.abs(w))
        bad = ~(np.abs(out[k] - w) <= tol) & ~(np.isnan(out[k]) & np.isnan(w))
        assert not bad.any(), (k, np.abs(out[k] - w)[bad].max())


# ---- 1. the references are the sampler's -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["unitree_g1", "booster_t1", "stanford_toddy"])
@pytest.mark.parametrize("loop", [True, False])
def test_references_are_the_samplers_bits(hip, robot, loop):
    from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT
    fk = KinematicsModel(ROBOT_XML_DICT[robot]).hip_handle
    rng = np.random.default_rng(41 + len(robot) + loop)
    motions = make_motions(rng, [1, 2, 65, 300] + rng.integers(2, 120, size=12).tolist(), fk.ndof, 0)
    lib = device_library(hip, motions)
    N = 777
    clip = rng.integers(0, lib.num_clips, size=N).astype(np.int32)
    time = rng.uniform(-0.5, 6.0, size=N).astype(F)
    time[:8] = [0.0, 1.0 / 30.0, 2.0 / 50.0, 1e-7, 9.999, 100.0, 5.0, 0.5]
    want = lib.sample(clip, time.astype(np.float64), loop)
    assert not want["status"].any()
    t = tracker(lib, N, 0.02, loop=loop)
    assert t.nrobot_dof == fk.ndof and t.assign(clip, time) == 0
    st = t.state()
    assert np.array_equal(st["clip"], clip) and np.array_equal(_bits(st["time"]), _bits(time))
    got = t.step()
    for k in REFS:
        assert np.array_equal(_bits(got[k]), _bits(want[k[4:]])), k
    assert not got["status"].any()
    # a map: a permutation with some dofs on their defaults
    R = min(fk.ndof + 3, 64)
    dmap = rng.permutation(np.concatenate([np.arange(fk.ndof), np.full(R - fk.ndof, -1)])[:R]).astype(np.int32)
    dmap[rng.integers(0, R, size=3)] = -1
    default = rng.uniform(-1, 1, size=R).astype(F)
    t.set_dof_map(dmap, default)
    t.assign(clip, time)
    got = t.step()
    on = dmap >= 0
    for k, off_value in (("ref_dof_pos", default), ("ref_dof_vel", np.zeros(R, F))):
        assert got[k].shape == (N, R)
        assert np.array_equal(_bits(got[k][:, on]), _bits(want[k[4:]][:, dmap[on]])), k
        assert np.array_equal(_bits(got[k][:, ~on]), _bits(np.tile(off_value[~on], (N, 1)))), k
    for k in REFS[:4]:
        assert np.array_equal(_bits(got[k]), _bits(want[k[4:]])), k
    t.close()


def test_device_reproduces_the_reference_loop(hip):
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    g = golden()
    motions = [{k: g[f"c{c}_{k}"] for k in ("root_pos", "root_rot", "dof_pos")} | {"fps": float(g[f"c{c}_fps"])} for c in range(int(g["nclip"]))]
    lib = MotionLibrary.from_motions(motions, ang_vel="reference")
    mlib = golden_library(g)
    mlib.root_ang_vel = lib.array("root_ang_vel").copy()
    mirror = tm.Tracker(mlib, 6, float(g["dt"]), dof_map=g["map_stage1"], dof_default=g["dof_default"])
    t = tracker(lib, 6, float(g["dt"]), dof_map=g["map_stage1"], dof_default=g["dof_default"], scales=g["scales"])
    for s in range(g["s_time"].shape[0]):
        for s_, e, c, tt in g["script"]:
            if int(s_) == s:
                for x in (t, mirror):
                    x.assign([int(c)], [tt], [int(e)])
        if s == int(g["stage2_from"]):
            for x in (t, mirror):
                x.set_dof_map(g["map_full"], g["dof_default"])
        assert np.array_equal(_bits(t.state()["time"]), _bits(g["s_time"][s])), s
        sim = {k: g[f"s_{k}"][s] for k in tm.SIM}
        out, want = t.step(sim), mirror.step(sim)
        for k in ("ref_root_pos", "ref_root_vel", "ref_dof_pos", "ref_dof_vel"):
            close(out[k], g[f"s_{k}"][s], rel=1e-6, abs_=1e-7)
        close(out["ref_root_rot"], g["s_ref_root_rot"][s], abs_=1e-6)
        close(out["ref_root_ang_vel"], g["s_ref_root_ang_vel"][s], rel=1e-6, abs_=1e-5)
        close(out["err"], g["s_err"][s], rel=2e-5, abs_=2e-5)
        close(out["term"], g["s_term"][s], rel=1e-4, abs_=2e-5)
        assert_refs_equal(out, want)
    assert np.array_equal(_bits(t.state()["time"]), _bits(g["final_time"]))


# ---- 2. clocks -------------------------------------------------------------------------------------------------------------------
def test_clocks_and_redraws_without_loop_are_the_mirrors(hip):
    rng = np.random.default_rng(5)
    lens = [3, 7, 400, 25, 1, 60, 900, 12]
    motions = make_motions(rng, lens, 12, 0, fps_choices=(30.0, 50.0))
    lib = device_library(hip, motions)
    N, dt, seed = 300, 0.02, 0xDEADBEEF12345678
    t, m = tracker(lib, N, dt, loop=False, seed=seed), tm.Tracker(mirror_library(lib, motions), N, dt, loop=False, seed=seed)
    assert_state_equal(t, m)
    assert t.reset() == 0 and m.reset() == 0
    finished_total = 0
    for s in range(200):
        if s == 60:
            ids = rng.choice(N, size=90, replace=False)
            assert t.reset(ids, resample=True, time_offset_range=(0.0, 0.3)) == 0
            m.reset(ids, True, (0.0, 0.3))
        if s == 130:
            ids = np.concatenate([rng.choice(N, size=40, replace=False), [N, -1, N + 5]])
            assert t.reset(ids, resample=False, time_offset_range=(0.1, 0.1)) == 3
            assert m.reset(ids, False, (0.1, 0.1)) == 3
        got, want = t.step(), m.step()
        assert np.array_equal(got["finished"], want["finished"]) and np.array_equal(got["status"], want["status"]), s
        assert_refs_equal(got, want)
        assert_state_equal(t, m)
        finished_total += int(got["finished"].sum())
    assert finished_total > 100 and t.state()["draws"].max() >= 4


def test_an_environment_draws_the_same_sequence_whatever_surrounds_it(hip):
    rng = np.random.default_rng(6)
    motions = make_motions(rng, [5, 9, 14, 3, 21, 8, 30], 6, 0, fps_choices=(30.0,))
    lib = device_library(hip, motions)
    seqs = []
    for N in (64, 5000):
        t = tracker(lib, N, 0.05, loop=False, seed=99)
        if N == 5000:
            t.reset([4999, 8, 9])
        t.reset([7], time_offset_range=(0.0, 0.2))
        seq = []
        for _ in range(60):
            out = t.step()
            s = t.state()
            seq.append((int(s["clip"][7]), float(s["time"][7]), int(out["finished"][7]), out["ref_root_pos"][7].tobytes()))
        seqs.append(seq)
        if N == 64:      # the first draw of environment 0 under seed 0 is the first known-answer vector
            t0 = tracker(lib, 3, 0.05, seed=0)
            t0.reset([0], time_offset_range=(0.0, 1.0))
            s = t0.state()
            assert s["clip"][0] == (0x6627E8D5 * 7) >> 32 and s["time"][0] == F(0xE169C58D >> 8) * F(2.0 ** -24) and s["draws"].tolist() == [1, 0, 0]
    assert seqs[0] == seqs[1] and sum(x[2] for x in seqs[0]) >= 2


def test_clip_weights_shape_the_draws(hip):
    rng = np.random.default_rng(8)
    motions = make_motions(rng, [4] * 6, 3, 0, fps_choices=(30.0,))
    lib = device_library(hip, motions)
    w = np.array([0.0, 3.0, 1.0, 0.0, 4.0, 0.0])
    N = 20000
    t, m = tracker(lib, N, 0.02, clip_weights=w, seed=3), tm.Tracker(mirror_library(lib, motions), N, 0.02, clip_weights=w, seed=3)
    t.reset()
    m.reset()
    assert_state_equal(t, m)
    count = np.bincount(t.state()["clip"], minlength=6)
    p = w / w.sum()
    assert not count[p == 0].any()
    assert (np.abs(count - N * p) <= 4 * np.sqrt(N * p * (1 - p))).all(), count
    from general_motion_retargeting_amd import _lib
    import ctypes as C
    h, bad = C.c_void_p(), np.array([1.0, np.nan, 1, 1, 1, 1])
    assert _lib.lib().gmr_motion_tracker_create(lib.handle, 4, 0.02, 0, 3, None, None, None, _lib._ptr(bad), 0, C.byref(h)) != 0 and not h.value
    dmap = np.array([0, 3, 1], dtype=np.int32)
    assert _lib.lib().gmr_motion_tracker_create(lib.handle, 4, 0.02, 0, 3, _lib._ptr(dmap), None, None, None, 0, C.byref(h)) != 0 and not h.value
    assert b"dof_map[1] = 3" in _lib.lib().gmr_last_error()


# ---- 3. the terms ----------------------------------------------------------------------------------------------------------------
def test_terms_against_the_float64_mirror(hip):
    rng = np.random.default_rng(9)
    motions = make_motions(rng, [40, 90, 25, 300], 21, 0)
    lib = device_library(hip, motions)
    N = 1000
    dmap = np.array([-1, -1] + list(range(21)), dtype=np.int32)
    default, dw = rng.uniform(-0.3, 0.3, 23).astype(F), np.where(np.arange(23) >= 11, 0.0, 1.0).astype(F)
    kw = dict(dof_map=dmap, dof_default=default, dof_weight=dw, scales=[0.4, 0.6, 1.5, 1.2, 0.9, 0.2], weights=[1.0, 0.5, 0.25, 2.0, 3.0, 0.1])
    t, m = tracker(lib, N, 0.02, **kw), tm.Tracker(mirror_library(lib, motions), N, 0.02, **kw)
    clip, time = rng.integers(0, 4, size=N), rng.uniform(0, 4, size=N).astype(F)
    for x in (t, m):
        x.assign(clip, time)
    ref = t.step()
    for x in (t, m):
        x.assign(clip, time)
    sim = random_sim(rng, ref)
    out, want = t.step(sim), m.step(sim)
    close_terms(out, sim, m)
    assert (out["err"] > 1e-3).all()
    close(out["total"], want["total"], rel=1e-5, abs_=1e-5)             # (the mirror's own rows: root_rot is NumPy's slerp there)
    # a zero weight: that term leaves the total, the others stay; an absent array: its err and term are 0
    total_without = want["total"] - 2.0 * want["term"][:, 3]
    for x in (t, m):
        x.assign(clip, time)
    t.set_terms(weights=[1.0, 0.5, 0.25, 0.0, 3.0, 0.1])
    out0 = t.step(dict(sim, base_ang_vel=np.full((N, 3), np.nan, F)))            # a skipped term's input is not looked at
    close(out0["total"], total_without, rel=2e-6, abs_=2e-6)
    assert np.isnan(out0["err"][:, 3]).all() and np.array_equal(_bits(out0["term"][:, [0, 1, 2, 4, 5]]), _bits(out["term"][:, [0, 1, 2, 4, 5]]))
    t.assign(clip, time)
    out1 = t.step({k: v for k, v in sim.items() if k != "base_ang_vel"})
    assert not out1["err"][:, 3].any() and not out1["term"][:, 3].any() and np.array_equal(_bits(out1["total"]), _bits(out0["total"]))
    # a perfect tracker: every term 1 (the angle as far as float32 lets 2 acos(|<q, q>|) be zero: |q|^2 = 1 - 6e-8 is 1e-3 rad)
    t.assign(clip, time)
    perfect = {"base_pos": ref["ref_root_pos"], "base_quat": -ref["ref_root_rot"], "base_lin_vel": ref["ref_root_vel"],
               "base_ang_vel": ref["ref_root_ang_vel"], "dof_pos": ref["ref_dof_pos"], "dof_vel": ref["ref_dof_vel"]}
    out2 = t.step(perfect)
    close(out2["term"][:, [0, 2, 3, 4, 5]], 1.0, abs_=1e-6)
    close(out2["term"][:, 1], 1.0, abs_=3e-3)
    with pytest.raises(hip.GmrHipError, match="simulator"):
        t.step_dev(None, err=hip.DeviceBuffer(N * 24))


# ---- 4. bad input ----------------------------------------------------------------------------------------------------------------
def test_bad_assignments_are_neutralised_and_nothing_leaves_the_rows(hip):
    rng = np.random.default_rng(10)
    motions = make_motions(rng, [30, 50, 20], 29, 0)
    lib = device_library(hip, motions)
    N, R, G = 37, 29, 64                                   # G guard floats behind every output
    clip = rng.integers(0, 3, size=N).astype(np.int32)
    time = rng.uniform(0, 1, size=N).astype(F)
    bad = {3: (7, 0.1), 4: (-1, 0.2), 11: (1, np.nan), 12: (2, np.inf), 36: (3, 0.0)}
    for e, (c, tt) in bad.items():
        clip[e], time[e] = c, tt
    t = tracker(lib, N, 0.02)
    m = tm.Tracker(mirror_library(lib, motions), N, 0.02)
    for x in (t, m):
        x.assign(clip, time)
    counts, _ = t._counts()
    sentinel = F(-77.25)
    bufs = {k: hip.DeviceBuffer.from_host(np.full(N * w + G, sentinel, dtype=F)) for k, w in counts.items()}
    ref = m.step()
    m.assign(clip, time)
    sim = random_sim(rng, {k: np.nan_to_num(ref[k]) for k in REFS})
    want = m.step(sim)
    d_sim = {k: hip.DeviceBuffer.from_host(v) for k, v in sim.items()}
    t.step_dev(d_sim, **bufs)
    hip.check(hip.lib().gmr_stream_sync(None))
    isbad = np.zeros(N, bool)
    isbad[list(bad)] = True
    got = {}
    for k, w in counts.items():
        raw = bufs[k].to_host(N * w + G, F)
        assert (raw[N * w:] == sentinel).all(), k                               # the guard rows
        if k in ("status", "finished"):
            a = raw[:N * w].view(np.int32)
            assert np.array_equal(a, isbad.astype(np.int32) if k == "status" else np.zeros(N, np.int32)), k
            continue
        a = raw[:N * w].reshape(N, w)
        assert np.isnan(a[isbad]).all() and not np.isnan(a[~isbad]).any(), k
        got[k] = a
    assert_refs_equal(got, want, ~isbad)
    got["total"] = got["total"].reshape(N)
    close_terms(got, sim, m)
    assert np.isnan(got["total"][isbad]).all() and not np.isnan(got["total"][~isbad]).any()
    st = t.state()
    assert np.array_equal(_bits(st["time"][isbad]), _bits(time[isbad])) and np.array_equal(st["clip"], clip)       # the clock has not moved
    assert np.array_equal(_bits(st["time"][~isbad]), _bits((time[~isbad] + F(0.02)).astype(F)))
    assert_state_equal(t, m)
    # ids outside [0, N): ignored, counted, nothing else touched
    before = t.state()
    assert t.reset([-5, N, 2 ** 31 - 1]) == 3 and t.assign([0, 1], [0.5, 0.5], [N + 1, 5]) == 1
    after = t.state()
    assert after["ignored"] == before["ignored"] + 4 and after["clip"][5] == 1 and after["time"][5] == F(0.5)
    keep = np.arange(N) != 5
    for k in STATE:
        assert np.array_equal(_bits(after[k][keep]), _bits(before[k][keep])), k


# ---- 5. streams ------------------------------------------------------------------------------------------------------------------
def test_step_dev_on_a_stream_of_its_own_equals_step(hip):
    rng = np.random.default_rng(12)
    motions = make_motions(rng, [40, 90, 25], 23, 0)
    lib = device_library(hip, motions)
    N = 513
    ta, tb = tracker(lib, N, 0.02, loop=False, seed=5), tracker(lib, N, 0.02, loop=False, seed=5)
    st = hip.Stream()
    ta.reset(time_offset_range=(0.0, 0.4))
    tb.reset_dev(stream=st, time_offset_range=(0.0, 0.4))
    counts, _ = ta._counts()
    bufs = {k: hip.DeviceBuffer(N * w * 4) for k, w in counts.items()}
    sim = random_sim(rng, {k: np.zeros((N, counts[k]), F) + (k == "ref_root_rot") for k in REFS})
    d_sim = {k: hip.DeviceBuffer.from_host(v) for k, v in sim.items()}
    for _ in range(30):
        want = ta.step(sim)
        tb.step_dev(d_sim, stream=st, **bufs)
    st.sync()
    for k, w in counts.items():
        dtype = np.int32 if k in ("status", "finished") else F
        got = bufs[k].to_host(want[k].shape, dtype)
        assert np.array_equal(_bits(got), _bits(want[k])), k
    a, b = ta.state(), tb.state()
    for k in STATE:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["draws"].max() >= 2
