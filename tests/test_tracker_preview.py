"""The tracker's preview on a real MI355X (csrc/gmr_tracker_preview.hip through motion_tracker.py): the raw frame
against the sampler it shares its code with, bit for bit; the anchored frames against the float64 formulas of tests/preview_mirror.py
applied to the device's own raw rows; the valid mask, bad assignments, the launch shape, streams and the travelling configuration.
Every test makes one pass."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_mirror as mm  # noqa: E402
import preview_mirror as pm  # noqa: E402
from test_motion_library import _bits, device_library, make_motions  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
REFS = ("ref_root_pos", "ref_root_rot", "ref_root_vel", "ref_root_ang_vel", "ref_dof_pos", "ref_dof_vel")
STATE = ("clip", "time", "length", "draws")
SAMPLER = ("root_pos", "root_quat", "root_vel", "root_ang_vel", "dof_pos", "dof_vel")
ANCHORED = ("root_pos", "root_quat", "root_rot6", "root_vel", "root_ang_vel", "body_pos")
BOUND = {"root_pos": 2e-6, "root_quat": 2e-6, "root_rot6": 2e-6, "root_vel": 2e-6, "root_ang_vel": 2e-6, "body_pos": 4e-6}


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def tracker(lib, *a, **k):
    from general_motion_retargeting_amd import MotionTracker
    return MotionTracker(lib, *a, **k)


def mirror_library(motions):
    return mm.Library(motions, "world")


def within(got, want, bound, what):
    """|got - want| <= bound x max(1, |want|) everywhere, NaN exactly where want is NaN; the largest figure is printed first"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    rel = np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))
    print(f"{what}: max deviation {rel.max() if rel.size else 0.0:.3e} x max(1, |x|), bound {bound:.1e}")
    assert (rel <= bound).all(), (what, rel.max())


# ---- 1. the raw frame is the sampler's -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["unitree_g1", "booster_t1", "stanford_toddy"])
@pytest.mark.parametrize("loop", [True, False])
def test_raw_blocks_are_the_samplers_bits(hip, robot, loop):
    from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT
    ndof = KinematicsModel(ROBOT_XML_DICT[robot]).hip_handle.ndof
    rng = np.random.default_rng(141 + len(robot) + loop)
    nbody = 11
    motions = make_motions(rng, [1, 2, 65, 300] + rng.integers(2, 120, size=12).tolist(), ndof, nbody)
    lib = device_library(hip, motions)
    N = 777
    clip = rng.integers(0, lib.num_clips, size=N).astype(np.int32)
    time = rng.uniform(-0.5, 6.0, size=N).astype(F)
    time[:8] = [0.0, 1.0 / 30.0, 2.0 / 50.0, 1e-7, 9.999, 100.0, 5.0, 0.5]
    offsets = np.array([0.02, 0.0, -0.37, 0.04, 20.0], dtype=F)          # 0, a negative one, one past every clip's end (300 frames at >= 29.97)
    bodies = [10, 0, 4, 7]
    blocks = SAMPLER + ("body_pos",)
    K = len(offsets)
    tq = pm.query_times(time, offsets)
    want = lib.sample(np.repeat(clip, K), tq.reshape(-1), loop, local_body_pos=True)
    assert not want["status"].any()
    key = {"root_quat": "root_rot"}
    t = tracker(lib, N, 0.02, loop=loop)
    assert t.assign(clip, time) == 0
    lay = t.set_preview(offsets, blocks, "raw", bodies)
    assert lay["row_width"] == 3 + 4 + 3 + 3 + 2 * ndof + 12 and lay == pm.layout(blocks, ndof, 4) == t.preview_layout
    got = t.preview()
    assert got["obs"].shape == (N, K, lay["row_width"]) and got["obs"].dtype == F and not got["status"].any()
    for b in SAMPLER:
        assert np.array_equal(_bits(got["obs"][:, :, lay[b]]), _bits(want[key.get(b, b)].reshape(N, K, -1))), b
    assert np.array_equal(_bits(got["obs"][:, :, lay["body_pos"]]), _bits(want["local_body_pos"][:, bodies].reshape(N, K, 12)))
    # a map: a permutation with some dofs on their defaults; R, and with it D, changes under the configured preview
    R = min(ndof + 3, 64)
    dmap = rng.permutation(np.concatenate([np.arange(ndof), np.full(R - ndof, -1)])[:R]).astype(np.int32)
    dmap[rng.integers(0, R, size=3)] = -1
    default = rng.uniform(-1, 1, size=R).astype(F)
    t.set_dof_map(dmap, default)
    lay = t.preview_layout
    assert lay["row_width"] == 13 + 2 * R + 12 and lay == pm.layout(blocks, R, 4)
    got = t.preview()
    assert got["obs"].shape == (N, K, lay["row_width"])
    on = dmap >= 0
    for b, off_value in (("dof_pos", default), ("dof_vel", np.zeros(R, F))):
        a = got["obs"][:, :, lay[b]]
        assert np.array_equal(_bits(a[:, :, on]), _bits(want[b].reshape(N, K, ndof)[:, :, dmap[on]])), b
        assert np.array_equal(_bits(a[:, :, ~on]), _bits(np.broadcast_to(off_value[~on], (N, K, int((~on).sum()))))), b
    for b in SAMPLER[:4]:
        assert np.array_equal(_bits(got["obs"][:, :, lay[b]]), _bits(want[key.get(b, b)].reshape(N, K, -1))), b
    assert np.array_equal(_bits(got["obs"][:, :, lay["body_pos"]]), _bits(want["local_body_pos"][:, bodies].reshape(N, K, 12)))
    t.close()


# ---- 2. a preview at offset 0 is what the next step emits, and moves nothing -----------------------------------------------------
def test_offset_zero_is_the_next_steps_reference_and_the_state_stays(hip):
    rng = np.random.default_rng(202)
    motions = make_motions(rng, [40, 3, 90, 25, 1], 23, 0)
    lib = device_library(hip, motions)
    N = 1000
    dmap = np.array([-1] + list(range(22, -1, -1)), dtype=np.int32)
    t = tracker(lib, N, 0.02, loop=False, dof_map=dmap, dof_default=rng.uniform(-1, 1, 24).astype(F), seed=17)
    t.reset(time_offset_range=(0.0, 1.5))
    for _ in range(3):
        t.step()
    lay = t.set_preview([0.0, 0.02], SAMPLER, "raw")
    before = t.state()
    pv = t.preview()
    after = t.state()
    for k in STATE:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
    assert before["ignored"] == after["ignored"] and before["draws"].max() >= 1
    out = t.step()
    for ref, b in zip(REFS, SAMPLER):
        assert np.array_equal(_bits(out[ref]), _bits(pv["obs"][:, 0, lay[b]])), b
    assert not out["status"].any() and not pv["status"].any()


# ---- 3. the anchored frames --------------------------------------------------------------------------------------------------------
def walking_motions(rng, lens, ndof, nbody):
    """``make_motions`` with a root that moves like a robot's: the frames of ``make_motions`` are independent draws, so its root
    velocities reach 300 m/s and 350 rad/s at 120 fps.  A rotation about z mixes x and y, so the float32 error of a rotated velocity is
    about 3e-7 |v| in BOTH components, also in the one that comes out small: against the bound 2e-6 x max(1, |x|) per component the
    float32 formulas themselves (evaluated in NumPy, on the CPU) then deviate by up to 8.5e-6.  Here the root follows a smooth path of
    at most 1.5 m/s per axis and turns by a random walk of 1 rad/s per axis, flips of the quaternion's sign kept: the float32 floor of
    the five root blocks is then 1.4e-7 to 6.0e-7 and that of body_pos 8.1e-7 x max(1, |x|) (six seeds, 54 000 rows each), a factor 3 to 5 under
    the bounds."""
    out = make_motions(rng, lens, ndof, nbody)
    for m in out:
        n, fps = len(m["root_pos"]), m["fps"]
        tt = np.arange(n)[:, None] / fps
        amp, om = rng.uniform(0.1, 0.5, 3), rng.uniform(0.5, 3.0, 3)
        m["root_pos"] = np.array([0.3, -0.2, 0.8]) + amp * np.sin(om * tt + rng.uniform(0, 6.28, 3))
        q = np.empty((n, 4))
        q[0] = rng.normal(size=4)
        q[0] /= np.linalg.norm(q[0])
        for i in range(1, n):
            v = rng.normal(0, 1.0, 3) / fps
            a = np.linalg.norm(v)
            dq = np.concatenate([v / a * np.sin(a / 2), [np.cos(a / 2)]])
            q[i] = mm.qmul_xyzw(q[i - 1][None], dq[None])[0]
            q[i] /= np.linalg.norm(q[i])
        q[np.arange(n) % 5 == 0] *= -1.0
        m["root_rot"] = q
    return out


@pytest.mark.parametrize("frame", ["reference", "sim"])
def test_anchored_frames_against_the_float64_transform_of_the_devices_raw_rows(hip, frame):
    rng = np.random.default_rng(303 + len(frame))
    nbody = 9
    motions = walking_motions(rng, [40, 90, 25, 300, 2, 1], 21, nbody)
    lib = device_library(hip, motions)
    N = 1500
    clip = rng.integers(0, 6, size=N).astype(np.int32)
    time = rng.uniform(-0.2, 5.0, size=N).astype(F)
    bad = {5: (6, 0.1), 77: (1, np.nan), 1499: (-1, 0.0)}
    for e, (c, tt) in bad.items():
        clip[e], time[e] = c, tt
    isbad = np.zeros(N, bool)
    isbad[list(bad)] = True
    offsets = np.array([0.04, 0.02, 0.0, 0.5, -0.1, 3.0], dtype=F)          # offset 0 is row k = 2
    bodies = [8, 1, 0, 5, 3, 2]
    dmap = np.array([3, -1] + list(range(21)), dtype=np.int32)
    t = tracker(lib, N, 0.02, dof_map=dmap, dof_default=rng.uniform(-1, 1, 23).astype(F))
    t.assign(clip, time)
    lay = t.set_preview(offsets, pm.BLOCKS, "raw", bodies)
    raw = t.preview()["obs"]
    assert np.isnan(raw[isbad]).all() and not np.isnan(raw[~isbad]).any()
    sim = None
    if frame == "sim":
        q = rng.normal(size=(N, 4))
        sim = {"base_pos": (rng.normal(0, 0.5, (N, 3)) + np.array([0.3, -0.2, 0.8])).astype(F), "base_quat": (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)}
        anchor = sim["base_pos"], sim["base_quat"]
    else:
        anchor = raw[:, 2, lay["root_pos"]], raw[:, 2, lay["root_quat"]]      # the device's own row at offset 0
    assert t.set_preview(offsets, pm.BLOCKS, frame, bodies) == lay
    got = t.preview(sim)
    assert np.array_equal(got["status"], isbad.astype(np.int32))
    rows = {b: raw[:, :, lay[b]] for b in ("root_pos", "root_quat", "root_vel", "root_ang_vel")}
    rows["body_pos"] = raw[:, :, lay["body_pos"]].reshape(N, len(offsets), len(bodies), 3)
    with np.errstate(invalid="ignore"):
        want = pm.transform(rows, *anchor)
    for b in ANCHORED:
        within(got["obs"][:, :, lay[b]], want[b].reshape(N, len(offsets), -1), BOUND[b], f"{frame} {b}")
    for b in ("dof_pos", "dof_vel"):
        assert np.array_equal(_bits(got["obs"][:, :, lay[b]]), _bits(raw[:, :, lay[b]])), b
    assert np.isnan(got["obs"][isbad]).all() and not np.isnan(got["obs"][~isbad]).any()
    if frame == "reference":          # the anchor sees itself: no displacement at offset 0
        assert np.abs(got["obs"][~isbad][:, 2, lay["root_pos"]]).max() == 0.0


# ---- 4. valid, and rot6 in the raw frame -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [True, False])
def test_valid_is_the_mirrors_and_raw_rot6_is_the_matrix_of_the_raw_quaternion(hip, loop):
    rng = np.random.default_rng(404 + loop)
    motions = make_motions(rng, [9, 1, 64, 120, 2], 7, 0, fps_choices=(64.0, 30.0, 50.0))
    lib, mlib = device_library(hip, motions), mirror_library(motions)
    N = 2000
    clip = rng.integers(0, 5, size=N).astype(np.int32)
    time = rng.uniform(-0.3, 3.0, size=N).astype(F)
    # the edges: the last frame of every clip exactly as float32 can say it, one ulp to either side, zero
    for i, c in enumerate(range(5)):
        last = F((mlib.seg[c + 1] - mlib.seg[c] - 1) / mlib.fps[c])
        for j, tt in enumerate((last, np.nextafter(last, F(np.inf)), np.nextafter(last, F(-np.inf)), F(0.0))):
            clip[4 * i + j], time[4 * i + j] = c, tt
    clip[100], time[101] = 5, np.inf
    offsets = np.array([0.0, 1.0 / 64.0, -1.0 / 64.0, 0.5, -2.0, 40.0], dtype=F)
    t = tracker(lib, N, 0.02, loop=loop)
    t.assign(clip, time)
    lay = t.set_preview(offsets, ("root_quat", "root_rot6"), "raw")
    got = t.preview()
    want = pm.valid_mask(mlib, clip, time, offsets)
    assert got["valid"].dtype == np.int32 and np.array_equal(got["valid"], want)
    assert 0.1 < want.mean() < 0.9 and not want[[100, 101]].any() and got["status"].sum() == 2
    with np.errstate(invalid="ignore"):
        within(got["obs"][:, :, lay["root_rot6"]], pm.rot6(got["obs"][:, :, lay["root_quat"]].astype(np.float64)), BOUND["root_rot6"], "raw root_rot6")


# ---- 5. bad input ------------------------------------------------------------------------------------------------------------------
def test_bad_assignments_are_neutralised_and_nothing_leaves_the_rows(hip):
    rng = np.random.default_rng(505)
    motions = make_motions(rng, [30, 0, 50, 20], 29, 5)          # clip 1 is empty
    lib = device_library(hip, motions)
    N, K, G = 37, 3, 64                                     # G guard words behind every output
    clip = rng.choice([0, 2, 3], size=N).astype(np.int32)
    time = rng.uniform(0, 1, size=N).astype(F)
    bad = {3: (4, 0.1), 4: (-1, 0.2), 9: (1, 0.3), 11: (2, np.nan), 12: (3, np.inf), 36: (0, -np.inf)}
    for e, (c, tt) in bad.items():
        clip[e], time[e] = c, tt
    isbad = np.zeros(N, bool)
    isbad[list(bad)] = True
    t = tracker(lib, N, 0.02)
    t.assign(clip, time)
    offsets = np.array([0.0, 0.1, -0.05], dtype=F)
    q = rng.normal(size=(N, 4))
    sim = {"base_pos": rng.normal(size=(N, 3)).astype(F), "base_quat": (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)}
    d_sim = {k: hip.DeviceBuffer.from_host(v) for k, v in sim.items()}
    good = None
    for frame in ("raw", "reference", "sim"):
        lay = t.set_preview(offsets, pm.BLOCKS, frame, [4, 0])
        D = lay["row_width"]
        sentinel = F(-77.25)
        bufs = {"obs": hip.DeviceBuffer.from_host(np.full(N * K * D + G, sentinel, F)), "valid": hip.DeviceBuffer.from_host(np.full(N * K + G, sentinel, F)),
                "status": hip.DeviceBuffer.from_host(np.full(N + G, sentinel, F))}
        t.preview_dev(d_sim if frame == "sim" else None, **bufs)
        hip.check(hip.lib().gmr_stream_sync(None))
        obs = bufs["obs"].to_host(N * K * D + G, F)
        valid = bufs["valid"].to_host(N * K + G, F)
        status = bufs["status"].to_host(N + G, F)
        for name, a, n in (("obs", obs, N * K * D), ("valid", valid, N * K), ("status", status, N)):
            assert (a[n:] == sentinel).all(), (frame, name)                     # the guard words
        obs, valid, status = obs[:N * K * D].reshape(N, K, D), valid[:N * K].view(np.int32).reshape(N, K), status[:N].view(np.int32)
        assert np.isnan(obs[isbad]).all() and not np.isnan(obs[~isbad]).any(), frame
        assert np.array_equal(status, isbad.astype(np.int32)) and not valid[isbad].any() and valid[~isbad].any()
        # the neighbours of a bad environment are what they are without it
        if frame == "raw":
            ok_clip, ok_time = np.where(isbad, 0, clip), np.where(isbad, F(0.25), time).astype(F)
            t.assign(ok_clip, ok_time)
            good = t.preview()
            t.assign(clip, time)
            assert np.array_equal(_bits(good["obs"][~isbad]), _bits(obs[~isbad])) and np.array_equal(good["valid"][~isbad], valid[~isbad])
    assert good is not None


# ---- 6. the launch shape -----------------------------------------------------------------------------------------------------------
def test_an_environment_previews_the_same_bits_whatever_surrounds_it(hip):
    rng = np.random.default_rng(606)
    motions = make_motions(rng, [5, 90, 14, 300, 21], 12, 6)
    lib = device_library(hip, motions)
    sixteen = np.linspace(-0.1, 0.5, 16).astype(F)
    cases = [(sixteen, pm.BLOCKS, "reference", [5, 2, 3]),                  # K = 16, D = 3 + 4 + 6 + 3 + 3 + 24 + 9 = 52
             (sixteen[3:4], ("root_rot6",), "raw", None),                   # K = 1, a single block
             (sixteen[:5], ("root_pos", "dof_pos", "body_pos"), "sim", [1]),     # D = 3 + 12 + 3 = 18, no multiple of 4
             (sixteen[:3], ("dof_vel", "root_quat", "root_pos"), "raw", None)]   # D = 19
    rows = []
    for N in (64, 5000):
        t = tracker(lib, N, 0.05, seed=99)
        clip, time = rng.integers(0, 5, size=N).astype(np.int32), rng.uniform(0, 3, size=N).astype(F)
        clip[7], time[7] = 3, F(1.2345)
        t.assign(clip, time)
        sim = {"base_pos": np.tile(F([0.5, -1.0, 0.7]), (N, 1)), "base_quat": np.tile(F([0.1, -0.2, 0.6, 0.7]), (N, 1))}
        got = []
        for offsets, blocks, frame, bodies in cases:
            lay = t.set_preview(offsets, blocks, frame, bodies)
            out = t.preview(sim if frame == "sim" else None)
            assert out["obs"].shape == (N, len(offsets), lay["row_width"]) and not np.isnan(out["obs"]).any()
            got.append((out["obs"][7].tobytes(), out["valid"][7].tobytes(), int(out["status"][7])))
        rows.append(got)
        assert [t.set_preview(*c)["row_width"] for c in cases] == [52, 6, 18, 19]
    assert rows[0] == rows[1]


# ---- 7. streams --------------------------------------------------------------------------------------------------------------------
def test_preview_dev_on_a_stream_of_its_own_equals_preview(hip):
    rng = np.random.default_rng(707)
    motions = make_motions(rng, [40, 90, 25], 23, 4)
    lib = device_library(hip, motions)
    N = 513
    offsets = np.array([0.0, 0.02, 0.04, 0.3], dtype=F)
    ta, tb = tracker(lib, N, 0.02, loop=False, seed=5), tracker(lib, N, 0.02, loop=False, seed=5)
    st = hip.Stream()
    ta.reset(time_offset_range=(0.0, 0.4))
    tb.reset_dev(stream=st, time_offset_range=(0.0, 0.4))
    for x in (ta, tb):
        lay = x.set_preview(offsets, pm.BLOCKS, "reference", [3, 1])
    K, D = len(offsets), lay["row_width"]
    obs, valid, status = hip.DeviceBuffer(N * K * D * 4), hip.DeviceBuffer(N * K * 4), hip.DeviceBuffer(N * 4)
    obs_only, valid_only = hip.DeviceBuffer(N * K * D * 4), hip.DeviceBuffer(N * K * 4)
    for _ in range(20):
        ta.step()
        tb.step_dev(stream=st)
    tb.preview_dev(stream=st, obs=obs, valid=valid, status=status)          # ordered after the steps: the same stream
    tb.preview_dev(stream=st, obs=obs_only)
    tb.preview_dev(stream=st, valid=valid_only)
    st.sync()
    want = ta.preview()
    assert np.array_equal(_bits(obs.to_host((N, K, D), F)), _bits(want["obs"])) and np.array_equal(_bits(obs_only.to_host((N, K, D), F)), _bits(want["obs"]))
    assert np.array_equal(valid.to_host((N, K), np.int32), want["valid"]) and np.array_equal(valid_only.to_host((N, K), np.int32), want["valid"])
    assert np.array_equal(status.to_host(N, np.int32), want["status"]) and want["valid"].any() and not want["valid"].all()
    a, b = ta.state(), tb.state()
    for k in STATE:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    with pytest.raises(ValueError, match="needed"):
        tb.preview_dev(stream=st, obs=hip.DeviceBuffer(N * K * D * 4 - 4))


# ---- 8. the configuration travels with the launch ------------------------------------------------------------------------------------
def test_each_launch_uses_the_configuration_it_was_launched_with(hip):
    rng = np.random.default_rng(808)
    motions = make_motions(rng, [40, 90, 25], 10, 3)
    lib = device_library(hip, motions)
    N = 4096
    t = tracker(lib, N, 0.02)
    t.reset(time_offset_range=(0.0, 2.0))
    first = (np.array([0.0, 0.1], dtype=F), ("root_pos", "dof_pos"), "raw", None)
    second = (np.array([0.3, -0.2, 0.0], dtype=F), ("root_quat", "root_vel", "body_pos"), "reference", [2, 0])
    st = hip.Stream()
    bufs = []
    for cfg in (first, second, first):
        lay = t.set_preview(*cfg)
        b = hip.DeviceBuffer(N * len(cfg[0]) * lay["row_width"] * 4)
        t.preview_dev(stream=st, obs=b)          # enqueued; the configuration is replaced before it has to have run
        bufs.append((b, (N, len(cfg[0]), lay["row_width"])))
    st.sync()
    got = [b.to_host(shape, F) for b, shape in bufs]
    for cfg, g in zip((first, second, first), got):
        t.set_preview(*cfg)
        assert np.array_equal(_bits(t.preview()["obs"]), _bits(g))
    assert not np.array_equal(got[0][:, 0, :3], got[1][:, 0, :3])
    # K = 0 detaches: the Python layer and the library both refuse a preview
    assert t.set_preview([]) is None and t.preview_layout is None
    with pytest.raises(ValueError, match="set_preview"):
        t.preview()
    assert hip.lib().gmr_motion_tracker_preview_dev(t.handle, None, bufs[0][0].ptr, None, None, None) != 0
    assert b"no preview configured" in hip.lib().gmr_last_error()
    # the library's own refusals, with their messages
    D = C.c_int(-1)
    off = np.array([0.0, np.inf], dtype=F)
    sel = np.array([0, 3], dtype=np.int32)
    L = hip.lib()
    for args, why in (((17, hip._ptr(np.zeros(17, F)), 1, 0, None, 0), b"K = 17"), ((2, hip._ptr(off), 1, 0, None, 0), b"not finite"),
                      ((1, hip._ptr(off), 256, 0, None, 0), b"unknown preview block"), ((1, hip._ptr(off), 0, 0, None, 0), b"at least one block"),
                      ((1, hip._ptr(off), 1, 3, None, 0), b"unknown preview frame"), ((1, hip._ptr(off), 128, 0, None, 0), b"selection"),
                      ((1, hip._ptr(off), 128, 0, hip._ptr(sel), 2), b"outside"), ((1, hip._ptr(off), 128, 0, hip._ptr(sel), 33), b"selection"),
                      ((1, hip._ptr(np.array([1, 1], np.int32)), 128, 0, hip._ptr(np.array([1, 1], np.int32)), 2), b"twice"),
                      ((1, hip._ptr(off), 1, 0, hip._ptr(sel), 1), b"without GMR_PREVIEW_BODY_POS")):
        assert L.gmr_motion_tracker_set_preview(t.handle, *args, C.byref(D)) != 0 and why in L.gmr_last_error(), why
    assert L.gmr_motion_tracker_set_preview(t.handle, 1, hip._ptr(off), 2, 2, None, 0, C.byref(D)) == 0 and D.value == 4
    assert L.gmr_motion_tracker_preview_dev(t.handle, None, bufs[0][0].ptr, None, None, None) != 0 and b"base_pos" in L.gmr_last_error()
    nobody = device_library(hip, make_motions(rng, [5, 6], 10, 0), ang_vel="reference")
    t2 = tracker(nobody, 8, 0.02)
    assert L.gmr_motion_tracker_set_preview(t2.handle, 1, hip._ptr(off), 128, 0, hip._ptr(sel), 1, None) != 0 and b"local_body_pos" in L.gmr_last_error()
    assert L.gmr_motion_tracker_set_preview(t2.handle, 1, hip._ptr(off), 16, 1, None, 0, None) != 0 and b"GMR_MOTION_ANGVEL_WORLD" in L.gmr_last_error()
    assert L.gmr_motion_tracker_set_preview(t2.handle, 1, hip._ptr(off), 16, 0, None, 0, None) == 0
