"""Per-body state of the motion library on a real MI355X (csrc/gmr_body_state.hip through motion_library.py): against the sampler
and the FK kernel it joins (bit for bit), against the NumPy mirror (tests/body_state_mirror.py) for the velocities, and the
selection, NULL outputs, bad queries, streams and the hand-over from the dataset driver."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import get_setup

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_state_mirror as bm  # noqa: E402
import motion_mirror as mm  # noqa: E402
from test_motion_body_state_host import ROBOTS, constant_rates, kinematics  # noqa: E402
from test_motion_library import _bits, device_library, make_motions, queries  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
STATE = ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel")
BODY = {"body_pos": 3, "body_rot": 4, "body_vel": 3, "body_ang_vel": 3}
VEL_TOL = 1.5e-5        # x max(1, |row|_inf): float32 walk against the float64 mirror; twice the 6.7e-6 measured over the 14 cases below


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def assert_velocities(got, tree, bodies=None):
    """the device's body_vel / body_ang_vel against the float64 walk of the device's own sampled state"""
    ok = got["status"] == 0
    st = {k: got[k][ok].astype(np.float64) for k in STATE}
    _, _, v, w = bm.walk(tree, st["root_pos"], st["root_rot"], st["root_vel"], st["root_ang_vel"], st["dof_pos"], st["dof_vel"])
    sel = slice(None) if bodies is None else list(bodies)
    worst = 0.0
    for k, want in (("body_vel", v[:, sel]), ("body_ang_vel", w[:, sel])):
        scale = np.maximum(1.0, np.abs(want).max(axis=2, keepdims=True))
        worst = max(worst, float((np.abs(got[k][ok] - want) / scale).max()))
    assert worst <= VEL_TOL, worst
    return worst


@pytest.mark.parametrize("robot", ROBOTS)
@pytest.mark.parametrize("loop", [True, False])
def test_body_state_joins_the_sampler_and_the_fk_kernel(hip, robot, loop):
    km = kinematics(robot)
    fk, tree = km.hip_handle, bm.tree_of(km)
    rng = np.random.default_rng(17 + ROBOTS.index(robot) + 100 * loop)
    motions = make_motions(rng, [1, 2, 40, 257, 300, 3], fk.ndof, 0)
    lib = device_library(hip, motions)
    clip, time = queries(rng, mm.Library(motions), 3001)            # times before 0, on frame boundaries, past the end
    got = lib.body_state(clip, time, kinematics=km, loop=loop)
    assert not got["status"].any()
    ref = lib.sample(clip, time, loop)
    for k in STATE:                                                  # the sampler's arrays, bit for bit
        assert same_bits(got[k], ref[k]), k
    bp, br, _ = fk.fk(ref["root_pos"], ref["root_rot"], ref["dof_pos"])
    assert same_bits(got["body_pos"], bp) and same_bits(got["body_rot"], br)     # the same per-body code: bit-equal
    for k, r in (("body_pos", "root_pos"), ("body_rot", "root_rot"), ("body_vel", "root_vel"), ("body_ang_vel", "root_ang_vel")):
        assert same_bits(got[k][:, 0], got[r]), k                    # body 0 is the root
    worst = assert_velocities(got, tree)
    print(f"\n{robot} loop={loop}: max velocity error / max(1, |row|) = {worst:.3e}")
    # the device-pointer twin, asynchronous, into buffers of exactly the output sizes
    N = len(time)
    d_clip, d_time = hip.DeviceBuffer.from_host(clip), hip.DeviceBuffer.from_host(time)
    outs = {k: hip.DeviceBuffer(N * fk.nbody * w * 4) for k, w in BODY.items()}
    lib.body_state_dev(N, d_clip, d_time, kinematics=fk, loop=loop, **outs)
    hip.check(hip.lib().gmr_stream_sync(None))
    for k, w in BODY.items():
        assert same_bits(outs[k].to_host((N, fk.nbody, w), F), got[k]), k


def sentinel_buffer(hip, rows, width, guard=64):
    a = np.full((rows + guard, width), -7.25, dtype=F)
    return hip.DeviceBuffer.from_host(a), a


def test_a_selection_gives_rows_of_the_full_call_and_writes_nothing_else(hip):
    km = kinematics("unitree_g1")
    names = km.body_names
    rng = np.random.default_rng(5)
    motions = make_motions(rng, [50, 120, 7], km.num_dof, 0)
    lib = device_library(hip, motions).attach_kinematics(km)
    clip, time = queries(rng, mm.Library(motions), 1000)
    full = lib.body_state(clip, time)
    leaves = [n for n in names if "ankle_roll" in n or "wrist_yaw" in n]
    assert len(leaves) == 4
    for bodies in (leaves, [names.index(n) for n in leaves], [30, 3, 4, 5, 6, 7, 8, 0, 29], list(range(37, -1, -1)), [0]):
        idx = [names.index(b) if isinstance(b, str) else b for b in bodies]
        sub = lib.body_state(clip, time, bodies=bodies, state=False)
        assert sorted(sub) == sorted(list(BODY) + ["status"])
        for k in BODY:
            assert same_bits(sub[k], full[k][:, idx]), (k, bodies)
    # a leaf-only selection on the device, sentinels behind every output and in the outputs not asked for
    N, nsel = len(time), len(leaves)
    d_clip, d_time = hip.DeviceBuffer.from_host(clip), hip.DeviceBuffer.from_host(time)
    bufs = {k: sentinel_buffer(hip, N, nsel * w) for k, w in BODY.items()}
    bufs["dof_vel"] = sentinel_buffer(hip, N, km.num_dof)
    skipped = {k: sentinel_buffer(hip, N, w) for k, w in (("root_pos", 3), ("root_rot", 4), ("dof_pos", km.num_dof))}
    lib.body_state_dev(N, d_clip, d_time, bodies=leaves, **{k: b for k, (b, _) in bufs.items()})
    hip.check(hip.lib().gmr_stream_sync(None))
    idx = [names.index(b) for b in leaves]
    for k, (b, init) in bufs.items():
        a = b.to_host(init.shape, F)
        want = full[k][:, idx].reshape(N, -1) if k in BODY else full[k]
        assert same_bits(a[:N], want), k
        assert np.array_equal(a[N:], init[N:]), k                   # nothing behind row N
    for k, (b, init) in skipped.items():
        assert np.array_equal(b.to_host(init.shape, F), init), k     # a NULL output is not touched (these were never handed over)


def test_bad_queries_and_refused_arguments(hip):
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    km = kinematics("unitree_g1")
    rng = np.random.default_rng(9)
    motions = make_motions(rng, [20, 1, 30], km.num_dof, 0)
    lib = device_library(hip, motions)           # (NaN rows behind row B of every input: a read past the library would show)
    clip = np.array([0, 3, -1, 1, 1, 2, 2 ** 31 - 1, -2 ** 31, 0, 1], np.int32)
    time = np.array([0.1, 0.1, 0.1, np.nan, np.inf, 0.1, 0.0, 0.0, -np.inf, 5.0])
    bad, good = [1, 2, 3, 4, 6, 7, 8], [0, 5, 9]
    for loop in (True, False):
        got = lib.body_state(clip, time, kinematics=km, loop=loop)
        assert got["status"].tolist() == [0, 1, 1, 1, 1, 0, 1, 1, 1, 0]
        for k in STATE + tuple(BODY):
            assert np.isnan(got[k][bad]).all() and np.isfinite(got[k][good]).all(), k
        ref = lib.sample(clip, time, loop)
        for k in STATE:
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
        # the clip of one frame: the pose of the frame, no velocity anywhere
        assert not got["body_vel"][9].any() and not got["body_ang_vel"][9].any()
        bp, _, _ = km.hip_handle.fk(ref["root_pos"][9:], ref["root_rot"][9:], ref["dof_pos"][9:])
        assert same_bits(got["body_pos"][9:], bp)
    L = hip.lib()
    table = hip.BodyStateOut()
    args = (lib.handle, km.hip_handle.handle, 4, C.c_void_p(256), C.c_void_p(256), 1)
    sel = np.array([1, 2, 38], np.int32)
    assert L.gmr_motion_body_state_dev(*args, hip._ptr(sel), 3, C.byref(table), None) == -1 and b"body_sel[2]" in L.gmr_last_error()
    assert L.gmr_motion_body_state_dev(*args, hip._ptr(sel), 0, C.byref(table), None) == -1
    assert L.gmr_motion_body_state_dev(*args, hip._ptr(np.array([1, 1], np.int32)), 2, C.byref(table), None) == -1
    assert L.gmr_motion_body_state_dev(*args, None, 0, None, None) == -1
    assert L.gmr_motion_body_state_dev(lib.handle, km.hip_handle.handle, 4, None, None, 1, None, 0, C.byref(table), None) == -1
    assert L.gmr_motion_body_state_dev(lib.handle, km.hip_handle.handle, 4, C.c_void_p(256), C.c_void_p(256), 2, None, 0, C.byref(table), None) == -1
    assert L.gmr_motion_body_state_dev(lib.handle, km.hip_handle.handle, 0, None, None, 1, None, 0, C.byref(table), None) == 0
    other = kinematics("booster_t1").hip_handle
    with pytest.raises(hip.GmrHipError, match="dofs"):
        hip.check(L.gmr_motion_body_state_dev(lib.handle, other.handle, 4, C.c_void_p(256), C.c_void_p(256), 1, None, 0, C.byref(table), None))
    ref_lib = device_library(hip, motions, "reference")
    with pytest.raises(hip.GmrHipError, match="GMR_MOTION_ANGVEL_WORLD"):
        hip.check(L.gmr_motion_body_state_dev(ref_lib.handle, km.hip_handle.handle, 4, C.c_void_p(256), C.c_void_p(256), 1, None, 0,
                                              C.byref(table), None))
    with pytest.raises(ValueError, match='ang_vel="world"'):
        ref_lib.body_state([0], [0.0], kinematics=km)
    with pytest.raises(ValueError):
        lib.body_state_dev(4, hip.DeviceBuffer(16), hip.DeviceBuffer(32), kinematics=km, body_pos=hip.DeviceBuffer(100))
    assert isinstance(lib, MotionLibrary)


def test_constant_rates_and_rigid_motion_on_the_device(hip):
    km = kinematics("unitree_g1")
    m = constant_rates(km.num_dof, T=40)
    lib = device_library(hip, [m]).attach_kinematics(km)
    dt, h = 1.0 / 50.0, 2e-3
    t = (np.arange(2, 36) + 0.5) * dt
    c = np.zeros(len(t), np.int32)
    mid, lo, hi = (lib.body_state(c, t + d, loop=False) for d in (0.0, -h, h))
    # central differences of the device's own float32 positions: 1e-7 of rounding over 2h = 4 ms limits this to ~1e-4 relative
    num = (hi["body_pos"].astype(np.float64) - lo["body_pos"]) / (2 * h)
    assert np.abs(mid["body_vel"] - num).max() <= 2e-3
    assert np.abs(mid["body_ang_vel"][:, 0] - [0.0, 0.0, 1.7]).max() <= 2e-4
    # rigid: no joint moves.  Without rotation every body has the root's velocity; with a yaw rate v_b = v_0 + w x r_b
    for yaw in (0.0, 1.3):
        r = constant_rates(km.num_dof, T=40, yaw=yaw)
        r["dof_pos"] = np.tile(r["dof_pos"][:1], (40, 1))
        rl = device_library(hip, [r])
        out = rl.body_state(c, t, kinematics=km)
        assert not out["dof_vel"].any()
        w = out["root_ang_vel"].astype(np.float64)
        assert np.abs(w - [0.0, 0.0, yaw]).max() <= 2e-4
        assert np.abs(out["body_ang_vel"] - out["root_ang_vel"][:, None]).max() == 0.0
        rb = out["body_pos"].astype(np.float64) - out["root_pos"][:, None]
        want = out["root_vel"][:, None] + np.cross(w[:, None], rb)
        assert np.abs(out["body_vel"] - want).max() <= 1e-5
        if yaw == 0.0:
            assert np.abs(out["body_vel"] - out["root_vel"][:, None]).max() <= 1e-6


def test_two_streams_in_flight_give_the_serial_results(hip):
    rng = np.random.default_rng(11)
    jobs = []
    for robot, lens in (("unitree_g1", [300] * 20), ("booster_t1", [17, 1, 250, 90])):
        km = kinematics(robot)
        motions = make_motions(rng, lens, km.num_dof, 0)
        st = hip.Stream()
        lib = device_library(hip, motions, "world", stream=st).attach_kinematics(km)
        clip, time = queries(rng, mm.Library(motions), 5000)
        bufs = {k: hip.DeviceBuffer(5000 * len(km.body_names) * w * 4) for k, w in BODY.items()}
        jobs.append((lib, km, st, clip, time, hip.DeviceBuffer.from_host(clip), hip.DeviceBuffer.from_host(time), bufs))
    for _ in range(3):                                # enqueued back to back, no synchronisation in between
        for lib, km, st, _, _, d_clip, d_time, bufs in jobs:
            lib.body_state_dev(5000, d_clip, d_time, stream=st, **bufs)
    for job in jobs:
        job[2].sync()
    for lib, km, st, clip, time, _, _, bufs in jobs:
        want = lib.body_state(clip, time, state=False)
        for k, w in BODY.items():
            assert same_bits(bufs[k].to_host((5000, len(km.body_names), w), F), want[k]), k


def test_a_library_from_the_dataset_driver_knows_its_robot(hip, monkeypatch):
    from general_motion_retargeting_amd import dataset, synth
    g1 = get_setup()
    monkeypatch.delenv("GMR_DATASET_POST", raising=False)
    lens, fps = [7, 12, 1, 9], [30.0, 50.0, 30.0, 120.0]
    human, _ = synth.make_streams(g1.model, g1.tt, len(lens), 12, seed=31)
    motions, lib = dataset.retarget_clips("smplx", "unitree_g1", [human[i, :n] for i, n in enumerate(lens)], fps=fps, library=True)
    for c, m in enumerate(motions):
        T = lens[c]
        out = lib.body_state(np.full(T, c), np.arange(T) / fps[c] + 1e-9, loop=False)      # frame times: blend ~ 0
        assert not out["status"].any() and out["body_pos"].shape == (T, 38, 3)
        q = np.asarray(m["root_rot"], dtype=np.float64)
        want = np.asarray(m["root_pos"], dtype=np.float64)[:, None] + bm.qrot(q[:, None], np.asarray(m["local_body_pos"], dtype=np.float64))
        assert np.abs(out["body_pos"] - want).max() <= 5e-6
    _, ref = dataset.retarget_clips("smplx", "unitree_g1", [human[0, :7]], fps=[30.0], library="reference")
    with pytest.raises(ValueError, match='ang_vel="world"'):
        ref.body_state([0], [0.0])
