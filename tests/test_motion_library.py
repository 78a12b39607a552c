"""The motion library on a real MI355X (csrc/gmr_motion.hip through motion_library.py) against the NumPy mirror
(tests/motion_mirror.py) and against the fixture generated from the reference's training loader (tests/golden/g_motion.npz)."""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import get_setup

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_mirror as mm  # noqa: E402
from test_motion_edges_host import ANGVEL_C  # noqa: E402
from test_motion_library_host import FIELDS, check_against_golden, close, constant_rate_clip, golden, golden_motions  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
ROBOTS = ["unitree_g1", "booster_t1", "booster_t1_4dof", "stanford_toddy", "fourier_n1", "kuavo_s45", "hightorque_hi"]
LIB_ARRAYS = ("root_pos", "root_rot", "dof_pos", "root_vel", "root_ang_vel", "dof_vel", "stats")


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_motions(rng, lens, ndof, nbody, fps_choices=(30.0, 50.0, 120.0, 29.97)):
    """float64 clips as the post-processing leaves them; quaternion tracks with flips, near-identical runs and large steps"""
    out = []
    for n in lens:
        q = rng.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        for i in range(1, n):          # thirds: a random jump, a small step, a small step in the other hemisphere
            if i % 3:
                q[i] = q[i - 1] + rng.normal(size=4) * (3e-3 if i % 3 == 1 else 0.2)
                q[i] /= np.linalg.norm(q[i])
                if i % 5 == 0:
                    q[i] = -q[i]
        out.append({"fps": float(rng.choice(fps_choices)), "root_pos": rng.normal(0, 0.5, size=(n, 3)) + np.array([0.3, -0.2, 0.8]),
                    "root_rot": q, "dof_pos": rng.uniform(-1.2, 1.2, size=(n, ndof)),
                    "local_body_pos": rng.normal(size=(n, nbody, 3)).astype(F) if nbody else None})
    return out


def device_library(hip, motions, ang_vel="world", stream=None, pad_rows=3):
    """``MotionLibrary.from_device`` from float64 device arrays that carry NaN sentinel rows behind row B: a read past the
    batch shows in the result"""
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    seg = np.concatenate([[0], np.cumsum([len(m["root_pos"]) for m in motions])]).astype(np.int32)
    fps = [m["fps"] for m in motions]
    has_body = motions[0]["local_body_pos"] is not None
    bufs = []
    for k, dt in (("root_pos", np.float64), ("root_rot", np.float64), ("dof_pos", np.float64), ("local_body_pos", np.float32)):
        if k == "local_body_pos" and not has_body:
            bufs.append(None)
            continue
        a = np.concatenate([np.asarray(m[k], dtype=dt) for m in motions])
        a = np.concatenate([a, np.full((pad_rows,) + a.shape[1:], np.nan, dtype=dt)])
        bufs.append(hip.DeviceBuffer.from_host(a))
    ndof = motions[0]["dof_pos"].shape[1]
    nbody = motions[0]["local_body_pos"].shape[1] if has_body else 0
    lib = MotionLibrary.from_device(seg, fps, ndof, nbody, *bufs, ang_vel=ang_vel, stream=stream)
    (stream.sync if stream is not None else lambda: hip.check(hip.lib().gmr_stream_sync(None)))()
    return lib


def assert_library_equals_mirror(lib, mirror):
    for k in ("root_pos", "root_rot", "dof_pos", "root_vel", "dof_vel"):
        got, want = lib.array(k), getattr(mirror, k)
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), k
    if mirror.local_body_pos is not None:
        assert np.array_equal(_bits(lib.array("local_body_pos")), _bits(mirror.local_body_pos))
    # root_ang_vel and the stats' mean and std are FP64 evaluations rounded once, here and in the mirror: one float32 spacing apart at
    # the most (tests/test_motion_edges.py holds both to mpmath), or, for a component of root_ang_vel near zero, the FP64 floor of
    # both evaluations (ANGVEL_C 2^-52 / dt each, dt >= 1 / 120 here).  min and max are data: bit for bit.
    def spacing_apart(a, b, floor=0.0):
        a, b = a.astype(np.float64), b.astype(np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        tol = np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(F)).astype(np.float64), floor)
        return bool((np.abs(a - b)[~np.isnan(a)] <= tol[~np.isnan(a)]).all())

    assert spacing_apart(lib.array("root_ang_vel"), mirror.root_ang_vel, 2 * ANGVEL_C * 2.0 ** -52 * 120.0)
    stats = lib.array("stats")
    assert spacing_apart(stats[:, :2], mirror.stats[:, :2])
    assert np.array_equal(_bits(stats[:, 2:]), _bits(mirror.stats[:, 2:]))


# ---- 1. fill -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
@pytest.mark.parametrize("ang_vel", ["world", "reference"])
def test_fill_equals_the_mirror_on_ragged_batches(hip, robot, ang_vel):
    from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT
    fk = KinematicsModel(ROBOT_XML_DICT[robot]).hip_handle
    rng = np.random.default_rng(7 + ROBOTS.index(robot))
    lens = [1, 2, 63, 64, 65, 1, 129, 2, 300] + rng.integers(1, 200, size=30).tolist()
    motions = make_motions(rng, lens, fk.ndof, fk.nbody)
    lib = device_library(hip, motions, ang_vel)
    assert (lib.num_clips, lib.num_frames, lib.ndof, lib.nbody) == (len(lens), sum(lens), fk.ndof, fk.nbody)
    mirror = mm.Library(motions, ang_vel)
    assert_library_equals_mirror(lib, mirror)
    one = lib.clip(0)                                   # a clip of one frame: zero velocities, NaN std
    assert one.num_frames == 1 and not one.root_vel.any() and not one.root_ang_vel.any() and not one.dof_vel.any()
    assert np.isnan(one.root_pos_std).all() and np.isnan(one.dof_pos_std).all()
    v = lib.clip(8)
    assert v.num_frames == 300 and v.fps == motions[8]["fps"] and v.dt == 1.0 / v.fps and v.motion_duration == 300 / v.fps
    assert np.array_equal(v.dof_pos_max, mirror.stats[8, 3, 3:]) and np.array_equal(v.root_vel[0], v.root_vel[1])


def test_fill_of_a_long_clip_and_without_local_body_pos(hip):
    rng = np.random.default_rng(3)
    motions = make_motions(rng, [10000, 5, 1], 29, 0)
    lib = device_library(hip, motions)
    assert not lib.has_local_body_pos
    assert_library_equals_mirror(lib, mm.Library(motions))
    with pytest.raises(KeyError):
        lib.sample([0], [0.0], local_body_pos=True)
    with pytest.raises(hip.GmrHipError, match="without local_body_pos"):
        lib.sample_dev(1, hip.DeviceBuffer(4), hip.DeviceBuffer(8), local_body_pos=hip.DeviceBuffer(64))


def test_the_synchronous_fill_with_and_without_local_body_pos(hip):
    """``gmr_motion_lib_fill`` takes host arrays (the package itself fills from device memory): with local_body_pos and with the
    mandatory arrays alone, the arrays both libraries hold are the same bits, and those of a library filled on the device.  2 clips of
    4 and 5 frames, 2 dofs, 3 bodies."""
    from general_motion_retargeting_amd.motion_library import ANGVEL, MotionLibrary
    rng = np.random.default_rng(19)
    motions = make_motions(rng, [4, 5], 2, 3)
    seg = np.concatenate([[0], np.cumsum([len(m["root_pos"]) for m in motions])]).astype(np.int32)
    rp, rr, dp = (np.ascontiguousarray(np.concatenate([m[k] for m in motions]), dtype=np.float64) for k in ("root_pos", "root_rot", "dof_pos"))
    body = np.ascontiguousarray(np.concatenate([m["local_body_pos"] for m in motions]), dtype=F)

    def filled(lbp):
        lib = MotionLibrary.__new__(MotionLibrary)
        lib.device = lib.motion_dir = None
        lib._create(seg, [m["fps"] for m in motions], 2, 3, "world")
        hip.check(hip.lib().gmr_motion_lib_fill(lib.handle, hip._ptr(rp), hip._ptr(rr), hip._ptr(dp), hip._ptr(lbp), ANGVEL["world"]))
        lib.has_local_body_pos = lbp is not None
        return lib

    full, bare, ref = filled(body), filled(None), device_library(hip, motions)
    for k in LIB_ARRAYS:
        assert np.array_equal(_bits(full.array(k)), _bits(bare.array(k))) and np.array_equal(_bits(full.array(k)), _bits(ref.array(k))), k
    assert np.array_equal(_bits(full.array("local_body_pos")), _bits(ref.array("local_body_pos"))) and full.array("dof_vel").any()
    assert bare.device_array("local_body_pos") == (None, 0)


def test_world_mode_on_constant_rates(hip):
    for axis in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
        m = constant_rate_clip(axis, 1.7)
        m["local_body_pos"] = None
        lib = device_library(hip, [m], "world")
        close(lib.array("root_ang_vel"), np.tile(np.array(axis, F) * F(1.7), (20, 1)), abs_=2e-4)


# ---- 2. the reference's numbers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 1, 2])
def test_device_reproduces_the_reference_loader(hip, c):
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    g = golden()
    lib = MotionLibrary.from_motions([golden_motions(g)[c]], ang_vel="reference")
    v = lib.clip(0)
    derived = {k: getattr(v, k) for k in ("root_vel", "root_ang_vel", "dof_vel")}
    check_against_golden(g, c, derived, lib.array("stats")[0], lambda t, loop: lib.sample(np.zeros(len(t), np.int32), t, loop))


# ---- 3. sample -----------------------------------------------------------------------------------------------------------------
def queries(rng, mirror, N):
    C_ = len(mirror.fps)
    clip = rng.integers(0, C_, size=N)
    T = (mirror.seg[clip + 1] - mirror.seg[clip]).astype(np.float64)
    dur = T / mirror.fps[clip]
    time = rng.uniform(-1.0, 2.5, size=N) * dur
    k = N // 4                          # a quarter on exact frame times, some of them on the last frame
    time[:k] = rng.integers(0, 400, size=k) % T[:k] / mirror.fps[clip[:k]]
    time[k:k + k // 4] = (T[k:k + k // 4] - 1 + rng.uniform(0, 1, size=k // 4)) / mirror.fps[clip[k:k + k // 4]]
    return clip.astype(np.int32), time


def assert_sample_equals_mirror(got, want, local_body_pos):
    for k in ("root_pos", "root_vel", "root_ang_vel", "dof_pos", "dof_vel") + (("local_body_pos",) if local_body_pos else ()):
        assert got[k].shape == want[k].shape and np.array_equal(_bits(got[k]), _bits(want[k])), k
    close(got["root_rot"], want["root_rot"], abs_=1e-6)
    assert np.array_equal(got["status"], want["status"])


@pytest.mark.parametrize("N", [1, 4096, 65537])
@pytest.mark.parametrize("loop", [True, False])
def test_sample_equals_the_mirror(hip, N, loop):
    rng = np.random.default_rng(N + loop)
    motions = make_motions(rng, [1, 2, 40, 257, 1000, 3], 29, 38)
    lib = device_library(hip, motions)
    mirror = mm.Library(motions)
    mirror.root_ang_vel = lib.array("root_ang_vel").copy()      # (pinned above to 1e-5; from here on the lerp is bit for bit)
    clip, time = queries(rng, mirror, N) if N > 1 else (np.array([3], np.int32), np.array([0.7321]))
    got = lib.sample(clip, time, loop, local_body_pos=True)
    want = mirror.sample(clip, time, loop, local_body_pos=True)
    if N > 1:       # the query set reaches every branch: frame itself, nlerp, slerp, each also with a flipped hemisphere
        assert {0, 1, 2, 5, 6} <= set(want["branch"].tolist())
    assert_sample_equals_mirror(got, want, True)
    assert not got["status"].any() and all(np.isfinite(got[k]).all() for k in FIELDS)


# ---- 4. the drop-in classes --------------------------------------------------------------------------------------------------
def test_motion_loader_is_a_row_of_the_batched_sample(hip, tmp_path):
    from general_motion_retargeting_amd import MotionLibrary, MotionLoader, data_loader
    g = golden()
    ms = golden_motions(g)
    for c, m in enumerate(ms):
        m["link_body_list"] = [f"b{k}" for k in range(5)]
        data_loader.save_robot_motion(str(tmp_path / f"m{c}.pkl"), m, training_compatible=(c == 1))
    ld = MotionLoader(str(tmp_path / "m2.pkl"), loop=True, motion_time_offset=0.123)
    assert (ld.fps, ld.num_frames, ld.dt, ld.motion_duration, ld.get_motion_length()) == (120.0, 240, 1 / 120.0, 2.0, 2.0)
    assert ld.link_body_list == [f"b{k}" for k in range(5)] and ld.local_body_pos.shape == (240, 5, 3) and ld.library.ang_vel == "reference"
    close(ld.root_ang_vel, g["c2_root_ang_vel"], abs_=1e-5)
    close(np.concatenate([ld.root_pos_mean, ld.dof_pos_mean]), g["c2_stats"][0], rel=1e-5, abs_=1e-6)
    times = np.array([0.0, 0.2, 0.5004, 1.99, 2.0, 7.77, -0.4])
    batch = ld.library.sample(np.zeros(len(times), np.int32), times + 0.123, True)
    for i, t in enumerate(times):
        st = ld.get_motion_state(float(t))
        assert sorted(st) == sorted(FIELDS)
        for k in FIELDS:
            assert st[k].shape == batch[k].shape[1:] and np.array_equal(_bits(st[k]), _bits(batch[k][i])), (k, t)
    close(ld.get_motion_state(0.2)["root_pos"], g["c2_offset_root_pos"], rel=1e-6)
    ld.reset(0.0)
    ld.loop = False
    assert ld.motion_time_offset == 0.0 and np.array_equal(ld.get_motion_state(50.0)["dof_pos"], ld.get_motion_state(2.0 - 1 / 120.0)["dof_pos"])
    with pytest.raises(FileNotFoundError):
        MotionLoader(str(tmp_path / "missing.pkl"))
    # the directory form: one library for the files of one robot, a file that does not fit is reported and skipped
    (tmp_path / "broken.pkl").write_bytes(b"not a pickle")
    lib = MotionLibrary(str(tmp_path), motion_files=["m0.pkl", "broken.pkl", "m2.pkl"])
    assert lib.get_motion_names() == ["m0", "m2"] and lib.num_clips == 2 and lib.ang_vel == "world"
    a = lib.sample_motion("m2")
    assert a is lib.sample_motion("m2") and a.num_frames == 240 and lib.sample_motion().library is lib
    assert np.array_equal(a.get_motion_state(0.3)["dof_pos"], ld.get_motion_state(0.3)["dof_pos"])
    with pytest.raises(ValueError):
        lib.sample_motion("m1")
    both = MotionLibrary.from_files([str(tmp_path / "m0.pkl"), str(tmp_path / "m2.pkl")])
    for k in LIB_ARRAYS:
        assert np.array_equal(_bits(both.array(k)), _bits(lib.array(k)), ), k


# ---- 5. bad queries ------------------------------------------------------------------------------------------------------------
def test_bad_queries_are_neutralised(hip):
    rng = np.random.default_rng(5)
    motions = make_motions(rng, [20, 30], 12, 4)
    lib = device_library(hip, motions)
    mirror = mm.Library(motions)
    mirror.root_ang_vel = lib.array("root_ang_vel").copy()
    clip = np.array([0, 2, -1, 1, 1, 1, 2 ** 31 - 1, -2 ** 31, 0], np.int32)
    time = np.array([0.1, 0.1, 0.1, np.nan, np.inf, 0.1, 0.0, 0.0, -np.inf])
    for loop in (True, False):
        got = lib.sample(clip, time, loop, local_body_pos=True)
        assert got["status"].tolist() == [0, 1, 1, 1, 1, 0, 1, 1, 1]
        want = mirror.sample(clip, time, loop, local_body_pos=True)
        assert_sample_equals_mirror(got, want, True)
        for k in FIELDS + ("local_body_pos",):
            assert np.isnan(got[k][[1, 2, 3, 4, 6, 7, 8]]).all() and np.isfinite(got[k][[0, 5]]).all(), k
    # huge and negative times without loop are clamped to the clip
    got = lib.sample([1, 1, 1], [1e300, -1e300, -0.01], loop=False)
    assert not got["status"].any()
    assert np.array_equal(got["dof_pos"][1], mirror.dof_pos[20]) and np.array_equal(got["dof_pos"][2], mirror.dof_pos[20])
    # argument checks of the entry points
    L = hip.lib()
    assert L.gmr_motion_sample_dev(lib.handle, -1, None, None, 0, *[None] * 9) == -1
    assert L.gmr_motion_sample_dev(lib.handle, 4, None, None, 0, *[None] * 9) == -1
    assert L.gmr_motion_sample_dev(lib.handle, 4, None, None, 2, *[None] * 9) == -1 and b"flag" in L.gmr_last_error()
    assert L.gmr_motion_sample_dev(lib.handle, 0, None, None, 0, *[None] * 9) == 0
    assert L.gmr_motion_lib_array(lib.handle, 10, None, None) == -1
    assert L.gmr_motion_lib_fill_dev(lib.handle, None, None, None, None, 0, None) == -1
    assert L.gmr_motion_lib_fill_dev(lib.handle, C.c_void_p(256), C.c_void_p(256), C.c_void_p(256), None, 2, None) == -1
    with pytest.raises(ValueError):
        lib.sample_dev(4, hip.DeviceBuffer(16), hip.DeviceBuffer(32), root_pos=hip.DeviceBuffer(47))


# ---- 6. hand-over from the dataset driver ----------------------------------------------------------------------------------------
def test_retarget_clips_hands_its_batch_to_a_library(hip, monkeypatch):
    from general_motion_retargeting_amd import MotionLibrary, dataset, synth
    g1 = get_setup()
    monkeypatch.delenv("GMR_DATASET_POST", raising=False)
    assert dataset.post_path() == "device"
    lens = [7, 12, 1, 9, 64, 65]
    fps = [30.0, 50.0, 30.0, 120.0, 30.0, 60.0]
    human, _ = synth.make_streams(g1.model, g1.tt, len(lens), 65, seed=31)
    clips = [human[i, :n] for i, n in enumerate(lens)]
    plain = dataset.retarget_clips("smplx", "unitree_g1", clips, fps=fps)
    for mode, arg in (("world", True), ("reference", "reference")):
        motions, lib = dataset.retarget_clips("smplx", "unitree_g1", clips, fps=fps, library=arg)
        assert lib.ang_vel == mode and lib.seg_start.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist() and lib.fps_list == fps
        assert len(motions) == len(plain)
        for a, b in zip(motions, plain):
            assert pickle.dumps({k: a[k] for k in dataset.SMPLX_KEYS}) == pickle.dumps({k: b[k] for k in dataset.SMPLX_KEYS})
        up = MotionLibrary.from_motions(motions, ang_vel=mode)
        for k in LIB_ARRAYS + ("local_body_pos",):
            assert np.array_equal(_bits(lib.array(k)), _bits(up.array(k))), k
        assert lib.clip(4).link_body_list == list(motions[4]["link_body_list"])
        t = np.linspace(-0.5, 3.0, 50)
        a, b = lib.sample(np.arange(50) % 6, t, local_body_pos=True), up.sample(np.arange(50) % 6, t, local_body_pos=True)
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    # the host post-processing path builds the same library through one upload
    monkeypatch.setenv("GMR_DATASET_POST", "host")
    motions_h, lib_h = dataset.retarget_clips("smplx", "unitree_g1", clips, fps=fps, library="reference")
    for k in LIB_ARRAYS:
        assert np.array_equal(_bits(lib_h.array(k)), _bits(lib.array(k))), k


# ---- 7. streams and lifetimes --------------------------------------------------------------------------------------------------
def test_two_libraries_on_their_own_streams(hip):
    rng = np.random.default_rng(11)
    jobs = []
    for lens, ndof, nbody in (([300] * 40, 29, 38), ([17, 1, 250, 90], 23, 24)):
        motions = make_motions(rng, lens, ndof, nbody)
        st = hip.Stream()
        lib = device_library(hip, motions, "world", stream=st)
        mirror = mm.Library(motions)
        clip, time = queries(rng, mirror, 5000)
        d_clip, d_time = hip.DeviceBuffer.from_host(clip), hip.DeviceBuffer.from_host(time)
        d_body = hip.DeviceBuffer(5000 * nbody * 12)
        outs = {"root_pos": hip.DeviceBuffer(5000 * 12), "root_rot": hip.DeviceBuffer(5000 * 16), "dof_vel": hip.DeviceBuffer(5000 * ndof * 4),
                "local_body_pos": d_body.ptr.value, "status": hip.DeviceBuffer(5000 * 4)}       # (a raw address is taken too)
        jobs.append((lib, mirror, st, clip, time, d_clip, d_time, outs, ndof, (nbody, d_body)))
    for lib, _, st, _, _, d_clip, d_time, outs, _, _ in jobs:      # enqueued back to back, no synchronisation in between
        lib.sample_dev(5000, d_clip, d_time, loop=True, stream=st, **outs)
    for job in jobs:
        job[2].sync()
    for lib, mirror, st, clip, time, _, _, outs, ndof, (nbody, d_body) in jobs:
        mirror.root_ang_vel = lib.array("root_ang_vel").copy()
        want = mirror.sample(clip, time, True, local_body_pos=True)
        assert np.array_equal(_bits(outs["root_pos"].to_host((5000, 3), F)), _bits(want["root_pos"]))
        assert np.array_equal(_bits(outs["dof_vel"].to_host((5000, ndof), F)), _bits(want["dof_vel"]))
        close(outs["root_rot"].to_host((5000, 4), F), want["root_rot"], abs_=1e-6)
        assert not outs["status"].to_host((5000,), np.int32).any()
        assert np.array_equal(_bits(d_body.to_host((5000, nbody, 3), F)), _bits(want["local_body_pos"]))
        host = lib.sample(clip, time, True, local_body_pos=True)       # the host-pointer twin gives the same bits
        assert np.array_equal(_bits(host["local_body_pos"]), _bits(want["local_body_pos"]))
    jobs[0][0].close()
    assert jobs[1][0].sample([0], [0.1])["status"].tolist() == [0]


def test_sample_dev_writes_into_torch_tensors(hip):
    """anything with ``data_ptr()``: tensors of a ROCm build of PyTorch, on the stream both sides use by default"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("this PyTorch build sees no GPU")
    rng = np.random.default_rng(2)
    motions = make_motions(rng, [50, 120, 7], 29, 38)
    lib = device_library(hip, motions)
    mirror = mm.Library(motions)
    mirror.root_ang_vel = lib.array("root_ang_vel").copy()
    N, dev = 1000, "cuda:0"
    clip, time = queries(rng, mirror, N)
    t_clip, t_time = torch.from_numpy(clip).to(dev), torch.from_numpy(time).to(dev)
    shapes = {"root_pos": (3,), "root_rot": (4,), "root_vel": (3,), "root_ang_vel": (3,), "dof_pos": (29,), "dof_vel": (29,),
              "local_body_pos": (38, 3)}
    outs = {k: torch.full((N,) + s, -7.0, dtype=torch.float32, device=dev) for k, s in shapes.items()}
    status = torch.full((N,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lib.sample_dev(N, t_clip, t_time, loop=True, status=status, **outs)
    hip.check(hip.lib().gmr_stream_sync(None))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    got["status"] = status.cpu().numpy()
    assert_sample_equals_mirror(got, mirror.sample(clip, time, True, local_body_pos=True), True)
    # what a tensor says about itself is checked before anything is launched
    for bad in (outs["root_pos"].double(), outs["root_pos"][:10], outs["dof_pos"].t(), torch.zeros(N, 3)):
        with pytest.raises(ValueError):
            lib.sample_dev(N, t_clip, t_time, root_pos=bad)
    with pytest.raises(ValueError):
        lib.sample_dev(N, t_clip.long(), t_time)
    with pytest.raises(ValueError):
        lib.sample_dev(N, t_clip, t_time.float())
