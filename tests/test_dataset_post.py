"""The dataset drivers' post-processing on the device (``gmr_postprocess_clips_dev``, ``dataset.DevicePost``) against the
host path it replaces (``dataset.postprocess_clips``): byte for byte, on a real MI355X."""
import json
import os
import pickle
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every shipped robot pack KinematicsModel accepts (engineai_pm01's top file has no <worldbody>: rejected like the reference does)
ROBOTS = ["unitree_g1", "booster_t1", "booster_t1_4dof", "stanford_toddy", "fourier_n1", "kuavo_s45", "hightorque_hi"]


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _km(robot):
    from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT
    return KinematicsModel(ROBOT_XML_DICT[robot])


def _qpos(rng, S, T, nq, lens):
    """valid qpos rows where a clip has frames, NaN where it has none (a read of a padded row shows in the result)"""
    q = np.full((S, T, nq), np.nan)
    for s, n in enumerate(lens):
        q[s, :n, :3] = rng.normal(0, 0.5, size=(n, 3)) + np.array([0.3, -0.2, 0.8])
        w = rng.normal(size=(n, 4))
        q[s, :n, 3:7] = w / np.linalg.norm(w, axis=1, keepdims=True)
        q[s, :n, 7:] = rng.uniform(-1.2, 1.2, size=(n, nq - 7))
    return q


def _device(hip, km, sources, height, origin, ground=0.0, stream=None, want_lowest=True):
    """sources = [(q f64[S,T,nq], lens i32[S] or None)] -> (root_pos, root_rot, dof_pos, local_body_pos, lowest)"""
    fk = km.hip_handle
    nb, ndof = fk.nbody, fk.ndof
    lens_all = np.concatenate([np.full(q.shape[0], q.shape[1], np.int32) if ln is None else np.asarray(ln, np.int32) for q, ln in sources])
    seg = np.concatenate([[0], np.cumsum(lens_all)]).astype(np.int32)
    C, B = len(lens_all), int(seg[-1])
    keep, src = [], []
    for q, ln in sources:
        d_q = hip.DeviceBuffer.from_host(q)
        d_l = None if ln is None else hip.DeviceBuffer.from_host(np.asarray(ln, np.int32))
        keep += [d_q, d_l]
        src.append((q.shape[0], q.shape[1], d_q, d_l))
    d_seg = hip.DeviceBuffer.from_host(seg)
    outs = [hip.DeviceBuffer(max(B, 1) * n) for n in (24, 32, max(ndof, 1) * 8, nb * 12)]
    d_low = hip.DeviceBuffer(max(C, 1) * 4) if want_lowest else None
    fk.postprocess_clips_dev(src, d_seg, C, B, *outs, d_low, height, origin, ground, stream)
    (stream.sync if stream is not None else lambda: hip.check(hip.lib().gmr_stream_sync(None)))()
    res = [outs[0].to_host((B, 3), np.float64), outs[1].to_host((B, 4), np.float64), outs[2].to_host((B, ndof), np.float64),
           outs[3].to_host((B, nb, 3), np.float32)]
    res.append(d_low.to_host((C,), np.float32) if want_lowest else None)
    return res, seg


def _host(km, sources, height, origin, ground=0.0):
    from general_motion_retargeting_amd import dataset
    clips = []
    for q, ln in sources:
        for s in range(q.shape[0]):
            clips.append(q[s, : (q.shape[1] if ln is None else ln[s])])
    return dataset.postprocess_clips(clips, km, [30.0] * len(clips), height, origin, ground), clips


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same(dev, seg, host):
    rp, rr, dp, lb, _ = dev
    for c, md in enumerate(host):
        a, b = int(seg[c]), int(seg[c + 1])
        for got, key in ((rp, "root_pos"), (rr, "root_rot"), (dp, "dof_pos"), (lb, "local_body_pos")):
            want = np.asarray(md[key])
            assert want.dtype == got.dtype and want.shape == got[a:b].shape, (c, key)
            assert np.array_equal(_bits(got[a:b]), _bits(want)), (c, key)


def _host_lowest(km, clips):
    out = np.full(len(clips), np.inf, np.float32)
    for c, q in enumerate(clips):
        if len(q):
            out[c] = km.hip_handle.fk(q[:, :3].astype(np.float32), q[:, [4, 5, 6, 3]].astype(np.float32), q[:, 7:].astype(np.float32),
                                      want_rot=False, want_min_z=True)[2]
    return out


@pytest.mark.parametrize("robot", ROBOTS)
def test_device_post_is_byte_equal_to_the_host_path(hip, robot):
    """every shipped robot (their nbody differ: the flush alignment, the trees that do not split), the four flag combinations,
    a non-zero ground offset, ragged lengths around the 64-row blocks with empty clips first, in the middle and last, and
    NaN in every padded row"""
    km = _km(robot)
    nq, T = km.num_dof + 7, 130
    rng = np.random.default_rng(100 + ROBOTS.index(robot))
    lens = np.array([0, 1, 63, 64, 65, 0, 127, T, 5, 0], np.int32)
    q = _qpos(rng, len(lens), T, nq, lens)
    for height in (False, True):
        for origin in (False, True):
            ground = 0.037 if height else 0.0
            dev, seg = _device(hip, km, [(q, lens)], height, origin, ground)
            host, clips = _host(km, [(q, lens)], height, origin, ground)
            _assert_same(dev, seg, host)
            if height:
                assert np.array_equal(_bits(dev[4]), _bits(_host_lowest(km, clips)))
                assert np.isinf(dev[4][[0, 5, 9]]).all()


def test_one_clip_and_a_large_batch(hip):
    km = _km("unitree_g1")
    rng = np.random.default_rng(3)
    q = _qpos(rng, 1, 9, 36, [9])
    dev, seg = _device(hip, km, [(q, np.array([9], np.int32))], True, True)
    _assert_same(dev, seg, _host(km, [(q, [9])], True, True)[0])
    S, T = 2100, 24
    lens = rng.integers(0, T + 1, size=S).astype(np.int32)
    q = _qpos(rng, S, T, 36, lens)
    dev, seg = _device(hip, km, [(q, lens)], True, True, 0.01, want_lowest=False)
    _assert_same(dev, seg, _host(km, [(q, lens)], True, True, 0.01)[0])


def test_two_sources_and_null_len(hip):
    km = _km("unitree_g1")
    rng = np.random.default_rng(4)
    la, lb = np.array([3, 0, 70, 11], np.int32), np.array([20, 20, 7], np.int32)
    qa, qb = _qpos(rng, 4, 70, 36, la), _qpos(rng, 3, 20, 36, lb)
    dev, seg = _device(hip, km, [(qa, la), (qb, lb)], True, True)
    _assert_same(dev, seg, _host(km, [(qa, la), (qb, lb)], True, True)[0])
    full = _qpos(rng, 5, 13, 36, [13] * 5)
    d1, s1 = _device(hip, km, [(full, None)], True, False)
    d2, s2 = _device(hip, km, [(full, np.full(5, 13, np.int32))], True, False)
    assert np.array_equal(s1, s2) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(d1, d2))
    _assert_same(d1, s1, _host(km, [(full, None)], True, False)[0])


def test_bad_arguments_are_refused_before_any_launch(hip):
    km = _km("unitree_g1")
    fk = km.hip_handle
    L, C = hip.lib(), __import__("ctypes")
    q = hip.DeviceBuffer(2 * 4 * 36 * 8)
    seg = hip.DeviceBuffer.from_host(np.array([0, 4, 8], np.int32))
    out = [hip.DeviceBuffer(8 * n) for n in (24, 32, 29 * 8, 38 * 12)]
    src = (hip.PostSrc * 1)(hip.PostSrc(2, 4, q.ptr.value, None))

    def call(nq=36, Cn=2, B=8, flags=3, outs=None, srcp=src, nsrc=1, segp=seg.ptr):
        o = [b.ptr for b in out] if outs is None else outs
        return L.gmr_postprocess_clips_dev(fk.handle, C.cast(srcp, C.c_void_p), nsrc, nq, segp, Cn, B, flags, 0.0, o[0], o[1], o[2], o[3],
                                           None, None)

    assert call() == 0
    assert call(nq=35) == -1 and b"nq" in L.gmr_last_error()
    assert call(Cn=-1) == -1 and call(B=-1) == -1 and call(Cn=3) == -1 and call(B=9) == -1
    assert call(flags=4) == -1 and call(nsrc=9) == -1 and call(segp=None) == -1
    assert call(outs=[None, out[1].ptr, out[2].ptr, out[3].ptr]) == -1 and call(outs=[out[0].ptr, out[1].ptr, out[2].ptr, None]) == -1
    bad = (hip.PostSrc * 1)(hip.PostSrc(2, 4, None, None))
    assert call(srcp=bad) == -1
    hip.check(L.gmr_stream_sync(None))


def test_two_streams_in_flight_use_their_own_scratch(hip):
    """one call on each of two streams, enqueued back to back without a synchronisation in between, on one handle"""
    km = _km("unitree_g1")
    fk = km.hip_handle
    rng = np.random.default_rng(6)
    jobs = []
    for S, T in ((700, 64), (300, 90)):
        lens = rng.integers(1, T + 1, size=S).astype(np.int32)
        q = _qpos(rng, S, T, 36, lens)
        seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        B = int(seg[-1])
        jobs.append({"q": q, "lens": lens, "seg": seg, "B": B, "S": S, "T": T, "st": hip.Stream(), "d_q": hip.DeviceBuffer.from_host(q),
                     "d_l": hip.DeviceBuffer.from_host(lens), "d_seg": hip.DeviceBuffer.from_host(seg),
                     "outs": [hip.DeviceBuffer(B * n) for n in (24, 32, 29 * 8, 38 * 12)], "low": hip.DeviceBuffer(S * 4)})
    for j in jobs:
        fk.postprocess_clips_dev([(j["S"], j["T"], j["d_q"], j["d_l"])], j["d_seg"], j["S"], j["B"], *j["outs"], j["low"], True, True, 0.0,
                                 j["st"])
    for j in jobs:
        j["st"].sync()
    for j in jobs:
        B = j["B"]
        dev = [j["outs"][0].to_host((B, 3), np.float64), j["outs"][1].to_host((B, 4), np.float64), j["outs"][2].to_host((B, 29), np.float64),
               j["outs"][3].to_host((B, 38, 3), np.float32), None]
        _assert_same(dev, j["seg"], _host(km, [(j["q"], j["lens"])], True, True)[0])


def _dicts_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is None:
            continue
        assert list(x) == list(y) and x["fps"] == y["fps"] and x["link_body_list"] == y["link_body_list"]
        for k in ("root_pos", "root_rot", "dof_pos", "local_body_pos"):
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and np.array_equal(_bits(x[k]), _bits(y[k])), k


def _pkl(md, keys):
    return pickle.dumps({k: md[k] for k in keys})


def test_retarget_clips_device_path_equals_host_path(hip, g1, monkeypatch):
    from general_motion_retargeting_amd import dataset, synth
    lens = [7, 12, 1, 9, 64, 65]
    human, _ = synth.make_streams(g1.model, g1.tt, len(lens), 65, seed=31)
    clips = [human[i, :n] for i, n in enumerate(lens)]
    monkeypatch.delenv("GMR_DATASET_POST", raising=False)
    assert dataset.post_path() == "device"
    dev = dataset.retarget_clips("smplx", "unitree_g1", clips, fps=[30.0] * len(lens))
    monkeypatch.setenv("GMR_DATASET_POST", "host")
    assert dataset.post_path() == "host"
    host = dataset.retarget_clips("smplx", "unitree_g1", clips, fps=[30.0] * len(lens))
    _dicts_equal(dev, host)
    for a, b in zip(dev, host):
        assert _pkl(a, dataset.SMPLX_KEYS) == _pkl(b, dataset.SMPLX_KEYS) and _pkl(a, dataset.BVH_KEYS) == _pkl(b, dataset.BVH_KEYS)


def test_retarget_smplx_files_device_path_equals_host_path(hip, tmp_path, monkeypatch):
    from general_motion_retargeting_amd import dataset
    from general_motion_retargeting_amd.utils import smpl
    rng = np.random.default_rng(11)
    J, V = 55, 90
    v = rng.normal(0, 0.3, size=(V, 3)) + np.array([0, 0, 1.0])
    sd = rng.normal(0, 0.01, size=(V, 3, 20))
    jr = rng.uniform(0, 1, size=(J, V))
    jr /= jr.sum(1, keepdims=True)
    kt = np.stack([np.where(smpl.SMPLX_PARENTS < 0, 2**32 - 1, smpl.SMPLX_PARENTS), np.arange(J)]).astype(np.uint32)
    os.makedirs(tmp_path / "models" / "smplx")
    for gdr in ("NEUTRAL", "FEMALE"):
        np.savez(tmp_path / "models" / "smplx" / f"SMPLX_{gdr}.npz", v_template=v, shapedirs=sd, J_regressor=jr, kintree_table=kt)
    betas = [rng.normal(0, 0.5, size=16), rng.normal(0, 0.5, size=16)]
    files = []
    for i, (N, rate, subj, gdr) in enumerate(((40, 120.0, 0, "neutral"), (25, 60.0, 1, "female"), (31, 120.0, 0, "neutral"))):
        f = tmp_path / f"clip{i}.npz"
        np.savez(f, gender=np.array(gdr), betas=betas[subj], root_orient=np.cumsum(rng.normal(0, 0.02, size=(N, 3)), 0),
                 pose_body=np.cumsum(rng.normal(0, 0.02, size=(N, 63)), 0),
                 trans=np.cumsum(rng.normal(0, 0.01, size=(N, 3)), 0) + np.array([0, 0, 0.9]), mocap_frame_rate=np.array(rate))
        files.append(str(f))
    files.insert(1, str(tmp_path / "missing.npz"))
    monkeypatch.delenv("GMR_DATASET_POST", raising=False)
    dev = dataset.retarget_smplx_files(files, str(tmp_path / "models"), "unitree_g1")
    monkeypatch.setenv("GMR_DATASET_POST", "host")
    host = dataset.retarget_smplx_files(files, str(tmp_path / "models"), "unitree_g1")
    assert dev[1] is None
    _dicts_equal(dev, host)
    for a, b in zip(dev, host):
        if a is not None:
            assert _pkl(a, dataset.SMPLX_KEYS) == _pkl(b, dataset.SMPLX_KEYS)


def test_nine_jobs_in_one_run_equal_their_clips_as_one_job(hip, g1):
    """More jobs than one post-processing call takes (8): the second call starts at a row that is a multiple of 4, and every
    clip gets what it gets as a stream of ONE job (the streams of a group launch do not depend on each other)."""
    from general_motion_retargeting_amd import GeneralMotionRetargeting, dataset, synth
    nine = [[3, 2], [1], [2], [1, 1], [3], [2], [1], [2, 1], [2]]
    spans9 = [[(0, 3), (3, 5)], [(5, 6)], [(6, 8)], [(8, 9), (9, 10)], [(10, 13)], [(13, 15)], [(15, 16)], [(16, 18), (18, 19)], [(20, 22)]]
    gmr, km = GeneralMotionRetargeting("smplx", "unitree_g1"), _km("unitree_g1")
    human, _ = synth.make_streams(g1.model, g1.tt, 12, 3, seed=47)
    human = np.ascontiguousarray(human, dtype=np.float64)
    job = lambda a, lens: {"solver": gmr.hip_solver, "human": human[a:a + len(lens)], "lens": np.array(lens, np.int32), "q0": gmr.model.qpos0}   # noqa: E731
    first = np.cumsum([0] + [len(l) for l in nine])
    post = dataset.DevicePost()
    many = post.run([job(int(a), l) for a, l in zip(first, nine)], km)
    one = post.run([job(0, [n for l in nine for n in l])], km)
    assert many[4] == spans9 and [len(s) for s in many[5]] == [len(l) for l in nine] and many[0].shape[0] == 24
    assert one[4] == [[(a, a + n) for a, n in zip(np.cumsum([0, 3, 2, 1, 2, 1, 1, 3, 2, 1, 2, 1]).tolist(), [n for l in nine for n in l])]]
    assert np.array_equal(np.concatenate(many[5]), one[5][0]) and one[5][0].dtype == np.int32 and len(one[5][0]) == 12
    for (a, b), (c, d) in zip([s for sp in many[4] for s in sp], one[4][0]):
        for x, y in zip(many[:4], one[:4]):
            assert x.dtype == y.dtype and np.array_equal(_bits(x[a:b]), _bits(y[c:d])), (a, b, c, d)


def test_dicts_of_an_earlier_batch_survive_later_batches(hip, g1, monkeypatch):
    from general_motion_retargeting_amd import dataset, synth
    monkeypatch.delenv("GMR_DATASET_POST", raising=False)
    rt = dataset.ClipRetargeter("smplx", "unitree_g1")
    human, _ = synth.make_streams(g1.model, g1.tt, 6, 20, seed=41)
    first = rt([human[i, : 20 - i] for i in range(3)], [30.0] * 3)
    snap = [{k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in md.items()} for md in first]
    second = rt([human[i, : 20 - i] for i in range(3, 6)], [30.0] * 3)
    third = rt([human[i, :11] for i in range(2)], [30.0] * 2)
    _dicts_equal(first, snap)
    assert not any(np.shares_memory(a["dof_pos"], b["dof_pos"]) for a in first for b in second + third)
    assert set(rt.timing) >= {"h2d", "ik", "post", "d2h"} and all(np.isfinite(v) and v >= 0 for v in rt.timing.values())
    pool = rt._dev_post.pool
    assert pool.blocks_allocated == 3 and pool.free_blocks == 0
    del second, third
    assert pool.free_blocks == 2                        # a block comes back when the last view of it dies ...
    rt([human[0, :5]], [30.0])
    assert pool.blocks_allocated == 3                   # ... and serves a later batch
    monkeypatch.setenv("GMR_DATASET_POST", "host")
    _dicts_equal(first, dataset.retarget_clips("smplx", "unitree_g1", [human[i, : 20 - i] for i in range(3)], [30.0] * 3))


def test_pipeline_with_a_slow_writer_writes_what_the_host_path_writes(hip, g1, tmp_path, monkeypatch):
    from general_motion_retargeting_amd import dataset, synth
    human, _ = synth.make_streams(g1.model, g1.tt, 12, 16, seed=43)
    lens = [16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5]
    src = {str(tmp_path / "src" / f"c{i:02d}.bvh"): human[i, :n] for i, n in enumerate(lens)}
    real_dump = dataset._dump

    def slow_dump(tgt, motion, keys):
        time.sleep(0.05)                                # the dicts of several batches wait for the writers
        real_dump(tgt, motion, keys)

    def run(tag):
        rt = dataset.ClipRetargeter("smplx", "unitree_g1")
        pipe = dataset.DatasetPipeline(lambda f: src[f], dataset._Staged(rt, 30), len, dataset.SMPLX_KEYS, frames_budget=48, max_clips=3,
                                       writers=1, verbose=False)
        jobs = [(f, str(tmp_path / tag / os.path.basename(f).replace(".bvh", ".pkl"))) for f in src]
        assert pipe.run(jobs) == len(src) and pipe.stats["batches"] >= 4
        return [open(t, "rb").read() for _, t in jobs]

    monkeypatch.setattr(dataset, "_dump", slow_dump)
    monkeypatch.delenv("GMR_DATASET_POST", raising=False)
    dev = run("dev")
    monkeypatch.setenv("GMR_DATASET_POST", "host")
    assert dev == run("host")


@pytest.mark.timeout(600)
def test_post_probe_reports_finite_numbers(hip):
    """tools/dataset_post_probe.py (the measurement of the device post-processing by itself) at a small size, in a process of
    its own as a user runs it"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dataset_post_probe.py"), "512", "64", "3"], capture_output=True,
                       text=True, timeout=550)
    assert r.returncode == 0, r.stderr[-2000:]
    leg = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for k in ("device_both_adjustments", "device_no_adjustment", "fk_f32_positions_only"):
        assert np.isfinite(leg[k]) and leg[k] > 0
    assert leg["n"] == 3 and leg["host_path"]["bytes_equal_to_device"] is True
    assert all(0 < v < 1 for v in leg["fraction_of_hbm_peak"].values())
