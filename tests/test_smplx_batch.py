"""gmr_smplx_batch_frames(_dev) (csrc/gmr_smplx.hip): a ragged batch of AMASS-shaped clips -> packed human frames written where
the IK kernels read them, against one gmr_smplx_frames call per clip -- BIT FOR BIT (the sign of a zero included) --, and the
SMPL-X dataset drivers on top of it against their per-clip path (GMR_DATASET_SMPLX=host)."""
import ctypes as C
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import smplx_synth as sx
from conftest import ROOT

pytestmark = pytest.mark.gpu
SENT, GUARD, NG = -12345.678, 7.0e77, 64


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def lib():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def setup(lib):
    from general_motion_retargeting_amd.utils import smpl
    bms = [sx.body_model(1), sx.body_model(2)]
    return bms, smpl._handle(smpl.SMPLX_PARENTS, sx.G1_BODIES)


def _entries(bms, specs, seed0=1000):
    """specs = [(N, fps)] -> (clips, raw entries, body model of each); a different subject (betas) per clip"""
    from general_motion_retargeting_amd.utils import smpl
    clips = [sx.clip(N, fps, seed0 + i) for i, (N, fps) in enumerate(specs)]
    which = [bms[i % len(bms)] for i in range(len(clips))]
    return clips, [smpl.smplx_raw_clip(c, bm) for c, bm in zip(clips, which)], which


def _upload(lib, h, entries, jobs_T, job_of, stream=None):
    """device inputs of one call; every clip's destination is a block of its job's T frames of its own, sentinel-filled, with
    guard words in front and behind.  Returns (argument tuple, device buffers, block offsets, host image of the output)."""
    r = sx.ragged(entries)
    W = h.rows * 7
    offs, pos = [], 0
    for e, j in zip(entries, job_of):
        offs.append(pos + NG)
        pos += 2 * NG + jobs_T[j] * W
    host = np.full((max(pos, 1),), GUARD)
    for o, j in zip(offs, job_of):
        host[o:o + jobs_T[j] * W] = SENT
    d_out = lib.DeviceBuffer.from_host(host, stream)
    tab = np.array([d_out.ptr.value + 8 * o for o in offs], dtype=np.uint64)
    names = ("root_orient", "pose_body", "trans", "src_start", "nout", "align", "j_rest")
    # the inputs lie in ONE device block with guard words between them
    parts, img = {}, []
    for k, a in list((k, r[k]) for k in names) + [("tab", tab)]:
        img.append(np.full(256, 0xA5, np.uint8))
        parts[k] = sum(len(x) for x in img)
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        img.append(np.concatenate([raw, np.zeros(-len(raw) % 256, np.uint8)]))
    img.append(np.full(256, 0xA5, np.uint8))
    img = np.concatenate(img)
    d_in = lib.DeviceBuffer.from_host(img, stream)
    at = lambda k: C.c_void_p(d_in.ptr.value + parts[k])      # noqa: E731
    args = (len(entries), int(r["src_start"][-1]), at("root_orient"), at("pose_body"), at("trans"), at("src_start"), at("nout"),
            at("align"), at("j_rest"), at("tab"))
    return args, (d_in, img, d_out, host), offs


def _specs():
    rng = np.random.default_rng(7)
    specs = [(1, 30.0), (2, 120.0), (2, 60.0), (3, 120.0), (4, 120.0), (7, 120.0), (8, 120.0), (2, 50.0), (1, 30.0), (2, 30.0),
             (4000, 120.0), (1200, 30.0), (2500, 59.94), (63, 30.0), (64, 30.0), (65, 30.0), (255, 120.0), (256, 120.0), (257, 100.0)]
    while len(specs) < 320:
        fps = sx.FPS[len(specs) % len(sx.FPS)]
        specs.append((int(rng.integers(1 if fps == 30.0 else 2, 400)), fps))
    return specs


@pytest.fixture(scope="module")
def big(lib, setup):
    bms, h = setup
    specs = _specs()
    clips, entries, which = _entries(bms, specs)
    # a clip with exact and negative zeros in its poses (the host path adds the model's zero mean pose: -0.0 -> +0.0)
    entries[20]["pose_body"][::2, :9] = -0.0
    entries[20]["root_orient"][1::2] = 0.0
    clips[20]["pose_body"], clips[20]["root_orient"] = entries[20]["pose_body"].astype(np.float64), entries[20]["root_orient"].astype(np.float64)
    nouts = [e["nout"] for e in entries]
    job_of = [0 if n <= 60 else 1 for n in nouts]
    jobs_T = [60, max(nouts)]
    st = lib.Stream()
    args, (d_in, img, d_out, host), offs = _upload(lib, h, entries, jobs_T, job_of, st)
    h.batch_frames_dev(*args, st)
    st.sync()
    return {"clips": clips, "entries": entries, "which": which, "job_of": job_of, "jobs_T": jobs_T, "offs": offs,
            "back": d_out.to_host(host.shape, np.float64), "in_back": d_in.to_host(img.shape, np.uint8), "img": img}


def test_ragged_batch_has_the_bits_of_the_per_clip_calls(setup, big):
    bms, h = setup
    W = h.rows * 7
    nouts = [e["nout"] for e in big["entries"]]
    assert len(nouts) >= 300 and 0 in nouts and 1 in nouts and max(nouts) >= 1000
    aligned_same_count = [e for e in big["entries"] if e["align"] and e["nout"] == e["N"]]
    assert aligned_same_count, "a 50 -> 30 fps clip: interpolated although no frame is dropped"
    for i, (c, e, bm) in enumerate(zip(big["clips"], big["entries"], big["which"])):
        ref = sx.reference_frames(h, bm, c)
        o = big["offs"][i]
        got = big["back"][o:o + e["nout"] * W].reshape(e["nout"], h.rows, 7)
        assert ref.shape[0] == e["nout"] and _bits(got, ref), (i, e["N"], float(c["mocap_frame_rate"]))


def test_nothing_is_written_outside_the_frames_of_a_clip(setup, big):
    _, h = setup
    W = h.rows * 7
    for i, e in enumerate(big["entries"]):
        o, T = big["offs"][i], big["jobs_T"][big["job_of"][i]]
        assert np.all(big["back"][o + e["nout"] * W: o + T * W] == SENT)                 # frames at and beyond nout[c]
        assert np.all(big["back"][o - NG:o] == GUARD) and np.all(big["back"][o + T * W: o + T * W + NG] == GUARD)
    assert np.array_equal(big["in_back"], big["img"])                                   # the inputs and the words between them


def test_a_clip_does_not_depend_on_its_neighbours(lib, setup):
    bms, h = setup
    specs = [(333, 120.0), (50, 30.0), (97, 59.94), (2, 120.0), (700, 100.0), (41, 50.0)]
    clips, entries, which = _entries(bms, specs, seed0=50)
    k = 2
    alone = h.batch_frames(**sx.ragged([entries[k]]))[0]
    assert _bits(alone, sx.reference_frames(h, which[k], clips[k]))
    for order in ([2, 0, 1, 3, 4, 5], [0, 1, 3, 4, 5, 2], [0, 1, 3, 2, 4, 5]):
        out = h.batch_frames(**sx.ragged([entries[i] for i in order]))
        assert _bits(out[order.index(k), : entries[k]["nout"]], alone)
        assert not out[order.index(k), entries[k]["nout"]:].any()                       # the host entry point: zeros beyond nout


def _model_folder(tmp_path):
    return sx.write_models(tmp_path / "models")


def test_driver_output_does_not_depend_on_batch_composition(lib, tmp_path):
    from general_motion_retargeting_amd import dataset
    models = _model_folder(tmp_path)
    betas = np.random.default_rng(3).normal(0, 0.5, size=(2, 16))
    raws = [sx.clip(90, 120.0, 1, "neutral", betas[0]), sx.clip(33, 30.0, 2, "female", betas[1]), sx.clip(61, 59.94, 3, "neutral", betas[0])]
    assert dataset.smplx_path() == "device"
    calls = []
    orig = lib.SmplxHandle.batch_frames_dev
    lib.SmplxHandle.batch_frames_dev = lambda self, *a, **k: (calls.append(a[0]), orig(self, *a, **k))[1]
    try:
        together = dataset.retarget_smplx_loaded(raws, models, "unitree_g1")
        assert calls == [3]                                                              # ONE call for both height groups
        for i in (2, 0, 1):
            single = dataset.retarget_smplx_loaded([raws[i]], models, "unitree_g1")[0]
            for key in dataset.SMPLX_KEYS:
                assert pickle.dumps(single[key]) == pickle.dumps(together[i][key]), (i, key)
    finally:
        lib.SmplxHandle.batch_frames_dev = orig


def test_every_shipped_selection_is_taken_and_a_hand_joint_is_refused(lib, setup, tmp_path, monkeypatch):
    from general_motion_retargeting_amd import GeneralMotionRetargeting, IK_CONFIG_DICT, dataset
    from general_motion_retargeting_amd.utils import smpl
    bms, _ = setup
    clips, entries, which = _entries(bms, [(40, 120.0), (9, 30.0), (17, 50.0)], seed0=70)
    for robot in IK_CONFIG_DICT["smplx"]:
        g = GeneralMotionRetargeting("smplx", robot)
        assert smpl.smplx_device_takes(bms[0], g), robot
        h = smpl.smplx_batch_handle(bms[0], g)
        assert h.batch_takes and h.rows == len(g.human_body_names)
        out = h.batch_frames(**sx.ragged(entries))
        for i, (c, e, bm) in enumerate(zip(clips, entries, which)):
            assert _bits(out[i, : e["nout"]], sx.reference_frames(h, bm, c)), (robot, i)
    hand = smpl._handle(smpl.SMPLX_PARENTS, [0, 20, smpl.SMPLX_JOINT_NAMES.index("left_index1")])
    assert not hand.batch_takes
    with pytest.raises(lib.GmrHipError, match="body joints"):
        hand.batch_frames(**sx.ragged(entries))
    a = (3, int(sum(e["N"] for e in entries))) + (C.c_void_p(256),) * 8               # refused before anything is read or launched
    with pytest.raises(lib.GmrHipError, match="body joints"):
        hand.batch_frames_dev(*a)
    everything = smpl._handle(smpl.SMPLX_PARENTS)                                        # all 55 joints
    assert not everything.batch_takes
    # a body model the device path does not take (a mean pose on a body joint): the driver computes the frames per clip, with
    # the results of GMR_DATASET_SMPLX=host
    models = _model_folder(tmp_path)
    bm = smpl.body_model_for(models, "neutral")
    raws = [sx.clip(44, 120.0, 5, "neutral"), sx.clip(20, 30.0, 6, "neutral")]
    monkeypatch.setattr(lib.SmplxHandle, "batch_frames_dev", lambda *a, **k: pytest.fail("the batch entry point was called"))
    try:
        bm.pose_mean[3] = 0.01
        assert not smpl.smplx_device_takes(bm, GeneralMotionRetargeting("smplx", "unitree_g1"))
        fell_back = dataset.retarget_smplx_loaded(raws, models, "unitree_g1")
        monkeypatch.setenv("GMR_DATASET_SMPLX", "host")
        host = dataset.retarget_smplx_loaded(raws, models, "unitree_g1")
    finally:
        bm.pose_mean[3] = 0.0
    for x, y in zip(fell_back, host):
        assert pickle.dumps({k: x[k] for k in dataset.SMPLX_KEYS}) == pickle.dumps({k: y[k] for k in dataset.SMPLX_KEYS})


def test_host_entry_refuses_inconsistent_tables(lib, setup):
    bms, h = setup
    _, entries, _ = _entries(bms, [(40, 120.0), (9, 30.0), (17, 50.0)], seed0=80)
    good = sx.ragged(entries)
    assert h.batch_frames(**good).shape == (3, 17, h.rows, 7)

    def bad(**kw):
        a = {k: v.copy() for k, v in good.items()}
        for k, f in kw.items():
            f(a[k])
        with pytest.raises(lib.GmrHipError):
            h.batch_frames(**a)

    def setitem(i, v):
        return lambda arr: arr.__setitem__(i, v)
    bad(src_start=setitem(1, 50))                 # descending
    bad(src_start=setitem(3, 65))                 # the last entry is not B
    bad(src_start=setitem(0, 1))                  # does not start at 0
    bad(nout=setitem(1, 10))                      # nout > N
    bad(nout=setitem(1, 8))                       # without alignment nout must be N
    bad(nout=setitem(0, -1))
    bad(src_start=lambda s: s.__setitem__(slice(1, 3), [40, 41]), nout=setitem(1, 0), align=setitem(1, 1))      # alignment of one frame
    with pytest.raises(lib.GmrHipError):
        h.batch_frames(**good, T=16)              # a clip longer than T
    with pytest.raises(ValueError):
        h.batch_frames(**{**good, "j_rest": good["j_rest"][:2]})
    assert h.batch_frames(**sx.ragged([])).shape == (0, 1, h.rows, 7)
    # ... and what the per-clip path rejects, the raw entry rejects before anything is uploaded
    from general_motion_retargeting_amd.utils import smpl
    with pytest.raises(lib.GmrHipError, match="two source frames"):
        smpl.smplx_raw_clip(sx.clip(1, 120.0, 1), bms[0])
    with pytest.raises(lib.GmrHipError, match="two source frames"):
        smpl.smplx_frames_packed_fused(type("R", (), {"human_body_names": ["pelvis"]})(), sx.clip(1, 120.0, 1), bms[0])


def test_two_streams_in_flight_use_their_own_scratch(lib, setup):
    bms, h = setup
    ca, ea, wa = _entries(bms, [(3000, 120.0), (500, 30.0), (77, 50.0)] * 6, seed0=300)
    cb, eb, wb = _entries(bms, [(100, 60.0), (2000, 100.0)] * 9, seed0=400)
    s1, s2 = lib.Stream(), lib.Stream()
    W = h.rows * 7
    runs = []
    for st, e in ((s1, ea), (s2, eb)):
        T = max(x["nout"] for x in e)
        runs.append((e, T) + _upload(lib, h, e, [T], [0] * len(e), st))
    for _ in range(2):                                   # the second round reuses the blocks the first one grew
        for (e, T, args, bufs, offs), st in zip(runs, (s1, s2)):
            h.batch_frames_dev(*args, st)
    s1.sync()
    s2.sync()
    for (e, T, args, (d_in, img, d_out, host), offs), clips, which in zip(runs, (ca, cb), (wa, wb)):
        back = d_out.to_host(host.shape, np.float64)
        for i, x in enumerate(e):
            got = back[offs[i]: offs[i] + x["nout"] * W].reshape(x["nout"], h.rows, 7)
            assert _bits(got, sx.reference_frames(h, which[i], clips[i]))


_CHILD = r"""
import json, pickle, sys
sys.path.insert(0, sys.argv[1])
from general_motion_retargeting_amd import dataset
assert dataset.smplx_path() == "host"
out = dataset.retarget_smplx_files(json.loads(sys.argv[2]), sys.argv[3], "unitree_g1")
with open(sys.argv[4], "wb") as f:
    pickle.dump(out, f)
"""


def test_files_dataset_and_cli_against_the_per_clip_path(lib, tmp_path, capfd):
    from general_motion_retargeting_amd import dataset
    models = _model_folder(tmp_path)
    src = tmp_path / "src"
    betas = np.random.default_rng(5).normal(0, 0.5, size=(3, 16))
    files = []
    for i, (N, fps, gdr, subj) in enumerate(((120, 120.0, "neutral", 0), (45, 30.0, "female", 1), (64, 60.0, "female", 2), (51, 50.0, "neutral", 0),
                                             (200, 59.94, "neutral", 1), (9, 120.0, "female", 2), (1, 30.0, "neutral", 2))):
        files.append(sx.write_clip(str(src / ("sub" if i % 3 == 2 else "") / f"clip{i}.npz"), sx.clip(N, fps, 40 + i, gdr, betas[subj])))
    broken = str(src / "broken.npz")
    with open(broken, "wb") as f:
        f.write(b"not an npz file")
    assert dataset.smplx_path() == "device"
    dev = dataset.retarget_smplx_files(files[:3] + [broken] + files[3:], models, "unitree_g1")
    assert "Error loading" in capfd.readouterr().out and dev[3] is None
    dev = dev[:3] + dev[4:]
    env = dict(os.environ, GMR_DATASET_SMPLX="host")
    ref_pkl = str(tmp_path / "host.pkl")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(files), models, ref_pkl], check=True, env=env, timeout=900)
    with open(ref_pkl, "rb") as f:
        ref = pickle.load(f)
    as_file = lambda md: pickle.dumps({k: md[k] for k in dataset.SMPLX_KEYS})      # noqa: E731  (what dataset._dump writes)
    assert len(dev) == len(ref) == len(files)
    for a, b in zip(dev, ref):
        assert as_file(a) == as_file(b)
    assert dev[5]["dof_pos"].shape[0] == 2 and dev[6]["dof_pos"].shape[0] == 1       # 9 frames at 120 fps, a one-frame clip
    # the dataset driver on the folder: the unreadable file is printed and skipped, every other file is written
    tgt = str(tmp_path / "tgt")
    stats = {}
    n = dataset.run_smplx_dataset(str(src), tgt, "unitree_g1", models, verbose=False, loader_workers=2, stats=stats)
    assert n == len(files) and stats["load_errors"] == 1
    assert "Error loading" in capfd.readouterr().out
    parts = stats["seconds_gpu_parts"]
    assert parts["frames"] > 0.0 and parts["ik"] > 0.0
    by_name = {os.path.relpath(f, str(src))[:-4]: md for f, md in zip(files, ref)}
    for name, md in by_name.items():
        with open(os.path.join(tgt, name + ".pkl"), "rb") as f:
            assert f.read() == as_file(md), name
    assert not os.path.exists(os.path.join(tgt, "broken.pkl"))
    # ... and the CLI in a child process on the per-clip path: the same bytes in every file, no `frames` stage
    tgt2 = str(tmp_path / "tgt_host")
    r = subprocess.run([sys.executable, "-m", "general_motion_retargeting_amd.dataset", "--source", "smplx", "--src_folder", str(src),
                        "--tgt_folder", tgt2, "--smplx_folder", models, "--hard_motions", "--num_cpus", "2", "--quiet"],
                       env=dict(env, PYTHONPATH=ROOT), cwd=ROOT, timeout=900, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    summary = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"dataset_summary"')][-1])["dataset_summary"]
    assert summary["files_written"] == len(files) and "frames" not in summary["rank0"]["seconds_gpu_parts"]
    assert "Error loading" in r.stdout
    for name in by_name:
        with open(os.path.join(tgt, name + ".pkl"), "rb") as f, open(os.path.join(tgt2, name + ".pkl"), "rb") as f2:
            assert f.read() == f2.read(), name
    assert dataset.main(["--source", "smplx", "--src_folder", str(src), "--tgt_folder", str(tmp_path / "tgt3"), "--smplx_folder", models,
                         "--hard_motions", "--num_cpus", "0", "--quiet"]) == 0
    for name in by_name:
        with open(os.path.join(tgt, name + ".pkl"), "rb") as f, open(os.path.join(str(tmp_path / "tgt3"), name + ".pkl"), "rb") as f2:
            assert f.read() == f2.read(), name
