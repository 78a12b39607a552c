"""The host half of the SMPL-X batch path, no GPU: the target times the kernels compute against np.linspace bit for bit,
which (body model, retargeter) pairs the device path takes, the raw job entries, the environment switch and the no-GPU
fallback, the C interface."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import smplx_synth as sx
from conftest import ROOT

from general_motion_retargeting_amd import _lib, dataset
from general_motion_retargeting_amd.utils import smpl


def test_target_times_are_linspace_bit_for_bit():
    for N in list(range(1, 300)) + [1000, 2001, 5003, 99991, 1 << 20]:
        for skip in (1, 2, 3, 4, 5, 8):
            nout = N // skip
            got, ref = _lib.smplx_target_times(N, nout), np.linspace(0, N - 1, nout)
            assert got.shape == ref.shape and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (N, skip)
    assert _lib.smplx_target_times(7, 0).shape == (0,) and _lib.smplx_target_times(7, 1)[0] == 0.0
    with pytest.raises(_lib.GmrHipError):
        _lib.smplx_target_times(0, 3)


def _retargeter(names):
    return types.SimpleNamespace(human_body_names=list(names))


def test_which_pairs_the_device_path_takes():
    from general_motion_retargeting_amd import GeneralMotionRetargeting, IK_CONFIG_DICT
    bm = sx.body_model(1)
    assert bm.pose_mean[22:].any() and not bm.pose_mean[:22].any()            # the hands' mean pose only
    for robot in IK_CONFIG_DICT["smplx"]:
        assert smpl.smplx_device_takes(bm, GeneralMotionRetargeting("smplx", robot)), robot
    assert smpl.smplx_device_takes(bm, _retargeter(["right_wrist", "head", "pelvis"]))
    assert not smpl.smplx_device_takes(bm, _retargeter(["pelvis", "left_index1"]))       # a hand joint
    assert not smpl.smplx_device_takes(bm, _retargeter(["pelvis", "jaw"]))
    assert not smpl.smplx_device_takes(bm, _retargeter(["pelvis", "no_such_joint"]))
    assert not smpl.smplx_device_takes(bm, _retargeter(["pelvis", "pelvis"]))
    assert not smpl.smplx_device_takes(bm, _retargeter([]))
    other = sx.body_model(1)
    other.pose_mean[9] = 1e-3                                                          # spine3: an ancestor of the wrists
    assert not smpl.smplx_device_takes(other, _retargeter(["left_wrist"])) and smpl.smplx_device_takes(other, _retargeter(["left_foot"]))
    assert not smpl.smplx_device_takes(types.SimpleNamespace(parents=smpl.SMPLX_PARENTS), _retargeter(["pelvis"]))   # a foreign model


def test_raw_entries():
    bm = sx.body_model(2)
    for N, fps in ((1, 30.0), (2, 120.0), (3, 120.0), (97, 59.94), (50, 50.0), (240, 120.0), (241, 100.0), (77, 60.0), (40, 24.0)):
        c = sx.clip(N, fps, 10 + N)
        e = smpl.smplx_raw_clip(c, bm, tgt_fps=30)
        tt, afps = smpl._frame_counts(c, N, 30)
        assert e["N"] == N and e["align"] == (tt is not None) and e["nout"] == (N if tt is None else len(tt)) and e["aligned_fps"] == afps
        assert type(e["nout"]) is int and type(e["align"]) is bool and e["nout"] <= N
        for k, w in (("root_orient", 3), ("pose_body", 63), ("trans", 3)):
            assert e[k].dtype == np.float32 and e[k].shape == (N, w) and e[k].flags.c_contiguous
            assert np.array_equal(e[k], np.asarray(c[k], np.float32))
        assert e["j_rest"].dtype == np.float64 and np.array_equal(e["j_rest"], bm.rest_joints(c["betas"]))
        assert e["height"] == float(1.66 + 0.1 * c["betas"][0])
        # the poses the per-clip path uploads are these, with zeros for the joints nothing reads
        full = bm.full_pose(c["root_orient"], c["pose_body"])
        assert np.array_equal(full[:, 0], e["root_orient"]) and np.array_equal(full[:, 1:22].reshape(N, 63), e["pose_body"])
    e = smpl.smplx_raw_clip({**sx.clip(12, 120.0, 1), "betas": np.zeros((1, 10)), "pose_body": np.zeros((12, 21, 3))}, bm)
    assert e["pose_body"].shape == (12, 63) and e["height"] == 1.66
    for N, fps in ((1, 120.0), (1, 50.0), (0, 30.0)):
        with pytest.raises(_lib.GmrHipError):
            smpl.smplx_raw_clip(sx.clip(N, fps, 3), bm)
    r = sx.ragged([smpl.smplx_raw_clip(sx.clip(N, 120.0, N), bm) for N in (5, 9, 2)])
    assert r["src_start"].tolist() == [0, 5, 14, 16] and r["nout"].tolist() == [1, 2, 0] and r["pose_body"].shape == (16, 63)


def test_environment_switch_and_no_gpu_fallback(monkeypatch):
    monkeypatch.setenv("GMR_DATASET_SMPLX", "host")
    assert dataset.smplx_path() == "host"
    monkeypatch.setenv("GMR_DATASET_SMPLX", " HOST ")
    assert dataset.smplx_path() == "host"
    monkeypatch.delenv("GMR_DATASET_SMPLX")
    monkeypatch.setenv("GMR_DATASET_POST", "host")
    assert dataset.smplx_path() == "host"                    # the batch path writes into the device post-processing's buffers
    monkeypatch.delenv("GMR_DATASET_POST")
    assert dataset.smplx_path() == dataset.post_path()
    if _lib.lib().gmr_device_count() <= 0:
        assert dataset.smplx_path() == "host"
    monkeypatch.setattr(dataset, "post_path", lambda: "host")
    assert dataset.smplx_path() == "host"
    assert dataset.retarget_smplx_loaded([], "nowhere", "unitree_g1") == []


def test_c_interface_declares_and_exports_the_batch_entries():
    from general_motion_retargeting_amd import build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "gmr_hip.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in ("gmr_smplx_batch_frames_dev", "gmr_smplx_batch_frames", "gmr_smplx_batch_takes", "gmr_smplx_target_times"):
        assert re.search(rf"\bint {sym}\s*\(", hdr), sym
        assert hasattr(L, sym) and sym in _lib.EXPORTED_SYMBOLS
    proto = re.search(r"int gmr_smplx_batch_frames_dev\(([^;]*)\);", hdr).group(1)
    for arg in ("nclip", "int B", "d_root_orient", "d_pose_body", "d_trans", "d_src_start", "d_nout", "d_align", "d_j_rest", "d_clip_out",
                "void* stream"):
        assert arg in proto, arg
    assert all(hasattr(_lib.SmplxHandle, m) for m in ("batch_frames_dev", "batch_frames", "batch_takes"))
