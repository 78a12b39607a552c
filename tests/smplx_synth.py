"""Synthetic SMPL-X material for the batch tests: body models built the way tests/test_smplx_frames.py::_synthetic_model
builds one (in memory and as ``SMPLX_<GENDER>.npz`` files), AMASS-shaped clips, and ragged batches of them."""
import os

import numpy as np

from general_motion_retargeting_amd.utils import smpl

FPS = (120.0, 100.0, 60.0, 59.94, 50.0, 30.0)
G1_BODIES = [0, 1, 2, 4, 5, 7, 8, 12, 16, 17, 18, 19, 20, 21]


def model_arrays(seed, J=55, V=90, nb=20):
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 0.3, size=(V, 3)) + np.array([0, 0, 1.0])
    sd = rng.normal(0, 0.01, size=(V, 3, nb))
    jr = rng.uniform(0, 1, size=(J, V))
    jr /= jr.sum(1, keepdims=True)
    hm = rng.normal(0, 0.1, size=(30, 3))
    return v, sd, jr, hm


def body_model(seed, J=55):
    v, sd, jr, hm = model_arrays(seed, J)
    return smpl.SmplxBodyModel.from_arrays(v, sd, jr, smpl.SMPLX_PARENTS[:J], num_betas=10, hand_mean=hm)


def write_models(folder, genders=("NEUTRAL", "FEMALE")):
    """``folder/smplx/SMPLX_<GENDER>.npz`` with a different synthetic model per gender (hands' mean pose included)"""
    J = 55
    kt = np.stack([np.where(smpl.SMPLX_PARENTS < 0, 2**32 - 1, smpl.SMPLX_PARENTS), np.arange(J)]).astype(np.uint32)
    os.makedirs(os.path.join(folder, "smplx"), exist_ok=True)
    for i, g in enumerate(genders):
        v, sd, jr, hm = model_arrays(100 + i)
        np.savez(os.path.join(folder, "smplx", f"SMPLX_{g}.npz"), v_template=v, shapedirs=sd, J_regressor=jr, kintree_table=kt,
                 hands_meanl=hm[:15].reshape(-1), hands_meanr=hm[15:].reshape(-1))
    return str(folder)


def clip(N, fps, seed, gender="neutral", betas=None, dtype=np.float64):
    """the arrays of one AMASS file (float64 like the files; the drivers cast)"""
    rng = np.random.default_rng(seed)
    return {"gender": np.array(gender), "betas": rng.normal(0, 0.5, size=16) if betas is None else np.asarray(betas),
            "root_orient": np.cumsum(rng.normal(0, 0.03, size=(N, 3)), 0).astype(dtype),
            "pose_body": np.cumsum(rng.normal(0, 0.03, size=(N, 63)), 0).astype(dtype),
            "trans": (np.cumsum(rng.normal(0, 0.01, size=(N, 3)), 0) + np.array([0, 0, 0.9])).astype(dtype),
            "mocap_frame_rate": np.array(fps)}


def write_clip(path, c):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, **c)
    return str(path)


def reference_frames(handle, bm, c, tgt_fps=30):
    """one ``gmr_smplx_frames`` call for the clip: what the per-clip driver computes"""
    full = bm.full_pose(c["root_orient"], c["pose_body"])
    tt, _ = smpl._frame_counts(c, full.shape[0], tgt_fps)
    return handle.frames(bm.rest_joints(c["betas"]), full, np.asarray(c["trans"], np.float32).reshape(-1, 3), tt)


def ragged(entries):
    """the arguments of ``SmplxHandle.batch_frames`` for a list of ``smpl.smplx_raw_clip`` entries"""
    seg = np.concatenate([[0], np.cumsum([e["N"] for e in entries])]).astype(np.int32)
    cat = lambda k, w: (np.concatenate([e[k] for e in entries]) if entries else np.zeros((0, w), np.float32))      # noqa: E731
    return {"root_orient": cat("root_orient", 3), "pose_body": cat("pose_body", 63), "trans": cat("trans", 3), "src_start": seg,
            "nout": np.array([e["nout"] for e in entries], dtype=np.int32), "align": np.array([e["align"] for e in entries], dtype=np.uint8),
            "j_rest": np.stack([e["j_rest"] for e in entries]) if entries else np.zeros((0, 55, 3))}
