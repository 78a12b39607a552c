#!/usr/bin/env python3
"""Generate tests/golden/g_tracker.npz by RUNNING the reference's training-side loader (``booster_gym/utils/motion_loader.py``, CPU
torch + scipy) the way its imitation environment drives it (``booster_gym/envs/t1_imitation.py:103-207, 249-309``; the environment
itself needs a simulator and cannot run here): per environment one ``get_motion_state`` at a float32 clock that a float32 torch
tensor advances with ``+= dt``, the 21 -> 23 map of the motion's dofs onto the robot's (head at zero; in stage 1 the legs at their
default pose with velocity zero), scripted clip changes, and the six tracking formulas evaluated in float32 torch against a seeded
simulator state.

Three clips of 21 dofs -- 40 / 90 / 25 frames at 30 / 50 / 120 fps -- six environments, 60 steps of dt = 0.02, loop on; the map
changes from stage 1 to the full map after step 30.  Only numbers are stored (``np.savez_compressed``; loadable with
allow_pickle=False); no line of the reference is copied.

    python tests/golden/make_tracker_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import importlib.util
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_motion_golden import make_clip  # noqa: E402

CLIPS = ((40, 30, 21), (90, 50, 21), (25, 120, 21))     # frames, fps, ndof
ENVS, STEPS, DT, STAGE2_FROM = 6, 60, 0.02, 30
R = 23
# robot [0-1 head] [2-9 arms] [10 waist] [11-22 legs] <- motion [0-7 arms] [8 waist] [9-20 legs]
MAP_FULL = np.array([-1, -1] + list(range(0, 8)) + [8] + list(range(9, 21)), dtype=np.int32)
MAP_STAGE1 = np.where(np.arange(R) >= 11, -1, MAP_FULL).astype(np.int32)
SCALES = (0.5, 0.5, 2.0, 1.0, 1.0, 0.1)
# (step, environment, clip, time): applied before that step
SCRIPT = ((0, 0, 0, 0.0), (0, 1, 1, 0.25), (0, 2, 2, 0.1), (0, 3, 1, 1.7), (0, 4, 0, 1.3), (0, 5, 2, 0.0),
          (12, 2, 1, 0.0), (20, 4, 2, 0.05), (35, 0, 1, 0.9), (35, 5, 0, 0.333), (50, 3, 2, 0.0))


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    spec = importlib.util.spec_from_file_location("reference_motion_loader", os.path.join(ref, "booster_gym", "utils", "motion_loader.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(20250921)
    out = {"nclip": np.array(len(CLIPS)), "dt": np.array(DT), "map_full": MAP_FULL, "map_stage1": MAP_STAGE1, "stage2_from": np.array(STAGE2_FROM),
           "scales": np.array(SCALES), "script": np.array(SCRIPT, dtype=np.float64)}
    default = rng.uniform(-0.4, 0.4, R).astype(np.float32)
    default[:2] = 0.0                                       # the head stays at zero in either stage
    out["dof_default"] = default
    loaders = []
    with tempfile.TemporaryDirectory() as tmp:
        for c, (T, fps, ndof) in enumerate(CLIPS):
            m = make_clip(rng, T, fps, ndof)
            f = os.path.join(tmp, f"clip{c}.pkl")
            with open(f, "wb") as fh:
                pickle.dump(m, fh)
            for k in ("root_pos", "root_rot", "dof_pos"):
                out[f"c{c}_{k}"] = m[k]
            out[f"c{c}_fps"] = np.array(float(fps))
            loaders.append(mod.MotionLoader(f, device="cpu", loop=True))
    motion_times = torch.zeros(ENVS, dtype=torch.float32)
    env_clip = [0] * ENVS
    default_t = torch.from_numpy(default)
    names = ("ref_root_pos", "ref_root_rot", "ref_root_vel", "ref_root_ang_vel", "ref_dof_pos", "ref_dof_vel")
    sim_names = ("base_pos", "base_quat", "base_lin_vel", "base_ang_vel", "dof_pos", "dof_vel")
    rec = {k: [] for k in names + sim_names + ("err", "term", "time", "clip")}
    for step in range(STEPS):
        for s, e, c, t in SCRIPT:
            if s == step:
                env_clip[e] = c
                motion_times[e] = t
        stage1 = step < STAGE2_FROM
        ref = {"ref_root_pos": torch.zeros(ENVS, 3), "ref_root_rot": torch.zeros(ENVS, 4), "ref_root_vel": torch.zeros(ENVS, 3),
               "ref_root_ang_vel": torch.zeros(ENVS, 3), "ref_dof_pos": torch.zeros(ENVS, R), "ref_dof_vel": torch.zeros(ENVS, R)}
        rec["time"].append(motion_times.numpy().copy())
        rec["clip"].append(np.array(env_clip, dtype=np.int32))
        for e in range(ENVS):
            st = loaders[env_clip[e]].get_motion_state(motion_times[e].item())
            for k in ("root_pos", "root_rot", "root_vel", "root_ang_vel"):
                ref[f"ref_{k}"][e] = st[k]
            pos, vel = torch.zeros(R), torch.zeros(R)
            pos[2:11], vel[2:11] = st["dof_pos"][0:9], st["dof_vel"][0:9]
            if stage1:
                pos[11:23] = default_t[11:23]
            else:
                pos[11:23], vel[11:23] = st["dof_pos"][9:21], st["dof_vel"][9:21]
            ref["ref_dof_pos"][e], ref["ref_dof_vel"][e] = pos, vel
        motion_times += DT
        # a simulator that follows the reference loosely (a random offset per array, smaller every ten steps)
        amp = 0.4 / (1 + step // 10)
        q = ref["ref_root_rot"] + amp * torch.from_numpy(rng.standard_normal((ENVS, 4)).astype(np.float32))
        sim = {"base_pos": ref["ref_root_pos"] + amp * torch.from_numpy(rng.standard_normal((ENVS, 3)).astype(np.float32)),
               "base_quat": q / q.norm(dim=1, keepdim=True),
               "base_lin_vel": ref["ref_root_vel"] + amp * torch.from_numpy(rng.standard_normal((ENVS, 3)).astype(np.float32)),
               "base_ang_vel": ref["ref_root_ang_vel"] + amp * torch.from_numpy(rng.standard_normal((ENVS, 3)).astype(np.float32)),
               "dof_pos": ref["ref_dof_pos"] + 0.3 * amp * torch.from_numpy(rng.standard_normal((ENVS, R)).astype(np.float32)),
               "dof_vel": ref["ref_dof_vel"] + 0.1 * amp * torch.from_numpy(rng.standard_normal((ENVS, R)).astype(np.float32))}
        if step % 7 == 3:
            sim["base_quat"][1] = -sim["base_quat"][1]          # the other hemisphere: the same rotation
        # :249-309 in float32 torch; the w of conj(q) * q_ref for xyzw quaternions is their dot product
        a, b = sim["base_quat"], ref["ref_root_rot"]
        w = a[:, 3] * b[:, 3] + a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]
        err = torch.stack([torch.norm(sim["base_pos"] - ref["ref_root_pos"], dim=1),
                           2.0 * torch.acos(torch.clamp(torch.abs(w), 0.0, 1.0)),
                           torch.norm(sim["base_lin_vel"] - ref["ref_root_vel"], dim=1),
                           torch.norm(sim["base_ang_vel"] - ref["ref_root_ang_vel"], dim=1),
                           torch.norm(sim["dof_pos"] - ref["ref_dof_pos"], dim=1),
                           torch.norm(sim["dof_vel"] - ref["ref_dof_vel"], dim=1)], dim=1)
        term = torch.exp(-err / torch.tensor(SCALES, dtype=torch.float32))
        for k in names:
            rec[k].append(ref[k].numpy().copy())
        for k in sim_names:
            rec[k].append(sim[k].numpy().copy())
        rec["err"].append(err.numpy().copy())
        rec["term"].append(term.numpy().copy())
    for k, v in rec.items():
        out[f"s_{k}"] = np.stack(v)
    out["final_time"] = motion_times.numpy().copy()
    np.savez_compressed(os.path.join(HERE, "g_tracker.npz"), **out)
    print("wrote g_tracker.npz:", {k: v.shape for k, v in out.items() if k.startswith("s_")})


if __name__ == "__main__":
    main(sys.argv)
