#!/usr/bin/env python3
"""Generate tests/golden/g_proprio.npz by RUNNING the reference's own ``quat_rotate_inverse``
(``general_motion_retargeting/torch_utils.py:78-87``) and ``apply_randomization`` (``booster_gym/utils/utils.py:5-30``) in float32 CPU
torch the way its environment drives them after the physics of a step (``booster_gym/envs/t1.py:463-473, 554-557, 574-603, 622-694,
492-494``; the environment itself needs a simulator and cannot be imported): a scripted episode of six environments, 40 steps of dt =
0.02 and R = 23 dofs with seeded root and dof states and two scripted resets.  Stored per step: the inputs, the three rotated vectors,
the two filtered velocities, the clean privileged block and (for the first eight steps) observation row, the fourteen penalties with the sum of the absolute
summands behind every one of them, and the three termination flags -- all evaluated here in float32 torch with the formulas restated
below --, plus one call of ``apply_randomization`` per distribution with the noise it drew.  Only numbers are stored
(``np.savez_compressed``; loadable with allow_pickle=False); no line of the reference is copied.

    python tests/golden/make_proprio_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ENVS, STEPS, R, C, DT = 6, 40, 23, 5, 0.02
FILTER_WEIGHT = 0.1
NORM = {"gravity": 1.0, "lin_vel": 1.0, "ang_vel": 1.0, "dof_pos": 1.0, "dof_vel": 0.1}
SOFT = (0.9, 0.8, 0.85)                  # position, velocity, torque
HEIGHT_TARGET, TERMINATE_VEL, TERMINATE_HEIGHT, MAX_STEPS = 0.68, 50.0, 0.3, 30
OBS_STEPS = 8
RESETS = ((11, (1, 4)), (27, (0, 4, 5)))     # before that step, those environments
NOISE = {"gaussian": {"distribution": "gaussian", "operation": "additive", "range": [0.02, 0.05]},
         "uniform": {"distribution": "uniform", "operation": "scaling", "range": [0.9, 1.15]}}


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    rotate = load(os.path.join(ref, "general_motion_retargeting", "torch_utils.py"), "reference_torch_utils").quat_rotate_inverse
    randomize = load(os.path.join(ref, "booster_gym", "utils", "utils.py"), "reference_utils").apply_randomization
    rng = np.random.default_rng(20251018)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    default = f32(rng.uniform(-0.4, 0.4, R))
    lim = np.sort(rng.uniform(-2.0, 2.0, (R, 2)), axis=1)
    lim[:, 1] += 0.5
    pos_lim, vel_lim, tq_lim = f32(lim), f32(rng.uniform(3.0, 12.0, R)), f32(rng.uniform(10.0, 60.0, R))
    gravity = torch.tensor([0.0, 0.0, -1.0]).repeat(ENVS, 1)
    filt_lin, filt_ang = torch.zeros(ENVS, 3), torch.zeros(ENVS, 3)
    last_root_vel, last_actions, last_dof_vel = torch.zeros(ENVS, 6), torch.zeros(ENVS, R), torch.zeros(ENVS, R)
    names = ("root_states", "dof_pos", "dof_vel", "actions", "torques", "extra", "ground", "episode_steps", "base_lin_vel", "base_ang_vel",
             "projected_gravity", "filtered_lin_vel", "filtered_ang_vel", "obs", "priv", "term", "abs_sum", "done")
    rec = {k: [] for k in names}
    reset_roots = {}
    steps = torch.zeros(ENVS, dtype=torch.int32)
    for step in range(STEPS):
        # the simulator: a seeded state per step
        quat = rng.standard_normal((ENVS, 4))
        quat /= np.linalg.norm(quat, axis=1, keepdims=True)
        root = f32(np.concatenate([rng.uniform(-3, 3, (ENVS, 2)), rng.uniform(0.2, 0.9, (ENVS, 1)), quat,
                                   rng.normal(0, 1.5, (ENVS, 3)), rng.normal(0, 2.0, (ENVS, 3))], axis=1))
        if step % 13 == 6:
            root[3, 7:13] *= 4.0                            # past the velocity threshold
        q, qd = f32(rng.uniform(-2.2, 2.7, (ENVS, R))), f32(rng.normal(0, 6.0, (ENVS, R)))
        act, tau = f32(np.clip(rng.normal(0, 0.8, (ENVS, R)), -1, 1)), f32(rng.normal(0, 25.0, (ENVS, R)))
        extra, ground = f32(rng.uniform(-1, 1, (ENVS, C))), f32(rng.uniform(-0.1, 0.3, ENVS))
        for s, envs in RESETS:
            if s == step:                                   # :310-313
                ids = torch.tensor(envs)
                rows = f32(rng.normal(0, 1.0, (len(envs), 13)))
                reset_roots[step] = rows.numpy().copy()
                last_root_vel[ids] = rows[:, 7:13]
                filt_lin[ids] = 0.0
                filt_ang[ids] = 0.0
                steps[ids] = 0
        steps += 1
        # :463-473
        base_lin, base_ang, proj = rotate(root[:, 3:7], root[:, 7:10]), rotate(root[:, 3:7], root[:, 10:13]), rotate(root[:, 3:7], gravity)
        filt_lin = base_lin * FILTER_WEIGHT + filt_lin * (1.0 - FILTER_WEIGHT)
        filt_ang = base_ang * FILTER_WEIGHT + filt_ang * (1.0 - FILTER_WEIGHT)
        height = root[:, 2] - ground
        # :554-557
        done = ((root[:, 7:13].square().sum(dim=-1) > TERMINATE_VEL).int() + 2 * (height < TERMINATE_HEIGHT).int()
                + 4 * (steps > np.ceil(MAX_STEPS)).int())
        # :622-625, :631-694: (summands, reduced) per term
        lower = pos_lim[:, 0] + 0.5 * (1 - SOFT[0]) * (pos_lim[:, 1] - pos_lim[:, 0])
        upper = pos_lim[:, 1] - 0.5 * (1 - SOFT[0]) * (pos_lim[:, 1] - pos_lim[:, 0])
        summands = [torch.square(filt_lin[:, 2:3]), torch.square(base_ang[:, :2]), torch.square(proj[:, :2]), torch.square(tau), torch.square(qd),
                    torch.square((last_dof_vel - qd) / DT), torch.square((last_root_vel - root[:, 7:13]) / DT), torch.square(last_actions - act),
                    ((q < lower) | (q > upper)).float(), (torch.abs(qd) - vel_lim * SOFT[1]).clip(min=0.0, max=1.0),
                    (torch.abs(tau) - tq_lim * SOFT[2]).clip(min=0.0), torch.square(tau / tq_lim).clip(max=1.0), (tau * qd).clip(min=0.0),
                    torch.square(height - HEIGHT_TARGET).unsqueeze(-1)]
        term = torch.stack([torch.sum(x, dim=-1) for x in summands], dim=1)
        abs_sum = torch.stack([torch.sum(x.double().abs(), dim=-1) for x in summands], dim=1)
        # :580-597 without noise: apply_randomization with no spec hands its tensor back
        obs = torch.cat((randomize(proj, None) * NORM["gravity"], randomize(base_ang, None) * NORM["ang_vel"], extra,
                         randomize(q - default, None) * NORM["dof_pos"], randomize(qd, None) * NORM["dof_vel"], act), dim=-1)
        priv = torch.cat((randomize(base_lin, None) * NORM["lin_vel"], randomize(height, None).unsqueeze(-1)), dim=-1)
        for k, v in (("root_states", root), ("dof_pos", q), ("dof_vel", qd), ("actions", act), ("torques", tau), ("extra", extra), ("ground", ground),
                     ("episode_steps", steps), ("base_lin_vel", base_lin), ("base_ang_vel", base_ang), ("projected_gravity", proj),
                     ("filtered_lin_vel", filt_lin), ("filtered_ang_vel", filt_ang), ("obs", obs), ("priv", priv), ("term", term),
                     ("abs_sum", abs_sum), ("done", done)):
            rec[k].append(v.numpy().copy())
        # :492-494
        last_actions, last_dof_vel, last_root_vel = act.clone(), qd.clone(), root[:, 7:13].clone()
    out = {f"s_{k}": np.stack(v) for k, v in rec.items()}
    out["s_obs"], out["s_abs_sum"] = out["s_obs"][:OBS_STEPS], out["s_abs_sum"].astype(np.float32)      # (the file stays under 200 KB)
    out.update({"dt": np.array(DT), "filter_weight": np.array(FILTER_WEIGHT), "soft": np.array(SOFT), "default_dof_pos": default.numpy(),
                "dof_pos_limits": pos_lim.numpy(), "dof_vel_limits": vel_lim.numpy(), "torque_limits": tq_lim.numpy(),
                "norm": np.array([NORM[k] for k in ("gravity", "lin_vel", "ang_vel", "dof_pos", "dof_vel")]),
                "scalars": np.array([HEIGHT_TARGET, TERMINATE_VEL, TERMINATE_HEIGHT, MAX_STEPS]),
                "reset_steps": np.array([s for s, _ in RESETS]), "final_last_root_vel": last_root_vel.numpy(),
                "final_last_actions": last_actions.numpy(), "final_last_dof_vel": last_dof_vel.numpy()})
    for (s, envs) in RESETS:
        out[f"reset{s}_envs"], out[f"reset{s}_roots"] = np.array(envs, dtype=np.int32), reset_roots[s]
    # the reference's noise application on its own draws: x, the unit noise it drew, the result
    torch.manual_seed(7)
    x = f32(rng.uniform(-2, 2, (ENVS, R)))
    for name, spec in NOISE.items():
        res, unit = randomize(x, spec, return_noise=True)
        out[f"noise_{name}_range"], out[f"noise_{name}_unit"], out[f"noise_{name}_result"] = np.array(spec["range"]), unit.numpy(), res.numpy()
    out["noise_x"] = x.numpy()
    # the rotation alone on many unit quaternions (the bound of the host test was measured on such a set)
    big_q = rng.standard_normal((400, 4))
    big_q /= np.linalg.norm(big_q, axis=1, keepdims=True)
    big_v = f32(rng.normal(0, 3.0, (400, 3)))
    out["rot_q"], out["rot_v"], out["rot_out"] = np.float32(big_q), big_v.numpy(), rotate(f32(big_q), big_v).numpy()
    np.savez_compressed(os.path.join(HERE, "g_proprio.npz"), **out)
    print("wrote g_proprio.npz:", {k: v.shape for k, v in out.items() if k.startswith("s_")})


if __name__ == "__main__":
    main(sys.argv)
