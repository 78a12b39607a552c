#!/usr/bin/env python3
"""Generate tests/golden/g_feet.npz by RUNNING the reference's own ``Terrain.terrain_heights`` (``booster_gym/utils/terrain.py:101-121``) and
``quat_rotate`` (``general_motion_retargeting/torch_utils.py:66-75``) in float32 CPU torch the way its environment drives them for the feet
(``booster_gym/envs/t1.py:474-478, 495, 529-549, 553, 585-586, 627-629, 696-730``; the environment itself needs a simulator and cannot be
imported): a scripted episode of six environments, 40 steps of dt = 0.02 with 11 rigid bodies and the T1's four edge points on a 23 x 17
height field with a border of 3 pixels.  ``terrain.py`` imports isaacgym, which is not installed: empty stand-in modules take its place in
``sys.modules``, the instance is made with ``object.__new__`` and only the attributes ``terrain_heights`` reads are set.  The roll and yaw of
isaacgym's ``get_euler_xyz`` are restated below (isaacgym is not there to run).  Stored per step: the inputs, the edge points the reference's
rotation gives, the heights the reference's function gives under them and under the root, the contact flags, the angles, the gait clock and
its two columns, the eight terms and the termination flag -- all evaluated here in float32 torch with the formulas restated below --, plus a
set of points of their own for the heights alone: on cell lines, on the last valid cell, inside cells.  Only numbers are stored
(``np.savez_compressed``; loadable with allow_pickle=False).  The reference's two functions are loaded and run, never restated; what the
environment does around them is written here in this project's own words, one foot at a time, with the reference's line numbers beside
each part.

The generator asserts that no edge clearance lies within 1e-5 of the contact threshold and no final angle within 1e-3 of +-pi (or a raw
one of the 0 / 2 pi seam), so that a test may expect the flags exactly and bound the angles; the seed is one for which both hold.

    python tests/golden/make_feet_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ENVS, STEPS, NB, DT = 6, 40, 11, 0.02
NX, NY, BORDER, HS, VS = 23, 17, 3, 0.1, 0.005
FEET = (4, 9)
EDGES = [[0.1215, 0.05, -0.03], [0.1215, -0.05, -0.03], [-0.1015, 0.05, -0.03], [-0.1015, -0.05, -0.03]]      # T1.yaml:79-82
TERMINATION, PENALIZED = (0, 3), (1, 2, 5, 7)
THRESHOLD, CLEARANCE, DISTANCE_REF, SWING_PERIOD = 1.0, 0.01, 0.2, 0.2
SEED = 20251026


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def euler_roll_yaw(q):
    """roll and yaw of isaacgym's get_euler_xyz for xyzw quaternions, restated"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    roll = torch.atan2(2.0 * (w * x + y * z), w * w - x * x - y * y + z * z)
    yaw = torch.atan2(2.0 * (w * z + x * y), w * w + x * x - y * y - z * z)
    return torch.remainder(roll, 2 * np.pi), torch.remainder(yaw, 2 * np.pi)


def wrap(a):
    """an angle brought into [-pi, pi): + pi, the remainder by 2 pi, - pi"""
    return torch.remainder(a + torch.pi, 2 * torch.pi) - torch.pi


def quat_of(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    for name in ("isaacgym", "isaacgym.gymapi", "isaacgym.terrain_utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["isaacgym"].gymapi, sys.modules["isaacgym"].terrain_utils = sys.modules["isaacgym.gymapi"], sys.modules["isaacgym.terrain_utils"]
    Terrain = load(os.path.join(ref, "booster_gym", "utils", "terrain.py"), "reference_terrain").Terrain
    rotate = load(os.path.join(ref, "general_motion_retargeting", "torch_utils.py"), "reference_torch_utils").quat_rotate
    rng = np.random.default_rng(SEED)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    field = rng.integers(-20, 60, (NX, NY)).astype(np.int16)
    field[:BORDER], field[-BORDER:], field[:, :BORDER], field[:, -BORDER:] = 0, 0, 0, 0
    ter = object.__new__(Terrain)
    ter.type, ter.device = "trimesh", "cpu"
    ter.border_pixels, ter.horizontal_scale, ter.vertical_scale, ter.height_field_raw = BORDER, HS, VS, field
    x_hi, y_hi = (NX - 1 - BORDER) * HS, (NY - 1 - BORDER) * HS          # the world extent of the field: [-BORDER HS, x_hi] x [-BORDER HS, y_hi]
    # ---- the heights alone: inside cells, on cell lines, on the corners of the first and of the last valid cell
    inside = np.stack([rng.uniform(-BORDER * HS, x_hi - 1e-3, 300), rng.uniform(-BORDER * HS, y_hi - 1e-3, 300), rng.normal(0, 1, 300)], axis=1)
    on_x = np.stack([(rng.integers(0, NX - 1, 30) - BORDER) * HS, rng.uniform(-BORDER * HS, y_hi - 1e-3, 30), np.zeros(30)], axis=1)
    on_y = np.stack([rng.uniform(-BORDER * HS, x_hi - 1e-3, 30), (rng.integers(0, NY - 1, 30) - BORDER) * HS, np.zeros(30)], axis=1)
    lines = np.concatenate([on_x, on_y])
    eps = 1e-4
    corners = np.array([[-BORDER * HS, -BORDER * HS, 0], [x_hi - HS, y_hi - HS, 0], [x_hi - eps, y_hi - eps, 0], [x_hi - HS, y_hi - eps, 0],
                        [x_hi - eps, -BORDER * HS, 0], [0.0, 0.0, 0], [0.5, 0.7, 0]])
    points = f32(np.concatenate([inside, lines, corners]))
    # (every point must lie inside the field for the reference: its cell's far corner exists)
    px = np.floor(BORDER + points[:, 0].numpy() / HS).astype(int)
    py = np.floor(BORDER + points[:, 1].numpy() / HS).astype(int)
    assert (px >= 0).all() and (px + 1 <= NX - 1).all() and (py >= 0).all() and (py + 1 <= NY - 1).all()
    point_heights = ter.terrain_heights(points)
    assert point_heights.dtype == torch.float32 and len(np.unique(point_heights.numpy())) > 150

    edges = f32(EDGES)
    E = len(EDGES)
    names = ("body_pos", "body_rot", "root_states", "contact_forces", "episode_steps", "gait_frequency", "feet_pos", "feet_roll", "feet_yaw",
             "edge_pos", "edge_height", "feet_contact", "ground", "gait_process", "gait", "term", "done")
    rec = {k: [] for k in names}
    last_feet_pos, gait_process = torch.zeros(ENVS, 2, 3), torch.zeros(ENVS)
    steps = torch.zeros(ENVS, dtype=torch.int32)
    gait_frequency = f32(rng.uniform(1.0, 2.5, ENVS))
    gait_frequency[2] = 0.0                                  # standing: no gait
    least_clear, least_angle = np.inf, np.inf
    feet_xy = np.stack([rng.uniform(0.1, x_hi - 0.3, (ENVS, 2)), rng.uniform(0.1, y_hi - 0.3, (ENVS, 2))], axis=-1)
    for step in range(STEPS):
        # the simulator: seeded rigid bodies, the two feet walking over the field near its surface
        body_pos = rng.uniform(-1, 2, (ENVS, NB, 3))
        quat = rng.standard_normal((ENVS, NB, 4))
        quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
        feet_xy = np.clip(feet_xy + rng.normal(0, 0.02, (ENVS, 2, 2)), [0.05, 0.05], [x_hi - 0.2, y_hi - 0.2])
        under = ter.terrain_heights(f32(feet_xy.reshape(-1, 2))).numpy().reshape(ENVS, 2)
        body_pos[:, FEET, :2] = feet_xy
        body_pos[:, FEET, 2] = under + 0.03 + rng.uniform(-0.03, 0.06, (ENVS, 2))
        heading = rng.uniform(-3.0, 3.0, (ENVS, 1))
        quat[:, FEET] = quat_of(rng.uniform(-0.25, 0.25, (ENVS, 2)), rng.uniform(-0.25, 0.25, (ENVS, 2)), heading + rng.uniform(-0.4, 0.4, (ENVS, 2)))
        if step % 9 == 4:
            quat[1, FEET[1]] = quat_of(0.1, -0.05, heading[1, 0] + 3.3)          # |yaw_1 - yaw_0| beyond pi
        root_quat = quat_of(rng.uniform(-0.2, 0.2, ENVS), rng.uniform(-0.2, 0.2, ENVS), heading[:, 0] + rng.uniform(-0.3, 0.3, ENVS))
        root = f32(np.concatenate([feet_xy.mean(axis=1), rng.uniform(0.5, 0.8, (ENVS, 1)), root_quat, rng.normal(0, 1, (ENVS, 6))], axis=1))
        forces = rng.normal(0, 0.6, (ENVS, NB, 3))
        forces[rng.uniform(size=(ENVS, NB)) < 0.5] = 0.0
        body_pos, body_rot, forces = f32(body_pos), f32(quat), f32(forces)
        if step in (13, 29):
            steps[[1, 4]] = 0                                # an episode reset: nothing of the feet state is reset (:310-313)
        # ---- what the environment computes for the feet, one foot at a time, in float32 torch; the reference's line numbers beside each part
        steps += 1                                                                             # :476
        moving = gait_frequency > 1.0e-8
        gait_process = torch.fmod(gait_process + DT * gait_frequency, 1.0)                     # :478
        turn = 2 * torch.pi * gait_process
        gait = torch.stack([torch.cos(turn), torch.sin(turn)], dim=1) * moving.float().unsqueeze(1)          # :585-586
        hard = torch.norm(forces, dim=-1) > THRESHOLD                                          # [ENVS, NB]
        done, collision = hard[:, TERMINATION].any(dim=1), hard[:, PENALIZED].sum(dim=1)       # :553, :629
        ground = ter.terrain_heights(root[:, 0:3])                                             # :555, :624 (the reference's function)
        _, base_yaw = euler_roll_yaw(root[:, 3:7])
        pos, rolls, yaws, raws, corners, under, touching, speed2, rise2 = [], [], [], [], [], [], [], [], []
        for f, body in enumerate(FEET):
            p, q = body_pos[:, body], body_rot[:, body]                                        # :530-531
            raw_roll, raw_yaw = euler_roll_yaw(q)                                              # :532
            rolls.append(wrap(raw_roll))                                                       # :533
            yaws.append(wrap(raw_yaw))                                                         # :534
            raws += [raw_roll, raw_yaw]
            # every edge point of the foot: the reference's quat_rotate on (environment, edge) rows, then its terrain_heights (:535-545)
            c = p.repeat_interleave(E, dim=0) + rotate(q.repeat_interleave(E, dim=0), edges.repeat(ENVS, 1))
            h = ter.terrain_heights(c)
            clear = c[:, 2] - h
            least_clear = min(least_clear, float((clear.double() - CLEARANCE).abs().min()))
            touching.append((clear < CLEARANCE).view(ENVS, E).any(dim=1))                      # :544-549
            corners.append(c.view(ENVS, E, 3))
            under.append(h.view(ENVS, E))
            v = (last_feet_pos[:, f] - p) / DT
            speed2.append(torch.square(v).sum(dim=-1))
            rise2.append(torch.square(v[:, 2]))
            pos.append(p)
        feet_pos, feet_roll, feet_yaw = torch.stack(pos, dim=1), torch.stack(rolls, dim=1), torch.stack(yaws, dim=1)
        feet_contact = torch.stack(touching, dim=1)
        edge_pos, edge_height = torch.stack(corners, dim=1), torch.stack(under, dim=1)
        split = feet_yaw[:, 1] - feet_yaw[:, 0]
        pi32 = torch.tensor(np.pi, dtype=torch.float32)
        middle = (feet_yaw[:, 0] + feet_yaw[:, 1]) / 2 + torch.where(split.abs() > torch.pi, pi32, torch.zeros(()))     # :716
        yaw_diff, yaw_off = wrap(split), wrap(base_yaw - middle)                               # :713, :717
        gap = feet_pos[:, 1] - feet_pos[:, 0]
        across = (torch.cos(base_yaw) * gap[:, 1] - torch.sin(base_yaw) * gap[:, 0]).abs()     # :721-724
        airborne = [((gait_process - c).abs() < 0.5 * SWING_PERIOD) & moving for c in (0.25, 0.75)]          # :728-729
        term = torch.stack([collision.float(),
                            (speed2[0] * feet_contact[:, 0].float() + speed2[1] * feet_contact[:, 1].float()) * (steps > 1).float(),       # :698-704
                            rise2[0] + rise2[1],                                               # :707
                            torch.square(feet_roll[:, 0]) + torch.square(feet_roll[:, 1]),     # :710
                            torch.square(yaw_diff), torch.square(yaw_off),
                            (DISTANCE_REF - across).clamp(min=0.0, max=0.1),                   # :725
                            (airborne[0] & ~feet_contact[:, 0]).float() + (airborne[1] & ~feet_contact[:, 1]).float()], dim=1)             # :730
        wrapped = torch.cat([feet_roll.reshape(-1), feet_yaw.reshape(-1), yaw_diff, yaw_off, split]).double()
        raw = torch.cat(raws + [base_yaw]).double()
        least_angle = min(least_angle, float((wrapped.abs() - np.pi).abs().min()), float(torch.minimum(raw, 2 * np.pi - raw).min()))
        for k, v in (("body_pos", body_pos), ("body_rot", body_rot), ("root_states", root), ("contact_forces", forces), ("episode_steps", steps),
                     ("gait_frequency", gait_frequency), ("feet_pos", feet_pos), ("feet_roll", feet_roll), ("feet_yaw", feet_yaw),
                     ("edge_pos", edge_pos), ("edge_height", edge_height), ("feet_contact", feet_contact),
                     ("ground", ground), ("gait_process", gait_process), ("gait", gait), ("term", term), ("done", done)):
            rec[k].append(v.numpy().copy())
        # :495
        last_feet_pos = feet_pos.clone()
    assert least_clear > 1e-5, f"an edge clearance lies {least_clear:.2e} from the threshold: choose another seed"
    assert least_angle > 1e-3, f"an angle lies {least_angle:.2e} from a seam: choose another seed"
    out = {f"s_{k}": np.stack(v) for k, v in rec.items()}
    contact, term = out["s_feet_contact"], out["s_term"]
    assert 0.2 < contact.mean() < 0.8 and out["s_done"].any() and not out["s_done"].all() and (term[:, :, 0] > 0).any() and (term[:, :, 7] > 0).any()
    assert (term[:, :, 6] > 0).any() and (np.abs(out["s_feet_yaw"][:, :, 1] - out["s_feet_yaw"][:, :, 0]) > np.pi).any()
    out.update({"dt": np.array(DT), "field": field, "terrain": np.array([HS, VS, BORDER]), "feet_body": np.array(FEET, dtype=np.int32),
                "edge_pos": edges.numpy(), "termination_body": np.array(TERMINATION, dtype=np.int32), "penalized_body": np.array(PENALIZED, dtype=np.int32),
                "scalars": np.array([THRESHOLD, CLEARANCE, DISTANCE_REF, SWING_PERIOD]), "t_points": points.numpy(), "t_heights": point_heights.numpy(),
                "final_last_feet_pos": last_feet_pos.numpy(), "final_gait_process": gait_process.numpy(),
                "margins": np.array([least_clear, least_angle])})
    np.savez_compressed(os.path.join(HERE, "g_feet.npz"), **out)
    print("wrote g_feet.npz:", {k: v.shape for k, v in out.items() if k.startswith("s_")}, "margins", least_clear, least_angle)


if __name__ == "__main__":
    main(sys.argv)
