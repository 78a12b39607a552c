#!/usr/bin/env python3
"""Generate tests/golden/g_motion.npz by RUNNING the reference's training-side loader
(``booster_gym/utils/motion_loader.py``, CPU torch + scipy) on seeded synthetic motion pkl files.  This pins row N3 of
SURVEY.md section 8a beyond the schema: ``_compute_motion_stats`` (:101-113), ``_compute_derivatives`` (:120-149) and
``get_motion_state`` (:151-247).

Three clips -- 2 / 37 / 240 frames at 30 / 50 / 120 fps with 29 / 23 / 29 dofs -- whose root quaternion tracks contain a
hemisphere flip, runs of near-identical rotations (dot > 0.9995: the normalised-lerp branch) and a step of more than 90 degrees.
The middle clip is written in the list-valued "training compatible" pkl variant, the others hold ndarrays.  Queries: exact frame
times, mid-frame times, the last interval and times beyond the end, with loop on and off, and negative times with loop on.

Only numbers are stored (``np.savez_compressed``; loadable with allow_pickle=False); no line of the loader is copied.

    python tests/golden/make_motion_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import importlib.util
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CLIPS = ((2, 30, 29), (37, 50, 23), (240, 120, 29))     # frames, fps, ndof
NBODY = 5


def quat_xyzw(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def make_clip(rng, T, fps, ndof):
    t = np.arange(T) / fps
    root_pos = np.stack([0.8 * t + 0.05 * np.sin(3 * t), 0.3 * np.sin(1.3 * t), 0.78 + 0.04 * np.cos(5 * t)], axis=1)
    root_pos += 1e-3 * rng.standard_normal(root_pos.shape)
    dof_pos = 0.6 * np.sin(np.outer(t, rng.uniform(0.5, 6.0, ndof)) + rng.uniform(0, 6.28, ndof)) + 0.01 * rng.standard_normal((T, ndof))
    q = quat_xyzw(rng.standard_normal(3), rng.uniform(0.2, 1.0))
    rot = []
    for i in range(T):
        if i % 12 == 5:
            step = quat_xyzw(rng.standard_normal(3), rng.uniform(1.7, 2.6))        # more than 90 degrees in one frame
        elif (i // 6) % 2 == 0:
            step = quat_xyzw(rng.standard_normal(3), rng.uniform(1e-4, 2e-2))      # near-identical: dot > 0.9995
        else:
            step = quat_xyzw(rng.standard_normal(3), rng.uniform(0.08, 0.5))
        q = qmul(step, q)
        q = q / np.linalg.norm(q)
        rot.append(-q if (i // 4) % 3 == 1 else q)                                   # hemisphere flips along the track
    local_body_pos = rng.standard_normal((T, NBODY, 3)).astype(np.float32)
    return {"fps": fps, "root_pos": root_pos, "root_rot": np.array(rot), "dof_pos": dof_pos, "local_body_pos": local_body_pos,
            "link_body_list": [f"b{k}" for k in range(NBODY)]}


def query_times(rng, T, fps):
    dur, dt = T / fps, 1.0 / fps
    frames = sorted(set([0, 1, T // 2, T - 2, T - 1]) & set(range(T)))
    times = [k / fps for k in frames]
    times += [(k + f) / fps for k in range(max(T - 1, 1)) for f in rng.uniform(0.05, 0.95, 2)][:200]
    times += [(T - 1 + f) / fps for f in (0.25, 0.5, 0.9)]
    times += [dur - dt, dur + 0.37, 3 * dur + 0.4 * dt, 17.123]
    return [float(x) for x in times]


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    path = os.path.join(ref, "booster_gym", "utils", "motion_loader.py")
    spec = importlib.util.spec_from_file_location("reference_motion_loader", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(20250607)
    out = {"nclip": np.array(len(CLIPS)), "nbody": np.array(NBODY)}
    with tempfile.TemporaryDirectory() as tmp:
        for c, (T, fps, ndof) in enumerate(CLIPS):
            m = make_clip(rng, T, fps, ndof)
            f = os.path.join(tmp, f"clip{c}.pkl")
            with open(f, "wb") as fh:
                if c == 1:      # lists + protocol 2 ("training compatible"); its local_body_pos stays an array, as the loader needs
                    pickle.dump({k: (v.tolist() if isinstance(v, np.ndarray) and k != "local_body_pos" else v) for k, v in m.items()},
                                fh, protocol=2)
                else:
                    pickle.dump(m, fh)
            for k in ("root_pos", "root_rot", "dof_pos", "local_body_pos"):
                out[f"c{c}_{k}"] = m[k]
            out[f"c{c}_fps"] = np.array(float(fps))
            ld = mod.MotionLoader(f, device="cpu", loop=True)
            for k in ("root_vel", "root_ang_vel", "dof_vel"):
                out[f"c{c}_{k}"] = getattr(ld, k).numpy()
            out[f"c{c}_stats"] = np.stack([np.concatenate([getattr(ld, f"root_pos_{s}").numpy(), getattr(ld, f"dof_pos_{s}").numpy()])
                                           for s in ("mean", "std", "min", "max")])
            times = query_times(rng, T, fps)
            q_time, q_loop, rows = [], [], {k: [] for k in ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel")}
            for loop in (True, False):
                ld.loop = loop
                for tm in times + ([-0.3 / fps, -2.5 * T / fps - 0.01] if loop else []):
                    st = ld.get_motion_state(tm)
                    q_time.append(tm)
                    q_loop.append(loop)
                    for k in rows:
                        rows[k].append(st[k].numpy())
            out[f"c{c}_q_time"], out[f"c{c}_q_loop"] = np.array(q_time), np.array(q_loop)
            for k, v in rows.items():
                out[f"c{c}_q_{k}"] = np.stack(v)
            # one run with a time offset (the wrapper adds it before anything else, :162)
            ld.loop, ld.motion_time_offset = True, 0.123
            st = ld.get_motion_state(0.2)
            out[f"c{c}_offset_root_pos"] = st["root_pos"].numpy()
    np.savez_compressed(os.path.join(HERE, "g_motion.npz"), **out)
    print("wrote g_motion.npz:", {k: v.shape for k, v in out.items() if k.startswith("c1_")})


if __name__ == "__main__":
    main(sys.argv)
