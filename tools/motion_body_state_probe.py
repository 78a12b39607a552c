"""Per-body state of the motion library: device-event times of ``gmr_motion_body_state_dev`` next to the
bytes it moves and next to the composition it replaces, in one run.

  library   4 096 clips of 256 frames, G1 shapes (29 dofs, 38 bodies), uniformly random (clip, time)
  per N     in {4 096, 65 536, 1 048 576}: the fused call with all bodies, with a 6-body selection (pelvis, torso, the two ankle-roll
            and the two wrist-yaw links), and ``gmr_motion_sample_dev`` followed by ``gmr_fk_batch_dev`` with rotations on its
            outputs (which gives no velocities)

Each figure is the mean of ``--reps`` repetitions between two device events on one stream, after a warm-up.  Bytes come from the
shapes (the query, two source rows, every output row once); the share is bytes/s over the 8 TB/s HBM peak.  Prints one JSON
document; --out writes it to a file as well.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from motion_library_probe import HBM_PEAK, row, timed  # noqa: E402

SELECTION = ("pelvis", "torso_link", "left_ankle_roll_link", "right_ankle_roll_link", "left_wrist_yaw_link", "right_wrist_yaw_link")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 1048576])
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT, _lib as hip
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    hip.require_gpu()
    km = KinematicsModel(ROBOT_XML_DICT["unitree_g1"])
    fk = km.hip_handle
    ndof, nb = fk.ndof, fk.nbody
    S, T = args.clips, args.frames
    B = S * T
    rng = np.random.default_rng(0)
    st = hip.Stream()
    w = np.cumsum(rng.normal(size=(S, T, 4)) * 0.05, axis=1) + rng.normal(size=(S, 1, 4))
    src = [rng.normal(0, 0.5, size=(B, 3)) + np.array([0.3, -0.2, 0.8]), (w / np.linalg.norm(w, axis=2, keepdims=True)).reshape(B, 4),
           rng.uniform(-1.2, 1.2, size=(B, ndof))]
    bufs = [hip.DeviceBuffer.from_host(a) for a in src]
    del src, w
    lib = MotionLibrary.from_device((np.arange(S + 1) * T).astype(np.int32), np.full(S, 30.0), ndof, 0, *bufs, stream=st)
    st.sync()
    lib.attach_kinematics(km)
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "clips": S, "frames_per_clip": T, "B": B, "ndof": ndof, "nbody": nb,
           "reps": args.reps, "hbm_peak_GB_per_s": HBM_PEAK / 1e9, "selection": list(SELECTION), "N": {}}
    state_row = 12 + 16 + 12 + 12 + 8 * ndof                      # the six arrays of the sampler, one row
    for N in args.sizes:
        d_clip = hip.DeviceBuffer.from_host(rng.integers(0, S, size=N).astype(np.int32))
        d_time = hip.DeviceBuffer.from_host(rng.uniform(0.0, T / 30.0, size=N))
        o = {"root_pos": hip.DeviceBuffer(N * 12), "root_rot": hip.DeviceBuffer(N * 16), "root_vel": hip.DeviceBuffer(N * 12),
             "root_ang_vel": hip.DeviceBuffer(N * 12), "dof_pos": hip.DeviceBuffer(N * ndof * 4), "dof_vel": hip.DeviceBuffer(N * ndof * 4),
             "status": hip.DeviceBuffer(N * 4)}
        body = {"body_pos": hip.DeviceBuffer(N * nb * 12), "body_rot": hip.DeviceBuffer(N * nb * 16), "body_vel": hip.DeviceBuffer(N * nb * 12),
                "body_ang_vel": hip.DeviceBuffer(N * nb * 12)}
        query = N * (12 + 4)                                        # clip, time in; status out
        res = {}
        for name, bodies, nsel in (("all_bodies", None, nb), ("six_bodies", SELECTION, len(SELECTION))):
            t = timed(hip, st, lambda: lib.body_state_dev(N, d_clip, d_time, bodies=bodies, stream=st, **o, **body), args.reps)
            res[name] = dict(row(t, query + N * (3 * state_row + nsel * 52)), queries_per_s=N / t, nsel=nsel)

        def composition():
            lib.sample_dev(N, d_clip, d_time, True, stream=st, **o)
            fk.fk_dev(N, o["root_pos"], o["root_rot"], o["dof_pos"], body["body_pos"], body["body_rot"], None, st)

        t = timed(hip, st, composition, args.reps)
        fk_in = N * (12 + 16 + 4 * ndof)
        res["sample_dev_then_fk_batch_dev"] = dict(row(t, query + N * (3 * state_row + nb * 28) + fk_in), queries_per_s=N / t,
                                                   note="pose only: the composition gives no velocities")
        res["fused_over_composition"] = res["all_bodies"]["us"] / res["sample_dev_then_fk_batch_dev"]["us"]
        res["all_over_six_bodies"] = res["all_bodies"]["us"] / res["six_bodies"]["us"]
        doc["N"][str(N)] = res
        for b in list(o.values()) + list(body.values()) + [d_clip, d_time]:
            b.free()
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
