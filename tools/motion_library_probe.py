"""Motion library on the device: device-event times of its kernels next to the bytes they move.

  fill     B = 2^20 frames (4 096 clips of 256, G1 shapes: 29 dofs, 38 bodies) from the float64 arrays
           ``gmr_postprocess_clips_dev`` leaves -- the fill kernel and the stats kernel together, as one fill enqueues them --
           and, for scale, that post-processing call on the same batch
  sample   N = 4 096 and 65 536 queries with and without ``local_body_pos``, uniformly random (clip, time)

Each figure is the mean of ``--reps`` repetitions between two device events on one stream, after a warm-up.  Byte counts come
from the shapes (every array read or written once; the second pass of the stats kernel is counted too), the share is bytes/s
over the 8 TB/s HBM peak.  Prints one JSON document; --out writes it to a file as well.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes/s, MI355X (8 TB/s HBM3E)


def timed(hip, st, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    st.sync()
    a, b = hip.Event(), hip.Event()
    a.record(st)
    for _ in range(reps):
        fn()
    b.record(st)
    st.sync()
    return a.elapsed_ms(b) * 1e-3 / reps


def row(seconds, nbytes):
    return {"us": seconds * 1e6, "MB": nbytes / 1e6, "GB_per_s": nbytes / seconds / 1e9, "share_of_hbm_peak": nbytes / seconds / HBM_PEAK}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT, _lib as hip
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    hip.require_gpu()
    fk = KinematicsModel(ROBOT_XML_DICT["unitree_g1"]).hip_handle
    ndof, nb, nq = fk.ndof, fk.nbody, fk.ndof + 7
    S, T = args.clips, args.frames
    B = S * T
    rng = np.random.default_rng(0)
    # an IK output to post-process: valid unit quaternions, joint angles in range
    q = np.empty((S, T, nq))
    q[..., :3] = rng.normal(0, 0.5, size=(S, T, 3)) + np.array([0.3, -0.2, 0.8])
    w = np.cumsum(rng.normal(size=(S, T, 4)) * 0.05, axis=1) + rng.normal(size=(S, 1, 4))
    q[..., 3:7] = w / np.linalg.norm(w, axis=2, keepdims=True)
    q[..., 7:] = rng.uniform(-1.2, 1.2, size=(S, T, ndof))
    seg = (np.arange(S + 1) * T).astype(np.int32)
    st = hip.Stream()
    d_q, d_seg = hip.DeviceBuffer.from_host(q), hip.DeviceBuffer.from_host(seg)
    del q, w
    outs = [hip.DeviceBuffer(B * n) for n in (24, 32, ndof * 8, nb * 12)]
    post = lambda: fk.postprocess_clips_dev([(S, T, d_q, None)], d_seg, S, B, *outs, None, True, True, 0.0, st)   # noqa: E731
    t_post = timed(hip, st, post, args.reps)
    lib = MotionLibrary.from_device(seg, np.full(S, 30.0), ndof, nb, *outs, stream=st)
    t_fill = timed(hip, st, lambda: lib.fill_dev(*outs, stream=st), args.reps)
    fill_read = B * (24 + 32 + 8 * ndof + 12 * nb)
    fill_write = B * (12 + 16 + 4 * ndof + 12 * nb + 12 + 12 + 4 * ndof)
    stats_read = 2 * B * (12 + 4 * ndof)
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "clips": S, "frames_per_clip": T, "B": B, "ndof": ndof, "nbody": nb,
           "reps": args.reps, "hbm_peak_GB_per_s": HBM_PEAK / 1e9,
           "fill": dict(row(t_fill, fill_read + fill_write + stats_read), read_MB=fill_read / 1e6, write_MB=fill_write / 1e6,
                        stats_read_MB=stats_read / 1e6, note="fill kernel + stats kernel, as one fill enqueues them"),
           "postprocess_clips_dev_same_batch": {"us": t_post * 1e6}, "sample": {}}
    doc["fill"]["fill_over_post"] = t_fill / t_post
    for N in (4096, 65536):
        clip = rng.integers(0, S, size=N).astype(np.int32)
        time = rng.uniform(0.0, T / 30.0, size=N)
        d_clip, d_time = hip.DeviceBuffer.from_host(clip), hip.DeviceBuffer.from_host(time)
        o = {"root_pos": hip.DeviceBuffer(N * 12), "root_rot": hip.DeviceBuffer(N * 16), "root_vel": hip.DeviceBuffer(N * 12),
             "root_ang_vel": hip.DeviceBuffer(N * 12), "dof_pos": hip.DeviceBuffer(N * ndof * 4), "dof_vel": hip.DeviceBuffer(N * ndof * 4),
             "status": hip.DeviceBuffer(N * 4)}
        d_body = hip.DeviceBuffer(N * nb * 12)
        for body in (False, True):
            kw = dict(o, local_body_pos=d_body) if body else o
            t = timed(hip, st, lambda: lib.sample_dev(N, d_clip, d_time, True, stream=st, **kw), args.reps)
            per_row = 12 + 16 + 12 + 12 + 8 * ndof + (12 * nb if body else 0)
            nbytes = N * (12 + 2 * per_row + per_row + 4)       # the query, two source rows, one output row, the status word
            doc["sample"][f"N{N}_{'with' if body else 'without'}_local_body_pos"] = dict(row(t, nbytes), queries_per_s=N / t)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
