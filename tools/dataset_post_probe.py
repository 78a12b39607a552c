#!/usr/bin/env python3
"""The dataset drivers' post-processing on the device (``gmr_postprocess_clips_dev``) by itself: synthetic but valid qpos of S
ragged clips of up to T frames on the G1, resident in HBM as an IK launch would leave them; device events around ``reps``
calls, mean.  Beside it one float32 FK pass on as many frames and the same clips through the host path
(``dataset.postprocess_clips``) on a sub-sample, extrapolated by frames.  Prints one JSON object.

    python tools/dataset_post_probe.py [S] [T] [reps]          (defaults 4096 256 20; needs an MI355X)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT, _lib, dataset  # noqa: E402

HBM_PEAK_GBS = 8000.0          # HBM3E 8 TB/s spec


def measure(S=4096, T=256, reps=20, host_clips=64, seed=5):
    _lib.require_gpu()
    km = KinematicsModel(ROBOT_XML_DICT["unitree_g1"])
    fk = km.hip_handle
    nb, ndof, nq = fk.nbody, fk.ndof, fk.ndof + 7
    rng = np.random.default_rng(seed)
    lens = rng.integers(max(T // 4, 1), T + 1, size=S).astype(np.int32)
    lens[0] = T
    q = np.empty((S, T, nq))
    q[..., :3] = rng.standard_normal((S, T, 3), dtype=np.float32) * 0.5 + np.array([0.0, 0.0, 0.8])
    quat = rng.standard_normal((S, T, 4), dtype=np.float32).astype(np.float64)
    q[..., 3:7] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    q[..., 7:] = rng.uniform(-0.7, 0.7, size=(S, T, ndof)).astype(np.float32)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    B = int(seg[-1])
    d_q, d_len, d_seg = _lib.DeviceBuffer.from_host(q), _lib.DeviceBuffer.from_host(lens), _lib.DeviceBuffer.from_host(seg)
    d_rp, d_rr, d_dp, d_lb = (_lib.DeviceBuffer(B * n) for n in (24, 32, ndof * 8, nb * 12))
    d_low = _lib.DeviceBuffer(S * 4)
    st = _lib.Stream()
    e0, e1 = _lib.Event(), _lib.Event()

    def timed(fn, n):
        for _ in range(2):
            fn()
        e0.record(st)
        for _ in range(n):
            fn()
        e1.record(st)
        st.sync()
        return e0.elapsed_ms(e1) / n

    def post(height, origin):
        fk.postprocess_clips_dev([(S, T, d_q, d_len)], d_seg, S, B, d_rp, d_rr, d_dp, d_lb, d_low, height, origin, 0.0, st)

    ms_full = timed(lambda: post(True, True), reps)
    ms_plain = timed(lambda: post(False, False), reps)
    # the float32 entry point on as many frames (positions only): what one FK pass costs when its inputs are float32 arrays
    d_f = [_lib.DeviceBuffer(B * n) for n in (12, 16, ndof * 4)]
    for b in d_f:
        b.zero(st)
    ms_fk32 = timed(lambda: fk.fk_dev(B, d_f[0], d_f[1], d_f[2], d_lb, None, None, st), reps)
    post(True, True)
    st.sync()
    per = (1 << 20) / B
    row = nq * 8
    # bytes the algorithm moves per frame: the row map (12 written, 8 read by each of its readers + 4), the local FK pass
    # (dofs in, positions out), the gather (row in, row out) and -- with the height adjustment -- the world pass (row in,
    # positions to scratch and back for the per-clip minimum)
    bytes_plain = B * (12 + 8 * 2 + 4 + ndof * 8 + nb * 12 + 2 * row)
    bytes_full = bytes_plain + B * (8 + row + 2 * nb * 12)
    # the host path on the first clips (every clip costs the same per frame: extrapolated by frames)
    nh = min(host_clips, S)
    qh = d_q.to_host((nh, T, nq), np.float64)
    clips = [qh[i, : lens[i]] for i in range(nh)]
    dataset.postprocess_clips(clips, km, [30.0] * nh)
    t0 = time.perf_counter()
    host = dataset.postprocess_clips(clips, km, [30.0] * nh)
    t_host = time.perf_counter() - t0
    fh = int(seg[nh])
    rp = d_rp.to_host((fh, 3), np.float64)
    lb = d_lb.to_host((fh, nb, 3), np.float32)
    same = bool(np.array_equal(rp.view(np.uint64), np.concatenate([m["root_pos"] for m in host]).view(np.uint64)) and
                np.array_equal(lb.view(np.uint32), np.concatenate([m["local_body_pos"] for m in host]).view(np.uint32)))
    return {"workload": f"post-processing of S={S} clips x up to T={T} frames ({B} frames) of the G1, qpos resident in HBM; device events "
                        f"around n={reps} calls after 2 warm-up calls, mean",
            "unit": "ms per 2^20 frames", "n": reps, "frames": B,
            "device_both_adjustments": ms_full * per, "device_no_adjustment": ms_plain * per,
            "fk_f32_positions_only": ms_fk32 * per,
            "algorithmic_bytes": {"both_adjustments": int(bytes_full), "no_adjustment": int(bytes_plain)},
            "fraction_of_hbm_peak": {"both_adjustments": bytes_full / (ms_full * 1e-3) / (HBM_PEAK_GBS * 1e9),
                                     "no_adjustment": bytes_plain / (ms_plain * 1e-3) / (HBM_PEAK_GBS * 1e9)},
            "host_path": {"ms_per_2p20_frames": t_host * 1e3 * (1 << 20) / fh, "measured_on": f"the first {nh} clips ({fh} frames), "
                          "one call after one warm-up call, wall clock; extrapolated by frames", "bytes_equal_to_device": same}}


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:4]]
    print(json.dumps(measure(*a)))
