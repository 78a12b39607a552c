#!/usr/bin/env python3
"""gmr_bvh_frames_dev alone: ragged G1 clips resident in device memory, mean of 20 calls between device events.

    python tools/bvh_frames_probe.py [--out FILE]

Two batches on LAFAN1's skeleton (22 joints, 69 doubles per row, the 14 bodies of bvh_to_g1): 2 400 clips of 80 .. 420
frames (the shape of tools/dataset_probe.py) and 77 long clips (LAFAN1's shape: up to 9 855 frames).  Reports ms per call,
ms per 2^20 frames and the fraction of the HBM roof on the algorithmic traffic of 552 B in + 784 B out per frame.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12        # B/s, spec (MI355X)


def batch(name, lens, seed):
    from general_motion_retargeting_amd import GeneralMotionRetargeting, _lib
    from general_motion_retargeting_amd.utils import lafan1
    raw = lafan1.read_bvh_raw(os.path.join(ROOT, "tests", "golden", "synthetic.bvh"))
    g = GeneralMotionRetargeting("bvh", "unitree_g1", actual_human_height=1.75)
    sp, sr = lafan1.selection(raw.names, g.human_body_names)
    h = _lib.BvhHandle(raw.parents, 3, "zyx", sp, sr)
    rng = np.random.default_rng(seed)
    B, T, S = int(lens.sum()), int(lens.max()), len(lens)
    rows = rng.uniform(-180.0, 180.0, size=(B, h.ncol))
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    off = np.tile(raw.offsets, (S, 1, 1)) * rng.uniform(0.9, 1.1, size=(S, 1, 1))
    d_rows, d_seg, d_off = (_lib.DeviceBuffer.from_host(a) for a in (rows, seg, off))
    d_h = _lib.DeviceBuffer(S * T * h.rows * 56)
    st, e0, e1 = _lib.Stream(), _lib.Event(), _lib.Event()
    for _ in range(3):
        h.frames_dev(S, B, d_rows, d_seg, d_off, T, d_h, st)
    st.sync()
    n = 20
    e0.record(st)
    for _ in range(n):
        h.frames_dev(S, B, d_rows, d_seg, d_off, T, d_h, st)
    e1.record(st)
    st.sync()
    ms = e0.elapsed_ms(e1) / n
    bytes_alg = B * (h.ncol * 8 + h.rows * 56)
    return {"batch": name, "clips": S, "frames": B, "longest": T, "ms_per_call": ms, "ms_per_2p20_frames": ms * (1 << 20) / B,
            "algorithmic_bytes_per_frame": h.ncol * 8 + h.rows * 56, "achieved_GBps": bytes_alg / ms * 1e-6,
            "fraction_of_hbm_peak_8TBps": bytes_alg / (ms * 1e-3) / HBM_PEAK, "calls_timed": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    res = {"device": _lib.lib().gmr_backend_info().decode(),
           "batches": [batch("dataset_probe shape", rng.integers(80, 420, size=2400), 1),
                       batch("LAFAN1 shape", np.sort(rng.integers(2000, 9856, size=77))[::-1].copy(), 2)]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
