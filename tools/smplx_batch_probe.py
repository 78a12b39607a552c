#!/usr/bin/env python3
"""gmr_smplx_batch_frames_dev alone: ragged AMASS-shaped clips resident in device memory, calls timed between device events.

    python tools/smplx_batch_probe.py [--frames OUTPUT_FRAMES] [--reps N] [--out FILE]

One batch per source rate (120, 60, 50 and 30 fps against tgt_fps = 30; clips of 80 .. 2 000 source frames, the 14 bodies of
smplx_to_g1, a different subject per clip), each of about --frames output frames.  Reports, per batch, the median / min / max
over --reps calls of the ms per call, the ms per 2^20 OUTPUT frames, and the fraction of the HBM roof on the algorithmic
traffic (276 B per source frame in, 784 B per output frame out; the scratch planes are not counted).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12        # B/s, spec (MI355X)
G1_BODIES = [0, 1, 2, 4, 5, 7, 8, 12, 16, 17, 18, 19, 20, 21]


def batch(fps, out_frames, reps, seed):
    from general_motion_retargeting_amd import _lib
    from general_motion_retargeting_amd.utils import smpl
    h = smpl._handle(smpl.SMPLX_PARENTS, G1_BODIES)
    rng = np.random.default_rng(seed)
    skip = int(fps / 30.0) if fps > 30.0 else 1
    lens = []
    while sum(n // skip for n in lens) < out_frames:
        lens.append(int(rng.integers(80, 2001)))
    lens = np.array(lens, dtype=np.int64)
    nout = (lens // skip).astype(np.int32)
    S, B, T = len(lens), int(lens.sum()), int(nout.max())
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ro = rng.normal(0, 0.6, size=(B, 3)).astype(np.float32)
    pb = rng.normal(0, 0.6, size=(B, 63)).astype(np.float32)
    tr = rng.normal(0, 1.0, size=(B, 3)).astype(np.float32)
    align = np.full(S, 1 if fps > 30.0 else 0, dtype=np.uint8)
    jrest = np.cumsum(rng.normal(0, 0.1, size=(S, 55, 3)), axis=1)
    out_off = np.concatenate([[0], np.cumsum(nout.astype(np.int64))])          # dense destinations: clip after clip
    d_out = _lib.DeviceBuffer(max(int(out_off[-1]), 1) * h.rows * 56)
    tab = (d_out.ptr.value + out_off[:-1] * h.rows * 56).astype(np.uint64)
    d = [_lib.DeviceBuffer.from_host(a) for a in (ro, pb, tr, seg, nout, align, jrest, tab)]
    st, e0, e1 = _lib.Stream(), _lib.Event(), _lib.Event()
    for _ in range(3):
        h.batch_frames_dev(S, B, *d, st)
    st.sync()
    ms = []
    for _ in range(reps):
        e0.record(st)
        h.batch_frames_dev(S, B, *d, st)
        e1.record(st)
        st.sync()
        ms.append(e0.elapsed_ms(e1))
    ms = np.array(ms)
    F = int(nout.sum())
    bytes_alg = B * 276 + F * h.rows * 56
    med = float(np.median(ms))
    return {"src_fps": fps, "clips": S, "source_frames": B, "output_frames": F, "longest_output": T, "calls_timed": reps,
            "ms_per_call": {"median": med, "min": float(ms.min()), "max": float(ms.max())},
            "ms_per_2p20_output_frames": {"median": med * (1 << 20) / F, "min": float(ms.min()) * (1 << 20) / F, "max": float(ms.max()) * (1 << 20) / F},
            "algorithmic_bytes": bytes_alg, "achieved_GBps": bytes_alg / med * 1e-6,
            "fraction_of_hbm_peak_8TBps": bytes_alg / (med * 1e-3) / HBM_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 19)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    res = {"device": _lib.lib().gmr_backend_info().decode(),
           "batches": [batch(fps, a.frames, a.reps, i) for i, fps in enumerate((120.0, 60.0, 50.0, 30.0))]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
