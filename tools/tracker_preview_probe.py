"""Tracker preview: device-event times of ``MotionTracker.preview_dev`` beside the sampler answering the same
queries, in one run.

  library   4 096 clips of 256 frames, G1 (29 dofs, 38 bodies with local_body_pos), identity dof map, clocks spread over 8 s, loop on
  preview   K = 8 offsets 0 .. 7 dt; per N in {4 096, 8 192, 131 072} (N x K = 32 768, 65 536, 1 048 576 queries):
              raw frame, the six sampler blocks   against ``sample_dev`` on clip i32 / time f64 arrays of the same N x K queries that
                                                  already lie on the device, six output arrays (the pass line: at most 1.35 x)
              frames reference and sim, all eight blocks with six bodies
              and -- when torch is importable -- what a user composes today for the anchored row: the clocks read back, N x K query
              times, ``sample_dev``, the yaw of the anchor taken out, the blocks concatenated, as torch operations

The preview and the sampler are timed alternately, ``--rounds`` times each: every figure is the mean of ``--reps`` repetitions between
two device events on one stream after a warm-up, and the spread over the rounds of one identical measurement is printed beside the
mean (the torch composition: a host clock around a device synchronise).  Prints one JSON document; --out writes it to a file as well.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time as clock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from motion_library_probe import HBM_PEAK, timed  # noqa: E402

SIX = ("left_ankle_roll_link", "right_ankle_roll_link", "left_wrist_yaw_link", "right_wrist_yaw_link", "torso_link", "head_link")
SAMPLER_BLOCKS = ("root_pos", "root_quat", "root_vel", "root_ang_vel", "dof_pos", "dof_vel")
ALL_BLOCKS = ("root_pos", "root_quat", "root_rot6", "root_vel", "root_ang_vel", "dof_pos", "dof_vel", "body_pos")


def figure(rounds, nbytes=None):
    """mean and spread of the rounds of one measurement (seconds each)"""
    us = [s * 1e6 for s in rounds]
    mean = float(np.mean(us))
    out = {"us": mean, "rounds_us": us, "spread": (max(us) - min(us)) / mean}
    if nbytes is not None:
        out.update(MB=nbytes / 1e6, GB_per_s=nbytes / (mean * 1e-6) / 1e9, share_of_hbm_peak=nbytes / (mean * 1e-6) / HBM_PEAK)
    return out


def torch_composition(torch, lib, trk, offsets, sel, N, reps):
    """seconds per anchored observation composed by hand: state read-back, query times, sample_dev, frame arithmetic, concatenation"""
    dev = torch.device("cuda")
    K, ndof, nb = len(offsets), lib.ndof, lib.nbody
    off = torch.tensor(offsets, device=dev, dtype=torch.float64)
    idx = torch.tensor(sel, device=dev, dtype=torch.int64)
    out = {k: torch.empty(N * K, w, device=dev) for k, w in (("root_pos", 3), ("root_rot", 4), ("root_vel", 3), ("root_ang_vel", 3), ("dof_pos", ndof),
                                                             ("dof_vel", ndof), ("local_body_pos", nb * 3))}
    stream = torch.cuda.current_stream().cuda_stream

    def rz(c, s, v):
        return torch.stack([c * v[..., 0] + s * v[..., 1], c * v[..., 1] - s * v[..., 0], v[..., 2]], dim=-1)

    def compose():
        st = trk.state()                                          # (synchronises: the clocks have no device-side view)
        clip = torch.from_numpy(st["clip"]).to(dev).repeat_interleave(K)
        tq = (torch.from_numpy(st["time"]).to(dev).double()[:, None] + off[None, :]).reshape(-1)
        lib.sample_dev(N * K, clip, tq, loop=True, stream=stream, **out)
        p, q = out["root_pos"].view(N, K, 3), out["root_rot"].view(N, K, 4)
        pa, qa = p[:, :1], q[:, 0]
        n = torch.sqrt(qa[:, 2] ** 2 + qa[:, 3] ** 2)
        z, w = (qa[:, 2] / n)[:, None], (qa[:, 3] / n)[:, None]
        c, s = w * w - z * z, 2.0 * z * w
        qr = torch.stack([w * q[..., 0] + z * q[..., 1], w * q[..., 1] - z * q[..., 0], w * q[..., 2] - z * q[..., 3], w * q[..., 3] + z * q[..., 2]], dim=-1)
        x, y, zz, ww = qr.unbind(-1)
        r6 = torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y + zz * ww), 2 * (x * zz - y * ww), 2 * (x * y - zz * ww), 1 - 2 * (x * x + zz * zz),
                          2 * (y * zz + x * ww)], dim=-1)
        lb = out["local_body_pos"].view(N, K, nb, 3)[:, :, idx]
        u, qw = q[..., None, :3].expand(-1, -1, len(sel), -1), q[..., None, 3:4]
        t = 2.0 * torch.cross(u, lb, dim=-1)
        world = p[:, :, None, :] + lb + qw * t + torch.cross(u, t, dim=-1) - pa[:, :, None, :]
        body = rz(c[..., None], s[..., None], world).reshape(N, K, -1)
        return torch.cat([rz(c, s, p - pa), qr, r6, rz(c, s, out["root_vel"].view(N, K, 3)), rz(c, s, out["root_ang_vel"].view(N, K, 3)),
                          out["dof_pos"].view(N, K, ndof), out["dof_vel"].view(N, K, ndof), body], dim=-1)

    for _ in range(3):
        compose()
    torch.cuda.synchronize()
    t0 = clock.perf_counter()
    for _ in range(reps):
        compose()
    torch.cuda.synchronize()
    return (clock.perf_counter() - t0) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--offsets", type=int, default=8)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192, 131072])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition even when torch is importable")
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    from general_motion_retargeting_amd import KinematicsModel, MotionTracker, ROBOT_XML_DICT, _lib as hip
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    hip.require_gpu()
    km = KinematicsModel(ROBOT_XML_DICT["unitree_g1"])
    names = list(km.body_names)
    ndof, nb, S, T, K, dt = km.num_dof, len(names), args.clips, args.frames, args.offsets, 0.02
    B = S * T
    rng = np.random.default_rng(0)
    st = hip.Stream()
    w = np.cumsum(rng.normal(size=(S, T, 4)) * 0.05, axis=1) + rng.normal(size=(S, 1, 4))
    src = [rng.normal(0, 0.5, size=(B, 3)) + np.array([0.3, -0.2, 0.8]), (w / np.linalg.norm(w, axis=2, keepdims=True)).reshape(B, 4),
           rng.uniform(-1.2, 1.2, size=(B, ndof)), rng.standard_normal(size=(B, nb, 3), dtype=np.float32)]
    bufs = [hip.DeviceBuffer.from_host(a) for a in src]
    del src, w
    lib = MotionLibrary.from_device((np.arange(S + 1) * T).astype(np.int32), np.full(S, 30.0), ndof, nb, *bufs, stream=st)
    st.sync()
    torch = None
    if not args.no_torch:
        try:
            import torch
            if not torch.cuda.is_available():
                torch = None
        except ImportError:
            torch = None
    offsets = (np.arange(K) * dt).astype(np.float32)
    six = [names.index(n) for n in SIX]
    row_in = 2 * (13 + 2 * ndof) * 4                       # the two source rows of a query, six arrays
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "clips": S, "frames_per_clip": T, "ndof": ndof, "bodies": nb, "offsets": K,
           "reps": args.reps, "rounds": args.rounds, "pass_line": "preview (raw, six sampler blocks) <= 1.35 x sample_dev on the same N x K queries",
           "composition": "torch " + torch.__version__ if torch else "not run (torch not importable, or --no-torch)", "N": {}}
    for N in args.sizes:
        NK = N * K
        trk = MotionTracker(lib, N, dt, loop=True, seed=1)
        trk.reset_dev(stream=st, time_offset_range=(0.0, 8.0))
        st.sync()
        s = trk.state()
        d_clip = hip.DeviceBuffer.from_host(np.repeat(s["clip"], K))
        d_time = hip.DeviceBuffer.from_host((s["time"].astype(np.float64)[:, None] + offsets.astype(np.float64)[None, :]).reshape(-1))
        sample_out = {k: hip.DeviceBuffer(NK * c * 4) for k, c in (("root_pos", 3), ("root_rot", 4), ("root_vel", 3), ("root_ang_vel", 3),
                                                                   ("dof_pos", ndof), ("dof_vel", ndof))}
        lay = trk.set_preview(offsets, SAMPLER_BLOCKS, "raw")
        D = lay["row_width"]
        obs = hip.DeviceBuffer(NK * D * 4)
        pv, sm = [], []
        for _ in range(args.rounds):                           # alternated
            pv.append(timed(hip, st, lambda: trk.preview_dev(stream=st, obs=obs), args.reps))
            sm.append(timed(hip, st, lambda: lib.sample_dev(NK, d_clip, d_time, loop=True, stream=st, **sample_out), args.reps))
        r = {"queries": NK, "row_width_raw": D,
             "preview_raw_six_blocks": figure(pv, NK * (row_in + D * 4) + N * 8),
             "sample_dev_same_queries": figure(sm, NK * (row_in + D * 4 + 12))}
        r["preview_over_sampler"] = r["preview_raw_six_blocks"]["us"] / r["sample_dev_same_queries"]["us"]
        r["pass_line_met"] = bool(r["preview_over_sampler"] <= 1.35)
        del obs, sample_out
        q = rng.normal(size=(N, 4))
        sim = {"base_pos": hip.DeviceBuffer.from_host(rng.normal(size=(N, 3)).astype(np.float32)),
               "base_quat": hip.DeviceBuffer.from_host((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32))}
        for frame in ("reference", "sim"):
            lay = trk.set_preview(offsets, ALL_BLOCKS, frame, six)
            Da = lay["row_width"]
            obs = hip.DeviceBuffer(NK * Da * 4)
            valid, status = hip.DeviceBuffer(NK * 4), hip.DeviceBuffer(N * 4)
            rounds = [timed(hip, st, lambda: trk.preview_dev(sim if frame == "sim" else None, stream=st, obs=obs, valid=valid, status=status), args.reps)
                      for _ in range(args.rounds)]
            r[f"preview_{frame}_all_blocks_six_bodies"] = dict(figure(rounds, NK * (row_in + 2 * 18 * 4 + Da * 4 + 4) + N * 12), row_width=Da)
            del obs
        if torch:
            trk.set_preview(offsets, ALL_BLOCKS, "reference", six)
            sec = torch_composition(torch, lib, trk, offsets, six, N, max(3, args.reps // 3))
            r["torch_composition_reference_row"] = {"us": sec * 1e6, "note": "host clock around a device synchronise; includes the read-back of the clocks"}
            r["torch_composition_over_preview"] = sec * 1e6 / r["preview_reference_all_blocks_six_bodies"]["us"]
        doc["N"][str(N)] = r
        trk.close()
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
