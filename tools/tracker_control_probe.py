"""Tracker control: device-event times of ``MotionTracker.targets_dev`` and of one ``torques_dev`` substep beside the
same computation written as torch operations on the same tensors, in one run.

  library    64 clips of 256 frames with 21 dofs, mapped onto R = 23 robot dofs (two on their defaults), clocks spread over 8 s, loop on
  control    action_scale 0.25, clip 1.0, 2 s of start-up, decimation M = 10; episode steps spread over both phases, delays over 0 .. M - 1
  actuators  stiffness, damping and friction per environment and dof, a torque limit per dof
  per N in {4 096, 65 536, 1 048 576}:
     targets_dev                  one launch             against  a preview of offset 0 for the reference row, then the easing, the
                                                                  clip and the residual as torch operations (what a user writes today)
     torques_dev, mean over the   one launch per substep  against the reference's lines as torch operations: masked assignment of the
     M substeps of a step                                         delayed targets, PD law, friction, clip, running sum
     a whole step                 1 + M launches         against  the two compositions with the zeroing and the division of the sum

Every figure is the mean of ``--reps`` (at least 50) repetitions between two device events on torch's current stream after a warm-up;
fused and composed are timed alternately, ``--rounds`` times each, and the spread over the rounds is printed beside the mean.  The bytes of
a call are counted from the shapes.  The composition is the yardstick; without torch on a GPU only the fused calls are timed (on device
buffers of this library).  Prints one JSON document; --out writes it to a file as well.
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
from motion_library_probe import HBM_PEAK  # noqa: E402
from tracker_preview_probe import figure  # noqa: E402

R, NDOF = 23, 21


def timer(hip, handle):
    """``timed(fn, reps)``: seconds per call of ``fn`` between two device events on the stream ``handle`` (None: the null stream) after a warm-up"""
    def sync():
        hip.check(hip.lib().gmr_stream_sync(handle))

    def timed(fn, reps, warm=3):
        for _ in range(warm):
            fn()
        sync()
        a, b = hip.Event(), hip.Event()
        a.record(handle)
        for _ in range(reps):
            fn()
        b.record(handle)
        sync()
        return a.elapsed_ms(b) * 1e-3 / reps

    return timed


def bytes_per_call(N, M):
    """(targets, one substep averaged over the M of a step) from the shapes: float32 [N, R] blocks and int32 [N] arrays"""
    nr = N * R * 4
    targets = 2 * NDOF * 4 * N + nr + 4 * N + 8 * N + 2 * nr + 4 * N          # two library rows, actions, steps, clip + time; targets, clipped, status
    # reads q, qd, held, kp, kd, fr always, acc in M - 1 substeps, the targets where the delay matches (once per environment and step);
    # writes tau and acc always, held where the delay matches, the mean once
    substep = (6 + (M - 1) / M + 1 / M) * nr + 4 * N + (2 + 2 / M) * nr
    return targets, substep


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--decimation", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 1048576])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition even when torch is importable")
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    if args.reps < 50:
        ap.error("--reps: the mean of at least 50 repetitions")
    from general_motion_retargeting_amd import MotionTracker, _lib as hip
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    hip.require_gpu()
    S, T, M, dt = args.clips, args.frames, args.decimation, 0.02
    B = S * T
    rng = np.random.default_rng(0)
    w = np.cumsum(rng.normal(size=(S, T, 4)) * 0.05, axis=1) + rng.normal(size=(S, 1, 4))
    src = [rng.normal(0, 0.5, size=(B, 3)) + np.array([0.3, -0.2, 0.8]), (w / np.linalg.norm(w, axis=2, keepdims=True)).reshape(B, 4),
           rng.uniform(-1.2, 1.2, size=(B, NDOF))]
    bufs = [hip.DeviceBuffer.from_host(a) for a in src]
    lib = MotionLibrary.from_device((np.arange(S + 1) * T).astype(np.int32), np.full(S, 30.0), NDOF, 0, *bufs, None)
    hip.check(hip.lib().gmr_stream_sync(None))
    torch = None
    if not args.no_torch:
        try:
            import torch
            if not torch.cuda.is_available():
                torch = None
        except ImportError:
            torch = None
    stream = (torch.cuda.current_stream().cuda_stream or None) if torch else None          # the stream torch enqueues on
    timed = timer(hip, stream)
    dmap = np.concatenate([np.arange(NDOF), [-1, -1]]).astype(np.int32)
    pose = rng.uniform(-0.5, 0.5, R).astype(np.float32)
    k, c, D, g0, g1 = 0.25, 1.0, 2.0, 0.1, 0.2
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "R": R, "library_dofs": NDOF, "decimation": M, "reps": args.reps, "rounds": args.rounds,
           "hbm_peak_bytes_per_s": HBM_PEAK, "composition": "torch " + torch.__version__ if torch else "not run (torch not importable, no GPU in it, or --no-torch)",
           "N": {}}
    for N in args.sizes:
        trk = MotionTracker(lib, N, dt, dmap, np.zeros(R, np.float32), loop=True, seed=1)
        trk.reset(time_offset_range=(0.0, 8.0))
        trk.set_control(pose, k, c, D, g0, g1, decimation=M)
        host = {"actions": rng.normal(0, 0.8, (N, R)), "q": rng.uniform(-1, 1, (N, R)), "qd": rng.uniform(-4, 4, (N, R)), "kp": rng.uniform(20, 200, (N, R)),
                "kd": rng.uniform(0.5, 5, (N, R)), "fr": rng.uniform(0, 3, (N, R)), "lim": rng.uniform(5, 40, R)}
        host = {name: a.astype(np.float32) for name, a in host.items()}
        host["steps"] = rng.integers(0, 2 * int(D / dt), N).astype(np.int32)
        host["delay"] = rng.integers(0, M, N).astype(np.int32)
        for name in ("tg", "clipped", "tau", "mean"):
            host[name] = np.zeros((N, R), np.float32)
        host["status"] = np.zeros(N, np.int32)
        if torch:
            d = {name: torch.from_numpy(a).cuda() for name, a in host.items()}
        else:
            d = {name: hip.DeviceBuffer.from_host(a) for name, a in host.items()}

        def fused_targets():
            trk.targets_dev(d["actions"], d["steps"], d["tg"], d["clipped"], d["status"], stream=stream)

        def fused_substep(i):
            trk.torques_dev(i, d["tg"], d["q"], d["qd"], d["kp"], d["kd"], d["tau"], d["fr"], d["lim"], d["delay"], d["mean"], per_env=True, stream=stream)

        def fused_substeps():
            for i in range(M):
                fused_substep(i)

        def fused_step():
            fused_targets()
            fused_substeps()

        b_targets, b_substep = bytes_per_call(N, M)
        ft, fs, fw, ct, cs, cw = [], [], [], [], [], []
        if torch:
            trk.set_preview([0.0], ("dof_pos",), "raw")
            ref = torch.empty(N, R, device="cuda")
            last, acc, default = torch.zeros(N, R, device="cuda"), torch.zeros(N, R, device="cuda"), torch.from_numpy(pose).cuda()
            comp = {}

            def composed_targets():
                trk.preview_dev(stream=stream, obs=ref)                  # the reference row at the new clock
                te = d["steps"] * dt
                startup = te < D
                s = 0.5 * (1.0 - torch.cos(torch.clamp(te / D, 0.0, 1.0) * 3.14159))
                a = torch.clip(d["actions"], -c, c)
                tg = torch.where(startup.unsqueeze(1), default * (1.0 - s.unsqueeze(1)) + ref * s.unsqueeze(1), ref.clone())
                gain = torch.where(startup, g0, g1)
                tg += k * a * gain.unsqueeze(1)
                comp["tg"] = tg

            def composed_substep(i):
                tg = comp["tg"]
                hit = d["delay"] == i
                last[hit] = tg[hit]
                tau = d["kp"] * (last - d["q"]) - d["kd"] * d["qd"]
                fric = torch.min(d["fr"], tau.abs()) * torch.sign(tau)
                tau = torch.clip(tau - fric, min=-d["lim"], max=d["lim"])
                acc.add_(tau)
                comp["tau"] = tau

            def composed_substeps():
                for i in range(M):
                    composed_substep(i)

            def composed_step():
                composed_targets()
                acc.zero_()
                composed_substeps()
                acc.div_(M)

            composed_targets()
        for _ in range(args.rounds):                                   # alternated
            ft.append(timed(fused_targets, args.reps))
            if torch:
                ct.append(timed(composed_targets, args.reps))
            fs.append(timed(fused_substeps, args.reps) / M)
            if torch:
                cs.append(timed(composed_substeps, args.reps) / M)
            fw.append(timed(fused_step, args.reps))
            if torch:
                cw.append(timed(composed_step, args.reps))
        r = {"elements": N * R, "targets_dev": figure(ft, b_targets), "torques_dev_per_substep": figure(fs, b_substep),
             "fused_step": dict(figure(fw, b_targets + M * b_substep), launches=1 + M)}
        if torch:
            r.update(torch_targets=figure(ct), torch_per_substep=figure(cs), torch_step=figure(cw))
            r["composition_over_fused"] = {"targets": r["torch_targets"]["us"] / r["targets_dev"]["us"],
                                           "substep": r["torch_per_substep"]["us"] / r["torques_dev_per_substep"]["us"],
                                           "step": r["torch_step"]["us"] / r["fused_step"]["us"]}
            # both have run whole steps last: the same held targets up to the cosine of the easing, so the same torques up to kp times that
            r["largest_difference_of_the_last_torques"] = float((comp["tau"] - d["tau"]).abs().max())
        doc["N"][str(N)] = r
        trk.close()
        del d
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
