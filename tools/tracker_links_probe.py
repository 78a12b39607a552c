"""Tracker links: device-event times of ``MotionTracker.step_links_dev`` beside what a user had before it, in one
run.

  library   4 096 clips of 256 frames, G1 (29 dofs, 38 bodies), the shape of tools/motion_tracker_probe.py; identity dof map
  per N     in {4 096, 65 536, 1 048 576}, for all bodies and for a six-link selection (ankles, wrists, torso, head):
              link step with simulator state (a packed [N][38][13] rigid-body tensor read in place), without and with ref_body_*
              outputs; link step that writes references only;
              the two launches it replaces: ``step_dev`` with simulator state + ``body_state_dev`` for the same selection;
              and -- when torch is importable -- the whole composition: those two launches, the float64 clock, the gather of the
              simulator's tensor into selection order and the four link formulas as torch operations

Each figure is the mean of ``--reps`` repetitions between two device events on one stream, after a warm-up (the torch composition: a host
clock around a device synchronise, since torch enqueues on its own stream).  Prints one JSON document; --out writes it to a file as well.
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
from motion_library_probe import timed  # noqa: E402

SIX = ("left_ankle_roll_link", "right_ankle_roll_link", "left_wrist_yaw_link", "right_wrist_yaw_link", "torso_link", "head_link")
WIDTH = {"body_pos": 3, "body_rot": 4, "body_vel": 3, "body_ang_vel": 3}


def torch_composition(torch, lib, trk, km, sel, N, nb, reps):
    """seconds per step of: step_dev + float64 clock + body_state_dev + gather + four link formulas, on torch's current stream"""
    dev = torch.device("cuda")
    nsel = len(sel)
    R = trk.nrobot_dof
    out = {k: torch.empty(N, w, device=dev) for k, w in (("ref_root_pos", 3), ("ref_root_rot", 4), ("ref_dof_pos", R), ("term", 6), ("total", 1))}
    sim = {k: torch.randn(N, w, device=dev) for k, w in (("base_pos", 3), ("base_quat", 4), ("base_lin_vel", 3), ("base_ang_vel", 3), ("dof_pos", R),
                                                          ("dof_vel", R))}
    body = {k: torch.empty(N, nsel, w, device=dev) for k, w in WIDTH.items()}
    rigid = torch.randn(N, nb, 13, device=dev)
    idx = torch.tensor(sel, device=dev, dtype=torch.int64)
    st = trk.state()
    clip = torch.from_numpy(st["clip"]).to(dev)
    times = torch.from_numpy(st["time"]).to(dev)
    scale = torch.tensor([0.3, 0.8, 2.0, 4.0], device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        t64 = times.double()                                     # (a shadow of the tracker's clock)
        lib.body_state_dev(N, clip, t64, kinematics=km, bodies=sel, stream=stream, **body)
        trk.step_dev(sim, stream=stream, **out)
        rb = rigid[:, idx]
        e_pos = (rb[..., 0:3] - body["body_pos"]).pow(2).sum(-1)
        dot = (rb[..., 3:7] * body["body_rot"]).sum(-1).abs().clamp(max=1.0)
        e_rot = (2.0 * torch.acos(dot)).pow(2)
        e_vel = (rb[..., 7:10] - body["body_vel"]).pow(2).sum(-1)
        e_ang = (rb[..., 10:13] - body["body_ang_vel"]).pow(2).sum(-1)
        err = torch.stack([e_pos.mean(1), e_rot.mean(1), e_vel.mean(1), e_ang.mean(1)], dim=1).sqrt()
        term = torch.exp(-err / scale)
        fail = ~(e_pos.max(dim=1).values.sqrt() <= 0.5)
        times.add_(0.02)
        return out["total"][:, 0] + term.sum(1), fail

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = clock.perf_counter()
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    return (clock.perf_counter() - t0) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 1048576])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition even when torch is importable")
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    from general_motion_retargeting_amd import KinematicsModel, MotionTracker, ROBOT_XML_DICT, _lib as hip
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    hip.require_gpu()
    km = KinematicsModel(ROBOT_XML_DICT["unitree_g1"])
    names = list(km.body_names)
    ndof, nb, S, T = km.num_dof, len(names), args.clips, args.frames
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
    torch = None
    if not args.no_torch:
        try:
            import torch
            if not torch.cuda.is_available():
                torch = None
        except ImportError:
            torch = None
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "clips": S, "frames_per_clip": T, "ndof": ndof, "bodies": nb, "reps": args.reps,
           "composition": "torch " + torch.__version__ if torch else "not run (torch not importable, or --no-torch)", "N": {}}
    cases = {"all_bodies": list(range(nb)), "six_links": [names.index(n) for n in SIX]}
    for N in args.sizes:
        doc["N"][str(N)] = {}
        rigid = hip.DeviceBuffer.from_host(rng.normal(size=(N, nb, 13)).astype(np.float32))
        for case, sel in cases.items():
            nsel = len(sel)
            trk = MotionTracker(lib, N, 0.02, loop=True, seed=1)
            trk.reset_dev(stream=st, time_offset_range=(0.0, 8.0))
            trk.set_links(km, bodies=sel, sim_bodies=sel)
            counts, sim_counts = trk._counts()
            out = {k: hip.DeviceBuffer(N * c * 4) for k, c in counts.items()}
            lout = {k: hip.DeviceBuffer(N * c * 4) for k, c in trk._link_counts().items()}
            terms = {k: v for k, v in lout.items() if not k.startswith("ref_body")}
            refs = {k: v for k, v in lout.items() if k.startswith("ref_body")}
            plain_refs = {k: v for k, v in out.items() if k not in ("err", "term", "total")}
            sim = {k: hip.DeviceBuffer.from_host(rng.normal(size=(N, c)).astype(np.float32)) for k, c in sim_counts.items()}
            links = {"body_state": rigid, "num_bodies": nb}
            r = {}
            sec = timed(hip, st, lambda: trk.step_links_dev(sim, links, stream=st, **out, **terms), args.reps)
            r["link_step_with_simulator_state"] = {"us": sec * 1e6}
            sec = timed(hip, st, lambda: trk.step_links_dev(sim, links, stream=st, **out, **lout), args.reps)
            r["link_step_with_simulator_state_and_ref_body"] = {"us": sec * 1e6}
            sec = timed(hip, st, lambda: trk.step_links_dev(None, None, stream=st, **plain_refs, **refs), args.reps)
            r["link_step_references_only"] = {"us": sec * 1e6}
            s = trk.state()
            d_clip, d_time = hip.DeviceBuffer.from_host(s["clip"]), hip.DeviceBuffer.from_host(s["time"].astype(np.float64))
            body = {k: hip.DeviceBuffer(N * nsel * c * 4) for k, c in WIDTH.items()}
            t_step = timed(hip, st, lambda: trk.step_dev(sim, stream=st, **out), args.reps)
            t_body = timed(hip, st, lambda: lib.body_state_dev(N, d_clip, d_time, kinematics=km, bodies=sel, stream=st, **body), args.reps)

            def both():
                lib.body_state_dev(N, d_clip, d_time, kinematics=km, bodies=sel, stream=st, **body)
                trk.step_dev(sim, stream=st, **out)
            t_both = timed(hip, st, both, args.reps)
            r["step_dev_alone"] = {"us": t_step * 1e6}
            r["body_state_dev_alone"] = {"us": t_body * 1e6}
            r["step_dev_plus_body_state_dev"] = {"us": t_both * 1e6, "note": "two launches back to back, no link formulas"}
            r["two_launches_over_link_step"] = t_both * 1e6 / r["link_step_with_simulator_state"]["us"]
            if torch:
                sec = torch_composition(torch, lib, trk, km, sel, N, nb, args.reps)
                r["torch_composition"] = {"us": sec * 1e6, "note": "host clock around a device synchronise"}
                r["torch_composition_over_link_step"] = sec * 1e6 / r["link_step_with_simulator_state"]["us"]
            doc["N"][str(N)][case] = r
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
