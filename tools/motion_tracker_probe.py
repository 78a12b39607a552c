"""Motion tracker: device-event times of ``MotionTracker.step_dev`` beside the sampler alone and beside the
composition it replaces, in one run.

  library   4 096 clips of 256 frames, G1 shapes (29 dofs), the shape of tools/motion_library_probe.py; the tracker maps the 29
            columns onto 31 robot dofs (two on their defaults)
  per N     in {4 096, 65 536, 1 048 576}: one step without simulator state (references only), one step with it (references, six
            errors, six terms, total), ``gmr_motion_sample_dev`` alone on the same (clip, time), and -- when torch is importable --
            the composition: ``sample_dev`` into torch tensors, the clock converted to float64, the scatter into robot order and the
            six formulas of t1_imitation.py:249-309 as torch operations, the clock advance

  --anchors per N, on the same tracker: the step with simulator state and a link step (six links of the G1, world
            frame, packed rigid-body tensor, ``total / fail / finished / link_err``) plain, then both again with anchors enabled and set
            to random moves, and ``anchor_to_root_dev`` alone with a mask of one in fifty and of all

Each figure is the mean of ``--reps`` repetitions between two device events on one stream, after a warm-up (the composition: a host
clock around a device synchronise, since torch enqueues on its own stream).  Bytes come from the shapes (state, two source rows,
simulator rows, every output row once); the share is bytes/s over the 8 TB/s HBM peak.  Prints one JSON document; --out writes it to
a file as well.
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
from motion_library_probe import HBM_PEAK, row, timed  # noqa: E402


def torch_composition(torch, lib, N, R, dmap, default, scales, reps):
    """seconds per step of: sample_dev + float64 clock + scatter + six formulas + clock advance, all on torch's current stream"""
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(0)
    clip = torch.randint(0, lib.num_clips, (N,), generator=g, dtype=torch.int32).to(dev)
    times = (torch.rand(N, generator=g) * 8.0).to(dev)
    ndof = lib.ndof
    o = {k: torch.empty(N, w, device=dev) for k, w in (("root_pos", 3), ("root_rot", 4), ("root_vel", 3), ("root_ang_vel", 3), ("dof_pos", ndof),
                                                         ("dof_vel", ndof))}
    sim = {k: torch.randn(N, w, device=dev) for k, w in (("base_pos", 3), ("base_quat", 4), ("base_lin_vel", 3), ("base_ang_vel", 3), ("dof_pos", R),
                                                           ("dof_vel", R))}
    on = torch.from_numpy(dmap >= 0).to(dev)
    col = torch.from_numpy(np.where(dmap >= 0, dmap, 0).astype(np.int64)).to(dev)
    dflt, sc = torch.from_numpy(default).to(dev), torch.tensor(scales, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def step():
        t64 = times.double()
        lib.sample_dev(N, clip, t64, True, stream=stream, **o)
        ref_pos = torch.where(on, o["dof_pos"][:, col], dflt)
        ref_vel = torch.where(on, o["dof_vel"][:, col], torch.zeros((), device=dev))
        w = (sim["base_quat"] * o["root_rot"]).sum(dim=1)
        err = torch.stack([torch.norm(sim["base_pos"] - o["root_pos"], dim=1), 2.0 * torch.acos(torch.clamp(torch.abs(w), 0.0, 1.0)),
                           torch.norm(sim["base_lin_vel"] - o["root_vel"], dim=1), torch.norm(sim["base_ang_vel"] - o["root_ang_vel"], dim=1),
                           torch.norm(sim["dof_pos"] - ref_pos, dim=1), torch.norm(sim["dof_vel"] - ref_vel, dim=1)], dim=1)
        term = torch.exp(-err / sc)
        total = term.sum(dim=1)
        times.add_(0.02)
        return total

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = clock.perf_counter()
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    return (clock.perf_counter() - t0) / reps


def anchored_legs(hip, st, t, rng, N, sim, out, reps):
    """the plain step and link step of tracker ``t``, the same two with anchors set, and ``anchor_to_root_dev`` alone -> microseconds"""
    from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT
    km = KinematicsModel(ROBOT_XML_DICT["unitree_g1"])
    sel = [29, 3, 15, 0, 36, 8]
    nb = len(km.body_names)
    t.set_links(km, bodies=sel, sim_bodies=sel, frame="world")
    links = {"body_state": hip.DeviceBuffer.from_host(rng.normal(size=(N, nb, 13)).astype(np.float32)), "num_bodies": nb}
    lout = {k: hip.DeviceBuffer(N * c * 4) for k, c in (("total", 1), ("fail", 1), ("finished", 1), ("link_err", 4))}
    legs = {"step": lambda: t.step_dev(sim, stream=st, **out), "step_links": lambda: t.step_links_dev(sim, links, stream=st, **lout)}
    r = {}
    for name, fn in legs.items():
        r[name + "_plain_us"] = timed(hip, st, fn, reps) * 1e6
    t.enable_anchors()
    t.set_anchor_dev(hip.DeviceBuffer.from_host(rng.uniform(-10, 10, (N, 3)).astype(np.float32)),
                     hip.DeviceBuffer.from_host(rng.uniform(-np.pi, np.pi, N).astype(np.float32)), stream=st)
    for name, fn in legs.items():
        r[name + "_anchored_us"] = timed(hip, st, fn, reps) * 1e6
        r[name + "_anchored_over_plain"] = r[name + "_anchored_us"] / r[name + "_plain_us"]
    q = rng.normal(size=(N, 4))
    root_pos = hip.DeviceBuffer.from_host(rng.uniform(-5, 5, (N, 3)).astype(np.float32))
    root_quat = hip.DeviceBuffer.from_host((q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32))
    for name, mask in (("one_in_fifty", (rng.uniform(size=N) < 0.02).astype(np.int32)), ("all", None)):
        d_mask = None if mask is None else hip.DeviceBuffer.from_host(mask)
        r[f"anchor_to_root_dev_{name}_us"] = timed(hip, st, lambda: t.anchor_to_root_dev(root_pos, root_quat, mask=d_mask, yaw=True, z=True, stream=st), reps) * 1e6
    t.enable_anchors(False)
    t.set_links(bodies=[])
    return r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 1048576])
    ap.add_argument("--no-torch", action="store_true", help="skip the composition even when torch is importable")
    ap.add_argument("--anchors", action="store_true", help="add the anchored legs of DESIGN.md section 6o")
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    from general_motion_retargeting_amd import MotionTracker, _lib as hip
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    hip.require_gpu()
    ndof, S, T = 29, args.clips, args.frames
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
    dmap = np.concatenate([[-1, -1], np.arange(ndof)]).astype(np.int32)
    R = len(dmap)
    default = rng.uniform(-0.3, 0.3, R).astype(np.float32)
    scales = (0.5, 0.5, 2.0, 1.0, 1.0, 0.1)
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "clips": S, "frames_per_clip": T, "B": B, "ndof": ndof, "robot_dofs": R,
           "reps": args.reps, "hbm_peak_GB_per_s": HBM_PEAK / 1e9, "N": {}}
    torch = None
    if not args.no_torch:
        try:
            import torch
            if not torch.cuda.is_available():
                torch = None
        except ImportError:
            torch = None
    doc["composition"] = "torch " + torch.__version__ if torch else "not run (torch not importable, or --no-torch)"
    lib_row = 4 * (13 + 2 * ndof)                               # one row of the library's six arrays
    for N in args.sizes:
        t = MotionTracker(lib, N, 0.02, dof_map=dmap, dof_default=default, loop=True, seed=1)
        t.reset_dev(stream=st, time_offset_range=(0.0, 8.0))
        counts, sim_counts = t._counts()
        out = {k: hip.DeviceBuffer(N * c * 4) for k, c in counts.items()}
        sim = {k: hip.DeviceBuffer.from_host(rng.normal(size=(N, c)).astype(np.float32)) for k, c in sim_counts.items()}
        refs = {k: v for k, v in out.items() if k not in ("err", "term", "total")}
        r = {}
        state_bytes = N * (4 + 4) + N * 4                                       # clip and clock read, clock written
        ref_bytes = N * (2 * lib_row + 4 * (13 + 2 * R) + 8)                    # two source rows, the reference rows, status and finished
        sec = timed(hip, st, lambda: t.step_dev(None, stream=st, **refs), args.reps)
        r["step_references_only"] = dict(row(sec, state_bytes + ref_bytes), envs_per_s=N / sec)
        sec = timed(hip, st, lambda: t.step_dev(sim, stream=st, **out), args.reps)
        r["step_with_simulator_state"] = dict(row(sec, state_bytes + ref_bytes + N * 4 * (13 + 2 * R) + N * 4 * 13), envs_per_s=N / sec)
        s = t.state()
        d_clip, d_time = hip.DeviceBuffer.from_host(s["clip"]), hip.DeviceBuffer.from_host(s["time"].astype(np.float64))
        so = {k: hip.DeviceBuffer(N * c * 4) for k, c in (("root_pos", 3), ("root_rot", 4), ("root_vel", 3), ("root_ang_vel", 3), ("dof_pos", ndof),
                                                          ("dof_vel", ndof), ("status", 1))}
        sec = timed(hip, st, lambda: lib.sample_dev(N, d_clip, d_time, True, stream=st, **so), args.reps)
        r["sample_dev_alone"] = dict(row(sec, N * (12 + 3 * lib_row + 4)), queries_per_s=N / sec)
        if torch:
            sec = torch_composition(torch, lib, N, R, dmap, default, scales, args.reps)
            r["composition_sample_dev_plus_torch"] = {"us": sec * 1e6, "note": "host clock around a device synchronise"}
            r["composition_over_step"] = sec * 1e6 / r["step_with_simulator_state"]["us"]
        if args.anchors:
            r["anchors"] = anchored_legs(hip, st, t, rng, N, sim, out, args.reps)
        doc["N"][str(N)] = r
        t.close()
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
