"""Tracker proprioception: device-event times of ``MotionTracker.proprio_dev`` beside the same computation written
as torch operations on the same tensors, in one run.

  tracker    R = 23 robot dofs on a 21-dof library, C = 5 pass-through columns (W = 80), dt = 0.02, filter weight 0.1
  noise      all six blocks gaussian and additive, drawn in every timed call (the composition: ``torch.randn_like`` per block)
  per N in {4 096, 65 536, 1 048 576}:
     proprio_dev   one launch   against   the reference's lines as torch operations (``compose``): three rotations, the two filters, the
                                          noisy observation row and privileged block, the fourteen penalties and their weighted sum, the
                                          three termination tests, the roll-over of the three last_* tensors

Every figure is the mean of ``--reps`` (at least 50) repetitions between two device events on torch's current stream after a warm-up;
fused and composed are timed alternately, ``--rounds`` times each, and the spread over the rounds is printed beside the mean.  The bytes of
a call are counted from the shapes.  With noise off the two paths make one step from the same state and the largest difference of their
outputs is reported.  The composition is the yardstick; without torch on a GPU only the fused call is timed (on device buffers of this
library).  Prints one JSON document; --out writes it to a file as well.
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
from tracker_control_probe import timer  # noqa: E402
from tracker_preview_probe import figure  # noqa: E402

R, NDOF, CX, DT = 23, 21, 5, 0.02
W = 6 + CX + 3 * R
CFG = dict(base_height_target=0.68, terminate_vel=50.0, terminate_height=0.3, max_episode_steps=500, extra_cols=CX, filter_weight=0.1,
           normalization={"gravity": 1.0, "lin_vel": 2.0, "ang_vel": 0.25, "dof_pos": 1.0, "dof_vel": 0.1}, soft_dof_pos_limit=0.9,
           soft_dof_vel_limit=0.8, soft_torque_limit=0.85)
NOISE = {k: {"distribution": "gaussian", "operation": "additive", "range": (0.0, b)} for k, b in
         (("gravity", 0.05), ("ang_vel", 0.2), ("dof_pos", 0.01), ("dof_vel", 1.5), ("lin_vel", 0.1), ("height", 0.05))}
SCALES = {"lin_vel_z": -2.0, "ang_vel_xy": -0.2, "orientation": -5.0, "torques": -2e-4, "dof_vel": -1e-4, "dof_acc": -1e-7, "root_acc": -1e-4,
          "action_rate": -1.0, "dof_pos_limits": -1.0, "dof_vel_limits": -1.0, "torque_limits": -0.1, "torque_tiredness": -1e-2, "power": -2e-3,
          "base_height": -20.0}
OUTPUTS = {"base_lin_vel": 3, "base_ang_vel": 3, "projected_gravity": 3, "filtered_lin_vel": 3, "filtered_ang_vel": 3, "obs": W, "priv": 4, "term": 14,
           "total": 1}


def bytes_per_call(N):
    """from the shapes: float32 [N, R] blocks, the root rows, the per-environment scalars and every output"""
    nr = N * R * 4
    reads = 13 * 4 * N + 4 * nr + 2 * nr + (3 + 3 + 6) * 4 * N + CX * 4 * N + 3 * 4 * N          # root, q qd a tau, last_a last_qd, filters last_rv, extra, ground steps tick
    writes = 2 * nr + (3 + 3 + 6 + 1) * 4 * N + (15 + W + 4 + 14 + 1 + 1) * 4 * N                 # the roll-over and the tick; the ten outputs
    return reads + writes


def unrotate(torch, q, v):
    """a world vector in the body frame of the xyzw quaternion q: the operations of the reference's quat_rotate_inverse"""
    w, u = q[:, 3:4], q[:, :3]
    return v * (2.0 * w ** 2 - 1.0) - torch.cross(u, v, dim=-1) * w * 2.0 + u * (u * v).sum(dim=-1, keepdim=True) * 2.0


def compose(torch, d, st, tab, noise):
    """one step as torch operations; ``st``: the five state tensors, ``tab``: the configuration tensors -> the outputs"""
    def noisy(x, block):
        if not noise:
            return x
        mu, var = NOISE[block]["range"]
        return x + (mu + var * torch.randn_like(x))

    nm = CFG["normalization"]
    fw = CFG["filter_weight"]
    root = d["root_states"]
    quat = root[:, 3:7]
    lin, ang, grav = unrotate(torch, quat, root[:, 7:10]), unrotate(torch, quat, root[:, 10:13]), unrotate(torch, quat, tab["gravity"])
    st["flv"][:] = lin * fw + st["flv"] * (1.0 - fw)
    st["fav"][:] = ang * fw + st["fav"] * (1.0 - fw)
    height = root[:, 2] - d["ground"]
    done = (root[:, 7:13].square().sum(dim=-1) > CFG["terminate_vel"]).int() + 2 * (height < CFG["terminate_height"]).int() \
        + 4 * (d["episode_steps"] > CFG["max_episode_steps"]).int()
    q, qd, act, tau = d["dof_pos"], d["dof_vel"], d["actions"], d["mean_torques"]
    term = torch.stack([torch.square(st["flv"][:, 2]), torch.sum(torch.square(ang[:, :2]), dim=-1), torch.sum(torch.square(grav[:, :2]), dim=-1),
                        torch.sum(torch.square(tau), dim=-1), torch.sum(torch.square(qd), dim=-1), torch.sum(torch.square((st["ldv"] - qd) / DT), dim=-1),
                        torch.sum(torch.square((st["lrv"] - root[:, 7:13]) / DT), dim=-1), torch.sum(torch.square(st["la"] - act), dim=-1),
                        torch.sum(((q < tab["lower"]) | (q > tab["upper"])).float(), dim=-1),
                        torch.sum((torch.abs(qd) - tab["vel_lim"] * CFG["soft_dof_vel_limit"]).clip(min=0.0, max=1.0), dim=-1),
                        torch.sum((torch.abs(tau) - tab["tq_lim"] * CFG["soft_torque_limit"]).clip(min=0.0), dim=-1),
                        torch.sum(torch.square(tau / tab["tq_lim"]).clip(max=1.0), dim=-1), torch.sum((tau * qd).clip(min=0.0), dim=-1),
                        torch.square(height - CFG["base_height_target"])], dim=1)
    total = torch.zeros_like(height)
    for k, name in enumerate(SCALES):
        total += term[:, k] * SCALES[name]
    obs = torch.cat((noisy(grav, "gravity") * nm["gravity"], noisy(ang, "ang_vel") * nm["ang_vel"], d["extra"], noisy(q - tab["default"], "dof_pos") * nm["dof_pos"],
                     noisy(qd, "dof_vel") * nm["dof_vel"], act), dim=-1)
    priv = torch.cat((noisy(lin, "lin_vel") * nm["lin_vel"], noisy(height, "height").unsqueeze(-1)), dim=-1)
    st["la"][:] = act
    st["ldv"][:] = qd
    st["lrv"][:] = root[:, 7:13]
    return {"base_lin_vel": lin, "base_ang_vel": ang, "projected_gravity": grav, "filtered_lin_vel": st["flv"], "filtered_ang_vel": st["fav"], "obs": obs,
            "priv": priv, "term": term, "total": total, "done": done}


def tables(rng):
    pose = rng.uniform(-0.5, 0.5, R).astype(np.float32)
    lim = np.sort(rng.uniform(-2.0, 2.0, (R, 2)), axis=1).astype(np.float32)
    lim[:, 1] += np.float32(0.5)
    return pose, lim, rng.uniform(3, 12, R).astype(np.float32), rng.uniform(10, 60, R).astype(np.float32)


def host_inputs(rng, N):
    quat = rng.standard_normal((N, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    x = {"root_states": np.concatenate([rng.uniform(-3, 3, (N, 2)), rng.uniform(0.2, 0.9, (N, 1)), quat, rng.normal(0, 1.5, (N, 3)), rng.normal(0, 2.0, (N, 3))], axis=1),
         "dof_pos": rng.uniform(-2.2, 2.7, (N, R)), "dof_vel": rng.normal(0, 6.0, (N, R)), "actions": np.clip(rng.normal(0, 0.8, (N, R)), -1, 1),
         "mean_torques": rng.normal(0, 25.0, (N, R)), "extra": rng.uniform(-1, 1, (N, CX)), "ground": rng.uniform(-0.1, 0.3, N)}
    x = {k: a.astype(np.float32) for k, a in x.items()}
    x["episode_steps"] = rng.integers(0, 600, N).astype(np.int32)
    return x


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 1048576])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition even when torch is importable")
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    if args.reps < 50:
        ap.error("--reps: the mean of at least 50 repetitions")
    from general_motion_retargeting_amd import MotionTracker, _lib as hip
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    hip.require_gpu()
    S, T = 8, 64
    B = S * T
    rng = np.random.default_rng(0)
    w = rng.normal(size=(B, 4))
    bufs = [hip.DeviceBuffer.from_host(a) for a in (rng.normal(0, 0.5, size=(B, 3)), w / np.linalg.norm(w, axis=1, keepdims=True), rng.uniform(-1.2, 1.2, size=(B, NDOF)))]
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
    pose, lim, vlim, tlim = tables(rng)
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "R": R, "extra_cols": CX, "row_width": W, "noise": "six gaussian blocks", "reps": args.reps,
           "rounds": args.rounds, "hbm_peak_bytes_per_s": HBM_PEAK,
           "composition": "torch " + torch.__version__ if torch else "not run (torch not importable, no GPU in it, or --no-torch)", "N": {}}
    for N in args.sizes:
        def new_tracker():
            trk = MotionTracker(lib, N, DT, dmap, np.zeros(R, np.float32), loop=True, seed=1)
            trk.set_proprio(pose, lim, vlim, tlim, noise=NOISE, scales=SCALES, **CFG)
            return trk

        trk = new_tracker()
        host = host_inputs(rng, N)
        outs = {k: np.zeros((N, c) if c > 1 else N, np.float32) for k, c in OUTPUTS.items()}
        outs["done"] = np.zeros(N, np.int32)
        if torch:
            d = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
            o = {k: torch.from_numpy(a).cuda() for k, a in outs.items()}
        else:
            d = {k: hip.DeviceBuffer.from_host(a) for k, a in host.items()}
            o = {k: hip.DeviceBuffer.from_host(a) for k, a in outs.items()}

        def fused(t=trk, noise=True):
            t.proprio_dev(**d, noise=noise, stream=stream, **o)

        nbytes = bytes_per_call(N)
        ff, cc = [], []
        if torch:
            def zeros(*shape):
                return torch.zeros(*shape, device="cuda")

            def new_state():
                return {"flv": zeros(N, 3), "fav": zeros(N, 3), "lrv": zeros(N, 6), "la": zeros(N, R), "ldv": zeros(N, R)}

            half = 0.5 * (1 - CFG["soft_dof_pos_limit"])
            tl = torch.from_numpy(lim).cuda()
            tab = {"gravity": torch.tensor([0.0, 0.0, -1.0], device="cuda").repeat(N, 1), "default": torch.from_numpy(pose).cuda(),
                   "lower": tl[:, 0] + half * (tl[:, 1] - tl[:, 0]), "upper": tl[:, 1] - half * (tl[:, 1] - tl[:, 0]),
                   "vel_lim": torch.from_numpy(vlim).cuda(), "tq_lim": torch.from_numpy(tlim).cuda()}
            st = new_state()
            comp = {}

            def composed():
                comp.update(compose(torch, d, st, tab, True))
        for _ in range(args.rounds):                                   # alternated
            ff.append(timed(fused, args.reps))
            if torch:
                cc.append(timed(composed, args.reps))
        r = {"elements": N * R, "proprio_dev": dict(figure(ff, nbytes), launches=1)}
        if torch:
            r["torch_step"] = figure(cc)
            r["composition_over_fused"] = r["torch_step"]["us"] / r["proprio_dev"]["us"]
            # noise off, one step of either path from a fresh state
            fresh = new_tracker()
            fused(fresh, False)
            clean = compose(torch, d, new_state(), tab, False)
            torch.cuda.synchronize()
            diff = {k: float((clean[k].float() - o[k].float()).abs().max()) for k in OUTPUTS}
            diff["done"] = int((clean["done"] != o["done"]).sum())
            r["largest_difference_noise_off"] = diff
            fresh.close()
        doc["N"][str(N)] = r
        trk.close()
        del d, o
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
