"""Tracker feet: device-event times of ``MotionTracker.feet_dev`` beside the same computation written as torch
operations on the same tensors, in one run.

  tracker    nb = 13 rigid bodies, the T1's four edge points per foot, 9 penalised and 2 termination bodies, dt = 0.02, a 400 x 300 field
  per N in {4 096, 65 536, 1 048 576}:
     feet_dev   one launch   against   the reference's lines as torch operations (``compose``): the feet pose and the two euler angles, the
                                       rotated edge points, the terrain height under them and under the root THROUGH THE HOST as the
                                       reference has it (positions to the host, NumPy interpolation, upload: booster_gym/utils/terrain.py:101-121), the
                                       gait clock and its two columns, the eight terms and their weighted sum, the contact-force
                                       termination, the roll-over of last_feet_pos

Every figure is the mean of ``--reps`` (at least 50) repetitions between two device events on torch's current stream after a warm-up;
fused and composed are timed alternately, ``--rounds`` times each, and the spread over the rounds is printed beside the mean
(``--compose-reps`` shortens the composition alone, whose round trip takes seconds at the largest N; the document says what was used).  The
bytes of a call are counted from the shapes.  The two paths make one step from the same state and the largest difference of their outputs
is reported.  The composition is the yardstick; without torch on a GPU only the fused call is timed (on device buffers of this library).
Prints one JSON document; --out writes it to a file as well.
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

NB, NDOF, DT = 13, 21, 0.02
FEET, TERMINATION, PENALIZED = (5, 11), (0, 1), (2, 3, 4, 6, 7, 8, 9, 10, 12)
EDGES = np.array([[0.1215, 0.05, -0.03], [0.1215, -0.05, -0.03], [-0.1015, 0.05, -0.03], [-0.1015, -0.05, -0.03]], np.float32)
E = len(EDGES)
NX, NY, BORDER, HS, VS = 400, 300, 50, 0.1, 0.005
CFG = dict(feet_distance_ref=0.2, swing_period=0.2)
SCALES = {"collision": -1.0, "feet_slip": -0.1, "feet_vel_z": -0.05, "feet_roll": -0.2, "feet_yaw_diff": -1.0, "feet_yaw_mean": -1.0, "feet_distance": -10.0,
          "feet_swing": 3.0}
OUTPUTS = {"feet_pos": 6, "feet_roll": 2, "feet_yaw": 2, "ground": 1, "gait": 2, "term": 8, "total": 1}


def bytes_per_call(N):
    """from the shapes: the two feet rows of the body tensor, the listed force rows, the root's seven floats, the per-environment scalars,
    four int16 gathers per edge point and per root, the state both ways and every output"""
    reads = 2 * 7 * 4 * N + (len(TERMINATION) + len(PENALIZED)) * 12 * N + 7 * 4 * N + 2 * 4 * N + (2 * E + 1) * 4 * 2 * N + 7 * 4 * N
    writes = 7 * 4 * N + (sum(OUTPUTS.values()) + 2 + 1) * 4 * N
    return reads + writes


def remainder_pi(torch, a):
    """an angle brought into [-pi, pi)"""
    return torch.remainder(a + np.pi, 2 * np.pi) - np.pi


def roll_of(torch, q):
    """rotation about x of an xyzw quaternion ``[..., 4]``, in [0, 2 pi)"""
    x, y, z, w = q.unbind(-1)
    return torch.remainder(torch.atan2(2.0 * (w * x + y * z), w * w - x * x - y * y + z * z), 2 * np.pi)


def yaw_of(torch, q):
    """rotation about z of an xyzw quaternion ``[..., 4]``, in [0, 2 pi)"""
    x, y, z, w = q.unbind(-1)
    return torch.remainder(torch.atan2(2.0 * (w * z + x * y), w * w + x * x - y * y - z * z), 2 * np.pi)


def turn(torch, q, v):
    """``v [..., 3]`` rotated by the xyzw quaternion ``q [..., 4]`` (broadcast over the leading axes)"""
    u, w = q[..., :3], q[..., 3:]
    q, v = torch.broadcast_tensors(u, v)
    return (2.0 * w * w - 1.0) * v + 2.0 * w * torch.linalg.cross(q, v) + 2.0 * (q * v).sum(-1, keepdim=True) * q


def heights_through_the_host(torch, field, xy):
    """The yardstick's terrain height of ``xy [M, 2]``: what a caller without ``terrain_heights_dev`` does, and what the reference does --
    the positions go to the host, the bilinear interpolation of the int16 field runs in NumPy, the result is uploaded."""
    pix = BORDER + xy.detach().cpu().numpy().astype(np.float64) / HS
    cell = np.floor(pix)
    frac = pix - cell
    i, j = cell[:, 0].astype(np.int64), cell[:, 1].astype(np.int64)
    near = field[i, j] + frac[:, 0] * (field[i + 1, j].astype(np.float64) - field[i, j])            # along x at the cell's near y
    far = field[i, j + 1] + frac[:, 0] * (field[i + 1, j + 1].astype(np.float64) - field[i, j + 1])
    h = (near + frac[:, 1] * (far - near)) * VS
    return torch.from_numpy(h.astype(np.float32)).to(xy.device)


def compose(torch, d, st, tab, field):
    """one step as torch operations, one foot at a time; ``st``: the two state tensors -> the outputs"""
    N = d["root_states"].shape[0]
    bodies = d["body_state"].view(N, NB, 13)
    forces = d["contact_forces"].view(N, NB, 3)
    root, gf = d["root_states"], d["gait_frequency"]
    moving = gf > 1.0e-8
    # the gait clock and its two columns
    st["gait"].add_(DT * gf).fmod_(1.0)
    phase = st["gait"]
    gait = torch.stack([torch.cos(2 * np.pi * phase), torch.sin(2 * np.pi * phase)], dim=1) * moving.float().unsqueeze(1)
    # per foot: pose, angles, the edge points against the terrain under them, the velocity since the last step
    pos, roll, yaw, touching, speed2, rise2 = [], [], [], [], [], []
    for f, body in enumerate(FEET):
        p, q = bodies[:, body, 0:3], bodies[:, body, 3:7]
        corners = p.unsqueeze(1) + turn(torch, q.unsqueeze(1), tab["edges"].unsqueeze(0))          # [N, E, 3]
        under = heights_through_the_host(torch, field, corners.reshape(-1, 3)[:, :2]).view(N, E)
        touching.append((corners[..., 2] - under < 0.01).any(dim=1))
        v = (st["last"][:, f] - p) / DT
        speed2.append((v * v).sum(dim=1))
        rise2.append(v[:, 2] * v[:, 2])
        pos.append(p)
        roll.append(remainder_pi(torch, roll_of(torch, q)))
        yaw.append(remainder_pi(torch, yaw_of(torch, q)))
    ground = heights_through_the_host(torch, field, root[:, :2])
    heading = yaw_of(torch, root[:, 3:7])
    # the eight terms
    hard = torch.linalg.vector_norm(forces, dim=-1) > 1.0                                            # [N, NB]
    split = yaw[1] - yaw[0]
    middle = 0.5 * (yaw[0] + yaw[1]) + torch.where(split.abs() > np.pi, np.pi, 0.0)
    gap = pos[1] - pos[0]
    across = (torch.cos(heading) * gap[:, 1] - torch.sin(heading) * gap[:, 0]).abs()
    airborne = [(phase - c).abs() < 0.5 * CFG["swing_period"] for c in (0.25, 0.75)]
    term = torch.stack([hard[:, PENALIZED].sum(dim=1).float(),
                        (speed2[0] * touching[0] + speed2[1] * touching[1]) * (d["episode_steps"] > 1),
                        rise2[0] + rise2[1],
                        roll[0] ** 2 + roll[1] ** 2,
                        remainder_pi(torch, split) ** 2,
                        remainder_pi(torch, heading - middle) ** 2,
                        (CFG["feet_distance_ref"] - across).clamp(0.0, 0.1),
                        sum((airborne[f] & moving & ~touching[f]).float() for f in range(2))], dim=1)
    total = term @ tab["scales"]
    for f in range(2):
        st["last"][:, f] = pos[f]
    return {"feet_pos": torch.cat(pos, dim=1), "feet_roll": torch.stack(roll, dim=1), "feet_yaw": torch.stack(yaw, dim=1),
            "feet_contact": torch.stack(touching, dim=1).int(), "ground": ground, "gait": gait, "term": term, "total": total,
            "done": hard[:, TERMINATION].any(dim=1).int() * 8}


def host_inputs(rng, N, field):
    state = rng.normal(0, 1, (N, NB, 13))
    quat = rng.standard_normal((N, NB, 4))
    state[:, :, 3:7] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    x_hi, y_hi = (NX - 1 - BORDER) * HS, (NY - 1 - BORDER) * HS
    xy = np.stack([rng.uniform(0.5, x_hi - 0.5, (N, 2)), rng.uniform(0.5, y_hi - 0.5, (N, 2))], axis=-1)
    ij = np.floor(BORDER + xy / HS).astype(int)
    state[:, FEET, :2] = xy
    state[:, FEET, 2] = field[ij[..., 0], ij[..., 1]] * VS + rng.uniform(0.0, 0.09, (N, 2))
    root = np.concatenate([xy.mean(axis=1), rng.uniform(0.5, 0.8, (N, 1)), state[:, 0, 3:7], rng.normal(0, 1, (N, 6))], axis=1)
    forces = rng.normal(0, 0.6, (N, NB, 3))
    return {"body_state": state.reshape(N, NB * 13).astype(np.float32), "root_states": root.astype(np.float32),
            "contact_forces": forces.reshape(N, NB * 3).astype(np.float32), "episode_steps": rng.integers(0, 600, N).astype(np.int32),
            "gait_frequency": rng.uniform(1.0, 2.5, N).astype(np.float32)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--compose-reps", type=int, default=None, help="repetitions of the torch composition (default: --reps)")
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
    field = rng.integers(-20, 60, (NX, NY)).astype(np.int16)
    creps = args.compose_reps or args.reps
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "bodies": NB, "edge_points": E, "field": [NX, NY], "reps": args.reps, "composition_reps": creps,
           "rounds": args.rounds, "hbm_peak_bytes_per_s": HBM_PEAK,
           "composition": "torch " + torch.__version__ + ", heights through the host as the reference has them" if torch else
           "not run (torch not importable, no GPU in it, or --no-torch)", "N": {}}
    for N in args.sizes:
        def new_tracker():
            trk = MotionTracker(lib, N, DT, None, None, loop=True, seed=1)
            trk.set_terrain(field, HS, VS, BORDER)
            trk.set_feet(FEET, EDGES, NB, termination_bodies=TERMINATION, penalized_bodies=PENALIZED, scales=SCALES, **CFG)
            return trk

        trk = new_tracker()
        host = host_inputs(rng, N, field)
        outs = {k: np.zeros((N, c) if c > 1 else N, np.float32) for k, c in OUTPUTS.items()}
        outs["done"], outs["feet_contact"] = np.zeros(N, np.int32), np.zeros((N, 2), np.int32)
        if torch:
            d = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
            o = {k: torch.from_numpy(a).cuda() for k, a in outs.items()}
        else:
            d = {k: hip.DeviceBuffer.from_host(a) for k, a in host.items()}
            o = {k: hip.DeviceBuffer.from_host(a) for k, a in outs.items()}

        def fused(t=trk):
            t.feet_dev({"body_state": d["body_state"]}, d["root_states"], d["contact_forces"], d["episode_steps"], d["gait_frequency"], stream=stream, **o)

        nbytes = bytes_per_call(N)
        ff, cc = [], []
        if torch:
            def new_state():
                return {"last": torch.zeros(N, 2, 3, device="cuda"), "gait": torch.zeros(N, device="cuda")}

            tab = {"edges": torch.from_numpy(EDGES).cuda(), "scales": torch.tensor([SCALES[k] for k in SCALES], device="cuda")}
            st = new_state()
            comp = {}

            def composed():
                comp.update(compose(torch, d, st, tab, field))
        for _ in range(args.rounds):                                   # alternated
            ff.append(timed(fused, args.reps))
            if torch:
                cc.append(timed(composed, creps))
        r = {"feet_dev": dict(figure(ff, nbytes), launches=1)}
        if torch:
            r["torch_step"] = figure(cc)
            r["composition_over_fused"] = r["torch_step"]["us"] / r["feet_dev"]["us"]
            # one step of either path from a fresh state
            fresh = new_tracker()
            fused(fresh)
            clean = compose(torch, d, new_state(), tab, field)
            torch.cuda.synchronize()
            diff = {k: float((clean[k].float() - o[k].float().reshape(clean[k].shape)).abs().max()) for k in OUTPUTS}
            diff["done"] = int((clean["done"] != o["done"]).sum())
            diff["feet_contact"] = int((clean["feet_contact"] != o["feet_contact"]).sum())
            r["largest_difference"] = diff
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
