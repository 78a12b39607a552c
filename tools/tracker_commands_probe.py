"""Tracker commands: device-event times of ``MotionTracker.commands_dev`` -- without and with the curriculum -- and of
``MotionTracker.disturb_dev`` on a push-start step, beside the same steps written as torch operations on the same tensors, in one run.

  per N in {4 096, 65 536, 1 048 576}:
     commands_dev   one launch (three with the curriculum)   against   ``compose``: the four terms and their weighted sum, the boundary flag,
                                                                        the curriculum's bookkeeping WITH THE REFERENCE'S PYTHON LOOP over the
                                                                        reset environments (one device read per environment and per branch,
                                                                        booster_gym/envs/t1.py:400-412), the reset of the resample time, the
                                                                        resample with ``nonzero`` and its size read-back, ``multinomial``,
                                                                        ``randperm`` and ``randint`` (:362-389, :415-435), the command columns
                                                                        of the observation row
     disturb_dev    one launch                                against   ``compose_push``: two randomisations of zeros written into the base
                                                                        body's rows of the [N, nb, 3] tensors, the six push columns

Every call resets one environment in 512 (at least one): those reset, succeed where their velocities allow, and resample; nobody else meets
its resample time, so every repetition does the same work.  Every figure is the mean of ``--reps`` (at least 50) repetitions between two
device events on torch's current stream after a warm-up; fused and composed are timed alternately, ``--rounds`` times each, and the spread
over the rounds is printed beside the mean (``--compose-reps`` shortens the composition alone, whose Python loop takes long at the largest
N; the document says what was used).  The composition is the yardstick; without torch on a GPU only the fused calls are timed (on device
buffers of this library) and the document says so.  Prints one JSON document; --out writes it to a file as well.
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

NDOF, DT, NB, BASE, W = 21, 0.02, 13, 0, 80
L, A = 10, 10
RANGES = dict(lin_vel_x=(-1.0, 1.0), lin_vel_y=(-0.5, 0.5), ang_vel_yaw=(-1.0, 1.0), gait_frequency=(1.0, 2.0), resample_steps=(250, 500))
COMMON = dict(still_proportion=0.1, tracking_sigma=0.25, scales=(0.025, 1.0, 1.0, 0.5), obs_scales=(1.0, 1.0, 1.0))
CUR = dict(lin_vel_levels=L, ang_vel_levels=A, update_rate=0.125, tolerances=(0.2, 0.2, 0.2), resolutions=(0.2, 0.1, 0.2), min_success_steps=450)
KICK_EVERY, PUSH_EVERY, PUSH_DURATION, PUSH_STEP = 7, 10, 3, 10
PUSH = dict(push_force={"distribution": "gaussian", "operation": "additive", "range": (0.0, 10.0)},
            push_torque={"distribution": "gaussian", "operation": "additive", "range": (0.0, 2.0)},
            kick_lin_vel={"distribution": "gaussian", "operation": "additive", "range": (0.0, 0.1)})


def bytes_per_call(N, curriculum):
    """from the shapes: steps, done, the two velocity rows, commands, gait and the resample time in; terms, total, commands, gait, flags and
    the three observation columns out (the resampling environments' state writes are one in 512 and left out); with the curriculum the carry
    word both ways"""
    return (4 + 4 + 24 + 12 + 4 + 4) * N + (16 + 4 + 12 + 4 + 4 + 12) * N + (8 * N if curriculum else 0)


def compose(torch, d, st, cur):
    """one call as torch operations; ``st``: the state tensors; ``cur``: the curriculum's configuration or None"""
    steps, done, f, g = d["episode_steps"], d["done"], d["lin_vel"], d["ang_vel"]
    c, rt = st["commands"], st["resample_time"]
    sigma = COMMON["tracking_sigma"]
    term = torch.stack([torch.ones_like(c[:, 0]), torch.exp(-torch.square(c[:, 0] - f[:, 0]) / sigma), torch.exp(-torch.square(c[:, 1] - f[:, 1]) / sigma),
                        torch.exp(-torch.square(c[:, 2] - g[:, 2]) / sigma)], dim=1)
    total = term @ st["scales"]
    flags = (steps == rt).int()
    ids = done.nonzero(as_tuple=False).flatten()
    if cur is not None:
        ok = steps[ids] > cur["min_success_steps"]
        ok &= torch.abs(f[ids, 0] - c[ids, 0]) < cur["tolerances"][0]
        ok &= torch.abs(f[ids, 1] - c[ids, 1]) < cur["tolerances"][1]
        ok &= torch.abs(g[ids, 2] - c[ids, 2]) < cur["tolerances"][2]
        prob, rate = st["prob"], cur["update_rate"]
        for i in range(len(ids)):                              # the reference's loop: the host reads the device once per branch
            if ok[i]:
                x, y = st["level"][ids[i], 0] + L, st["level"][ids[i], 1] + A
                prob[x, y] += rate
                if x > 0:
                    prob[x - 1, y] += rate
                if x < prob.shape[0] - 1:
                    prob[x + 1, y] += rate
                if y > 0:
                    prob[x, y - 1] += rate
                if y < prob.shape[1] - 1:
                    prob[x, y + 1] += rate
        prob.clamp_(max=1.0)
        flags[ids] |= ok.int() * 4
    rt[ids] = 0
    now = torch.where(done != 0, torch.zeros_like(steps), steps)
    rs = (now == rt).nonzero(as_tuple=False).flatten()
    n = len(rs)                                                # a size read-back
    if n:
        u = torch.rand(4, n, device=c.device)
        if cur is not None:
            cell = torch.multinomial(st["prob"].flatten(), n, replacement=True)
            lin, ang = cell // st["prob"].shape[1] - L, cell % st["prob"].shape[1] - A
            st["level"][rs, 0], st["level"][rs, 1] = lin, ang
            res = cur["resolutions"]
            c[rs, 0] = (lin + (u[0] - 0.5)) * res[0]
            c[rs, 1] = torch.abs(lin) * (2.0 * u[1] - 1.0) * res[1]
            c[rs, 2] = (ang + (u[2] - 0.5)) * res[2]
        else:
            for k, name in enumerate(("lin_vel_x", "lin_vel_y", "ang_vel_yaw")):
                lo, hi = RANGES[name]
                c[rs, k] = (hi - lo) * u[k] + lo
        lo, hi = RANGES["gait_frequency"]
        st["gait"][rs] = (hi - lo) * u[3] + lo
        still = rs[torch.randperm(n, device=c.device)[: int(COMMON["still_proportion"] * n)]]
        c[still, :] = 0.0
        st["gait"][still] = 0.0
        rt[rs] += torch.randint(RANGES["resample_steps"][0], RANGES["resample_steps"][1], (n,), device=c.device, dtype=rt.dtype)
        flags[rs] |= 2
    d["obs"][:, 6:9] = c * st["obs_scale"]
    return {"term": term, "total": total, "flags": flags}


def compose_push(torch, d):
    """a push start as torch operations: the two randomisations of zeros, the base body's rows, the six observation columns"""
    N = d["forces"].shape[0]
    force = 0.0 + 10.0 * torch.randn(N, 3, device=d["forces"].device)
    torque = 0.0 + 2.0 * torch.randn(N, 3, device=d["forces"].device)
    d["forces"][:, BASE, :] = force
    d["torques"][:, BASE, :] = torque
    d["push_obs"][:] = torch.cat([force * 1.0, torque * 1.0], dim=1)


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
    creps = args.compose_reps or args.reps
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "grid": [2 * L + 1, 2 * A + 1], "resets_per_call": "one environment in 512, at least one",
           "reps": args.reps, "composition_reps": creps, "rounds": args.rounds, "hbm_peak_bytes_per_s": HBM_PEAK,
           "composition": "torch " + torch.__version__ + ", the reference's Python loop over the reset environments and its size read-backs" if torch else
           "not run (torch not importable, no GPU in it, or --no-torch)", "N": {}}
    for N in args.sizes:
        done = np.zeros(N, np.int32)
        done[::512] = 1
        host = {"episode_steps": np.where(done != 0, 480, -1).astype(np.int32), "done": done, "lin_vel": rng.normal(0, 0.1, (N, 3)).astype(np.float32),
                "ang_vel": rng.normal(0, 0.1, (N, 3)).astype(np.float32)}
        outs = {"term": np.zeros((N, 4), np.float32), "total": np.zeros(N, np.float32), "commands": np.zeros((N, 3), np.float32),
                "gait_frequency": np.zeros(N, np.float32), "flags": np.zeros(N, np.int32)}
        extra = {"obs": np.zeros((N, W), np.float32), "forces": np.zeros((N, NB, 3), np.float32), "torques": np.zeros((N, NB, 3), np.float32),
                 "push_obs": np.zeros((N, 6), np.float32), "root_states": np.zeros((N, 13), np.float32)}
        if torch:
            up = lambda a: torch.from_numpy(a).cuda()                                       # noqa: E731
            address = lambda x: x.data_ptr()                                                # noqa: E731
        else:
            up = hip.DeviceBuffer.from_host
            address = lambda x: x.ptr.value                                                 # noqa: E731
        d, o, x = ({k: up(a) for k, a in t.items()} for t in (host, outs, extra))
        r = {}
        for tag, cur in (("commands_dev", None), ("commands_dev_curriculum", CUR)):
            trk = MotionTracker(lib, N, DT, None, None, loop=True, seed=1)
            trk.set_commands(**RANGES, **COMMON, curriculum=cur)

            def fused(t=trk):
                t.commands_dev(d["episode_steps"], d["done"], d["lin_vel"], d["ang_vel"], cmd_obs=address(x["obs"]) + 24, cmd_obs_stride=W, stream=stream, **o)

            ff, cc = [], []
            if torch:
                dev = torch.device("cuda")
                st = {"commands": torch.zeros(N, 3, device=dev), "gait": torch.zeros(N, device=dev), "resample_time": torch.zeros(N, dtype=torch.int32, device=dev),
                      "scales": torch.tensor(COMMON["scales"], device=dev), "obs_scale": torch.tensor(COMMON["obs_scales"], device=dev),
                      "level": torch.zeros(N, 2, dtype=torch.int64, device=dev), "prob": torch.zeros(2 * L + 1, 2 * A + 1, device=dev)}
                st["prob"][L, A] = 1.0
                dd = dict(d, obs=x["obs"])

                def composed(st=st, cur=cur, dd=dd):
                    compose(torch, dd, st, cur)
            for _ in range(args.rounds):                                   # alternated
                ff.append(timed(fused, args.reps))
                if torch:
                    cc.append(timed(composed, creps))
            r[tag] = dict(figure(ff, bytes_per_call(N, cur is not None)), launches=3 if cur else 1)
            if torch:
                r[tag.replace("commands_dev", "torch_commands")] = figure(cc)
                r[tag + "_composition_over_fused"] = figure(cc)["us"] / r[tag]["us"]
            trk.close()
        trk = MotionTracker(lib, N, DT, None, None, loop=True, seed=1)
        trk.set_disturbances(KICK_EVERY, PUSH_EVERY, PUSH_DURATION, **PUSH)

        def push(t=trk):
            t.disturb_dev(PUSH_STEP, x["root_states"], push_force=address(x["forces"]) + 12 * BASE, push_torque=address(x["torques"]) + 12 * BASE,
                          push_obs=x["push_obs"], push_force_stride=NB * 3, push_torque_stride=NB * 3, stream=stream)

        assert MotionTracker.disturb_actions(PUSH_STEP, KICK_EVERY, PUSH_EVERY, PUSH_DURATION) == 2
        ff, cc = [], []
        for _ in range(args.rounds):
            ff.append(timed(push, args.reps))
            if torch:
                cc.append(timed(lambda: compose_push(torch, x), args.reps))
        r["disturb_dev_push_start"] = dict(figure(ff, 12 * 4 * N), launches=1)
        if torch:
            r["torch_push_start"] = figure(cc)
            r["push_composition_over_fused"] = r["torch_push_start"]["us"] / r["disturb_dev_push_start"]["us"]
        trk.close()
        doc["N"][str(N)] = r
        del d, o, x
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
