"""Tracker episode: device-event times of ``MotionTracker.rewards_dev`` -- without and with the episode statistics --,
of ``MotionTracker.reset_states_dev`` masked by the reward call's ``reset`` word and of the two back to back (the end of one step and the
start of the next episode), beside the same steps written as torch operations on the same tensors, in one run.

  per N in {4 096, 65 536, 1 048 576}:
     rewards_dev            one launch                      the 32 columns of the four blocks and 2 of the caller's, two groups
     rewards_dev_stats      two launches                    with the Recorder's episode sums
     reset_states_dev       one launch                      masked by ``reset``, 21 dofs, three uniform specs, the yaw, the delay
     episode_step           the three launches of a step    against   ``compose``: the weighted columns, the two sums, the clip and the
                                                            total; the Recorder WITH ITS PYTHON LOOP (one ``.item()`` per finished
                                                            environment and per key, booster_gym/utils/recorder.py:36-53); then
                                                            ``nonzero`` with its size read-back and the index-assigned resets of
                                                            booster_gym/envs/t1.py:316-340

Every call resets one environment in 512 (at least one), the same ones, so every repetition does the same work.  Every figure is the mean
of ``--reps`` (at least 50) repetitions between two device events on torch's current stream after a warm-up; fused and composed are timed
alternately, ``--rounds`` times each, and the spread over the rounds is printed beside the mean (the composition, whose Python loop takes
long at the largest N, runs fewer repetitions: the document says how many).  The composition is the yardstick; without torch on a GPU only
the fused calls are timed (on device buffers of this library) and the document says so.  Prints one JSON document; --out writes it to a file
as well.
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

NDOF, DT, NB, E = 21, 0.02, 13, 2
WIDTHS = {"term": 6, "proprio_term": 14, "feet_term": 8, "cmd_term": 4, "extra": E}
C = sum(WIDTHS.values())
LOC_W, IMI_W = 0.1, 1.0
UNI = {"init_dof_pos": {"distribution": "uniform", "operation": "additive", "range": (-0.1, 0.1)},
       "init_base_pos_xy": {"distribution": "uniform", "operation": "additive", "range": (-1.0, 1.0)},
       "init_base_lin_vel_xy": {"distribution": "uniform", "operation": "additive", "range": (-0.5, 0.5)}}
DECIMATION = 10


def reward_bytes(N, stats):
    """from the shapes: the C term columns, done and flags in; reward, scaled, the two totals, reset and time_outs out; with the statistics
    the episode sums and steps both ways"""
    return (C * 4 + 8) * N + (4 + C * 4 + 8 + 8) * N + (2 * ((C + 1) * 4 + 4) * N if stats else 0)


def compose(torch, d, st):
    """the end of a step and the resets it causes as torch operations on the same tensors"""
    terms = torch.cat([d[k] for k in WIDTHS], dim=1)
    scaled = terms * st["w"]
    loc = (scaled * st["g0"]).sum(1).clip(min=0.0)
    imi = (scaled * st["g1"]).sum(1)
    rew = LOC_W * loc + IMI_W * imi
    reset = d["done"] != 0
    time_outs = ((d["done"] & 4) | (d["flags"] & 1)) != 0
    # the Recorder (recorder.py:36-53)
    if st["started"]:
        st["ep_steps"] += 1
    st["started"] = True
    fin = []
    for val in st["ep_steps"][reset]:
        fin.append(val.item())
    st["ep_steps"][reset] = 0
    for k in range(C + 1):
        st["ep_sum"][k] += rew if k == 0 else scaled[:, k - 1]
        for v in st["ep_sum"][k][reset]:
            fin.append(v.item())
        st["ep_sum"][k][reset] = 0
    # the resets (t1.py:485, :316-340)
    ids = reset.nonzero(as_tuple=False).flatten()
    n = len(ids)                                               # a size read-back
    if n:
        dev = rew.device
        d["dof_pos"][ids] = st["default"] + (-0.1 + 0.2 * torch.rand_like(st["default"]))
        d["dof_vel"][ids] = 0.0
        d["root_states"][ids] = st["base"]
        d["root_states"][ids, :2] += st["origins"][ids]
        d["root_states"][ids, :2] = d["root_states"][ids, :2] + (-1.0 + 2.0 * torch.rand(n, 2, device=dev))
        yaw = torch.rand(n, device=dev) * (2 * torch.pi)
        zero = torch.zeros_like(yaw)
        d["root_states"][ids, 3:7] = torch.stack([zero, zero, torch.sin(0.5 * yaw), torch.cos(0.5 * yaw)], dim=1)
        d["root_states"][ids, 7:9] = torch.zeros(n, 2, device=dev) + (-0.5 + 1.0 * torch.rand(n, 2, device=dev))
        d["episode_steps"][ids] = 0
        d["delay_steps"][ids] = torch.randint(0, DECIMATION, (n,), device=dev, dtype=d["delay_steps"].dtype)
    return rew, time_outs, fin


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
    doc = {"backend": hip.lib().gmr_backend_info().decode(), "columns": C, "dofs": NDOF, "resets_per_call": "one environment in 512, at least one",
           "reps": args.reps, "rounds": args.rounds, "hbm_peak_bytes_per_s": HBM_PEAK,
           "composition": "torch " + torch.__version__ + ", the Recorder's Python loop over the finished environments and the nonzero read-back" if torch else
           "not run (torch not importable, no GPU in it, or --no-torch)", "N": {}}
    pose = rng.uniform(-0.5, 0.5, NDOF).astype(np.float32)
    base = np.array([0, 0, 0.72, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32)
    lim = np.stack([-np.ones(NDOF), np.ones(NDOF)], axis=1).astype(np.float32)
    for N in args.sizes:
        done = np.zeros(N, np.int32)
        done[::512] = 1
        host = {k: rng.uniform(0, 1, (N, wd)).astype(np.float32) for k, wd in WIDTHS.items()}
        host.update({"done": done, "flags": rng.integers(0, 2, N).astype(np.int32), "root_states": rng.normal(0, 1, (N, 13)).astype(np.float32),
                     "dof_pos": rng.normal(0, 1, (N, NDOF)).astype(np.float32), "dof_vel": rng.normal(0, 1, (N, NDOF)).astype(np.float32),
                     "delay_steps": np.zeros(N, np.int32), "episode_steps": np.full(N, 7, np.int32)})
        outs = {"reward": np.zeros(N, np.float32), "scaled": np.zeros((N, C), np.float32), "group_total": np.zeros((N, 2), np.float32),
                "reset": np.zeros(N, np.int32), "time_outs": np.zeros(N, np.int32)}
        origins = rng.uniform(0, 50, (N, 2)).astype(np.float32)
        up = (lambda a: torch.from_numpy(a).cuda()) if torch else hip.DeviceBuffer.from_host
        d, o = ({k: up(a) for k, a in t.items()} for t in (host, outs))
        r = {}
        trackers = {}
        for stats in (False, True):
            trk = MotionTracker(lib, N, DT, None, None, loop=True, seed=1)
            trk.set_proprio(pose, lim, np.full(NDOF, 10.0, np.float32), np.full(NDOF, 30.0, np.float32), base_height_target=0.68, terminate_vel=50.0,
                            terminate_height=0.3, max_episode_steps=1000, scales={"lin_vel_z": -2.0, "torques": -2e-4, "base_height": -20.0})
            trk.set_feet((4, 9), np.array([[0.12, 0.05, -0.03]], np.float32), NB, feet_distance_ref=0.2, swing_period=0.2,
                         scales={"feet_slip": -0.1, "feet_swing": 3.0})
            trk.set_commands((-1.0, 1.0), (-0.5, 0.5), (-1.0, 1.0), (1.0, 2.0), (250, 500), scales=(0.025, 1.0, 1.0, 0.5))
            trk.set_reset_states(base, pose, env_origins=origins, decimation=DECIMATION, **UNI)
            layout = trk.set_rewards(extra_names=("smooth", "alive"), extra_weights=(0.5, 0.1), groups={k: 3 for k in ("root_pos", "root_rot", "root_vel",
                                     "root_ang_vel", "dof_pos", "dof_vel")}, group_weight=(LOC_W, IMI_W), only_positive=(True, False), stats=stats)
            assert layout["num_cols"] == C
            trackers[stats] = trk
        ins = {k: d[k] for k in list(WIDTHS) + ["done", "flags"]}

        def reward(stats):
            trackers[stats].rewards_dev(**ins, stream=stream, **o)

        def reset(t=trackers[True]):
            t.reset_states_dev(d["root_states"], d["dof_pos"], d["dof_vel"], mask=o["reset"], delay_steps=d["delay_steps"], episode_steps=d["episode_steps"],
                               stream=stream)

        def fused():
            reward(True)
            reset()

        composed = None
        if torch:
            dev = torch.device("cuda")
            g0 = np.ones(C, np.float32)
            g1 = np.zeros(C, np.float32)
            g1[:6] = 1
            st = {"w": torch.from_numpy(rng.uniform(-1, 1, C).astype(np.float32)).to(dev), "g0": torch.from_numpy(g0).to(dev), "g1": torch.from_numpy(g1).to(dev),
                  "started": False, "ep_steps": torch.zeros(N, dtype=torch.int64, device=dev), "ep_sum": [torch.zeros(N, device=dev) for _ in range(C + 1)],
                  "default": torch.from_numpy(pose).to(dev).unsqueeze(0), "base": torch.from_numpy(base).to(dev), "origins": torch.from_numpy(origins).to(dev)}

            def composed(st=st):
                compose(torch, d, st)
        items = int(done.sum()) * (C + 2)
        creps = int(min(args.reps, max(3, 100000 // items)))
        f0, f1, fr, ff, cc = [], [], [], [], []
        for _ in range(args.rounds):                                   # alternated
            f0.append(timed(lambda: reward(False), args.reps))
            f1.append(timed(lambda: reward(True), args.reps))
            fr.append(timed(reset, args.reps))
            ff.append(timed(fused, args.reps))
            if composed:
                cc.append(timed(composed, creps, warm=1))
        r["rewards_dev"] = dict(figure(f0, reward_bytes(N, False)), launches=1)
        r["rewards_dev_stats"] = dict(figure(f1, reward_bytes(N, True)), launches=2)
        r["reset_states_dev"] = dict(figure(fr), launches=1, reset_environments=int(done.sum()))
        r["episode_step"] = dict(figure(ff), launches=3)
        if composed:
            r["torch_episode_step"] = dict(figure(cc), reps=creps, item_reads_per_call=items)
            r["composition_over_fused"] = r["torch_episode_step"]["us"] / r["episode_step"]["us"]
        stats_out = trackers[True].reward_stats(raw=True)
        r["episodes_counted"] = stats_out["episodes"]
        for trk in trackers.values():
            trk.close()
        doc["N"][str(N)] = r
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
