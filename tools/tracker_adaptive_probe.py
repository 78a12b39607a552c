"""Adaptive sampling and masked resets of the tracker: what the masked reset costs beside the path it replaces,
what the grown tracker state costs the steps, and what an Adapt costs.

  library   4 096 clips of 256 frames at 30 fps, G1 (29 dofs), loop off
  reset     N in {4 096, 65 536, 1 048 576}, 2 % of the environments done, a host clock around a device synchronise:
              masked    ``reset_done_dev(done=mask)``, one launch
              compact   the path without it: ``torch.nonzero`` on the mask, the read of its size, ``reset_dev`` on the list
  steps     ``step_dev`` with simulator state at N = 65 536 and ``step_links_dev`` (six links, training outputs), device events
  adapt     ``adapt_dev`` at bin_seconds 0.5 (73 728 bins) and 1 / 30 (1 048 576 bins), device events
  failing   the masked reset at N = 1 048 576 with every environment done and failed, all clocks in ONE bin against clocks spread over
            the library

Every leg runs in a child process of its own, so that ``--parent-tree`` (a checkout of the parent commit with its library built) and
``--variant-lib`` (a ``build_variant`` of this tree, through GMR_HIP_LIBRARY) are measured by the same lines; the children of the two
trees alternate, ``--rounds`` times each, and the spread over the rounds of one identical measurement is printed beside the mean.  The
parent's tree has no masked reset: its child times the compact path alone, which is the pass line's other leg.  Prints one JSON
document; --out writes it to a file as well.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time as clock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = ("left_ankle_roll_link", "right_ankle_roll_link", "left_wrist_yaw_link", "right_wrist_yaw_link", "torso_link", "head_link")


def timed(hip, st, fn, reps, warm=3):
    """seconds per call between two device events on one stream"""
    for _ in range(warm):
        fn()
    st.sync()
    a, b = hip.Event(), hip.Event()
    a.record(st)
    for _ in range(reps):
        fn()
    b.record(st)
    st.sync()
    return a.elapsed_ms(b) * 1e-3 / reps


def host_timed(fn, reps, warm=3):
    """seconds per call on the host clock; fn ends with a device synchronise"""
    for _ in range(warm):
        fn()
    t0 = clock.perf_counter()
    for _ in range(reps):
        fn()
    return (clock.perf_counter() - t0) / reps


def child(args):
    """one tree, one pass over every leg it has -> a JSON line on stdout"""
    sys.path.insert(0, args.tree)
    from general_motion_retargeting_amd import KinematicsModel, MotionTracker, ROBOT_XML_DICT, _lib as hip
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    hip.require_gpu()
    masked = hasattr(MotionTracker, "reset_done_dev")
    km = KinematicsModel(ROBOT_XML_DICT["unitree_g1"])
    ndof, S, T, dt = km.num_dof, args.clips, args.frames, 0.02
    B = S * T
    rng = np.random.default_rng(0)
    st = hip.Stream()
    w = np.cumsum(rng.normal(size=(S, T, 4)) * 0.05, axis=1) + rng.normal(size=(S, 1, 4))
    src = [rng.normal(0, 0.5, size=(B, 3)) + np.array([0.3, -0.2, 0.8]), (w / np.linalg.norm(w, axis=2, keepdims=True)).reshape(B, 4),
           rng.uniform(-1.2, 1.2, size=(B, ndof))]
    bufs = [hip.DeviceBuffer.from_host(a) for a in src]
    del src, w
    lib = MotionLibrary.from_device((np.arange(S + 1) * T).astype(np.int32), np.full(S, 30.0), ndof, 0, *bufs, None, stream=st)
    st.sync()
    out = {"masked_reset": masked, "library": hip.LIB_PATH}
    torch = None
    if "reset" in args.legs:
        try:
            import torch
            if not torch.cuda.is_available():
                torch = None
        except ImportError:
            torch = None
    # ---- resets: a host clock around a synchronise, the default stream (torch's current one)
    if "reset" in args.legs:
        for N in args.sizes:
            trk = MotionTracker(lib, N, dt, loop=False, seed=1)
            done = (rng.uniform(size=N) < 0.02).astype(np.int32)
            r = {"done": int(done.sum())}
            if torch is not None:
                mask = torch.from_numpy(done).cuda()

                def compact():
                    ids = torch.nonzero(mask).flatten().to(torch.int32)
                    n = int(ids.numel())                                 # (the read of the size: a synchronisation)
                    trk.reset_dev(n, ids)
                    torch.cuda.synchronize()

                r["compact_us"] = host_timed(compact, args.reps) * 1e6
                if masked:
                    def one_launch():
                        trk.reset_done_dev(done=mask)
                        torch.cuda.synchronize()

                    r["masked_us"] = host_timed(one_launch, args.reps) * 1e6
            if masked:                                                   # the launch alone, between device events
                d_done = hip.DeviceBuffer.from_host(done)
                r["masked_kernel_us"] = timed(hip, st, lambda: trk.reset_done_dev(done=d_done, stream=st), args.reps) * 1e6
            d_ids, n_done = hip.DeviceBuffer.from_host(np.nonzero(done)[0].astype(np.int32)), int(done.sum())
            r["reset_dev_kernel_us"] = timed(hip, st, lambda: trk.reset_dev(n_done, d_ids, stream=st), args.reps) * 1e6
            out[f"reset_N{N}"] = r
            trk.close()
    # ---- steps: the grown state must not cost them anything
    if "step" in args.legs:
        N = 65536
        trk = MotionTracker(lib, N, dt, loop=False, seed=1)
        trk.reset_dev(stream=st, time_offset_range=(0.0, 8.0))
        q = rng.normal(size=(N, 4))
        sim = {"base_pos": rng.normal(size=(N, 3)), "base_quat": q / np.linalg.norm(q, axis=1, keepdims=True), "base_lin_vel": rng.normal(size=(N, 3)),
               "base_ang_vel": rng.normal(size=(N, 3)), "dof_pos": rng.normal(size=(N, ndof)), "dof_vel": rng.normal(size=(N, ndof))}
        d_sim = {k: hip.DeviceBuffer.from_host(v.astype(np.float32)) for k, v in sim.items()}
        widths = {"ref_root_pos": 3, "ref_root_rot": 4, "ref_root_vel": 3, "ref_root_ang_vel": 3, "ref_dof_pos": ndof, "ref_dof_vel": ndof, "err": 6,
                  "term": 6, "total": 1, "status": 1, "finished": 1}
        d_out = {k: hip.DeviceBuffer(N * c * 4) for k, c in widths.items()}
        out["step_N65536_us"] = timed(hip, st, lambda: trk.step_dev(d_sim, stream=st, **d_out), args.reps) * 1e6
        names = list(km.body_names)
        trk.set_links(km, bodies=[names.index(n) for n in SIX])
        links = {"body_pos": (3,), "body_rot": (4,), "body_vel": (3,), "body_ang_vel": (3,)}
        d_links = {}
        for k, (c,) in links.items():
            a = rng.normal(size=(N, len(SIX), c))
            if c == 4:
                a /= np.linalg.norm(a, axis=2, keepdims=True)
            d_links[k] = hip.DeviceBuffer.from_host(a.astype(np.float32))
        l_out = {"total": d_out["total"], "finished": d_out["finished"], "fail": hip.DeviceBuffer(N * 4), "link_err": hip.DeviceBuffer(N * 16)}
        out["step_links_N65536_us"] = timed(hip, st, lambda: trk.step_links_dev(d_sim, d_links, stream=st, **l_out), args.reps) * 1e6
        trk.close()
    # ---- an Adapt, and a reset in which everything fails
    if "adapt" in args.legs and masked:
        N = args.sizes[-1]
        trk = MotionTracker(lib, N, dt, loop=False, seed=1)
        for name, bs in (("adapt_bins_0.5s", 0.5), ("adapt_bins_one_frame", 1.0 / 30.0)):
            trk.set_adaptive(bs)
            Bt = len(trk.adaptive_state()["prob"])
            out[name] = {"bins": Bt, "us": timed(hip, st, lambda: trk.adapt_dev(stream=st), max(3, args.reps // 3)) * 1e6}
        trk.set_adaptive(0.5)
        ones = hip.DeviceBuffer.from_host(np.ones(N, np.int32))
        clip_s, time_s = rng.integers(0, S, size=N).astype(np.int32), rng.uniform(0.0, T / 30.0, size=N).astype(np.float32)
        d_cs, d_ts = hip.DeviceBuffer.from_host(clip_s), hip.DeviceBuffer.from_host(time_s)
        d_c1, d_t1 = hip.DeviceBuffer.from_host(np.full(N, 7, np.int32)), hip.DeviceBuffer.from_host(np.full(N, 3.3, np.float32))

        def failing(d_clip, d_time):
            trk.assign_dev(N, d_clip, d_time, stream=st)
            trk.reset_done_dev(done=ones, failed=ones, stream=st)

        out["assign_alone_us"] = timed(hip, st, lambda: trk.assign_dev(N, d_cs, d_ts, stream=st), args.reps) * 1e6
        out["all_fail_spread_us"] = timed(hip, st, lambda: failing(d_cs, d_ts), args.reps) * 1e6
        out["all_fail_one_bin_us"] = timed(hip, st, lambda: failing(d_c1, d_t1), args.reps) * 1e6
        out["all_fail_N"] = N
        trk.close()
    print("PROBE " + json.dumps(out))
    return 0


def run_child(args, tree, legs, lib_path=None):
    env = dict(os.environ)
    env.pop("GMR_HIP_LIBRARY", None)
    if lib_path:
        env["GMR_HIP_LIBRARY"] = lib_path
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--legs", *legs, "--clips", str(args.clips), "--frames", str(args.frames),
           "--reps", str(args.reps), "--sizes", *[str(n) for n in args.sizes]]
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.child_timeout)
    if res.returncode != 0:
        raise RuntimeError(f"child on {tree} failed ({res.returncode}):\n{res.stderr[-3000:]}")
    line = [x for x in res.stdout.splitlines() if x.startswith("PROBE ")][-1]
    return json.loads(line[6:])


def figure(us):
    mean = float(np.mean(us))
    return {"us": mean, "rounds_us": [float(x) for x in us], "spread": (max(us) - min(us)) / mean if mean else 0.0}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 1048576])
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with libgmrhip.so built in it")
    ap.add_argument("--variant-lib", help="a build_variant of this tree (-DGMR_ADAPTIVE_AGGREGATE=0: one atomic per lane) for the failing legs")
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_tracker_adaptive_probe.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--legs", nargs="+", default=["reset", "step", "adapt"], help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:
        return child(args)
    runs = {"this": [], "parent": []}
    for _ in range(args.rounds):                               # alternated: the parent's tree, then this one
        if args.parent_tree:
            runs["parent"].append(run_child(args, os.path.abspath(args.parent_tree), ["reset", "step"]))
        runs["this"].append(run_child(args, ROOT, ["reset", "step", "adapt"]))
    doc = {"clips": args.clips, "frames_per_clip": args.frames, "reps": args.reps, "rounds": args.rounds,
           "timing": "resets: host clock around a device synchronise; steps, Adapt and the failing legs: device events",
           "parent": "measured" if args.parent_tree else "not measured (no --parent-tree)", "reset": {}, "steps": {}}
    for N in args.sizes:
        key = f"reset_N{N}"
        r = {"done": runs["this"][0][key]["done"]}
        for name in ("masked_us", "compact_us", "masked_kernel_us", "reset_dev_kernel_us"):
            if name in runs["this"][0][key]:
                r["this_" + name[:-3]] = figure([x[key][name] for x in runs["this"]])
        if runs["parent"] and "compact_us" in runs["parent"][0][key]:
            r["parent_compact"] = figure([x[key]["compact_us"] for x in runs["parent"]])
            if "this_masked" in r:
                spread_us = max(r["parent_compact"]["spread"] * r["parent_compact"]["us"], r["this_masked"]["spread"] * r["this_masked"]["us"])
                r["masked_over_parent_compact"] = r["this_masked"]["us"] / r["parent_compact"]["us"]
                r["pass_line_met"] = bool(r["this_masked"]["us"] <= r["parent_compact"]["us"] + spread_us)
        doc["reset"][str(N)] = r
    for key in ("step_N65536_us", "step_links_N65536_us"):
        s = {"this": figure([x[key] for x in runs["this"]])}
        if runs["parent"]:
            s["parent"] = figure([x[key] for x in runs["parent"]])
            s["this_over_parent"] = s["this"]["us"] / s["parent"]["us"]
            s["pass_line_met"] = bool(abs(s["this"]["us"] - s["parent"]["us"]) <= 2 * s["parent"]["spread"] * s["parent"]["us"])
        doc["steps"][key[:-3]] = s
    last = runs["this"]
    doc["adapt"] = {k: {"bins": last[0][k]["bins"], **figure([x[k]["us"] for x in last])} for k in ("adapt_bins_0.5s", "adapt_bins_one_frame")}
    doc["all_fail"] = {"N": last[0]["all_fail_N"], **{k[:-3]: figure([x[k] for x in last]) for k in ("assign_alone_us", "all_fail_spread_us", "all_fail_one_bin_us")}}
    if args.variant_lib:
        var = [run_child(args, ROOT, ["adapt"], os.path.abspath(args.variant_lib)) for _ in range(args.rounds)]
        doc["all_fail_variant_library"] = {k[:-3]: figure([x[k] for x in var]) for k in ("all_fail_spread_us", "all_fail_one_bin_us")}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
