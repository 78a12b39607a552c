"""Tracker rollout: device-event times of ``MotionTracker.record_dev`` -- the six rows of a step into their slot --
and of ``MotionTracker.advantages_dev`` -- the bootstrap, GAE, the returns and the normalisation of a mini-epoch --, and the number of
kernels each call launches, with the device time of each kernel from the same trace.

  N = 4 096, (H, O, P, A) = (32, 80, 14, 23) and (24, 47, 14, 12): the horizons and row widths of T1Imitation.yaml and T1.yaml
     record_dev             one launch                      all six inputs of a step, the slot moving through the horizon
     advantages_dev         two launches                    every output, normalised

Every time is the mean of ``--calls`` (at least 200) calls between two device events on the null stream after a warm-up, ``--rounds``
times, the spread over the rounds beside the mean.  The kernels per call are counted in a run of its own: this program again as a child
under ``rocprofv3 --kernel-trace``, started before this process opens the device, whose trace is read for the kernels of
``gmr_tracker_rollout.hip``; without rocprofv3 the document says so.  If that run exceeds its time limit or ends with any status but 0,
the probe ends there with status 3: nothing more is started on the device and nothing is timed.  What stands beside these figures is not a time: the reference's runner issues six indexed assignments per step and, per mini-epoch,
about 9 H + 12 small device operations (``reference_ops``, counted from booster_gym/utils/runner.py:135-145 and utils/utils.py:33-44).
Prints one JSON document; --out writes it to a file as well.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tracker_control_probe import timer  # noqa: E402
from tracker_preview_probe import figure  # noqa: E402

N = 4096
CONFIGS = ((32, 80, 14, 23), (24, 47, 14, 12))
GAMMA, LAM = 0.995, 0.95
NDOF, DT = 21, 0.02
TRACE_CALLS = 20
KERNELS = ("tracker_rollout_record_kernel", "tracker_rollout_scan_kernel", "tracker_rollout_chain_kernel", "tracker_rollout_normalize_kernel")


def reference_ops(H):
    """device operations of one mini-epoch of the reference, from its lines: the masked gather and scatter of runner.py:135 (4 with the
    two mask expansions), the | of :138, per step of utils.py:37-43 nine (float(), 1 - x, two products and a sum and a difference for
    delta, two products and a sum for the advantage; the slot assignment shares the last), zeros_like twice, :144, and mean, std, the
    difference, the sum with 1e-8 and the quotient of :145"""
    return 9 * H + 12


def setup(hip, cfg):
    """a tracker with the rollout set and every array of a step and of a mini-epoch on the device -> (tracker, calls)"""
    from general_motion_retargeting_amd import MotionTracker
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    H, O, P, A = cfg
    rng = np.random.default_rng(H)
    S, T = 4, 32
    B = S * T
    w = rng.normal(size=(B, 4))
    bufs = [hip.DeviceBuffer.from_host(a) for a in (rng.normal(0, 0.5, size=(B, 3)), w / np.linalg.norm(w, axis=1, keepdims=True), rng.uniform(-1.2, 1.2, size=(B, NDOF)))]
    lib = MotionLibrary.from_device((np.arange(S + 1) * T).astype(np.int32), np.full(S, 30.0), NDOF, 0, *bufs, None)
    trk = MotionTracker(lib, N, DT, None, None, loop=True, seed=1)
    trk.set_rollout(H, O, P, A, GAMMA, LAM)
    up = hip.DeviceBuffer.from_host
    f32 = lambda *shape: up(rng.normal(0, 1, shape).astype(np.float32))      # noqa: E731
    io = {"obs": f32(H, N, O), "priv": f32(H, N, P), "actions": f32(H, N, A), "rewards": f32(H, N), "dones": up(np.zeros((H, N), np.uint8)),
          "time_outs": up(np.zeros((H, N), np.uint8))}
    step = {"obs": f32(N, O), "priv": f32(N, P), "actions": f32(N, A), "reward": f32(N), "done": up((rng.uniform(size=N) < 0.02).astype(np.int32)),
            "time_outs": up((rng.uniform(size=N) < 0.02).astype(np.int32))}
    values, last = f32(H, N), f32(N)
    out = {"advantages": f32(H, N), "returns": f32(H, N), "normalized": f32(H, N), "stats": up(np.zeros(4))}
    slot = [0]

    def record():
        trk.record_dev(slot[0], io, **step)
        slot[0] = (slot[0] + 1) % H

    def advantages():
        trk.advantages_dev(io, values, last, out)

    keep = (lib, bufs, io, step, values, last, out)
    return trk, record, advantages, keep


def traced(hip):
    """the child under rocprofv3: TRACE_CALLS calls of each kind per configuration, nothing else"""
    for cfg in CONFIGS:
        trk, record, advantages, keep = setup(hip, cfg)
        for _ in range(TRACE_CALLS):
            record()
        for _ in range(TRACE_CALLS):
            advantages()
        hip.check(hip.lib().gmr_stream_sync(None))
        trk.close()
    return 0


class TraceFailed(RuntimeError):
    """the traced run hung, faulted or left nothing: the probe ends there and starts nothing more on the device"""


def kernels_per_call(timeout):
    """-> {kernel: launches per call} from a rocprofv3 --kernel-trace run of this program; a string when rocprofv3 is not there.  A
    traced run that exceeds its time limit (it is ended with everything it started), ends with any other status than 0 or leaves no
    trace raises TraceFailed."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "not counted: rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "rollout", "--", sys.executable, os.path.abspath(__file__), "--traced"]
        # a session of its own: at the time limit the whole group goes, the traced program under rocprofv3 included
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
        try:
            stdout, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            try:
                os.killpg(p.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
            p.communicate()
            raise TraceFailed(f"the traced run exceeded its time limit of {timeout:g} s and was ended")
        if p.returncode != 0:
            raise TraceFailed(f"the traced run ended with status {p.returncode}: {stdout[-400:]}")
        rows = []
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise TraceFailed("the traced run left no kernel trace")
        for path in files:
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    for k in KERNELS:
                        if k in row.get("Kernel_Name", ""):
                            rows.append((int(row["Start_Timestamp"]), k, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3))
    rows.sort()
    count = {k: sum(1 for _, name, _ in rows if name == k) for k in KERNELS}
    calls = TRACE_CALLS * len(CONFIGS)
    out = {"record_dev": count[KERNELS[0]] / calls, "advantages_dev": sum(count[k] for k in KERNELS[1:]) / calls, "launches": count,
           "calls_of_each_kind": calls, "kernel_us": {}}
    # the child runs the configurations one after the other: the launches of a kernel, in time order, fall into as many equal runs;
    # the first call of each run (a cold code object, cold caches) stays out of the mean
    for k in KERNELS:
        us = [x for _, name, x in rows if name == k]
        if len(us) != calls:
            continue
        for c, cfg in enumerate(CONFIGS):
            part = us[c * TRACE_CALLS + 1:(c + 1) * TRACE_CALLS]
            out["kernel_us"].setdefault("H%d_O%d_P%d_A%d" % cfg, {})[k] = {"mean": float(np.mean(part)), "min": float(np.min(part)), "max": float(np.max(part))}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-timeout", type=float, default=240.0)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run that counts the kernels")
    ap.add_argument("--traced", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    if args.traced:
        from general_motion_retargeting_amd import _lib as hip
        hip.require_gpu()
        return traced(hip)
    if args.calls < 200:
        ap.error("--calls: events around at least 200 calls")
    # the traced child first, before this process loads the library or opens the device: a run of its own.  If it hangs or faults,
    # the probe ends with its status and times nothing.
    try:
        counted = "not counted (--no-trace)" if args.no_trace else kernels_per_call(args.trace_timeout)
    except TraceFailed as e:
        print(f"tracker_rollout_probe: {e}; nothing was timed", file=sys.stderr)
        return 3
    from general_motion_retargeting_amd import _lib as hip
    hip.require_gpu()
    doc = {"N": N, "gamma": GAMMA, "lam": LAM, "calls": args.calls, "rounds": args.rounds, "kernels_per_call": counted, "configs": {}}
    doc["backend"] = hip.lib().gmr_backend_info().decode()
    timed = timer(hip, None)
    for cfg in CONFIGS:
        H, O, P, A = cfg
        trk, record, advantages, keep = setup(hip, cfg)
        rec, adv = [], []
        for _ in range(args.rounds):                                   # alternated
            rec.append(timed(record, args.calls, warm=10))
            adv.append(timed(advantages, args.calls, warm=10))
        # bytes from the shapes: a step's rows read and written; rewards, values and the two flags read, three arrays written, the
        # advantages read again
        rec_bytes = 2 * N * ((O + P + A + 1) * 4) + N * (8 + 2)
        adv_bytes = H * N * (4 + 4 + 2) + N * 4 + H * N * 4 * 2 + 2 * H * N * 4
        doc["configs"][f"H{H}_O{O}_P{P}_A{A}"] = {"record_dev": figure(rec, rec_bytes), "advantages_dev": figure(adv, adv_bytes),
                                                 "reference_ops_per_mini_epoch": reference_ops(H), "reference_assignments_per_step": 6}
        trk.close()
        del keep
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
