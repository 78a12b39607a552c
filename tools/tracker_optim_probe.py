"""Tracker optimiser: device-event times of ``MotionTracker.optimizer_step_dev`` -- the clip of the gradient norm and
the Adam step of a mini-epoch -- against the torch composition it replaces, ``clip_grad_norm_`` + ``torch.optim.Adam.step()``
(booster_gym/utils/runner.py:164-165), on the same tensors, on the same device, in the same session; the number of kernels each side
launches per step with the device time of each kernel from one trace; the bytes a step moves and their share of the HBM roof.

  K = 17 tensors: the reference's model (utils/model.py) at the sizes of T1.yaml, (O, P, A) = (47, 14, 12), and of T1Imitation.yaml,
  (80, 14, 23), in the order of ``model.parameters()``: logstd, the critic, the actor

Every time is the mean of ``--calls`` (at least 200) steps between two device events on the null stream after a warm-up, ``--rounds``
times, the two sides alternated, the spread over the rounds beside the mean.  The kernels per step are counted in a run of its own: this
program again as a child under ``rocprofv3 --kernel-trace``, started before this process opens the device; the child runs the library's
steps first and torch's afterwards, the library's kernels are told by their names and everything after the last of them is torch's;
without rocprofv3 the document says so.  If that run exceeds its time limit or ends with any status but 0, the
probe ends there with status 3: nothing more is started on the device and nothing is timed.  ``--no-torch`` leaves torch out.  Prints one
JSON document; --out writes it to a file as well.
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
import tracker_rollout_probe as rollout  # noqa: E402
from tracker_control_probe import timer  # noqa: E402
from tracker_preview_probe import figure  # noqa: E402

N = 16
CONFIGS = {"T1": (47, 14, 12), "T1Imitation": (80, 14, 23)}
NDOF, DT = 21, 0.02
LR = 1e-3
TRACE_CALLS = 20
OURS = ("tracker_optim_norm_kernel", "tracker_optim_fold_kernel", "tracker_optim_update_kernel")


def model_sizes(cfg):
    """the 17 tensors of utils/model.py's ActorCritic in the order of model.parameters()"""
    O, P, A = cfg
    critic = [(O + P) * 256, 256, 256 * 256, 256, 256 * 128, 128, 128, 1]
    actor = [O * 256, 256, 256 * 128, 128, 128 * 128, 128, 128 * A, A]
    return [A] + critic + actor


def inputs(cfg):
    rng = np.random.default_rng(cfg[0])
    sizes = model_sizes(cfg)
    return sizes, [rng.normal(0, 0.1, n).astype(np.float32) for n in sizes], [rng.normal(0, 0.05, n).astype(np.float32) for n in sizes]


def setup(hip, cfg):
    """a tracker with the optimiser set and the tensors of a step on the device -> (tracker, step call, keep)"""
    from general_motion_retargeting_amd import MotionTracker
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    rng = np.random.default_rng(1)
    S, T = 4, 32
    B = S * T
    w = rng.normal(size=(B, 4))
    bufs = [hip.DeviceBuffer.from_host(a) for a in (rng.normal(0, 0.5, size=(B, 3)), w / np.linalg.norm(w, axis=1, keepdims=True), rng.uniform(-1.2, 1.2, size=(B, NDOF)))]
    lib = MotionLibrary.from_device((np.arange(S + 1) * T).astype(np.int32), np.full(S, 30.0), NDOF, 0, *bufs, None)
    trk = MotionTracker(lib, N, DT, None, None, loop=True, seed=1)
    sizes, params, grads = inputs(cfg)
    trk.set_optimizer(sizes, learning_rate=LR)
    p, g = [hip.DeviceBuffer.from_host(a) for a in params], [hip.DeviceBuffer.from_host(a) for a in grads]
    info = hip.DeviceBuffer.from_host(np.zeros(4))

    def step():
        trk.optimizer_step_dev(p, g, info=info)

    return trk, step, (lib, bufs, p, g, info)


def torch_setup(torch, cfg):
    """the same tensors as torch parameters with their gradients, and the two lines of runner.py:164-165"""
    sizes, params, grads = inputs(cfg)
    dev = torch.device("cuda")
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(dev)) for a in params]
    gs = [torch.from_numpy(a).to(dev) for a in grads]
    opt = torch.optim.Adam(ps, lr=LR)

    for p, g in zip(ps, gs):
        p.grad = g

    def step():                                                        # (clip_grad_norm_ scales in place: from the second step on the norm is 1;
        torch.nn.utils.clip_grad_norm_(ps, 1.0)                        # the kernels it launches do not depend on that)
        opt.step()

    return step, (ps, gs, opt)


def traced(hip, with_torch):
    """the child under rocprofv3: TRACE_CALLS steps of the library per configuration, then as many of torch, nothing else"""
    for cfg in CONFIGS.values():
        trk, step, keep = setup(hip, cfg)
        for _ in range(TRACE_CALLS):
            step()
        hip.check(hip.lib().gmr_stream_sync(None))
        trk.close()
    if with_torch:
        import torch
        for cfg in CONFIGS.values():
            step, keep = torch_setup(torch, cfg)
            for _ in range(TRACE_CALLS):
                step()
            torch.cuda.synchronize()
    return 0


def kernels_per_call(timeout, with_torch):
    """-> launches per step and the device time of each kernel from a rocprofv3 --kernel-trace run of this program; a string when
    rocprofv3 is not there.  A traced run that exceeds its time limit (it is ended with everything it started), ends with any other
    status than 0 or leaves no trace raises TraceFailed."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "not counted: rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "optim", "--", sys.executable, os.path.abspath(__file__), "--traced"]
        if not with_torch:
            cmd.append("--no-torch")
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
            raise rollout.TraceFailed(f"the traced run exceeded its time limit of {timeout:g} s and was ended")
        if p.returncode != 0:
            raise rollout.TraceFailed(f"the traced run ended with status {p.returncode}: {stdout[-400:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise rollout.TraceFailed("the traced run left no kernel trace")
        rows = []
        for path in files:
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    rows.append((int(row["Start_Timestamp"]), row.get("Kernel_Name", ""), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3))
    rows.sort()
    steps = TRACE_CALLS * len(CONFIGS)
    out = {"steps_of_each_side": steps, "optimizer_step_dev": {}, "torch_composition": {}}
    ours = {k: [us for _, name, us in rows if k in name] for k in OURS}
    out["optimizer_step_dev"]["launches_per_step"] = sum(len(v) for v in ours.values()) / steps
    for k, us in ours.items():
        if len(us) != steps:
            continue
        for c, name in enumerate(CONFIGS):                             # the first step of a configuration (a cold code object) stays out
            part = us[c * TRACE_CALLS + 1:(c + 1) * TRACE_CALLS]
            out["optimizer_step_dev"].setdefault(name, {})[k] = {"mean_us": float(np.mean(part)), "min_us": float(np.min(part)), "max_us": float(np.max(part))}
    if with_torch:
        # everything after the library's last kernel is torch's: the uploads of its tensors and the steps; the uploads launch no kernel
        last = max(i for i, (_, name, _) in enumerate(rows) if any(k in name for k in OURS))
        theirs = rows[last + 1:]
        out["torch_composition"]["launches_per_step"] = len(theirs) / steps
        out["torch_composition"]["device_us_per_step"] = sum(us for _, _, us in theirs) / steps
        names = {}
        for _, name, us in theirs:
            short = name.split("(")[0][:96]
            n, total = names.get(short, (0, 0.0))
            names[short] = (n + 1, total + us)
        out["torch_composition"]["kernels"] = {k: {"per_step": n / steps, "mean_us": total / n} for k, (n, total) in sorted(names.items(), key=lambda kv: -kv[1][1])[:12]}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-timeout", type=float, default=240.0)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run that counts the kernels")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition")
    ap.add_argument("--traced", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    if args.traced:
        from general_motion_retargeting_amd import _lib as hip
        hip.require_gpu()
        return traced(hip, not args.no_torch)
    if args.calls < 200:
        ap.error("--calls: events around at least 200 calls")
    # the traced child first, before this process loads the library or opens the device: a run of its own.  If it hangs or faults,
    # the probe ends with its status and times nothing.
    try:
        counted = "not counted (--no-trace)" if args.no_trace else kernels_per_call(args.trace_timeout, not args.no_torch)
    except rollout.TraceFailed as e:
        print(f"tracker_optim_probe: {e}; nothing was timed", file=sys.stderr)
        return 3
    from general_motion_retargeting_amd import _lib as hip
    hip.require_gpu()
    torch = None
    if not args.no_torch:
        import torch
    doc = {"K": 17, "learning_rate": LR, "calls": args.calls, "rounds": args.rounds, "kernels_per_step": counted, "configs": {}}
    doc["backend"] = hip.lib().gmr_backend_info().decode()
    timed = timer(hip, None)
    for name, cfg in CONFIGS.items():
        sizes = model_sizes(cfg)
        trk, step, keep = setup(hip, cfg)
        if torch is not None:
            tstep, tkeep = torch_setup(torch, cfg)
            assert torch.cuda.current_stream().cuda_stream == 0          # the events of the timer are on the null stream: so is torch
        ours, theirs = [], []
        for _ in range(args.rounds):                                   # alternated
            ours.append(timed(step, args.calls, warm=10))
            if torch is not None:
                theirs.append(timed(tstep, args.calls, warm=10))
        # bytes from the shapes: the norm pass reads g; the update pass reads p, g, m, v and writes p, m, v
        entry = {"sizes": sizes, "floats": int(sum(sizes)), "chunks": int(sum(-(-n // hip.OPT_CHUNK) for n in sizes)),
                 "optimizer_step_dev": figure(ours, 8 * sum(sizes) * 4)}
        trk.close()
        del keep
        if torch is not None:
            entry["torch_composition"] = figure(theirs)
            entry["torch_over_optimizer_step_dev"] = entry["torch_composition"]["us"] / entry["optimizer_step_dev"]["us"]
            del tkeep
        doc["configs"][name] = entry
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
