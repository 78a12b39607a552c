"""Tracker loss: device-event times of ``MotionTracker.log_prob_dev`` -- the old log-probabilities of an iteration --
and of ``MotionTracker.loss_dev`` -- the loss head of a mini-epoch with every output, the KL and the learning-rate step --, the number of
kernels each call launches with the device time of each kernel from the same trace, the bytes each call moves and their share of the
HBM roof.

  (H, N, A) = (32, 4096, 23) and (24, 4096, 12): the horizons and action widths of T1Imitation.yaml and T1.yaml
     log_prob_dev           one launch
     loss_dev               two launches                    every output, the old policy, update_lr

Every time is the mean of ``--calls`` (at least 200) calls between two device events on the null stream after a warm-up, ``--rounds``
times, the spread over the rounds beside the mean.  The kernels per call are counted in a run of its own: this program again as a child
under ``rocprofv3 --kernel-trace``, started before this process opens the device, whose trace is read for the kernels of
``gmr_tracker_loss.hip``; without rocprofv3 the document says so.  If that run exceeds its time limit or ends with any status but 0, the
probe ends there with status 3: nothing more is started on the device and nothing is timed.  Beside these figures, in the same run, stands
a torch composition of what the call replaces -- the four terms, their sum, ``backward`` down to ``loc``, ``logstd`` and ``values``, and
the KL (booster_gym/utils/runner.py:146-174) -- on random tensors of the same shapes that stand in for the outputs of the networks; they
are not the networks.  ``--no-torch`` leaves it out.  Prints one JSON document; --out writes it to a file as well.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import math
import os
import re
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

N = 4096
CONFIGS = ((32, 23), (24, 12))
NDOF, DT = 21, 0.02
LOSS = dict(bound_coef=0.01, entropy_coef=-0.01, desired_kl=0.01, learning_rate=1e-3)
TRACE_CALLS = 20


def inputs(cfg):
    """random rows that stand in for the networks' outputs and the rollout: the old policy a small step away, the actions its samples"""
    H, A = cfg
    M = H * N
    rng = np.random.default_rng(H)
    f = np.float32
    loc, logstd = rng.normal(0, 0.8, (M, A)).astype(f), rng.normal(-2.0, 0.3, A).astype(f)
    old_loc, old_logstd = (loc + rng.normal(0, 0.02, (M, A))).astype(f), (logstd + rng.normal(0, 0.01, A)).astype(f)
    return {"loc": loc, "logstd": logstd, "actions": (old_loc + np.exp(old_logstd) * rng.normal(0, 1, (M, A))).astype(f),
            "old_log_prob": np.zeros(M, f), "values": rng.normal(0.5, 2, M).astype(f), "returns": rng.normal(0.5, 2, M).astype(f),
            "advantages": rng.normal(0, 1, M).astype(f), "old_loc": old_loc, "old_logstd": old_logstd}


def setup(hip, cfg):
    """a tracker with the loss set and every array of a call on the device -> (tracker, log_prob call, loss call, keep)"""
    from general_motion_retargeting_amd import MotionTracker
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    H, A = cfg
    M = H * N
    rng = np.random.default_rng(H)
    S, T = 4, 32
    B = S * T
    w = rng.normal(size=(B, 4))
    bufs = [hip.DeviceBuffer.from_host(a) for a in (rng.normal(0, 0.5, size=(B, 3)), w / np.linalg.norm(w, axis=1, keepdims=True), rng.uniform(-1.2, 1.2, size=(B, NDOF)))]
    lib = MotionLibrary.from_device((np.arange(S + 1) * T).astype(np.int32), np.full(S, 30.0), NDOF, 0, *bufs, None)
    trk = MotionTracker(lib, N, DT, None, None, loop=True, seed=1)
    trk.set_rollout(H, 4, 0, A, 0.995, 0.95)
    trk.set_loss(**LOSS)
    up = hip.DeviceBuffer.from_host
    x = {k: up(a) for k, a in inputs(cfg).items()}
    out = {"grad_loc": up(np.zeros((M, A), np.float32)), "grad_logstd": up(np.zeros(A, np.float32)), "grad_values": up(np.zeros(M, np.float32)),
           "log_prob": up(np.zeros(M, np.float32)), "terms": up(np.zeros(8))}
    trk.log_prob_dev(x["old_loc"], x["old_logstd"], x["actions"], x["old_log_prob"])      # the old log-probabilities the loss reads

    def log_prob():
        trk.log_prob_dev(x["old_loc"], x["old_logstd"], x["actions"], x["old_log_prob"])

    def loss():
        trk.loss_dev(x, out, update_lr=True)

    return trk, log_prob, loss, (lib, bufs, x, out)


def traced(hip):
    """the child under rocprofv3: TRACE_CALLS calls of each kind per configuration, nothing else"""
    for cfg in CONFIGS:
        trk, log_prob, loss, keep = setup(hip, cfg)
        for _ in range(TRACE_CALLS - 1):                               # (setup has made the first)
            log_prob()
        for _ in range(TRACE_CALLS):
            loss()
        hip.check(hip.lib().gmr_stream_sync(None))
        trk.close()
    return 0


def torch_composition(torch, cfg, timed, calls):
    """seconds per mini-epoch of the torch operations the call replaces, on leaf tensors in place of the networks' outputs"""
    H, A = cfg
    dev = torch.device("cuda")
    x = {k: torch.from_numpy(a).to(dev) for k, a in inputs(cfg).items()}
    loc, values = x["loc"].view(H, N, A).requires_grad_(), x["values"].view(H, N).requires_grad_()
    logstd = x["logstd"].view(1, A).requires_grad_()
    actions, returns, adv = x["actions"].view(H, N, A), x["returns"].view(H, N), x["advantages"].view(H, N)
    Normal = torch.distributions.Normal
    with torch.no_grad():
        old = Normal(x["old_loc"].view(H, N, A), torch.exp(x["old_logstd"].view(1, A)).expand(H, N, A))
        old_lp = old.log_prob(actions).sum(dim=-1)

    def mini_epoch():
        for t in (loc, logstd, values):
            t.grad = None
        dist = Normal(loc, torch.exp(logstd).expand_as(loc))
        value_loss = torch.nn.functional.mse_loss(values, returns)
        ratio = torch.exp(dist.log_prob(actions).sum(dim=-1) - old_lp)
        actor_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 0.8, 1.2)).mean()
        bound_loss = torch.clip(dist.loc - 1.0, min=0.0).square().mean() + torch.clip(dist.loc + 1.0, max=0.0).square().mean()
        entropy = dist.entropy().sum(dim=-1)
        (value_loss + actor_loss + LOSS["bound_coef"] * bound_loss + LOSS["entropy_coef"] * entropy.mean()).backward()
        with torch.no_grad():
            return torch.distributions.kl_divergence(old, dist).sum(dim=-1).mean()

    mini_epoch()
    assert loc.grad.shape == (H, N, A) and math.isfinite(float(mini_epoch()))
    return timed(mini_epoch, calls, warm=10)


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
        return traced(hip)
    if args.calls < 200:
        ap.error("--calls: events around at least 200 calls")
    # the traced child first, before this process loads the library or opens the device: a run of its own.  If it hangs or faults,
    # the probe ends with its status and times nothing.
    try:
        counted = "not counted (--no-trace)" if args.no_trace else kernels_per_call(args.trace_timeout)
    except rollout.TraceFailed as e:
        print(f"tracker_loss_probe: {e}; nothing was timed", file=sys.stderr)
        return 3
    from general_motion_retargeting_amd import _lib as hip
    hip.require_gpu()
    torch = None
    if not args.no_torch:
        import torch
    doc = {"N": N, "loss": LOSS, "calls": args.calls, "rounds": args.rounds, "kernels_per_call": counted, "configs": {}}
    doc["backend"] = hip.lib().gmr_backend_info().decode()
    timed = timer(hip, None)
    for cfg in CONFIGS:
        H, A = cfg
        M = H * N
        trk, log_prob, loss, keep = setup(hip, cfg)
        lp, ls = [], []
        for _ in range(args.rounds):                                   # alternated
            lp.append(timed(log_prob, args.calls, warm=10))
            ls.append(timed(loss, args.calls, warm=10))
        # bytes from the shapes: two [M][A] arrays read and [M] written; three [M][A] read and one written, four [M] read and two written
        lp_bytes = 2 * M * A * 4 + M * 4
        ls_bytes = 4 * M * A * 4 + 6 * M * 4
        entry = {"log_prob_dev": figure(lp, lp_bytes), "loss_dev": figure(ls, ls_bytes)}
        trk.close()
        del keep
        if torch is not None:
            tt = [torch_composition(torch, cfg, timed, args.calls) for _ in range(args.rounds)]
            entry["torch_composition"] = figure(tt)
            entry["torch_over_loss_dev"] = entry["torch_composition"]["us"] / entry["loss_dev"]["us"]
        doc["configs"][f"H{H}_N{N}_A{A}"] = entry
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


def kernels_per_call(timeout):
    """-> launches per call and the device time of each kernel from a rocprofv3 --kernel-trace run of this program; a string when
    rocprofv3 is not there.  A traced run that exceeds its time limit (it is ended with everything it started), ends with any other
    status than 0 or leaves no trace raises TraceFailed."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "not counted: rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "loss", "--", sys.executable, os.path.abspath(__file__), "--traced"]
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
                    name = row.get("Kernel_Name", "")
                    if "tracker_loss_fold_kernel" in name:
                        kind = "tracker_loss_fold_kernel"
                    elif "tracker_loss_kernel" in name:
                        # the instance: <16-byte lanes, mode>; mode 0 is the log-probability alone
                        m = re.search(r"tracker_loss_kernel<\s*(\w+)\s*,\s*(\d+)\s*>", name)
                        kind = "tracker_loss_kernel" if not m else ("tracker_loss_kernel<log_prob>" if int(m.group(2)) == 0 else "tracker_loss_kernel<loss>")
                    else:
                        continue
                    rows.append((int(row["Start_Timestamp"]), kind, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3))
    rows.sort()
    kinds = sorted({k for _, k, _ in rows})
    count = {k: sum(1 for _, name, _ in rows if name == k) for k in kinds}
    calls = TRACE_CALLS * len(CONFIGS)
    out = {"launches": count, "calls_of_each_kind": calls, "kernel_us": {}}
    if "tracker_loss_kernel<loss>" in count:
        out["log_prob_dev"] = count.get("tracker_loss_kernel<log_prob>", 0) / calls
        out["loss_dev"] = (count["tracker_loss_kernel<loss>"] + count.get("tracker_loss_fold_kernel", 0)) / calls
    # the child runs the configurations one after the other: the launches of a kernel, in time order, fall into as many equal runs;
    # the first call of each run (a cold code object, cold caches) stays out of the mean
    for k in kinds:
        us = [x for _, name, x in rows if name == k]
        if len(us) != calls:
            continue
        for c, cfg in enumerate(CONFIGS):
            part = us[c * TRACE_CALLS + 1:(c + 1) * TRACE_CALLS]
            out["kernel_us"].setdefault("H%d_N%d_A%d" % (cfg[0], N, cfg[1]), {})[k] = {"mean": float(np.mean(part)), "min": float(np.min(part)), "max": float(np.max(part))}
    return out


if __name__ == "__main__":
    sys.exit(main())
