"""Tracker policy: device-event times of ``MotionTracker.act_dev`` (sample on) and ``MotionTracker.values_dev`` -- the
forward pass of the two networks, one launch each -- against the torch composition they replace, ``model.act(obs).sample()`` and
``model.est_value(obs, priv)`` under ``no_grad`` (booster_gym/utils/model.py:29-36), on the same tensors, on the same device, in the same
session; the number of kernels each side launches per call with their device time from one trace; the floating-point operations of a call
and their share of the FP32-matrix peak.

  the reference's model (256, 128, 128 / 256, 256, 128) at the shapes of T1.yaml, (O, P, A) = (47, 14, 12), H = 24, and of
  T1Imitation.yaml, (80, 14, 23), H = 32; rows = N = 4 096 and rows = H N

Every time is the mean of ``--calls`` calls between two device events on the null stream after a warm-up, ``--rounds`` times, the two sides
alternated, the spread over the rounds beside the mean.  The kernels per call are counted in a run of its own: this program again as a child
under ``rocprofv3 --kernel-trace`` (no counters), started before this process opens the device; the child runs the library's calls first and
torch's afterwards, the library's kernels are told by their name and everything after the last of them is torch's; without rocprofv3 the
document says so.  If that run exceeds its time limit or ends with any status but 0, the probe ends there with status 3: nothing more is
started on the device and nothing is timed.  ``--no-torch`` leaves torch out.  Prints one JSON document; --out writes it to a file as well.
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

CONFIGS = {"T1": (47, 14, 12, 24), "T1Imitation": (80, 14, 23, 32)}          # O, P, A, H
N = 4096
ACTOR, CRITIC = (256, 128, 128), (256, 256, 128)
NDOF, DT = 21, 0.02
TRACE_CALLS = 10
OURS = "tracker_policy_kernel"
FP32_MATRIX_PEAK = 157.3e12                                                   # FLOP/s of the FP32-input matrix instructions of one MI355X


def widths(cfg):
    O, P, A, _ = cfg
    return {"actor": (O,) + ACTOR + (A,), "critic": (O + P,) + CRITIC + (1,)}


def flops(w, rows):
    return 2 * rows * sum(a * b for a, b in zip(w[:-1], w[1:]))


def inputs(cfg, rows):
    """the parameter list in the order of model.parameters() -- logstd, the critic, the actor -- and the rows"""
    O, P, A, _ = cfg
    rng = np.random.default_rng(O)
    w = widths(cfg)
    params = [np.full(A, -2.0, np.float32)]
    for net in ("critic", "actor"):
        for a, b in zip(w[net][:-1], w[net][1:]):
            params += [(rng.uniform(-1, 1, (b, a)) / np.sqrt(a)).astype(np.float32), (rng.uniform(-1, 1, b) / np.sqrt(a)).astype(np.float32)]
    return params, rng.normal(0, 1, (rows, O)).astype(np.float32), rng.normal(0, 1, (rows, P)).astype(np.float32)


def setup(hip, cfg, rows):
    """a tracker of ``rows`` environments with the policy set and the tensors of a call on the device -> (tracker, act call, values call, keep)"""
    from general_motion_retargeting_amd import MotionTracker
    from general_motion_retargeting_amd.motion_library import MotionLibrary
    rng = np.random.default_rng(1)
    S, T = 4, 32
    B = S * T
    q = rng.normal(size=(B, 4))
    bufs = [hip.DeviceBuffer.from_host(a) for a in (rng.normal(0, 0.5, size=(B, 3)), q / np.linalg.norm(q, axis=1, keepdims=True), rng.uniform(-1.2, 1.2, size=(B, NDOF)))]
    lib = MotionLibrary.from_device((np.arange(S + 1) * T).astype(np.int32), np.full(S, 30.0), NDOF, 0, *bufs, None)
    trk = MotionTracker(lib, rows, DT, None, None, loop=True, seed=1)
    O, P, A, _ = cfg
    trk.set_policy(O, P, A, ACTOR, CRITIC)
    params, obs, priv = inputs(cfg, rows)
    p = [hip.DeviceBuffer.from_host(a) for a in params]
    d_obs, d_priv = hip.DeviceBuffer.from_host(obs), hip.DeviceBuffer.from_host(priv)
    loc, actions, values = (hip.DeviceBuffer(4 * rows * A), hip.DeviceBuffer(4 * rows * A), hip.DeviceBuffer(4 * rows))

    def act():
        trk.act_dev(p, d_obs, loc, actions)

    def est():
        trk.values_dev(p, d_obs, d_priv, values)

    return trk, act, est, (lib, bufs, p, d_obs, d_priv, loc, actions, values)


def torch_setup(torch, cfg, rows):
    """the same tensors in two torch.nn.Sequential of Linear and ELU, and the two compositions under no_grad"""
    params, obs, priv = inputs(cfg, rows)
    dev = torch.device("cuda")
    w = widths(cfg)

    def mlp(ws, tensors):
        layers = []
        for l, (a, b) in enumerate(zip(ws[:-1], ws[1:])):
            lin = torch.nn.Linear(a, b)
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(tensors[2 * l]))
                lin.bias.copy_(torch.from_numpy(tensors[2 * l + 1]))
            layers += [lin] + ([torch.nn.ELU()] if l < len(ws) - 2 else [])
        return torch.nn.Sequential(*layers).to(dev)

    cut = 1 + 2 * (len(CRITIC) + 1)
    critic, actor = mlp(w["critic"], params[1:cut]), mlp(w["actor"], params[cut:])
    logstd = torch.from_numpy(params[0]).to(dev).reshape(1, -1)
    t_obs, t_priv = torch.from_numpy(obs).to(dev), torch.from_numpy(priv).to(dev)

    def act():
        with torch.no_grad():
            mean = actor(t_obs)
            return torch.distributions.Normal(mean, torch.exp(logstd).expand_as(mean)).sample()

    def est():
        with torch.no_grad():
            return critic(torch.cat((t_obs, t_priv), dim=-1)).squeeze(-1)

    return act, est, (critic, actor, logstd, t_obs, t_priv)


def legs():
    """(config, rows) of every measurement"""
    return [(name, rows) for name, cfg in CONFIGS.items() for rows in (N, cfg[3] * N)]


def traced(hip, with_torch):
    """the child under rocprofv3: TRACE_CALLS calls of either entry point per leg, then as many of torch's compositions, nothing else"""
    for name, rows in legs():
        trk, act, est, keep = setup(hip, CONFIGS[name], rows)
        for fn in (act, est):
            for _ in range(TRACE_CALLS):
                fn()
        hip.check(hip.lib().gmr_stream_sync(None))
        trk.close()
        del keep
    if with_torch:
        import torch
        for name, rows in legs():
            act, est, keep = torch_setup(torch, CONFIGS[name], rows)
            for fn in (act, est):
                for _ in range(TRACE_CALLS):
                    fn()
            torch.cuda.synchronize()
            del keep
    return 0


def kernels_per_call(timeout, with_torch):
    """-> launches per call and the device time of the kernels from a rocprofv3 --kernel-trace run of this program; a string when
    rocprofv3 is not there.  A traced run that exceeds its time limit (it is ended with everything it started), ends with any other
    status than 0 or leaves no trace raises TraceFailed."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "not counted: rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "policy", "--", sys.executable, os.path.abspath(__file__), "--traced"]
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
    out = {"calls_per_leg": TRACE_CALLS, "library": {}, "torch_composition": {}}
    ours = [us for _, name, us in rows if OURS in name]
    out["library"]["launches_per_call"] = len(ours) / (2 * TRACE_CALLS * len(legs()))
    if len(ours) == 2 * TRACE_CALLS * len(legs()):
        for i, (name, nrows) in enumerate(legs()):
            for j, call in enumerate(("act_dev", "values_dev")):           # the first call of a leg (cold weights) stays out
                part = ours[(2 * i + j) * TRACE_CALLS + 1:(2 * i + j + 1) * TRACE_CALLS]
                out["library"][f"{name}/{nrows}/{call}"] = {"mean_us": float(np.mean(part)), "min_us": float(np.min(part)), "max_us": float(np.max(part))}
    if with_torch:
        # everything after the library's last kernel is torch's: the uploads of its tensors launch no kernel of their own beside the copies
        # of the weights into the Linear modules, which are counted with it and named below
        last = max(i for i, (_, name, _) in enumerate(rows) if OURS in name)
        theirs = rows[last + 1:]
        calls = 2 * TRACE_CALLS * len(legs())
        out["torch_composition"]["launches_per_call_both_compositions_averaged"] = len(theirs) / calls
        out["torch_composition"]["device_us_per_call_averaged"] = sum(us for _, _, us in theirs) / calls
        names = {}
        for _, name, us in theirs:
            short = name.split("(")[0][:96]
            n, total = names.get(short, (0, 0.0))
            names[short] = (n + 1, total + us)
        out["torch_composition"]["kernels"] = {k: {"per_call": n / calls, "mean_us": total / n} for k, (n, total) in sorted(names.items(), key=lambda kv: -kv[1][1])[:12]}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
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
    if args.calls < 50:
        ap.error("--calls: events around at least 50 calls")
    # the traced child first, before this process loads the library or opens the device: a run of its own.  If it hangs or faults,
    # the probe ends with its status and times nothing.
    try:
        counted = "not counted (--no-trace)" if args.no_trace else kernels_per_call(args.trace_timeout, not args.no_torch)
    except rollout.TraceFailed as e:
        print(f"tracker_policy_probe: {e}; nothing was timed", file=sys.stderr)
        return 3
    from general_motion_retargeting_amd import _lib as hip
    hip.require_gpu()
    torch = None
    if not args.no_torch:
        import torch
    doc = {"actor_hidden": ACTOR, "critic_hidden": CRITIC, "calls": args.calls, "rounds": args.rounds, "fp32_matrix_peak_flops": FP32_MATRIX_PEAK,
           "kernels_per_call": counted, "legs": {}}
    doc["backend"] = hip.lib().gmr_backend_info().decode()
    timed = timer(hip, None)
    for name, rows in legs():
        cfg = CONFIGS[name]
        trk, act, est, keep = setup(hip, cfg, rows)
        if torch is not None:
            tact, test, tkeep = torch_setup(torch, cfg, rows)
            assert torch.cuda.current_stream().cuda_stream == 0          # the events of the timer are on the null stream: so is torch
        runs = {"act_dev": [], "values_dev": [], "torch_act_sample": [], "torch_est_value": []}
        for _ in range(args.rounds):                                   # alternated
            runs["act_dev"].append(timed(act, args.calls, warm=5))
            if torch is not None:
                runs["torch_act_sample"].append(timed(tact, args.calls, warm=5))
            runs["values_dev"].append(timed(est, args.calls, warm=5))
            if torch is not None:
                runs["torch_est_value"].append(timed(test, args.calls, warm=5))
        w = widths(cfg)
        entry = {"cols": cfg[:3], "rows": rows}
        for call, net in (("act_dev", "actor"), ("values_dev", "critic")):
            entry[call] = figure(runs[call])
            entry[call]["flop"] = flops(w[net], rows)
            entry[call]["share_of_fp32_matrix_peak"] = entry[call]["flop"] / (entry[call]["us"] * 1e-6) / FP32_MATRIX_PEAK
        trk.close()
        del keep
        if torch is not None:
            for call, ours in (("torch_act_sample", "act_dev"), ("torch_est_value", "values_dev")):
                entry[call] = figure(runs[call])
                entry[f"{call}_over_{ours}"] = entry[call]["us"] / entry[ours]["us"]
            del tkeep
        doc["legs"][f"{name}/{rows}"] = entry
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
