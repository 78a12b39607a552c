"""Tracker policy backward: device-event times of ``MotionTracker.act_backward_dev`` and ``values_backward_dev`` -- the
sweep, the weight gradients and the fold, three launches each -- against what they replace, ``torch.autograd.backward`` through two
``torch.nn.Sequential`` of Linear and ELU built on the same tensors (the graph made once, kept, the ``.grad`` cleared before every call so
that torch accumulates nothing), on the same device, in the same session; the number of kernels each side launches per call with their
device time from one trace; the floating-point operations of a call and their share of the FP32-matrix peak.

  the reference's model (256, 128, 128 / 256, 256, 128) at the shapes of T1.yaml, (O, P, A) = (47, 14, 12), H = 24, and of
  T1Imitation.yaml, (80, 14, 23), H = 32; rows = N = 4 096 and rows = H N

The method is tools/tracker_policy_probe.py's: every time is the mean of ``--calls`` calls between two device events on the null stream
after a warm-up, ``--rounds`` times, the two sides alternated, the spread beside the mean; the kernels per call are counted in a run of its
own, this program again as a child under ``rocprofv3 --kernel-trace`` (no counters), started before this process opens the device.  If that
run exceeds its time limit or ends with any status but 0, the probe ends there with status 3 and times nothing.  ``--no-torch`` leaves torch
out; ``GMR_HIP_LIBRARY`` names a library built with another ``GMR_POLICY_BWD_CHUNK`` (build.build_ik_variant(name, ["-DGMR_POLICY_BWD_CHUNK=128"],
sources=("gmr_tracker_policy_bwd.hip",))), which is how the chunk size was chosen.  Prints one JSON document; --out writes it to a file.
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
import tracker_policy_probe as fwd  # noqa: E402
import tracker_rollout_probe as rollout  # noqa: E402
from tracker_control_probe import timer  # noqa: E402
from tracker_preview_probe import figure  # noqa: E402

TRACE_CALLS = 10
OURS = ("tracker_policy_sweep_kernel", "tracker_policy_dw_kernel", "tracker_policy_fold_kernel")


def flops(w, rows):
    """the sweep (every layer but the first) and the weight gradients (every layer)"""
    pairs = [a * b for a, b in zip(w[:-1], w[1:])]
    return 2 * rows * (sum(pairs[1:]) + sum(pairs))


def setup(hip, cfg, rows):
    """a tracker with the policy and the backward pass set, the forward run once for the activations -> (tracker, actor call, critic call, keep)"""
    trk, _, _, keep = fwd.setup(hip, cfg, rows)
    _, _, p, d_obs, d_priv, loc, _, values = keep
    O, P, A, _ = cfg
    w = fwd.widths(cfg)
    state = trk.set_backward(rows)
    rng = np.random.default_rng(rows)
    hid = {net: [hip.DeviceBuffer(4 * rows * h) for h in w[net][1:-1]] for net in w}
    dlt = {net: [hip.DeviceBuffer(4 * rows * h) for h in w[net][1:-1]] for net in w}
    trk.act_dev(p, d_obs, loc, hidden=hid["actor"], sample=False, rows=rows)
    trk.values_dev(p, d_obs, d_priv, values, hidden=hid["critic"], rows=rows)
    g_loc = hip.DeviceBuffer.from_host((rng.normal(0, 1, (rows, A)) / rows).astype(np.float32))
    g_val = hip.DeviceBuffer.from_host((rng.normal(0, 1, rows) / rows).astype(np.float32))
    grads = [hip.DeviceBuffer(b.nbytes) for b in p]

    def actor():
        trk.act_backward_dev(p, grads, d_obs, hid["actor"], g_loc, dlt["actor"], rows=rows)

    def critic():
        trk.values_backward_dev(p, grads, d_obs, d_priv, hid["critic"], g_val, dlt["critic"], rows=rows)

    return trk, actor, critic, (keep, hid, dlt, g_loc, g_val, grads), state


def torch_setup(torch, cfg, rows):
    """the same tensors in two torch.nn.Sequential, the forward run once with the graph kept, and autograd.backward through either"""
    params, obs, priv = fwd.inputs(cfg, rows)
    O, P, A, _ = cfg
    dev = torch.device("cuda")
    w = fwd.widths(cfg)

    def mlp(ws, tensors):
        layers = []
        for l, (a, b) in enumerate(zip(ws[:-1], ws[1:])):
            lin = torch.nn.Linear(a, b)
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(tensors[2 * l]))
                lin.bias.copy_(torch.from_numpy(tensors[2 * l + 1]))
            layers += [lin] + ([torch.nn.ELU()] if l < len(ws) - 2 else [])
        return torch.nn.Sequential(*layers).to(dev)

    cut = 1 + 2 * (len(fwd.CRITIC) + 1)
    critic, actor = mlp(w["critic"], params[1:cut]), mlp(w["actor"], params[cut:])
    t_obs, t_priv = torch.from_numpy(obs).to(dev), torch.from_numpy(priv).to(dev)
    rng = np.random.default_rng(rows)
    g_loc = torch.from_numpy((rng.normal(0, 1, (rows, A)) / rows).astype(np.float32)).to(dev)
    g_val = torch.from_numpy((rng.normal(0, 1, rows) / rows).astype(np.float32)).to(dev)
    loc = actor(t_obs)
    values = critic(torch.cat((t_obs, t_priv), dim=-1)).squeeze(-1)

    def back_actor():
        for q in actor.parameters():
            q.grad = None
        torch.autograd.backward(loc, g_loc, retain_graph=True)

    def back_critic():
        for q in critic.parameters():
            q.grad = None
        torch.autograd.backward(values, g_val, retain_graph=True)

    return back_actor, back_critic, (critic, actor, t_obs, t_priv, g_loc, g_val, loc, values)


def traced(hip, with_torch):
    """the child under rocprofv3: TRACE_CALLS calls of either entry point per leg, then as many of torch's, nothing else"""
    for name, rows in fwd.legs():
        trk, actor, critic, keep, _ = setup(hip, fwd.CONFIGS[name], rows)
        for fn in (actor, critic):
            for _ in range(TRACE_CALLS):
                fn()
        hip.check(hip.lib().gmr_stream_sync(None))
        trk.close()
        del keep
    if with_torch:
        import torch
        for name, rows in fwd.legs():
            actor, critic, keep = torch_setup(torch, fwd.CONFIGS[name], rows)
            torch.cuda.synchronize()
            for fn in (actor, critic):
                for _ in range(TRACE_CALLS):
                    fn()
            torch.cuda.synchronize()
            del keep
    return 0


def kernels_per_call(timeout, with_torch):
    """-> launches per call and the device time of the library's three kernels per leg from a rocprofv3 --kernel-trace run of this program; a
    string when rocprofv3 is not there.  torch's kernels are everything after the library's last; the one forward per leg that makes its
    graph is in that count, as the key says.  Raises TraceFailed as the forward probe does."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "not counted: rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "backward", "--", sys.executable, os.path.abspath(__file__), "--traced"]
        if not with_torch:
            cmd.append("--no-torch")
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
    legs = fwd.legs()
    out = {"calls_per_leg": TRACE_CALLS, "library": {}, "torch_autograd": {}}
    calls = 2 * TRACE_CALLS * len(legs)
    per = {k: [us for _, name, us in rows if k in name] for k in OURS}
    out["library"]["launches_per_call"] = sum(len(v) for v in per.values()) / calls
    if all(len(v) == calls for v in per.values()):
        for i, (name, nrows) in enumerate(legs):
            for j, call in enumerate(("act_backward_dev", "values_backward_dev")):      # the first call of a leg stays out
                lo, hi = (2 * i + j) * TRACE_CALLS + 1, (2 * i + j + 1) * TRACE_CALLS
                out["library"][f"{name}/{nrows}/{call}"] = {k.replace("tracker_policy_", "").replace("_kernel", "") + "_us": float(np.mean(v[lo:hi])) for k, v in per.items()}
    if with_torch:
        last = max(i for i, (_, name, _) in enumerate(rows) if any(k in name for k in OURS))
        theirs = rows[last + 1:]
        out["torch_autograd"]["launches_per_call_with_one_forward_per_leg_in_the_count"] = len(theirs) / calls
        out["torch_autograd"]["device_us_per_call_averaged"] = sum(us for _, _, us in theirs) / calls
        names = {}
        for _, name, us in theirs:
            short = name.split("(")[0][:96]
            n, total = names.get(short, (0, 0.0))
            names[short] = (n + 1, total + us)
        out["torch_autograd"]["kernels"] = {k: {"per_call": n / calls, "mean_us": total / n} for k, (n, total) in sorted(names.items(), key=lambda kv: -kv[1][1])[:12]}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-timeout", type=float, default=240.0)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run that counts the kernels")
    ap.add_argument("--no-torch", action="store_true", help="skip torch's autograd")
    ap.add_argument("--traced", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    if args.traced:
        from general_motion_retargeting_amd import _lib as hip
        hip.require_gpu()
        return traced(hip, not args.no_torch)
    if args.calls < 20:
        ap.error("--calls: events around at least 20 calls")
    try:
        counted = "not counted (--no-trace)" if args.no_trace else kernels_per_call(args.trace_timeout, not args.no_torch)
    except rollout.TraceFailed as e:
        print(f"tracker_backward_probe: {e}; nothing was timed", file=sys.stderr)
        return 3
    from general_motion_retargeting_amd import _lib as hip
    hip.require_gpu()
    torch = None
    if not args.no_torch:
        import torch
    doc = {"library": hip.LIB_PATH.replace(ROOT, "."), "actor_hidden": fwd.ACTOR, "critic_hidden": fwd.CRITIC, "calls": args.calls, "rounds": args.rounds,
           "fp32_matrix_peak_flops": fwd.FP32_MATRIX_PEAK, "kernels_per_call": counted, "legs": {}}
    doc["backend"] = hip.lib().gmr_backend_info().decode()
    timed = timer(hip, None)
    for name, rows in fwd.legs():
        cfg = fwd.CONFIGS[name]
        trk, actor, critic, keep, state = setup(hip, cfg, rows)
        if torch is not None:
            tactor, tcritic, tkeep = torch_setup(torch, cfg, rows)
            assert torch.cuda.current_stream().cuda_stream == 0          # the events of the timer are on the null stream: so is torch
        runs = {"act_backward_dev": [], "values_backward_dev": [], "torch_backward_actor": [], "torch_backward_critic": []}
        for _ in range(args.rounds):                                   # alternated
            runs["act_backward_dev"].append(timed(actor, args.calls, warm=3))
            if torch is not None:
                runs["torch_backward_actor"].append(timed(tactor, args.calls, warm=3))
            runs["values_backward_dev"].append(timed(critic, args.calls, warm=3))
            if torch is not None:
                runs["torch_backward_critic"].append(timed(tcritic, args.calls, warm=3))
        w = fwd.widths(cfg)
        entry = {"cols": cfg[:3], "rows": rows, "backward_state": state}
        for call, net in (("act_backward_dev", "actor"), ("values_backward_dev", "critic")):
            entry[call] = figure(runs[call])
            entry[call]["flop"] = flops(w[net], rows)
            entry[call]["share_of_fp32_matrix_peak"] = entry[call]["flop"] / (entry[call]["us"] * 1e-6) / fwd.FP32_MATRIX_PEAK
        trk.close()
        del keep
        if torch is not None:
            for call, ours in (("torch_backward_actor", "act_backward_dev"), ("torch_backward_critic", "values_backward_dev")):
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
