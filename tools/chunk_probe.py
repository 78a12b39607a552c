"""Chunked retargeting of long clips: what warm-up buys, and what the mode costs and reaches.

  --oracle   CPU only: long synthetic clips (synth.make_streams), sequential vs chunked on the CPU oracle for W in a list:
             seam residual and deviation over owned frames against W, how far behind a seam the deviation lives, the share of
             seams over a few tolerances.  No GPU, no timing.
  (default)  on the GPU: the LAFAN1-shaped stand-in of BASELINE.json configs[2] (77 ragged lengths, 1 200-frame motifs played
             back and forth: the recipe of bench.py's leg, restated here), sequential launch vs chunked, IK only and end to end
             (DevicePost: H2D, IK, post-processing, D2H), per-pass times, gather / stitch / seams from device events with the
             bytes they move over the HBM peak.

Prints one JSON document; --out writes it to a file as well.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12          # bytes/s, MI355X (8 TB/s HBM3E)


def deviation_profile(q_seq, q_chk, chunk, horizon=120):
    """max |dq| over the hinge angles at distance d = 0 .. horizon-1 behind every seam (frames owned by chunks k >= 1)"""
    prof = np.zeros(horizon)
    for clip, src0, warm, owned in chunk:
        if warm == 0:
            continue
        o0 = src0 + warm
        n = min(owned, horizon)
        d = np.abs(q_chk[clip, o0:o0 + n, 7:] - q_seq[clip, o0:o0 + n, 7:]).max(axis=1)
        prof[:n] = np.maximum(prof[:n], d)
    return prof


def run_oracle(args):
    import chunk_mirror as cm
    from general_motion_retargeting_amd import GeneralMotionRetargeting, synth
    from oracle import oracle
    out = {"mode": "oracle", "T": args.T, "clips": args.clips, "L": args.L, "configs": {}}
    for src, robot in [c.split(":") for c in args.configs]:
        g = GeneralMotionRetargeting(src, robot, actual_human_height=1.75)
        human, q0 = synth.make_streams(g.model, g._tables, args.clips, args.T, seed=args.seed)
        lens = np.full(args.clips, args.T, dtype=np.int32)
        q_seq, ns_seq, st = oracle.retarget_streams(g._model_blob, g._taskset_blob, q0, human, nthreads=args.threads)
        assert (st == 0).all()
        ik = cm.oracle_ik(g._model_blob, g._taskset_blob, args.threads)
        rows = []
        for W in args.W:
            r = cm.run_chunked_np(ik, human, q0, lens, args.L, W, 0.0, 0)
            seams = r["chunk"][:, 2] > 0
            res = r["resid0"][seams]
            own = np.zeros(q_seq.shape[:2], dtype=bool)
            for clip, src0, warm, owned in r["chunk"]:
                own[clip, src0 + warm: src0 + warm + owned] = True
            dev = np.abs(r["q_out"] - q_seq)[own]
            prof = deviation_profile(q_seq, r["q_out"], r["chunk"])
            above = lambda tau: int(np.nonzero(prof > tau)[0].max() + 1) if (prof > tau).any() else 0      # noqa: E731
            row = {"W": W, "seams": int(seams.sum()), "resid_max": res.max(axis=0).tolist(), "resid_median": np.median(res, axis=0).tolist(),
                   "share_over": {f"{tau:g}": float((~np.all(res <= tau, axis=1)).mean()) for tau in (1e-2, 1e-3, 1e-4)},
                   "dev_max_hinge": float(dev[:, 7:].max()), "dev_max_root_pos": float(dev[:, :3].max()),
                   "frames_behind_seam_with_dev_over": {"1e-3": above(1e-3), "1e-4": above(1e-4), "1e-6": above(1e-6)},
                   "nsolve_differs_frames": int((r["nsolve"] != ns_seq)[own].any(axis=-1).sum()),
                   "warm_solves_share": float(r["warm_solves"].sum() / max(int(ns_seq.sum()), 1))}
            # repair at the default tolerance: what is left
            for tol in args.tol:
                rr = cm.run_chunked_np(ik, human, q0, lens, args.L, W, tol, None)
                d2 = np.abs(rr["q_out"] - q_seq)
                row[f"repair_tol_{tol:g}"] = {"passes": rr["passes"], "dev_max_hinge": float(d2[..., 7:].max()),
                                              "dev_max_root_pos": float(d2[..., :3].max()),
                                              "resid_max": rr["resid"].max(axis=0).tolist()}
            rows.append(row)
            print(json.dumps({f"{src}:{robot}": row}), file=sys.stderr, flush=True)
        out["configs"][f"{src}:{robot}"] = rows
    return out


def standin(seed=30, scale=1.0):
    """the 77 ragged lengths and back-and-forth motifs of BASELINE.json configs[2] (496 k frames at scale 1)"""
    from general_motion_retargeting_amd import GeneralMotionRetargeting, synth
    rng = np.random.default_rng(3)
    lens = rng.integers(3000, 9500, size=77)
    lens = np.maximum((lens * (496000 * scale / lens.sum())).astype(np.int32), 1)
    g = GeneralMotionRetargeting("bvh", "unitree_g1", actual_human_height=1.75)
    T = int(lens.max())
    base_h, _ = synth.make_streams(g.model, g._tables, 77, 1200, seed=seed, workers=4)
    idx = np.arange(T) % 2398
    idx = np.where(idx < 1200, idx, 2398 - idx)
    return g, base_h, idx, lens


def run_gpu(args):
    from general_motion_retargeting_amd import KinematicsModel, _lib, chunking, dataset
    g, base_h, idx, lens = standin(scale=args.scale)          # (forks workers: before the GPU is initialised)
    _lib.require_gpu()
    S, T, sol = 77, int(lens.max()), g.hip_solver
    nq, nh = sol.nq, sol.nhuman
    frames = int(lens.sum())
    human = _lib.pinned_empty((S, T, nh, 7))
    human[:] = base_h[:, idx]
    q0 = np.broadcast_to(g.model.qpos0, (S, nq)).copy()
    out = {"mode": "gpu", "backend": _lib.lib().gmr_backend_info().decode(), "frames": frames, "clips": S, "longest": T,
           "input_MB": S * T * nh * 56 / 1e6}
    st = _lib.Stream()
    d_q0, d_h, d_len = (_lib.DeviceBuffer.from_host(a, st) for a in (q0, human, lens))
    d_q, d_ns, d_st = _lib.DeviceBuffer(S * T * nq * 8), _lib.DeviceBuffer(S * T * 8), _lib.DeviceBuffer(S * 4)
    launch = (sol, S, T, d_q0, d_h, d_len, d_q, d_ns, d_st)
    # sequential launch, IK only
    ms = []
    for _ in range(2):
        a, b = _lib.Event(), _lib.Event()
        a.record(st)
        _lib.retarget_group_dev([launch], 0, st)
        b.record(st)
        ms.append(a.elapsed_ms(b))
    q_seq = d_q.to_host((S, T, nq), np.float64, st)
    ns_seq = d_ns.to_host((S, T, 2), np.int32, st)
    assert (d_st.to_host((S,), np.int32, st) == 0).all()
    out["sequential"] = {"ik_ms": min(ms), "frames_per_s": frames / (min(ms) * 1e-3)}
    own = np.arange(T)[None, :] < lens[:, None]
    runner = chunking.ChunkRunner()
    specs = [("auto", chunking.resolve("auto", lens))] + [(f"L{L}", chunking.ChunkSpec(L)) for L in args.L_list]
    specs += [("auto_report_only", dataclass_replace(chunking.resolve("auto", lens), max_passes=0)),
              ("auto_tol0", dataclass_replace(chunking.resolve("auto", lens), tol=0.0, max_passes=None))]
    out["chunked"] = {}
    for name, spec in specs:
        best = None
        for rep in range(2):                    # first run of a shape: buffers grow; the second is the steady state
            t0 = time.perf_counter()
            reports, = runner.run([launch], [lens], [spec], 0, st, timed=True)
            wall = time.perf_counter() - t0
            passes = [dict(p) for p in runner.pass_ms]
            tot = sum(p["gather"] + p["ik"] + p["stitch"] + p["seams"] for p in passes)
            if best is None or tot < best["device_ms"]:
                best = {"device_ms": tot, "host_wall_ms": wall * 1e3, "passes": passes}
        q = d_q.to_host((S, T, nq), np.float64, st)
        ns = d_ns.to_host((S, T, 2), np.int32, st)
        p = chunking.plan(lens, spec.frames, spec.warmup)
        s = chunking.summarize(reports)
        dev = np.abs(q - q_seq)[own]
        p0 = best["passes"][0]
        gather_bytes = 2 * int((p.chunk[:, 2] + p.chunk[:, 3]).sum()) * nh * 56
        stitch_bytes = 2 * frames * (nq * 8 + 8)
        best.update({"spec": {"frames": spec.frames, "warmup": spec.warmup, "tol": spec.tol, "max_passes": spec.max_passes},
                     "chunks": p.nchunk, "Tc": p.Tc, "frames_per_s_device": frames / (best["device_ms"] * 1e-3),
                     "frames_per_s_pass0": frames / ((p0["gather"] + p0["ik"] + p0["stitch"] + p0["seams"]) * 1e-3),
                     "speedup_vs_sequential": out["sequential"]["ik_ms"] / best["device_ms"],
                     "gather": {"ms": p0["gather"], "bytes": gather_bytes, "share_of_hbm_peak": gather_bytes / (p0["gather"] * 1e-3) / HBM_PEAK},
                     "stitch": {"ms": p0["stitch"], "bytes": stitch_bytes, "share_of_hbm_peak": stitch_bytes / (p0["stitch"] * 1e-3) / HBM_PEAK},
                     "seams_ms": p0["seams"], "summary": s, "dev_max_hinge": float(dev[:, 7:].max()), "dev_max_root_pos": float(dev[:, :3].max()),
                     "nsolve_differs_frames": int((ns != ns_seq)[own].any(axis=-1).sum()),
                     "warm_solves_share": s["warm_solves"] / max(int(ns_seq[own].sum()), 1)})
        out["chunked"][name] = best
        print(json.dumps({name: {k: best[k] for k in ("device_ms", "chunks", "speedup_vs_sequential", "dev_max_hinge")}}), file=sys.stderr, flush=True)
    for b in (d_q0, d_h, d_len, d_q, d_ns, d_st):
        b.free()
    # end to end through DevicePost (H2D of the padded batch, IK, post-processing on the device, D2H of the five arrays)
    km = KinematicsModel(g.xml_file)
    post = dataset.DevicePost()
    out["end_to_end"] = {}
    for name, chunk in (("sequential", None), ("auto", "auto")):
        best = None
        for rep in range(2):
            timing = {}
            t0 = time.perf_counter()
            post.run([{"solver": sol, "human": human, "lens": lens, "q0": g.model.qpos0}], km, 0, False, False, 0.0, timing, chunk=chunk)
            wall = time.perf_counter() - t0
            if best is None or wall < best["wall_s"]:
                best = {"wall_s": wall, "frames_per_s": frames / wall, "parts_s": timing}
        out["end_to_end"][name] = best
    return out


def dataclass_replace(spec, **kw):
    import dataclasses
    return dataclasses.replace(spec, **kw)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--configs", nargs="*", default=["bvh:unitree_g1", "smplx:unitree_g1"])
    ap.add_argument("--T", type=int, default=2400)
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--W", type=int, nargs="*", default=[5, 10, 20, 30, 60])
    ap.add_argument("--tol", type=float, nargs="*", default=[1e-3])
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--scale", type=float, default=1.0, help="GPU mode: scale of the stand-in's 496 k frames")
    ap.add_argument("--L_list", type=int, nargs="*", default=[120, 480])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args(argv)
    res = run_oracle(a) if a.oracle else run_gpu(a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
