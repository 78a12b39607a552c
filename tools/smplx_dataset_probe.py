#!/usr/bin/env python3
"""SMPL-X dataset driver on a synthetic tree of AMASS-shaped files: wall clock and stage breakdown of
``python -m general_motion_retargeting_amd.dataset --source smplx`` with the batch path on the device and with
``GMR_DATASET_SMPLX=host`` (one gmr_smplx_frames call per clip), alternating, and the written files compared byte for byte.

    python tools/smplx_dataset_probe.py [nclips] [--reps N] [--out FILE] [--ab smplx|heights]

``--ab heights`` alternates the default (one solver and one IK job per batch, the files' heights as per-stream scale rows) with
``GMR_DATASET_HEIGHTS=groups`` (one solver and job per height) instead.

The tree: two genders (two synthetic body models written like tests/test_smplx_frames.py::_synthetic_model builds one), a few
hundred distinct betas, 120 / 60 / 30 fps, 80 .. 2 000 frames per file.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_models(folder, seed=0):
    from general_motion_retargeting_amd.utils import smpl
    J, V = 55, 300
    kt = np.stack([np.where(smpl.SMPLX_PARENTS < 0, 2**32 - 1, smpl.SMPLX_PARENTS), np.arange(J)]).astype(np.uint32)
    os.makedirs(os.path.join(folder, "smplx"), exist_ok=True)
    for i, g in enumerate(("NEUTRAL", "FEMALE")):
        rng = np.random.default_rng(seed + i)
        v = rng.normal(0, 0.3, size=(V, 3)) + np.array([0, 0, 1.0])
        sd = rng.normal(0, 0.01, size=(V, 3, 20))
        jr = rng.uniform(0, 1, size=(J, V))
        jr /= jr.sum(1, keepdims=True)
        hm = rng.normal(0, 0.1, size=(30, 3))
        np.savez(os.path.join(folder, "smplx", f"SMPLX_{g}.npz"), v_template=v, shapedirs=sd, J_regressor=jr, kintree_table=kt,
                 hands_meanl=hm[:15].reshape(-1), hands_meanr=hm[15:].reshape(-1))


def _write_clip(args):
    path, N, fps, gender, betas, seed = args
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, gender=np.array(gender), betas=betas, root_orient=np.cumsum(rng.normal(0, 0.02, size=(N, 3)), 0),
             pose_body=np.cumsum(rng.normal(0, 0.02, size=(N, 63)), 0).clip(-1.5, 1.5),
             trans=np.cumsum(rng.normal(0, 0.01, size=(N, 3)), 0) + np.array([0, 0, 0.9]), mocap_frame_rate=np.array(fps))
    return N // max(int(fps / 30.0), 1)


def make_tree(src, nclips, subjects=300, seed=0):
    import multiprocessing as mp
    rng = np.random.default_rng(seed)
    betas = rng.normal(0, 0.5, size=(subjects, 16))
    betas[:, 0] = np.round(betas[:, 0], 2)                    # a file's height group is 1.66 + 0.1 betas[0]: a few dozen groups
    jobs = []
    for i in range(nclips):
        s = int(rng.integers(0, subjects))
        jobs.append((os.path.join(src, f"subject{s:03d}", f"clip_{i:05d}.npz"), int(rng.integers(80, 2001)), (120.0, 60.0, 30.0)[i % 3],
                     ("neutral", "female")[s % 2], betas[s], seed + 1 + i))
    with mp.get_context("fork").Pool(min(16, os.cpu_count() or 4)) as pool:      # (this process never touches the GPU)
        return sum(pool.map(_write_clip, jobs, chunksize=16))


def run_cli(src, tgt, models, path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GMR_DATASET_SMPLX", "GMR_DATASET_HEIGHTS"):
        env.pop(k, None)
    if path == "host":
        env["GMR_DATASET_SMPLX"] = "host"
    if path == "groups":
        env["GMR_DATASET_HEIGHTS"] = "groups"
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "general_motion_retargeting_amd.dataset", "--source", "smplx", "--src_folder", src,
                        "--tgt_folder", tgt, "--smplx_folder", models, "--hard_motions", "--robot", "unitree_g1", "--quiet"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(f"CLI failed ({path}): {r.stderr[-2000:]}")
    summary = [json.loads(ln)["dataset_summary"] for ln in r.stdout.splitlines() if ln.startswith('{"dataset_summary"')][-1]
    return {"path": path, "wall_seconds": dt, "summary": summary}


def tree_digest(folder):
    h, n = hashlib.sha256(), 0
    for dirpath, dirs, files in os.walk(folder):
        dirs.sort()
        for f in sorted(files):
            with open(os.path.join(dirpath, f), "rb") as fh:
                h.update(os.path.relpath(os.path.join(dirpath, f), folder).encode() + b"\0" + fh.read())
            n += 1
    return n, h.hexdigest()


def main():
    args = sys.argv[1:]
    nclips = int(args[0]) if args and args[0].isdigit() else 1200
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 2
    out_file = args[args.index("--out") + 1] if "--out" in args else None
    paths = {"smplx": ("device", "host"), "heights": ("merged", "groups")}[args[args.index("--ab") + 1] if "--ab" in args else "smplx"]
    base = os.environ.get("GMR_DS_PROBE_DIR", "/tmp/gmr_smplx_ds_probe")
    shutil.rmtree(base, ignore_errors=True)
    src, models = os.path.join(base, "src"), os.path.join(base, "models")
    t0 = time.perf_counter()
    write_models(models)
    frames = make_tree(src, nclips)
    out = {"clips": nclips, "output_frames": frames, "tree_seconds": time.perf_counter() - t0, "runs": []}
    digests = {}
    for rep in range(reps):
        for path in paths:                         # alternating: other work shares the host
            tgt = os.path.join(base, f"{path}_{rep}")
            run = run_cli(src, tgt, models, path)
            run["files_written"], run["sha256_of_tree"] = tree_digest(tgt)
            digests.setdefault(path, set()).add(run["sha256_of_tree"])
            out["runs"].append(run)
            shutil.rmtree(tgt, ignore_errors=True)
    out["both_paths_wrote_the_same_bytes"] = len(digests[paths[0]] | digests[paths[1]]) == 1
    shutil.rmtree(base, ignore_errors=True)
    print(json.dumps(out))
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if out["both_paths_wrote_the_same_bytes"] else 1


if __name__ == "__main__":
    raise SystemExit(main())
