"""Chunked retargeting of long clips on a real MI355X: the gather / stitch / seams kernels against their NumPy mirror
(``tests/chunk_mirror.py``), and the pass loop (``chunking.ChunkRunner``) through the public entry points."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import chunk_mirror as cm
import bvh_synth
from test_chunk_host import mirror_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64          # doubles / ints of canary on both sides of every device buffer


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


class Guarded:
    """a device copy of a host array between two canaries"""

    def __init__(self, hip, a):
        self.hip, self.shape, self.dtype = hip, a.shape, a.dtype
        canary = np.full(GUARD, 0x5A5A5A5A if a.dtype.kind == "i" else -7.25, dtype=a.dtype)
        self.flat = np.concatenate([canary, a.ravel(), canary])
        self.buf = hip.DeviceBuffer.from_host(self.flat)
        self.ptr = hip.C.c_void_p(self.buf.ptr.value + GUARD * a.dtype.itemsize)

    def get(self):
        out = self.buf.to_host(self.flat.shape, self.dtype)
        assert np.array_equal(out[:GUARD], self.flat[:GUARD]) and np.array_equal(out[-GUARD:], self.flat[-GUARD:]), "write outside the buffer"
        return out[GUARD:-GUARD].reshape(self.shape)


def _device_pass(hip, chunk, first, Tc, slots, mode, tol, host):
    """gather -> (the 'IK' of the test: q_out_c / nsolve_c / status_c given) -> stitch -> seams on the device; ``host`` holds the
    arrays of the mirror BEFORE the pass; returns them after it"""
    L = hip.lib()
    S, T, nh = host["human"].shape[:3]
    nq, n = host["q0"].shape[1], len(chunk)
    g = {k: Guarded(hip, np.ascontiguousarray(v)) for k, v in host.items()}
    g["chunk"], g["first"] = Guarded(hip, chunk), Guarded(hip, first)
    lst = Guarded(hip, np.asarray(slots, np.int32)) if mode == cm.REPAIR else None
    nl = len(slots) if mode == cm.REPAIR else 0
    hip.check(L.gmr_chunk_gather_dev(S, T, nh, nq, n, Tc, g["chunk"].ptr, lst.ptr if lst else None, nl, mode, g["human"].ptr, g["q0"].ptr,
                                     g["q_out"].ptr, g["human_c"].ptr, g["len_c"].ptr, g["q0_c"].ptr, g["q_seam"].ptr, None))
    hip.check(L.gmr_chunk_stitch_dev(S, T, nq, n, Tc, g["chunk"].ptr, g["first"].ptr, lst.ptr if lst else None, nl, mode, g["q_out_c"].ptr,
                                     g["nsolve_c"].ptr, g["status_c"].ptr, g["q_out"].ptr, g["nsolve"].ptr, g["chunk_status"].ptr,
                                     g["status"].ptr, g["q_seam"].ptr, g["warm_solves"].ptr, None))
    hip.check(L.gmr_chunk_seams_dev(S, T, nq, n, Tc, g["chunk"].ptr, g["first"].ptr, g["q_out"].ptr, g["q_seam"].ptr, g["chunk_status"].ptr,
                                    float(tol), g["resid"].ptr, g["bad"].ptr, g["nbad"].ptr, g["seam_max"].ptr, None))
    hip.check(L.gmr_stream_sync(None))
    return {k: v.get() for k, v in g.items()}


def _host_arrays(rng, S, T, nh, nq, n, Tc):
    quat = lambda *shape: (lambda w: w / np.linalg.norm(w, axis=-1, keepdims=True))(rng.normal(size=shape + (4,)))      # noqa: E731
    q_out, q_out_c = rng.normal(size=(S, T, nq)), rng.normal(size=(n, Tc, nq))
    q_out[..., 3:7], q_out_c[..., 3:7] = quat(S, T), quat(n, Tc)
    return {"human": rng.normal(size=(S, T, nh, 7)), "q0": rng.normal(size=(S, nq)), "q_out": q_out,
            "nsolve": rng.integers(1, 9, size=(S, T, 2)).astype(np.int32), "status": np.full(S, 77, np.int32),
            "human_c": rng.normal(size=(n, Tc, nh, 7)), "len_c": np.full(n, -5, np.int32), "q0_c": rng.normal(size=(n, nq)),
            "q_out_c": q_out_c, "nsolve_c": rng.integers(1, 9, size=(n, Tc, 2)).astype(np.int32),
            "status_c": rng.choice([0, 0, 0, -1], size=n).astype(np.int32), "chunk_status": np.zeros(n, np.int32),
            "q_seam": rng.normal(size=(n, nq)), "warm_solves": np.full(S, -3, np.int32), "resid": np.full((n, 3), -1.0),
            "bad": np.full(n, -9, np.int32), "nbad": np.full(1, -9, np.int32), "seam_max": np.full((S, 3), -1.0)}


def _mirror_pass(chunk, first, Tc, slots, mode, tol, host):
    h = {k: v.copy() for k, v in host.items()}
    cm.gather_np(chunk, Tc, slots, mode, h["human"], h["q0"], h["q_out"], h["human_c"], h["len_c"], h["q0_c"], h["q_seam"])
    cm.stitch_np(chunk, first, Tc, slots, mode, h["q_out_c"], h["nsolve_c"], h["status_c"], h["q_out"], h["nsolve"], h["chunk_status"],
                 h["status"], h["q_seam"], h["warm_solves"])
    resid, bad, smax = cm.seams_np(chunk, first, Tc, h["q_out"], h["q_seam"], h["chunk_status"], tol)
    h["resid"], h["seam_max"], h["nbad"][0] = resid, smax, len(bad)
    h["bad"][:len(bad)] = bad
    return h


def _compare(dev, ref):
    for k in ("human_c", "len_c", "q0_c", "q_out", "nsolve", "chunk_status", "status", "q_seam", "warm_solves", "bad", "nbad"):
        assert np.array_equal(dev[k], ref[k], equal_nan=(dev[k].dtype.kind == "f")), k            # bytes
    for k in ("resid", "seam_max"):
        assert np.allclose(dev[k], ref[k], rtol=1e-12, atol=1e-15, equal_nan=True), k


@pytest.mark.parametrize("nh,nq", [(14, 36), (13, 33)])           # 16-byte and 8-byte copy paths
def test_gather_stitch_seams_equal_the_numpy_mirror(hip, nh, nq):
    rng = np.random.default_rng(11)
    lens = np.array([700, 90, 0, 333, 1201], dtype=np.int32)
    S, T = len(lens), 1201
    chunk, first, Tc = cm.plan_np(lens, 100, 17)
    n = len(chunk)
    host = _host_arrays(rng, S, T, nh, nq, n, Tc)
    dev = _device_pass(hip, chunk, first, Tc, list(range(n)), cm.PASS0, 0.5, host)
    ref = _mirror_pass(chunk, first, Tc, list(range(n)), cm.PASS0, 0.5, host)
    _compare(dev, ref)
    assert dev["nbad"][0] > 0 and (dev["warm_solves"][[1, 2]] == 0).all() and dev["warm_solves"][0] > 0
    # rows of q_out beyond a clip's length are untouched, as are the slots' rows beyond len_c
    assert np.array_equal(dev["q_out"][1, 90:], host["q_out"][1, 90:])
    # a repair pass over the listed chunks only: the other chunks' rows keep their bytes
    slots = dev["bad"][:dev["nbad"][0]].tolist()
    before = {k: dev[k] for k in host}
    m = len(slots)
    before.update({k: host[k][:m] if k in ("human_c", "len_c", "q0_c", "q_out_c", "nsolve_c", "status_c") else before[k] for k in host})
    chunk_m = chunk
    dev2 = _device_pass(hip, chunk_m, first, Tc, slots, cm.REPAIR, 0.5, before)
    ref2 = _mirror_pass(chunk_m, first, Tc, slots, cm.REPAIR, 0.5, before)
    _compare(dev2, ref2)
    untouched = np.ones(n, bool)
    untouched[slots] = False
    for k in np.nonzero(untouched)[0]:
        c, s0, w, o = chunk[k]
        assert np.array_equal(dev2["q_out"][c, s0 + w:s0 + w + o], before["q_out"][c, s0 + w:s0 + w + o])


def test_bad_tables_stay_inside_the_buffers(hip):
    rng = np.random.default_rng(5)
    S, T, nh, nq, Tc = 3, 64, 14, 36, 20
    chunk = np.array([[0, 0, 0, 20], [0, 60, 10, 30], [2, -5, 50, 9], [7, 0, 0, 5], [-1, 3, 3, 3], [1, 63, 1, 1], [1, 2**30, 2**30, 2**30],
                      [2, 40, 5, -3]], dtype=np.int32)
    first = np.array([0, 9, -4, 3], dtype=np.int32)                      # descending, out of range
    n = len(chunk)
    host = _host_arrays(rng, S, T, nh, nq, n, Tc)
    for slots, mode in ((list(range(n)), cm.PASS0), ([5, -1, 99, 1, 1, 0, 3], cm.REPAIR)):
        h = dict(host)
        if mode == cm.REPAIR:
            h.update({k: host[k][:len(slots)] for k in ("human_c", "len_c", "q0_c", "q_out_c", "nsolve_c", "status_c")})
        dev = _device_pass(hip, chunk, first, Tc, slots, mode, 1e-3, h)         # (Guarded.get asserts the canaries)
        ref = _mirror_pass(chunk, np.clip(first, 0, n), Tc, slots, mode, 1e-3, h)
        for k in ("human_c", "len_c", "q0_c", "q_out", "nsolve"):
            assert np.array_equal(dev[k], ref[k]), k
        assert 0 <= dev["nbad"][0] <= n


def _clips(n, T, seed):
    from general_motion_retargeting_amd import GeneralMotionRetargeting, synth
    g = GeneralMotionRetargeting("bvh", "unitree_g1", actual_human_height=1.75)
    human, _ = synth.make_streams(g.model, g._tables, n, T, seed=seed)
    return g, human


def test_off_and_short_clips_are_todays_bytes(hip):
    from general_motion_retargeting_amd import chunking, dataset
    g, human = _clips(3, 90, 21)
    clips = [human[0], human[1, :40], human[2, :77]]
    base = dataset.retarget_clips("bvh", "unitree_g1", clips, [30] * 3, actual_human_height=1.75)
    rep = []
    for chunk in (None, chunking.ChunkSpec(90), "auto"):
        out = dataset.retarget_clips("bvh", "unitree_g1", clips, [30] * 3, actual_human_height=1.75, chunk=chunk, report=rep)
        for a, b in zip(base, out):
            for k in ("root_pos", "root_rot", "dof_pos", "local_body_pos"):
                assert a[k].tobytes() == b[k].tobytes(), (chunk, k)
    assert rep == []


def test_mirror_case_with_the_hip_launch_as_the_ik(hip):
    """the host test's clip: the device pass loop and the NumPy mirror around the same HIP IK agree byte for byte"""
    from general_motion_retargeting_amd import GeneralMotionRetargeting, chunking
    s, human, q0, lens, L, W = mirror_case()
    g = GeneralMotionRetargeting("bvh", "unitree_g1", actual_human_height=1.75)
    sol = g.hip_solver

    def ik(q0_c, human_c, len_c):
        return sol.retarget_streams(q0_c, human_c, lens=np.asarray(len_c, np.int32))
    ref = cm.run_chunked_np(ik, human, q0, lens, L, W, 1e-3, 2)
    q, ns, st, rep = chunking.retarget_chunked_host(sol, human, q0, lens, 0, chunking.ChunkSpec(L, W, 1e-3, 2))
    own = np.arange(human.shape[1])[None] < lens[:, None]
    assert np.array_equal(q[own], ref["q_out"][own]) and np.array_equal(ns[own], ref["nsolve"][own]) and np.array_equal(st, ref["status"])
    assert rep[0]["K"] == 4 and rep[1]["K"] == 1 and rep[0]["passes"] == ref["passes"]
    assert rep[0]["warm_solves"] == ref["warm_solves"][0] > 0 and rep[1]["warm_solves"] == 0


def test_tol_zero_unbounded_passes_reproduces_the_sequential_launch(hip):
    from general_motion_retargeting_amd import chunking
    g, human = _clips(3, 1500, 40)
    sol = g.hip_solver
    q0 = np.broadcast_to(g.model.qpos0, (3, sol.nq)).copy()
    q_seq, ns_seq, st = sol.retarget_streams(q0, human)
    assert (st == 0).all()
    q, ns, st2, rep = chunking.retarget_chunked_host(sol, human, q0, None, 0, chunking.ChunkSpec(100, 30, 0.0, None))
    assert (st2 == 0).all()
    for r in rep:
        assert r["K"] == 15 and r["seam_max"] == [0.0, 0.0, 0.0] and r["seams_left_bad"] == 0 and 1 <= r["passes"] <= 15
    assert np.abs(q - q_seq).max() < 1e-8
    assert np.array_equal(ns, ns_seq)


def test_defaults_report_repair_and_a_failing_chunk(hip):
    from general_motion_retargeting_amd import chunking
    g, human = _clips(4, 1200, 60)
    sol = g.hip_solver
    q0 = np.broadcast_to(g.model.qpos0, (4, sol.nq)).copy()
    q_seq, _, _ = sol.retarget_streams(q0, human)
    spec = chunking.ChunkSpec(150)
    tol = spec.tol
    _, _, st0, rep0 = chunking.retarget_chunked_host(sol, human, q0, None, 0, chunking.ChunkSpec(150, max_passes=0))       # report only
    assert (st0 == 0).all() and all(r["passes"] == 0 and r["seams_repaired"] == 0 and r["warm_solves"] > 0 for r in rep0)
    assert all(r["seams_left_bad"] == r["seams_bad_pass0"] and r["seam_max"] == r["seam_max_pass0"] for r in rep0)
    q, _, st, rep = chunking.retarget_chunked_host(sol, human, q0, None, 0, chunking.ChunkSpec(150, max_passes=None))      # repair to the end
    assert (st == 0).all()
    for r0, r in zip(rep0, rep):
        assert r["seam_max_pass0"] == r0["seam_max"] and max(r["seam_max"]) <= tol and r["seams_left_bad"] == 0
        assert r["seams_repaired"] == r["seams_bad_pass0"] == r0["seams_bad_pass0"]
    # with every seam within tol, a frame is within 10 tol of the sequential run
    assert np.abs(q - q_seq).max() <= 10 * tol
    # a NaN frame inside one chunk fails that clip only; the others equal the clean run
    broken = human.copy()
    broken[2, 700, 3, 1] = np.nan
    qb, _, stb, repb = chunking.retarget_chunked_host(sol, broken, q0, None, 0, chunking.ChunkSpec(150, max_passes=None))
    assert stb[2] != 0 and (stb[[0, 1, 3]] == 0).all()
    assert np.array_equal(qb[[0, 1, 3]], q[[0, 1, 3]])
    assert repb[2]["seams_left_bad"] >= 1


def test_bvh_dataset_driver_with_chunk_options(hip, tmp_path):
    src, tgt = tmp_path / "src", tmp_path / "tgt"
    src.mkdir()
    for i, n in enumerate((400, 60)):
        r = bvh_synth.make_raw(n, seed=50 + i)
        bvh_synth.write_bvh(str(src / f"clip{i}.bvh"), r.names, r.parents, r.offsets, r.rows)
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "general_motion_retargeting_amd.dataset", "--source", "bvh", "--src_folder", str(src), "--tgt_folder", str(tgt),
           "--robot", "unitree_g1", "--num_cpus", "0", "--quiet", "--chunk_frames", "100", "--chunk_warmup", "20", "--chunk_tol", "1e-3",
           "--chunk_passes", "-1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{"chunk_summary"')]
    assert len(line) == 1 and line[0]["chunk_summary"]["clips_split"] == 1 and line[0]["chunk_summary"]["chunks"] == 5
    assert line[0]["chunk_summary"]["seams_left_bad"] == 0 and line[0]["chunk_summary"]["warm_solves"] > 0
    from general_motion_retargeting_amd import KinematicsModel, ROBOT_XML_DICT
    km = KinematicsModel(ROBOT_XML_DICT["unitree_g1"])
    for i, n in enumerate((400, 60)):
        with open(tgt / f"clip{i}.pkl", "rb") as f:
            d = pickle.load(f)
        assert set(d) == {"root_pos", "root_rot", "dof_pos", "local_body_pos", "fps", "link_body_list"}           # nothing new in the pkl
        assert d["dof_pos"].shape[0] == n and np.isfinite(d["dof_pos"]).all()
        ident = np.zeros((n, 4), np.float32)
        ident[:, 3] = 1.0
        lbp, _ = km.forward_kinematics(np.zeros((n, 3), np.float32), ident, d["dof_pos"].astype(np.float32))
        assert np.array_equal(np.asarray(lbp), d["local_body_pos"])
