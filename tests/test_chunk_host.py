"""Chunked retargeting, the parts that need no GPU: the plan (``gmr_chunk_plan``, host code of the library), ``ChunkSpec`` and the
``--chunk_*`` options, and the NumPy mirror of gather -> IK -> stitch -> seams (``tests/chunk_mirror.py``) around the CPU oracle."""
import argparse
import ctypes as C

import numpy as np
import pytest

import chunk_mirror as cm
from conftest import get_setup


@pytest.fixture(scope="module")
def lib():
    from general_motion_retargeting_amd import _lib, build
    build.build()
    return _lib


def test_plan_properties_over_random_ragged_lengths(lib):
    from general_motion_retargeting_amd import chunking
    rng = np.random.default_rng(0)
    for _ in range(200):
        nclip = int(rng.integers(1, 12))
        lens = rng.integers(0, 3000, size=nclip).astype(np.int32)
        L, W = int(rng.integers(1, 700)), int(rng.integers(1, 90))
        p = chunking.plan(lens, L, W)
        chunk, first, Tc = cm.plan_np(lens, L, W)
        assert np.array_equal(p.chunk, chunk) and np.array_equal(p.clip_first, first) and p.Tc == Tc
        assert p.clip_first[0] == 0 and p.clip_first[-1] == p.nchunk
        for c, n in enumerate(lens.tolist()):
            rows = p.chunk[p.clip_first[c]:p.clip_first[c + 1]]
            K = len(rows)
            assert K == max(1, -(-n // L)) and (rows[:, 0] == c).all()
            o0 = rows[:, 1] + rows[:, 2]                           # first owned frame
            assert o0[0] == 0 and rows[0, 2] == 0                  # the first chunk starts its clip, without warm-up
            assert np.array_equal(o0[1:], (o0 + rows[:, 3])[:-1]) and o0[-1] + rows[-1, 3] == n     # a partition, in order
            assert rows[:, 3].max() - rows[:, 3].min() <= 1        # evenly
            assert (rows[:, 2] <= W).all() and (rows[:, 2] <= o0).all() and (rows[1:, 2] == np.minimum(W, o0[1:])).all()
            assert (rows[:, 2] + rows[:, 3] <= L + W).all() and (rows[:, 3] <= L).all()
            if n <= L:
                assert K == 1 and tuple(rows[0]) == (c, 0, 0, n)
        assert p.Tc == max(1, int((p.chunk[:, 2] + p.chunk[:, 3]).max()))


def test_plan_argument_errors_and_two_call_sizing(lib):
    L = lib.lib()
    lens = np.array([10, 500, 0], dtype=np.int32)
    n, Tc = C.c_int(), C.c_int()
    plan = lambda *a: L.gmr_chunk_plan(*a, C.byref(n), C.byref(Tc))      # noqa: E731
    assert plan(3, lib._ptr(lens), 100, 5, 0, None, None) == 0 and n.value == 7 and Tc.value == 105
    table = np.zeros((7, 4), np.int32)
    assert plan(3, lib._ptr(lens), 100, 5, 6, lib._ptr(table), None) == -1      # no room
    assert plan(3, lib._ptr(lens), 100, 5, 7, lib._ptr(table), None) == 0
    assert plan(3, lib._ptr(lens), 0, 5, 0, None, None) == -1                       # L >= 1
    assert plan(3, lib._ptr(lens), 100, 0, 0, None, None) == -1                     # a split clip needs warm-up
    assert b"W >= 1" in L.gmr_last_error()
    assert plan(3, lib._ptr(lens), 500, 0, 0, None, None) == 0 and n.value == 3     # nothing is split: W = 0 is fine
    assert plan(3, lib._ptr(np.array([1, -2, 3], np.int32)), 10, 1, 0, None, None) == -1
    assert plan(-1, None, 10, 1, 0, None, None) == -1
    assert plan(0, None, 10, 1, 0, None, None) == 0 and n.value == 0 and Tc.value == 1


def test_chunk_spec_resolution_and_cli_options():
    from general_motion_retargeting_amd import chunking
    S = chunking.ChunkSpec
    assert chunking.resolve(None, [5000]) is None
    assert chunking.resolve(S(100), [50, 100]) is None                 # no clip longer than L: the ordinary launch
    assert chunking.resolve(S(100), [50, 101]) == S(100)
    assert chunking.resolve({"frames": 64, "warmup": 8}, [500]) == S(64, 8)
    for bad in (dict(frames=0), dict(frames=10, warmup=0), dict(frames=10, tol=-1.0), dict(frames=10, tol=float("nan")),
                dict(frames=10, max_passes=-1)):
        with pytest.raises(ValueError):
            S(**bad)
    with pytest.raises(ValueError):
        chunking.resolve("fast", [500])
    # auto: as many chunks as the device holds streams, never below the floor
    assert chunking.auto_frames(496000, 2304) == 216 and chunking.auto_frames(1000, 2304) == chunking.AUTO_FLOOR
    auto = chunking.resolve("auto", [9000] * 77)
    assert auto is not None and auto.frames >= chunking.AUTO_FLOOR and auto.warmup == chunking.DEFAULT_WARMUP
    ap = argparse.ArgumentParser()
    chunking.add_cli_arguments(ap)
    assert chunking.spec_from_args(ap.parse_args([])) is None                                       # default: off
    assert chunking.spec_from_args(ap.parse_args(["--chunk_frames", "200"])) == S(200)
    sp = chunking.spec_from_args(ap.parse_args(["--chunk_frames", "150", "--chunk_warmup", "12", "--chunk_tol", "1e-4", "--chunk_passes", "-1"]))
    assert sp == S(150, 12, 1e-4, None)
    a = chunking.spec_from_args(ap.parse_args(["--chunk_frames", "auto", "--chunk_passes", "0"]))
    r = chunking.resolve_any(a, [9000] * 77)
    assert r.max_passes == 0 and r.frames == chunking.resolve("auto", [9000] * 77).frames


def test_dataset_cli_accepts_the_chunk_options():
    from general_motion_retargeting_amd import dataset
    with pytest.raises(SystemExit) as e:
        dataset.main(["--source", "bvh", "--src_folder", "x", "--tgt_folder", "y", "--chunk_frames", "200", "--chunk_bogus", "1"])
    assert e.value.code == 2
    import inspect
    for fn in (dataset.retarget_clips, dataset.retarget_bvh_files, dataset.retarget_smplx_files, dataset.ClipRetargeter.__init__,
               dataset.GeneralMotionRetargeting.retarget_clip, dataset.run_bvh_dataset, dataset.run_smplx_dataset):
        assert inspect.signature(fn).parameters["chunk"].default is None, fn


def mirror_case(seed=3, T=150, L=40, W=12):
    """one short bvh -> G1 clip and a shorter one: the case the GPU test repeats with the HIP launch as the IK"""
    from general_motion_retargeting_amd import synth
    s = get_setup("bvh", "unitree_g1", 1.75)
    human, q0 = synth.make_streams(s.model, s.tt, 2, T, seed=seed)
    lens = np.array([T, 30], dtype=np.int32)
    return s, human, q0, lens, L, W


def test_numpy_mirror_around_the_oracle(oracle):
    s, human, q0, lens, L, W = mirror_case()
    q_seq, ns_seq, st = oracle.retarget_streams(s.mb, s.ts, q0, human)
    assert (st == 0).all()
    ik = cm.oracle_ik(s.mb, s.ts)
    own = np.arange(human.shape[1])[None] < lens[:, None]
    r0 = cm.run_chunked_np(ik, human, q0, lens, L, W, 1e-3, 0)                 # report only
    assert r0["passes"] == 0 and len(r0["chunk"]) == 5 and (r0["status"] == 0).all()
    assert r0["warm_solves"][0] > 0 and r0["warm_solves"][1] == 0
    # the clip that is not split, and the first chunk of the one that is, are the sequential run's bits
    assert np.array_equal(r0["q_out"][1, :30], q_seq[1, :30]) and np.array_equal(r0["nsolve"][1, :30], ns_seq[1, :30])
    n0 = r0["chunk"][0, 3]
    assert np.array_equal(r0["q_out"][0, :n0], q_seq[0, :n0])
    assert (r0["resid0"][[0, 4]] == 0).all()                                      # first chunks have no seam
    # tol = 0, passes unbounded: every seam ends at residual 0 and the result is the sequential run (to rounding)
    r = cm.run_chunked_np(ik, human, q0, lens, L, W, 0.0, None)
    assert len(r["bad"]) == 0 and (r["resid"] == 0).all() and 1 <= r["passes"] <= 4
    assert np.abs(r["q_out"] - q_seq)[own].max() < 1e-8
    assert np.array_equal(r["nsolve"][own], ns_seq[own])
