"""Per-stage start of the QP's bound sets (StageStart, csrc/gmr_ik.hip): a frame's first solve of stage s starts from the
sets that the first solve of stage s ended with in the previous frame, not from the other stage's last ones.

A pivoting round computes x from (H, c, sets) alone and both starts end at the same sets: the policy changes how many
rounds a solve takes and nothing else.  Host part: tests/bpp_stage_mirror.py (the new start) against tests/bpp_mirror.py
(the carried start, -DGMR_QP_CARRIED_START) on the scattered joint-limit input of test_ik_bound_path.py, where the
policy costs rounds, and on two streams of the benchmark batch, where it saves them; the switch compiles.  GPU part:
the kernel with and without the switch gives the same bytes, and counts exactly the rounds of the matching mirror.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bpp_mirror
import bpp_stage_mirror
from conftest import ROOT
from test_ik_bound_path import _scatter, limits_input, wide_trunk  # noqa: F401  (fixtures)

CHILD = os.path.join(ROOT, "tests", "stage_start_child.py")


def _both_mirrors(oracle, su, q0, human):
    """Per stream: (q, nsolve, rounds) of the carried and of the per-stage start, and the restore statistics."""
    carried, staged, stats = [], [], {}
    for s in range(human.shape[0]):
        log = []
        q, ns = bpp_mirror.retarget_stream(oracle, su.mb, su.ts, q0[s], human[s], log)
        carried.append((q, ns, len(log)))
        log = []
        q, ns = bpp_stage_mirror.retarget_stream(oracle, su.mb, su.ts, q0[s], human[s], log, stats)
        staged.append((q, ns, len(log)))
    return carried, staged, stats


@pytest.fixture(scope="module")
def scattered_mirrors(oracle, g1, limits_input):
    q0, human = limits_input[:2]
    return _both_mirrors(oracle, g1, q0, human)


def test_mirrors_agree_on_scattered_input(scattered_mirrors, limits_input):
    ns_o = limits_input[3]
    carried, staged, stats = scattered_mirrors
    for s, ((q_c, ns_c, _), (q_s, ns_s, _)) in enumerate(zip(carried, staged)):
        assert np.array_equal(q_s, q_c), f"stream {s}: q differs between the two starts"
        assert np.array_equal(ns_s, ns_o[s]) and np.array_equal(ns_c, ns_o[s]), f"stream {s}: solve counts differ from the oracle's"
    print(f"rounds: carried {sum(r for _, _, r in carried)}, per stage {sum(r for _, _, r in staged)}; "
          f"{stats['restores']} restores, {stats['replaced']} of them replace the carried sets")
    assert stats["replaced"] >= 50, stats


def test_per_stage_start_saves_rounds_on_coherent_motion(oracle, g1):
    """Streams 89 and 59 of the benchmark batch (seed 0, T=100): the slowest two of the latency shape."""
    from general_motion_retargeting_amd import synth
    human, q0 = synth.make_streams_ids(g1.model, g1.tt, [89, 59], 100, seed=0)
    carried, staged, stats = _both_mirrors(oracle, g1, q0, human)
    for i, ((q_c, ns_c, r_c), (q_s, ns_s, r_s)) in zip((89, 59), zip(carried, staged)):
        print(f"stream {i}: {int(ns_c.sum())} solves, rounds carried {r_c}, per stage {r_s}")
        assert np.array_equal(ns_s, ns_c), i
        assert np.array_equal(q_s, q_c), i
        assert r_s < r_c, (i, r_s, r_c)


@pytest.fixture(scope="module")
def variant_libs():
    """The library with the parent's start, and the profile builds of both starts (gmr_ik.hip recompiled, the rest linked
    from the default objects).  Cached on disk."""
    from general_motion_retargeting_amd import build
    return {"carried": build.build_ik_variant("carried", ["-DGMR_QP_CARRIED_START"]),
            "prof": build.build_ik_variant("prof", ["-DGMR_IK_PROFILE"], sources=("gmr_ik.hip", "gmr_ik_host.hip")),
            "prof_carried": build.build_ik_variant("prof_carried", ["-DGMR_IK_PROFILE", "-DGMR_QP_CARRIED_START"],
                                                   sources=("gmr_ik.hip", "gmr_ik_host.hip"))}


def test_kernel_compiles_with_and_without_the_switch(variant_libs):
    from general_motion_retargeting_amd import build
    assert os.path.exists(build.build())
    for path in variant_libs.values():
        assert os.path.exists(path), path


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _child(tmp, lib, mode, su, q0, human, waves, no_wide=False):
    src, dst = str(tmp / "in.npz"), str(tmp / f"out_{mode}_{os.path.basename(lib)}_{waves}.npz")
    np.savez(src, mb=np.frombuffer(su.mb.tobytes(), np.uint8), ts=np.frombuffer(su.ts.tobytes(), np.uint8), q0=q0, human=human)
    env = dict(os.environ, GMR_HIP_LIBRARY=lib)
    env.pop("GMR_IK_NO_WIDE", None)
    if no_wide:
        env["GMR_IK_NO_WIDE"] = "1"
    out = subprocess.run([sys.executable, CHILD, mode, src, dst, str(waves)], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return np.load(dst)


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _here(hip, monkeypatch, su, q0, human, waves, no_wide):
    if no_wide:
        monkeypatch.setenv("GMR_IK_NO_WIDE", "1")       # read by gmr_solver_create
    try:
        sol = hip.Solver(su.mb, su.ts)
    finally:
        monkeypatch.delenv("GMR_IK_NO_WIDE", raising=False)
    sol.set_waves(waves)
    out = sol.retarget_streams(q0, human)
    sol.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [4, 1])
def test_switch_changes_no_byte_on_scattered_input(hip, monkeypatch, tmp_path, g1, limits_input, variant_libs, waves):
    """<36, 4, TREE_SMALL> and <36, 1, TREE_SMALL> (the one-wavefront rows form: GMR_IK_NO_WIDE)."""
    q0, human, q_o, ns_o = limits_input
    q_h, ns_h, st_h = _here(hip, monkeypatch, g1, q0, human, waves, no_wide=waves == 1)
    assert (st_h == 0).all()
    assert np.array_equal(ns_h, ns_o), "solve counts differ from the oracle's"
    err = np.abs(q_h - q_o).max()
    print(f"{waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
    assert err <= 1e-8, err
    ref = _child(tmp_path, variant_libs["carried"], "run", g1, q0, human, waves, no_wide=waves == 1)
    assert (ref["st"] == 0).all()
    assert ns_h.tobytes() == ref["ns"].tobytes()
    assert q_h.tobytes() == ref["q"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [4, 1])
def test_switch_changes_no_byte_on_wide_trunk(hip, monkeypatch, tmp_path, oracle, wide_trunk, variant_libs, waves):
    """The <8, 10> tree instance (4 wavefronts) and the dense solver's per-lane state (1 wavefront): S=3, T=8, seed 5."""
    from general_motion_retargeting_amd import synth
    su = wide_trunk
    human, q0 = synth.make_streams(su.model, su.tt, 3, 8, seed=5)
    human = _scatter(human)
    q_o, ns_o, st_o = oracle.retarget_streams(su.mb, su.ts, q0, human)
    assert (st_o == 0).all()
    q_h, ns_h, st_h = _here(hip, monkeypatch, su, q0, human, waves, no_wide=False)
    assert (st_h == 0).all()
    assert np.array_equal(ns_h, ns_o), "solve counts differ from the oracle's"
    err = np.abs(q_h - q_o).max()
    print(f"wide trunk, {waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
    assert err <= 1e-8, err
    ref = _child(tmp_path, variant_libs["carried"], "run", su, q0, human, waves)
    assert (ref["st"] == 0).all()
    assert ns_h.tobytes() == ref["ns"].tobytes()
    assert q_h.tobytes() == ref["q"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["prof", "prof_carried"])
def test_kernel_counts_the_mirrors_rounds(hip, tmp_path, g1, limits_input, scattered_mirrors, variant_libs, which):
    """NFACT of the profile build, per stream, against the mirror of the same start: exactly equal."""
    q0, human, q_o, ns_o = limits_input
    carried, staged, _ = scattered_mirrors
    want = np.array([r for _, _, r in (staged if which == "prof" else carried)])
    got = _child(tmp_path, variant_libs[which], "prof", g1, q0, human, 4)
    assert (got["st"] == 0).all()
    assert np.array_equal(got["ns"], ns_o)
    assert np.array_equal(got["nsolve"], ns_o.sum(axis=(1, 2)))
    print(f"{which}: rounds per stream {got['nfact'].tolist()}, mirror {want.tolist()}")
    assert np.array_equal(got["nfact"], want)
