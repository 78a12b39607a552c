"""The host side of the float32 FK (csrc/gmr_fk_tree.h: fk_build_split) on synthetic trees, without a GPU:
tests/cpp/fk_plan_check.cpp replays the per-wavefront records the way fk_split_kernel walks them (ownership, parent sources,
barrier counts, parked angles, capacities; see its header) for the trees of tests/fk_trees.py and the shipped robots, as a plain
build and as a stand-alone AddressSanitizer + UBSan build.  An unequal barrier count would be a hang on the device: this check is
what lets tests/test_fk_trees.py launch those trees.  Also here: the float64 walk of tests/fk_trees.py against the float32 oracle
and the reference's recorded outputs, and what the plan makes of the fixed GPU list (every path of the plan must be in it)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_trees as ft  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "fk_plan_check.cpp")
NSWEEP = 5600            # generated trees per build (400 of each family)


def robot_trees():
    from general_motion_retargeting_amd import params
    from general_motion_retargeting_amd.models import load_kinematics_tree
    trees = []
    for robot, xml in params.ROBOT_XML_DICT.items():
        try:
            t = dict(load_kinematics_tree(xml))
        except AssertionError:          # engineai_pm01: the reference's own parser rejects it (worldbody in an include)
            continue
        t["name"] = robot
        trees.append(t)
    return trees


def run_checker(exe, trees):
    out = subprocess.run([exe], input="\n".join(ft.checker_line(t) for t in trees) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith(f"ok {len(trees)}"), (out.stdout[-500:], out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "ERROR" not in out.stderr, out.stderr[-2000:]
    return ft.parse_checker(out.stdout)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cpp") / "fk_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, SRC])
    return exe


def test_generated_trees_are_what_they_claim():
    seen = set()
    for t in ft.sweep(20 * len(ft.FAMILIES)):
        par, nb = t["parent"], len(t["parent"])
        assert par[0] == -1 and all(0 <= par[b] < b for b in range(1, nb)) and ft.depth_of(par).max() + 1 <= ft.MAX_DEPTH
        hinged = np.sort(t["dof_idx"][t["dof_idx"] >= 0])
        assert np.array_equal(hinged, np.arange(len(hinged))) and t["dof_idx"][0] == -1 and np.array_equal(t["dof_dim"] > 0, t["dof_idx"] >= 0)
        seen.add(t["family"])
    assert seen == set(ft.FAMILIES)
    by = {t["name"]: t for t in ft.gpu_trees()}
    assert len(by) == len(ft.GPU_LIST) and 35 <= len(by) <= 45
    assert ft.depth_of(by["chain24-0"]["parent"]).max() + 1 == 24 and len(by["star-0"]["parent"]) == 64 and len(by["binary-0"]["parent"]) == 63
    assert {len(t["parent"]) for t in by.values()} >= {1, 2, 3, 5, 7}
    every = ft.gpu_trees()
    q = np.concatenate([t["local_rotation"] for t in every])
    a = np.concatenate([t["axis"][t["dof_idx"] >= 0] for t in every])
    assert (q == [0, 0, 0, 1]).all(axis=1).any() and (np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - 1) > 1e-4).any()
    for k in range(3):
        for s in (-1.0, 1.0):
            assert (a == s * np.eye(3)[k]).all(axis=1).any()
    assert ((a != 0).sum(axis=1) == 3).any() and any((t["dof_idx"][1:] < 0).any() for t in every)
    assert any((t["local_translation"] == 0).any() for t in every)


def test_plan_of_generated_trees_and_shipped_robots(checker):
    """at least 5 000 generated trees and the shipped robots, every wavefront limit, with and without the shared trunk"""
    robots = robot_trees()
    assert len(robots) >= 6
    res = run_checker(checker, list(ft.sweep(NSWEEP)) + robots)
    assert len(res) == 8 * (NSWEEP + len(robots))
    g1 = res[("unitree_g1", 4, 1)]
    assert g1["nwave"] == 4 and g1["shared"] == 1 and g1["fallback"] == 0, g1
    assert any(kv["fallback"] for kv in res.values()), "no generated tree takes the one-wavefront fallback"


def test_plan_code_is_clean_under_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer + UBSan, run directly: a record, slot or parking index written out
    of bounds on the host would become an out-of-bounds LDS access on the device"""
    exe = str(tmp_path / "fk_plan_check_asan")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC],
                        capture_output=True, text=True)
    if cc.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + cc.stderr[-200:])
    run_checker(exe, list(ft.sweep(NSWEEP, seed=1000)) + robot_trees() + ft.gpu_trees())


# the configurations tests/test_fk_trees.py builds a handle with: GMR_FK_WAVES = 2, 3, 4 and GMR_FK_NO_SHARE at 4
GPU_CONFIGS = ((2, 1), (3, 1), (4, 1), (4, 0))


def test_the_gpu_list_reaches_every_path_of_the_plan(checker, capsys):
    trees = ft.gpu_trees()
    res = run_checker(checker, trees)
    rows = {t["name"]: [res[(t["name"], w, s)] for w, s in GPU_CONFIGS] for t in trees}
    default = {n: r[2] for n, r in rows.items()}

    def count(pred, table=None):
        return sum(1 for n, r in rows.items() if (pred(default[n]) if table is None else any(pred(x) for x in r)))
    with capsys.disabled():
        print()
        for n, kv in default.items():
            print(f"  {n:12s} " + " ".join(f"{k}={v}" for k, v in kv.items() if k not in ("maxw", "share")))
    for nw in (2, 3, 4):
        assert count(lambda kv: kv["nwave"] == nw and not kv["fallback"], rows) >= 3, f"fewer than three trees run with {nw} wavefronts"
    split = lambda kv: kv["nwave"] > 1  # noqa: E731
    assert count(lambda kv: split(kv) and kv["shared"]) >= 2 and count(lambda kv: split(kv) and not kv["shared"]) >= 2
    assert count(lambda kv: split(kv) and kv["nextra"] > 0) >= 2
    assert count(lambda kv: split(kv) and kv["spare"] and kv["private"] == 0) >= 2, "spare slot only"
    assert count(lambda kv: split(kv) and kv["private"] > 0) >= 2, "a private slot beyond the spare"
    assert count(lambda kv: kv["fallback"], rows) >= 2, "fallback to one wavefront"
    assert sum(1 for t in trees if len(t["parent"]) < 8) >= 2 and all(default[t["name"]]["nwave"] == 1 for t in trees if len(t["parent"]) < 8)


def test_float64_walk_agrees_with_the_oracle_and_the_recorded_reference(oracle):
    """The float64 walk is written from the definition; the float32 oracle and the reference's recorded float32 outputs (g_fk.npz)
    follow it within float32 rounding: at most 12 bodies deep, some 40 roundings per body at magnitudes of at most 2 -- 12 x 40 x
    6e-8 x 2 = 6e-5 at the very worst, a random walk of it (sqrt) 5e-6; a wrong term would show at 1e-2."""
    g = np.load(os.path.join(GOLDEN, "g_fk.npz"))
    seen = 0
    for t in robot_trees():
        robot = t["name"]
        if robot + "__body_pos" not in g.files:
            continue
        rp, rq, dof = g[robot + "__root_pos"], g[robot + "__root_rot"], g[robot + "__dof"]
        pos, rot = ft.fk_f64(t, rp, rq, dof)
        obp, obr = oracle.fk_f32(t, rp, rq, dof)
        for ref, a, b in ((pos, obp, g[robot + "__body_pos"]), (rot, obr, g[robot + "__body_rot"])):
            assert np.abs(a - ref).max() <= 5e-6 and np.abs(b - ref).max() <= 5e-6, (robot, np.abs(a - ref).max(), np.abs(b - ref).max())
        seen += 1
    assert seen >= 6
    for t in ft.gpu_trees()[::4]:           # and on synthetic trees: a depth of 24 and three-decimal rotations amplify, still float32-sized
        rp, rq, dof = ft.make_inputs(t, 16)
        pos, rot = ft.fk_f64(t, rp, rq, dof)
        obp, obr = oracle.fk_f32(t, rp, rq, dof)
        assert np.abs(obp - pos).max() <= 1e-4 * max(1.0, np.abs(pos).max()) and np.abs(obr - rot).max() <= 1e-4 * max(1.0, np.abs(rot).max()), t["name"]
