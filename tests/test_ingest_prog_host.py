"""The host side of the clip ingest kernels (csrc/gmr_smplx_prog.h, csrc/gmr_bvh_prog.h: the walk programs of gmr_smplx.hip and
gmr_bvh.hip and the LDS sizes of their launches) without a GPU: tests/cpp/ingest_prog_check.cpp replays the programs the way
the kernels walk them (which joint's transform sits in the previous step, the register slot, every LDS slot, every stack level;
see its header) for generated trees and selections, the shipped SMPL-X selections and the golden BVH topology, as a plain build
and as a stand-alone AddressSanitizer + UBSan build.  A slot index beyond what the LDS size pays for would be an out-of-bounds
LDS access on the device: this check is what lets tests/test_smplx_trees.py and tests/test_bvh_trees.py launch the catalogue
of tests/ingest_trees.py.  Also here: what the programs make of that catalogue (every path must be in it), and the CPU oracle of
the SMPL-X steps against a walk written from the definition, off the SMPL-X tree."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_synth  # noqa: E402
import fk_trees as ft  # noqa: E402
import ingest_trees as it  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "ingest_prog_check.cpp")
NSWEEP = 5200            # generated cases per build, SMPL-X and BVH in turn


def shipped_lines():
    """SMPLX_PARENTS with the selection of every shipped smplx ik_config, and the golden BVH topology with all its rows"""
    from general_motion_retargeting_amd import IK_CONFIG_DICT
    from general_motion_retargeting_amd.models import load_ik_config
    from general_motion_retargeting_amd.utils import lafan1, smpl
    names = list(smpl.SMPLX_JOINT_NAMES)
    lines = [it.smplx_line("smplx", smpl.SMPLX_PARENTS)]
    for robot, path in IK_CONFIG_DICT["smplx"].items():
        cfg = load_ik_config(path)
        used = list(dict.fromkeys([v[0] for v in cfg["ik_match_table1"].values()] + [v[0] for v in cfg["ik_match_table2"].values()]))
        lines.append(it.smplx_line("smplx/" + robot, smpl.SMPLX_PARENTS, [names.index(n) for n in used]))
    raw = bvh_synth.golden_raw()
    body = bvh_synth.all_names(raw)
    lines.append(it.bvh_line("golden_bvh", raw.parents, *lafan1.selection(raw.names, body)))
    lines.append(it.bvh_line("golden_bvh/feet", raw.parents, *lafan1.selection(raw.names, ["RightFootMod", "Hips", "LeftFootMod"])))
    return lines


def run_checker(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith(f"ok {len(lines)}"), (out.stdout[-500:], out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "ERROR" not in out.stderr, out.stderr[-2000:]
    res = it.parse_checker(out.stdout)
    assert len(res) == len(lines)
    return res


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cpp") / "ingest_prog_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, SRC])
    return exe


def test_catalogue_is_what_it_claims():
    by = it.BY_NAME
    assert len(by) == len(it.CATALOGUE)
    for e in it.CATALOGUE:
        par = e["parent"]
        assert par[0] == -1 and all(0 <= par[j] < j for j in range(1, len(par))), e["name"]
        if e["sel"] is not None:
            assert len(set(e["sel"])) == len(e["sel"]) and all(0 <= j < len(par) for j in e["sel"])
        if e["bvh"] is not None:
            sp, sr = e["bvh"]
            assert len(sp) == len(sr) >= 1 and all(0 <= j < len(par) for j in list(sp) + list(sr))
    assert {len(e["parent"]) for e in it.smplx_trees()} >= {1, 2, 3, 5, 21, 22, 43, 63, 64}
    depth = lambda n: int(ft.depth_of(by[n]["parent"]).max()) + 1      # noqa: E731
    assert depth("chain64") == 64 and len(by["star64"]["parent"]) == 64 and depth("star64") == 2 and len(by["binary63"]["parent"]) == 63
    assert len(by["caterpillar27"]["parent"]) == 55 and len(by["caterpillar28"]["parent"]) == 57 and len(by["wide256"]["parent"]) == 256
    for e in it.batch_trees():
        assert len(e["parent"]) == it.BODY_JOINTS and e["sel"] is not None
    assert {e["name"] for e in it.batch_trees()} >= {"chain22", "star22", "binary22", "humanoid22"}
    sp, sr = by["wide256"]["bvh"]
    assert min(j for j in sp + sr if j) >= 223 and max(sp + sr) == 255 and len(it.closure(by["wide256"]["parent"], sp + sr)) <= 64
    # unrelated position / orientation joints, a joint in four rows, the root as an orientation-only row
    for n in ("binary63", "humanoid", "wide256", "comb43"):
        sp, sr = by[n]["bvh"]
        par = by[n]["parent"]
        unrelated = [(a, b) for a, b in zip(sp, sr) if a != b and a not in it.closure(par, [b]) and b not in it.closure(par, [a])]
        assert unrelated, n
        assert max((sp + sr).count(j) for j in set(sp + sr)) >= 4, n
    assert any(0 in e["bvh"][1] and 0 not in e["bvh"][0] for e in it.bvh_trees())


def test_programs_of_generated_trees_and_shipped_skeletons(checker):
    """at least 5 000 generated trees and selections, SMPLX_PARENTS with every shipped selection, the golden BVH topology"""
    ship = shipped_lines()
    assert len(ship) >= 8
    res = run_checker(checker, it.sweep_lines(NSWEEP) + ship)
    assert res["smplx"]["nslot"] == 3 and res["smplx"]["max_depth"] == 11 and res["smplx"]["lds_align"] < it.LDS_DEFAULT and res["smplx"]["refused"] == 0
    assert all(kv["refused"] == 0 and kv["batch_ok"] == 1 for n, kv in res.items() if n.startswith("smplx/"))
    assert res["golden_bvh"]["refused"] == 0 and res["golden_bvh"]["n"] == 22 and res["golden_bvh"]["nsel"] == 24
    S = [kv for kv in res.values() if kv["kind"] == "S"]
    B = [kv for kv in res.values() if kv["kind"] == "B"]
    # the sweep itself reaches what it is for: every refusal, duplicates, reuse, full closures, every nslot up to 6
    assert {kv["refused"] for kv in S} >= {0, 2} and {kv["refused"] for kv in B} == {0, 1, 2}
    assert {kv["nslot"] for kv in S if kv["refused"] == 0} >= {1, 2, 3, 4, 5, 6}
    assert sum(kv["reuse"] for kv in B if kv["refused"] == 0) >= 100 and sum(1 for kv in B if kv["refused"] == 0 and kv["n"] == 64) >= 3
    assert max(kv["J"] for kv in B) == 256 and sum(1 for kv in B if kv["J"] > 64 and kv["refused"] == 0) >= 100
    # the attribute branch of smplx_batch_align_kernel cannot be taken: a closure inside 22 joints is at most 22 levels deep
    assert max(kv["batch_lds_align"] for kv in S if kv.get("batch_ok")) <= it.BODY_JOINTS * 2048 < it.LDS_DEFAULT


def test_program_code_is_clean_under_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer + UBSan, run directly: a step, slot or ent index written out of
    bounds on the host would become an out-of-bounds LDS access on the device"""
    exe = str(tmp_path / "ingest_prog_check_asan")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC],
                        capture_output=True, text=True)
    if cc.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + cc.stderr[-200:])
    run_checker(exe, it.sweep_lines(NSWEEP, seed=1000) + shipped_lines() + it.catalogue_lines())


def test_the_gpu_list_reaches_every_path_of_the_programs(checker, capsys):
    res = run_checker(checker, it.catalogue_lines())
    with capsys.disabled():
        print()
        for n, kv in res.items():
            print(f"  {n:20s} " + " ".join(f"{k}={v}" for k, v in kv.items()))
    ok_s = [res[e["name"]] for e in it.smplx_trees()]
    assert all(kv["refused"] == 0 for kv in ok_s) and all(res[e["name"] + "/sel"]["refused"] == 0 for e in it.smplx_trees())
    ns = {kv["nslot"] for kv in ok_s}
    assert ns >= {1, 2, 3} and max(ns) >= 5, ns
    # the named cases
    assert res["chain64"]["nslot"] == 1 and res["chain64"]["lds_align"] == 131072 and res["chain64/sel"]["sel_depth"] == 64
    assert res["star64"]["nslot"] == 1 and res["star64"]["max_depth"] == 2
    assert res["binary63"]["nslot"] == 5
    assert res["caterpillar27"]["nslot"] == 27 and res["caterpillar27"]["lds_joints"] == 26 * 6144 == 159744 <= it.LDS_LIMIT
    assert res["caterpillar28"]["nslot"] == 28 and res["caterpillar28"]["lds_joints"] == 165888 > it.LDS_LIMIT and res["caterpillar28"]["refused"] == 1
    assert res["chain65"]["refused"] == 3
    # every hipFuncSetAttribute branch: the align kernels, the joints kernels, the batch joints kernel, the BVH frames kernel
    # (the batch align kernel's cannot be taken, see above); and rows_planes_kernel's tile at J = 64, which has no branch
    assert sum(kv["lds_align"] > it.LDS_DEFAULT for kv in ok_s) >= 2 and sum(kv["lds_joints"] > it.LDS_DEFAULT for kv in ok_s) >= 1
    batch = [res[e["name"] + "/sel"] for e in it.batch_trees()]
    assert all(kv["batch_ok"] == 1 for kv in batch) and {kv["batch_nslot"] for kv in batch} >= {1, 2, 3, 4}
    assert any(kv["batch_lds_joints"] > it.LDS_DEFAULT for kv in batch) and all(kv["batch_lds_align"] <= it.LDS_DEFAULT for kv in batch)
    assert all(res[e["name"] + "/sel"]["batch_ok"] == 0 for e in it.smplx_trees() if len(e["parent"]) > 22 and max(e["sel"]) >= 22)
    assert 64 * (64 * 3 + 1) * 4 == 49408 > it.LDS_DEFAULT and any(len(e["parent"]) == 64 for e in it.smplx_trees())
    ok_b = [res[e["name"] + "/bvh"] for e in it.bvh_trees()]
    assert all(kv["refused"] == 0 for kv in ok_b) and len(ok_b) >= 10
    assert any(kv["lds"] > it.LDS_DEFAULT for kv in ok_b) and sum(kv["reuse"] for kv in ok_b) >= 2 and {kv["nslot"] for kv in ok_b} >= {0, 1, 2, 4}
    assert res["chain64_tip/bvh"]["n"] == 64 and res["chain65_tip/bvh"]["refused"] == 1
    assert res["wide256/bvh"]["J"] == 256 and res["wide256/bvh"]["n"] <= 64 and res["wide256/bvh"]["reuse"] == 1
    s45, s46 = res["star45_sel44/bvh"], res["star46_sel45/bvh"]
    assert s45["nsel"] + s45["nslot"] == 45 and s45["lds"] == 161280 <= it.LDS_LIMIT and s45["refused"] == 0
    assert s46["nsel"] + s46["nslot"] == 46 and s46["lds"] == 164864 > it.LDS_LIMIT and s46["refused"] == 2


def _definition_walk(par, j_rest, pose, transl):
    """float64, from the definition: R_j = R_parent exp(pose_j), p_j = p_parent + R_parent (rest_j - rest_parent), the root at its
    rest position; joints + translation, global rotations as quaternions wxyz"""
    from scipy.spatial.transform import Rotation as R
    N, J = pose.shape[:2]
    rot, pos = [None] * J, np.zeros((N, J, 3))
    for j in range(J):
        local = R.from_rotvec(pose[:, j].astype(np.float64))
        if par[j] < 0:
            rot[j], pos[:, j] = local, j_rest[j]
        else:
            p = int(par[j])
            rot[j] = rot[p] * local
            pos[:, j] = pos[:, p] + rot[p].apply(j_rest[j] - j_rest[p])
    quat = np.stack([r.as_quat()[:, [3, 0, 1, 2]] for r in rot], axis=1)
    return pos + transl[:, None].astype(np.float64), quat


@pytest.mark.parametrize("name", ["small5", "humanoid22", "binary63"])
def test_oracle_follows_the_definition_off_the_smplx_tree(oracle, name):
    """oracle.smplx_joints and oracle.smplx_align walk joint by joint through parents[] (no program, no slots): the references of
    tests/test_smplx_trees.py.  Here they are compared, on catalogue trees and 8 frames, with a float64 walk written from the
    definition over SciPy's Rotation.

    Joints: the oracle restates the body model's Rodrigues formula with angle = |v + 1e-8| (each component shifted), so a
    joint's local rotation is off by at most 2 sqrt(3) 1e-8 = 3.5e-8 rad (sqrt(3) 1e-8 in the angle, as much again in the
    axis' scale v / angle, whatever |v|: at v = 0 the rotation is exactly the identity).  Every ancestor contributes that
    angle times its lever arm, at most the skeleton's diameter D: depth x 3.5e-8 x D, for these trees (depth <= 8, D <= 2)
    below 6e-7; plus the oracle's float32 output, half a float32 spacing at the largest coordinate.  A wrong parent or offset
    would show at 1e-2.
    Orientations without target times are the chained product of the local rotations: 1e-12 (normalisation after every product
    and libm against SciPy: a few 1e-16 per level).  Positions are the float32 joints as float64: equal."""
    e = it.BY_NAME[name]
    par = e["parent"]
    j_rest, pose, transl = it.smplx_inputs(e, 8)
    ref_pos, ref_quat = _definition_walk(par, j_rest, pose, transl)
    got = oracle.smplx_joints(par, j_rest, pose, transl)
    depth = int(ft.depth_of(par).max()) + 1
    D = 2.0 * np.linalg.norm(j_rest - j_rest[0], axis=1).max()
    tol = depth * 3.5e-8 * D + 0.5 * float(np.spacing(np.float32(np.abs(ref_pos).max())))
    err = np.abs(got.astype(np.float64) - ref_pos).max()
    print(f"{name}: joints err {err:.3e} tol {tol:.3e}")
    assert got.dtype == np.float32 and err <= tol, (err, tol)
    out = oracle.smplx_align(par, pose, got, None)
    assert out.shape == (8, len(par), 7) and np.array_equal(out[..., :3], got.astype(np.float64))
    qerr = np.abs(out[..., 3:] - ref_quat).max()
    print(f"{name}: quaternion err {qerr:.3e}")
    assert qerr <= 1e-12, qerr
    sel = e["sel"]
    assert np.array_equal(oracle.smplx_align(par, pose, got, None, sel), out[:, sel])
