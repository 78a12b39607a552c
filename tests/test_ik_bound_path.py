"""The joint-limit (bound) path of the tree QP: multipliers of fixed variables formed from each wavefront's own x.

Host part: a NumPy mirror of the kernel's block principal pivoting (tests/bpp_mirror.py) shows that the test input
exercises every case of that path -- rounds with a trunk (waist) variable fixed, rounds with only limb variables fixed,
multipliers that release a trunk variable and multipliers that release a limb variable.  GPU part: both launch shapes
against the oracle on that input, and on every shipped configuration (both instances of the tree solver).
"""
import os
import subprocess

import numpy as np
import pytest

import bpp_mirror
from conftest import ALL_CONFIGS, ROOT, get_setup


def _scatter(human):
    """The scatter of test_ik_joint_limits_active: targets far outside the reachable set."""
    from general_motion_retargeting_amd import synth
    rng = np.random.default_rng(0)
    human[..., :3] += rng.normal(0, 0.3, size=human[..., :3].shape)
    rv = rng.normal(0, 1.0, size=human.shape[:-1] + (3,))
    human[..., 3:] = synth.quat_mul(human[..., 3:], synth.rotvec_quat(rv))
    return human


@pytest.fixture(scope="module")
def tree_dump(tmp_path_factory):
    """The decomposition and the solver instance that the packed layout selects, as csrc/gmr_ik_layout.h computes them."""
    d = tmp_path_factory.mktemp("tree")
    exe = str(d / "tree_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "tree_dump.cpp")])

    def dump(su):
        blob = d / "blob.bin"
        with open(blob, "wb") as f:
            f.write(su.mb.tobytes())
            f.write(su.ts.tobytes())
        out = subprocess.run([exe, str(blob)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        kv = dict(w.split("=") for w in out.stdout.split())
        return {k: (int(v) if k.startswith("tree_") else [int(x) for x in v.split(",") if x]) for k, v in kv.items()}
    return dump


@pytest.fixture(scope="module")
def limits_input(oracle, g1):
    """G1, S=6, T=10, seed 21, scattered: (q0, human, oracle q, oracle solve counts).  Shared, never modified."""
    from general_motion_retargeting_amd import synth
    human, q0 = synth.make_streams(g1.model, g1.tt, 6, 10, seed=21)
    human = _scatter(human)
    q_o, ns_o, st_o = oracle.retarget_streams(g1.mb, g1.ts, q0, human)
    assert (st_o == 0).all()
    for a in (q0, human, q_o, ns_o):
        a.setflags(write=False)
    return q0, human, q_o, ns_o


def test_mirror_exercises_trunk_and_limb_multipliers(oracle, g1, tree_dump, limits_input):
    q0, human, q_o, ns_o = limits_input
    tree = tree_dump(g1)
    assert tree["tree_ok"] == 1
    trunk_mask = sum(1 << d for d in tree["trunk"])
    log = []
    for s in range(human.shape[0]):
        q_m, ns_m = bpp_mirror.retarget_stream(oracle, g1.mb, g1.ts, q0[s], human[s], log)
        assert np.array_equal(ns_m, ns_o[s]), f"stream {s}: the mirror's solve counts differ from the oracle's"
        assert np.abs(q_m - q_o[s]).max() <= 1e-8
    n_trunk, n_limb, rel_trunk, rel_limb = bpp_mirror.classify_rounds(log, trunk_mask)
    print(f"rounds: trunk fixed {n_trunk}, only limbs fixed {n_limb}; releases: trunk {rel_trunk}, limb {rel_limb}; "
          f"{len(log)} rounds for {int(ns_o.sum())} solves")
    assert n_trunk >= 100 and n_limb >= 100 and rel_trunk >= 10 and rel_limb >= 50, (n_trunk, n_limb, rel_trunk, rel_limb)


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _both_shapes(hip, mb, ts, q0, human):
    sol = hip.Solver(mb, ts)
    out = {}
    for waves in (4, 1):
        sol.set_waves(waves)
        out[waves] = sol.retarget_streams(q0, human)
    sol.set_waves(0)
    return out


@pytest.mark.gpu
def test_bound_path_matches_oracle_in_both_shapes(hip, g1, limits_input):
    q0, human, q_o, ns_o = limits_input
    out = _both_shapes(hip, g1.mb, g1.ts, q0, human)
    for waves, (q_h, ns_h, st_h) in out.items():
        assert (st_h == 0).all(), waves
        assert np.array_equal(ns_h, ns_o), f"{waves} wavefront(s): solve counts differ from the oracle's"
        err = np.abs(q_h - q_o).max()
        print(f"{waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
        assert err <= 1e-8, (waves, err)
    assert np.array_equal(out[4][1], out[1][1])
    d = np.abs(out[4][0] - out[1][0]).max()
    print(f"max |q_4 - q_1| = {d:.3e}")
    assert d <= 1e-12, d


@pytest.mark.gpu
@pytest.mark.parametrize("src,robot", ALL_CONFIGS)
def test_bound_path_all_configs(hip, oracle, src, robot):
    from general_motion_retargeting_amd import synth
    su = get_setup(src, robot, 1.7)
    human, q0 = synth.make_streams(su.model, su.tt, 3, 8, seed=5)
    human = _scatter(human)
    q_o, ns_o, st_o = oracle.retarget_streams(su.mb, su.ts, q0, human)
    assert (st_o == 0).all()
    for waves, (q_h, ns_h, st_h) in _both_shapes(hip, su.mb, su.ts, q0, human).items():
        assert (st_h == 0).all(), waves
        assert np.array_equal(ns_h, ns_o), f"{waves} wavefront(s): solve counts differ from the oracle's"
        err = np.abs(q_h - q_o).max()
        print(f"{src}/{robot} {waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
        assert err <= 1e-8, (waves, err)


class _Synthetic:
    """A robot outside the shipped set whose limbs have 8 dofs and whose trunk has 10 (floating base, two waist hinges,
    a two-hinge head): the layout selects the <8, 10> instance of the tree solver for it."""

    def __init__(self, tmp_path):
        from general_motion_retargeting_amd.ik_config import build_task_tables, pack_model, pack_taskset
        from general_motion_retargeting_amd.mjcf import compile_mjcf
        axes = ["1 0 0", "0 1 0", "0 0 1"]

        def chain(prefix, n, pos, inner=""):
            s, e = "", ""
            for i in range(n):
                s += (f'<body name="{prefix}{i}" pos="{pos if i == 0 else "0.02 0 -0.09"}" quat="0.98 0.1 0.05 0.12">'
                      f'<joint name="{prefix}j{i}" axis="{axes[(i + len(prefix)) % 3]}" range="-1.3 1.1"/>')
                e += "</body>"
            return s + inner + e
        upper = chain("a", 5, "0 0.2 0.2") + chain("b", 5, "0 -0.2 0.2") + chain("n", 2, "0 0 0.3")
        xml = ('<mujoco model="wide_trunk"><compiler angle="radian"/><worldbody><body name="base" pos="0 0 1"><freejoint/>'
               + chain("w", 2, "0 0 0.1", upper) + chain("l", 8, "0 0.1 0") + chain("r", 8, "0 -0.1 0")
               + "</body></worldbody></mujoco>")
        p = tmp_path / "wide_trunk.xml"
        p.write_text(xml)
        self.model = compile_mjcf(str(p))
        tasks = [("base", 100, 10), ("w1", 0, 10), ("l7", 50, 10), ("r7", 50, 10), ("a4", 10, 5), ("b4", 10, 5), ("n1", 0, 10)]
        names = [f"h{i}" for i in range(len(tasks))]
        tbl1 = {f: [h, wp, wr, [0.01, 0, 0], [1, 0, 0, 0]] for (f, wp, wr), h in zip(tasks, names)}
        tbl2 = {f: [h, wp * 2 + 1, max(wr / 2, 1), [0, 0, 0], [1, 0, 0, 0]] for (f, wp, wr), h in zip(tasks, names)}
        cfg = {"robot_root_name": "base", "human_root_name": "h0", "ground_height": 0.0, "human_height_assumption": 1.8,
               "use_ik_match_table1": True, "use_ik_match_table2": True, "human_scale_table": {n: 0.9 for n in names},
               "ik_match_table1": tbl1, "ik_match_table2": tbl2}
        self.tt = build_task_tables(cfg, 1.7)
        self.mb, self.ts = pack_model(self.model), pack_taskset(self.model, self.tt)


@pytest.fixture(scope="module")
def wide_trunk(tmp_path_factory):
    return _Synthetic(tmp_path_factory.mktemp("robot"))


def test_cases_cover_both_tree_solver_instances(tree_dump, wide_trunk):
    """`tree_small` of the packed layout over the cases of the GPU tests.  Every configuration of ALL_CONFIGS selects the
    <7, 9> instance (tree_small = 1 for all fourteen: no shipped robot has an 8-dof limb or a 10-dof trunk), so both
    values cannot come from ALL_CONFIGS alone; the synthetic robot of test_bound_path_large_instance supplies the other
    one, and the <8, 10> instance runs as well."""
    seen = {tree_dump(get_setup(src, robot, 1.7))["tree_small"] for src, robot in ALL_CONFIGS}
    assert seen == {1}, seen
    tree = tree_dump(wide_trunk)
    assert tree["tree_ok"] == 1 and tree["tree_small"] == 0 and len(tree["trunk"]) == 10, tree
    assert max(len(tree[f"limb{l}"]) for l in range(4)) == 8, tree


@pytest.mark.gpu
def test_bound_path_large_instance(hip, oracle, wide_trunk):
    """The <8, 10> instance (4 wavefronts) and the dense solver (1 wavefront) on scattered targets, S=3, T=8."""
    from general_motion_retargeting_amd import synth
    su = wide_trunk
    human, q0 = synth.make_streams(su.model, su.tt, 3, 8, seed=5)
    human = _scatter(human)
    q_o, ns_o, st_o = oracle.retarget_streams(su.mb, su.ts, q0, human)
    assert (st_o == 0).all()
    lo, hi = su.model.range_lo, su.model.range_hi
    th = q_o[..., 7:]
    at_limit = (np.abs(th - lo) < 1e-6) | (np.abs(th - hi) < 1e-6)
    assert at_limit[..., :2].any() and at_limit[..., 2:].any(), "the input must put waist and limb joints on their limits"
    for waves, (q_h, ns_h, st_h) in _both_shapes(hip, su.mb, su.ts, q0, human).items():
        assert (st_h == 0).all(), waves
        assert np.array_equal(ns_h, ns_o), f"{waves} wavefront(s): solve counts differ from the oracle's"
        err = np.abs(q_h - q_o).max()
        print(f"wide trunk, {waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
        assert err <= 1e-8, (waves, err)
