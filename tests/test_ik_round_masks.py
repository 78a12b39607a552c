"""The masks of a pivoting round of the tree QP (csrc/gmr_ik_tree.h): identity pivots of fixed and padding rows.

A fixed or padding row of the local matrix is an identity row.  The kernel keeps such a row at zero and hands the pivot
the 1.0 of its diagonal from the column's bit of the round's ballot, and a trunk lane reads its rows of the four Schur
parts as 16-byte pieces.  The cases below aim at what that could break: rounds without any fixed variable (only the
padding columns of the 6-dof legs are identity pivots), rounds in which every pivot of one wavefront is an identity
pivot, identity pivots at both ends of the boundable part of the trunk order, a fixed variable next to a padding
column, a variable released in the round after it was fixed, and the <8, 10> instance.

Every case is the packed G1 model with joint ranges narrowed in a copy of the blob (qpos0 has every hinge at zero, so
[-0.01, 0.01] holds the start), or the synthetic robot of test_ik_bound_path.py.  Host part: the round log of
tests/bpp_mirror.py shows that the case occurs in the input.  GPU part: both launch shapes against the oracle, with the
tolerances of test_ik_bound_path.py.  Seeds were chosen on the CPU so that the oracle returns status 0 for every stream.

The floating base has no bounds (lo = -inf, hi = +inf), so columns 0 .. 5 of the trunk are never fixed: the first and
the last trunk column that CAN be fixed are the first and the last waist hinge (trunk columns 6 and 8 of G1).
"""
import os
import subprocess

import numpy as np
import pytest

import bpp_mirror
from conftest import ALL_CONFIGS, ROOT, get_setup
from test_ik_bound_path import _both_shapes, _scatter, hip, tree_dump, wide_trunk  # noqa: F401  (fixtures)

HALF = 0.01                                        # narrowed range: [-HALF, HALF] rad around the start angle 0

# name -> (which dofs get the narrow range, given the decomposition), S, T, seed, scattered targets
CASES = {
    "plain":       (lambda tree: [], 4, 6, 6, False),
    "arm_limb":    (lambda tree: tree["limb0"], 4, 6, 21, True),
    "leg_limb":    (lambda tree: tree["limb2"], 4, 6, 21, True),
    "waist_all":   (lambda tree: tree["trunk"][6:], 4, 6, 21, True),
    "waist_first": (lambda tree: tree["trunk"][6:7], 4, 6, 21, True),
    "waist_last":  (lambda tree: tree["trunk"][-1:], 4, 6, 21, True),
    "hip_by_pad":  (lambda tree: tree["limb2"][-1:], 4, 6, 21, True),
}


def _mask(dofs):
    return sum(1 << d for d in dofs)


@pytest.fixture(scope="module")
def g1_tree(g1, tree_dump):
    tree = tree_dump(g1)
    assert tree["tree_ok"] == 1 and tree["tree_small"] == 1
    assert tree["trunk"][:6] == [0, 1, 2, 3, 4, 5] and len(tree["trunk"]) == 9
    assert len(tree["limb0"]) == 7 and len(tree["limb2"]) == 6      # an arm fills the 7-wide limb rows, a leg has a padding column
    return tree


@pytest.fixture(scope="module")
def case_input(oracle, g1, g1_tree):
    """name -> (blob, narrowed dofs, q0, human, oracle q, oracle solve counts), computed once per case, never modified."""
    from general_motion_retargeting_amd import synth
    cache = {}

    def get(name):
        if name not in cache:
            pick, S, T, seed, scatter = CASES[name]
            dofs = pick(g1_tree)
            mb = g1.mb.copy()
            for d in dofs:
                mb["range_lo"][0][d - 6], mb["range_hi"][0][d - 6] = -HALF, HALF
            human, q0 = synth.make_streams(g1.model, g1.tt, S, T, seed=seed)
            if scatter:
                human = _scatter(human)
            q_o, ns_o, st_o = oracle.retarget_streams(mb, g1.ts, q0, human)
            assert (st_o == 0).all(), (name, st_o)
            for a in (mb, q0, human, q_o, ns_o):
                a.setflags(write=False)
            cache[name] = (mb, dofs, q0, human, q_o, ns_o)
        return cache[name]
    return get


def _round_log(oracle, g1, case):
    mb, dofs, q0, human, q_o, ns_o = case
    log = []
    for s in range(human.shape[0]):
        q_m, ns_m = bpp_mirror.retarget_stream(oracle, mb, g1.ts, q0[s], human[s], log)
        assert np.array_equal(ns_m, ns_o[s]), f"stream {s}: the mirror's solve counts differ from the oracle's"
        assert np.abs(q_m - q_o[s]).max() <= 1e-8
    return log


@pytest.mark.parametrize("name", list(CASES))
def test_case_occurs_in_input(oracle, g1, g1_tree, case_input, name):
    """The mirror's round log (fixed set, released set per round) holds the rounds the case is named after."""
    case = case_input(name)
    dofs = case[1]
    log = _round_log(oracle, g1, case)
    waist = _mask(g1_tree["trunk"][6:])
    every = sum(1 for fixed, _ in log if fixed & _mask(dofs) == _mask(dofs))
    print(f"{name}: {len(log)} rounds, {sum(1 for f, _ in log if f)} with a fixed variable, {every} with all of {dofs} fixed")
    if name == "plain":
        assert all(fixed == 0 for fixed, _ in log) and len(log) >= 100
    elif name in ("arm_limb", "leg_limb", "waist_all"):
        assert every >= 50, every                  # every pivot of the limb (all three waist pivots) is an identity pivot
    elif name in ("waist_first", "waist_last"):
        alone = sum(1 for fixed, _ in log if fixed & waist == _mask(dofs))
        assert alone >= 50, alone                  # the only fixed trunk column of the round
    else:
        assert dofs == [g1_tree["limb2"][5]]       # column 5 of the leg's rows; column 6 is the padding column
        assert every >= 50, every
        # not in the fixed set of round i, fixed and released in round i + 1 (a solve's first round starts from the sets its
        # predecessor ended with, so such a pair always lies inside one solve)
        again = sum(bin(~f0 & f1 & r1).count("1") for (f0, _), (f1, r1) in zip(log, log[1:]))
        assert again >= 1, again


def _compare(out, q_o, ns_o, label, between_shapes):
    for waves, (q_h, ns_h, st_h) in out.items():
        assert (st_h == 0).all(), (label, waves)
        assert np.array_equal(ns_h, ns_o), f"{label}, {waves} wavefront(s): solve counts differ from the oracle's"
        err = np.abs(q_h - q_o).max()
        print(f"{label}, {waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
        assert err <= 1e-8, (label, waves, err)
    if between_shapes:
        assert np.array_equal(out[4][1], out[1][1])
        d = np.abs(out[4][0] - out[1][0]).max()
        print(f"{label}: max |q_4 - q_1| = {d:.3e}")
        assert d <= 1e-12, (label, d)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_round_masks_match_oracle_in_both_shapes(hip, g1, case_input, name):
    mb, dofs, q0, human, q_o, ns_o = case_input(name)
    _compare(_both_shapes(hip, mb, g1.ts, q0, human), q_o, ns_o, name, True)


@pytest.fixture(scope="module")
def wide_input(oracle, wide_trunk):
    from general_motion_retargeting_amd import synth
    su = wide_trunk
    human, q0 = synth.make_streams(su.model, su.tt, 4, 6, seed=5)
    human = _scatter(human)
    q_o, ns_o, st_o = oracle.retarget_streams(su.mb, su.ts, q0, human)
    assert (st_o == 0).all()
    for a in (q0, human, q_o, ns_o):
        a.setflags(write=False)
    return q0, human, q_o, ns_o


def test_large_instance_case_occurs(oracle, tree_dump, wide_trunk, wide_input):
    """The synthetic robot selects the <8, 10> instance, and the scatter fixes trunk (waist, head) and limb variables."""
    q0, human, q_o, ns_o = wide_input
    tree = tree_dump(wide_trunk)
    assert tree["tree_ok"] == 1 and tree["tree_small"] == 0, tree
    log = _round_log(oracle, wide_trunk, (wide_trunk.mb, [], q0, human, q_o, ns_o))
    hinges = _mask(tree["trunk"][6:])
    n_trunk = sum(1 for fixed, _ in log if fixed & hinges)
    n_limb = sum(1 for fixed, _ in log if fixed & ~hinges)
    print(f"wide trunk: {len(log)} rounds, {n_trunk} with a trunk hinge fixed, {n_limb} with a limb variable fixed")
    assert n_trunk >= 20 and n_limb >= 50, (n_trunk, n_limb)


@pytest.mark.gpu
def test_round_masks_large_instance(hip, wide_trunk, wide_input):
    """<8, 10> (four wavefronts, v_readlane broadcasts) and the dense solver (one wavefront) on the bound-heavy scatter."""
    q0, human, q_o, ns_o = wide_input
    _compare(_both_shapes(hip, wide_trunk.mb, wide_trunk.ts, q0, human), q_o, ns_o, "wide trunk", False)


# ---- the exchange buffers in the LDS layout -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def exchange_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("exchange")
    exe = str(d / "exchange_layout")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "exchange_layout.cpp")])

    def dump(su):
        blob = d / "blob.bin"
        with open(blob, "wb") as f:
            f.write(su.mb.tobytes())
            f.write(su.ts.tobytes())
        out = subprocess.run([exe, str(blob)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        rows = [{k: int(v) for k, v in (w.split("=") for w in line.split())} for line in out.stdout.splitlines()]
        return {r["nw"]: r for r in rows}
    return dump


def _check_exchange(lay, label):
    for nw, L in lay.items():
        # 16-byte boundaries: a row of a Schur part is 80 B, the parts are 800 B apart, the kernel reads 16-byte pieces
        assert L["spart"] % 2 == 0 and L["rpart"] % 2 == 0 and (nw == 1 or L["gpart"] % 2 == 0), (label, L)
        assert L["rpart"] >= L["spart"] + 4 * 10 * 10, (label, L)
        if nw == 4:                                                  # a region of their own behind c, x, lo, hi and the scalars
            assert L["spart"] >= L["c"] + 4 * L["nvp"] + 2 and L["gpart"] >= L["rpart"] + 40 and L["gpart"] + 40 <= L["n_double"], (label, L)
        else:                                                        # behind the 4 x 16 x 19 doubles of the dead assembly scratch, below H
            assert L["spart"] >= L["Kt"] + 4 * 16 * 19 and L["rpart"] + 40 <= L["H"], (label, L)
        assert 0 < L["smem"] <= 160 * 1024 - 1024, (label, L)       # what the launcher accepts (tests/cpp/layout_check.cpp)


@pytest.mark.parametrize("src,robot", ALL_CONFIGS)
def test_exchange_buffers_fit_and_are_aligned(exchange_layout, src, robot):
    _check_exchange(exchange_layout(get_setup(src, robot, 1.7)), f"{src}/{robot}")


def test_exchange_buffers_of_the_large_instance(exchange_layout, wide_trunk):
    _check_exchange(exchange_layout(wide_trunk), "wide trunk")
