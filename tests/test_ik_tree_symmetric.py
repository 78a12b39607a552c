"""The tree QP on full symmetric rows (csrc/gmr_ik_tree.h): each lane takes its column of the lower factor from its own
row, so neither the limb factor, nor Y_l, nor the trunk factor is transposed through LDS.

Host part (tests/tree_sym_mirror.py, exact fused multiply-adds): on 20 local matrices -- the <7, 9> and the <8, 10>
shape, five kinds of fixed set, two seeds each -- the scaled upper part of lane p equals column p of the lower factor
bit for bit, and that factor equals the one eliminated from lower-triangular rows bit for bit.  A second host test shows
that the bound-free GPU input really never fixes a variable.  GPU part: the inputs of tests/test_ik_bound_path.py (G1,
S = 6 x T = 10, seed 21: rounds with trunk and with limb variables fixed; the synthetic robot of the <8, 10> instance)
and the bound-free input, both launch shapes against the oracle.
"""
import numpy as np
import pytest

import bpp_mirror
import tree_sym_mirror as tsm
from test_ik_bound_path import _both_shapes, _scatter, hip, limits_input, wide_trunk  # noqa: F401  (fixtures)

SHAPES = [(7, 9), (8, 10)]
# rows / columns replaced by identity, as (limb rows, trunk rows): variables on a bound; the padding case drops the last
# limb row and the last trunk row (a limb / trunk shorter than the instance) and fixes one more of each
FIXED = {
    "none": lambda nl, nt: ([], []),
    "limb": lambda nl, nt: ([1, nl - 2], []),
    "trunk": lambda nl, nt: ([], [0, nt - 3]),
    "both": lambda nl, nt: ([0, 3, nl - 1], [2, nt - 1]),
    "padding": lambda nl, nt: ([2, nl - 1], [4, nt - 1]),
}
CASES = [(nl, nt, kind, seed) for nl, nt in SHAPES for kind in FIXED for seed in (0, 1)]
assert len(CASES) == 20


@pytest.mark.parametrize("nl,nt,kind,seed", CASES)
def test_own_row_is_the_factor_column(nl, nt, kind, seed):
    rng = np.random.default_rng(1000 * nl + 10 * seed + len(kind))
    A = tsm.spd_symmetric(rng, nl + nt)
    assert np.array_equal(A, A.T)
    fl, ft = FIXED[kind](nl, nt)
    fixed = set(fl) | {nl + t for t in ft}
    full = tsm.eliminate(A, nl, nt, fixed, full=True)
    lower = tsm.eliminate(A, nl, nt, fixed, full=False)
    for own, col in (("ltl", "L_l"), ("yl", "Y_l"), ("lt", "L_t")):
        assert np.array_equal(tsm.bits(full[own]), tsm.bits(full[col])), (own, "differs from the column the lanes below hold")
        assert np.array_equal(tsm.bits(full[col]), tsm.bits(lower[col])), (col, "differs from the factor of lower-triangular rows")
    # the factor is not trivial: every free pair below the diagonal is non-zero, every fixed row / column is zero
    L = np.asarray(full["L_l"])
    for m in range(nl):
        for a in range(m):
            assert (L[m, a] != 0.0) == (m not in fixed and a not in fixed), (m, a)
    Y = np.asarray(full["Y_l"])
    for u in range(nt):
        for a in range(nl):
            assert (Y[u, a] != 0.0) == (nl + u not in fixed and a not in fixed), (u, a)


def test_exact_fma_is_one_rounding():
    # 1 + 2^-53 + 2^-106 needs the unrounded product: two roundings give 1.0
    a = 1.0 + 2.0 ** -27
    assert tsm.fma(a, a, -1.0) == 2.0 ** -26 + 2.0 ** -54 and a * a - 1.0 == 2.0 ** -26
    assert np.signbit(tsm.fma(-0.0, 3.0, -0.0)) and not np.signbit(tsm.fma(-0.0, 3.0, 0.0))
    assert tsm.fma(3.0, 5.0, -15.0) == 0.0 and not np.signbit(tsm.fma(3.0, 5.0, -15.0))


@pytest.fixture(scope="module")
def free_input(oracle, g1):
    """G1 from the default configuration, S = 2 x T = 4, targets as generated: (q0, human, oracle q, oracle solve counts).
    Seed 6 is the first whose streams keep every variable inside its bounds in every round (seeds 0 .. 5 put a joint on
    a limit in 3 to 72 rounds); test_free_input_never_fixes_a_variable holds it to that."""
    from general_motion_retargeting_amd import synth
    human, q0 = synth.make_streams(g1.model, g1.tt, 2, 4, seed=6)
    assert np.array_equal(q0, np.broadcast_to(g1.model.qpos0, q0.shape))
    q_o, ns_o, st_o = oracle.retarget_streams(g1.mb, g1.ts, q0, human)
    assert (st_o == 0).all()
    for a in (q0, human, q_o, ns_o):
        a.setflags(write=False)
    return q0, human, q_o, ns_o


def test_free_input_never_fixes_a_variable(oracle, g1, free_input):
    q0, human, q_o, ns_o = free_input
    log = []
    for s in range(human.shape[0]):
        q_m, ns_m = bpp_mirror.retarget_stream(oracle, g1.mb, g1.ts, q0[s], human[s], log)
        assert np.array_equal(ns_m, ns_o[s])
        assert np.abs(q_m - q_o[s]).max() <= 1e-8
    assert len(log) == int(ns_o.sum()), "one round per solve"
    assert all(fixed == 0 and released == 0 for fixed, released in log)


def _check(out, q_o, ns_o, what):
    for waves, (q_h, ns_h, st_h) in out.items():
        assert (st_h == 0).all(), (what, waves)
        assert np.array_equal(ns_h, ns_o), f"{what}, {waves} wavefront(s): solve counts differ from the oracle's"
        err = np.abs(q_h - q_o).max()
        print(f"{what}, {waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
        assert err <= 1e-8, (what, waves, err)
    assert np.array_equal(out[4][1], out[1][1]), what
    d = np.abs(out[4][0] - out[1][0]).max()
    print(f"{what}: max |q_4 - q_1| = {d:.3e}")
    assert d <= 1e-12, (what, d)


@pytest.mark.gpu
def test_symmetric_rows_bound_input(hip, g1, limits_input):
    q0, human, q_o, ns_o = limits_input
    _check(_both_shapes(hip, g1.mb, g1.ts, q0, human), q_o, ns_o, "G1 6 x 10 scattered")


@pytest.mark.gpu
def test_symmetric_rows_free_input(hip, g1, free_input):
    q0, human, q_o, ns_o = free_input
    _check(_both_shapes(hip, g1.mb, g1.ts, q0, human), q_o, ns_o, "G1 2 x 4 from the default configuration")


@pytest.mark.gpu
def test_symmetric_rows_large_instance(hip, oracle, wide_trunk):
    """The <8, 10> instance (4 wavefronts; the 1-wavefront shape runs the dense solver for this robot)."""
    from general_motion_retargeting_amd import synth
    su = wide_trunk
    human, q0 = synth.make_streams(su.model, su.tt, 3, 8, seed=5)
    human = _scatter(human)
    q_o, ns_o, st_o = oracle.retarget_streams(su.mb, su.ts, q0, human)
    assert (st_o == 0).all()
    _check(_both_shapes(hip, su.mb, su.ts, q0, human), q_o, ns_o, "wide trunk 3 x 8 scattered")
