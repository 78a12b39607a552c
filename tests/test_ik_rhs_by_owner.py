"""The right-hand side of a pivoting round of the tree QP (csrc/gmr_ik_tree.h), formed by the owner of each row.

Host part: (1) the structure the change rests on -- H has exact zeros between two different limbs, for every shipped
configuration and both stages; (2) a NumPy mirror (tests/rhs_owner_mirror.py) of the by-owner sums against the dense
-c - H[:, fixed] x_fixed on every round of the joint-limit input of test_ik_bound_path.py -- the sum of the products
within 8 eps sum |H_ij x_j| (the same products in another order), the right-hand side itself within 8 eps (|c_i| + that
sum): c_i is one more term of the reordered sum and usually its largest, so a bound without it cannot hold; (3) the two streams of the
benchmark batch that the GPU part runs are the ones that were analysed (1 222 and 563 solves).
GPU part: those two streams -- the slowest of the batch, with 7 to 11 variables fixed at once across limbs and trunk,
and the median, which never fixes one -- against the oracle in both launch shapes, and twice for repeatability (a trunk
row's right-hand side now crosses wavefronts).
"""
import numpy as np
import pytest

import rhs_owner_mirror
from conftest import ALL_CONFIGS, get_setup
from test_ik_bound_path import _scatter, limits_input, tree_dump  # noqa: F401  (fixtures)

EPS = np.finfo(np.float64).eps


def _tree_lists(tree):
    return [tree[f"limb{l}"] for l in range(4)], tree["trunk"]


@pytest.mark.parametrize("src,robot", ALL_CONFIGS)
def test_h_is_zero_between_limbs(oracle, tree_dump, src, robot):
    from general_motion_retargeting_amd import synth
    su = get_setup(src, robot, 1.7)
    tree = tree_dump(su)
    assert tree["tree_ok"] == 1
    limbs, trunk = _tree_lists(tree)
    nv = int(su.mb["nv"][0])
    assert sorted(sum(limbs, []) + trunk) == list(range(nv)), "limbs and trunk must partition the dofs"
    human, q0 = synth.make_streams(su.model, su.tt, 3, 8, seed=5)
    human = _scatter(human)
    stages = [st for st in range(2) if int(su.ts["use_stage"][0][st])]
    assert stages
    for s in range(human.shape[0]):
        tgt = oracle.preprocess(su.ts, human[s, 0])
        for stage in stages:
            H = oracle.build_qp(su.mb, su.ts, stage, q0[s], tgt)[0]
            assert np.isfinite(H).all()
            for i in range(4):
                for j in range(4):
                    if i != j and limbs[i] and limbs[j]:
                        blk = H[np.ix_(limbs[i], limbs[j])]
                        assert (blk == 0.0).all(), (src, robot, stage, i, j, np.abs(blk).max())


def test_rhs_by_owner_matches_dense(oracle, g1, tree_dump, limits_input):
    q0, human, q_o, ns_o = limits_input
    tree = tree_dump(g1)
    limbs, trunk = _tree_lists(tree)
    limb_masks = [sum(1 << d for d in limb) for limb in limbs]
    trunk_mask = sum(1 << d for d in trunk)
    n_rounds = n_fixed = n_two_limbs = n_trunk_and_limb = 0
    worst = 0.0
    for s in range(human.shape[0]):
        q_m, ns_m, rounds = rhs_owner_mirror.capture_rounds(oracle, g1.mb, g1.ts, q0[s], human[s])
        assert np.array_equal(ns_m, ns_o[s])
        for H, c, lo, hi, lower, upper in rounds:
            n_rounds += 1
            fixedm = lower | upper
            if not fixedm:
                continue
            n_fixed += 1
            in_limbs = sum(1 for m in limb_masks if fixedm & m)
            n_two_limbs += in_limbs >= 2
            n_trunk_and_limb += bool(fixedm & trunk_mask) and in_limbs >= 1
            xfix, free = rhs_owner_mirror.bound_values(lo, hi, lower, upper)
            fixed = ~free
            rhs, products = rhs_owner_mirror.rhs_by_owner(H, c, xfix, free, limbs, trunk)
            terms = (np.abs(H[:, fixed]) * np.abs(xfix[fixed])).sum(axis=1)
            # the sum over the fixed columns: the same products in another order, the reordering bound of a sum of at
            # most a dozen terms
            d_prod = np.abs(products - H[:, fixed] @ xfix[fixed])[free]
            assert (d_prod <= (8 * EPS * terms)[free]).all(), (s, n_rounds, d_prod.max())
            # the right-hand side itself has one more term, c_i, whose magnitude enters the bound of the reordered sum
            d_rhs = np.abs(rhs - (-c - H[:, fixed] @ xfix[fixed]))[free]
            assert (d_rhs <= (8 * EPS * (np.abs(c) + terms))[free]).all(), (s, n_rounds, d_rhs.max())
            worst = max(worst, float((d_prod / np.maximum(8 * EPS * terms[free], 1e-300)).max()))
    print(f"{n_rounds} rounds: {n_fixed} with a fixed set, {n_two_limbs} with two or more limbs in it, "
          f"{n_trunk_and_limb} with trunk and limb together; largest |difference| / bound = {worst:.3f}")
    assert n_fixed >= 900 and n_two_limbs >= 400 and n_trunk_and_limb >= 200, (n_fixed, n_two_limbs, n_trunk_and_limb)


@pytest.fixture(scope="module")
def bench_streams(oracle, g1):
    """Streams 89 and 64 of the benchmark's batch (100 frames, seed 0) with the oracle's result.  Shared, never modified."""
    from general_motion_retargeting_amd import synth
    human, q0 = synth.make_streams_ids(g1.model, g1.tt, [89, 64], 100, seed=0)
    q_o, ns_o, st_o = oracle.retarget_streams(g1.mb, g1.ts, q0, human)
    assert (st_o == 0).all()
    for a in (q0, human, q_o, ns_o):
        a.setflags(write=False)
    return q0, human, q_o, ns_o


def test_bench_streams_are_the_analysed_ones(bench_streams):
    ns_o = bench_streams[3]
    assert [int(ns_o[s].sum()) for s in range(2)] == [1222, 563]


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _launch(hip, g1, q0, human, waves):
    sol = hip.Solver(g1.mb, g1.ts)
    sol.set_waves(waves)
    out = sol.retarget_streams(q0, human)
    sol.set_waves(0)
    return out


@pytest.fixture(scope="module")
def first_launch(hip, g1, bench_streams):
    q0, human = bench_streams[:2]
    return {waves: _launch(hip, g1, q0, human, waves) for waves in (4, 1)}


@pytest.mark.gpu
def test_bench_streams_match_oracle_in_both_shapes(first_launch, bench_streams):
    q0, human, q_o, ns_o = bench_streams
    for waves, (q_h, ns_h, st_h) in first_launch.items():
        assert (st_h == 0).all(), waves
        assert np.array_equal(ns_h, ns_o), f"{waves} wavefront(s): solve counts differ from the oracle's"
        err = np.abs(q_h - q_o).max()
        print(f"{waves} wavefront(s): max |q - q_oracle| = {err:.3e}")
        assert err <= 1e-8, (waves, err)
    assert np.array_equal(first_launch[4][1], first_launch[1][1])
    d = np.abs(first_launch[4][0] - first_launch[1][0]).max()
    print(f"max |q_4 - q_1| = {d:.3e}")
    assert d <= 1e-12, d


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [4, 1])
def test_bench_streams_repeat_bitwise(hip, g1, first_launch, bench_streams, waves):
    q0, human = bench_streams[:2]
    q_a, ns_a, _ = first_launch[waves]
    q_b, ns_b, st_b = _launch(hip, g1, q0, human, waves)
    assert (st_b == 0).all()
    assert np.array_equal(ns_a, ns_b)
    assert np.array_equal(q_a, q_b)
