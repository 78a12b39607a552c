"""-m gpu: the tree QP with its row broadcasts folded into the multiply-adds (csrc/gmr_ik_tree.h, row_bcast_fma and its
multi-update forms in csrc/gmr_device_math.h) and the short division by literals (div_const), end to end.

The inputs of tests/test_ik_bound_path.py (G1, S = 6 x T = 10, seed 21, scattered: rounds with trunk and with limb
variables fixed and releases of both kinds -- the only rounds that execute the folded right-hand-side sums and the folded
multiplier products) and the bound-free input of tests/test_ik_tree_symmetric.py, both launch shapes against the oracle:
equal solve counts, |q - q_oracle| <= 1e-8, |q_4 - q_1| <= 1e-12 (the bounds of those modules, unchanged).  These are the
smallest inputs that reach every folded site.
"""
import numpy as np
import pytest

from test_ik_bound_path import _both_shapes, hip, limits_input  # noqa: F401  (fixtures)
from test_ik_tree_symmetric import free_input  # noqa: F401  (fixture)


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
def test_fused_paths_bound_input(hip, g1, limits_input):
    q0, human, q_o, ns_o = limits_input
    _check(_both_shapes(hip, g1.mb, g1.ts, q0, human), q_o, ns_o, "G1 6 x 10 scattered")


@pytest.mark.gpu
def test_fused_paths_free_input(hip, g1, free_input):
    q0, human, q_o, ns_o = free_input
    _check(_both_shapes(hip, g1.mb, g1.ts, q0, human), q_o, ns_o, "G1 2 x 4 from the default configuration")
