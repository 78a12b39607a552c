"""div_const of csrc/gmr_device_math.h gives the bits of the division, for every literal the header divides a variable by.

The helper's three operations (multiply by the rounded reciprocal, exact remainder by one fused multiply-add, fused
correction) are mirrored on the host with exactly rounded fused multiply-adds (tests/div_const_cases.py) and compared
with the correctly rounded quotient:

  midpoint set   45 000 numerators per literal whose quotients lie as close to a rounding midpoint as a 53-bit numerator
                 allows; every one goes through rationals (`fractions`): helper and quotient
  random set     2^20 numerators per literal, signs mixed, exponents -110 .. +5; the fused operations are evaluated by the
                 vectorised error-free engine and the quotient by the IEEE division of NumPy, and both engines are held
                 to the rationals on the first 4096 numerators of the set and on the whole midpoint set (9.4 million
                 numerators through `fractions` would take minutes)

No numerator is left out, and no literal is excused.
"""
from fractions import Fraction

import numpy as np
import pytest

import div_const_cases as dc


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def numerators():
    return dc.random_numerators()


def test_literals_are_the_headers():
    """the list follows the header: every div_const(..., literal) there is in LITERALS, and nothing else is"""
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "general_motion_retargeting_amd", "csrc", "gmr_device_math.h")).read()
    body = src.split("double div_const(double x, double c) {", 1)[1]
    found = {float(m) for m in re.findall(r"div_const\([^;]*?, ([0-9.]+)\)", body)}
    assert found == set(dc.LITERALS), found ^ set(dc.LITERALS)
    assert not re.search(r"t2 / [0-9]|t / [0-9]", body), "a literal division of a variable is left in the header"


@pytest.mark.parametrize("c", dc.LITERALS)
def test_midpoint_set_exact(c):
    x = dc.midpoint_numerators(c)
    assert x.size == 3 * dc.N_MIDPOINT
    fc = Fraction(c)
    got = np.array([dc.div_const_exact(v, c) for v in x.tolist()])
    want = np.array([float(Fraction(v) / fc) for v in x.tolist()])
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (c, bad.size, [float.hex(float(x[i])) for i in bad[:4]])
    # both vectorised engines agree with the rationals here too
    assert np.array_equal(_bits(dc.div_const_np(x, c)), _bits(got)), c
    assert np.array_equal(_bits(x / c), _bits(want)), c


@pytest.mark.parametrize("c", dc.LITERALS)
def test_random_set(numerators, c):
    x = numerators
    assert x.size == 1 << 20 and (x < 0).any() and (x > 0).any()
    e = np.frexp(x)[1] - 1
    assert e.min() == -110 and e.max() == 5
    got = dc.div_const_np(x, c)
    want = x / c
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (c, bad.size, [float.hex(float(x[i])) for i in bad[:4]])
    # the engines against rationals on a slice of the same numerators
    head = x[:4096].tolist()
    fc = Fraction(c)
    assert np.array_equal(_bits([dc.div_const_exact(v, c) for v in head]), _bits(got[:4096])), c
    assert np.array_equal(_bits([float(Fraction(v) / fc) for v in head]), _bits(want[:4096])), c


def test_fma_engines_agree_on_hard_cases():
    """fma_np against rationals where the low part decides the rounding (1 + 2^-53 + 2^-106 and neighbours)"""
    a = 1.0 + 2.0 ** -27
    assert dc.fma_exact(a, a, -1.0) == 2.0 ** -26 + 2.0 ** -54
    rng = np.random.default_rng(3)
    p = 1.0 + rng.random(20000)
    q = 1.0 + rng.random(20000)
    # c cancels the product's high part, or sits half an ulp away from it
    for cc in (-(p * q), -(p * q) * (1.0 + 2.0 ** -52), np.ldexp(p, -53), np.ldexp(q, 53)):
        got = dc.fma_np(p, q, cc)
        want = [dc.fma_exact(u, v, w) for u, v, w in zip(p.tolist(), q.tolist(), np.asarray(cc).tolist())]
        assert np.array_equal(_bits(got + 0.0), _bits(np.asarray(want) + 0.0))
