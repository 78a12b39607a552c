"""-m gpu: the folded row broadcasts (row_bcast_fma, row_bcast_fnma_bcast, row_bcast_fnma_cols, row_bcast_fma_dot) and
div_const of csrc/gmr_device_math.h on the GPU (tests/hip/rowfma_probe.hip, built by build.build_rowfma_probe()).

  (a) the primitive for K = 0 .. 15 and both signs against fma(+-row_bcast_d(v, K), m, acc) on 64 lanes of random doubles
      with +0 and -0 among them: equal bits in all four 16-lane rows, and equal to the exactly rounded host value
  (b) one whole local elimination and solve of the <7, 9> shape written both ways (folded forms / row_bcast_d + fma) on
      the ten <7, 9> cases of tests/test_ik_tree_symmetric.py: factor, Y_l, Schur part, substituted right-hand sides and
      solution are bit-equal to each other, the factors to tree_sym_mirror.eliminate(.., full=True), the rest to a host
      mirror of the same operations built on tree_sym_mirror.fma
  (c) div_const against the division on the device, for every literal, over the midpoint set of tests/test_div_const.py

One wavefront and one launch for (a) and for (b), one launch for (c).
"""
import ctypes as C
import math

import numpy as np
import pytest

import div_const_cases as dc
import tree_sym_mirror as tsm
from test_ik_tree_symmetric import CASES, FIXED

pytestmark = pytest.mark.gpu

NL, NT, NV = 7, 9, 16
CASES_79 = [c for c in CASES if c[:2] == (NL, NT)]
assert len(CASES_79) == 10


@pytest.fixture(scope="module")
def probe():
    """a GPU host without the probe is a failure, not a skip"""
    from general_motion_retargeting_amd import _lib, build
    _lib.require_gpu()
    try:
        path = build.build_rowfma_probe()
    except Exception as exc:   # noqa: BLE001
        pytest.fail(f"the row-broadcast probe is missing and could not be built: {exc}")
    return C.CDLL(path)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- (a) ---------------------------------------------------------------------------------------------------------------
def test_primitive_matches_broadcast_and_fma(probe):
    rng = np.random.default_rng(7)
    v, m, acc = (rng.normal(size=64) * 10.0 ** rng.integers(-3, 4, size=64) for _ in range(3))
    v[[3, 21, 40]] = 0.0
    v[[9, 58]] = -0.0
    m[[0, 21, 33]] = 0.0
    m[[5, 47]] = -0.0
    acc[[2, 21, 50]] = 0.0
    acc[[5, 9, 63]] = -0.0
    prim, ref = np.empty((16, 2, 64)), np.empty((16, 2, 64))
    rc = probe.gmr_probe_rowfma_prim(_p(v), _p(m), _p(acc), _p(prim), _p(ref))
    assert rc == 0, f"gmr_probe_rowfma_prim: HIP error {rc}"
    assert np.array_equal(_u64(prim), _u64(ref))
    want = np.empty_like(prim)
    for k in range(16):
        for lane in range(64):
            src = v[16 * (lane // 16) + k]
            want[k, 0, lane] = tsm.fma(src, m[lane], acc[lane])
            want[k, 1, lane] = tsm.fma(-src, m[lane], acc[lane])
    assert np.array_equal(_u64(prim), _u64(want))
    assert np.signbit(want).any() and (want == 0.0).any()


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def _mirror_solve(A, rhs, fixed):
    """The operations of local_solve in tests/hip/rowfma_probe.hip, lane by lane, with exactly rounded fused
    multiply-adds.  Returns {schur[t][u], y[lane], yt[lane], x[lane]}."""
    free = [i not in fixed for i in range(NV)]
    r = []
    for i in range(NV):
        limb = i < NL
        row = [0.0] * NV
        for m in range(NL):
            if free[i] and free[m]:
                row[m] = float(A[i, m])
            if limb and m == i and not (free[i] and free[m]):
                row[m] = 1.0
        if limb and free[i]:
            for u in range(NT):
                if free[NL + u]:
                    row[NL + u] = float(A[i, NL + u])
        r.append(row)
    b = [float(rhs[i]) if i < NL else 0.0 for i in range(NV)]
    mydinv = [1.0] * NV
    for p in range(NL):
        dinv = 1.0 / math.sqrt(r[p][p])
        mydinv[p] = dinv
        l = [r[i][p] * dinv if i > p else 0.0 for i in range(NV)]
        yp = b[p] * dinv
        for i in range(NV):
            b[i] = tsm.fma(-l[i], yp, b[i])
            for k in range(p + 1, NV):
                r[i][k] = tsm.fma(-l[i], l[k], r[i][k])
    for i in range(NL):
        b[i] *= mydinv[i]
    yl = [[r[a][NL + u] * mydinv[a] for u in range(NT)] for a in range(NL)]
    ltl = [[r[a][m] * mydinv[a] if m > a else 0.0 for m in range(NL)] for a in range(NL)]
    schur = [[r[NL + t][NL + u] for u in range(NT)] for t in range(NT)]
    s = [[0.0] * NT for _ in range(NT)]
    bt = [0.0] * NT
    for t in range(NT):
        live = free[NL + t]
        for u in range(NT):
            ok = live and free[NL + u]
            s[t][u] = float(A[NL + t, NL + u]) + r[NL + t][NL + u] if ok else 0.0
            if u == t and not ok:
                s[t][u] = 1.0
        bt[t] = float(rhs[NL + t]) + b[NL + t] if live else float(rhs[NL + t])
    tdinv = [1.0] * NT
    for q in range(NT):
        dinv = 1.0 / math.sqrt(s[q][q])
        tdinv[q] = dinv
        l = [s[t][q] * dinv if t > q else 0.0 for t in range(NT)]
        yq = bt[q] * dinv
        for t in range(NT):
            bt[t] = tsm.fma(-l[t], yq, bt[t])
            for k in range(q + 1, NT):
                s[t][k] = tsm.fma(-l[t], l[k], s[t][k])
    lt = [[s[t][q] * tdinv[t] if q > t else 0.0 for q in range(NT)] for t in range(NT)]
    bt = [bt[t] * tdinv[t] for t in range(NT)]
    yt = list(bt)
    for q in range(NT - 1, -1, -1):
        xq = bt[q] * tdinv[q]
        bt = [tsm.fma(-lt[t][q], xq, bt[t]) for t in range(NT)]
    xt = [bt[t] * tdinv[t] for t in range(NT)]
    bb = b[:NL]
    for u in range(NT):
        bb = [tsm.fma(-yl[a][u], xt[u], bb[a]) for a in range(NL)]
    for p in range(NL - 1, -1, -1):
        xp = bb[p] * mydinv[p]
        bb = [tsm.fma(-ltl[a][p], xp, bb[a]) for a in range(NL)]
    xl = [bb[a] * mydinv[a] for a in range(NL)]
    return {"schur": schur, "y": b, "yt": [0.0] * NL + yt, "x": xl + xt}


@pytest.fixture(scope="module")
def eliminations(probe):
    """the ten cases (padded to twelve with the first two: four cases per trip of the wavefront), one launch"""
    mats, rhss, fixeds = [], [], []
    for nl, nt, kind, seed in CASES_79:
        rng = np.random.default_rng(1000 * nl + 10 * seed + len(kind))
        A = tsm.spd_symmetric(rng, NV)
        fl, ft = FIXED[kind](nl, nt)
        mats.append(A)
        rhss.append(rng.normal(size=NV))
        fixeds.append(set(fl) | {nl + t for t in ft})
    pad = [0, 1]
    A = np.ascontiguousarray(np.stack(mats + [mats[i] for i in pad]))
    rhs = np.ascontiguousarray(np.stack(rhss + [rhss[i] for i in pad]))
    masks = np.array([float(sum(1 << i for i in f)) for f in fixeds + [fixeds[i] for i in pad]])
    per_lane = probe.gmr_probe_rowfma_out_per_lane()
    assert per_lane == 44
    folded, plain = np.empty((12, NV, per_lane)), np.empty((12, NV, per_lane))
    rc = probe.gmr_probe_rowfma_elim(C.c_int(12), _p(A), _p(rhs), _p(masks), _p(folded), _p(plain))
    assert rc == 0, f"gmr_probe_rowfma_elim: HIP error {rc}"
    return mats, rhss, fixeds, folded, plain


def test_elimination_both_ways_bit_equal(eliminations):
    mats, rhss, fixeds, folded, plain = eliminations
    assert not np.isnan(folded).any() and not np.isnan(plain).any()
    assert np.array_equal(_u64(folded), _u64(plain))
    # the padding cases ran in other 16-lane rows of the wavefront than their originals (rows 2, 3 against 0, 1)
    assert np.array_equal(_u64(folded[10:]), _u64(folded[:2]))


@pytest.mark.parametrize("case", range(10))
def test_elimination_matches_host_mirror(eliminations, case):
    mats, rhss, fixeds, folded, plain = eliminations
    nl, nt, kind, seed = CASES_79[case]
    o = folded[case]                                   # [lane][44]
    full = tsm.eliminate(mats[case], nl, nt, fixeds[case], full=True)
    cols, own = o[:, :16], o[:, 16:32]
    L_l = [[cols[m, a] if m > a else 0.0 for a in range(NL)] for m in range(NL)]
    Y_l = [[cols[NL + u, a] for a in range(NL)] for u in range(NT)]
    L_t = [[cols[NL + q, NL + t] if q > t else 0.0 for t in range(NT)] for q in range(NT)]
    ltl = [[own[a, m] if m > a else 0.0 for a in range(NL)] for m in range(NL)]
    yl = [[own[a, NL + u] for a in range(NL)] for u in range(NT)]
    lt = [[own[NL + t, NL + q] if q > t else 0.0 for t in range(NT)] for q in range(NT)]
    for name, got in (("L_l", L_l), ("Y_l", Y_l), ("L_t", L_t), ("ltl", ltl), ("yl", yl), ("lt", lt)):
        assert np.array_equal(tsm.bits(got), tsm.bits(full[name])), (kind, seed, name)
    mirror = _mirror_solve(mats[case], rhss[case], fixeds[case])
    assert np.array_equal(tsm.bits(o[NL:, 32:41]), tsm.bits(mirror["schur"])), (kind, seed, "Schur part")
    assert np.array_equal(tsm.bits(o[:, 41]), tsm.bits(mirror["y"])), (kind, seed, "substituted right-hand side")
    assert np.array_equal(tsm.bits(o[NL:, 42]), tsm.bits(mirror["yt"][NL:])), (kind, seed, "trunk right-hand side")
    assert np.array_equal(tsm.bits(o[:, 43]), tsm.bits(mirror["x"])), (kind, seed, "solution")
    assert np.abs(np.asarray(mirror["x"])).max() > 0.0


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def test_div_const_on_the_device(probe):
    assert probe.gmr_probe_div_const_literals() == len(dc.LITERALS)
    x = np.ascontiguousarray(np.stack([dc.midpoint_numerators(c) for c in dc.LITERALS]))
    n = x.shape[1]
    helper, quotient = np.empty_like(x), np.empty_like(x)
    rc = probe.gmr_probe_div_const(C.c_int(n), _p(x), _p(helper), _p(quotient))
    assert rc == 0, f"gmr_probe_div_const: HIP error {rc}"
    for i, c in enumerate(dc.LITERALS):
        bad = np.nonzero(_u64(helper[i]) != _u64(quotient[i]))[0]
        assert bad.size == 0, (c, bad.size, [float.hex(float(x[i, j])) for j in bad[:4]])
        assert np.array_equal(_u64(quotient[i]), _u64(x[i] / c)), c
