"""The hazard-complete solver statements of csrc/gmr_device_math.h (row_bcast_fnma_pivot, row_backsub_fill,
row_dot_backsub): a pivot, a back substitution as ONE statement whose DPP sources get their wait states from instructions
of the same statement (tests/hip/filled_probe.hip, built by build.build_filled_probe()).

  CPU: the probe and csrc/gmr_ik.hip compile for gfx950 (the assembler checks every operand of the statements).
  -m gpu (a) every statement, at every (lane, count) the solver issues it with, against the composition of primitives it
         replaces (row_bcast_fnma_bcast, row_bcast_fnma_cols, row_bcast_fma, row_bcast_fma_dot, plain * ) on 64 lanes of
         random doubles with +0 and -0 among them: equal bits in all four 16-lane rows.  A DPP source read too early is
         a stale register: random operands make it a wrong bit.
  -m gpu (b) one whole local elimination and solve of the <7, 9> shape written with the new statements and with the
         per-step forms, on the ten <7, 9> cases of tests/test_ik_tree_symmetric.py: factor, Y_l, Schur part, substituted
         right-hand sides and solution bit-equal to each other, the factors to tree_sym_mirror.eliminate(.., full=True),
         the rest to the host mirror of tests/test_row_bcast_fma.py.

One wavefront and one launch for (a) and for (b).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tree_sym_mirror as tsm
from conftest import ROOT
from test_ik_tree_symmetric import CASES, FIXED
from test_row_bcast_fma import _mirror_solve

NL, NT, NV = 7, 9, 16
CASES_79 = [c for c in CASES if c[:2] == (NL, NT)]
assert len(CASES_79) == 10


def test_probe_and_kernel_compile_for_gfx950(tmp_path):
    from general_motion_retargeting_amd import build
    csrc = os.path.join(ROOT, "general_motion_retargeting_amd", "csrc")
    for src in (build.FILLED_PROBE_SRC, os.path.join(csrc, "gmr_ik.hip")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        out = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-c", src, "-o", obj], cwd=csrc,
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-4000:]
        assert os.path.getsize(obj) > 0


@pytest.fixture(scope="module")
def probe():
    """a GPU host without the probe is a failure, not a skip"""
    from general_motion_retargeting_amd import _lib, build
    _lib.require_gpu()
    try:
        path = build.build_filled_probe()
    except Exception as exc:   # noqa: BLE001
        pytest.fail(f"the probe of the filled statements is missing and could not be built: {exc}")
    return C.CDLL(path)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- (a) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_statements_match_the_primitives_they_replace(probe):
    n_in, n_out = probe.gmr_probe_filled_in_rows(), probe.gmr_probe_filled_out_rows()
    assert (n_in, n_out) == (39, 14 * 17 + 17 + 1)
    rng = np.random.default_rng(11)
    x = rng.normal(size=(n_in, 64)) * 10.0 ** rng.integers(-3, 4, size=(n_in, 64))
    for row in range(n_in):                              # +0 and -0 in every operand, in different lanes and rows of lanes
        x[row, rng.choice(64, size=3, replace=False)] = 0.0
        x[row, rng.choice(64, size=2, replace=False)] = -0.0
    x = np.ascontiguousarray(x)
    filled, composed = np.empty((n_out, 64)), np.empty((n_out, 64))
    rc = probe.gmr_probe_filled_stmt(_p(x), _p(filled), _p(composed))
    assert rc == 0, f"gmr_probe_filled_stmt: HIP error {rc}"
    assert not np.isnan(filled).any() and not np.isnan(composed).any()
    bad = np.nonzero((_u64(filled) != _u64(composed)).any(axis=1))[0]
    assert bad.size == 0, f"output rows that differ (17 per pivot, then f[16], acc, acc): {bad.tolist()}"
    # the inputs do what they are there for: results differ from row to row of lanes, and zeros of both signs occur
    piv = filled[:17]
    assert not np.array_equal(piv[:, :16], piv[:, 16:32]) and (filled == 0.0).any() and np.signbit(filled[filled == 0.0]).any()
    # the broadcast diagonal of the first pivot is the updated r[1] of lane 1 of each row, exactly rounded
    r1, l = x[1], x[16]
    for row in range(4):
        src = 16 * row + 1
        want = tsm.fma(-l[src], l[src], r1[src])
        assert _u64(np.array([want]))[0] == _u64(filled[16, 16 * row:16 * row + 16]).min() == _u64(filled[16, 16 * row:16 * row + 16]).max()


# ---- (b) ---------------------------------------------------------------------------------------------------------------
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
    per_lane = probe.gmr_probe_filled_out_per_lane()
    assert per_lane == 44
    filled, stepwise = np.empty((12, NV, per_lane)), np.empty((12, NV, per_lane))
    rc = probe.gmr_probe_filled_elim(C.c_int(12), _p(A), _p(rhs), _p(masks), _p(filled), _p(stepwise))
    assert rc == 0, f"gmr_probe_filled_elim: HIP error {rc}"
    return mats, rhss, fixeds, filled, stepwise


@pytest.mark.gpu
def test_elimination_both_ways_bit_equal(eliminations):
    mats, rhss, fixeds, filled, stepwise = eliminations
    assert not np.isnan(filled).any() and not np.isnan(stepwise).any()
    assert np.array_equal(_u64(filled), _u64(stepwise))
    # the padding cases ran in other 16-lane rows of the wavefront than their originals (rows 2, 3 against 0, 1)
    assert np.array_equal(_u64(filled[10:]), _u64(filled[:2]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(10))
def test_elimination_matches_host_mirror(eliminations, case):
    mats, rhss, fixeds, filled, stepwise = eliminations
    nl, nt, kind, seed = CASES_79[case]
    o = filled[case]                                   # [lane][44]
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
