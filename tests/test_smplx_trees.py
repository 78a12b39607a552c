"""The SMPL-X ingest kernels (csrc/gmr_smplx.hip) off the SMPL-X tree: every accepted skeleton of tests/ingest_trees.py through
SmplxHandle.joints, the three alignment entry points, the fused frames call and the ragged batch, against the CPU oracle
(oracle.smplx_joints, oracle.smplx_align), which walks joint by joint through parents[] with no program and no slots.
tests/test_ingest_prog_host.py checks that oracle against the definition, proves the programs' slot indices in bounds and
asserts which paths this list reaches (nslot 1, 2, 3, >= 5; LDS above 48 KB; the refusals).  Arithmetic is pinned elsewhere
(g_smplx.npz); this is about the walk programs and the edges of the data layouts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_trees as it  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-12
ULP32 = 2.4e-7           # the project's bound of the joints kernel: one float32 ulp at max(1, |ref|.max())


@pytest.fixture(scope="module")
def lib():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


_REF = {}


def _reference(oracle, e, N):
    """inputs and the oracle's joints of (tree, N), computed once and shared (read-only)"""
    key = (e["name"], N)
    if key not in _REF:
        j_rest, pose, transl = it.smplx_inputs(e, N)
        ref = oracle.smplx_joints(e["parent"], j_rest, pose, transl)
        for a in (j_rest, pose, transl, ref):
            a.setflags(write=False)
        _REF[key] = (j_rest, pose, transl, ref)
    return _REF[key]


def _ids(entries):
    return [e["name"] for e in entries]


@pytest.mark.parametrize("e", it.smplx_trees(), ids=_ids(it.smplx_trees()))
def test_joints_against_the_oracle(lib, oracle, e):
    """SmplxHandle.joints (rows_planes_kernel either side of smplx_joints_kernel, C = 3 J from 3 to 192) within one float32 ulp of
    the oracle; the rest offsets keep |ref| below 4.  J = 64 asks rows_planes_kernel for a 49 408-byte tile."""
    h = lib.SmplxHandle(e["parent"])
    for N in it.FRAME_COUNTS:
        j_rest, pose, transl, ref = _reference(oracle, e, N)
        got = h.joints(j_rest, pose, transl)
        big = float(np.abs(ref).max())
        err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        print(f"{e['name']} N={N}: |ref| {big:.3f} err {err:.3e} bound {ULP32 * max(1.0, big):.3e}")
        assert got.shape == ref.shape and np.isfinite(got).all() and big < 4.0
        assert err <= ULP32 * max(1.0, big), (e["name"], N, err)
    h.close()


def _align_three_ways(lib, h, pose, jts, tt):
    """align (host gather + compact kernel), align_dev (full rows, jstride = J + 3), align_compact_dev"""
    N, J = pose.shape[:2]
    nout = N if tt is None else len(tt)
    a = h.align(pose, jts, tt)
    pj, rj = h.compact_layout()
    d = [lib.DeviceBuffer.from_host(x) for x in (pose, jts, np.ascontiguousarray(pose[:, pj].transpose(1, 2, 0)),
                                                np.ascontiguousarray(jts[:, rj].transpose(1, 2, 0)))]
    d_tt = None if tt is None else lib.DeviceBuffer.from_host(np.ascontiguousarray(tt, dtype=np.float64))
    o1, o2 = lib.DeviceBuffer(nout * h.rows * 56), lib.DeviceBuffer(nout * h.rows * 56)
    h.align_dev(N, jts.shape[1], d[0], d[1], nout, d_tt, o1)
    h.align_compact_dev(N, d[2], d[3], nout, d_tt, o2)
    return a, o1.to_host((nout, h.rows, 7), np.float64), o2.to_host((nout, h.rows, 7), np.float64)


@pytest.mark.parametrize("e", it.smplx_trees(), ids=_ids(it.smplx_trees()))
def test_alignment_against_the_oracle(lib, oracle, e):
    """the all-joints handle and the catalogue selection, with and without target times: the three entry points agree bit for
    bit and lie within 1e-12 of the oracle; without target times the positions are the float32 joints, exactly"""
    par = e["parent"]
    J = len(par)
    worst = 0.0
    for sel in (None, e["sel"]):
        h = lib.SmplxHandle(par, sel)
        for N in it.FRAME_COUNTS:
            _, pose, _, ref_j = _reference(oracle, e, N)
            rng = np.random.default_rng([N, J])
            jts = np.concatenate([ref_j, rng.normal(size=(N, 3, 3)).astype(np.float32)], axis=1)     # jstride = J + 3
            for tt in it.target_times(N):
                a, b, c = _align_three_ways(lib, h, pose, jts, tt)
                assert np.array_equal(a, b) and np.array_equal(a, c), (e["name"], N, None if tt is None else len(tt))
                ref = oracle.smplx_align(par, pose, jts, tt, sel)
                err = float(np.abs(a - ref).max())
                worst = max(worst, err)
                assert a.shape == ref.shape and err <= TOL, (e["name"], sel is not None, N, None if tt is None else len(tt), err)
                if tt is None:
                    rows = list(range(J)) if sel is None else sel
                    assert np.array_equal(a[..., :3], jts[:, rows].astype(np.float64))
        h.close()
    print(f"{e['name']}: worst |align - oracle| {worst:.3e}")


def _cpu_frames(oracle, par, j_rest, pose, transl, tt, sel):
    """the composition on the CPU: the oracle's joints (float32) into the oracle's alignment"""
    return oracle.smplx_align(par, pose, oracle.smplx_joints(par, j_rest, pose, transl), tt, sel)


def _close_frames(got, ref, what):
    """orientations within 1e-12; positions within one float32 ulp of the joint magnitude (a joint may round differently; the
    interpolation is a convex combination of two float32 joints, so it moves by no more than they do)"""
    assert got.shape == ref.shape, what
    if got.size == 0:
        return
    assert np.abs(got[..., 3:] - ref[..., 3:]).max() <= TOL, (what, np.abs(got[..., 3:] - ref[..., 3:]).max())
    bound = ULP32 * max(1.0, float(np.abs(ref[..., :3]).max()))
    assert np.abs(got[..., :3] - ref[..., :3]).max() <= bound, (what, np.abs(got[..., :3] - ref[..., :3]).max(), bound)


@pytest.mark.parametrize("e", it.smplx_trees(), ids=_ids(it.smplx_trees()))
def test_fused_frames_against_the_cpu_composition(lib, oracle, e):
    """gmr_smplx_frames against oracle.smplx_joints -> float32 -> oracle.smplx_align, evaluated on the CPU alone: no other HIP
    path stands between the fused call and its reference"""
    par = e["parent"]
    h = lib.SmplxHandle(par, e["sel"])
    for N in it.FRAME_COUNTS:
        j_rest, pose, transl, _ = _reference(oracle, e, N)
        for tt in it.target_times(N):
            got = h.frames(j_rest, pose, transl, tt)
            _close_frames(got, _cpu_frames(oracle, par, j_rest, pose, transl, tt, e["sel"]), (e["name"], N, None if tt is None else len(tt)))
    h.close()


BATCH_LENS = (1, 2, 2, 3, 63, 64, 65, 130, 0, 7, 129, 64)
BATCH_ALIGN = (0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 0, 1)
BATCH_NOUT = (1, 1, 2, 0, 63, 16, 65, 32, 0, 1, 129, 64)


@pytest.mark.parametrize("e", it.batch_trees(), ids=_ids(it.batch_trees()))
def test_ragged_batch_against_the_cpu_composition(lib, oracle, e):
    """batch_frames on 22-joint trees (batch_nslot 1 .. 4 and 9 LDS slots in front of the pose tile): 12 clips, mixed align flags,
    nout of 0, 1 and N, a different j_rest per clip, against the CPU composition per clip; zeros beyond nout"""
    par, sel = e["parent"], e["sel"]
    assert len(par) == 22
    h = lib.SmplxHandle(par, sel)
    assert h.batch_takes
    clips = []
    for c, N in enumerate(BATCH_LENS):
        j_rest, pose, transl = it.smplx_inputs(e, max(N, 1), seed=100 + c)
        clips.append((j_rest * (1.0 + 0.05 * c), pose[:N], transl[:N]))
    seg = np.concatenate([[0], np.cumsum(BATCH_LENS)]).astype(np.int32)
    pose_all = np.concatenate([p for _, p, _ in clips])
    T = max(BATCH_NOUT) + 3
    out = h.batch_frames(pose_all[:, 0], pose_all[:, 1:].reshape(-1, 63), np.concatenate([t for _, _, t in clips]), seg, BATCH_NOUT, BATCH_ALIGN,
                         np.stack([j for j, _, _ in clips]), T=T)
    assert out.shape == (len(BATCH_LENS), T, len(sel), 7)
    for c, (N, al, nout) in enumerate(zip(BATCH_LENS, BATCH_ALIGN, BATCH_NOUT)):
        assert not out[c, nout:].any(), c
        if nout == 0:
            continue
        j_rest, pose, transl = clips[c]
        tt = np.linspace(0, N - 1, nout) if al else None
        _close_frames(out[c, :nout], _cpu_frames(oracle, par, j_rest, pose, transl, tt, sel), (e["name"], c))
    h.close()


def test_refusals_are_error_returns_and_the_process_goes_on(lib, oracle):
    by = it.BY_NAME
    with pytest.raises(lib.GmrHipError, match="tree too deep"):
        lib.SmplxHandle(by["caterpillar28"]["parent"])
    with pytest.raises(lib.GmrHipError, match="1 <= J <= 64"):
        lib.SmplxHandle(by["chain65"]["parent"])
    with pytest.raises(lib.GmrHipError, match="duplicate"):
        lib.SmplxHandle(by["binary63"]["parent"], [5, 9, 5])
    e = by["binary63"]
    h = lib.SmplxHandle(e["parent"], [3, 22, 1])          # joint 22 lies outside root_orient + pose_body
    assert not h.batch_takes
    with pytest.raises(lib.GmrHipError, match="beyond the body joints"):
        h.batch_frames(np.zeros((2, 3)), np.zeros((2, 63)), np.zeros((2, 3)), [0, 2], [2], [0], np.zeros((1, 63, 3)))
    # ... and the same process makes a correct call
    j_rest, pose, transl, ref = _reference(oracle, e, 65)
    got = lib.SmplxHandle(e["parent"]).joints(j_rest, pose, transl)
    assert np.abs(got.astype(np.float64) - ref).max() <= ULP32 * max(1.0, float(np.abs(ref).max()))
