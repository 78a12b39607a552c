"""The latency kernel's split evaluation after a solve (csrc/gmr_ik.hip: helper 1 walks the tree, the main wavefront walks
the rotations alone and evaluates what needs no position).

Host part: the input grids cross every switch of the split functions (checked on the inputs themselves, in NumPy).
GPU part, through tests/hip/split_eval_probe.hip (built by build.build_split_probe()):
  * the two halves of se3_log_rel5 (se3_log_rel5_rot, se3_log_rel5_pos) against the original, bit for bit;
  * the rotation walk against the full walk's xa[3..6], bit for bit, and the full walk against the oracle's FK, on G1 and on
    a robot of the <8, 10> class (another depth, another number of jumping rounds).
"""
import ctypes as C

import numpy as np
import pytest

from test_ik_bound_path import _Synthetic


def _quat(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * axis])


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def grid():
    """pose[n, 14] = (pb, qb, pt, qt) and, per row, the relative rotation q = conj(qb) qt it was built from.  (The t2 = 1e-10
    crossing is the identity switch of the Jl^-1 coefficients, which read the residual this grid checks.)

    Relative angles: 0 and a few 1e-6 (n2 = sin^2(angle / 2) on both sides of 1e-10, so t2 = angle^2 on both sides of 1e-10
    as well: 2e-5 / 2.1e-5 give n2 = 1.0e-10 / 1.1e-10, and 9e-6 / 1.1e-5 give t2 = 0.81e-10 / 1.21e-10), 0.09 / 0.11
    (t2 = 0.0081 / 0.0121: both sides of 1e-2), mid-range angles, and pi -+ 1e-10 / 1e-11 / 0 (|q.w| on both sides of 1e-10,
    q.w of either sign); every angle with both signs of q (q and -q are the same rotation: q.w < 0)."""
    rng = np.random.default_rng(19)
    angles = [0.0, 9e-6, 1.1e-5, 1.9e-5, 2.0e-5, 2.1e-5, 1e-3, 0.09, 0.0999, 0.1001, 0.11, 0.5, 1.5, 3.0,
              np.pi - 1e-9, np.pi - 1e-10, np.pi - 1e-11, np.pi, np.pi + 1e-11, np.pi + 1e-9, 4.0]
    rows, rel = [], []
    for ang in angles:
        for sign in (1.0, -1.0):
            for _ in range(6):
                qb = rng.normal(size=4)
                qb /= np.linalg.norm(qb)
                q = sign * _quat(rng.normal(size=3), ang)
                qt = _qmul(qb, q)
                rows.append(np.concatenate([rng.normal(0, 0.5, 3), qb, rng.normal(0, 0.5, 3), qt]))
                rel.append(q)
    # exact cases: the computed q is the built one (qb = identity), so the switches are hit as intended
    for q in ([1.0, 0, 0, 0], [-1.0, 0, 0, 0], [0.0, 1, 0, 0], [5e-11, 0, 1, 0], [-5e-11, 0, 0, 1], [2e-10, 0, 1, 0], [-2e-10, 1, 0, 0]):
        q = np.array(q)
        rows.append(np.concatenate([rng.normal(0, 0.5, 3), [1, 0, 0, 0], rng.normal(0, 0.5, 3), q]))
        rel.append(q)
    return np.array(rows), np.array(rel)


def test_grid_crosses_every_switch():
    pose, q = grid()
    n2 = (q[:, 1:] ** 2).sum(axis=1)
    big = n2 >= 1e-10
    assert (n2 < 1e-10).sum() >= 10 and big.sum() >= 10
    assert (big & (np.abs(q[:, 0]) < 1e-10)).sum() >= 4, "the |q.w| < 1e-10 branch"
    assert (big & (q[:, 0] < -1e-3)).sum() >= 10 and (big & (q[:, 0] > 1e-3)).sum() >= 10, "both signs of q.w"
    assert ((q[:, 0] == 0.0) & big).any() and ((q[:, 0] < 0) & (np.abs(q[:, 0]) < 1e-10)).any()
    # t2 = |log q|^2: angle^2 of the rotation in [0, pi]
    ang = 2.0 * np.arctan2(np.sqrt(n2), np.abs(q[:, 0]))
    t2 = ang * ang
    for lo, hi in ((0.0, 1e-10), (1e-10, 1e-2), (1e-2, 10.0)):
        assert ((t2 >= lo) & (t2 < hi)).sum() >= 10, (lo, hi)
    # close to the switches on both sides
    assert ((t2 > 0.5e-10) & (t2 < 1e-10)).any() and ((t2 >= 1e-10) & (t2 < 2e-10)).any()
    assert ((t2 > 0.9e-2) & (t2 < 1e-2)).any() and ((t2 >= 1e-2) & (t2 < 1.1e-2)).any()


@pytest.fixture(scope="module")
def probe():
    """a GPU host without the probe is a failure, not a skip"""
    from general_motion_retargeting_amd import _lib, build
    _lib.require_gpu()
    try:
        path = build.build_split_probe()
    except Exception as exc:   # noqa: BLE001
        pytest.fail(f"the split-evaluation probe is missing and could not be built: {exc}")
    return C.CDLL(path)


@pytest.mark.gpu
def test_split_residual_is_the_original_bit_for_bit(probe):
    pose, _ = grid()
    pose = np.ascontiguousarray(pose)
    n = len(pose)
    ref, split = np.empty((n, 11)), np.empty((n, 11))
    rc = probe.gmr_probe_split_eval(C.c_int(n), *[a.ctypes.data_as(C.c_void_p) for a in (pose, ref, split)])
    assert rc == 0, f"gmr_probe_split_eval: HIP error {rc}"
    assert np.isfinite(ref).all()
    series = ref[:, 9] == 0.0          # aux[3] = t is only set above the series switch
    print(f"{n} poses, {int(series.sum())} below the series switch of a")
    assert series.sum() >= 10 and (~series).sum() >= 10
    for name, sl in (("e", slice(0, 6)), ("aux", slice(6, 11))):
        a, b = ref[:, sl].copy().view(np.uint64), split[:, sl].copy().view(np.uint64)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{name}: {len(bad)} values differ, first at row {bad[0][0]} column {bad[0][1]}"


def _walk_inputs(model, max_hops):
    nb = len(model.parent)
    parent = np.asarray(model.parent)
    depth = np.zeros(nb, dtype=np.int64)
    chain = []
    for b in range(nb):
        path, a = [], b
        while a >= 0:
            path.append(a)
            a = parent[a]
        chain.append(path[::-1])           # root .. b
        depth[b] = len(path) - 1
    nhop = 0
    while (1 << nhop) < depth.max() + 1:
        nhop += 1
    assert nhop <= max_hops
    tree = np.zeros((2 + max_hops, nb), dtype=np.int32)
    tree[0] = depth
    tree[1] = model.body_hinge
    for r in range(nhop):
        for b in range(nb):
            tree[2 + r, b] = chain[b][depth[b] - (1 << r)] if depth[b] >= (1 << r) else 0
    local = np.zeros((nb, 10))
    local[:, 0:4] = model.body_quat
    local[:, 4:7] = model.body_pos
    for b in range(nb):
        if model.body_hinge[b] >= 0:
            local[b, 7:10] = model.hinge_axis[model.body_hinge[b]]
    return nb, nhop, np.ascontiguousarray(tree), np.ascontiguousarray(local), int(depth.max())


@pytest.fixture(scope="module")
def wide_trunk(tmp_path_factory):
    return _Synthetic(tmp_path_factory.mktemp("robot"))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["g1", "wide_trunk"])
def test_rotation_walk_is_the_full_walk(probe, oracle, g1, wide_trunk, which):
    su = g1 if which == "g1" else wide_trunk
    model = su.model
    max_hops = probe.gmr_probe_max_hops()
    nb, nhop, tree, local, maxd = _walk_inputs(model, max_hops)
    nh = len(model.hinge_body)
    rng = np.random.default_rng(7)
    for trial in range(3):
        q = np.zeros(7 + nh)
        q[:3] = rng.normal(0, 1.0, 3)
        b = rng.normal(size=4)
        q[3:7] = b / np.linalg.norm(b)
        q[7:] = rng.uniform(-2.5, 2.5, nh)
        xa, rot = np.empty((nb, 7)), np.empty((nb, 4))
        rc = probe.gmr_probe_walks(C.c_int(nb), C.c_int(nh), C.c_int(nhop), *[a.ctypes.data_as(C.c_void_p) for a in (q, tree, local, xa, rot)])
        assert rc == 0, f"gmr_probe_walks: HIP error {rc}"
        assert np.array_equal(xa[:, 3:].copy().view(np.uint64), rot.view(np.uint64)), f"{which}: the two walks' rotations differ"
        xpos, xquat = oracle.fk(su.mb, q)
        # the same product of at most depth + 1 unit quaternions (and sum of rotated offsets below 2 m), associated in
        # another order: every composition rounds a dozen times at 2^-53, so depth x 12 x 1.1e-16 x 2 < 1e-13 for depth <= 32
        dq, dp = np.abs(xa[:, 3:] - xquat).max(), np.abs(xa[:, :3] - xpos).max()
        print(f"{which} trial {trial}: nb {nb}, depth {maxd}, rounds {nhop}: max |dquat| = {dq:.2e}, max |dpos| = {dp:.2e}")
        assert dq <= 1e-13 and dp <= 1e-13 * max(1.0, np.abs(xpos).max()), (dq, dp)
