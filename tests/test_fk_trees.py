"""-m gpu: the float32 FK kernels (csrc/gmr_fk.hip) on the synthetic trees of tests/fk_trees.py -- every launch path
(fk_split_kernel with 2, 3 and 4 wavefronts, with and without the shared trunk; the staged one-wavefront kernel; the direct
kernel, which runs when a destination is off a 16-byte boundary), against a float64 walk written from the definition, bit
for bit against each other, with sentinels around every destination, plus the refusals of gmr_fk_create and the second
consumer of the handle (MotionLibrary.body_state).  tests/test_fk_trees_host.py checks on the CPU that the plan of each of
these trees executes the same number of barriers in every wavefront; no tree is launched that fails there.

The bound against the float64 walk is not fixed in advance: per tree, e_ref = max |oracle.fk_f32 - float64 walk| over the
frames of all five batches the tree is walked with (the error of the reference's own float32 operation order), and the kernel
may deviate by 2 e_ref plus one float32 spacing at the largest output magnitude of the batch.  (e_ref of ONE frame is a single
draw of the rounding noise: for the lone frame of B = 1 of brooms2-1 the oracle is 1.8e-7 from the walk in rotation, the kernel
4.9e-7, with another sin / cos and so another draw; over the tree's 323 frames both are alike, see the table.)

Measured on the MI355X (per family: the tree with the largest e_ref, the kernel's error at B = 130 as a ratio to it; the bound
allows 2 and a spacing.  A single body is a copy of the root: both errors are zero):

    family     e_ref pos  ratio   e_ref rot  ratio
    single     0.00e+00   -       0.00e+00   -
    small2     1.16e-07   0.94    1.30e-07   0.78
    small3     2.15e-07   1.00    1.96e-07   0.92
    small5     2.71e-07   1.00    2.30e-07   0.73
    small7     3.21e-07   1.35    2.70e-07   1.00
    chain24    9.79e-07   0.84    6.52e-07   0.79
    star       1.43e-07   1.00    1.85e-07   0.81
    comb       1.03e-06   1.00    6.08e-07   0.90
    binary     5.65e-07   1.00    3.37e-07   0.95
    broom      1.05e-06   0.73    5.77e-07   0.92
    brooms2    1.22e-06   0.75    5.70e-07   0.98
    humanoid   6.10e-07   0.95    3.70e-07   0.79
    random     5.37e-07   0.85    3.15e-07   0.98
    deep       1.09e-06   0.70    6.17e-07   0.73
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_state_mirror as bm  # noqa: E402
import fk_trees as ft  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = (1, 63, 64, 65, 130)
SENTINEL = 0xA5
GUARD = 256              # bytes of sentinel in front of and behind a destination


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def trees():
    return ft.gpu_trees()


_ref_cache = {}


def reference(tree, B):
    """inputs, the float64 walk and the float32 oracle's distance from it -- computed once per (tree, B), never modified"""
    key = (tree["name"], B)
    if key not in _ref_cache:
        from oracle import oracle as orc
        orc.build()
        rp, rq, dof = ft.make_inputs(tree, B)
        pos, rot = ft.fk_f64(tree, rp, rq, dof)
        obp, obr = orc.fk_f32(tree, rp, rq, dof)
        val = (rp, rq, dof, pos, rot, float(np.abs(obp - pos).max()), float(np.abs(obr - rot).max()))
        for a in val[:5]:
            a.setflags(write=False)
        _ref_cache[key] = val
    return _ref_cache[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_every_tree_against_the_float64_walk(hip, oracle, trees):
    worst = {}
    for tree in trees:
        fk = hip.FkHandle(tree)
        # e_ref of the tree: over all the frames it is walked with here (one frame alone is a single draw of the rounding noise)
        e_pos, e_rot = (max(reference(tree, B)[k] for B in SIZES) for k in (5, 6))
        for B in SIZES:
            rp, rq, dof, pos, rot = reference(tree, B)[:5]
            bp, br, mz = fk.fk(rp, rq, dof, want_min_z=True)
            d_pos, d_rot = float(np.abs(bp - pos).max()), float(np.abs(br - rot).max())
            print(f"{tree['name']:12s} B={B:3d} pos: e_ref {e_pos:.2e} kernel {d_pos:.2e}   rot: e_ref {e_rot:.2e} kernel {d_rot:.2e}")
            if B == SIZES[-1]:
                w = worst.setdefault(tree["family"], [0.0, 0.0, 0.0, 0.0])
                if e_pos >= w[0]: w[0], w[1] = e_pos, d_pos
                if e_rot >= w[2]: w[2], w[3] = e_rot, d_rot
            assert d_pos <= ft.bound(e_pos, pos), (tree["name"], B, d_pos, e_pos)
            assert d_rot <= ft.bound(e_rot, rot), (tree["name"], B, d_rot, e_rot)
            assert mz == bp[..., 2].min(), (tree["name"], B)
        fk.close()
    print("TABLE family, e_ref pos, ratio, e_ref rot, ratio")
    for fam, (ep, dp, er, dr) in worst.items():
        print(f"TABLE {fam:9s} {ep:.2e} {dp / ep if ep else 0.0:5.2f}   {er:.2e} {dr / er if er else 0.0:5.2f}")


def test_every_launch_path_gives_the_bits_of_one_wavefront(hip, trees, monkeypatch):
    """GMR_FK_WAVES = 1..4 and GMR_FK_NO_SHARE (read by gmr_fk_create): positions, rotations, positions alone and min_z, bit for
    bit; GMR_FK_NO_SPECIAL: the same values up to the sign of an exact zero"""
    B = SIZES[-1]
    for tree in trees:
        rp, rq, dof = reference(tree, B)[:3]
        monkeypatch.delenv("GMR_FK_NO_SHARE", raising=False)
        monkeypatch.delenv("GMR_FK_NO_SPECIAL", raising=False)
        monkeypatch.setenv("GMR_FK_WAVES", "1")
        one = hip.FkHandle(tree)
        bp1, br1, mz1 = one.fk(rp, rq, dof, want_min_z=True)
        assert mz1 == bp1[..., 2].min()
        for waves, no_share in (("2", False), ("3", False), ("4", False), ("4", True)):
            monkeypatch.setenv("GMR_FK_WAVES", waves)
            if no_share:
                monkeypatch.setenv("GMR_FK_NO_SHARE", "1")
            fk = hip.FkHandle(tree)
            bp, br, mz = fk.fk(rp, rq, dof, want_min_z=True)
            assert same_bits(bp, bp1) and same_bits(br, br1) and mz == mz1, (tree["name"], waves, no_share)
            bp_only, none, mz = fk.fk(rp, rq, dof, want_rot=False, want_min_z=True)
            assert none is None and same_bits(bp_only, bp1) and mz == mz1, (tree["name"], waves, no_share)
            fk.close()
        monkeypatch.delenv("GMR_FK_NO_SHARE")
        monkeypatch.delenv("GMR_FK_WAVES")
        monkeypatch.setenv("GMR_FK_NO_SPECIAL", "1")
        generic = hip.FkHandle(tree)
        monkeypatch.delenv("GMR_FK_NO_SPECIAL")
        for x, y in zip(generic.fk(rp, rq, dof)[:2], (bp1, br1)):
            assert np.array_equal(x, y), tree["name"]
            assert not ((bits(x) != bits(y)) & (x != 0)).any(), tree["name"]
        generic.close()
        one.close()


class Dest:
    """a destination of ``nbytes`` at ``off`` bytes from a 16-byte boundary, sentinel bytes all around it"""

    def __init__(self, hip, nbytes, off):
        self.hip, self.nbytes, self.start = hip, nbytes, GUARD + off
        self.init = np.full(GUARD + off + nbytes + GUARD, SENTINEL, dtype=np.uint8)
        self.buf = hip.DeviceBuffer.from_host(self.init)
        assert self.buf.ptr.value % 16 == 0
        self.ptr = C.c_void_p(self.buf.ptr.value + self.start)

    def result(self, shape):
        a = self.buf.to_host(self.init.shape, np.uint8)
        inside = a[self.start:self.start + self.nbytes]
        assert (a[:self.start] == SENTINEL).all() and (a[self.start + self.nbytes:] == SENTINEL).all(), "bytes outside the destination were written"
        return inside.copy().view(F).reshape(shape)


def run_dev(hip, fk, d_in, B, off_pos=0, off_rot=0, want_rot=True, want_min=False):
    nb = fk.nbody
    pos = Dest(hip, B * nb * 12, off_pos)
    rot = Dest(hip, B * nb * 16, off_rot) if want_rot else None
    mz = Dest(hip, 4, 0) if want_min else None
    fk.fk_dev(B, *d_in, pos.ptr, rot.ptr if rot else None, mz.ptr if mz else None)
    hip.check(hip.lib().gmr_stream_sync(None))
    return pos.result((B, nb, 3)), rot.result((B, nb, 4)) if rot else None, mz.result((1,))[0] if mz else None


def test_direct_variant_and_nothing_written_outside(hip, trees):
    """``fk_dev`` into destinations 4, 8 and 12 bytes off a 16-byte boundary (positions alone, rotations alone, both) takes
    fk_batch_kernel<false>: the bits of the aligned call, positions alone and with min_z too, and in every call -- the aligned ones
    at all five batch sizes included -- not a byte outside the destination changes.  Trees of 1, 2, 3, 5 and 7 bodies: a block's
    float count is no multiple of 4, the flush ends in its scalar tail."""
    pick = [t for t in trees if len(t["parent"]) < 8] + [t for t in trees if len(t["parent"]) >= 8][::2]
    assert {len(t["parent"]) for t in pick} >= {1, 2, 3, 5, 7}
    for tree in pick:
        fk = hip.FkHandle(tree)
        for B in SIZES:
            rp, rq, dof = reference(tree, B)[:3]
            want_p, want_r, want_mz = fk.fk(rp, rq, dof, want_min_z=True)
            d_in = [hip.DeviceBuffer.from_host(a if a.size else np.zeros(1, F)) for a in (rp, rq, dof)]
            for want_rot in (True, False):
                p, r, mz = run_dev(hip, fk, d_in, B, want_rot=want_rot, want_min=True)
                assert same_bits(p, want_p) and (r is None or same_bits(r, want_r)) and mz == want_mz, (tree["name"], B, "aligned")
            for off in (4, 8, 12) if B in (1, 65, 130) else (4,):
                for off_pos, off_rot in ((off, 0), (0, off), (off, off)):
                    p, r, mz = run_dev(hip, fk, d_in, B, off_pos, off_rot, want_min=(off == 8))
                    assert same_bits(p, want_p) and same_bits(r, want_r) and (mz is None or mz == want_mz), (tree["name"], B, off_pos, off_rot)
                p, r, mz = run_dev(hip, fk, d_in, B, off, 0, want_rot=False, want_min=(off != 8))
                assert same_bits(p, want_p) and (mz is None or mz == want_mz), (tree["name"], B, off, "positions alone")
        fk.close()


def test_qpos_source_into_a_misaligned_destination(hip, trees):
    """``postprocess_clips_dev`` makes no alignment check on ``d_local_body_pos``: a misaligned one is accepted and sends the identity-root
    pass (FkSrcQpos<false>) through the direct variant.  The world pass (FkSrcQpos<true>) writes to the call's own scratch, which is
    always aligned: its direct instantiation cannot be reached through the ABI.  Bits of the aligned call, of the float32 entry
    point on the same angles, and no byte outside."""
    for tree in [t for t in trees if len(t["parent"]) in (1, 3, 7)] + [t for t in trees if len(t["parent"]) >= 8][1::5]:
        fk = hip.FkHandle(tree)
        nb, nd = fk.nbody, fk.ndof
        for B in (1, 65, 130):
            rp, rq, dof = reference(tree, B)[:3]
            q = np.concatenate([rp, rq[:, [3, 0, 1, 2]], dof], axis=1).astype(np.float64)[None]        # [1, B, 7 + ndof], wxyz
            d_q, d_seg = hip.DeviceBuffer.from_host(q), hip.DeviceBuffer.from_host(np.array([0, B], np.int32))
            want_local, _, _ = fk.fk(np.zeros((B, 3), F), np.tile(np.array([0, 0, 0, 1], F), (B, 1)), dof, want_rot=False)
            _, _, want_low = fk.fk(rp, rq, dof, want_rot=False, want_min_z=True)
            for off in (0, 4, 8, 12):
                outs = [hip.DeviceBuffer(B * n) for n in (24, 32, max(nd, 1) * 8)]
                local, low = Dest(hip, B * nb * 12, off), Dest(hip, 4, 0)
                fk.postprocess_clips_dev([(1, B, d_q, None)], d_seg, 1, B, *outs, local.ptr, low.ptr)
                hip.check(hip.lib().gmr_stream_sync(None))
                assert same_bits(local.result((B, nb, 3)), want_local), (tree["name"], B, off)
                assert low.result((1,))[0] == want_low, (tree["name"], B, off)
        fk.close()


def test_gmr_fk_create_refusals(hip):
    L = hip.lib()

    def create(tree, ndof=None, nbody=None):
        arrays = [np.ascontiguousarray(tree[k], dtype=d) for k, d in (("parent", np.int32), ("local_translation", F), ("local_rotation", F),
                                                                      ("dof_idx", np.int32), ("axis", np.float64))]
        h = C.c_void_p()
        rc = L.gmr_fk_create(len(tree["parent"]) if nbody is None else nbody, *[hip._ptr(a) for a in arrays],
                             int((tree["dof_dim"] > 0).sum()) if ndof is None else ndof, C.byref(h))
        msg = L.gmr_last_error().decode()
        if rc == 0:
            L.gmr_fk_destroy(h)
        return rc, msg

    def tree_of(parent):
        t = ft.make_tree("star", 0)
        n = len(parent)
        t = {k: (v[:n].copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}
        t["parent"] = np.array(parent, np.int32)
        return t
    good = tree_of([-1, 0, 1, 1])
    assert create(good)[0] == 0
    for rc, msg, word in (create(good, nbody=0) + ("nbody",), create(ft.make_tree("star", 0), nbody=65) + ("nbody",),
                          create(tree_of([-1] + list(range(24)))) + ("deep",), create(tree_of([0, 0, 1])) + ("root",),
                          create(tree_of([-1, 0, 2, 1])) + ("parent[2]",), create(tree_of([-1, 0, 3, 1])) + ("parent[2]",),
                          create(good, ndof=2) + ("dof_idx",), create(good, ndof=100) + ("ndof",), create(good, ndof=65) + ("ndof",)):
        assert rc != 0 and word in msg, (rc, msg, word)
    assert create(tree_of([-1] + list(range(23))))[0] == 0          # depth exactly 24
    star = ft.make_tree("star", 0)
    assert create(star, ndof=64)[0] == 0                            # ndof = FK_MAX_BODIES itself is in range


def body_state_lds(tree):
    """csrc/gmr_body_state.hip: body_state_lds (64 queries per workgroup, 13 floats per parked parent, runs of 4 staged bodies)"""
    par = tree["parent"]
    parked = {int(par[b]) for b in range(1, len(par)) if par[b] != b - 1}          # a child that does not follow its parent immediately
    ndof, nslot = int((tree["dof_dim"] > 0).sum()), max(1, len(parked))
    return 4 * (64 * ((2 * ndof) | 1) + nslot * 13 * 64 + 64 * (3 * 13 + 17) + 4 * 64)


def test_the_motion_library_walks_the_same_trees(hip, trees):
    """``MotionLibrary.body_state`` on a synthetic handle, all bodies and a random selection: positions and rotations are the FK
    kernel's bits on the sampled state, velocities follow the float64 mirror at the tolerance of tests/test_motion_body_state.py;
    a tree whose parked parents do not fit 64 KB of LDS (comb, binary) is refused with the documented message, not launched."""
    from test_motion_body_state import STATE, VEL_TOL
    from test_motion_library import device_library, make_motions, queries
    import motion_mirror as mm
    names = ("comb-0", "binary-0", "random-1", "small3-0", "small7-4", "chain24-0", "star-0", "broom-0", "brooms2-1", "humanoid-2", "humanoid-3",
             "random-4", "deep-3")
    pick = [t for t in trees if t["name"] in names]
    assert len(pick) == len(names)
    refused = walked = 0
    for tree in pick:
        rng = np.random.default_rng(len(tree["parent"]))
        fk = hip.FkHandle(tree)
        motions = make_motions(rng, [40, 3, 90], fk.ndof, 0)
        lib = device_library(hip, motions)
        clip, time = queries(rng, mm.Library(motions), 130)
        if body_state_lds(tree) > 64 * 1024:
            with pytest.raises(hip.GmrHipError, match="bytes of LDS per workgroup"):
                lib.body_state(clip, time, kinematics=fk)
            refused += 1
            continue
        full = lib.body_state(clip, time, kinematics=fk)
        assert not full["status"].any()
        bp, br, _ = fk.fk(full["root_pos"], full["root_rot"], full["dof_pos"])
        assert same_bits(full["body_pos"], bp) and same_bits(full["body_rot"], br), tree["name"]
        axis = tree["axis"] / np.maximum(np.linalg.norm(tree["axis"], axis=1, keepdims=True), 1e-9)
        mt = {"parent": tree["parent"].astype(np.int64), "t": tree["local_translation"].astype(np.float64), "r": tree["local_rotation"].astype(np.float64),
              "axis": axis, "dof_idx": tree["dof_idx"].astype(np.int64)}
        st = {k: full[k].astype(np.float64) for k in STATE}
        _, _, v, w = bm.walk(mt, st["root_pos"], st["root_rot"], st["root_vel"], st["root_ang_vel"], st["dof_pos"], st["dof_vel"])
        for k, want in (("body_vel", v), ("body_ang_vel", w)):
            scale = np.maximum(1.0, np.abs(want).max(axis=2, keepdims=True))
            assert (np.abs(full[k] - want) / scale).max() <= VEL_TOL, (tree["name"], k)
        sel = [int(x) for x in rng.permutation(fk.nbody)[:max(1, fk.nbody // 3)]]
        sub = lib.body_state(clip, time, kinematics=fk, bodies=sel, state=False)
        for k in ("body_pos", "body_rot", "body_vel", "body_ang_vel"):
            assert same_bits(sub[k], full[k][:, sel]), (tree["name"], k)
        walked += 1
        fk.close()
    assert refused >= 2 and walked >= 8, (refused, walked)
