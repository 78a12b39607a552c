"""Per-body state on a real MI355X (csrc/gmr_body_state.hip) on the synthetic trees of tests/fk_trees.py: stars, combs, brooms,
chains of depth 24, permuted dof indices, bodies without a hinge, general and negative axes, un-normalised local rotations --
everything the kernel adds to the FK walk (velocity propagation, the general-axis branch, parked parents of 13 floats, the
ancestor-closure plan with runs of at most four, the LDS budget) on trees no robot has.  The 26 listed trees that fit the budget and
a comb and a binary tree small enough to fit are walked; the 14 that do not fit are refused, by both entry points, with the numbers
of the layout in the message.  tests/test_body_state_trees_host.py holds the cases, the split and the measured constant of the
velocity bound.  Each test makes one pass over 134 queries."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_trees as ft  # noqa: E402
from test_body_state_trees_host import (FITTING, REFUSED, SELECTION_TREES, SIZES, TREES, VEL_F32_DEV, selections, tree_motions,  # noqa: E402
                                        tree_queries, velocity_deviation)
from test_motion_library import _bits, device_library  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
STATE = ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel")
BODY = {"body_pos": 3, "body_rot": 4, "body_vel": 3, "body_ang_vel": 3}
GUARD = 64                            # sentinel rows behind every output


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def sentinels(hip, rows, widths):
    """{name: (device buffer, its initial host image)} of ``rows`` + GUARD rows, float32 -7.25 (status: int32 -7)"""
    out = {}
    for k, w in widths.items():
        a = np.full((rows + GUARD, max(w, 1)), -7, dtype=np.int32) if k == "status" else np.full((rows + GUARD, max(w, 1)), -7.25, dtype=F)
        out[k] = (hip.DeviceBuffer.from_host(a), a)
    return out


def widths_of(ndof, nsel):
    return {"root_pos": 3, "root_rot": 4, "root_vel": 3, "root_ang_vel": 3, "dof_pos": ndof, "dof_vel": ndof,
            **{k: nsel * w for k, w in BODY.items()}, "status": 1}


def read_back(bufs, N, widths):
    """{name: (rows [:N] in the output's own width, True when nothing else of the buffer changed)}"""
    res = {}
    for k, (b, init) in bufs.items():
        a = b.to_host(init.shape, init.dtype)
        w = widths[k]
        flat, flat0 = a.reshape(-1), init.reshape(-1)
        res[k] = (flat[:N * w].reshape(N, w), bool(np.array_equal(flat[N * w:], flat0[N * w:])))
    return res


@pytest.mark.parametrize("name", FITTING)
def test_body_state_on_a_synthetic_tree(hip, oracle, name):
    tree = TREES[name]
    fk = hip.FkHandle(tree)
    loop = FITTING.index(name) % 2 == 0
    lib = device_library(hip, tree_motions(tree))            # world mode; NaN rows behind row B of every input
    assert lib.ndof == fk.ndof
    clip, time, status = tree_queries(tree)
    got = lib.body_state(clip, time, kinematics=fk, loop=loop)
    ref = lib.sample(clip, time, loop)
    assert np.array_equal(got["status"], status) and np.array_equal(ref["status"], status)
    for k in STATE:                                           # the sampler's bits, NaN rows included
        assert same_bits(got[k], ref[k]), k
    ok, bad = status == 0, status == 1
    for k in STATE + tuple(BODY):
        assert np.isnan(got[k][bad]).all() and np.isfinite(got[k][ok]).all(), k
    # the pose: the bits of the FK kernel on the sampled state (DESIGN.md section 6j claims this for any tree) ...
    rp, rq, dof = ref["root_pos"][ok], ref["root_rot"][ok], ref["dof_pos"][ok]
    bp, br, _ = fk.fk(rp, rq, dof)
    assert same_bits(got["body_pos"][ok], bp) and same_bits(got["body_rot"][ok], br)
    # ... and within the FK tests' bound of the float64 walk: twice the error of the reference's own float32 operation order
    pos, rot = ft.fk_f64(tree, rp, rq, dof)
    obp, obr = oracle.fk_f32(tree, rp, rq, dof)
    e_pos, e_rot = float(np.abs(obp - pos).max()), float(np.abs(obr - rot).max())
    d_pos, d_rot = float(np.abs(got["body_pos"][ok] - pos).max()), float(np.abs(got["body_rot"][ok] - rot).max())
    # the velocities: against the float64 walk of the device's own sampled state
    state = [got[k][ok] for k in STATE]
    worst, inside = velocity_deviation(tree, state, got["body_vel"][ok], got["body_ang_vel"][ok])
    print(f"\n{name:12s} loop={loop}: pos e_ref {e_pos:.2e} kernel {d_pos:.2e}  rot e_ref {e_rot:.2e} kernel {d_rot:.2e}  "
          f"velocities {worst:.3e} max(1, |row|) (float32 walk at most {VEL_F32_DEV:.3e})")
    assert d_pos <= ft.bound(e_pos, pos) and d_rot <= ft.bound(e_rot, rot)
    assert inside, worst
    for k, r in (("body_pos", "root_pos"), ("body_rot", "root_rot"), ("body_vel", "root_vel"), ("body_ang_vel", "root_ang_vel")):
        assert same_bits(got[k][:, 0], got[r]), k             # body 0 is the root
    # calls of 1, 63, 64 and 65 queries on the device: the rows of the full call, nothing behind row N
    widths = widths_of(fk.ndof, fk.nbody)
    d_clip, d_time = hip.DeviceBuffer.from_host(clip), hip.DeviceBuffer.from_host(time)
    for N in SIZES:
        bufs = sentinels(hip, N, widths)
        lib.body_state_dev(N, d_clip, d_time, kinematics=fk, loop=loop, **{k: b for k, (b, _) in bufs.items()})
        hip.check(hip.lib().gmr_stream_sync(None))
        for k, (rows, untouched) in read_back(bufs, N, widths).items():
            assert untouched, (k, N)
            assert same_bits(rows, got[k][:N].reshape(N, -1)), (k, N)
    fk.close()


@pytest.mark.parametrize("name", SELECTION_TREES)
def test_selections_give_the_rows_of_the_full_call(hip, name):
    tree = TREES[name]
    fk = hip.FkHandle(tree)
    lib = device_library(hip, tree_motions(tree))
    clip, time, status = tree_queries(tree)
    N = len(clip)
    full = lib.body_state(clip, time, kinematics=fk)
    d_clip, d_time = hip.DeviceBuffer.from_host(clip), hip.DeviceBuffer.from_host(time)
    for i, (what, sel) in enumerate(selections(tree).items()):
        widths = {**{k: len(sel) * w for k, w in BODY.items()}, "status": 1}
        asked = list(widths) if i % 2 == 0 else ["body_pos", "body_ang_vel"]       # every other selection leaves outputs out
        bufs = sentinels(hip, N, widths)
        lib.body_state_dev(N, d_clip, d_time, kinematics=fk, bodies=sel, **{k: bufs[k][0] for k in asked})
        hip.check(hip.lib().gmr_stream_sync(None))
        for k, (rows, untouched) in read_back(bufs, N, widths).items():
            if k not in asked:                                # an output not asked for: the sentinels, all of them
                b, init = bufs[k]
                assert np.array_equal(b.to_host(init.shape, init.dtype), init), (what, k)
                continue
            assert untouched, (what, k)
            want = full[k] if k == "status" else full[k][:, sel]
            assert same_bits(rows, want.reshape(N, -1)), (what, k)
        sub = lib.body_state(clip, time, kinematics=fk, bodies=sel, state=False)      # the host-pointer twin
        for k in BODY:
            assert same_bits(sub[k], full[k][:, sel]), (what, k)
    fk.close()


def test_trees_beyond_the_lds_budget_are_refused_by_both_entry_points(hip):
    """the 14 listed trees whose parked parents and dof rows need more than 64 KiB: an error that names the dof count, the slot
    count and the bytes of the layout, outputs untouched, and the same library answers for a tree that fits right after"""
    L = hip.lib()
    for name in REFUSED:
        tree = TREES[name]
        ndof, nslot, nbytes = ft.body_state_lds(tree)
        assert nbytes > ft.BODY_STATE_LDS_LIMIT
        message = f"a tree of {ndof} dofs and {nslot} parked bodies needs {nbytes} bytes of LDS per workgroup"
        fk = hip.FkHandle(tree)
        lib = device_library(hip, tree_motions(tree))
        clip, time, status = tree_queries(tree)
        N = len(clip)
        widths = widths_of(ndof, fk.nbody)
        # the device-pointer entry point
        bufs = sentinels(hip, N, widths)
        d_clip, d_time = hip.DeviceBuffer.from_host(clip), hip.DeviceBuffer.from_host(time)
        with pytest.raises(hip.GmrHipError, match=re.escape(message)):
            lib.body_state_dev(N, d_clip, d_time, kinematics=fk, **{k: b for k, (b, _) in bufs.items()})
        hip.check(L.gmr_stream_sync(None))
        for k, (b, init) in bufs.items():
            assert np.array_equal(b.to_host(init.shape, init.dtype), init), (name, k)
        # the host-pointer entry point, into host arrays that carry the same sentinels
        host = {k: (np.full((N, max(w, 1)), -7, dtype=np.int32) if k == "status" else np.full((N, max(w, 1)), -7.25, dtype=F))
                for k, w in widths.items()}
        table = hip.BodyStateOut(**{k: a.ctypes.data for k, a in host.items()})
        rc = L.gmr_motion_body_state(lib.handle, fk.handle, N, hip._ptr(clip), hip._ptr(time), 1, None, 0, C.byref(table))
        assert rc != 0 and message in L.gmr_last_error().decode(), (name, L.gmr_last_error())
        for k, a in host.items():
            assert (a == (-7 if k == "status" else F(-7.25))).all(), (name, k)
        with pytest.raises(hip.GmrHipError, match="bytes of LDS per workgroup"):
            lib.body_state(clip, time, kinematics=fk)
        # a tree of the same dof count that fits (a star: one parked parent), same library, right after
        star = ft.tree_from_parents(ft._star(ndof + 1), "star", 0, name=f"star{ndof + 1}")
        assert ft.body_state_lds(star)[0] == ndof and ft.body_state_lds(star)[2] <= ft.BODY_STATE_LDS_LIMIT
        fits = hip.FkHandle(star)
        got = lib.body_state(clip, time, kinematics=fits)
        assert np.array_equal(got["status"], status) and np.isfinite(got["body_vel"][status == 0]).all()
        ref = lib.sample(clip, time)
        bp, br, _ = fits.fk(ref["root_pos"][status == 0], ref["root_rot"][status == 0], ref["dof_pos"][status == 0])
        assert same_bits(got["body_pos"][status == 0], bp) and same_bits(got["body_rot"][status == 0], br)
        fits.close()
        fk.close()
