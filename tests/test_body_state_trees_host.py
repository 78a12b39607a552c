"""Per-body state on the synthetic trees of tests/fk_trees.py, host side: which trees ``gmr_motion_body_state`` takes and which it
must refuse (its LDS budget, computed from the layout of csrc/gmr_body_state.hip), the libraries, queries and selections the GPU
tests (tests/test_body_state_trees.py) walk them with, the generated trees being exactly what they were before ``make_tree`` was
split, and the float32 walk's own distance from the float64 walk, which is what the device's velocities are bounded by.  No GPU."""
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_state_mirror as bm  # noqa: E402
import fk_trees as ft  # noqa: E402
import motion_cases as mc  # noqa: E402
import motion_mirror as mm  # noqa: E402
from test_motion_library import queries  # noqa: E402

F = np.float32
LENS = (1, 2, 0, 65, 3)               # a one-frame clip, an empty clip in the middle, a clip longer than a block of queries
FPS = (30.0, 50.0, 120.0, 29.97, 50.0)
NQ = 130                              # answered queries: three blocks of 64, the last with two
SIZES = (1, 63, 64, 65)               # calls whose last block is full, one short of it, and one beyond
REFUSED = ("comb-0", "comb-1", "comb-5", "binary-0", "binary-1", "random-0", "random-1", "random-2", "random-3", "deep-0", "deep-1", "deep-4",
           "deep-5", "deep-6")
SELECTION_TREES = ("star-0", "broom-0", "brooms2-1", "humanoid-3", "deep-3", "chain24-0", "small5-1", "comb8-0", "binary15-0")

TREES = {t["name"]: t for t in ft.gpu_trees() + ft.small_family_trees()}
FITTING = tuple(n for n in TREES if n not in REFUSED)

# The largest deviation of the FLOAT32 WALK of tests/body_state_mirror.py (one rounding per operation, the kernel's order of terms,
# libm's sine and cosine) from the float64 walk of the same sampled state, over the 28 fitting trees with ``tree_motions`` and
# ``tree_queries``, body_vel and body_ang_vel, in units of max(1, |row|_inf) of the float64 row: measured on the CPU by
# test_the_float32_walk_stays_within_what_was_measured (the largest is broom-0's: a trunk of 15 and a fan of 46), never from the device.  The device may deviate from
# the float64 walk of its own sampled state by twice that (its own sine and cosine: another draw of the same rounding noise, the rule
# of fk_trees.bound) plus one float32 spacing at the row's magnitude.  VEL_TOL of tests/test_motion_body_state.py stays what it is for
# the robots.
VEL_F32_DEV = 9.106244228306679e-06


def vel_bound(scale):
    """``scale``: max(1, |row|_inf) of the float64 rows -> what a component of the device's row may be off"""
    return 2.0 * VEL_F32_DEV * scale + np.spacing(scale.astype(F)).astype(np.float64)


def tree_motions(tree):
    """float64 clips of LENS frames for a world-mode library with the tree's dofs"""
    ndof = int((tree["dof_dim"] > 0).sum())
    rng = np.random.default_rng([53, len(tree["parent"]), ndof])
    return [{"fps": FPS[c], "root_pos": rng.normal(0, 0.5, size=(n, 3)) + np.array([0.3, -0.2, 0.8]), "root_rot": mc.quat_track(rng, n),
             "dof_pos": rng.uniform(-1.2, 1.2, size=(n, ndof)), "local_body_pos": None} for c, n in enumerate(LENS)]


def tree_queries(tree):
    """(clip i32, time f64, expected status): NQ queries of ``test_motion_library.queries`` over the clips that have frames (times
    before 0, on frame times, past the end) and, spread among them, a clip id at and below the range, the empty clip and a NaN time"""
    rng = np.random.default_rng([59, len(tree["parent"])])
    live = np.array([c for c, n in enumerate(LENS) if n > 0])
    shim = SimpleNamespace(fps=np.array(FPS)[live], seg=np.concatenate([[0], np.cumsum(np.array(LENS)[live])]))
    clip, time = queries(rng, shim, NQ)
    clip, time = live[clip].astype(np.int32), time.copy()
    bad = [(len(LENS), 0.1), (-1, 0.1), (LENS.index(0), 0.0), (3, np.nan)]
    at = [5, 63, 64, 101]
    for k, (c, t) in zip(at, bad):
        clip, time = np.insert(clip, k, c).astype(np.int32), np.insert(time, k, t)
    status = np.zeros(len(clip), dtype=np.int32)
    status[at] = 1
    return clip, time, status


def selections(tree):
    """the selections of the GPU test: all leaves; the deepest leaf (its closure is one chain, shorter than the tree); every other
    body; the reverse order; five bodies in descending order (runs of one); six consecutive bodies (a full run of four and one of
    two; five on a tree of five); body 0 alone"""
    par = tree["parent"]
    nb = len(par)
    leaves = [b for b in range(nb) if b not in set(par.tolist())]
    deepest = int(np.argmax(ft.depth_of(par)))
    start = max(0, nb // 2 - 3)
    return {"leaves": leaves, "deepest": [deepest], "every_other": list(range(0, nb, 2)), "reverse": list(range(nb - 1, -1, -1)),
            "descending5": [int(b) for b in np.linspace(nb - 1, 0, 5).astype(int)], "consecutive6": list(range(start, min(start + 6, nb))),
            "root": [0]}


def sampled_state(tree, loop=True):
    """the mirror's sampled state of the answered queries: what the walk is measured on where there is no device"""
    lib = mm.Library(tree_motions(tree))
    clip, time, status = tree_queries(tree)
    out = lib.sample(clip, time, loop)
    assert np.array_equal(out["status"], status)
    ok = status == 0
    return [out[k][ok] for k in ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel")]


def velocity_deviation(tree, state, got_v, got_w, bodies=None):
    """(largest |got - float64 walk| / max(1, |row|_inf), all within ``vel_bound``) for body_vel / body_ang_vel rows ``got_*``
    [N, nsel, 3] of ``state`` (the six sampled arrays)"""
    _, _, v, w = bm.walk(bm.tree_of_dict(tree), *state)
    sel = slice(None) if bodies is None else list(bodies)
    worst, inside = 0.0, True
    for got, want in ((got_v, v[:, sel]), (got_w, w[:, sel])):
        scale = np.maximum(1.0, np.abs(want).max(axis=2, keepdims=True))
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        worst = max(worst, float((err / scale).max()))
        inside &= bool((err <= vel_bound(scale)).all())
    return worst, inside


def test_the_generated_trees_are_what_they_were():
    """``make_tree`` was split so that a tree can be built from a given parent list: the listed trees and the sweep are the same bytes"""
    h = hashlib.sha256()
    for t in ft.gpu_trees() + list(ft.sweep(84, 3)):
        h.update(t["name"].encode())
        for k in ("parent", "local_translation", "local_rotation", "dof_idx", "dof_dim", "axis"):
            a = np.ascontiguousarray(t[k])
            h.update(str(a.dtype).encode())
            h.update(a.tobytes())
    assert h.hexdigest() == "b9988d1c36ab605509be6869be084fa874c2bc7027ea2157807cca1da409abfe"
    comb, binary = ft.small_family_trees()
    assert (comb["name"], comb["family"], len(comb["parent"])) == ("comb8-0", "comb", 17) and comb["parent"].tolist() == ft._comb(8)
    assert (binary["name"], binary["family"], len(binary["parent"])) == ("binary15-0", "binary", 15) and binary["parent"].tolist() == ft._binary(15)
    for t in (comb, binary):
        assert ft.body_state_lds(t)[2] < 48 * 1024 and ft.depth_of(t["parent"]).max() + 1 <= ft.MAX_DEPTH
        assert np.array_equal(np.sort(t["dof_idx"][t["dof_idx"] >= 0]), np.arange(int((t["dof_dim"] > 0).sum())))


def test_the_lds_budget_refuses_exactly_fourteen_of_the_listed_trees():
    listed = [t["name"] for t in ft.gpu_trees()]
    assert len(listed) == 40 and len(TREES) == 42
    refused = [n for n in listed if ft.body_state_lds(TREES[n])[2] > ft.BODY_STATE_LDS_LIMIT]
    assert tuple(refused) == REFUSED and len(FITTING) == 28
    need = [ft.body_state_lds(TREES[n])[2] for n in listed if n not in REFUSED]
    assert (min(need), max(need)) == (18944, 61952)
    assert {TREES[n]["family"] for n in FITTING} == set(ft.FAMILIES)          # no family is left to the refusals alone
    ndofs = {int((TREES[n]["dof_dim"] > 0).sum()) for n in FITTING}
    assert {0, 63} <= ndofs                                                   # single-0 and star-0
    assert set(SELECTION_TREES) <= set(FITTING)


def test_the_queries_and_selections_are_what_they_claim():
    for name in FITTING:
        tree = TREES[name]
        clip, time, status = tree_queries(tree)
        assert len(clip) == NQ + 4 and status.sum() == 4 and clip.dtype == np.int32
        good = status == 0
        assert set(clip[good].tolist()) == {0, 1, 3, 4} and np.isfinite(time[good]).all() and (time[good] < 0).any()
        assert sorted(clip[~good].tolist()) == [-1, 2, 3, 5] and np.isnan(time[~good]).sum() == 1
    for name in SELECTION_TREES:
        tree = TREES[name]
        nb, par = len(tree["parent"]), tree["parent"]
        sel = selections(tree)
        assert len(sel) == 7 and all(len(set(s)) == len(s) and 0 <= min(s) and max(s) < nb for s in sel.values())
        assert all(b not in par.tolist() for b in sel["leaves"]) and sel["descending5"] == sorted(sel["descending5"], reverse=True)
        closure = set()
        b = sel["deepest"][0]
        while b >= 0:
            closure.add(b)
            b = int(par[b])
        assert len(closure) == ft.depth_of(par).max() + 1 and (len(closure) < nb or name == "chain24-0")
        assert sel["consecutive6"] == list(range(sel["consecutive6"][0], sel["consecutive6"][0] + min(6, nb)))


def test_the_float32_walk_stays_within_what_was_measured():
    worst = {}
    for name in FITTING:
        tree = TREES[name]
        state = sampled_state(tree)
        _, _, v, w = bm.walk(bm.tree_of_dict(tree), *state, dtype=np.float32)
        assert v.dtype == np.float32 and w.dtype == np.float32
        _, _, v64, w64 = bm.walk(bm.tree_of_dict(tree), *state)
        worst[name] = max(float((np.abs(a - b) / np.maximum(1.0, np.abs(b).max(axis=2, keepdims=True))).max()) for a, b in ((v, v64), (w, w64)))
        print(f"{name:12s} float32 walk: velocities at most {worst[name]:.3e} max(1, |row|) from the float64 walk")
    top = max(worst, key=worst.get)
    print(f"largest: {top} {worst[top]!r} (measured {VEL_F32_DEV!r})")
    assert worst[top] <= VEL_F32_DEV
    assert worst["single-0"] == 0.0                                            # a single body is a copy of the root


@pytest.mark.parametrize("name", ["small5-1", "humanoid-3", "comb8-0"])
def test_the_float32_walk_gives_the_pose_of_the_float64_walk_and_of_fk_f64(name):
    """the two walks of the mirror and the FK tests' float64 walk are three writings of one recursion"""
    tree = TREES[name]
    state = sampled_state(tree, loop=False)
    p, q, _, _ = bm.walk(bm.tree_of_dict(tree), *state)
    pos, rot = ft.fk_f64(tree, state[0], state[1], state[4])
    assert np.abs(p - pos).max() <= 1e-12 and np.abs(q - rot).max() <= 1e-12
    p32, q32, _, _ = bm.walk(bm.tree_of_dict(tree), *state, dtype=np.float32)
    assert np.abs(p32 - pos).max() <= 5e-6 and np.abs(q32 - rot).max() <= 5e-6
