"""The tracker anchors on a real MI355X (csrc/gmr_tracker_anchor.hip and the anchored paths of the step, link step and preview kernels
through motion_tracker.py): a tracker without anchors is the tracker it was; anchored rows are the float32
statement of tests/anchor_mirror.py applied to the same tracker's unanchored rows, bit for bit; anchored terms against the float64
formulas on the device's own anchored rows; ``anchor_to_root`` against the mirror from the sampler's rows; the device entry points on a
stream of their own; continuity across a redraw by composition; the preview's sim frame.  N = 37 environments (no multiple of 16 or 64)
on four clips of 1, 2, 33 and 70 frames; every test makes one pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchor_mirror as am  # noqa: E402
import links_mirror as lm  # noqa: E402
import preview_mirror as pm  # noqa: E402
import tracker_mirror as tm  # noqa: E402
from test_motion_body_state_host import kinematics  # noqa: E402
from test_motion_library import _bits, device_library  # noqa: E402
from test_motion_tracker import STATE, random_sim, tracker  # noqa: E402
from test_tracker_links import assert_close_to_mirror, random_links  # noqa: E402
from test_tracker_preview import BOUND, walking_motions, within  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
N = 37
DT = 0.02
ROOT_ROWS = ("ref_root_pos", "ref_root_rot", "ref_root_vel", "ref_root_ang_vel")
BODY_ROWS = ("ref_body_pos", "ref_body_rot", "ref_body_vel", "ref_body_ang_vel")
LINK_OUT = ("link_err", "link_term", "max_dist", "fail")
OFFSETS = np.array([0.04, -0.06, 0.0], dtype=F)
PREVIEW_BODIES = [4, 0, 2]


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def world(hip):
    """the robot, six of its bodies in an order that is not the tree's, and the library of four clips (built once, never written)"""
    km = kinematics("booster_t1")
    rng = np.random.default_rng(1700)
    sel = rng.permutation(len(km.body_names))[:6].tolist()
    assert sel != sorted(sel)
    motions = walking_motions(rng, [1, 2, 33, 70], km.num_dof, 5)
    for m, fps in zip(motions, (30.0, 50.0, 120.0, 29.97)):
        m["fps"] = fps
    return {"km": km, "sel": sel, "lib": device_library(hip, motions)}


def clocks(rng, lib, near_end=()):
    """a clip and a clock inside it per environment; the environments of ``near_end`` sit one step before the end of clip 3 or 2"""
    clip = rng.integers(0, 4, size=N).astype(np.int32)
    length = np.array([1 / 30.0, 2 / 50.0, 33 / 120.0, 70 / 29.97])
    time = (rng.uniform(0.0, 0.7, size=N) * length[clip]).astype(F)
    for i, e in enumerate(near_end):
        clip[e] = 3 if i % 2 else 2
        time[e] = F(length[clip[e]] - 0.5 * DT)
    return clip, time


def random_anchors(rng, n=N):
    return rng.uniform(-10, 10, (n, 3)).astype(F), rng.uniform(-np.pi, np.pi, n).astype(F)


def mirror_rows(anchor, out, rows=ROOT_ROWS):
    """tests/anchor_mirror.py applied to the four rows of an unanchored step (root or body rows)"""
    p, y = anchor["pos"], anchor["yaw_zw"]
    return {rows[0]: am.apply_pos(p, y, out[rows[0]]), rows[1]: am.apply_quat(y, out[rows[1]]), rows[2]: am.apply_vec(y, out[rows[2]]),
            rows[3]: am.apply_vec(y, out[rows[3]])}


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(_bits(a), _bits(b)) if a.dtype == F else np.array_equal(a, b), what


def bound_of(root_xy, anchor_pos):
    """1e-6 x max(1, |x| + |y| + |t|): six roundings of 2^-24 on operands of that size, doubled"""
    return 1e-6 * np.maximum(1.0, np.abs(root_xy).sum(axis=1) + np.abs(anchor_pos).sum(axis=1))


def heading_gap(qa, qb):
    d = am.heading(qa) - am.heading(qb)
    return np.abs((d + np.pi) % (2 * np.pi) - np.pi)


# ---- 1. nothing moves without anchors ---------------------------------------------------------------------------------------------
def test_a_tracker_without_anchors_and_one_at_the_identity_are_the_tracker_it_was(hip, world):
    km, sel, lib = world["km"], world["sel"], world["lib"]
    rng = np.random.default_rng(1)
    clip, time = clocks(rng, lib, near_end=(3, 20, 36))
    never, identity, off = (tracker(lib, N, DT, loop=False, seed=5) for _ in range(3))
    identity.enable_anchors()
    off.enable_anchors()
    off.set_anchor(*random_anchors(rng))
    off.enable_anchors(False)
    assert never.anchor_state() is None and off.anchor_state() is None
    st = identity.anchor_state()
    assert np.array_equal(st["pos"], np.zeros((N, 3), F)) and np.array_equal(_bits(st["yaw_zw"]), _bits(np.tile(F([0, 1]), (N, 1))))
    trio = (never, identity, off)
    for t in trio:
        assert t.assign(clip, time) == 0
    sim = links = None
    finished = 0
    for step in range(5):
        got = []
        for t in trio:
            out = {}
            for frame in ("raw", "reference", "sim"):
                t.set_preview(OFFSETS, pm.BLOCKS, frame, PREVIEW_BODIES)
                if frame != "sim" or sim is not None:
                    out.update({f"preview_{frame}_{k}": v for k, v in t.preview(sim).items()})
            for frame in ("world", "heading"):
                t.set_links(km, bodies=sel, frame=frame)
                t.set_link_terms(fail_dist=0.3)
                if frame == "world" or sim is not None:
                    out.update({f"links_{frame}_{k}": v for k, v in t.step_links(sim, links, advance=False).items()})
            if sim is None:
                ref = {k: out[f"links_world_{k}"] for k in ROOT_ROWS + BODY_ROWS + ("ref_dof_pos", "ref_dof_vel")}
            out.update({f"step_{k}": v for k, v in t.step(sim).items()})
            out.update({f"state_{k}": v for k, v in t.state().items() if k in STATE})
            got.append(out)
        if sim is None:
            sim, links = random_sim(rng, ref), random_links(rng, ref)
        finished += int(got[0]["step_finished"].sum())
        assert set(got[0]) == set(got[1]) == set(got[2])
        for k in got[0]:
            assert not np.isnan(got[0][k]).any(), k
            assert np.array_equal(got[0][k], got[1][k]), (step, k)
            same(got[0][k], got[2][k], (step, k))
    assert finished >= 3 and any(k.startswith("links_heading_link_err") for k in got[0])


# ---- 2. rows ----------------------------------------------------------------------------------------------------------------------
def test_anchored_rows_are_the_float32_mirror_of_the_unanchored_rows(hip, world):
    km, sel, lib = world["km"], world["sel"], world["lib"]
    rng = np.random.default_rng(2)
    clip, time = clocks(rng, lib, near_end=(8,))
    clip[30] = 4                                     # a bad assignment: NaN rows with and without an anchor
    ok = clip < 4
    plain, moved = tracker(lib, N, DT, loop=False, seed=9), tracker(lib, N, DT, loop=False, seed=9)
    pos, yaw = random_anchors(rng)
    assert moved.set_anchor(pos, yaw) == 0
    anchor = moved.anchor_state()
    same(anchor["pos"], pos, "anchor_pos")
    same(anchor["yaw_zw"], am.half_angle(yaw), "anchor_yaw: the host's half angle is the mirror's")
    lay = None
    for t in (plain, moved):
        assert t.assign(clip, time) == 0
        t.set_links(km, bodies=sel, frame="world")
        lay = t.set_preview(OFFSETS, pm.BLOCKS, "raw", PREVIEW_BODIES)
    finished = np.zeros(N, np.int32)
    for step in range(2):
        pv, pw = plain.preview(), moved.preview()
        lp, lw = plain.step_links(advance=False), moved.step_links(advance=False)
        sp, sw = plain.step(), moved.step()
        for got, base in ((lw, lp), (sw, sp)):
            want = mirror_rows(anchor, base)
            for k in ROOT_ROWS:
                same(got[k][ok], want[k][ok], (step, k))
                assert np.isnan(got[k][~ok]).all(), k
            for k in ("ref_dof_pos", "ref_dof_vel", "status", "finished"):
                same(got[k], base[k], (step, k))
        finished |= sw["finished"]
        want = mirror_rows(anchor, lp, BODY_ROWS)
        for k in BODY_ROWS:
            same(lw[k][ok], want[k][ok], (step, k))
            assert np.isnan(lw[k][~ok]).all(), k
        # the preview: K = 3 offsets, one of them negative
        raw = {b: pv["obs"][:, :, lay[b]] for b in pm.BLOCKS}
        want = {"root_pos": am.apply_pos(anchor["pos"], anchor["yaw_zw"], raw["root_pos"]), "root_quat": am.apply_quat(anchor["yaw_zw"], raw["root_quat"]),
                "root_vel": am.apply_vec(anchor["yaw_zw"], raw["root_vel"]), "root_ang_vel": am.apply_vec(anchor["yaw_zw"], raw["root_ang_vel"])}
        want["root_rot6"] = am.rot6(want["root_quat"])
        for b in pm.BLOCKS:
            same(pw["obs"][:, :, lay[b]][ok], want.get(b, raw[b])[ok], (step, "preview", b))
        assert np.isnan(pw["obs"][~ok]).all()
        same(pw["valid"], pv["valid"], "valid")
        same(pw["status"], pv["status"], "status")
        a, b = plain.state(), moved.state()
        for k in STATE:
            same(a[k], b[k], (step, k))
    assert finished[8] == 1 and sw["status"][30] == 1
    after = moved.anchor_state()          # a redraw leaves the anchor as it is
    same(after["pos"], anchor["pos"], "anchor_pos after a redraw")
    same(after["yaw_zw"], anchor["yaw_zw"], "anchor_yaw after a redraw")


# ---- 3. terms ---------------------------------------------------------------------------------------------------------------------
def test_anchored_terms_against_the_float64_formulas_on_the_devices_anchored_rows(hip, world):
    km, sel, lib = world["km"], world["sel"], world["lib"]
    rng = np.random.default_rng(3)
    clip, time = clocks(rng, lib)
    exact, far = 11, 29
    weight = np.array([1.0, 0.5, 2.0, 0.0, 1.0, 3.0], F)
    plain, moved = tracker(lib, N, DT, seed=9), tracker(lib, N, DT, seed=9)
    moved.set_anchor(*random_anchors(rng))
    for t in (plain, moved):
        t.assign(clip, time)
        t.set_links(km, bodies=sel, link_weight=weight, frame="world")
        t.set_link_terms(weights=[1.0, 0.5, 0.25, 2.0], fail_dist=0.45)
    ref = moved.step_links(advance=False)
    sim, links = random_sim(rng, ref), random_links(rng, ref, amp=0.05)          # the anchored reference plus noise
    for k, r in (("base_pos", "ref_root_pos"), ("base_quat", "ref_root_rot"), ("base_lin_vel", "ref_root_vel"), ("base_ang_vel", "ref_root_ang_vel"),
                 ("dof_pos", "ref_dof_pos"), ("dof_vel", "ref_dof_vel")):
        sim[k][exact] = ref[r][exact]
    for k in lm.FIELDS:
        links[k][exact] = ref["ref_" + k][exact]
    links["body_pos"][far, 2] += F([0.0, 0.7, 0.0])
    out = moved.step_links(sim, links, advance=False)
    for k in ROOT_ROWS + BODY_ROWS:
        same(out[k], ref[k], k)
    err, term, total = tm.tracking_terms(out, sim, np.ones(km.num_dof), tm.DEFAULT_SCALES, np.ones(6))
    lwant = lm.link_terms(out, links, weight, lm.DEFAULT_LINK_SCALES, (1.0, 0.5, 0.25, 2.0), 0.45)
    rest = np.arange(N) != exact
    # (the rotation terms of an exact match are acos at 1, where float32 and float64 part ways: that environment is pinned below)
    link_total = assert_close_to_mirror({k: out[k][rest] for k in LINK_OUT}, tuple(a[rest] for a in lwant), 0.45)
    for k, w in (("err", err), ("term", term), ("total", total + lwant[4])):
        dev = np.abs(out[k][rest] - w[rest]) / np.maximum(1.0, np.abs(w[rest]))
        print(f"anchored {k}: max deviation {dev.max():.3e} x max(1, |x|), bound 2.0e-06")
        assert (dev <= 2e-6).all(), (k, dev.max())
    assert not np.isnan(link_total).any()
    assert out["fail"][far] == 1 and out["max_dist"][far] > 0.6 and out["fail"].sum() == 1
    # the exact match: no distance at all; its two angles are 2 acos(|q|^2) of a quaternion that is a unit one to a few 2^-24
    nonrot = [0, 2, 3, 4, 5]
    assert not out["err"][exact, nonrot].any() and (out["term"][exact, nonrot] == 1.0).all()
    assert not out["link_err"][exact, [0, 2, 3]].any() and out["max_dist"][exact] == 0.0 and out["fail"][exact] == 0
    assert out["err"][exact, 1] <= 3e-3 and out["link_err"][exact, 1] <= 3e-3          # 2 acos(1 - 1e-6) = 2.8e-3
    assert 6 + 3.75 - 0.05 <= out["total"][exact] <= 6 + 3.75
    # the heading frame does not see the anchor: link rows and link terms bit for bit, with an anchor and without
    for t in (plain, moved):
        t.set_links(km, bodies=sel, link_weight=weight, frame="heading")
    hp, hw = plain.step_links(sim, links, advance=False), moved.step_links(sim, links, advance=False)
    for k in BODY_ROWS + LINK_OUT:
        same(hw[k], hp[k], ("heading", k))
    assert not np.array_equal(hw["err"][:, 0], hp["err"][:, 0]) and hw["max_dist"].max() > 0


# ---- 4. anchor_to_root ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("listed", [False, True])
def test_anchor_to_root_is_the_mirrors_from_the_samplers_rows(hip, world, listed):
    lib = world["lib"]
    rng = np.random.default_rng(40 + listed)
    clip, time = clocks(rng, lib)
    bad_clip, bad_root = 6, 17
    clip[bad_clip] = 7
    t = tracker(lib, N, DT, loop=False, seed=2)
    t.assign(clip, time)
    s = lib.sample(clip, time.astype(np.float64), False)
    sampled = s["status"] == 0
    assert not sampled[bad_clip] and sampled.sum() == N - 1
    pos0, yaw0 = random_anchors(rng)
    root_pos = rng.uniform(-5, 5, (N, 3)).astype(F)
    q = rng.normal(size=(N, 4))
    root_quat = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    root_pos[bad_root, 0] = np.nan
    mask = rng.uniform(size=N) < 0.5
    mask[[bad_clip, bad_root, 0, 1]] = True
    mask[2] = False
    if listed:          # a list in another order that leaves environments out and names two ids outside [0, N)
        ids = np.concatenate([rng.permutation(N)[:30], [N, -1]]).astype(np.int32)
        rng.shuffle(ids)
    else:
        ids = np.arange(N, dtype=np.int32)
    inside = (ids >= 0) & (ids < N)
    e = np.where(inside, ids, 0)
    serve = np.zeros(N, bool)
    serve[e[inside & mask[e]]] = True
    args = dict(mask=mask[e], env_ids=ids) if listed else dict(mask=mask)
    for flags in (0, 1, 2, 3):
        t.set_anchor(pos0, yaw0)
        before = t.anchor_state()
        ignored = t.anchor_to_root(root_pos[e], root_quat[e], yaw=bool(flags & 1), z=bool(flags & 2), **args)
        assert ignored == int((~inside & mask[e]).sum())
        got = t.anchor_state()
        want_pos, want_yaw = am.to_root(before["pos"], before["yaw_zw"], s["root_pos"], s["root_rot"], root_pos, root_quat, flags, serve & sampled)
        same(got["pos"], want_pos, ("pos", flags))
        same(got["yaw_zw"], want_yaw, ("yaw_zw", flags))
        kept = ~serve
        kept[[bad_clip, bad_root]] = True
        same(got["pos"][kept], before["pos"][kept], ("kept pos", flags))
        same(got["yaw_zw"][kept], before["yaw_zw"][kept], ("kept yaw", flags))
        assert not np.array_equal(got["pos"][~kept, :2], before["pos"][~kept, :2])
    # YAW | Z: the reference now stands where the robot stands, in position and heading
    on = ~kept
    assert 5 <= on.sum() <= N - 4
    out = t.step_links(advance=False)
    bound = bound_of(s["root_pos"][:, :2], got["pos"])
    dev = np.abs(out["ref_root_pos"].astype(np.float64) - root_pos)[on].max(axis=1) / bound[on]
    gap = heading_gap(out["ref_root_rot"][on], root_quat[on]) / bound[on]
    print(f"anchor_to_root: position {dev.max():.3f}, heading {gap.max():.3f} of 1e-6 x max(1, |x| + |y| + |t|)")
    assert dev.max() <= 1.0 and gap.max() <= 1.0
    st = t.state()
    same(st["clip"], clip, "clip")
    same(st["time"], time, "time")


# ---- 5. device entry points and streams -------------------------------------------------------------------------------------------
def test_device_entry_points_on_a_stream_of_their_own_equal_the_host_twins(hip, world):
    km, sel, lib = world["km"], world["sel"], world["lib"]
    rng = np.random.default_rng(5)
    clip, time = clocks(rng, lib)
    host, dev = tracker(lib, N, DT, loop=False, seed=4), tracker(lib, N, DT, loop=False, seed=4)
    st = hip.Stream()
    L = hip.lib()
    some = hip.DeviceBuffer(N * 16)
    assert L.gmr_motion_tracker_set_anchor_dev(dev.handle, N, None, some.ptr, None, st.ptr) != 0
    assert b"not enabled" in L.gmr_last_error()
    assert L.gmr_motion_tracker_anchor_to_root_dev(dev.handle, N, None, None, some.ptr, some.ptr, 3, None) != 0 and b"not enabled" in L.gmr_last_error()
    assert L.gmr_motion_tracker_anchor_state(dev.handle, None, None) != 0 and b"not enabled" in L.gmr_last_error()
    with pytest.raises(ValueError, match="enable_anchors"):
        dev.set_anchor_dev(pos=some)
    dev.enable_anchors()
    for t in (host, dev):
        t.assign(clip, time)
        t.set_links(km, bodies=sel, frame="world")
    # set_anchor: every environment, then a list with three ids outside [0, N)
    pos, yaw = random_anchors(rng)
    ids = np.array([5, N, 36, -3, 0, 19, 1 << 20], dtype=np.int32)
    pos2, yaw2 = random_anchors(rng, len(ids))
    assert host.set_anchor(pos, yaw) == 0 and host.set_anchor(pos2, None, env_ids=ids) == 3 and host.set_anchor(None, yaw2, env_ids=ids) == 3
    dev.set_anchor_dev(hip.DeviceBuffer.from_host(pos), hip.DeviceBuffer.from_host(yaw), stream=st)
    d_ids = hip.DeviceBuffer.from_host(ids)
    dev.set_anchor_dev(pos=hip.DeviceBuffer.from_host(pos2), env_ids=d_ids, n=len(ids), stream=st)
    dev.set_anchor_dev(yaw=hip.DeviceBuffer.from_host(yaw2), env_ids=d_ids, n=len(ids), stream=st)
    st.sync()
    a, b = host.anchor_state(), dev.anchor_state()
    same(b["pos"], a["pos"], "set_anchor_dev pos")
    same(b["yaw_zw"], a["yaw_zw"], "set_anchor_dev yaw: the kernel's half angle is the host's")
    assert host.state()["ignored"] == dev.state()["ignored"] == 6
    # anchor_to_root with a mask, then a link step, all on the stream
    root_pos = rng.uniform(-5, 5, (N, 3)).astype(F)
    q = rng.normal(size=(N, 4))
    root_quat = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    mask = (rng.uniform(size=N) < 0.5).astype(np.int32)
    assert host.anchor_to_root(root_pos, root_quat, mask=mask, yaw=True, z=True) == 0
    want = host.step_links()
    G, sentinel = 64, F(-77.25)
    widths = {"ref_root_pos": 3, "ref_root_rot": 4, "ref_root_vel": 3, "ref_root_ang_vel": 3, "ref_dof_pos": km.num_dof, "ref_dof_vel": km.num_dof,
              "status": 1, "finished": 1, "ref_body_pos": 18, "ref_body_rot": 24, "ref_body_vel": 18, "ref_body_ang_vel": 18}
    bufs = {k: hip.DeviceBuffer.from_host(np.full(N * w + G, sentinel, F)) for k, w in widths.items()}
    dev.anchor_to_root_dev(hip.DeviceBuffer.from_host(root_pos), hip.DeviceBuffer.from_host(root_quat), mask=hip.DeviceBuffer.from_host(mask),
                           yaw=True, z=True, stream=st)
    dev.step_links_dev(stream=st, **bufs)
    st.sync()
    a, b = host.anchor_state(), dev.anchor_state()
    same(b["pos"], a["pos"], "anchor_to_root_dev pos")
    same(b["yaw_zw"], a["yaw_zw"], "anchor_to_root_dev yaw")
    assert not np.array_equal(a["pos"], pos)
    for k, w in widths.items():
        got = bufs[k].to_host(N * w + G, F)
        assert (got[N * w:] == sentinel).all(), k          # the guard words
        got = got[:N * w].view(want[k].dtype).reshape(want[k].shape)
        same(got, want[k], k)
    sa, sb = host.state(), dev.state()
    for k in STATE:
        same(sa[k], sb[k], k)


# ---- 6. continuity by composition -------------------------------------------------------------------------------------------------
def test_a_finished_clip_continues_from_the_pose_it_ended_in(hip, world):
    lib = world["lib"]
    rng = np.random.default_rng(6)
    ending = (1, 5, 16, 33, 36)
    clip, time = clocks(rng, lib, near_end=ending)
    t = tracker(lib, N, DT, loop=False, seed=8)
    t.set_anchor(*random_anchors(rng))
    t.assign(clip, time)
    pre = t.anchor_state()
    st = hip.Stream()
    pos, rot, fin = hip.DeviceBuffer(N * 12), hip.DeviceBuffer(N * 16), hip.DeviceBuffer(N * 4)
    t.step_dev(stream=st, ref_root_pos=pos, ref_root_rot=rot, finished=fin)
    t.anchor_to_root_dev(pos, rot, mask=fin, yaw=True, z=False, stream=st)          # the step's own buffers: no copy, no read-back
    st.sync()
    end_pos, end_rot, finished = pos.to_host((N, 3), F), rot.to_host((N, 4), F), fin.to_host(N, np.int32)
    assert finished.sum() >= len(ending) and finished[list(ending)].all()
    fin_b = finished == 1
    before = t.anchor_state()
    s0 = t.state()
    assert (s0["time"][fin_b] == 0).all()
    # the mirror: the anchor from the sampler's row at the new (clip, clock), then that anchor on the rows of the next two clocks
    a0 = lib.sample(s0["clip"], s0["time"].astype(np.float64), False)
    want_pos, want_yaw = am.to_root(pre["pos"], pre["yaw_zw"], a0["root_pos"], a0["root_rot"], end_pos, end_rot, am.ANCHOR_YAW, fin_b)
    same(before["pos"], want_pos, "anchor_pos from the step's own buffers")
    same(before["yaw_zw"], want_yaw, "anchor_yaw from the step's own buffers")
    same(before["pos"][~fin_b], pre["pos"][~fin_b], "environments that went on keep their anchor")
    nxt = t.step()
    same(nxt["ref_root_pos"], am.apply_pos(before["pos"], before["yaw_zw"], a0["root_pos"]), "next ref_root_pos")
    same(nxt["ref_root_rot"], am.apply_quat(before["yaw_zw"], a0["root_rot"]), "next ref_root_rot")
    bound = bound_of(a0["root_pos"][:, :2], before["pos"])
    dev = np.abs(nxt["ref_root_pos"][:, :2].astype(np.float64) - end_pos[:, :2])[fin_b].max(axis=1) / bound[fin_b]
    gap = heading_gap(nxt["ref_root_rot"][fin_b], end_rot[fin_b]) / bound[fin_b]
    print(f"continuity: xy {dev.max():.3f}, heading {gap.max():.3f} of 1e-6 x max(1, |x| + |y| + |t|)")
    assert dev.max() <= 1.0 and gap.max() <= 1.0
    # one clock step on: the end pose plus the new clip's own root motion over that step, as the mirror moves it
    s1 = t.state()
    ok = s1["draws"] == s0["draws"]                      # (clips of one or two frames end again at once)
    a1 = lib.sample(s1["clip"], s1["time"].astype(np.float64), False)
    after = t.step()
    same(after["ref_root_pos"][ok], am.apply_pos(before["pos"], before["yaw_zw"], a1["root_pos"])[ok], "ref_root_pos one step on")
    moved = am.apply_pos(before["pos"], before["yaw_zw"], a1["root_pos"]).astype(np.float64) - am.apply_pos(before["pos"], before["yaw_zw"], a0["root_pos"])
    both = fin_b & ok
    if both.any():
        dev = np.abs(after["ref_root_pos"][:, :2] - (end_pos[:, :2].astype(np.float64) + moved[:, :2]))[both].max(axis=1) / bound[both]
        assert dev.max() <= 1.0
    same(t.anchor_state()["pos"], before["pos"], "the anchor stays")


# ---- 7. the preview's sim frame ---------------------------------------------------------------------------------------------------
def test_sim_frame_preview_is_the_anchored_reference_seen_from_the_simulators_root(hip, world):
    lib = world["lib"]
    rng = np.random.default_rng(7)
    clip, time = clocks(rng, lib)
    plain, moved = tracker(lib, N, DT, seed=1), tracker(lib, N, DT, seed=1)
    moved.set_anchor(*random_anchors(rng))
    for t in (plain, moved):
        t.assign(clip, time)
    lay = moved.set_preview(OFFSETS, pm.BLOCKS, "raw", PREVIEW_BODIES)
    raw = moved.preview()["obs"]
    q = rng.normal(size=(N, 4))
    sim = {"base_pos": (raw[:, 2, lay["root_pos"]] + rng.normal(0, 0.5, (N, 3))).astype(F), "base_quat": (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)}
    assert moved.set_preview(OFFSETS, pm.BLOCKS, "sim", PREVIEW_BODIES) == lay
    got = moved.preview(sim)
    rows = {b: raw[:, :, lay[b]] for b in ("root_pos", "root_quat", "root_vel", "root_ang_vel")}
    rows["body_pos"] = raw[:, :, lay["body_pos"]].reshape(N, len(OFFSETS), len(PREVIEW_BODIES), 3)
    want = pm.transform(rows, sim["base_pos"], sim["base_quat"])
    for b in ("root_pos", "root_quat", "root_rot6", "root_vel", "root_ang_vel", "body_pos"):
        within(got["obs"][:, :, lay[b]], want[b].reshape(N, len(OFFSETS), -1), BOUND[b], f"anchored sim {b}")
    for b in ("dof_pos", "dof_vel"):
        same(got["obs"][:, :, lay[b]], raw[:, :, lay[b]], b)
    plain.set_preview(OFFSETS, pm.BLOCKS, "sim", PREVIEW_BODIES)
    unmoved = plain.preview(sim)
    assert np.abs(got["obs"][:, :, lay["root_pos"]] - unmoved["obs"][:, :, lay["root_pos"]]).max() > 1.0
    # the reference frame does not see the anchor
    for t in (plain, moved):
        t.set_preview(OFFSETS, pm.BLOCKS, "reference", PREVIEW_BODIES)
    a, b = plain.preview(), moved.preview()
    for k in ("obs", "valid", "status"):
        same(b[k], a[k], ("reference", k))
