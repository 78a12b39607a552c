"""The tracker's link step on a real MI355X (csrc/gmr_tracker_links.hip through motion_tracker.py): reference rows bit-equal to
``gmr_motion_body_state``, the plain outputs and the state bit-equal to a twin tracker driven by plain ``step``, the link terms against
the float64 mirror (tests/links_mirror.py), layouts, frames, bad rows, the no-advance flag and detaching.  Every test makes one pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import links_mirror as lm  # noqa: E402
from test_motion_body_state import same_bits, sentinel_buffer  # noqa: E402
from test_motion_body_state_host import kinematics  # noqa: E402
from test_motion_library import _bits, device_library, make_motions  # noqa: E402
from test_motion_tracker import STATE, random_sim, tracker  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
PLAIN = ("ref_root_pos", "ref_root_rot", "ref_root_vel", "ref_root_ang_vel", "ref_dof_pos", "ref_dof_vel", "err", "term", "total", "status", "finished")
REF = {"ref_body_pos": "body_pos", "ref_body_rot": "body_rot", "ref_body_vel": "body_vel", "ref_body_ang_vel": "body_ang_vel"}


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def random_links(rng, out, amp=0.2):
    """a simulator near the device's own reference rows: ``[N, nsel, k]`` float32, quaternions tens of degrees away"""
    q = out["ref_body_rot"] + rng.normal(0, 0.4, out["ref_body_rot"].shape)
    links = {"body_pos": out["ref_body_pos"] + rng.normal(0, amp, out["ref_body_pos"].shape), "body_rot": q / np.linalg.norm(q, axis=2, keepdims=True),
             "body_vel": out["ref_body_vel"] + rng.normal(0, amp, out["ref_body_vel"].shape),
             "body_ang_vel": out["ref_body_ang_vel"] + rng.normal(0, amp, out["ref_body_ang_vel"].shape)}
    return {k: np.ascontiguousarray(v, dtype=F) for k, v in links.items()}


def assert_close_to_mirror(out, want, fail_dist=np.inf):
    err, term, md, fail, total = want
    for k, w in (("link_err", err), ("link_term", term), ("max_dist", md)):
        tol = 2e-6 * np.maximum(1.0, np.abs(w))
        if k == "link_err":          # the angle: acos turns the rounding of its argument into 1.2e-7 / sin(theta / 2) per link
            tol = tol + np.array([0.0, 2e-5, 0.0, 0.0])
        if k == "link_term":
            tol = tol + np.array([0.0, 4e-5, 0.0, 0.0])
        bad = ~(np.abs(out[k] - w) <= tol) & ~(np.isnan(out[k]) & np.isnan(w))
        assert not bad.any(), (k, np.abs(out[k] - w)[bad].max())
    near = np.abs(md - fail_dist) <= 2e-6 * np.maximum(1.0, np.abs(md))
    assert np.array_equal(out["fail"][~near], fail[~near])
    return total


@pytest.mark.parametrize("robot", ["unitree_g1", "booster_t1", "stanford_toddy"])
@pytest.mark.parametrize("loop", [True, False])
@pytest.mark.parametrize("all_bodies", [True, False])
def test_references_are_body_states_bits_and_the_plain_step_is_untouched(hip, robot, loop, all_bodies):
    km = kinematics(robot)
    rng = np.random.default_rng(11 + len(robot) + 2 * loop + all_bodies)
    motions = make_motions(rng, [1, 2, 65, 300] + rng.integers(2, 120, size=8).tolist(), km.num_dof, 0)
    lib = device_library(hip, motions)
    N = 333
    sel = None if all_bodies else rng.permutation(len(km.body_names))[:6].tolist()
    a, b = tracker(lib, N, 0.02, loop=loop, seed=77), tracker(lib, N, 0.02, loop=loop, seed=77)
    a.set_links(km, bodies=sel)
    sim = None
    for step in range(200):
        if step in (0, 120):
            for t in (a, b):
                t.reset(time_offset_range=(0.0, 3.0))
        if step % 40 == 0:
            st = a.state()
            want = lib.body_state(st["clip"], st["time"].astype(np.float64), kinematics=km, loop=loop, bodies=sel, state=False)
        got, plain = a.step_links(sim), b.step(sim)
        if step % 40 == 0:
            for k, r in REF.items():
                assert same_bits(got[k], want[r]), (step, k)
        for k in PLAIN:
            if k in plain:
                assert same_bits(got[k], plain[k]), (step, k)
        if sim is None:
            sim = random_sim(rng, plain)
    sa, sb = a.state(), b.state()
    for k in STATE:
        assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
    if not loop:
        assert sa["draws"].max() > 2
    a.close(), b.close()


@pytest.mark.parametrize("frame", ["world", "heading"])
def test_link_terms_against_the_mirror_packed_and_separate_layouts(hip, frame):
    km = kinematics("unitree_g1")
    names = km.body_names
    rng = np.random.default_rng(23)
    motions = make_motions(rng, [40, 257, 90], km.num_dof, 0)
    lib = device_library(hip, motions)
    N, sel = 700, [29, 3, 15, 0, 36, 8]
    weight = np.array([1.0, 0.5, 2.0, 0.0, 1.0, 3.0], F)
    t = tracker(lib, N, 0.02, seed=3)
    t.reset(time_offset_range=(0.0, 4.0))
    t.set_links(km, bodies=[names[i] for i in sel], link_weight=weight, frame=frame)
    t.set_link_terms(weights=[1.0, 0.5, 0.0, 2.0], fail_dist=0.45)
    ref = t.step_links(advance=False)
    sim = random_sim(rng, ref)
    links = random_links(rng, ref)
    if frame == "heading":       # the rows above are heading-frame rows: put them around the simulator's (drifted) root
        z, w = lm.yaw_quat(sim["base_quat"])
        c, s = (w * w - z * z)[:, None], (2 * z * w)[:, None]
        p = links["body_pos"].astype(np.float64)
        links["body_pos"] = (np.stack([c * p[..., 0] - s * p[..., 1], s * p[..., 0] + c * p[..., 1], p[..., 2]], -1) + sim["base_pos"][:, None]).astype(F)
    links["body_pos"][5, 2] = np.nan
    out = t.step_links(sim, links, advance=False)
    base = (sim["base_pos"], sim["base_quat"]) if frame == "heading" else None
    want = lm.link_terms(out, links, weight, lm.DEFAULT_LINK_SCALES, (1.0, 0.5, 0.0, 2.0), 0.45, base)
    link_total = assert_close_to_mirror(out, want, 0.45)
    assert out["fail"][5] == 1 and np.isnan(out["max_dist"][5]) and 0 < out["fail"].sum() < N
    plain = t.step(sim)                                   # the six terms alone: total = theirs + the link terms
    ok = ~np.isnan(link_total)
    assert np.abs(out["total"][ok] - (plain["total"][ok].astype(np.float64) + link_total[ok])).max() < 1e-5
    # world frame: the references are body_state's; heading: the mirror's within a tolerance
    t.assign(np.zeros(N, np.int32), rng.uniform(0, 1, N).astype(F))
    st = t.state()
    got = t.step_links(advance=False)
    bs = lib.body_state(st["clip"], st["time"].astype(np.float64), kinematics=km, bodies=sel)
    rows = [bs[k] for k in lm.FIELDS]
    if frame == "heading":
        rows = lm.to_heading(bs["root_pos"], bs["root_rot"], *rows)
        for k, r in zip(REF, rows):
            assert np.abs(got[k] - r).max() < 5e-6 * max(1.0, np.abs(r).max()), k
    else:
        for k, r in zip(REF, rows):
            assert same_bits(got[k], r), k
    # packed [N][nb][13] with a permuting sim_body gives the bits of the four gathered arrays
    nb = len(names) + 3
    perm = rng.permutation(nb)[:len(sel)].astype(np.int32)
    packed = rng.normal(size=(N, nb, 13)).astype(F)
    for k, (off, wd) in {"body_pos": (0, 3), "body_rot": (3, 4), "body_vel": (7, 3), "body_ang_vel": (10, 3)}.items():
        packed[:, perm, off:off + wd] = links[k]
    sep = t.step_links(sim, links, advance=False)
    t.set_links(km, bodies=sel, sim_bodies=perm, link_weight=weight, frame=frame)
    pk = t.step_links(sim, {"body_state": packed}, advance=False)
    for k in ("link_err", "link_term", "max_dist", "fail", "total"):
        assert same_bits(sep[k], pk[k]), k
    t.close()


@pytest.mark.parametrize("sel", [[37], [18, 37, 7, 0, 15, 17]])
def test_one_wavefront_and_shared_trunk_bodies_with_weights(hip, sel):
    """[37]: the plan is one chain, a workgroup of ONE wavefront.  The other: the root and the torso (walked by several wavefronts, served
    by one) beside leaves of three limbs, weighted."""
    km = kinematics("unitree_g1")
    rng = np.random.default_rng(40 + len(sel))
    lib = device_library(hip, make_motions(rng, [90, 33, 150], km.num_dof, 0))
    N = 515
    weight = rng.uniform(0.2, 2.0, len(sel)).astype(F)
    t, twin = tracker(lib, N, 0.02, seed=8), tracker(lib, N, 0.02, seed=8)
    for x in (t, twin):
        x.reset(time_offset_range=(0.0, 3.0))
    t.set_links(km, bodies=sel, link_weight=weight)
    st = t.state()
    want = lib.body_state(st["clip"], st["time"].astype(np.float64), kinematics=km, bodies=sel, state=False)
    ref = t.step_links(advance=False)
    for k, r in REF.items():
        assert same_bits(ref[k], want[r]), k
    sim, links = random_sim(rng, ref), random_links(rng, ref)
    out = t.step_links(sim, links, advance=False)
    assert_close_to_mirror(out, lm.link_terms(out, links, weight))
    got, plain = t.step_links(sim), twin.step(sim)                # no link arrays: the plain step, total included
    for k in PLAIN:
        assert same_bits(got[k], plain[k]), k
    t.close(), twin.close()


def long_trunk_handle(hip, rng, trunk=22, leaves=42):
    """an FK handle of a tree the three robots do not resemble: a serial trunk of ``trunk`` bodies (the FK handle takes 24 levels) with ``leaves`` leaves at
    its end, a hinge on every body but the root: four wavefronts re-walk the trunk, 4 x 22 + 42 = 130 steps"""
    nb = trunk + leaves
    axis = rng.normal(size=(nb, 3))
    axis[::3] = np.eye(3)[rng.integers(0, 3, size=len(axis[::3]))]          # some exactly along an axis
    q = rng.normal(size=(nb, 4)) * 0.2 + np.array([0, 0, 0, 1.0])
    q[::2] = [0, 0, 0, 1]
    tree = {"parent": np.array([-1] + list(range(trunk - 1)) + [trunk - 1] * leaves, np.int32), "local_translation": rng.normal(0, 0.05, (nb, 3)).astype(F),
            "local_rotation": (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F), "dof_idx": np.arange(-1, nb - 1).astype(np.int32),
            "dof_dim": np.array([0] + [1] * (nb - 1), np.int32), "axis": axis / np.linalg.norm(axis, axis=1, keepdims=True)}
    return hip.FkHandle(tree)


def test_a_long_trunk_needs_more_than_128_steps_and_walks_right(hip):
    rng = np.random.default_rng(12)
    fk = long_trunk_handle(hip, rng)
    assert fk.nbody == 64 and fk.ndof == 63
    lib = device_library(hip, make_motions(rng, [60, 45], fk.ndof, 0))
    N = 200
    t = tracker(lib, N, 0.02, seed=1)
    t.reset(time_offset_range=(0.0, 1.0))
    st = t.state()
    for sel in (None, [63, 5, 22, 0, 40]):
        t.set_links(fk, bodies=sel)
        want = lib.body_state(st["clip"], st["time"].astype(np.float64), kinematics=fk, bodies=sel, state=False)
        ref = t.step_links(advance=False)
        for k, r in REF.items():
            assert same_bits(ref[k], want[r]), (sel, k)
        sim, links = random_sim(rng, ref), random_links(rng, ref)
        out = t.step_links(sim, links, advance=False)
        assert_close_to_mirror(out, lm.link_terms(out, links))
    t.close()


def test_heading_frame_does_not_see_drift_on_the_device(hip):
    km = kinematics("booster_t1")
    rng = np.random.default_rng(31)
    lib = device_library(hip, make_motions(rng, [120, 80], km.num_dof, 0))
    N = 256
    t = tracker(lib, N, 0.02, seed=9)
    t.reset(time_offset_range=(0.0, 2.0))
    t.set_links(km, frame="heading")
    ref = t.step_links(advance=False)
    sim = random_sim(rng, ref)
    links = random_links(rng, ref)
    e0 = t.step_links(sim, links, advance=False)["link_err"]
    a = 0.9
    c, s = np.cos(a), np.sin(a)
    shift = np.array([4.0, -3.0, 0.0], F)

    def rz(v):
        return np.stack([c * v[..., 0] - s * v[..., 1], s * v[..., 0] + c * v[..., 1], v[..., 2]], -1)

    qa = np.array([0.0, 0.0, np.sin(a / 2), np.cos(a / 2)])
    sim2 = dict(sim, base_pos=(rz(sim["base_pos"]) + shift).astype(F), base_quat=lm.bm.qmul(np.broadcast_to(qa, (N, 4)), sim["base_quat"]).astype(F))
    links2 = {"body_pos": (rz(links["body_pos"]) + shift).astype(F), "body_rot": lm.bm.qmul(np.broadcast_to(qa, links["body_rot"].shape), links["body_rot"]).astype(F),
              "body_vel": rz(links["body_vel"]).astype(F), "body_ang_vel": rz(links["body_ang_vel"]).astype(F)}
    e1 = t.step_links(sim2, links2, advance=False)["link_err"]
    assert (np.abs(e1 - e0) <= 2e-5 * np.maximum(1.0, e0)).all() and (e0 > 1e-2).all()          # (the moved rows are rounded to float32)
    # ... and it is not blind to a sunken robot
    sim3 = dict(sim, base_pos=sim["base_pos"] + np.array([0, 0, 0.3], F))
    e2 = t.step_links(sim3, links, advance=False)["link_err"]
    assert (np.abs(e2 - e0)[:, 0] > 1e-2).any()
    t.close()


def test_bad_assignments_no_advance_one_link_and_detaching(hip):
    km = kinematics("unitree_g1")
    rng = np.random.default_rng(5)
    lib = device_library(hip, make_motions(rng, [50, 70, 31], km.num_dof, 0))
    N, sel = 130, [12, 4, 33]
    t = tracker(lib, N, 0.02, loop=False, seed=2)
    t.reset(time_offset_range=(0.0, 0.5))
    t.set_links(km, bodies=sel)
    t.assign([7, -1, 1], [0.1, 0.2, np.nan], env_ids=[3, 64, 129])
    before = t.state()
    ref = t.step_links(advance=False)
    links = random_links(rng, {k: np.nan_to_num(v) for k, v in ref.items()})
    sim = random_sim(rng, {k: np.nan_to_num(v) for k, v in ref.items()})
    # device buffers with guard floats behind every link output, on a stream of its own
    shapes = {"ref_body_pos": 9, "ref_body_rot": 12, "ref_body_vel": 9, "ref_body_ang_vel": 9, "link_err": 4, "link_term": 4, "max_dist": 1,
              "total": 1}
    bufs = {k: sentinel_buffer(hip, N, w) for k, w in shapes.items()}
    d_links = {k: hip.DeviceBuffer.from_host(v) for k, v in links.items()}
    d_sim = {k: hip.DeviceBuffer.from_host(v) for k, v in sim.items()}
    d_fail, d_status = hip.DeviceBuffer.from_host(np.full(N + 64, -9, np.int32)), hip.DeviceBuffer.from_host(np.full(N + 64, -9, np.int32))
    st = hip.Stream()
    t.step_links_dev(d_sim, d_links, advance=False, stream=st, fail=d_fail, status=d_status, **{k: b for k, (b, _) in bufs.items()})
    st.sync()
    host = t.step_links(sim, links, advance=False)           # the synchronous twin: the same bits
    bad = np.array([3, 64, 129])
    for k, w in shapes.items():
        got = bufs[k][0].to_host((N + 64, w), F)
        assert np.array_equal(_bits(got[N:]), _bits(bufs[k][1][N:])), k          # the guard floats
        assert same_bits(got[:N].reshape(host[k].shape), host[k]), k
        assert np.isnan(got[bad]).all() and not np.isnan(np.delete(got[:N], bad, axis=0)).any(), k
    fail, status = d_fail.to_host((N + 64,), np.int32), d_status.to_host((N + 64,), np.int32)
    assert (fail[N:] == -9).all() and (status[N:] == -9).all()
    assert (fail[bad] == 0).all() and (status[bad] == 1).all() and status[:N].sum() == 3
    after = t.state()
    for k in STATE:                                          # the no-advance steps left the state alone
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
    adv = t.step_links(sim, links)                           # the advancing step computes the same rows, then moves
    for k in host:
        if k != "finished":
            assert same_bits(adv[k], host[k]), k
    moved = t.state()
    good = np.delete(np.arange(N), bad)
    assert (moved["time"][good] != before["time"][good]).all() and np.array_equal(_bits(moved["time"][bad]), _bits(before["time"][bad]))
    # reference-state initialisation: after a reset the no-advance rows sit at the new clocks
    t.reset(time_offset_range=(0.0, 0.4))
    s2 = t.state()
    init = t.step_links(advance=False)
    want = lib.body_state(s2["clip"], s2["time"].astype(np.float64), kinematics=km, loop=False, bodies=sel, state=False)
    for k, r in REF.items():
        assert same_bits(init[k], want[r]), k
    # one link of weight one: e_pos is that link's distance
    t.set_links(km, bodies=sel, link_weight=[0.0, 1.0, 0.0])
    one = t.step_links(sim, links, advance=False)
    d = np.linalg.norm(links["body_pos"][:, 1].astype(np.float64) - one["ref_body_pos"][:, 1], axis=1)
    assert np.abs(one["link_err"][:, 0] - d).max() < 2e-6 and np.abs(one["max_dist"] - d).max() < 2e-6
    # detached: a link step is a plain step and demands no link arrays
    t.set_links(bodies=[])
    twin = tracker(lib, N, 0.02, loop=False, seed=2)
    twin.assign(s2["clip"], s2["time"])
    got, plain = t.step_links(sim), twin.step(sim)
    assert set(got) == set(plain) and all(same_bits(got[k], plain[k]) for k in plain)
    with pytest.raises(ValueError, match="set_links"):
        t.step_links(sim, links)
    t.close(), twin.close()


def test_an_environment_sees_the_same_links_whatever_surrounds_it(hip):
    km = kinematics("unitree_g1")
    rng = np.random.default_rng(6)
    lib = device_library(hip, make_motions(rng, [50, 70, 31, 200], km.num_dof, 0))
    outs = []
    for N in (64, 5000):
        t = tracker(lib, N, 0.02, loop=False, seed=4)
        t.reset(time_offset_range=(0.0, 0.5))
        t.set_links(km, bodies=[5, 20, 31, 11])
        rows = []
        for _ in range(60):
            o = t.step_links()
            rows.append(np.concatenate([o[k][7].ravel() for k in REF] + [o["finished"][7:8].astype(F)]))
        outs.append(np.stack(rows))
        t.close()
    assert same_bits(outs[0], outs[1])
