"""The tracker's terrain and feet on a real MI355X (csrc/gmr_tracker_feet.hip through motion_tracker.py): the terrain
heights are the reference's bits (the fixture's) and the mirror's; every output of a feet step and both state arrays are the statement of
tests/feet_mirror.py bit for bit, except what passes through atan2f, cosf or sinf -- the two angles, the two gait columns, four terms and the
total --, which is bounded from the largest deviation met on an MI355X.  N = 37 environments (no multiple of 16 or 64) on the four-clip
library of test_tracker_control.py, nb = 11 bodies, E in {1, 4, 8} edge points, a 23 x 17 field and the plane, 64 guard floats behind every
device output; every test makes one pass."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feet_mirror as fm  # noqa: E402
from test_motion_library import device_library, make_motions  # noqa: E402
from test_motion_tracker import STATE, tracker  # noqa: E402
from test_tracker_control import G, SENTINEL, hip, same, world  # noqa: E402,F401
from test_tracker_feet_host import ANGLE_UNIT, EPS, clamped_height, golden, golden_terrain, rough_field, term_bounds  # noqa: E402
from test_tracker_proprio import STATE6  # noqa: E402
from test_tracker_proprio import inputs as proprio_inputs  # noqa: E402
from test_tracker_proprio import setup as proprio_setup  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
N, NB, DT = 37, 11, 0.02
NX, NY, BORDER, HS, VS = 23, 17, 3, 0.1, 0.005
X_HI, Y_HI = (NX - 1 - BORDER) * HS, (NY - 1 - BORDER) * HS
FEET, TERMINATION, PENALIZED = (4, 9), (0, 3, 10), (1, 2, 5, 7, 8)
T1_EDGES = np.array([[0.1215, 0.05, -0.03], [0.1215, -0.05, -0.03], [-0.1015, 0.05, -0.03], [-0.1015, -0.05, -0.03]], F)
OUTPUTS = ("feet_pos", "feet_roll", "feet_yaw", "feet_contact", "ground", "gait", "term", "total", "done")
EXACT = ("feet_pos", "feet_contact", "ground", "done")
EXACT_TERMS, ANGLE_TERMS = (0, 1, 2, 7), (3, 4, 5, 6)
SCALES = {"collision": -1.0, "feet_slip": -0.1, "feet_vel_z": -0.05, "feet_roll": -0.2, "feet_yaw_diff": -1.0, "feet_yaw_mean": -1.0, "feet_distance": -10.0,
          "feet_swing": 3.0}
# No ulp figures of atan2f, cosf and sinf ship with the ROCm on the test machines, so the bounds are four times the largest deviation met on
# an MI355X at the shapes of this file: the mirror forms the float32 arguments bit-exactly and evaluates the function
# in float64.  Angles (feet_roll, feet_yaw) in units of 2^-24 max(1, 3 pi): largest met 1.698.  The gait columns in units of 2^-24: 1.0.
ANGLE_BOUND = 4 * 1.698
GAIT_BOUND = 4 * 1.0
CLEARANCE_MARGIN, ANGLE_MARGIN = 2e-5, 2e-3          # how far inputs stay from the contact threshold and from the angles' seams


def field_of(rng):
    field = rng.integers(-20, 60, (NX, NY)).astype(np.int16)
    field[:BORDER], field[-BORDER:], field[:, :BORDER], field[:, -BORDER:] = 0, 0, 0, 0
    return field


def edges_of(E):
    """the T1's four edge points, their first one alone, or the four and their midpoints-ish mirror images (eight)"""
    return {1: T1_EDGES[:1], 4: T1_EDGES, 8: np.concatenate([T1_EDGES, T1_EDGES * F(0.5) + F(0.004)])}[E].astype(F)


def setup(world, rng, n=N, E=4, terrain=True, termination=TERMINATION, penalized=PENALIZED, scales=SCALES, seed=3):
    """a tracker on the world's library with proprio, terrain and feet set, the feet mirror and the proprio mirror"""
    t, pmirror = proprio_setup(world, rng, n=n, seed=seed)
    ter = None
    if terrain:
        field = field_of(rng)
        t.set_terrain(field, HS, VS, BORDER)
        ter = fm.terrain(field, HS, VS, BORDER)
    kw = dict(termination_bodies=termination, penalized_bodies=penalized, feet_distance_ref=0.2, swing_period=0.2, scales=scales)
    t.set_feet(FEET, edges_of(E), NB, **kw)
    cfg = fm.config(FEET, edges_of(E), NB, termination, penalized, 1.0, 0.01, 0.2, 0.2, scales)
    return t, fm.Feet(cfg, ter, n, DT), pmirror


def quat_of(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)


def inputs(rng, mirror, n=N):
    """:func:`draw`, drawn again until the mirror's step stays 2e-5 clear of the contact threshold and 2e-3 of the angles' seams (the bounds of
    :func:`check` hold away from those discontinuities only; the same draws on every machine)"""
    for _ in range(100):
        x = draw(rng, mirror, n)
        trial = copy.deepcopy(mirror)
        mirror_step(trial, x)
        if trial.margins["clearance"] > CLEARANCE_MARGIN and trial.margins["angle"] > ANGLE_MARGIN:
            return x
    raise AssertionError("no draw away from the discontinuities")


def draw(rng, mirror, n=N):
    """seeded rigid bodies with the two feet near the terrain's surface inside the field, some feet turned past each other"""
    state = rng.normal(0, 1, (n, NB, 13))
    quat = rng.standard_normal((n, NB, 4))
    state[:, :, 3:7] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    xy = np.stack([rng.uniform(0.05, X_HI - 0.2, (n, 2)), rng.uniform(0.05, Y_HI - 0.2, (n, 2))], axis=-1)
    under, _ = fm.heights(mirror.ter, xy.reshape(-1, 2).astype(F))
    state[:, FEET, :2] = xy
    state[:, FEET, 2] = under.reshape(n, 2) + 0.03 + rng.uniform(-0.03, 0.06, (n, 2))
    heading = rng.uniform(-3.0, 3.0, (n, 1))
    turn = rng.uniform(-0.4, 0.4, (n, 2))
    turn[::7, 1] += 3.3                                        # |yaw_1 - yaw_0| beyond pi
    state[:, FEET, 3:7] = quat_of(rng.uniform(-0.25, 0.25, (n, 2)), rng.uniform(-0.25, 0.25, (n, 2)), heading + turn)
    root_quat = quat_of(rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), heading[:, 0] + rng.uniform(-0.3, 0.3, n))
    root = np.concatenate([xy.mean(axis=1), rng.uniform(0.5, 0.8, (n, 1)), root_quat, rng.normal(0, 1, (n, 6))], axis=1)
    forces = rng.normal(0, 0.6, (n, NB, 3))
    forces[rng.uniform(size=(n, NB)) < 0.5] = 0.0
    gf = rng.uniform(1.0, 2.5, n)
    gf[2 % n] = 0.0
    return {"body_state": state.astype(F), "root_states": root.astype(F), "contact_forces": forces.astype(F),
            "episode_steps": rng.integers(0, 4, n).astype(np.int32), "gait_frequency": gf.astype(F)}


def mirror_step(mirror, x):
    return mirror.step(x["body_state"][:, :, 0:3], x["body_state"][:, :, 3:7], x["root_states"], x["contact_forces"], x["episode_steps"], x["gait_frequency"])


def run_dev(hip, t, x, stream=None, want=OUTPUTS, keep=None):
    """feet_dev on the packed tensor into guarded buffers -> the outputs on the host, the guard floats checked"""
    n = t.num_envs
    _, counts = t._feet_counts()
    up = {k: None if a is None else hip.DeviceBuffer.from_host(a) for k, a in x.items()}
    out = {k: hip.DeviceBuffer.from_host(np.full(n * counts[k] + G, SENTINEL, dtype=F)) for k in want}
    t.feet_dev({"body_state": up["body_state"]}, up["root_states"], up["contact_forces"], up["episode_steps"], up["gait_frequency"], stream=stream, **out)
    hip.check(hip.lib().gmr_stream_sync(None if stream is None else stream.ptr))
    got = {}
    for k, b in out.items():
        raw = b.to_host(n * counts[k] + G, F)
        assert (raw[n * counts[k]:] == SENTINEL).all(), k                  # the guard floats
        a = raw[:n * counts[k]]
        if k in ("done", "feet_contact"):
            a = a.view(np.int32)
        got[k] = a.reshape({"feet_pos": (n, 2, 3), "ground": (n,), "total": (n,), "done": (n,)}.get(k, (n, counts[k]))).copy()
    if keep is not None:
        keep.update(out)
    return got


def check(got, want, mirror, what, forces=True, margins=True):
    """bit for bit, except the angles, the gait columns, the four angle terms and the total: bounded"""
    if margins:
        assert mirror.margins["clearance"] > 1e-5 and mirror.margins["angle"] > 1e-3, (what, mirror.margins)
    for k in EXACT:
        if k in got:
            same(got[k], want[k], (what, k))
    dev_angle = 0.0
    for k in ("feet_roll", "feet_yaw"):
        if k in got:
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (what, k)
            dev_angle = max(dev_angle, float(np.nanmax(np.abs(got[k].astype(D) - want[k]), initial=0.0)) / ANGLE_UNIT)
    dev_gait = 0.0
    if "gait" in got:
        assert np.array_equal(np.isnan(got["gait"]), np.isnan(want["gait"])), what
        dev_gait = float(np.nanmax(np.abs(got["gait"].astype(D) - want["gait"]), initial=0.0)) / EPS
    print(f"{what}: angles {dev_angle:.3f} x 2^-24 x 3 pi (bound {ANGLE_BOUND}), gait columns {dev_gait:.3f} x 2^-24 (bound {GAIT_BOUND})")
    assert dev_angle <= ANGLE_BOUND and dev_gait <= GAIT_BOUND, (what, dev_angle, dev_gait)
    if "term" in got:
        same(got["term"][:, EXACT_TERMS], want["term"][:, EXACT_TERMS], (what, "exact terms"))
        d = ANGLE_BOUND * ANGLE_UNIT
        bound, total = term_bounds(want["term"], want["feet_roll"], want["feet_pos"], mirror.cfg["scale"], d, d, GAIT_BOUND * EPS, forces)
        dev = np.abs(got["term"].astype(D) - want["term"])
        ok = np.isfinite(want["term"])
        assert np.array_equal(np.isnan(got["term"]), np.isnan(want["term"])), what
        assert (dev[ok] <= bound[ok]).all(), (what, np.argwhere(ok & (dev > bound)))
        if "total" in got:
            ok = np.isfinite(want["total"])
            assert np.array_equal(np.isnan(got["total"]), np.isnan(want["total"])), what
            assert (np.abs(got["total"].astype(D) - want["total"])[ok] <= total[ok]).all(), (what, "total")


def check_state(t, mirror, what):
    st = t.feet_state()
    for k in ("last_feet_pos", "gait_process"):
        same(st[k], mirror.state()[k], (what, k))


# ---- 1. terrain heights ------------------------------------------------------------------------------------------------------------------
def test_terrain_heights_are_the_fixtures_and_the_mirrors_bits(hip, world):
    g = golden()
    rng = np.random.default_rng(81)
    t, _, _ = setup(world, rng)
    hs, vs, border = g["terrain"].tolist()
    t.set_terrain(g["field"], hs, vs, int(border))
    ter = golden_terrain(g)
    h, outside = t.terrain_heights(g["t_points"])
    assert outside == 0
    same(h, g["t_heights"], "the fixture's points")
    same(h, fm.heights(ter, g["t_points"])[0], "the mirror")
    pts = g["s_edge_pos"].reshape(-1, 3)
    same(t.terrain_heights(pts)[0], g["s_edge_height"].reshape(-1), "the fixture's edge points")
    # device memory: a row stride of 13 (root states as they lie), the count added to what the caller zeroed, M = 1
    roots = g["s_root_states"].reshape(-1, 13).copy()
    roots[5, 0], roots[9, 1], roots[11, 0] = -0.31, 7.0, np.nan
    M = len(roots)
    d_pts, d_h = hip.DeviceBuffer.from_host(roots), hip.DeviceBuffer.from_host(np.full(M + G, SENTINEL, F))
    d_out = hip.DeviceBuffer.from_host(np.array([5], np.int32))
    t.terrain_heights_dev(d_pts, M, d_h, outside=d_out, stride=13)
    hip.check(hip.lib().gmr_stream_sync(None))
    raw = d_h.to_host(M + G, F)
    want, count = fm.heights(ter, roots)
    assert (raw[M:] == SENTINEL).all() and count == 3 and d_out.to_host(1, np.int32)[0] == 5 + 3
    same(raw[:M], want, "stride 13")
    assert np.isnan(want[11]) and np.isfinite(np.delete(want, 11)).all()
    keep = np.ones(M, bool)
    keep[[5, 9, 11]] = False
    same(raw[:M][keep], g["s_ground"].reshape(-1)[keep], "the fixture's ground")
    d_one = hip.DeviceBuffer.from_host(np.full(1 + G, SENTINEL, F))
    t.terrain_heights_dev(d_pts, 1, d_one, stride=2)
    hip.check(hip.lib().gmr_stream_sync(None))
    raw = d_one.to_host(1 + G, F)
    assert (raw[1:] == SENTINEL).all()
    same(raw[:1], want[:1], "M = 1")
    # clamping, on a field whose border rows and columns are distinct and not zero: points of any width on the host -- outside in x only,
    # in y only, the far corners, scattered --, every index clamped to the field with the weights as computed; then the plane
    field = rough_field(NX, NY)
    t.set_terrain(field, HS, VS, BORDER)
    ter = fm.terrain(field, HS, VS, BORDER)
    wide = rng.uniform(-0.6, 2.3, (101, 5)).astype(F)
    wide[:8, :2] = [[-0.35, 0.23], [X_HI + 0.04, 0.23], [0.27, -0.31], [0.27, Y_HI + 0.02], [-50.0, -50.0], [50.0, 50.0], [-50.0, 50.0], [50.0, -50.0]]
    h, outside = t.terrain_heights(wide)
    want, count = fm.heights(ter, wide)
    same(h, want, "clamped")
    assert outside == count > 20 and not (h[:8] == 0).any() and len(np.unique(h[:8])) == 8
    for k in range(8):
        assert h[k] == clamped_height(field, HS, VS, BORDER, wide[k, 0], wide[k, 1]), k
    assert h[4] == F(field[0, 0] * VS) and h[5] == F(field[-1, -1] * VS) and h[6] == F(field[0, -1] * VS) and h[7] == F(field[-1, 0] * VS)
    t.set_terrain(None)
    h, outside = t.terrain_heights(wide)
    assert outside == 0 and not h.any()


# ---- 2. five steps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,terrain,seed", [(4, True, 82), (1, True, 83), (8, True, 84), (4, False, 85)])
def test_five_steps_are_the_mirrors(hip, world, E, terrain, seed):
    """Largest deviations met on an MI355X: see ANGLE_BOUND, GAIT_BOUND and DESIGN.md section 6r."""
    rng = np.random.default_rng(seed)
    t, m, _ = setup(world, rng, E=E, terrain=terrain)
    before, pbefore = t.state(), t.proprio_state()
    contacts, flagged, swings = [], 0, 0
    for s in range(5):
        x = inputs(rng, m)
        got = run_dev(hip, t, x)
        want = mirror_step(m, x)
        check(got, want, m, (E, terrain, s))
        check_state(t, m, s)
        contacts.append(got["feet_contact"].mean())
        flagged += int((np.abs(want["feet_yaw"][:, 1] - want["feet_yaw"][:, 0]) > np.pi).sum())
        swings += int((got["term"][:, 7] > 0).sum())
        assert not got["gait"][2].any() and (got["done"] == 8).any() and (got["done"] == 0).any() and (got["term"][:, 0] > 0).any()
    assert 0.05 < np.mean(contacts) < 0.95 and flagged >= 3 and swings > 0
    after, pafter = t.state(), t.proprio_state()
    for k in STATE:
        same(before[k], after[k], k)
    for k in STATE6:
        same(pbefore[k], pafter[k], k)
    assert before["ignored"] == after["ignored"]


# ---- 3. absent inputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("absent", ["contact_forces", "gait_frequency", "episode_steps"])
def test_absent_inputs(hip, world, absent):
    rng = np.random.default_rng(86)
    t, m, _ = setup(world, rng)
    first = inputs(rng, m)
    run_dev(hip, t, first, want=("term",))
    mirror_step(m, first)                                      # last_feet_pos and the gait clock are not zero from here on
    x = inputs(rng, m)
    x["episode_steps"][:] = rng.integers(0, 3, N)
    x[absent] = None
    got = run_dev(hip, t, x)
    want = mirror_step(m, x)
    check(got, want, m, absent, forces=absent != "contact_forces")
    check_state(t, m, absent)
    if absent == "contact_forces":
        assert not got["term"][:, 0].any() and not got["done"].any()
        sc = m.cfg["scale"]
        assert sc[0] != 0 and (got["term"][:, 1] != 0).any()
    if absent == "gait_frequency":
        assert not got["gait"].any() and not got["term"][:, 7].any()
        same(t.feet_state()["gait_process"], m.state()["gait_process"], "the clock stands")
    if absent == "episode_steps":
        assert (got["term"][:, 1] != 0).sum() > N // 4           # no gate
    else:
        assert not got["term"][x["episode_steps"] <= 1, 1].any()


# ---- 4. the force threshold --------------------------------------------------------------------------------------------------------------
def test_forces_at_under_over_the_threshold_and_nan_and_the_done_word(hip, world):
    rng = np.random.default_rng(87)
    t, m, pm_ = setup(world, rng)
    x = inputs(rng, m)
    f = x["contact_forces"]
    f[:] = 0
    one = F(1.0)
    over, under = np.nextafter(one, F(2)), np.nextafter(one, F(0))
    f[0, 0] = (one, 0, 0)                                       # exactly 1: not above
    f[1, 3] = (0, over, 0)
    f[2, 10] = (0, 0, under)
    f[3, 0] = (np.nan, 5, 5)                                    # a NaN compares false
    f[4, 3] = (F(0.6), F(0.8), 0)                               # 0.36 + 0.64 in float32
    f[5, 0], f[5, 3], f[5, 10] = (2, 0, 0), (0, 2, 0), (0, 0, 2)
    f[6, 1], f[6, 2], f[6, 5], f[6, 7], f[6, 8] = (over, 0, 0), (one, 0, 0), (0, -3, 0), (np.inf, 0, 0), (under, 0, 0)
    f[7, 4], f[7, 6], f[7, 9] = (9, 9, 9), (9, 9, 9), (9, 9, 9)            # bodies on neither list
    got = run_dev(hip, t, x)
    want = mirror_step(m, x)
    check(got, want, m, "threshold")
    expect = np.zeros(N, np.int32)
    expect[[1, 5]] = 8
    expect[4] = 8 if fm.force_norm(f[4, 3]) > one else 0
    assert np.array_equal(got["done"], expect)
    collision = np.zeros(N, F)
    collision[6] = 3
    same(got["term"][:, 0], collision, "collision")
    # done | proprio's done is a mask reset_done takes as it lies
    px = proprio_inputs(rng)
    px["root_states"][:, 7:13] = 0
    px["root_states"][:, 2], px["ground"] = 0.6, None
    px["episode_steps"][:] = 3
    px["root_states"][8, 2], px["episode_steps"][9], px["episode_steps"][1] = 0.1, 40, 40
    pdone = t.proprio(**px, noise=False)["done"]
    word = got["done"] | pdone
    assert word[1] == 12 and word[5] == 8 and word[8] == 2 and word[9] == 4 and (word != 0).sum() == 4 + int(expect[4] != 0)
    d_done = hip.DeviceBuffer.from_host(word)
    before = t.state()
    t.reset_done_dev(done=d_done)
    hip.check(hip.lib().gmr_stream_sync(None))
    after = t.state()
    assert np.array_equal(after["draws"] != before["draws"], word != 0)
    check_state(t, m, "a reset leaves the feet state")


# ---- 5. ground into proprio --------------------------------------------------------------------------------------------------------------
def test_ground_goes_straight_into_proprio_dev(hip, world):
    rng = np.random.default_rng(88)
    (ta, ma, _), (tb, mb, _) = (setup(world, np.random.default_rng(880)) for _ in range(2))
    x = inputs(rng, ma)
    px = proprio_inputs(rng)
    px["root_states"][:, :3] = x["root_states"][:, :3]
    x["root_states"] = px["root_states"]
    keep = {}
    got = run_dev(hip, ta, x, want=("ground", "gait"), keep=keep)
    want = mirror_step(ma, x)
    same(got["ground"], want["ground"], "ground")
    assert len(np.unique(got["ground"])) > N // 2
    # on the device: the buffer feet_dev wrote, guard floats and all
    n = N
    _, counts = ta._proprio_counts()
    up = {k: None if a is None else hip.DeviceBuffer.from_host(a) for k, a in px.items() if k != "ground"}
    out = {k: hip.DeviceBuffer.from_host(np.full(n * counts[k] + G, SENTINEL, dtype=F)) for k in ("priv", "term", "done")}
    ta.proprio_dev(**up, ground=keep["ground"], noise=False, **out)
    hip.check(hip.lib().gmr_stream_sync(None))
    px["ground"] = want["ground"]
    host = tb.proprio(**px, noise=False)
    for k, b in out.items():
        raw = b.to_host(n * counts[k] + G, F)
        a = raw[:n * counts[k]]
        a = a.view(np.int32) if k == "done" else a.reshape(n, counts[k])
        same(a, host[k], k)
    assert (host["priv"][:, 3] != px["root_states"][:, 2]).any()


# ---- 6. outside the field, a NaN foot ----------------------------------------------------------------------------------------------------
def test_edge_points_outside_the_field_and_a_nan_foot(hip, world):
    rng = np.random.default_rng(89)
    t, m, _ = setup(world, rng)
    field = rough_field(NX, NY)                                # the border rows and columns distinct and not zero: a clamp elsewhere shows
    t.set_terrain(field, HS, VS, BORDER)
    m.ter = fm.terrain(field, HS, VS, BORDER)
    x = inputs(rng, m)
    st = x["body_state"]
    st[0, 4, :2] = (-0.29, 0.4)                                 # some edge points left of the field: outside in x only
    st[1, 9, :2] = (X_HI - 0.05, Y_HI - 0.02)                   # past its far corner
    st[12, 4, :2] = (0.6, Y_HI + 0.03)                          # outside in y only
    for e, b in ((0, 4), (1, 9), (12, 4)):                      # just above the clamped surface, so that the clamped heights decide the contact
        st[e, b, 2] = fm.heights(m.ter, st[e, b, :2][None])[0][0] + F(0.035)
    st[2, 4, :2] = (50.0, -50.0)
    st[3, 9, :2] = (1e30, 0.3)
    st[4, 4, 0] = np.nan
    st[5, 9, 2] = np.nan
    st[6, 4, 3:7] = np.nan
    st[7, 9, :3] = (np.inf, 0.2, 0.0)
    st[8, 4, 3:7] = 0                                           # a zero quaternion: atan2f(0, 0)
    x["root_states"][9, 0], x["root_states"][10, 1], x["root_states"][11, 3:7] = np.nan, -7.0, np.nan
    got = run_dev(hip, t, x)
    want = mirror_step(m, x)
    check(got, want, m, "outside", margins=False)
    check_state(t, m, "outside")
    assert got["feet_contact"][4, 0] == 0 and got["feet_contact"][6, 0] == 0 and got["feet_contact"][7, 1] == 0
    assert np.isnan(got["ground"][9]) and np.isfinite(got["ground"][10]) and np.isnan(got["term"][11, 5]) and np.isnan(got["feet_roll"][6, 0])
    assert got["feet_roll"][8, 0] == 0 and got["feet_yaw"][8, 0] == 0
    assert np.isnan(t.feet_state()["last_feet_pos"][4, 0, 0])


# ---- 7. one environment, empty lists -----------------------------------------------------------------------------------------------------
def test_one_environment_and_empty_body_lists(hip, world):
    rng = np.random.default_rng(90)
    t, m, _ = setup(world, rng, n=1, termination=(), penalized=())
    for s in range(2):
        x = inputs(rng, m, n=1)
        x["gait_frequency"][:] = 1.7
        x["contact_forces"][:] = 9.0
        got = run_dev(hip, t, x)
        check(got, mirror_step(m, x), m, ("one", s), margins=False)
        check_state(t, m, s)
        assert got["done"][0] == 0 and got["term"][0, 0] == 0 and got["gait"].any()


# ---- 8. streams --------------------------------------------------------------------------------------------------------------------------
def test_the_device_call_on_a_stream_of_its_own_gives_the_synchronous_bytes(hip, world):
    rng = np.random.default_rng(91)
    (ta, ma, _), (tb, _, _) = (setup(world, np.random.default_rng(910)) for _ in range(2))
    st = hip.Stream()
    for s in range(2):
        x = inputs(rng, ma)
        host = ta.feet({"body_pos": x["body_state"][:, :, 0:3], "body_rot": x["body_state"][:, :, 3:7]}, x["root_states"], x["contact_forces"],
                       x["episode_steps"], x["gait_frequency"])
        packed = ta.feet_state()
        got = run_dev(hip, tb, x, stream=st)
        for k in OUTPUTS:
            same(got[k], host[k], (s, k))
        other = tb.feet_state()
        for k in ("last_feet_pos", "gait_process"):
            same(packed[k], other[k], (s, k))
        assert packed["gait_process"].any()
    sa, sb = ta.state(), tb.state()
    for k in STATE:
        same(sa[k], sb[k], k)


# ---- 9. the synchronous calls with every optional array and with the mandatory ones alone ------------------------------------------------
def small_twins(hip, rng, n, nb):
    """two trackers alike on a library of 2 clips of 4 and 5 frames with 2 dofs, terrain and feet set (bodies 0 and 2 of nb) -> them, the field"""
    lib = device_library(hip, make_motions(rng, [4, 5], 2, 0))
    field = field_of(rng)
    twins = [tracker(lib, n, DT) for _ in range(2)]
    for t in twins:
        t.set_terrain(field, HS, VS, BORDER)
        t.set_feet((0, 2), edges_of(4), nb, termination_bodies=(1,), penalized_bodies=(0, 2), feet_distance_ref=0.2, swing_period=0.2, scales=SCALES)
    return twins, field


def test_synchronous_feet_with_every_optional_input_and_with_none(hip):
    """``feet`` on host arrays: the packed tensor (one copy of the hull of its two views) with every optional input against a twin given
    two separate body arrays and root_states alone, two steps each.  What does not read the absent inputs -- the feet's positions,
    angles and contacts, the ground, the terms from feet_vel_z to feet_distance, last_feet_pos -- is the same bits; collision, done
    and the gait columns of the twin are zero.  5 environments (no multiple of the 16-lane group), 3 bodies."""
    rng = np.random.default_rng(92)
    n, nb = 5, 3
    (ta, tb), field = small_twins(hip, rng, n, nb)
    ter = fm.terrain(field, HS, VS, BORDER)
    for s in range(2):
        state = rng.normal(0, 1, (n, nb, 13)).astype(F)
        state[:, :, 3:7] /= np.linalg.norm(state[:, :, 3:7], axis=-1, keepdims=True)
        state[:, :, 0], state[:, :, 1] = rng.uniform(0.05, X_HI - 0.2, (n, nb)), rng.uniform(0.05, Y_HI - 0.2, (n, nb))
        under, _ = fm.heights(ter, state[:, :, :2].reshape(-1, 2))
        state[:, :, 2] = under.reshape(n, nb) + rng.uniform(-0.03, 0.2, (n, nb)).astype(F)
        root = np.concatenate([state[:, 1, :7], rng.normal(0, 1, (n, 6)).astype(F)], axis=1)
        every = ta.feet({"body_state": state}, root, rng.normal(0, 2.0, (n, nb, 3)).astype(F), rng.integers(0, 4, n).astype(np.int32),
                        rng.uniform(1.0, 2.5, n).astype(F))
        alone = tb.feet({"body_pos": state[:, :, 0:3], "body_rot": state[:, :, 3:7]}, root)
        for k in ("feet_pos", "feet_roll", "feet_yaw", "feet_contact", "ground"):
            same(every[k], alone[k], (s, k))
        same(every["term"][:, 2:7], alone["term"][:, 2:7], (s, "term"))
        same(ta.feet_state()["last_feet_pos"], tb.feet_state()["last_feet_pos"], (s, "last_feet_pos"))
        assert not alone["done"].any() and not alone["gait"].any() and not alone["term"][:, 0].any()
        assert every["gait"].any() and every["term"][:, 0].any() and (every["term"][:, 2:6] != 0).any(axis=0).all() and every["ground"].any()
        assert np.array_equal(every["feet_pos"], state[:, (0, 2), 0:3])
    assert tb.feet_state()["gait_process"].tolist() == [0.0] * n and ta.feet_state()["gait_process"].all()


def test_synchronous_terrain_heights_with_and_without_the_counter(hip):
    """``terrain_heights`` on host arrays with its one optional array, the counter of the points outside, and without: the same heights"""
    rng = np.random.default_rng(93)
    n = 5
    (t, _), field = small_twins(hip, rng, n, 3)
    pts = rng.uniform(-0.6, 2.3, (n, 2)).astype(F)
    pts[0] = (-50.0, 0.3)
    h, outside = t.terrain_heights(pts)
    alone = np.full(n, SENTINEL, F)
    hip.check(hip.lib().gmr_motion_tracker_terrain_heights(t.handle, n, hip._ptr(pts), 2, hip._ptr(alone), None))
    want, count = fm.heights(fm.terrain(field, HS, VS, BORDER), pts)
    same(h, alone, "heights")
    same(h, want, "the mirror")
    assert outside == count >= 1
