"""The tracker's terrain and feet without a GPU: the exports, their ctypes signatures and the layout of the three structs
against the header, every argument check that must fire before the library is loaded, and the NumPy statement (tests/feet_mirror.py)
against the fixture generated from the reference's own ``Terrain.terrain_heights`` and ``quat_rotate`` (tests/golden/g_feet.npz): heights bit
for bit, contact flags, collision counts and termination flags exactly, rotations and terms within bounds derived here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header as abi  # noqa: E402
import feet_mirror as fm  # noqa: E402
from test_tracker_proprio_host import offline_tracker  # noqa: E402

FEET_SYMBOLS = ("gmr_motion_tracker_set_terrain", "gmr_motion_tracker_terrain_heights_dev", "gmr_motion_tracker_terrain_heights",
                "gmr_motion_tracker_set_feet", "gmr_motion_tracker_feet_dev", "gmr_motion_tracker_feet", "gmr_motion_tracker_feet_state")
F = np.float32
D = np.float64
EPS = 2.0 ** -24
ANGLE_UNIT = EPS * max(1.0, 3 * np.pi)          # the unit of an angle's deviation: a wrapped angle passes through values up to 3 pi
# Two float32 evaluations of one angle.  atan2f: the reference's is good to 1 ulp, the mirror's (float64, rounded once) to 0.5, of a value
# below 4 (ulp 2^-22): 1.5 x 2^-22.  Then every operation of rem and wrap rounds once in each evaluation, to half an ulp of its result: the
# + 2 pi of a negative remainder (below 8: 2 x 2^-22), the + pi (below 16: 2 x 2^-21), the - pi (below 4: 2 x 2^-23); fmod is exact.
BASE_YAW_HOST = 3.5 * 2.0 ** -22                # atan2f and the remainder: base_yaw
ANGLE_HOST = 8.5 * 2.0 ** -22                   # and the wrap: roll, yaw
TRIG_HOST = 2 * EPS                             # cosf / sinf of the same float32 argument: 1 ulp and 0.5 ulp of a value up to 1


def term_bounds(term, feet_roll, feet_pos, scale, d_angle, d_base_yaw, d_trig, forces=True):
    """Bounds on |term - term'| for the four terms that pass through angles, and on the total, between two evaluations whose feet angles
    differ by at most ``d_angle``, whose base yaw by ``d_base_yaw`` and whose cosf / sinf of one argument by ``d_trig``; everything else
    is the same float32 arithmetic on numbers that differ by that much, so every operation adds at most one ulp of its result between
    the two (a rounding to half an ulp in each).
      feet_roll      sum of roll_f^2: |a^2 - b^2| <= 2 |a| d + d^2 per foot, plus three roundings of the result
      feet_yaw_diff  x = wrap(yaw_1 - yaw_0): dx = 2 d and one ulp for each of the subtraction, the + pi and the - pi, all of values
                     below 16 (ulp 2^-20); x^2 as above
      feet_yaw_mean  x = wrap(base_yaw - m), m the mean of the yaws (deviation d, plus a rounding): the same dx with d_base_yaw + d
      feet_distance  |c dy - s dx|, clipped (1-Lipschitz): (|dy| + |dx|) (d_base_yaw + d_trig) -- the argument moves cos and sin by at most
                     its own deviation -- plus four roundings of products and sums of that size
      total          sum of |scale_k| bound_k plus one rounding per product and per sum of the total (16 ulp of the sum of |scale_k term_k|)"""
    term = np.asarray(term, dtype=D)
    b = np.zeros_like(term)
    roll = np.abs(np.asarray(feet_roll, dtype=D))
    b[:, 3] = (2 * roll * d_angle + d_angle ** 2).sum(axis=1) + 6 * EPS * term[:, 3]
    for k, dx in ((4, 2 * d_angle + 3 * 2.0 ** -20), (5, d_base_yaw + d_angle + 4 * 2.0 ** -20)):
        x = np.sqrt(term[:, k])
        b[:, k] = 2 * x * dx + dx ** 2 + 4 * EPS * term[:, k]
    p = np.asarray(feet_pos, dtype=D)
    reach = np.abs(p[:, 1, 1] - p[:, 0, 1]) + np.abs(p[:, 1, 0] - p[:, 0, 0])
    b[:, 6] = reach * (d_base_yaw + d_trig + 8 * EPS)
    sc = np.abs(np.asarray(scale, dtype=D))
    first = 0 if forces else 1
    total = (sc[first:] * b[:, first:]).sum(axis=1) + 32 * EPS * (sc[first:] * np.abs(term[:, first:])).sum(axis=1)
    return b, total


def test_the_library_exports_the_feet_entry_points_with_the_headers_signatures():
    from general_motion_retargeting_amd import _lib
    from general_motion_retargeting_amd import motion_tracker as mt
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmr_hip.h")).read()
    assert "N11: tracker feet" in hdr and hdr.index("N11: tracker feet") > hdr.index("N10: tracker proprioception")
    for sym in FEET_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        m = re.search(r"\bint " + sym + r"\(([^;]*)\);", hdr)
        assert m, sym
        params = abi.parameters(hdr, sym)
        res, args = _lib._SIGS[sym]
        assert res is C.c_int and args == params, (sym, params, args)
        # the comment in front of the prototype (a _dev call and its twin share one) cites the reference lines it replaces
        section = hdr[hdr.index("N11: tracker feet"):m.start()]
        comment = [c for c in re.findall(r"/\*.*?\*/", section, flags=re.S) if "\n" in c][-1]
        assert re.search(r"(t1|terrain)\.py:\d+", comment), sym

    for name, struct in (("gmr_feet_config_t", _lib.FeetConfig), ("gmr_feet_in_t", _lib.FeetIn), ("gmr_feet_out_t", _lib.FeetOut)):
        assert abi.fields(hdr, name) == [f for f, _ in struct._fields_], name
    P = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.FeetIn) == 4 * P and C.sizeof(_lib.FeetOut) == 9 * P
    assert _lib.FeetConfig.feet_body.offset == 4 * P and _lib.FeetConfig.force_threshold.offset == 4 * P + 24 and C.sizeof(_lib.FeetConfig) == 4 * P + 56
    for define, value in (("GMR_FEET_TERMS", len(_lib.FEET_TERMS)), ("GMR_FEET_MAX_EDGES", _lib.FEET_MAX_EDGES), ("GMR_FEET_MAX_BODIES", _lib.FEET_MAX_BODIES),
                          ("GMR_FEET_DONE_CONTACT", _lib.FEET_DONE_CONTACT)):
        assert abi.define(hdr, define) == value, define
    assert mt.FEET_TERMS == _lib.FEET_TERMS == fm.TERMS and mt.FEET_DONE_CONTACT == _lib.FEET_DONE_CONTACT == fm.DONE_CONTACT == 8
    assert (mt.FEET_MAX_EDGES, mt.FEET_MAX_BODIES) == (_lib.FEET_MAX_EDGES, _lib.FEET_MAX_BODIES)
    for name in ("set_terrain", "terrain_heights", "terrain_heights_dev", "set_feet", "feet", "feet_dev", "feet_state"):
        assert callable(getattr(mt.MotionTracker, name)), name
    from general_motion_retargeting_amd import build
    assert "gmr_tracker_feet.hip" in build.SOURCES


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_terrain_and_feet_arguments_are_refused_before_the_library_is_loaded(monkeypatch):
    from general_motion_retargeting_amd import _lib

    def no_device():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    N, nb = 8, 11
    t = offline_tracker(N)
    field = np.zeros((5, 4), np.int16)
    ok = dict(height_field=field, horizontal_scale=0.1, vertical_scale=0.005, border_pixels=2)
    for kw, exc, match in ((dict(horizontal_scale=0.0), ValueError, "horizontal_scale"), (dict(horizontal_scale=-0.1), ValueError, "horizontal_scale"),
                           (dict(horizontal_scale=np.nan), ValueError, "horizontal_scale"), (dict(horizontal_scale=np.inf), ValueError, "horizontal_scale"),
                           (dict(horizontal_scale=1e-60), ValueError, "horizontal_scale"), (dict(horizontal_scale=1e60), ValueError, "horizontal_scale"),
                           (dict(vertical_scale=0.0), ValueError, "vertical_scale"), (dict(vertical_scale=-1.0), ValueError, "vertical_scale"),
                           (dict(vertical_scale=np.inf), ValueError, "vertical_scale"), (dict(vertical_scale=np.nan), ValueError, "vertical_scale"),
                           (dict(border_pixels=-1), ValueError, "border_pixels"), (dict(border_pixels=1.5), ValueError, "border_pixels"),
                           (dict(height_field=field.astype(np.int32)), TypeError, "int16"), (dict(height_field=field.astype(F)), TypeError, "int16"),
                           (dict(height_field=field.tolist()), TypeError, "int16"), (dict(height_field=field[0]), ValueError, "dimensions"),
                           (dict(height_field=field[None]), ValueError, "dimensions"), (dict(height_field=field[:1]), ValueError, "shape"),
                           (dict(height_field=field[:, :1]), ValueError, "shape"), (dict(height_field=None, horizontal_scale=-1.0), ValueError, "horizontal_scale")):
        with pytest.raises(exc, match=match):
            t.set_terrain(**{**ok, **kw})
    got = t._terrain_setup(field[:, ::2], 0.1, 0.005, 3)
    assert got[0].flags.c_contiguous and got[0].shape == (5, 2) and got[1:] == (0.1, 0.005, 3)
    assert t._terrain_setup(None, 1.0, 1.0, 0) == (None, 1.0, 1.0, 0)
    # the heights
    for call, exc, match in ((lambda: t.terrain_heights(np.zeros((4, 1), F)), ValueError, "points: shape"), (lambda: t.terrain_heights(np.zeros(4, F)), ValueError, "points: shape"),
                             (lambda: t.terrain_heights_dev(1234, -1, 1234), ValueError, "n = -1"), (lambda: t.terrain_heights_dev(1234, 4, 1234, stride=1), ValueError, "stride"),
                             (lambda: t.terrain_heights_dev(None, 4, 1234), ValueError, "needed"), (lambda: t.terrain_heights_dev(1234, 4, None), ValueError, "needed"),
                             (lambda: t.terrain_heights_dev(np.zeros((4, 3), F), 4, 1234), TypeError, "device address")):
        with pytest.raises(exc, match=match):
            call()
    # feet not set: every call says so
    assert t.feet_state() is None
    bodies = {"body_pos": np.zeros((N, nb, 3), F), "body_rot": np.zeros((N, nb, 4), F)}
    roots = np.zeros((N, 13), F)
    for call in (lambda: t.feet(bodies, roots), lambda: t.feet_dev({"body_state": 1234}, 1234, feet_pos=1234)):
        with pytest.raises(ValueError, match="set_feet"):
            call()
    # the configuration
    edges = np.array([[0.1, 0.05, -0.03], [-0.1, -0.05, -0.03]], F)
    ok = dict(feet_bodies=(4, 9), edge_pos=edges, num_bodies=nb, feet_distance_ref=0.2, swing_period=0.2, termination_bodies=(0, 3), penalized_bodies=(1, 2))
    for kw, exc, match in ((dict(feet_bodies=(4,)), ValueError, "left and the right"), (dict(feet_bodies=(4, 9, 2)), ValueError, "left and the right"),
                           (dict(feet_bodies=(4, nb)), ValueError, "feet_bodies entries"), (dict(feet_bodies=(-1, 2)), ValueError, "feet_bodies entries"),
                           (dict(feet_bodies=(4.0, 9.0)), TypeError, "integers"), (dict(edge_pos=np.zeros((0, 3), F)), ValueError, "edge_pos has shape"),
                           (dict(edge_pos=np.zeros((9, 3), F)), ValueError, "edge_pos has shape"), (dict(edge_pos=np.zeros((2, 2), F)), ValueError, "edge_pos has shape"),
                           (dict(edge_pos=edges * np.nan), ValueError, "not finite"), (dict(num_bodies=0), ValueError, "num_bodies"), (dict(num_bodies=2.5), ValueError, "num_bodies"),
                           (dict(termination_bodies=(0, 0)), ValueError, "twice"), (dict(penalized_bodies=(1, nb)), ValueError, "penalized_bodies entries"),
                           (dict(penalized_bodies=list(range(65)), num_bodies=70), ValueError, "65 entries"), (dict(termination_bodies=(0.5,)), TypeError, "integers"),
                           (dict(force_threshold=np.nan), ValueError, "force_threshold"), (dict(contact_clearance=np.inf), ValueError, "contact_clearance"),
                           (dict(feet_distance_ref=1e60), ValueError, "feet_distance_ref"), (dict(swing_period=np.nan), ValueError, "swing_period"),
                           (dict(scales=np.ones(7, F)), ValueError, "scales has 7"), (dict(scales={"feet_slip": np.inf}), ValueError, "scales must be finite"),
                           (dict(scales={"torques": 1.0}), KeyError, "unknown terms")):
        with pytest.raises(exc, match=match):
            t.set_feet(**{**ok, **kw})
    assert getattr(t, "_feet", None) is None
    got = t._feet_setup(**{**ok, "force_threshold": 1.0, "contact_clearance": 0.01, "scales": {"feet_swing": -3.0}, "termination_bodies": ()})
    assert got["scales"].tolist() == [0] * 7 + [-3.0] and len(got["termination_bodies"]) == 0 and got["feet_bodies"].dtype == np.int32
    # shapes and dtypes of the step
    t._feet = (nb, 2)
    forces = np.zeros((N, nb, 3), F)
    for call, exc, match in ((lambda: t.feet(bodies["body_pos"], roots), TypeError, "bodies is"), (lambda: t.feet({"body_pos": bodies["body_pos"]}, roots), TypeError, "bodies is either"),
                             (lambda: t.feet({"body_state": np.zeros((N, nb, 12), F)}, roots), ValueError, "body_state: shape"),
                             (lambda: t.feet({**bodies, "body_rot": np.zeros((N, nb, 3), F)}, roots), ValueError, "body_rot: shape"),
                             (lambda: t.feet({**bodies, "body_pos": np.zeros((N, nb + 1, 3), F)}, roots), ValueError, "body_pos: shape"),
                             (lambda: t.feet(bodies, roots[:, :12]), ValueError, "root_states: shape"), (lambda: t.feet(bodies, None), ValueError, "root_states is needed"),
                             (lambda: t.feet(bodies, roots, contact_forces=forces[:, :10]), ValueError, "contact_forces: shape"),
                             (lambda: t.feet(bodies, roots, gait_frequency=np.zeros((N, 1), F)), ValueError, "gait_frequency: shape"),
                             (lambda: t.feet(bodies, roots, episode_steps=np.zeros(N, F)), TypeError, "integers"),
                             (lambda: t.feet(bodies, roots, episode_steps=np.zeros(N + 1, np.int32)), ValueError, "episode_steps: shape"),
                             (lambda: t.feet_dev({"body_state": 1234}, None), ValueError, "root_states is needed"),
                             (lambda: t.feet_dev({"body_state": 1234}, 1234, reward=1234), TypeError, "unknown outputs"),
                             (lambda: t.feet_dev({"body_state": roots}, 1234), TypeError, "device address"), (lambda: t.feet_dev({"body_state": 1234}, 1234, term=[1]), TypeError, "device address")):
        with pytest.raises(exc, match=match):
            call()
    assert not (t._links or t._preview or t._adaptive or t._anchors or t._control or t._proprio)


# ---- the mirror against the fixture from the reference's functions ------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(GOLDEN, "g_feet.npz"), allow_pickle=False)


def golden_terrain(g):
    hs, vs, border = g["terrain"].tolist()
    return fm.terrain(g["field"], hs, vs, int(border))


def golden_config(g, **kw):
    th, cl, ref, sw = g["scalars"].tolist()
    return fm.config(g["feet_body"], g["edge_pos"], g["s_body_pos"].shape[2], g["termination_body"], g["penalized_body"], th, cl, ref, sw, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def test_the_heights_of_the_mirror_are_the_references_bit_for_bit():
    g = golden()
    ter = golden_terrain(g)
    assert g["field"].dtype == np.int16 and g["field"].shape == (23, 17) and ter["border"] == 3
    h, outside = fm.heights(ter, g["t_points"])
    assert outside == 0 and np.array_equal(bits(h), bits(g["t_heights"])) and len(np.unique(h)) > 150
    # every edge point and every root of the scripted episode
    pts = g["s_edge_pos"].reshape(-1, 3)
    h, outside = fm.heights(ter, pts)
    assert outside == 0 and np.array_equal(bits(h), bits(g["s_edge_height"].reshape(-1)))
    h, outside = fm.heights(ter, g["s_root_states"].reshape(-1, 13))
    assert outside == 0 and np.array_equal(bits(h), bits(g["s_ground"].reshape(-1)))
    # the plane
    h, outside = fm.heights(None, g["t_points"])
    assert outside == 0 and not h.any() and h.dtype == F


def rough_field(nx=23, ny=17):
    """a field of distinct numbers, none of them zero, its border rows and columns included: a clamp to another element shows"""
    return (np.random.default_rng(5).permutation(nx * ny).reshape(nx, ny) * 5 - 900).astype(np.int16)


def clamped_height(field, hs, vs, b, px, py):
    """the issue's rule restated for one point: x in float32, the weights as computed, every index clamped to the field"""
    nx, ny = field.shape
    x, y = D(F(b) + F(px) / F(hs)), D(F(b) + F(py) / F(hs))
    x1, y1 = np.floor(x), np.floor(y)
    cx = lambda v: int(min(max(v, 0), nx - 1))      # noqa: E731
    cy = lambda v: int(min(max(v, 0), ny - 1))      # noqa: E731
    h = field.astype(D)
    s = ((x1 + 1 - x) * (y1 + 1 - y) * h[cx(x1), cy(y1)] + (x - x1) * (y1 + 1 - y) * h[cx(x1 + 1), cy(y1)]
         + (x1 + 1 - x) * (y - y1) * h[cx(x1), cy(y1 + 1)] + (x - x1) * (y - y1) * h[cx(x1 + 1), cy(y1 + 1)])
    return F(s * vs)


def test_clamping_the_outside_count_and_nan():
    g = golden()
    hs, vs, b = 0.1, 0.005, 3
    field = rough_field()
    nx, ny = field.shape
    assert len(np.unique(field)) == field.size
    ter = fm.terrain(field, hs, vs, b)
    x_hi, y_hi = (nx - 1 - b) * hs, (ny - 1 - b) * hs
    # inside: on a cell line the far weight is zero, and a corner of the last valid cell is the field's own number
    h, outside = fm.heights(ter, np.array([[0.5, 0.73], [(nx - 2 - b) * hs, (ny - 2 - b) * hs], [x_hi - 1e-4, 0.2]], F))
    assert outside == 0
    x0 = int(np.floor(D(F(b) + F(0.5) / F(hs))))
    assert D(F(b) + F(0.5) / F(hs)) == x0 == 8 and h[0] == clamped_height(field, hs, vs, b, 0.5, 0.73)
    y = D(F(b) + F(0.73) / F(hs))
    assert h[0] == F(((np.floor(y) + 1 - y) * field[8, 10] + (y - np.floor(y)) * field[8, 11]) * vs)          # nothing of row 9
    px, py = D(F(b) + F((nx - 2 - b) * hs) / F(hs)), D(F(b) + F((ny - 2 - b) * hs) / F(hs))
    if px == nx - 2 and py == ny - 2:
        assert h[1] == F(field[nx - 2, ny - 2] * vs)
    assert h[1] == clamped_height(field, hs, vs, b, (nx - 2 - b) * hs, (ny - 2 - b) * hs)
    # outside: in x only (left, right), in y only (below, above), the four far corners, a huge coordinate; then what is not finite
    pts = np.array([[-0.35, 0.23], [x_hi + 0.04, 0.23], [0.27, -0.31], [0.27, y_hi + 0.02], [-50.0, -50.0], [50.0, 50.0], [-50.0, 50.0], [50.0, -50.0],
                    [x_hi - 0.03, y_hi + 0.06], [1e30, 0.2], [np.nan, 0.2], [0.2, np.inf], [-np.inf, np.nan], [3e38, 0.2]], F)
    h, outside = fm.heights(ter, pts)
    assert outside == len(pts)
    assert np.isfinite(h[:10]).all() and np.isnan(h[10:]).all()             # F(3e38) / F(0.1) overflows float32: not finite either
    for k in range(10):
        assert h[k] == clamped_height(field, hs, vs, b, pts[k, 0], pts[k, 1]), k
    # what a clamp to the wrong element, a wrap or a zero outside would give differs
    assert h[4] == F(field[0, 0] * vs) and h[5] == F(field[nx - 1, ny - 1] * vs) and h[6] == F(field[0, ny - 1] * vs) and h[7] == F(field[nx - 1, 0] * vs)
    assert len({float(v) for v in h[:9]}) == 9 and not (h[:9] == 0).any()
    assert h[9] == 0                                                        # beyond 2^53 pixels x + 1 == x: both x weights as computed are zero
    wrapped = field[-1, 5]                                                  # the reference's silent wrap of x1 = -1
    assert h[0] != F(wrapped * vs) and field[0, 5] != wrapped
    ter = golden_terrain(g)
    # a NaN foot: no contact, NaN angles, and the rest of the row untouched by it
    N, nb = 3, 11
    m = fm.Feet(golden_config(g), ter, N, 0.02)
    bp, bq, rs = g["s_body_pos"][0][:N].copy(), g["s_body_rot"][0][:N].copy(), g["s_root_states"][0][:N].copy()
    bp[1, 4] = np.nan
    rs[2, 0] = np.nan
    out = m.step(bp, bq, rs, g["s_contact_forces"][0][:N])
    assert out["feet_contact"][1, 0] == 0 and np.isnan(out["feet_pos"][1, 0]).all() and np.isfinite(out["feet_roll"]).all()
    assert np.isnan(out["ground"][2]) and np.isfinite(out["ground"][:2]).all() and np.isnan(out["term"][1, 6]) and np.isfinite(out["term"][0]).all()
    assert np.isnan(m.last_feet_pos[1, 0]).all()


def test_the_rotation_of_the_mirror_is_the_references_within_the_6q_bound():
    g = golden()
    steps, N, _, E, _ = g["s_edge_pos"].shape
    worst, equal = 0.0, []
    for s in range(steps):
        fp, fq = g["s_body_pos"][s][:, g["feet_body"]], g["s_body_rot"][s][:, g["feet_body"]]
        for f in range(2):
            for k in range(E):
                v = np.tile(g["edge_pos"][k], (N, 1))
                got = (fp[:, f] + fm.rotate(fq[:, f], v)).astype(F)
                want = g["s_edge_pos"][s][:, f, k]
                # within 8 x 2^-24 max(1, |v|), the position added on both sides
                bound = 8 * EPS * max(1.0, float(np.linalg.norm(v[0].astype(D))))
                dev = np.abs(got.astype(D) - want)
                assert (dev <= bound).all(), (s, f, k)
                worst = max(worst, float((dev / (8 * EPS)).max()))
                equal.append(np.mean(got == want))
    print(f"edge points: largest deviation {worst:.3f} x 8 x 2^-24, {np.mean(equal) * 100:.1f} % bit-equal")


def test_the_mirror_follows_the_scripted_episode_of_the_fixture():
    """Exact: feet_pos, contact flags, collision counts, termination flags, the gait clock, feet_slip's gate, feet_swing.  The heights under the
    mirror's own edge points differ from the fixture's only through the rotation (8 x 2^-24) times the terrain's slope, far below the 7.8e-5
    the generator kept between every clearance and the threshold, so the flags are the reference's.  Bounded: the angles (ANGLE_HOST), the
    gait columns (TRIG_HOST) and the four angle terms (term_bounds); feet_slip and feet_vel_z are the same float32 operations on the same
    numbers in another order of summation at most: 4 ulp."""
    g = golden()
    steps, N, nb, _ = g["s_body_pos"].shape
    assert (steps, N, nb) == (40, 6, 11) and g["margins"][0] > 1e-5 and g["margins"][1] > 1e-3
    m = fm.Feet(golden_config(g), golden_terrain(g), N, float(g["dt"]))
    seen_done, flagged = set(), 0
    worst = {"angle": 0.0, "gait": 0.0}
    for s in range(steps):
        out = m.step(g["s_body_pos"][s], g["s_body_rot"][s], g["s_root_states"][s], g["s_contact_forces"][s], g["s_episode_steps"][s], g["s_gait_frequency"][s])
        assert m.margins["clearance"] > 1e-5 and m.margins["angle"] > 1e-3 - 1e-5, (s, m.margins)
        assert np.array_equal(bits(out["feet_pos"]), bits(g["s_feet_pos"][s])), s
        assert np.array_equal(out["feet_contact"], g["s_feet_contact"][s].astype(np.int32)), s
        assert np.array_equal(bits(out["ground"]), bits(g["s_ground"][s])), s
        assert np.array_equal(bits(m.gait_process), bits(g["s_gait_process"][s])), s
        assert np.array_equal(out["done"], np.where(g["s_done"][s], 8, 0)), s
        want = g["s_term"][s].astype(D)
        assert np.array_equal(out["term"][:, 0], g["s_term"][s][:, 0]) and np.array_equal(out["term"][:, 7], g["s_term"][s][:, 7]), s
        for k in (1, 2):
            assert (np.abs(out["term"][:, k].astype(D) - want[:, k]) <= 4 * EPS * np.abs(want[:, k])).all(), (s, k)
        for k in ("feet_roll", "feet_yaw"):
            dev = np.abs(out[k].astype(D) - g[f"s_{k}"][s])
            assert (dev <= ANGLE_HOST).all(), (s, k, dev.max() / ANGLE_UNIT)
            worst["angle"] = max(worst["angle"], float(dev.max()))
        dev = np.abs(out["gait"].astype(D) - g["s_gait"][s])
        assert (dev <= TRIG_HOST).all(), (s, dev.max() / EPS)
        worst["gait"] = max(worst["gait"], float(dev.max()))
        bound, _ = term_bounds(want, g["s_feet_roll"][s], g["s_feet_pos"][s], np.zeros(8), ANGLE_HOST, BASE_YAW_HOST, TRIG_HOST)
        dev = np.abs(out["term"].astype(D) - want)
        assert (dev[:, 3:7] <= bound[:, 3:7]).all(), (s, np.argwhere(dev[:, 3:7] > bound[:, 3:7]), dev[:, 3:7] / np.maximum(bound[:, 3:7], 1e-300))
        seen_done |= set(out["done"].tolist())
        flagged += int((np.abs(out["feet_yaw"][:, 1] - out["feet_yaw"][:, 0]) > np.pi).sum())
    print(f"angles: largest deviation {worst['angle'] / ANGLE_UNIT:.3f} x 2^-24 x 3 pi; gait columns: {worst['gait'] / EPS:.3f} x 2^-24")
    assert seen_done == {0, 8} and flagged >= 3
    assert np.array_equal(bits(m.last_feet_pos), bits(g["final_last_feet_pos"])) and np.array_equal(bits(m.gait_process), bits(g["final_gait_process"]))
    assert not g["s_gait"][:, 2].any() and (g["s_term"][:, 2, 7] == 0).all()                   # the standing environment: no gait columns, no swing
    # total: the weighted terms in rising order, a zero scale and an absent input left out
    scales = {"collision": -1.0, "feet_slip": -0.1, "feet_roll": -0.2, "feet_distance": -10.0, "feet_swing": 3.0}
    m2 = fm.Feet(golden_config(g, scales=scales), golden_terrain(g), N, float(g["dt"]))
    args = (g["s_body_pos"][0], g["s_body_rot"][0], g["s_root_states"][0])
    full = m2.step(*args, g["s_contact_forces"][0])
    sc = m2.cfg["scale"]
    want = np.zeros(N, F)
    for k in (0, 1, 3, 6, 7):
        want = want + sc[k] * full["term"][:, k]
    assert np.array_equal(bits(full["total"]), bits(want)) and (sc != 0).sum() == 5
    m3 = fm.Feet(m2.cfg, golden_terrain(g), N, float(g["dt"]))
    bare = m3.step(*args)
    want = np.zeros(N, F)
    for k in (1, 3, 6, 7):
        want = want + sc[k] * bare["term"][:, k]
    assert np.array_equal(bits(bare["total"]), bits(want)) and not bare["term"][:, 0].any() and not bare["done"].any() and not bare["gait"].any()
    assert not m3.gait_process.any() and np.array_equal(bare["term"][:, 1], full["term"][:, 1])      # no episode_steps: the gate is 1
