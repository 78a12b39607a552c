"""The tracker anchors without a GPU: the exports and their ctypes signatures against the header, every argument
check that must fire before a device is touched, and the properties of the float32 statement (tests/anchor_mirror.py) that the device
reproduces bit for bit -- identity, composition, the half-angle routine, and ``anchor_to_root`` landing on the root it was given."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header as abi  # noqa: E402
import anchor_mirror as am  # noqa: E402
from test_motion_body_state_host import _OfflineLibrary  # noqa: E402
from test_motion_library import _bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHOR_SYMBOLS = ("gmr_motion_tracker_enable_anchors", "gmr_motion_tracker_set_anchor_dev", "gmr_motion_tracker_set_anchor",
                  "gmr_motion_tracker_anchor_to_root_dev", "gmr_motion_tracker_anchor_to_root", "gmr_motion_tracker_anchor_state")
F = np.float32
U = 2.0 ** -24          # the unit roundoff of float32


def test_the_library_exports_the_anchor_entry_points_with_the_headers_signatures():
    from general_motion_retargeting_amd import _lib
    from general_motion_retargeting_amd import motion_tracker as mt
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmr_hip.h")).read()
    assert "N8: tracker anchors" in hdr
    for sym in ANCHOR_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        m = re.search(r"\bint " + sym + r"\(([^;]*)\);", hdr)
        assert m, sym
        params = abi.parameters(hdr, sym)
        res, args = _lib._SIGS[sym]
        assert res is C.c_int and args == params, (sym, params, args)
    for name, value in (("GMR_ANCHOR_YAW", _lib.ANCHOR_YAW), ("GMR_ANCHOR_Z", _lib.ANCHOR_Z)):
        assert int(re.search(r"#define " + name + r"\s+(\d+)", hdr).group(1)) == value == getattr(am, name[4:])
    for name in ("enable_anchors", "set_anchor", "set_anchor_dev", "anchor_to_root", "anchor_to_root_dev", "anchor_state"):
        assert callable(getattr(mt.MotionTracker, name)), name


def test_the_sources_of_the_other_kernels_do_not_see_the_changed_headers():
    csrc = os.path.join(ROOT, "general_motion_retargeting_amd", "csrc")
    for src in ("gmr_ik.hip", "gmr_ik_wide.hip", "gmr_fk.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert "gmr_tracker_dev.h" not in text and "gmr_handles.h" not in text, src
    from general_motion_retargeting_amd import build
    assert "gmr_tracker_anchor.hip" in build.SOURCES


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def offline_tracker(N=8, ang_vel="world"):
    from general_motion_retargeting_amd import MotionTracker
    t = MotionTracker.__new__(MotionTracker)
    t._init_state(_OfflineLibrary(5, ang_vel), N, 5)
    return t


def test_anchor_arguments_are_refused_before_anything_touches_a_device(monkeypatch):
    from general_motion_retargeting_amd import _lib

    def no_device():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    t = offline_tracker()
    pos, yaw = np.zeros((8, 3), F), np.zeros(8, F)
    quat = np.tile(F([0, 0, 0, 1]), (8, 1))
    bad_pos, bad_yaw = pos.copy(), yaw.copy()
    bad_pos[3, 1], bad_yaw[5] = np.inf, np.nan
    # shapes and values of set_anchor
    for kw, match in ((dict(pos=np.zeros((7, 3), F)), "pos has shape"), (dict(pos=np.zeros((8, 2), F)), "pos has shape"), (dict(yaw=np.zeros((8, 1), F)), "yaw has shape"),
                      (dict(pos=pos, env_ids=[1, 2]), "pos has shape"), (dict(yaw=yaw[:3], env_ids=[1, 2]), "yaw has shape"),
                      (dict(pos=bad_pos), "pos is not finite"), (dict(yaw=bad_yaw), "yaw is not finite"), (dict(pos=pos, yaw=np.full(8, np.inf, F)), "yaw is not finite")):
        with pytest.raises(ValueError, match=match):
            t.set_anchor(**kw)
    # shapes, masks and the list of anchor_to_root
    for args, kw, exc, match in (((pos[:7], quat), {}, ValueError, "root_pos has shape"), ((pos, quat[:, :3]), {}, ValueError, "root_quat has shape"),
                                 ((pos, quat), dict(mask=np.ones(7, bool)), ValueError, "mask: shape"), ((pos, quat), dict(mask=np.ones(8, F)), TypeError, "bool or integer"),
                                 ((pos[:3], quat[:3]), dict(env_ids=[1, 2, 1]), ValueError, "twice"), ((pos, quat), dict(env_ids=[1, 2]), ValueError, "root_pos has shape"),
                                 ((pos[:2], quat[:2]), dict(env_ids=[1, 2], mask=np.ones(8, bool)), ValueError, "mask: shape")):
        with pytest.raises(exc, match=match):
            t.anchor_to_root(*args, **kw)
    # a yaw on a library whose root_ang_vel cannot be rotated; a translation is fine as far as the checks go
    r = offline_tracker(ang_vel="reference")
    with pytest.raises(ValueError, match='ang_vel="world"'):
        r.set_anchor(yaw=yaw)
    with pytest.raises(ValueError, match='ang_vel="world"'):
        r.anchor_to_root(pos, quat)
    assert r._anchor_setup("set_anchor", pos, None, None)[0] == 8
    r._anchors = True
    with pytest.raises(ValueError, match='ang_vel="world"'):
        r.set_anchor_dev(yaw=1234)
    with pytest.raises(ValueError, match='ang_vel="world"'):
        r.anchor_to_root_dev(1234, 5678)
    # _dev calls without enabled anchors, and their list lengths
    assert t.anchor_state() is None
    with pytest.raises(ValueError, match="enable_anchors"):
        t.set_anchor_dev(pos=1234)
    with pytest.raises(ValueError, match="enable_anchors"):
        t.anchor_to_root_dev(1234, 5678)
    t._anchors = True
    with pytest.raises(ValueError, match="needs n"):
        t.set_anchor_dev(pos=1234, env_ids=99)
    with pytest.raises(ValueError, match="every environment"):
        t.anchor_to_root_dev(1234, 5678, n=7)
    with pytest.raises(ValueError, match="needed"):
        t.anchor_to_root_dev(None, 5678)
    with pytest.raises(TypeError, match="device address"):
        t.anchor_to_root_dev(pos, quat)
    assert not (t._links or t._preview or t._adaptive)


# ---- the float32 statement ---------------------------------------------------------------------------------------------------------
def random_anchor(rng, N):
    pos = rng.uniform(-10, 10, (N, 3)).astype(F)
    return pos, am.half_angle(rng.uniform(-np.pi, np.pi, N).astype(F))


def test_the_identity_anchor_returns_its_input():
    rng = np.random.default_rng(1)
    N = 500
    pos, yaw = np.zeros((N, 3), F), np.tile(F(am.IDENTITY_YAW), (N, 1))
    p, q = rng.uniform(-5, 5, (N, 4, 3)).astype(F), rng.normal(size=(N, 4, 4)).astype(F)
    p[0, 0], q[0, 0] = [-0.0, 0.0, -1.5], [0.0, -0.0, 0.0, 1.0]
    assert np.array_equal(am.apply_pos(pos, yaw, p), p) and np.array_equal(am.apply_vec(yaw, p), p) and np.array_equal(am.apply_quat(yaw, q), q)
    assert np.array_equal(_bits(am.half_angle(F(0.0))), _bits(F([0.0, 1.0])))


def test_half_angle_is_sine_and_cosine_to_float32():
    rng = np.random.default_rng(2)
    psi = np.concatenate([rng.uniform(-np.pi, np.pi, 20000), rng.uniform(-40.0, 40.0, 5000), [0.0, np.pi, -np.pi, np.pi / 2, 1e-30, 6.2831855]]).astype(F)
    zw = am.half_angle(psi).astype(np.float64)
    h = (psi * F(0.5)).astype(np.float64)
    dev = max(np.abs(zw[:, 0] - np.sin(h)).max(), np.abs(zw[:, 1] - np.cos(h)).max())
    print(f"half_angle: largest deviation from float64 sin / cos {dev / U:.2f} x 2^-24")
    assert dev <= 4 * U          # each polynomial is good to about an ulp of a number below 1; 4 x 2^-24 leaves room for the reduction
    assert np.abs(np.hypot(zw[:, 0], zw[:, 1]) - 1.0).max() <= 4 * U


def test_two_anchors_in_sequence_are_their_float64_composition():
    rng = np.random.default_rng(3)
    N = 4000
    (ta, ya), (tb, yb) = random_anchor(rng, N), random_anchor(rng, N)
    p, v = rng.uniform(-5, 5, (N, 3)).astype(F), rng.uniform(-3, 3, (N, 3)).astype(F)
    q = rng.normal(size=(N, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    tc, yc = am.compose(ta, ya, tb, yb)
    d = np.float64
    c, s = yc[:, 1] ** 2 - yc[:, 0] ** 2, 2 * yc[:, 0] * yc[:, 1]
    want_p = np.stack([c * p[:, 0].astype(d) - s * p[:, 1] + tc[:, 0], s * p[:, 0].astype(d) + c * p[:, 1] + tc[:, 1], p[:, 2].astype(d) + tc[:, 2]], axis=-1)
    want_v = np.stack([c * v[:, 0].astype(d) - s * v[:, 1], s * v[:, 0].astype(d) + c * v[:, 1], v[:, 2].astype(d)], axis=-1)
    z, w = yc[:, 0:1], yc[:, 1:2]
    qd = q.astype(d)
    want_q = np.concatenate([w * qd[:, 0:1] - z * qd[:, 1:2], w * qd[:, 1:2] + z * qd[:, 0:1], w * qd[:, 2:3] + z * qd[:, 3:4], w * qd[:, 3:4] - z * qd[:, 2:3]], axis=-1)
    got_p = am.apply_pos(tb, yb, am.apply_pos(ta, ya, p))
    got_v = am.apply_vec(yb, am.apply_vec(ya, v))
    got_q = am.apply_quat(yb, am.apply_quat(ya, q))
    size = np.abs(p[:, 0]) + np.abs(p[:, 1]) + np.abs(ta).sum(axis=1) + np.abs(tb).sum(axis=1)
    rel_p = np.abs(got_p - want_p).max(axis=1) / (1e-6 * size)
    rel_v = np.abs(got_v - want_v).max(axis=1) / (1e-6 * (np.abs(v[:, 0]) + np.abs(v[:, 1])))
    rel_q = np.abs(got_q - want_q).max(axis=1) / 1e-6
    print(f"composition: position {rel_p.max():.3f}, vector {rel_v.max():.3f}, quaternion {rel_q.max():.3f} of 1e-6 x (|x| + |y| + |t|)")
    assert rel_p.max() <= 1.0 and rel_v.max() <= 1.0 and rel_q.max() <= 1.0


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_anchor_to_root_lands_on_the_root_it_was_given(flags):
    rng = np.random.default_rng(4 + flags)
    N = 4000
    pos0, yaw0 = random_anchor(rng, N)
    rp, sp = rng.uniform(-5, 5, (N, 3)).astype(F), rng.uniform(-5, 5, (N, 3)).astype(F)
    rq, sq = rng.normal(size=(N, 4)), rng.normal(size=(N, 4))
    rq, sq = (rq / np.linalg.norm(rq, axis=1, keepdims=True)).astype(F), (sq / np.linalg.norm(sq, axis=1, keepdims=True)).astype(F)
    serve = rng.uniform(size=N) < 0.5
    sp[7, 1], sq[9, 0] = np.nan, np.inf
    serve[[7, 9]] = True
    pos, yaw = am.to_root(pos0, yaw0, rp, rq, sp, sq, flags, serve)
    kept = ~serve
    kept[[7, 9]] = True
    assert np.array_equal(_bits(pos[kept]), _bits(pos0[kept])) and np.array_equal(_bits(yaw[kept]), _bits(yaw0[kept]))
    on = ~kept
    if not flags & am.ANCHOR_YAW:
        assert np.array_equal(_bits(yaw), _bits(yaw0))
    if not flags & am.ANCHOR_Z:
        assert np.array_equal(_bits(pos[:, 2]), _bits(pos0[:, 2]))
    got_p, got_q = am.apply_pos(pos, yaw, rp), am.apply_quat(yaw, rq)
    size = np.abs(rp[:, 0]) + np.abs(rp[:, 1]) + np.abs(pos).sum(axis=1)
    bound = 1e-6 * size
    assert (np.abs(got_p[on, :2].astype(np.float64) - sp[on, :2]).max(axis=1) <= bound[on]).all()
    if flags & am.ANCHOR_Z:
        assert (np.abs(got_p[on, 2].astype(np.float64) - sp[on, 2]) <= bound[on]).all()
    if flags & am.ANCHOR_YAW:
        d = am.heading(got_q[on]) - am.heading(sq[on])
        d = np.abs((d + np.pi) % (2 * np.pi) - np.pi)
        print(f"flags {flags}: largest heading error {d.max():.3e} rad")
        assert d.max() <= 1e-6
