"""NumPy statement of the tracker anchors (general_motion_retargeting_amd/csrc/gmr_tracker_anchor.hip and the anchor helpers of
gmr_tracker_dev.h; include/gmr_hip.h section N8).  Everything here is float32 with one rounding per operation, in
the order the header states, so that the device reproduces the bits: the move itself (:func:`apply_pos`, :func:`apply_vec`,
:func:`apply_quat`, :func:`rot6`), the angle of ``set_anchor`` (:func:`half_angle`) and ``anchor_to_root`` (:func:`to_root`) from sampled
reference roots.  :func:`compose` is the float64 composition of two anchors that the property tests compare against."""
import numpy as np

F = np.float32
IDENTITY_POS, IDENTITY_YAW = (0.0, 0.0, 0.0), (0.0, 1.0)
ANCHOR_YAW, ANCHOR_Z = 1, 2


def _f(a):
    return np.asarray(a, dtype=F)


def cs(yaw_zw):
    """``c = w w - z z``, ``s = 2 z w`` of ``yaw_zw [..., 2]``"""
    z, w = _f(yaw_zw)[..., 0], _f(yaw_zw)[..., 1]
    return w * w - z * z, F(2.0) * z * w


def _lead(a, x):
    """``a [N]`` shaped to broadcast against the leading axes of ``x [N, ..., k]``"""
    return a.reshape(a.shape + (1,) * (x.ndim - 1 - a.ndim))


def apply_vec(yaw_zw, v):
    """``(c x - s y, s x + c y, z)`` for ``v [N, ..., 3]`` under the anchors ``yaw_zw [N, 2]``"""
    v = _f(v)
    c, s = (_lead(a, v) for a in cs(yaw_zw))
    x, y = v[..., 0], v[..., 1]
    return np.stack([c * x - s * y, s * x + c * y, v[..., 2]], axis=-1).astype(F)


def apply_pos(pos, yaw_zw, p):
    """``((c x - s y) + tx, (s x + c y) + ty, z + tz)`` for ``p [N, ..., 3]`` under the anchors ``pos [N, 3]``, ``yaw_zw [N, 2]``"""
    p, t = _f(p), _f(pos)
    c, s = (_lead(a, p) for a in cs(yaw_zw))
    x, y = p[..., 0], p[..., 1]
    return np.stack([(c * x - s * y) + _lead(t[:, 0], p), (s * x + c * y) + _lead(t[:, 1], p), p[..., 2] + _lead(t[:, 2], p)], axis=-1).astype(F)


def apply_quat(yaw_zw, q):
    """``(0, 0, z, w) * q`` for ``q [N, ..., 4]`` xyzw, not renormalised: ``(w qx - z qy, w qy + z qx, w qz + z qw, w qw - z qz)``"""
    q = _f(q)
    z, w = _lead(_f(yaw_zw)[..., 0], q), _lead(_f(yaw_zw)[..., 1], q)
    qx, qy, qz, qw = (q[..., i] for i in range(4))
    return np.stack([w * qx - z * qy, w * qy + z * qx, w * qz + z * qw, w * qw - z * qz], axis=-1).astype(F)


def rot6(q):
    """columns 0 and 1 of R(q) in float32, q xyzw as it is, in the order of the preview kernel"""
    q = _f(q)
    x, y, z, w = (q[..., i] for i in range(4))
    one, two = F(1.0), F(2.0)
    return np.stack([one - two * (y * y + z * z), two * (x * y + z * w), two * (x * z - y * w),
                     two * (x * y - z * w), one - two * (x * x + z * z), two * (y * z + x * w)], axis=-1).astype(F)


def half_angle(psi):
    """``(z, w) = (sin(psi / 2), cos(psi / 2))`` as ``anchor_half_angle`` computes them: ``h = psi / 2`` in float32, reduced in float64 by
    ``k = floor(h 2/pi + 1/2)`` quarter turns, the two single-precision polynomials in float32, the quadrant ``k mod 4``"""
    h = _f(psi) * F(0.5)
    hd = h.astype(np.float64)
    kd = np.floor(hd * 0.63661977236758134308 + 0.5)
    r = (hd - kd * 1.57079632679489661923).astype(F)
    quad = (kd - 4.0 * np.floor(kd * 0.25)).astype(np.int64)
    r2 = r * r
    sn = ((F(-1.9515295891e-4) * r2 + F(8.3321608736e-3)) * r2 - F(1.6666654611e-1)) * r2 * r + r
    cn = ((F(2.443315711809948e-5) * r2 - F(1.388731625493765e-3)) * r2 + F(4.166664568298827e-2)) * r2 * r2 - F(0.5) * r2 + F(1.0)
    z = np.choose(quad, [sn, cn, -sn, -cn])
    w = np.choose(quad, [cn, -sn, -cn, sn])
    return np.stack([z, w], axis=-1).astype(F)


def yaw_of(qz, qw):
    """``normalize(0, 0, qz, qw)`` in float32 -> ``(z, w)``, the identity where both are zero: ``yaw_of_exact`` of gmr_tracker_dev.h,
    whose square root and divisions are correctly rounded as NumPy's are"""
    qz, qw = _f(qz), _f(qw)
    n2 = qz * qz + qw * qw
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.sqrt(n2)
        return np.where(n2 != 0, qz / n, F(0)).astype(F), np.where(n2 != 0, qw / n, F(1)).astype(F)


def to_root(pos, yaw_zw, ref_pos, ref_rot, root_pos, root_quat, flags, serve):
    """``anchor_to_root``: the new ``(pos [N,3], yaw_zw [N,2])`` from the sampled reference roots ``ref_pos / ref_rot`` (float32, the
    sampler's rows) and the given roots, for the environments where ``serve`` is set; the others keep theirs.  An environment whose
    given root is not finite is kept too."""
    pos, yaw_zw = _f(pos).copy(), _f(yaw_zw).copy()
    rp, rq, sp, sq = _f(ref_pos), _f(ref_rot), _f(root_pos), _f(root_quat)
    serve = np.asarray(serve, dtype=bool) & np.isfinite(sp).all(axis=1) & np.isfinite(sq).all(axis=1)
    z, w = yaw_zw[:, 0], yaw_zw[:, 1]
    if flags & ANCHOR_YAW:
        zr, wr = yaw_of(rq[:, 2], rq[:, 3])
        zs, ws = yaw_of(sq[:, 2], sq[:, 3])
        z, w = yaw_of(zs * wr - ws * zr, ws * wr + zs * zr)
    c, s = w * w - z * z, F(2.0) * z * w
    tx = sp[:, 0] - (c * rp[:, 0] - s * rp[:, 1])
    ty = sp[:, 1] - (s * rp[:, 0] + c * rp[:, 1])
    tz = sp[:, 2] - rp[:, 2] if flags & ANCHOR_Z else pos[:, 2]
    new_pos, new_yaw = np.stack([tx, ty, tz], axis=-1).astype(F), np.stack([z, w], axis=-1).astype(F)
    pos[serve], yaw_zw[serve] = new_pos[serve], new_yaw[serve]
    return pos, yaw_zw


def compose(pos_a, yaw_a, pos_b, yaw_b):
    """the anchor "a, then b" in float64: yaw ``q_b q_a``, translation ``Rz(b) t_a + t_b``"""
    ta, tb = np.asarray(pos_a, dtype=np.float64), np.asarray(pos_b, dtype=np.float64)
    za, wa = np.asarray(yaw_a, dtype=np.float64)[..., 0], np.asarray(yaw_a, dtype=np.float64)[..., 1]
    zb, wb = np.asarray(yaw_b, dtype=np.float64)[..., 0], np.asarray(yaw_b, dtype=np.float64)[..., 1]
    c, s = wb * wb - zb * zb, 2.0 * zb * wb
    t = np.stack([c * ta[..., 0] - s * ta[..., 1] + tb[..., 0], s * ta[..., 0] + c * ta[..., 1] + tb[..., 1], ta[..., 2] + tb[..., 2]], axis=-1)
    return t, np.stack([wb * za + zb * wa, wb * wa - zb * za], axis=-1)


def heading(q):
    """the yaw angle of ``q [..., 4]`` xyzw in float64: the angle of ``yaw_of``'s quaternion, in (-pi, pi]"""
    q = np.asarray(q, dtype=np.float64)
    return np.arctan2(2.0 * q[..., 2] * q[..., 3], q[..., 3] ** 2 - q[..., 2] ** 2)


__all__ = ["apply_pos", "apply_vec", "apply_quat", "rot6", "half_angle", "yaw_of", "to_root", "compose", "heading", "cs"]
