"""NumPy mirror of the tracker's preview (general_motion_retargeting_amd/csrc/gmr_tracker_preview.hip): the semantics of DESIGN.md
section 6m, independently of the kernel.  The clocks are ``tracker_mirror.Tracker``'s, the sampled rows ``motion_mirror.Library.sample``
at ``(clip, float64(time) + float64(offset))``: float32, the bits the device must reproduce in the raw frame.  The anchored frames
are float64 formulas on whatever raw rows they are handed (:func:`transform`), so that a device test can apply them to the device's
own raw rows."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import links_mirror as lm  # noqa: E402
import tracker_mirror as tm  # noqa: E402

F = np.float32
BLOCKS = ("root_pos", "root_quat", "root_rot6", "root_vel", "root_ang_vel", "dof_pos", "dof_vel", "body_pos")      # row order
BITS = {b: 1 << i for i, b in enumerate(BLOCKS)}
FRAMES = ("raw", "reference", "sim")
ROOT = ("root_pos", "root_quat", "root_rot6", "root_vel", "root_ang_vel")


def layout(blocks, R, nsel=0):
    """``{block: slice, ..., "row_width": D}``: the selected blocks in the fixed order, one that is not selected takes no room"""
    width = {"root_pos": 3, "root_quat": 4, "root_rot6": 6, "root_vel": 3, "root_ang_vel": 3, "dof_pos": R, "dof_vel": R, "body_pos": 3 * nsel}
    out, at = {}, 0
    for b in BLOCKS:
        if b in blocks:
            out[b] = slice(at, at + width[b])
            at += width[b]
    out["row_width"] = at
    return out


def query_times(time, offsets):
    """tq [N, K] = (double)time[e] + (double)offset[k], clocks and offsets float32"""
    return np.asarray(time, dtype=F).astype(np.float64)[:, None] + np.asarray(offsets, dtype=F).astype(np.float64)[None, :]


def valid_mask(lib, clip, time, offsets):
    """``i32 [N, K]``: 1 iff 0 <= tq <= duration - 1 / fps of the environment's clip in float64; 0 for a bad assignment"""
    clip = np.asarray(clip, dtype=np.int64)
    tq = query_times(time, offsets)
    ok = (clip >= 0) & (clip < len(lib.fps)) & np.isfinite(np.asarray(time, dtype=F))
    c = np.where(ok, clip, 0)
    T = lib.seg[c + 1] - lib.seg[c]
    ok &= T >= 1
    fps = lib.fps[c]
    last = T / fps - 1.0 / fps
    with np.errstate(invalid="ignore"):
        return (ok[:, None] & (tq >= 0.0) & (tq <= last[:, None])).astype(np.int32)


def rot6(q):
    """columns 0 and 1 of R(q), q xyzw as it is (not renormalised), col0 then col1"""
    x, y, z, w = (q[..., i] for i in range(4))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w),
                     2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w)], axis=-1)


def qrot(q, v):
    """R(q) v = v + w t + u x t, t = 2 (u x v)"""
    u, w = q[..., :3], q[..., 3:4]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def transform(raw, anchor_pos, anchor_quat):
    """The anchored frame in float64.  ``raw``: any of ``root_pos [..., 3]``, ``root_quat [..., 4]``, ``root_vel``, ``root_ang_vel`` and
    ``body_pos [..., nsel, 3]`` (root-local, as stored; needs ``root_pos`` and ``root_quat`` beside it) with leading axes ``[N, K]``;
    the anchor ``[N, 3]``, ``[N, 4]`` xyzw.  Returns the blocks of the table, ``root_rot6`` included when ``root_quat`` is given."""
    d = np.float64
    z, w = lm.yaw_quat(np.asarray(anchor_quat, dtype=d))
    c, s = (w * w - z * z)[:, None], (2.0 * z * w)[:, None]
    pa = np.asarray(anchor_pos, dtype=d)[:, None, :]

    def rz(a):
        cc, ss = (c, s) if a.ndim == 3 else (c[..., None], s[..., None])
        return np.stack([cc * a[..., 0] + ss * a[..., 1], cc * a[..., 1] - ss * a[..., 0], a[..., 2]], axis=-1)

    out = {}
    if "root_pos" in raw:
        out["root_pos"] = rz(np.asarray(raw["root_pos"], dtype=d) - pa)
    if "root_quat" in raw:
        q = np.asarray(raw["root_quat"], dtype=d)
        zz, ww = z[:, None], w[:, None]
        out["root_quat"] = np.stack([ww * q[..., 0] + zz * q[..., 1], ww * q[..., 1] - zz * q[..., 0], ww * q[..., 2] - zz * q[..., 3],
                                     ww * q[..., 3] + zz * q[..., 2]], axis=-1)
        out["root_rot6"] = rot6(out["root_quat"])
    for k in ("root_vel", "root_ang_vel"):
        if k in raw:
            out[k] = rz(np.asarray(raw[k], dtype=d))
    if "body_pos" in raw:
        p, q = np.asarray(raw["root_pos"], dtype=d)[..., None, :], np.asarray(raw["root_quat"], dtype=d)[..., None, :]
        out["body_pos"] = rz(p + qrot(q, np.asarray(raw["body_pos"], dtype=d)) - pa[..., None, :])
    return out


def raw_rows(tracker, offsets, bodies=None):
    """the sampled rows per (environment, offset) as ``[N, K, ...]`` float32 arrays -- ``root_pos, root_quat, root_vel, root_ang_vel``,
    ``dof_pos / dof_vel [N, K, R]`` through the tracker's dof map, ``body_pos [N, K, nsel, 3]`` -- plus ``status [N]``"""
    N, K = tracker.N, len(offsets)
    tq = query_times(tracker.time, offsets)
    with np.errstate(invalid="ignore"):
        s = tracker.lib.sample(np.repeat(tracker.clip, K), tq.reshape(-1), tracker.loop, local_body_pos=bodies is not None)
    ok = (s["status"] == 0)[:, None]
    on = tracker.map >= 0
    col = np.where(on, tracker.map, 0)
    rows = {"root_pos": s["root_pos"], "root_quat": s["root_rot"], "root_vel": s["root_vel"], "root_ang_vel": s["root_ang_vel"],
            "dof_pos": np.where(ok, np.where(on, s["dof_pos"][:, col], tracker.default), F(np.nan)).astype(F),
            "dof_vel": np.where(ok, np.where(on, s["dof_vel"][:, col], F(0)), F(np.nan)).astype(F)}
    if bodies is not None:
        rows["body_pos"] = s["local_body_pos"][:, np.asarray(bodies, dtype=np.int64)]
    rows = {k: a.reshape((N, K) + a.shape[1:]) for k, a in rows.items()}
    rows["status"] = s["status"].reshape(N, K)[:, 0].copy()
    return rows


def preview(tracker, offsets, blocks, frame="raw", bodies=None, sim=None):
    """``{"obs" [N, K, D], "valid" i32 [N, K], "status" i32 [N], "layout"}`` of a ``tracker_mirror.Tracker`` at its current clocks;
    ``obs`` is float32 (the sampler's bits) in the raw frame and float64 in the anchored ones.  Nothing of the tracker is written."""
    if frame not in FRAMES:
        raise ValueError(frame)
    offsets = np.asarray(offsets, dtype=F).reshape(-1)
    N, K = tracker.N, len(offsets)
    rows = raw_rows(tracker, offsets, bodies if "body_pos" in blocks else None)
    if frame == "raw":
        blocks_out = dict(rows, root_rot6=rot6(rows["root_quat"].astype(np.float64)))
    else:
        if frame == "reference":
            a = raw_rows(tracker, [0.0])
            anchor = a["root_pos"][:, 0], a["root_quat"][:, 0]
        else:
            anchor = np.asarray(sim["base_pos"], dtype=F), np.asarray(sim["base_quat"], dtype=F)
        with np.errstate(invalid="ignore"):
            blocks_out = transform({k: rows[k] for k in ("root_pos", "root_quat", "root_vel", "root_ang_vel", "body_pos") if k in rows}, *anchor)
        blocks_out["dof_pos"], blocks_out["dof_vel"] = rows["dof_pos"], rows["dof_vel"]
    lay = layout(blocks, len(tracker.map), 0 if bodies is None else len(bodies))
    obs = np.empty((N, K, lay["row_width"]), dtype=F if frame == "raw" and "root_rot6" not in blocks else np.float64)
    for b in BLOCKS:
        if b in blocks:
            obs[:, :, lay[b]] = np.asarray(blocks_out[b]).reshape(N, K, -1)
    bad = rows["status"] != 0
    obs[bad] = np.nan
    return {"obs": obs, "valid": valid_mask(tracker.lib, tracker.clip, tracker.time, offsets), "status": rows["status"], "layout": lay}


__all__ = ["preview", "transform", "layout", "valid_mask", "query_times", "raw_rows", "rot6", "qrot", "tm", "lm"]
