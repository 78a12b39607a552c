"""NumPy mirror of ``gmr_motion_body_state`` (csrc/gmr_body_state.hip): the specification of DESIGN.md section 6j in float64.
The sampled state comes from tests/motion_mirror.py, the tree arrays from ``KinematicsModel``; the walk is the recursion

    p_b = p_p + R_p t_b        R_b = R_p r_b joint(a_b, theta_b)
    v_b = v_p + w_p x (p_b - p_p)        w_b = w_p + (R_b a_b) dtheta_b        (w_b = w_p for a body without a hinge)

with body 0 carrying the sampled root state."""
import numpy as np


def tree_of(km):
    """the arrays of the walk from a ``KinematicsModel``: parent, local translation, local rotation (xyzw, normalised here as a
    rotation), normalised hinge axis, dof of the body or -1"""
    t = km._tree
    axis = np.asarray(t["axis"], dtype=np.float64)
    axis = axis / np.maximum(np.linalg.norm(axis, axis=1, keepdims=True), 1e-9)
    return {"parent": np.asarray(t["parent"], dtype=np.int64), "t": np.asarray(t["local_translation"], dtype=np.float32).astype(np.float64),
            "r": np.asarray(t["local_rotation"], dtype=np.float32).astype(np.float64), "axis": axis,
            "dof_idx": np.asarray(t["dof_idx"], dtype=np.int64), "names": [str(x) for x in t["body_names"]]}


def tree_of_dict(tree):
    """the same arrays from the dict ``_lib.FkHandle`` takes (tests/fk_trees.py): the local rotations stay un-normalised, as the
    walk and the device take them"""
    axis = np.asarray(tree["axis"], dtype=np.float64)
    axis = axis / np.maximum(np.linalg.norm(axis, axis=1, keepdims=True), 1e-9)
    nb = len(tree["parent"])
    return {"parent": np.asarray(tree["parent"], dtype=np.int64), "t": np.asarray(tree["local_translation"], dtype=np.float32).astype(np.float64),
            "r": np.asarray(tree["local_rotation"], dtype=np.float32).astype(np.float64), "axis": axis,
            "dof_idx": np.asarray(tree["dof_idx"], dtype=np.int64), "names": [f"b{k}" for k in range(nb)]}


def qmul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0)
    bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def qrot(q, v):
    """the quat_rotate of the reference (torch_utils.py:65-75): exact for a unit q, and what the walk does with the un-normalised
    product of un-normalised local rotations.  Sums in the kernel's order (qrot_xyzw of csrc/gmr_fk_walk.h)."""
    w, u = q[..., 3:4], q[..., :3]
    d = (u[..., 0:1] * v[..., 0:1] + u[..., 1:2] * v[..., 1:2]) + u[..., 2:3] * v[..., 2:3]
    return v * (2.0 * w * w - 1.0) + np.cross(u, v) * w * 2.0 + u * d * 2.0


def walk(tree, root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, half_f32=True, dtype=np.float64):
    """arrays [N, ...] -> body_pos [N, nb, 3], body_rot [N, nb, 4] xyzw, body_vel, body_ang_vel [N, nb, 3].  ``half_f32``: the
    half angle of a joint is the float32 value the device takes the sine of; off for an exact walk.  ``dtype``: float64 is the
    specification; float32 evaluates the same recursion with one rounding per operation and the terms in the kernel's order
    (the joint quaternion, as there, in float64 from the float32 sine and cosine, normalised, rounded once) -- what a float32
    walk costs against the specification, with libm's sine and cosine where the device has its own"""
    dtype = np.dtype(dtype)
    f = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)   # noqa: E731
    root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel = map(f, (root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel))
    N, nb = len(root_pos), len(tree["parent"])
    p, q = np.zeros((N, nb, 3), dtype), np.zeros((N, nb, 4), dtype)
    v, w = np.zeros((N, nb, 3), dtype), np.zeros((N, nb, 3), dtype)
    p[:, 0], q[:, 0], v[:, 0], w[:, 0] = root_pos, root_rot, root_vel, root_ang_vel
    for b in range(1, nb):
        pa, d = int(tree["parent"][b]), int(tree["dof_idx"][b])
        off = qrot(q[:, pa], np.broadcast_to(tree["t"][b].astype(dtype), (N, 3)))
        p[:, b] = p[:, pa] + off
        lr = np.broadcast_to(tree["r"][b].astype(dtype), (N, 4))
        if d >= 0:
            if dtype == np.float32:
                half = dof_pos[:, d] / np.float32(2.0)
                sn, cs = np.sin(half).astype(np.float64), np.cos(half).astype(np.float64)
                jr = np.concatenate([tree["axis"][b] * sn[:, None], cs[:, None]], axis=1)
                jr = (jr / np.linalg.norm(jr, axis=1, keepdims=True)).astype(dtype)
            else:
                half = (dof_pos[:, d].astype(np.float32).astype(np.float64) if half_f32 else dof_pos[:, d]) / 2.0
                jr = np.concatenate([tree["axis"][b] * np.sin(half)[:, None], np.cos(half)[:, None]], axis=1)
            lr = qmul(lr, jr)
        q[:, b] = qmul(q[:, pa], lr)
        v[:, b] = v[:, pa] + np.cross(w[:, pa], off)
        w[:, b] = w[:, pa]
        if d >= 0:
            w[:, b] = w[:, pa] + qrot(q[:, b], np.broadcast_to(tree["axis"][b].astype(dtype), (N, 3))) * dof_vel[:, d:d + 1]
    return p, q, v, w


def body_state(library, tree, clip, time, loop=True, bodies=None):
    """``library``: a ``motion_mirror.Library`` in world mode.  The sampler's dict plus the four body arrays (float64; NaN rows for a
    bad query), rows in the order of ``bodies`` (indices; ``None``: all)."""
    out = library.sample(clip, time, loop)
    ok = out["status"] == 0
    z = lambda k: np.where(ok[:, None], out[k], 0.0)   # noqa: E731
    rot = np.where(ok[:, None], out["root_rot"], np.array([0.0, 0.0, 0.0, 1.0]))
    res = walk(tree, z("root_pos"), rot, z("root_vel"), z("root_ang_vel"), z("dof_pos"), z("dof_vel"))
    sel = np.arange(len(tree["parent"])) if bodies is None else np.asarray(bodies, dtype=np.int64)
    for k, a in zip(("body_pos", "body_rot", "body_vel", "body_ang_vel"), res):
        out[k] = np.where(ok[:, None, None], a[:, sel], np.nan)
    return out
