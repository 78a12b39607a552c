"""NumPy mirror of the motion library (general_motion_retargeting_amd/csrc/gmr_motion.hip): the semantics of DESIGN.md section 6h
written out once more, independently of the kernels, so that the GPU tests have something to be bit-equal to and the host
tests can pin the semantics against the fixture generated from the reference loader (tests/golden/g_motion.npz).

float32 where the reference computes in float32 (one rounding per operation), float64 where it goes through scipy."""
import numpy as np

F = np.float32


def rotvec(q_xyzw):
    """Shortest-arc log of quaternions ``[n, 4]`` (scalar last), float64, normalising first as scipy's from_quat does."""
    q = np.asarray(q_xyzw, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    q = np.where(q[:, 3:4] < 0, -q, q)
    v, w = q[:, :3], q[:, 3]
    n = np.linalg.norm(v, axis=1)
    angle = 2.0 * np.arctan2(n, w)
    small = n < 1e-6
    scale = np.where(small, 2.0 / np.where(small, w, 1.0), angle / np.where(small, 1.0, n))
    return v * scale[:, None]


def qmul_xyzw(a, b):
    ax, ay, az, aw = a.T
    bx, by, bz, bw = b.T
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], axis=1)


def derivatives(root_pos, root_rot, dof_pos, fps, ang_vel="world"):
    """One clip: float32 arrays in, (root_vel, root_ang_vel, dof_vel) float32 out."""
    T = len(root_pos)
    dt = 1.0 / fps
    rv, dv, av = np.zeros_like(root_pos), np.zeros_like(dof_pos), np.zeros_like(root_pos)
    if T < 2:
        return rv, av, dv
    rv[1:] = (root_pos[1:] - root_pos[:-1]) / F(dt)
    dv[1:] = (dof_pos[1:] - dof_pos[:-1]) / F(dt)
    q = root_rot.astype(np.float64)
    if ang_vel == "reference":
        q = q[:, [3, 0, 1, 2]]            # the reorder of motion_loader.py:131-132, then read scalar-last all the same
    elif ang_vel != "world":
        raise ValueError(ang_vel)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    inv = q[:-1] * np.array([-1.0, -1.0, -1.0, 1.0])
    av[1:] = (rotvec(qmul_xyzw(q[1:], inv)) / dt).astype(F)
    rv[0], dv[0], av[0] = rv[1], dv[1], av[1]
    return rv, av, dv


def stats(root_pos, dof_pos):
    """[4][3 + ndof] float32: mean, unbiased std, min, max, accumulated in float64.  An empty clip has no statistics: NaN in all
    four rows."""
    x = np.concatenate([root_pos, dof_pos], axis=1).astype(np.float64)
    if len(x) == 0:
        return np.full((4, x.shape[1]), np.nan, dtype=F)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = x.std(axis=0, ddof=1) if len(x) > 1 else np.full(x.shape[1], np.nan)
    return np.stack([x.mean(axis=0), std, x.min(axis=0), x.max(axis=0)]).astype(F)


class Library:
    """Many clips, clip-contiguous; ``motions`` = list of dicts with float32/float64 ``root_pos, root_rot (xyzw), dof_pos``,
    optional ``local_body_pos`` and ``fps``."""

    def __init__(self, motions, ang_vel="world"):
        self.fps = np.array([float(m["fps"]) for m in motions])
        lens = [len(m["root_pos"]) for m in motions]
        self.seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        cat = lambda k: np.concatenate([np.asarray(m[k], dtype=np.float64).astype(F) for m in motions])   # noqa: E731
        self.root_pos, self.root_rot, self.dof_pos = cat("root_pos"), cat("root_rot"), cat("dof_pos")
        self.local_body_pos = cat("local_body_pos") if all(m.get("local_body_pos") is not None for m in motions) else None
        self.root_vel, self.dof_vel, self.root_ang_vel = (np.zeros_like(a) for a in (self.root_pos, self.dof_pos, self.root_pos))
        self.stats = np.zeros((len(motions), 4, 3 + self.dof_pos.shape[1]), dtype=F)
        for c in range(len(motions)):
            s = slice(self.seg[c], self.seg[c + 1])
            self.root_vel[s], self.root_ang_vel[s], self.dof_vel[s] = derivatives(self.root_pos[s], self.root_rot[s], self.dof_pos[s],
                                                                                 self.fps[c], ang_vel)
            self.stats[c] = stats(self.root_pos[s], self.dof_pos[s])

    def frames(self, clip, time, loop=True):
        """(ok, lo, hi, blend) per query; lo and hi are rows of the library"""
        clip, time = np.asarray(clip, dtype=np.int64), np.asarray(time, dtype=np.float64)
        C = len(self.fps)
        ok = (clip >= 0) & (clip < C) & np.isfinite(time)
        c = np.where(ok, clip, 0)
        T = self.seg[c + 1] - self.seg[c]
        ok &= T >= 1
        c, T = np.where(ok, c, 0), np.where(ok, T, 1)       # (a refused query, an empty clip among them, reads row 0 and is masked)
        fps = self.fps[c]
        dt, dur = 1.0 / fps, T / fps
        tm = np.where(ok, time, 0.0)
        if loop:
            t = np.fmod(tm, dur)
            t = np.where(t < 0, t + dur, t)
        else:
            t = np.minimum(tm, dur - dt)
        x = t * fps
        fl = np.floor(x)
        under, over = ~(fl >= 0), fl > T - 1
        lo = np.where(under, 0, np.where(over, T - 1, fl)).astype(np.int64)
        blend = np.where(under | over, 0.0, x - fl)
        hi = np.minimum(lo + 1, T - 1)
        return ok, self.seg[c] + lo, self.seg[c] + hi, blend

    def sample(self, clip, time, loop=True, local_body_pos=False):
        ok, lo, hi, blend = self.frames(clip, time, loop)
        same = (lo == hi)[:, None]
        w0, w1 = (1.0 - blend).astype(F)[:, None], blend.astype(F)[:, None]
        out = {}
        names = ["root_pos", "root_vel", "root_ang_vel", "dof_pos", "dof_vel"] + (["local_body_pos"] if local_body_pos else [])
        for k in names:
            a = getattr(self, k)
            al, ah = a[lo].reshape(len(lo), -1), a[hi].reshape(len(lo), -1)
            v = np.where(same, al, w0 * al + w1 * ah)
            out[k] = np.where(ok[:, None], v, F(np.nan)).reshape((len(lo),) + a.shape[1:])
        # slerp on wxyz in float32, every sum in the order the kernel takes
        q1, q2 = self.root_rot[lo][:, [3, 0, 1, 2]], self.root_rot[hi][:, [3, 0, 1, 2]]
        dot = q1[:, 0] * q2[:, 0]
        for k in (1, 2, 3):
            dot = dot + q1[:, k] * q2[:, k]
        flip = dot < 0
        sgn = np.where(flip, F(-1), F(1))
        q2 = sgn[:, None] * q2
        dot = np.clip(sgn * dot, F(-1), F(1))
        lin = w0 * q1 + w1 * q2
        n2 = lin[:, 0] * lin[:, 0]
        for k in (1, 2, 3):
            n2 = n2 + lin[:, k] * lin[:, k]
        with np.errstate(invalid="ignore", divide="ignore"):
            nlerp = lin / np.sqrt(n2)[:, None]
            th0 = np.arccos(dot)
            sn0 = np.sin(th0)
            th = th0 * w1[:, 0]
            sn = np.sin(th)
            s0, s1 = np.cos(th) - dot * sn / sn0, sn / sn0
            slerp = s0[:, None] * q1 + s1[:, None] * q2
        near = dot > F(0.9995)
        r = np.where(same, q1, np.where(near[:, None], nlerp, slerp)).astype(F)
        out["root_rot"] = np.where(ok[:, None], r[:, [1, 2, 3, 0]], F(np.nan))
        out["status"] = (~ok).astype(np.int32)
        # which branch a query took: 0 lo == hi, 1 normalised lerp, 2 slerp, +4 with a flipped hemisphere (for the tests' coverage checks)
        out["branch"] = np.where(same[:, 0], 0, np.where(near, 1, 2)) + 4 * (flip & ~same[:, 0])
        return out
