"""Terrain heights and the feet half of the motion tracker in NumPy: the statement of record of
``csrc/gmr_tracker_feet.hip``.  One rounding per operation -- every array is float32 and NumPy rounds after each operator; the terrain's
weights, products and sum are float64 as the reference's NumPy promotion makes them --, so the device reproduces these lines bit for bit
except what passes through ``atan2f``, ``cosf`` or ``sinf``: here the float32 arguments are formed bit-exactly and the function is evaluated
in float64 and rounded once, which an implementation of the float32 function misses by an ulp or two.

    terrain(field, hs, vs, border)     the terrain as the kernels carry it (None: the plane)
    heights(ter, points)               Terrain.terrain_heights (booster_gym/utils/terrain.py:101-121) -> (f32[M], outside)
    config(...)                        the feet configuration as the kernels carry it
    Feet(cfg, ter, N, dt)              the two state arrays and the call that writes them: step
"""
import numpy as np

F = np.float32
D = np.float64
TERMS = ("collision", "feet_slip", "feet_vel_z", "feet_roll", "feet_yaw_diff", "feet_yaw_mean", "feet_distance", "feet_swing")
ANGLE_TERMS = (3, 4, 5, 6)                # the terms that pass through atan2f / cosf / sinf
PI, TWO_PI = F(3.1415927), F(6.2831855)
DONE_CONTACT = 8


# ---- terrain ---------------------------------------------------------------------------------------------------------------------------
def terrain(height_field, horizontal_scale, vertical_scale, border_pixels):
    if height_field is None:
        return None
    field = np.asarray(height_field)
    assert field.dtype == np.int16 and field.ndim == 2 and min(field.shape) >= 2
    return {"field": field, "hs": F(horizontal_scale), "vs": float(vertical_scale), "border": F(int(border_pixels))}


def heights(ter, points):
    """terrain.py:105-118 in its NumPy promotion: x in float32, the weights, the four products and their sum (from the left) in float64, one
    rounding to float32.  Each of the four indices is clamped to the field, the weights stay as computed and the point is counted; a
    coordinate that is not finite gives NaN and is counted too."""
    p = np.asarray(points, dtype=F)
    M = len(p)
    if ter is None:
        return np.zeros(M, F), 0
    field = ter["field"]
    nx, ny = field.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = (ter["border"] + p[:, 0] / ter["hs"]).astype(F)                  # :105
        y = (ter["border"] + p[:, 1] / ter["hs"]).astype(F)                  # :106
    finite = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(finite, x, F(0)), np.where(finite, y, F(0))
    x1, y1 = np.floor(xs).astype(D), np.floor(ys).astype(D)                  # :107-110
    x2, y2 = x1 + 1.0, y1 + 1.0
    xd, yd = xs.astype(D), ys.astype(D)
    outside = ~finite | (x1 < 0) | (x2 > nx - 1) | (y1 < 0) | (y2 > ny - 1)
    ix1, ix2 = np.clip(x1, 0, nx - 1).astype(np.int64), np.clip(x2, 0, nx - 1).astype(np.int64)
    iy1, iy2 = np.clip(y1, 0, ny - 1).astype(np.int64), np.clip(y2, 0, ny - 1).astype(np.int64)
    h = field.astype(D)
    s = ((x2 - xd) * (y2 - yd) * h[ix1, iy1] + (xd - x1) * (y2 - yd) * h[ix2, iy1]
         + (x2 - xd) * (yd - y1) * h[ix1, iy2] + (xd - x1) * (yd - y1) * h[ix2, iy2])          # :113-116
    out = (s * ter["vs"]).astype(F)                                                             # :118-119
    out[~finite] = np.nan
    return out, int(outside.sum())


# ---- feet ------------------------------------------------------------------------------------------------------------------------------
def config(feet_body, edge_pos, nb, termination_body=(), penalized_body=(), force_threshold=1.0, contact_clearance=0.01, feet_distance_ref=0.2,
           swing_period=0.2, scales=None):
    """float32 scalars as torch makes them where a Python number meets a float32 tensor (t1.py:545, :553, :725, :728)"""
    sc = np.zeros(len(TERMS), F) if scales is None else np.asarray([scales.get(k, 0.0) for k in TERMS] if isinstance(scales, dict) else scales, dtype=F)
    return {"feet_body": [int(b) for b in feet_body], "edge": np.asarray(edge_pos, dtype=F).reshape(-1, 3), "nb": int(nb),
            "term_body": [int(b) for b in termination_body], "pen_body": [int(b) for b in penalized_body], "threshold": F(force_threshold),
            "clearance": F(contact_clearance), "distance_ref": F(feet_distance_ref), "half_swing": F(0.5 * float(swing_period)), "scale": sc}


def rotate(q, v):
    """the reference's quat_rotate (torch_utils.py:66-75) for xyzw ``q [N,4]`` and ``v [N,3]``, a + b + c in this grouping; q as given"""
    q, v = np.asarray(q, dtype=F), np.asarray(v, dtype=F)
    w, qv = q[:, 3:4], q[:, :3]
    a = v * (F(2.0) * (w * w) - F(1.0))
    cross = np.stack([qv[:, 1] * v[:, 2] - qv[:, 2] * v[:, 1], qv[:, 2] * v[:, 0] - qv[:, 0] * v[:, 2], qv[:, 0] * v[:, 1] - qv[:, 1] * v[:, 0]], axis=1)
    b = cross * w * F(2.0)
    dot = ((qv[:, 0] * v[:, 0] + qv[:, 1] * v[:, 1]) + qv[:, 2] * v[:, 2])[:, None]
    c = qv * dot * F(2.0)
    return ((a + b) + c).astype(F)


def rem(a, b):
    """torch's remainder for a positive divisor: fmod (exact), then the divisor is added to a negative result"""
    r = np.fmod(np.asarray(a, dtype=F), b).astype(F)
    return np.where((r != 0) & (r < 0), r + b, r).astype(F)


def wrap(a):
    """(a + pi) % 2 pi - pi (t1.py:533-534, :713, :717)"""
    return (rem(np.asarray(a, dtype=F) + PI, TWO_PI) - PI).astype(F)


def atan2(y, x):
    return np.arctan2(np.asarray(y, dtype=F).astype(D), np.asarray(x, dtype=F).astype(D)).astype(F)


def cos(a):
    return np.cos(np.asarray(a, dtype=F).astype(D)).astype(F)


def sin(a):
    return np.sin(np.asarray(a, dtype=F).astype(D)).astype(F)


def euler_roll(q):
    """roll of get_euler_xyz for xyzw ``q [N,4]``, % 2 pi"""
    x, y, z, w = (np.asarray(q, dtype=F)[:, k] for k in range(4))
    return rem(atan2(F(2.0) * (w * x + y * z), ((w * w - x * x) - y * y) + z * z), TWO_PI)


def euler_yaw(q):
    x, y, z, w = (np.asarray(q, dtype=F)[:, k] for k in range(4))
    return rem(atan2(F(2.0) * (w * z + x * y), ((w * w + x * x) - y * y) - z * z), TWO_PI)


def force_norm(f):
    f = np.asarray(f, dtype=F)
    return np.sqrt((f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2]).astype(F)


class Feet:
    """the state of N environments, zeros at first, and the launch of a step.  After a step ``margins`` holds how far the step stayed from
    its discontinuities: ``clearance`` -- the least |edge clearance - threshold| --, ``angle`` -- the least distance of a wrapped angle
    (roll, yaw, the two wrapped differences, |yaw_1 - yaw_0|) from pi, and of an unwrapped one (the raw atan2 values) from the 0 / 2 pi seam."""

    def __init__(self, cfg, ter, N, dt):
        self.cfg, self.ter, self.N, self.dt = cfg, ter, N, F(dt)
        self.last_feet_pos, self.gait_process = np.zeros((N, 2, 3), F), np.zeros(N, F)
        self.margins = {}

    def state(self):
        return {"last_feet_pos": self.last_feet_pos.copy(), "gait_process": self.gait_process.copy()}

    def step(self, body_pos, body_rot, root_states, contact_forces=None, episode_steps=None, gait_frequency=None):
        cfg, N = self.cfg, self.N
        bp, bq, rs = np.asarray(body_pos, dtype=F), np.asarray(body_rot, dtype=F), np.asarray(root_states, dtype=F)
        assert bp.shape == (N, cfg["nb"], 3) and bq.shape == (N, cfg["nb"], 4) and rs.shape == (N, 13)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            fp, fq = bp[:, cfg["feet_body"]].copy(), bq[:, cfg["feet_body"]].copy()                 # :530-531
            raw_roll = np.stack([euler_roll(fq[:, f]) for f in range(2)], axis=1)
            raw_yaw = np.stack([euler_yaw(fq[:, f]) for f in range(2)], axis=1)
            roll, yaw = wrap(raw_roll), wrap(raw_yaw)                                                 # :533-534
            contact = np.zeros((N, 2), bool)
            clear_margin = np.inf
            for f in range(2):
                for k in range(len(cfg["edge"])):
                    edge = (fp[:, f] + rotate(fq[:, f], np.tile(cfg["edge"][k], (N, 1)))).astype(F)  # :543
                    h, _ = heights(self.ter, edge[:, :2])
                    clear = (edge[:, 2] - h).astype(F)
                    contact[:, f] |= clear < cfg["clearance"]                                         # :545
                    gap = np.abs(clear.astype(D) - float(cfg["clearance"]))
                    if np.isfinite(gap).any():
                        clear_margin = min(clear_margin, float(np.nanmin(gap)))
            ground, _ = heights(self.ter, rs[:, :2])
            base_yaw = euler_yaw(rs[:, 3:7])
            gf = np.zeros(N, F) if gait_frequency is None else np.asarray(gait_frequency, dtype=F)
            gp = np.fmod(self.gait_process + self.dt * gf, F(1.0)).astype(F)                          # :478
            moving = gf > F(1.0e-8)
            on = moving.astype(F)
            ga = (TWO_PI * gp).astype(F)
            gait = np.stack([cos(ga) * on, sin(ga) * on], axis=1).astype(F)                           # :585-586
            # the terms
            term = np.zeros((N, len(TERMS)), F)
            n_term = np.zeros(N, np.int32)
            if contact_forces is not None:
                cf = np.asarray(contact_forces, dtype=F)
                assert cf.shape == (N, cfg["nb"], 3)
                norm = force_norm(cf)
                term[:, 0] = (norm[:, cfg["pen_body"]] > cfg["threshold"]).sum(axis=1).astype(F)      # :629
                n_term = (norm[:, cfg["term_body"]] > cfg["threshold"]).sum(axis=1)
            d = ((self.last_feet_pos - fp) / self.dt).astype(F)
            s = ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).astype(F)
            gate = np.ones(N, F) if episode_steps is None else (np.asarray(episode_steps).astype(np.int64) > 1).astype(F)
            c = contact.astype(F)
            term[:, 1] = (s[:, 0] * c[:, 0] + s[:, 1] * c[:, 1]) * gate                               # :698-704
            term[:, 2] = d[:, 0, 2] * d[:, 0, 2] + d[:, 1, 2] * d[:, 1, 2]                            # :707
            term[:, 3] = roll[:, 0] * roll[:, 0] + roll[:, 1] * roll[:, 1]                            # :710
            dy = (yaw[:, 1] - yaw[:, 0]).astype(F)
            yd = wrap(dy)                                                                             # :713
            term[:, 4] = yd * yd
            mean = ((yaw[:, 0] + yaw[:, 1]) * F(0.5) + np.where(np.abs(dy) > PI, PI, F(0))).astype(F)  # :716
            ym = wrap(base_yaw - mean)                                                                # :717
            term[:, 5] = ym * ym
            dist = np.abs(cos(base_yaw) * (fp[:, 1, 1] - fp[:, 0, 1]) - sin(base_yaw) * (fp[:, 1, 0] - fp[:, 0, 0])).astype(F)   # :721-724
            dr = (cfg["distance_ref"] - dist).astype(F)
            dr = np.where(dr < 0, F(0), dr)
            term[:, 6] = np.where(dr > F(0.1), F(0.1), dr)                                            # :725; a NaN stays one
            left = (np.abs(gp - F(0.25)) < cfg["half_swing"]) & moving                                # :728
            right = (np.abs(gp - F(0.75)) < cfg["half_swing"]) & moving                               # :729
            term[:, 7] = (left & ~contact[:, 0]).astype(F) + (right & ~contact[:, 1]).astype(F)       # :730
            total = np.zeros(N, F)
            for k in range(len(TERMS)):
                given = contact_forces is not None if k == 0 else True
                if given and cfg["scale"][k] != 0:
                    total = total + cfg["scale"][k] * term[:, k]
            done = np.where(n_term > 0, DONE_CONTACT, 0).astype(np.int32)                             # :553
            # how far from a discontinuity the angles stayed
            seams = [np.abs(np.abs(a.astype(D)) - np.pi) for a in (roll, yaw, yd, ym, dy)]
            seams += [np.minimum(a.astype(D), 2 * np.pi - a.astype(D)) for a in (raw_roll, raw_yaw, base_yaw)]
            with np.errstate(all="ignore"):
                finite = [a[np.isfinite(a)] for a in seams]
            self.margins = {"clearance": clear_margin, "angle": min([float(a.min()) for a in finite if a.size] + [np.inf])}
        # the roll-over
        self.last_feet_pos, self.gait_process = fp.copy(), gp
        return {"feet_pos": fp, "feet_roll": roll, "feet_yaw": yaw, "feet_contact": contact.astype(np.int32), "ground": ground, "gait": gait,
                "term": term, "total": total.astype(F), "done": done}
