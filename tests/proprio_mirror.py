"""The proprioception half of the motion tracker in NumPy float32: the statement of record of
``csrc/gmr_tracker_proprio.hip``.  One rounding per operation -- every array is float32 and NumPy rounds after each operator --, so the
device reproduces these lines bit for bit except the gaussian draw, whose ``logf`` and ``cosf`` differ between implementations by an ulp or
two (``gaussian64`` is the same draw in float64, what a test measures the device against).

    config(...)                the configuration as the kernels carry it
    Proprio(cfg, N, R, dt, seed)   the six state arrays and the two calls that write them: step, reset
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_mirror as tm  # noqa: E402

F = np.float32
TERMS = ("lin_vel_z", "ang_vel_xy", "orientation", "torques", "dof_vel", "dof_acc", "root_acc", "action_rate", "dof_pos_limits", "dof_vel_limits",
         "torque_limits", "torque_tiredness", "power", "base_height")
NOISE_BLOCKS = ("gravity", "ang_vel", "dof_pos", "dof_vel", "lin_vel", "height")
NEEDS_ACTIONS, NEEDS_TORQUES = (7,), (3, 10, 11, 12)
TWO_PI = F(6.2831855)
GROUP = 16


def config(default_pos, dof_pos_limits, dof_vel_limits, torque_limits, *, base_height_target, terminate_vel, terminate_height, max_episode_steps,
           extra_cols=0, filter_weight=1.0, normalization=None, noise=None, soft_dof_pos_limit=1.0, soft_dof_vel_limit=1.0, soft_torque_limit=1.0,
           scales=None):
    """float32 scalars and tables; the soft limits are formed as the reference forms them (t1.py:665-670, :677, :684): a Python number
    becomes float32 when it meets a float32 tensor"""
    lim = np.asarray(dof_pos_limits, dtype=F)
    half = F(0.5 * (1.0 - float(soft_dof_pos_limit)))
    span = (lim[:, 1] - lim[:, 0]).astype(F)
    norm = {"gravity": 1.0, "lin_vel": 1.0, "ang_vel": 1.0, "dof_pos": 1.0, "dof_vel": 1.0}
    norm.update(normalization or {})
    specs = {}
    for k in NOISE_BLOCKS:
        s = (noise or {}).get(k)
        if s is None or s.get("distribution", "none") == "none":
            continue
        a, b = (float(x) for x in s["range"])
        specs[k] = {"dist": s["distribution"], "op": s["operation"], "a": F(a), "m": F(b) if s["distribution"] == "gaussian" else F(b - a)}
    sc = np.zeros(len(TERMS), F) if scales is None else np.asarray([scales.get(k, 0.0) for k in TERMS] if isinstance(scales, dict) else scales, dtype=F)
    return {"default_pos": np.asarray(default_pos, dtype=F), "lower": (lim[:, 0] + half * span).astype(F), "upper": (lim[:, 1] - half * span).astype(F),
            "vel_soft": (np.asarray(dof_vel_limits, dtype=F) * F(soft_dof_vel_limit)).astype(F), "tq_lim": np.asarray(torque_limits, dtype=F),
            "tq_soft": (np.asarray(torque_limits, dtype=F) * F(soft_torque_limit)).astype(F), "C": int(extra_cols), "fw": F(filter_weight),
            "fw1": F(1.0 - float(filter_weight)), "norm": {k: F(v) for k, v in norm.items()}, "noise": specs, "height_target": F(base_height_target),
            "term_vel": F(terminate_vel), "term_height": F(terminate_height), "max_steps": int(max_episode_steps), "scale": sc}


def rotate_inverse(q, v):
    """the reference's quat_rotate_inverse (torch_utils.py:78-87) for xyzw ``q [N,4]`` and ``v [N,3]``, in its grouping; q as given"""
    q, v = np.asarray(q, dtype=F), np.asarray(v, dtype=F)
    w, qv = q[:, 3:4], q[:, :3]
    a = v * (F(2.0) * (w * w) - F(1.0))
    cross = np.stack([qv[:, 1] * v[:, 2] - qv[:, 2] * v[:, 1], qv[:, 2] * v[:, 0] - qv[:, 0] * v[:, 2], qv[:, 0] * v[:, 1] - qv[:, 1] * v[:, 0]], axis=1)
    b = cross * w * F(2.0)
    dot = ((qv[:, 0] * v[:, 0] + qv[:, 1] * v[:, 1]) + qv[:, 2] * v[:, 2])[:, None]
    c = qv * dot * F(2.0)
    return ((a - b) + c).astype(F)


def group_sum(x):
    """the sum over the dofs in the kernel's order: lane l of 16 adds the columns l, l + 16, .. in rising order, then the butterfly
    x = x + x[lane ^ m], m = 1, 2, 4, 8"""
    x = np.asarray(x, dtype=F)
    N, R = x.shape
    lanes = np.zeros((N, GROUP), F)
    for j in range(R):
        lanes[:, j % GROUP] = lanes[:, j % GROUP] + x[:, j]
    idx = np.arange(GROUP)
    for m in (1, 2, 4, 8):
        lanes = lanes + lanes[:, idx ^ m]
    return lanes[:, 0].astype(F)


def words(key, e, tick, i):
    """the two Philox words of element i of environment e at its tick: an even i takes words (0, 1), an odd i words (2, 3)"""
    return pair(tm.philox4x32((e, tick, i >> 1, 1), key), i)


def pair(w, i):
    return (w[2], w[3]) if i & 1 else (w[0], w[1])


def unit(w):
    return F(w >> 8) * F(2.0 ** -24)          # [0, 1)


def unit_open(w):
    return F((w >> 8) + 1) * F(2.0 ** -24)    # (0, 1]


def gaussian32(wa, wb):
    with np.errstate(divide="ignore"):
        return F(np.sqrt(F(-2.0) * np.log(unit_open(wa), dtype=F), dtype=F) * np.cos(TWO_PI * unit(wb), dtype=F))


def gaussian64(wa, wb):
    """the same draw in float64 on the same words (the angle's factor is the float32 literal)"""
    return float(np.sqrt(-2.0 * np.log(float(unit_open(wa)))) * np.cos(float(TWO_PI) * float(unit(wb))))


def apply_noise(x, spec, r):
    """apply_randomization (utils/utils.py:9-25) with the unit draw ``r`` (z or u) given: n = a + m r, then x + n or x n"""
    with np.errstate(invalid="ignore", over="ignore"):
        n = (spec["a"] + spec["m"] * np.asarray(r, dtype=F)).astype(F)
        x = np.asarray(x, dtype=F)
        return (x * n if spec["op"] == "scaling" else x + n).astype(F)


class Proprio:
    """the state of N environments with R dofs, zeros at first, and the launch of a step"""

    def __init__(self, cfg, N, R, dt, seed=0):
        self.cfg, self.N, self.R, self.dt = cfg, N, R, F(dt)
        self.key = (seed & tm.M32, (seed >> 32) & tm.M32)
        self.W = 6 + cfg["C"] + 3 * R
        self.filtered_lin_vel, self.filtered_ang_vel = np.zeros((N, 3), F), np.zeros((N, 3), F)
        self.last_root_vel = np.zeros((N, 6), F)
        self.last_actions, self.last_dof_vel = np.zeros((N, R), F), np.zeros((N, R), F)
        self.noise_tick = np.zeros(N, np.uint32)
        self.ignored = 0

    def state(self):
        return {k: getattr(self, k).copy() for k in ("filtered_lin_vel", "filtered_ang_vel", "last_root_vel", "last_actions", "last_dof_vel", "noise_tick")}

    def reset(self, root_states, mask=None, env_ids=None):
        """entry i -- environment env_ids[i], or i -- with its mask set: filtered velocities 0, last_root_vel = root_states[i, 7:13];
        returns the ids dropped"""
        rs = np.asarray(root_states, dtype=F)
        n = len(rs)
        ids = np.arange(n) if env_ids is None else np.asarray(env_ids, dtype=np.int64)
        dropped = 0
        for i in range(n):
            if mask is not None and not mask[i]:
                continue
            e = int(ids[i])
            if not 0 <= e < self.N:
                dropped += 1
                continue
            self.filtered_lin_vel[e] = 0
            self.filtered_ang_vel[e] = 0
            self.last_root_vel[e] = rs[i, 7:13]
        self.ignored += dropped
        return dropped

    def _noisy(self, x, block, first, draw, wide=False):
        """apply_randomization (utils/utils.py:9-25) on the columns ``first ..`` of the row; ``wide``: also the float64 noise value"""
        x = np.asarray(x, dtype=F)
        spec = self.cfg["noise"].get(block)
        if not draw or spec is None:
            return x, None
        r, r64 = np.zeros(x.shape, F), np.zeros(x.shape)
        for e in range(x.shape[0]):
            for k in range(x.shape[1]):
                wa, wb = words(self.key, e, int(self.noise_tick[e]), first + k)
                if spec["dist"] == "gaussian":
                    r[e, k] = gaussian32(wa, wb)
                    if wide:
                        r64[e, k] = gaussian64(wa, wb)
                else:
                    r[e, k] = unit(wa)
                    r64[e, k] = float(r[e, k])
        return apply_noise(x, spec, r), r64

    def step(self, root_states, dof_pos, dof_vel, actions=None, mean_torques=None, extra=None, ground=None, episode_steps=None, noise=True,
             wide=False):
        """one launch -> the dict of outputs; with ``wide`` also ``z64``: the float64 draws behind obs and priv (``[N, W + 4]``, 0 where no
        draw was made)"""
        cfg, N, R = self.cfg, self.N, self.R
        rs, q, qd = (np.asarray(a, dtype=F) for a in (root_states, dof_pos, dof_vel))
        assert rs.shape == (N, 13) and q.shape == (N, R) and qd.shape == (N, R) and (extra is not None) == (cfg["C"] > 0)
        act = None if actions is None else np.asarray(actions, dtype=F)
        tau = None if mean_torques is None else np.asarray(mean_torques, dtype=F)
        draw = bool(noise) and bool(cfg["noise"])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            rv = rs[:, 7:13]
            h = (rs[:, 2] - (F(0) if ground is None else np.asarray(ground, dtype=F))).astype(F)
            blv, bav = rotate_inverse(rs[:, 3:7], rs[:, 7:10]), rotate_inverse(rs[:, 3:7], rs[:, 10:13])
            pg = rotate_inverse(rs[:, 3:7], np.tile(np.array([0, 0, -1], F), (N, 1)))
            flv = (blv * cfg["fw"] + self.filtered_lin_vel * cfg["fw1"]).astype(F)
            fav = (bav * cfg["fw"] + self.filtered_ang_vel * cfg["fw1"]).astype(F)
            root_acc, speed2 = np.zeros(N, F), np.zeros(N, F)
            for k in range(6):
                d = ((self.last_root_vel[:, k] - rv[:, k]) / self.dt).astype(F)
                root_acc = root_acc + d * d
                speed2 = speed2 + rv[:, k] * rv[:, k]
            term = np.zeros((N, len(TERMS)), F)
            term[:, 0] = flv[:, 2] * flv[:, 2]
            term[:, 1] = bav[:, 0] * bav[:, 0] + bav[:, 1] * bav[:, 1]
            term[:, 2] = pg[:, 0] * pg[:, 0] + pg[:, 1] * pg[:, 1]
            term[:, 4] = group_sum(qd * qd)
            dd = ((self.last_dof_vel - qd) / self.dt).astype(F)
            term[:, 5] = group_sum(dd * dd)
            term[:, 6] = root_acc
            term[:, 8] = group_sum(((q < cfg["lower"]) | (q > cfg["upper"])).astype(F))
            ex = np.abs(qd) - cfg["vel_soft"]
            ex = np.where(ex < 0, F(0), ex)
            term[:, 9] = group_sum(np.where(ex > 1, F(1), ex))
            if act is not None:
                da = self.last_actions - act
                term[:, 7] = group_sum(da * da)
            if tau is not None:
                term[:, 3] = group_sum(tau * tau)
                over = np.abs(tau) - cfg["tq_soft"]
                term[:, 10] = group_sum(np.where(over < 0, F(0), over))
                rel = (tau / cfg["tq_lim"]).astype(F)
                tired = rel * rel
                term[:, 11] = group_sum(np.where(tired > 1, F(1), tired))
                pw = tau * qd
                term[:, 12] = group_sum(np.where(pw < 0, F(0), pw))
            dh = h - cfg["height_target"]
            term[:, 13] = dh * dh
            total = np.zeros(N, F)
            for k in range(len(TERMS)):
                given = act is not None if k in NEEDS_ACTIONS else (tau is not None if k in NEEDS_TORQUES else True)
                if given and cfg["scale"][k] != 0:
                    total = total + cfg["scale"][k] * term[:, k]
            # the observation row and the privileged block
            C = cfg["C"]
            nm = cfg["norm"]
            z64 = np.zeros((N, self.W + 4))
            parts, first = [], 0
            for block, x, sc in (("gravity", pg, nm["gravity"]), ("ang_vel", bav, nm["ang_vel"]), (None, extra, None),
                                 ("dof_pos", (q - cfg["default_pos"]).astype(F), nm["dof_pos"]), ("dof_vel", qd, nm["dof_vel"]),
                                 (None, np.zeros((N, R), F) if act is None else act, None)):
                if x is None:
                    continue
                x = np.asarray(x, dtype=F)
                if block is not None:
                    x, r64 = self._noisy(x, block, first, draw, wide)
                    if r64 is not None:
                        z64[:, first:first + x.shape[1]] = r64
                    x = (x * sc).astype(F)
                parts.append(x)
                first += x.shape[1]
            obs = np.concatenate(parts, axis=1).astype(F)
            assert obs.shape == (N, self.W)
            lin, r64 = self._noisy(blv, "lin_vel", self.W, draw, wide)
            if r64 is not None:
                z64[:, self.W:self.W + 3] = r64
            hh, r64 = self._noisy(h[:, None], "height", self.W + 3, draw, wide)
            if r64 is not None:
                z64[:, self.W + 3:] = r64
            priv = np.concatenate([(lin * nm["lin_vel"]).astype(F), hh], axis=1).astype(F)
            done = (speed2 > cfg["term_vel"]).astype(np.int32) | 2 * (h < cfg["term_height"]).astype(np.int32)
            if episode_steps is not None:
                done = done | 4 * (np.asarray(episode_steps).astype(np.int64) > cfg["max_steps"]).astype(np.int32)
        # the roll-over
        self.filtered_lin_vel, self.filtered_ang_vel = flv, fav
        if act is not None:
            self.last_actions = act.copy()
        self.last_dof_vel, self.last_root_vel = qd.copy(), rv.copy()
        if draw:
            self.noise_tick = self.noise_tick + np.uint32(1)
        out = {"base_lin_vel": blv, "base_ang_vel": bav, "projected_gravity": pg, "filtered_lin_vel": flv.copy(), "filtered_ang_vel": fav.copy(),
               "obs": obs, "priv": priv, "term": term, "total": total.astype(F), "done": done.astype(np.int32)}
        if wide:
            out["z64"] = z64
        return out
