"""The control half of the motion tracker in NumPy float32: the statement of record of
``csrc/gmr_tracker_control.hip``.  One rounding per operation -- every array is float32 and NumPy rounds after each operator --, so the
device reproduces these lines bit for bit except ``cos``, whose float32 implementations differ by an ulp or two.

    targets(cfg, ref, actions, steps, dt, bad)   the PD targets of a step from the reference's joint row
    Actuators(cfg, N, R)                         held / torque_acc and the two calls that write them: hold, torques
"""
import numpy as np

F = np.float32
PI_LITERAL = F(3.14159)          # the literal of the easing, not pi


def config(default_pos, action_scale, clip_actions, decimation, startup_seconds=2.0, gain_startup=0.1, gain_run=0.2):
    """the control configuration as the kernels carry it: float32 scalars and the default pose"""
    return {"default_pos": np.asarray(default_pos, dtype=F), "k": F(action_scale), "c": F(clip_actions), "D": F(startup_seconds),
            "g0": F(gain_startup), "g1": F(gain_run), "M": int(decimation)}


def clip_sym(x, c):
    """min(max(x, -c), c); a NaN stays one"""
    x = np.asarray(x, dtype=F)
    lo = F(-c) if np.ndim(c) == 0 else (-c).astype(F)
    x = np.where(x < lo, lo, x)
    return np.where(x > c, c, x).astype(F)


def phase(cfg, steps, dt):
    """``(startup bool[N], s f32[N])`` of the episode step counters; ``s`` is meaningful where ``startup`` is set"""
    with np.errstate(divide="ignore", invalid="ignore"):
        te = np.asarray(steps).astype(F) * F(dt)
        startup = te < cfg["D"]
        p = np.minimum(np.maximum(np.where(startup, te / cfg["D"], F(0)).astype(F), F(0)), F(1))
        s = F(0.5) * (F(1.0) - np.cos(p * PI_LITERAL, dtype=F))
    return startup, s.astype(F)


def targets(cfg, ref, actions=None, steps=None, dt=0.02, bad=None):
    """``(dof_targets f32[N,R], actions_clipped or None, status i32[N])`` from ``ref``, the reference's joint row ``[N,R]`` at the
    clock.  ``bad bool[N]``: the environments with a bad assignment (a NaN row, status 1)."""
    ref = np.asarray(ref, dtype=F)
    N, R = ref.shape
    if steps is None:
        startup, s = np.zeros(N, bool), np.zeros(N, F)
    else:
        startup, s = phase(cfg, steps, dt)
    su, sc = startup[:, None], s[:, None]
    d = cfg["default_pos"][None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        eased = d * (F(1.0) - sc) + ref * sc
        base = np.where(su, eased, ref).astype(F)
        clipped = None
        out = base
        if actions is not None:
            clipped = clip_sym(actions, cfg["c"])
            gain = np.where(su, cfg["g0"], cfg["g1"]).astype(F)
            out = base + (cfg["k"] * clipped) * gain
    out = out.astype(F)
    status = np.zeros(N, np.int32)
    if bad is not None:
        out[bad] = np.nan
        status[bad] = 1
    return out, clipped, status


class Actuators:
    """``held`` and ``torque_acc`` of N environments and R dofs, zeros at first (last_dof_targets and torques of the reference)"""

    def __init__(self, cfg, N, R):
        self.cfg, self.N, self.R = cfg, N, R
        self.held, self.acc = np.zeros((N, R), F), np.zeros((N, R), F)
        self.ignored = 0

    def hold(self, dof_pos, mask=None, env_ids=None):
        """entry i -- environment env_ids[i], or i -- with its mask set: held = dof_pos[i], torque_acc = 0; returns the ids dropped"""
        dof_pos = np.asarray(dof_pos, dtype=F)
        n = len(dof_pos)
        ids = np.arange(n) if env_ids is None else np.asarray(env_ids, dtype=np.int64)
        dropped = 0
        for i in range(n):
            if mask is not None and not mask[i]:
                continue
            e = int(ids[i])
            if not 0 <= e < self.N:
                dropped += 1
                continue
            self.held[e] = dof_pos[i]
            self.acc[e] = 0
        self.ignored += dropped
        return dropped

    def torques(self, i, dof_targets, q, qd, kp, kd, friction=None, limit=None, delay=None):
        """substep i -> ``(dof_torques, mean_torques or None)``; kp, kd, friction are [N,R] or [R] (broadcast), limit [R]"""
        M = self.cfg["M"]
        assert 0 <= i < M
        tg, q, qd = (np.asarray(a, dtype=F) for a in (dof_targets, q, qd))
        kp, kd = np.asarray(kp, dtype=F), np.asarray(kd, dtype=F)
        hit = (np.zeros(self.N, np.int64) if delay is None else np.asarray(delay)) == i
        self.held[hit] = tg[hit]
        with np.errstate(invalid="ignore", over="ignore"):
            tau = (kp * (self.held - q) - kd * qd).astype(F)
            if friction is not None:
                fr = np.broadcast_to(np.asarray(friction, dtype=F), tau.shape)
                a = np.abs(tau)
                f = np.where(fr < a, fr, a)
                f = np.where(np.isnan(fr), fr, f).astype(F)
                sg = np.where(tau > 0, F(1), np.where(tau < 0, F(-1), F(0))).astype(F)
                tau = (tau - f * sg).astype(F)
            if limit is not None:
                tau = clip_sym(tau, np.broadcast_to(np.asarray(limit, dtype=F), tau.shape))
            self.acc = ((self.acc if i else np.zeros_like(self.acc)) + tau).astype(F)
            mean = (self.acc / F(M)).astype(F) if i == M - 1 else None
        return tau, mean
