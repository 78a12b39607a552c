"""The command half of the motion tracker in NumPy float32: the statement of record of
``csrc/gmr_tracker_commands.hip``.  One rounding per operation -- every value is float32 and NumPy rounds after each operator --, so the
device reproduces these lines bit for bit except ``expf`` of a tracking term and the gaussian draw of a kick or push, whose ``logf`` and
``cosf`` differ between implementations by an ulp or two (``term64`` and ``proprio_mirror.gaussian64`` are what a test measures the device
against).

    config(...)                    the command configuration as the kernels carry it
    Commands(cfg, N, seed)         the state arrays and the call that writes them: step
    disturb_config(...), disturb_actions(...), disturb(...)     kicks and pushes: no state
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proprio_mirror as pm  # noqa: E402
import tracker_mirror as tm  # noqa: E402

F = np.float32
D = np.float64
TERMS = ("survival", "tracking_lin_vel_x", "tracking_lin_vel_y", "tracking_ang_vel")
BOUNDARY, RESAMPLED, SUCCESS = 1, 2, 4
KICK, PUSH_START, PUSH_STOP = 1, 2, 4
CHUNK = 8
SPECS = ("kick_lin_vel", "kick_ang_vel", "push_force", "push_torque")
M32 = 0xFFFFFFFF


def config(lin_vel_x, lin_vel_y, ang_vel_yaw, gait_frequency, resample_steps, *, still_proportion=0.0, tracking_sigma=0.25, scales=None,
           obs_scales=None, curriculum=None):
    """float32 scalars; the span of a uniform is formed in double and rounded once; a Python number becomes float32 where it meets a
    float32 tensor"""
    rng = (lin_vel_x, lin_vel_y, ang_vel_yaw, gait_frequency)
    c = {"lo": [F(float(r[0])) for r in rng], "span": [F(float(r[1]) - float(r[0])) for r in rng], "rs_lo": int(resample_steps[0]),
         "rs_span": int(resample_steps[1]) - int(resample_steps[0]), "still": F(still_proportion), "sigma": F(tracking_sigma),
         "scale": np.zeros(4, F) if scales is None else np.asarray([scales.get(k, 0.0) for k in TERMS] if isinstance(scales, dict) else scales, dtype=F),
         "obs_scale": np.asarray((1.0, 1.0, 1.0) if obs_scales is None else obs_scales, dtype=F), "curriculum": None}
    if curriculum is not None:
        L, A = int(curriculum["lin_vel_levels"]), int(curriculum["ang_vel_levels"])
        order = curriculum.get("index_order", "grid")
        if order == "reference" and L != A:
            raise ValueError("index_order 'reference' needs lin_vel_levels == ang_vel_levels")
        c["curriculum"] = {"L": L, "A": A, "order": order, "rate": F(curriculum["update_rate"]), "tol": [F(x) for x in curriculum["tolerances"]],
                           "res": [F(x) for x in curriculum["resolutions"]], "min_success": int(curriculum["min_success_steps"])}
    return c


def min_success_steps(episode_length_s, dt, toler):
    """floor(ceil(episode_length_s / dt) * (1 - toler)): steps > that, for a whole steps, is the comparison of t1.py:394-396"""
    return int(np.floor(np.ceil(episode_length_s / dt) * (1 - toler)))


def term64(c, f, sigma):
    """a tracking term in float64 from the exactly formed float32 argument -((c - f) * (c - f)) / sigma"""
    d = (np.asarray(c, dtype=F) - np.asarray(f, dtype=F)).astype(F)
    arg = (-(d * d).astype(F) / F(sigma)).astype(F)
    return np.exp(arg.astype(D))


def update_grid(prob, hits, rate):
    """step 5, first half: prob = min(prob + rate * (float)hits, 1) in float32, one rounding per operation; hits -> 0"""
    p = (prob.reshape(-1) + (F(rate) * hits.astype(F)).astype(F)).astype(F)
    return np.minimum(p, F(1.0)).reshape(prob.shape)


def cumulate(prob):
    """step 5, second half: cum f64[G + 1] of the flattened grid, operation by operation.  Lane k sums the cells 8k .. 8k + 7 in rising
    order: s_0 = 0, s_{i+1} = s_i + (double)prob[8k + i]; base_0 = 0, base_{k+1} = base_k + (s at the end of chunk k), chained in rising
    k; cum[8k + i] = base_k + s_i; cum[G] = base of the last chunk + its end sum."""
    p = prob.reshape(-1).astype(D)
    G = len(p)
    nch = (G + CHUNK - 1) // CHUNK
    cum = np.zeros(G + 1, D)
    base = D(0.0)
    for k in range(nch):
        s = D(0.0)
        for g in range(k * CHUNK, min(G, (k + 1) * CHUNK)):
            cum[g] = base + s
            s = s + p[g]
        if k == nch - 1:
            cum[G] = base + s
        base = base + s
    return cum


def philox_np(e, n, j, domain, key):
    """tracker_mirror.philox4x32 on arrays: counters (e, n, j, domain) -> four uint32 arrays"""
    m = np.uint64(M32)
    c0, c1 = np.asarray(e).astype(np.uint64), np.asarray(n).astype(np.uint64)
    c2, c3 = np.full_like(c0, j), np.full_like(c0, domain)
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & m, p1 & m, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & m, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def unit_np(w):
    return (w >> np.uint32(8)).astype(F) * F(2.0 ** -24)          # [0, 1): 24 bits, exact


def draw_cells(cum, words):
    """draw_cell on an array of words"""
    G = len(cum) - 1
    target = (words.astype(D) * D(2.0 ** -32)) * cum[G]
    return np.searchsorted(cum[:G], target, side="right") - 1


def draw_cell(cum, word):
    """the largest g in [0, G) with cum[g] <= (double)word * 2^-32 * cum[G]"""
    G = len(cum) - 1
    target = D(word) * D(2.0 ** -32) * cum[G]
    return int(np.searchsorted(cum[:G], target, side="right")) - 1


def split_cell(g, L, A, order):
    """(lin, ang) of cell g: "reference" as t1.py:417-418 (the transpose of the grid's own indexing), "grid" the consistent split"""
    ny = 2 * A + 1
    g = np.asarray(g)
    return (g % ny - L, g // ny - A) if order == "reference" else (g // ny - L, g % ny - A)


def curriculum_commands(lin, ang, u0, u1, u2, res):
    """t1.py:425-435 in the grouping of the header: c0 = ((float)lin + (u0 + -0.5f)) * res_x, c1 = ((float)|lin| * (2.0f * u1 + -1.0f)) *
    res_y, c2 = ((float)ang + (u2 + -0.5f)) * res_yaw; arrays or scalars"""
    lin, ang = np.asarray(lin), np.asarray(ang)
    u0, u1, u2 = (np.asarray(u, dtype=F) for u in (u0, u1, u2))
    a0 = (u0 + F(-0.5)).astype(F)
    c0 = ((lin.astype(F) + a0).astype(F) * F(res[0])).astype(F)
    a1 = ((F(2.0) * u1).astype(F) + F(-1.0)).astype(F)
    c1 = ((np.abs(lin).astype(F) * a1).astype(F) * F(res[1])).astype(F)
    a2 = (u2 + F(-0.5)).astype(F)
    c2 = ((ang.astype(F) + a2).astype(F) * F(res[2])).astype(F)
    return c0, c1, c2


def uniform(lo, span, u):
    """torch_rand_float as restated: (upper - lower) * u + lower"""
    return ((F(span) * np.asarray(u, dtype=F)).astype(F) + F(lo)).astype(F)


def below(word, n):
    return (int(word) * int(n)) >> 32


class Commands:
    def __init__(self, cfg, N, seed=0):
        self.cfg, self.N = cfg, int(N)
        self.key = (seed & M32, (seed >> 32) & M32)
        self.commands = np.zeros((N, 3), F)
        self.gait_frequency = np.zeros(N, F)
        self.cmd_resample_time = np.zeros(N, np.int32)
        self.cmd_draws = np.zeros(N, np.uint32)
        cur = cfg["curriculum"]
        if cur is not None:
            nx, ny = 2 * cur["L"] + 1, 2 * cur["A"] + 1
            self.env_level = np.zeros((N, 2), np.int32)
            self.curriculum_prob = np.zeros((nx, ny), F)
            self.curriculum_prob[cur["L"], cur["A"]] = F(1.0)
            self.hits = np.zeros(nx * ny, np.uint32)
            self.cum = np.zeros(nx * ny + 1, D)

    def step(self, episode_steps, done=None, lin_vel=None, ang_vel=None, cfg=None):
        """the call in the order of the header; returns term, term64 (the float64 evaluation), total, commands, gait_frequency, flags, cmd_obs"""
        cfg = self.cfg if cfg is None else cfg
        cur, N = cfg["curriculum"], self.N
        steps = np.asarray(episode_steps, dtype=np.int32)
        d = np.zeros(N, bool) if done is None else np.asarray(done) != 0
        if cur is not None and (lin_vel is None or ang_vel is None):
            raise ValueError("the curriculum needs the velocities")
        lin = None if lin_vel is None else np.asarray(lin_vel, dtype=F)
        ang = None if ang_vel is None else np.asarray(ang_vel, dtype=F)
        c = self.commands
        # 1: the terms
        term, t64 = np.zeros((N, 4), F), np.zeros((N, 4), D)
        term[:, 0] = t64[:, 0] = 1.0
        given = [True, lin is not None, lin is not None, ang is not None]
        for k, (src, col) in enumerate(((lin, 0), (lin, 1), (ang, 2)), start=1):
            if src is not None:
                t64[:, k] = term64(c[:, col], src[:, col], cfg["sigma"])
                term[:, k] = t64[:, k].astype(F)
        total, total64 = np.zeros(N, F), np.zeros(N, D)
        for k in range(4):
            if given[k] and cfg["scale"][k] != 0:
                total = (total + (cfg["scale"][k] * term[:, k]).astype(F)).astype(F)
                total64 = total64 + D(cfg["scale"][k]) * t64[:, k]
        # 2: the boundary
        flags = np.where(steps == self.cmd_resample_time, BOUNDARY, 0).astype(np.int32)
        # 3: the curriculum's bookkeeping
        if cur is not None:
            tol, L, A = cur["tol"], cur["L"], cur["A"]
            nx, ny = 2 * L + 1, 2 * A + 1
            ok = d & (steps > cur["min_success"])
            ok &= np.abs((lin[:, 0] - c[:, 0]).astype(F)) < tol[0]
            ok &= np.abs((lin[:, 1] - c[:, 1]).astype(F)) < tol[1]
            ok &= np.abs((ang[:, 2] - c[:, 2]).astype(F)) < tol[2]
            flags[ok] |= SUCCESS
            for e in np.nonzero(ok)[0]:
                x, y = int(self.env_level[e, 0]) + L, int(self.env_level[e, 1]) + A
                for xx, yy in ((x, y), (x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                    if 0 <= xx < nx and 0 <= yy < ny:
                        self.hits[xx * ny + yy] += 1
        # 4: the reset
        self.cmd_resample_time[d] = 0
        now = np.where(d, 0, steps)
        # 5: the grid
        if cur is not None:
            self.curriculum_prob = update_grid(self.curriculum_prob, self.hits, cur["rate"])
            self.hits[:] = 0
            self.cum = cumulate(self.curriculum_prob)
        # 6: the resample, every environment on its own words
        ids = np.nonzero(now == self.cmd_resample_time)[0]
        if len(ids):
            w = philox_np(ids, self.cmd_draws[ids], 0, 2, self.key)
            v = philox_np(ids, self.cmd_draws[ids], 1, 2, self.key)
            u = [unit_np(x) for x in w] + [unit_np(v[0])]
            if cur is not None:
                g = draw_cells(self.cum, v[2])
                lv, av = split_cell(g, cur["L"], cur["A"], cur["order"])
                self.env_level[ids, 0], self.env_level[ids, 1] = lv, av
                cc = curriculum_commands(lv, av, u[0], u[1], u[2], cur["res"])
            else:
                cc = [uniform(cfg["lo"][k], cfg["span"][k], u[k]) for k in range(3)]
            gf = uniform(cfg["lo"][3], cfg["span"][3], u[3])
            still = u[4] < cfg["still"]
            self.commands[ids] = np.where(still[:, None], F(0.0), np.stack(cc, axis=1))
            self.gait_frequency[ids] = np.where(still, F(0.0), gf)
            self.cmd_resample_time[ids] += (cfg["rs_lo"] + ((v[1].astype(np.uint64) * np.uint64(cfg["rs_span"])) >> np.uint64(32))).astype(np.int32)
            self.cmd_draws[ids] += np.uint32(1)
            flags[ids] |= RESAMPLED
            self.last = {"ids": ids, "still": still, "cells": g if cur is not None else None}
        # 7: the outputs
        return {"term": term, "term64": t64, "total": total, "total64": total64, "commands": self.commands.copy(),
                "gait_frequency": self.gait_frequency.copy(), "flags": flags, "cmd_obs": (self.commands * cfg["obs_scale"][None, :]).astype(F)}

    def state(self):
        out = {"commands": self.commands, "gait_frequency": self.gait_frequency, "cmd_resample_time": self.cmd_resample_time, "cmd_draws": self.cmd_draws}
        if self.cfg["curriculum"] is not None:
            out.update({"env_level": self.env_level, "curriculum_prob": self.curriculum_prob, "hits": self.hits, "cum": self.cum})
        return out


# ---- kicks and pushes ------------------------------------------------------------------------------------------------------------
def disturb_config(kick_every, push_every, push_duration, kick_lin_vel=None, kick_ang_vel=None, push_force=None, push_torque=None,
                   scale_push_force=1.0, scale_push_torque=1.0):
    specs = []
    for s in (kick_lin_vel, kick_ang_vel, push_force, push_torque):
        if s is None or s.get("distribution", "none") == "none":
            specs.append(None)
            continue
        a, b = (float(x) for x in s["range"])
        specs.append({"dist": s["distribution"], "op": s["operation"], "a": F(a), "m": F(b) if s["distribution"] == "gaussian" else F(b - a)})
    return {"specs": specs, "kick_every": int(kick_every), "push_every": int(push_every), "push_duration": int(push_duration),
            "s_force": F(scale_push_force), "s_torque": F(scale_push_torque)}


def disturb_actions(step, kick_every, push_every, push_duration):
    """the modulo rule of t1.py:501, :508, :517"""
    act = KICK if step % kick_every == 0 else 0
    if step % push_every == 0:
        act |= PUSH_START
    elif step % push_every == push_duration:
        act |= PUSH_STOP
    return act


def draw(spec, key, e, step, i, wide=False):
    """the unit draw (u or z) of element i of environment e at common_step: philox4x32((e, step, i >> 1, 3), key), words (0, 1) for an even
    i, (2, 3) for an odd one; ``wide``: the gaussian in float64 on the same words"""
    wa, wb = pm.pair(tm.philox4x32((e, step, i >> 1, 3), key), i)
    if spec["dist"] == "gaussian":
        return pm.gaussian64(wa, wb) if wide else pm.gaussian32(wa, wb)
    return pm.unit(wa)


def disturb(cfg, N, seed, step, root_states, wide=False):
    """-> (actions, root_states after the kick, push_force [N,3], push_torque [N,3], push_obs [N,6]); the last three are None on a step
    that neither starts nor stops a push.  ``wide``: gaussian draws in float64, applied in float64 (what a test bounds the device against)"""
    key = (seed & M32, (seed >> 32) & M32)
    act = disturb_actions(step, cfg["kick_every"], cfg["push_every"], cfg["push_duration"])
    T = D if wide else F
    rs = np.array(root_states, dtype=F).astype(T)
    apply = (lambda x, s, r: (x * (T(s["a"]) + T(s["m"]) * T(r)) if s["op"] == "scaling" else x + (T(s["a"]) + T(s["m"]) * T(r)))) if wide else \
        (lambda x, s, r: pm.apply_noise(x, s, r))
    if act & KICK:
        for i in range(6):
            s = cfg["specs"][i // 3]
            if s is not None:
                for e in range(N):
                    rs[e, 7 + i] = apply(rs[e, 7 + i], s, draw(s, key, e, step, i, wide))
    push = None
    if act & (PUSH_START | PUSH_STOP):
        push = np.zeros((N, 6), T)
        if act & PUSH_START:
            for i in range(6, 12):
                s = cfg["specs"][2 + (i - 6) // 3]
                if s is not None:
                    for e in range(N):
                        push[e, i - 6] = apply(T(0.0), s, draw(s, key, e, step, i, wide))
    if push is None:
        return act, rs, None, None, None
    obs = np.concatenate([(push[:, :3] * T(cfg["s_force"])).astype(T), (push[:, 3:] * T(cfg["s_torque"])).astype(T)], axis=1)
    return act, rs, push[:, :3].copy(), push[:, 3:].copy(), obs
