"""The start and the end of an episode on the motion tracker in NumPy float32: the statement of record of
``csrc/gmr_tracker_episode.hip``.  One rounding per operation -- every value is float32 and NumPy rounds after each operator --, so the device
reproduces these lines bit for bit except the two yaw components of a reset quaternion, whose ``sinf`` and ``cosf`` differ between
implementations by an ulp or two (``yaw64`` is what a test measures the device against), and a gaussian draw (``proprio_mirror.gaussian64``).
The sums of the finished episodes are float64 in the association stated at :func:`Rewards.step`.

    reset_config(...), Resets(cfg, N, R, seed)     the reset counters and the call that writes the simulator's rows: reset
    reward_config(...), Rewards(cfg, N)            the reward of a step, the episode sums and the accumulators: step, stats
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import commands_mirror as cm  # noqa: E402
import feet_mirror as fm  # noqa: E402
import proprio_mirror as pm  # noqa: E402
import tracker_mirror as tm  # noqa: E402

F = np.float32
D = np.float64
M32 = 0xFFFFFFFF
DOMAIN = 4                               # word 3 of a reset's Philox counter
SPECS = ("init_dof_pos", "init_base_pos_xy", "init_base_lin_vel_xy")
TERMS = ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel")
LINK_TERMS = ("link_pos", "link_rot", "link_vel", "link_ang_vel")
BLOCKS = ("terms", "links", "proprio", "feet", "commands")             # column order; then the caller's columns
BLOCK_BITS = {"terms": 1, "links": 2, "proprio": 4, "feet": 8, "commands": 16}
WIDTH = {"terms": 6, "links": 4, "proprio": 14, "feet": 8, "commands": 4}
LOCOMOTION, IMITATION = 1, 2
DONE_TIME_OUT, CMD_BOUNDARY = 4, 1
ENVS = 16                                # environments per workgroup of the reward launch
MAX_EXTRA, MAX_COLS = 16, 52


# ---- A. reset states ---------------------------------------------------------------------------------------------------------------
def reset_config(base_init_state, default_dof_pos, env_origins=None, init_dof_pos=None, init_base_pos_xy=None, init_base_lin_vel_xy=None,
                 yaw_range=(0.0, 2.0 * np.pi), decimation=0, use_terrain=True):
    """float32 scalars; the span of a uniform is formed in double and rounded once"""
    specs = []
    for s in (init_dof_pos, init_base_pos_xy, init_base_lin_vel_xy):
        if s is None or s.get("distribution", "none") == "none":
            specs.append(None)
            continue
        a, b = (float(x) for x in s["range"])
        specs.append({"dist": s["distribution"], "op": s["operation"], "a": F(a), "m": F(b) if s["distribution"] == "gaussian" else F(b - a)})
    yaw = None if yaw_range is None else (F(float(yaw_range[0])), F(float(yaw_range[1]) - float(yaw_range[0])))
    return {"base": np.asarray(base_init_state, dtype=F).copy(), "default": np.asarray(default_dof_pos, dtype=F).copy(),
            "origins": None if env_origins is None else np.asarray(env_origins, dtype=F)[:, :2].copy(), "specs": specs, "yaw": yaw,
            "decimation": int(decimation), "use_terrain": bool(use_terrain)}


def reset_words(key, e, n, i):
    """the two Philox words of element i of environment e at its reset count n: an even i takes words (0, 1), an odd i words (2, 3)"""
    return pm.pair(tm.philox4x32((e, n, i >> 1, DOMAIN), key), i)


def reset_words_np(key, e, n, i):
    """reset_words on arrays of environments and reset counts"""
    w = cm.philox_np(e, n, i >> 1, DOMAIN, key)
    return (w[2], w[3]) if i & 1 else (w[0], w[1])


def unit_draw(spec, key, e, n, i, wide=False):
    wa, wb = reset_words(key, e, n, i)
    if spec["dist"] == "gaussian":
        return pm.gaussian64(wa, wb) if wide else pm.gaussian32(wa, wb)
    return pm.unit(wa)


def yaw_angle(yaw, u):
    """yaw = (float)lo + (float)(hi - lo) * u, then half = 0.5f * yaw"""
    return F(F(0.5) * F(yaw[0] + F(yaw[1] * F(u))))


def yaw_quat(half):
    """(0, 0, sin(half), cos(half)) in float32 from a float64 evaluation: what the device's sinf / cosf are measured against"""
    return np.array([0.0, 0.0, np.sin(D(half)), np.cos(D(half))], dtype=F)


def yaw64(half):
    return np.sin(D(half)), np.cos(D(half))


class Resets:
    def __init__(self, cfg, N, R, seed=0, terrain=None):
        self.cfg, self.N, self.R = cfg, int(N), int(R)
        self.key = (seed & M32, (seed >> 32) & M32)
        self.terrain = terrain               # feet_mirror.terrain(...) or None: the plane
        self.reset_draws = np.zeros(N, np.uint32)
        self.ignored = 0

    def reset(self, root_states, dof_pos, dof_vel, mask=None, env_ids=None, delay_steps=None, episode_steps=None, init_root_states=None,
              init_dof_pos=None, init_dof_vel=None, variates=None):
        """entry i -- environment env_ids[i], or i -- with its mask set, in the order of t1.py:319-340, :311, :316; the arrays are written
        in place.  ``variates``: {"dof": [n, R], "xy": [n, 2], "yaw": [n], "vel": [n, 2]} unit draws by list position that take the place
        of the Philox draws (how the fixture's recorded variates are replayed).  Returns the ids dropped and the half angles of the yaws
        drawn ({environment: half})."""
        c, R, key = self.cfg, self.R, self.key
        n = self.N if env_ids is None else len(env_ids)
        ids = np.arange(n) if env_ids is None else np.asarray(env_ids, dtype=np.int64)
        dropped, halves = 0, {}
        for i in range(n):
            if mask is not None and not mask[i]:
                continue
            e = int(ids[i])
            if not 0 <= e < self.N:
                dropped += 1
                continue
            nd = int(self.reset_draws[e])

            def draw(spec, elem, name, k):
                if variates is not None:
                    return F(np.asarray(variates[name])[i][k] if name != "yaw" else np.asarray(variates[name])[i])
                return unit_draw(spec, key, e, nd, elem)
            # 1: the dofs
            q = (c["default"] if init_dof_pos is None else np.asarray(init_dof_pos, dtype=F)[i]).copy()
            if c["specs"][0] is not None:
                for j in range(R):
                    q[j] = pm.apply_noise(q[j], c["specs"][0], draw(c["specs"][0], j, "dof", j))
            dof_pos[e] = q
            dof_vel[e] = 0 if init_dof_vel is None else np.asarray(init_dof_vel, dtype=F)[i]
            # 2: the root row, its origin, the randomised xy
            r = (c["base"] if init_root_states is None else np.asarray(init_root_states, dtype=F)[i]).copy()
            if c["origins"] is not None:
                r[0] = F(r[0] + c["origins"][e, 0])
                r[1] = F(r[1] + c["origins"][e, 1])
            if c["specs"][1] is not None:
                for k in range(2):
                    r[k] = pm.apply_noise(r[k], c["specs"][1], draw(c["specs"][1], R + k, "xy", k))
            # 3: the terrain
            if c["use_terrain"]:
                with np.errstate(invalid="ignore"):
                    r[2] = F(r[2] + fm.heights(self.terrain, r[None, :2])[0][0])
            # 4: the yaw
            if c["yaw"] is not None:
                u = F(np.asarray(variates["yaw"])[i]) if variates is not None else pm.unit(reset_words(key, e, nd, R + 2)[0])
                halves[e] = yaw_angle(c["yaw"], u)
                r[3:7] = yaw_quat(halves[e])
            # 5: the planar velocity
            if init_root_states is None:
                r[7:9] = 0
            if c["specs"][2] is not None:
                for k in range(2):
                    r[7 + k] = pm.apply_noise(r[7 + k], c["specs"][2], draw(c["specs"][2], R + 3 + k, "vel", k))
            root_states[e] = r
            # 6, 7, 8
            if c["decimation"] > 0 and delay_steps is not None:
                delay_steps[e] = (int(reset_words(key, e, nd, R + 5)[0]) * c["decimation"]) >> 32
            if episode_steps is not None:
                episode_steps[e] = 0
            self.reset_draws[e] = nd + 1
        self.ignored += dropped
        return dropped, halves


# ---- B, C. the reward and the episode statistics -----------------------------------------------------------------------------------
def reward_config(blocks, weights, extra_weights=(), groups=None, group_weight=(1.0, 1.0), only_positive=(False, False), stats=False):
    """``blocks``: the configured blocks, any order; ``weights``: {block: the weights of its columns}.  -> the columns in the fixed order"""
    blocks = [b for b in BLOCKS if b in blocks]
    col_block, w = [], []
    for b in blocks:
        wb = np.asarray(weights[b], dtype=F)
        assert wb.shape == (WIDTH[b],), (b, wb.shape)
        col_block += [(b, j) for j in range(WIDTH[b])]
        w += list(wb)
    E = len(extra_weights)
    col_block += [("extra", j) for j in range(E)]
    w += [F(x) for x in extra_weights]
    C = len(w)
    assert E <= MAX_EXTRA and C <= MAX_COLS
    if groups is None:
        groups = [IMITATION if b in ("terms", "links") else LOCOMOTION for b, _ in col_block]
    assert len(groups) == C and all(0 <= g <= 3 for g in groups)
    return {"blocks": blocks, "cols": col_block, "w": np.asarray(w, dtype=F), "C": C, "E": E, "groups": np.asarray(groups, dtype=np.uint8),
            "gw": np.asarray(group_weight, dtype=F), "pos": tuple(bool(x) for x in only_positive), "stats": bool(stats)}


class Rewards:
    def __init__(self, cfg, N):
        self.cfg, self.N = cfg, int(N)
        K = cfg["C"] + 1
        self.ep_steps = np.zeros(N, np.int32)
        self.ep_sum = np.zeros((N, K), F)
        self.fin_count, self.fin_steps = 0, 0
        self.fin_sum = np.zeros(K, D)
        self.started = False

    def step(self, terms, done=None, flags=None):
        """``terms``: {block or "extra": [N, width] or None}.  Per environment, in column order:
          1. scaled_c = w_c * term_c; a column whose weight is zero or whose array is absent is +0 and stays out
          2. S_g = the sum of the scaled columns of group g that are in, from +0 in rising c
          3. only_positive[g]: S_g < 0 ? 0 : S_g (a NaN stays)
          4. reward = gw_0 * S_0 + gw_1 * S_1, each product rounded, then the sum
          5. reset = done != 0, time_outs = ((done & 4) | (flags & 1)) != 0
        With statistics: ep_steps += 1 except in the first call; ep_sum += (reward, scaled) in float32; for a reset environment fin_count
        += 1, fin_steps += ep_steps, its row joins fin_sum, then ep_steps = 0 and ep_sum = 0.  fin_sum: the workgroup of the environments
        16 w .. 16 w + 15 forms p = +0, p = p + (double)ep_sum[e][k] over its reset environments in rising e; then fin_sum[k] = fin_sum[k]
        + p_w over the workgroups with a reset environment in rising w."""
        c, N = self.cfg, self.N
        C = c["C"]
        scaled = np.zeros((N, C), F)
        inn = np.zeros(C, bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for k, (b, j) in enumerate(c["cols"]):
                a = terms.get(b)
                if a is None or c["w"][k] == 0:
                    continue
                inn[k] = True
                scaled[:, k] = (c["w"][k] * np.asarray(a, dtype=F)[:, j]).astype(F)
            S = np.zeros((N, 2), F)
            for k in range(C):
                for g in (0, 1):
                    if inn[k] and c["groups"][k] & (1 << g):
                        S[:, g] = (S[:, g] + scaled[:, k]).astype(F)
            for g in (0, 1):
                if c["pos"][g]:
                    S[:, g] = np.where(S[:, g] < 0, F(0), S[:, g])
            reward = ((c["gw"][0] * S[:, 0]).astype(F) + (c["gw"][1] * S[:, 1]).astype(F)).astype(F)
        dn = np.zeros(N, np.int32) if done is None else np.asarray(done, dtype=np.int32)
        fl = np.zeros(N, np.int32) if flags is None else np.asarray(flags, dtype=np.int32)
        reset = (dn != 0)
        out = {"reward": reward, "scaled": scaled, "group_total": S, "reset": reset.astype(np.int32),
               "time_outs": (((dn & DONE_TIME_OUT) | (fl & CMD_BOUNDARY)) != 0).astype(np.int32)}
        if c["stats"]:
            if self.started:
                self.ep_steps += 1
            self.started = True
            with np.errstate(invalid="ignore", over="ignore"):
                self.ep_sum = (self.ep_sum + np.concatenate([reward[:, None], scaled], axis=1)).astype(F)
            self.fin_count += int(reset.sum())
            self.fin_steps += int(self.ep_steps[reset].sum())
            for w in range((N + ENVS - 1) // ENVS):
                es = [e for e in range(w * ENVS, min(N, (w + 1) * ENVS)) if reset[e]]
                if not es:
                    continue
                p = np.zeros(C + 1, D)
                for e in es:
                    p = p + self.ep_sum[e].astype(D)
                with np.errstate(invalid="ignore"):
                    self.fin_sum = self.fin_sum + p
            self.ep_steps[reset] = 0
            self.ep_sum[reset] = 0
        return out

    def stats(self, clear=True):
        """the three accumulators -> (episodes, steps, sums f64[C + 1]); cleared"""
        out = (self.fin_count, self.fin_steps, self.fin_sum.copy())
        if clear:
            self.fin_count, self.fin_steps = 0, 0
            self.fin_sum = np.zeros_like(self.fin_sum)
        return out

    @staticmethod
    def means(episodes, steps, sums):
        """the Recorder's ``_mean`` (recorder.py:86-90): 0.0 for no episode"""
        if episodes == 0:
            return 0.0, np.zeros(len(sums))
        return steps / episodes, np.asarray(sums, dtype=D) / episodes
