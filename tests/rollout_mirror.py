"""The rollout of a training iteration on the motion tracker in NumPy: the statement of record of
``csrc/gmr_tracker_rollout.hip``.  What the reference's runner does between the outputs of a step and the tensors its loss reads: the six
``update_data`` calls of a step (booster_gym/utils/runner.py:107-108, :115-118), the bootstrap of the timed-out rewards (:135),
``discount_values`` (utils/utils.py:33-44), the returns (:144) and the normalisation (:145).  Every value is float32 and NumPy rounds after
each operator, so the device reproduces these lines bit for bit; the two sums behind the mean and the deviation are float64 in the
association stated at :func:`sums`.

    Rollout(H, N, O, P, A, gamma, lam)       the six arrays, record(n, ...) and advantages(values, last_values, normalize)
    advantages(...)                          the same on arrays of the caller's
"""
import numpy as np

F = np.float32
D = np.float64
ENVS = 64                                # environments per group of the partial sums (GMR_ROLLOUT_ENVS)
FOLD = 64                                # groups up to which the normalisation launch chains the partials itself (GMR_ROLLOUT_FOLD)
EPS = F(1e-8)


def sums(adv):
    """S1 = the sum of (double)adv and S2 = the sum of (double)adv * (double)adv (each product exact in double) over ``adv [H, N]``:
    per environment from +0 in falling t; the environments of a group of ENVS consecutive ones (an absent one counts +0) by the balanced
    tree x[i] = x[i] + x[i + s] for s = 1, 2, 4, ..; the groups from +0 in rising order"""
    H, N = adv.shape
    G = (N + ENVS - 1) // ENVS
    out = []
    for power in (1, 2):
        lane = np.zeros(G * ENVS, D)
        for t in range(H - 1, -1, -1):
            x = adv[t].astype(D)
            lane[:N] = lane[:N] + (x if power == 1 else x * x)
        x = lane.reshape(G, ENVS)
        while x.shape[1] > 1:
            x = x[:, 0::2] + x[:, 1::2]
        S = D(0.0)
        for g in range(G):
            S = S + x[g, 0]
        out.append(S)
    return out[0], out[1]


def advantages(rewards, dones, time_outs, values, last_values, gamma, lam, normalize=True):
    """``rewards f32[H, N]`` is rewritten in place where ``time_outs`` (runner.py:135).  Returns ``advantages``, ``returns`` and, with
    ``normalize``, ``normalized`` and ``stats = (S1, S2, mean, std)`` as float64."""
    H, N = rewards.shape
    assert rewards.dtype == F and values.dtype == F and last_values.dtype == F and values.shape == (H, N) and last_values.shape == (N,)
    to = np.asarray(time_outs) != 0
    rewards[to] = values[to]                                           # 1 (runner.py:135)
    nn = F(1.0) - ((np.asarray(dones) != 0) | to).astype(F)            # 2 (runner.py:138, utils.py:37)
    g, gl = F(float(gamma)), F(float(gamma) * float(lam))              # 3 (the product in double)
    adv = np.zeros((H, N), F)
    last = np.zeros(N, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(H - 1, -1, -1):                                 # 4 (utils.py:36-43)
            nv = last_values if t == H - 1 else values[t + 1]
            delta = (rewards[t] + (g * nn[t]) * nv) - values[t]
            last = delta + (gl * nn[t]) * last
            adv[t] = last
        out = {"advantages": adv, "returns": values + adv}            # 5 (runner.py:144)
        if normalize:                                                  # 6 (runner.py:145)
            M = D(H * N)
            if H * N < 2:
                raise ValueError("normalize needs two advantages")
            S1, S2 = sums(adv)
            mean = S1 / M
            std = np.sqrt((S2 - S1 * S1 / M) / (M - D(1.0)))
            out["normalized"] = (adv - F(mean)) / (F(std) + EPS)
            out["stats"] = np.array([S1, S2, mean, std], D)
    return out


class Rollout:
    def __init__(self, H, N, O, P, A, gamma, lam):
        if H < 1 or O < 1 or A < 1 or P < 0 or not (0.0 <= gamma <= 1.0) or not (0.0 <= lam <= 1.0):
            raise ValueError("rollout configuration")
        self.H, self.N, self.O, self.P, self.A, self.gamma, self.lam = H, N, O, P, A, float(gamma), float(lam)
        self.io = {"obs": np.zeros((H, N, O), F), "priv": np.zeros((H, N, P), F) if P else None, "actions": np.zeros((H, N, A), F),
                   "rewards": np.zeros((H, N), F), "dones": np.zeros((H, N), np.uint8), "time_outs": np.zeros((H, N), np.uint8)}

    def record(self, n, obs=None, priv=None, actions=None, reward=None, done=None, time_outs=None):
        """slot n of each array receives the rows handed in; None leaves the slot as it is; the two words become 0 / 1 bytes"""
        if not 0 <= n < self.H:
            raise ValueError("slot")
        for k, a in (("obs", obs), ("priv", priv), ("actions", actions), ("rewards", reward)):
            if a is not None:
                self.io[k][n] = np.asarray(a, F)
        for k, a in (("dones", done), ("time_outs", time_outs)):
            if a is not None:
                self.io[k][n] = (np.asarray(a) != 0).astype(np.uint8)

    def advantages(self, values, last_values, normalize=True):
        return advantages(self.io["rewards"], self.io["dones"], self.io["time_outs"], values, last_values, self.gamma, self.lam, normalize)
