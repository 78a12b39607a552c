"""The forward pass of the actor and the critic of a training iteration on the motion tracker in NumPy: the statement
of record of ``csrc/gmr_tracker_policy.hip``.  What the reference's ``ActorCritic`` (booster_gym/utils/model.py) computes without autograd:
``model.act(obs).loc`` and ``.sample()`` (:29-32) and ``model.est_value(obs, privileged_obs)`` (:34-36).  A network is an MLP ``in -> h_1 -> ..
-> h_L -> out``: ``y = x W^T + b`` with ``W [out, in]``, the layout of ``torch.nn.Linear``, ELU after every hidden layer and none after the
last.  Every value is ``dtype`` and NumPy rounds after each operator.

    linear(x, W, b)                      b_j + sum_k x_k W_jk, the sum from +0 over k in rising order, the bias last
    elu(z)                               z > 0 ? z : expm1(z)
    forward(x, layers)                   -> (the output, the activations after every ELU)
    sizes(O, P, A, actor, critic)        the element counts of the parameter list: logstd, the critic's (W, b) pairs, the actor's
    draws(key, counts, A)                the Gaussian draw of every (environment, action): the tracker's Box-Muller (proprio_mirror) on the
                                         Philox words of element i of environment e at its count, counter domain DRAW_ACTION
    Policy(...)                          the counts and the two calls: act, values
    golden_parameters(O, P, A)           the parameters of the fixture tests/golden/policy_golden.npz, from a generator written out here

``dtype=np.float64`` evaluates the same statement in float64 on the same float32 inputs: the yardstick of the device test.  The device sums
in an order of its own (a function of the layer's shape alone) with one rounding per term; both stay within the bound measured from this
mirror's own float32 error.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proprio_mirror as pm  # noqa: E402
import tracker_mirror as tm  # noqa: E402

F = np.float32
D = np.float64
DRAW_ACTION = 5                          # word 3 of the Philox counter (gmr_tracker_dev.h)
TILE, MAX_HIDDEN, WIDTH_STEP, MAX_WIDTH, MAX_IN, MAX_ACT = 32, 4, 32, 256, 512, 32
ACTOR_HIDDEN, CRITIC_HIDDEN = (256, 128, 128), (256, 256, 128)          # model.py:9-26


def elu(z):
    with np.errstate(over="ignore"):
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0))).astype(z.dtype)


def linear(x, W, b):
    """``x [rows, in]``, ``W [out, in]``, ``b [out]`` of one dtype -> ``[rows, out]``: every product and every sum rounded, k rising"""
    acc = np.zeros((x.shape[0], W.shape[0]), x.dtype)
    for k in range(x.shape[1]):
        acc = acc + x[:, k:k + 1] * W[None, :, k]
    return acc + b[None, :]


def forward(x, layers, dtype=F):
    """``layers``: the ``(W, b)`` pairs of one network -> ``(out [rows, out], [the activations after every ELU])``"""
    x = np.asarray(x, F).astype(dtype)
    hidden = []
    for l, (W, b) in enumerate(layers):
        z = linear(x, np.asarray(W, F).astype(dtype), np.asarray(b, F).astype(dtype).reshape(-1))
        if l == len(layers) - 1:
            return z, hidden
        x = elu(z)
        hidden.append(x)


def widths(O, P, A, actor=ACTOR_HIDDEN, critic=CRITIC_HIDDEN):
    return {"critic": (O + P,) + tuple(critic) + (1,), "actor": (O,) + tuple(actor) + (A,)}


def shapes(O, P, A, actor=ACTOR_HIDDEN, critic=CRITIC_HIDDEN):
    """the shapes of the parameter list in the order of ``model.parameters()``: logstd, the critic, the actor"""
    out = [(A,)]
    w = widths(O, P, A, actor, critic)
    for net in ("critic", "actor"):
        for l in range(len(w[net]) - 1):
            out += [(w[net][l + 1], w[net][l]), (w[net][l + 1],)]
    return out


def sizes(O, P, A, actor=ACTOR_HIDDEN, critic=CRITIC_HIDDEN):
    return tuple(int(np.prod(s)) for s in shapes(O, P, A, actor, critic))


def split(params, n_critic):
    """the parameter list -> (logstd, the critic's pairs, the actor's pairs); ``n_critic``: the critic's hidden layers"""
    params = list(params)
    cut = 1 + 2 * (n_critic + 1)
    pairs = lambda p: [(p[i], p[i + 1]) for i in range(0, len(p), 2)]      # noqa: E731
    return params[0], pairs(params[1:cut]), pairs(params[cut:])


def draws(key, counts, A):
    """-> ``(r f32[N, A], r f64[N, A])``: the draw in float32 as the kernel forms it, and the same draw in float64 on the same words"""
    N = len(counts)
    r32, r64 = np.zeros((N, A), F), np.zeros((N, A), D)
    for e in range(N):
        for i in range(A):
            wa, wb = pm.pair(tm.philox4x32((e, int(counts[e]), i >> 1, DRAW_ACTION), key), i)
            r32[e, i], r64[e, i] = pm.gaussian32(wa, wb), pm.gaussian64(wa, wb)
    return r32, r64


class Policy:
    """The two networks of one tracker: the shapes, the seed's key and one count per environment."""

    def __init__(self, O, P, A, actor=ACTOR_HIDDEN, critic=CRITIC_HIDDEN, num_envs=1, seed=0, dtype=F):
        assert O >= 1 and P >= 0 and O + P <= MAX_IN and 1 <= A <= MAX_ACT
        for h in (actor, critic):
            assert 1 <= len(h) <= MAX_HIDDEN and all(WIDTH_STEP <= x <= MAX_WIDTH and x % WIDTH_STEP == 0 for x in h)
        self.O, self.P, self.A, self.actor, self.critic, self.N, self.T = O, P, A, tuple(actor), tuple(critic), int(num_envs), dtype
        self.key = (seed & tm.M32, (seed >> 32) & tm.M32)
        self.counts = np.zeros(self.N, np.uint32)

    def act(self, params, obs, sample=True):
        """-> ``{"loc", "hidden"}`` and with ``sample`` ``"actions" = loc + exp(logstd) * r`` (and ``"noise"``, that product); sampling
        takes a row per environment and advances every count"""
        logstd, _, layers = split(params, len(self.critic))
        loc, hidden = forward(obs, layers, self.T)
        out = {"loc": loc, "hidden": hidden}
        if sample:
            assert loc.shape[0] == self.N
            r32, r64 = draws(self.key, self.counts, self.A)
            r = r32 if self.T is F else r64
            out["noise"] = np.exp(np.asarray(logstd, F).astype(self.T).reshape(-1))[None, :] * r
            out["actions"] = loc + out["noise"]
            out["r"] = r64
            self.counts = self.counts + np.uint32(1)
        return out

    def values(self, params, obs, priv=None):
        """-> ``{"values", "hidden"}``; the critic's input is ``(obs, priv)`` side by side (model.py:35)"""
        _, layers, _ = split(params, len(self.critic))
        x = np.asarray(obs, F) if self.P == 0 else np.concatenate([np.asarray(obs, F), np.asarray(priv, F)], axis=1)
        v, hidden = forward(x, layers, self.T)
        return {"values": v[:, 0], "hidden": hidden}


# ---- the parameters of the fixture (tests/golden/make_policy_golden.py fills the reference's state_dict with them) ------------------
GOLDEN_KEY = (20261020, 6)
GOLDEN_COLS = (5, 2, 3)                  # O, P, A
GOLDEN_ROWS = 70


def golden_uniform(tensor, n):
    """``n`` float32 numbers in [-1, 1): element i of tensor ``tensor`` is word ``i & 3`` of philox4x32((i >> 2, tensor, 0, 0), GOLDEN_KEY),
    its top 24 bits as a fraction u, 2 u - 1"""
    out = np.empty(n, F)
    for c in range((n + 3) // 4):
        w = tm.philox4x32((c, tensor, 0, 0), GOLDEN_KEY)
        for j in range(min(4, n - 4 * c)):
            out[4 * c + j] = F(2.0) * pm.unit(w[j]) - F(1.0)
    return out


def golden_parameters(O=GOLDEN_COLS[0], P=GOLDEN_COLS[1], A=GOLDEN_COLS[2]):
    """The parameter list of the reference's model at ``(O, P, A)``: tensor t is ``golden_uniform(t, size)`` times ``1 / sqrt(fan_in)`` (the
    first layers: times 1, so that the hidden activations reach both branches of the ELU and some ``|loc|`` pass 1), which is about the
    magnitude of torch's default initialisation; logstd is ``-1.5 + 0.5 u``."""
    out = []
    for t, shape in enumerate(shapes(O, P, A)):
        u = golden_uniform(t, int(np.prod(shape)))
        if t == 0:
            out.append((F(-1.5) + F(0.5) * u).astype(F))
            continue
        fan_in = shape[1] if len(shape) == 2 else shapes(O, P, A)[t - 1][1]
        scale = F(1.0) if fan_in <= O + P else F(1.0 / np.sqrt(D(fan_in)))
        out.append((u * scale).astype(F).reshape(shape))
    return out
