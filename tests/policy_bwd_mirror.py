"""The backward pass through the actor and the critic of a training iteration on the motion tracker in NumPy: the
statement of record of ``csrc/gmr_tracker_policy_bwd.hip``.  What ``loss.backward()`` (runner.py:163) computes behind the gradients at
the outputs of the reference's ``ActorCritic`` (booster_gym/utils/model.py:9-27).  The notation is ``policy_mirror``'s: layer ``l = 0 .. L``
maps ``width[l] -> width[l + 1]`` with ``W_l [width[l + 1], width[l]]``; ``hidden[l]`` is the activation after layer ``l``'s ELU; ``a_0`` is
the input row (the critic's: ``obs`` and ``priv`` side by side), ``a_l = hidden[l - 1]``.  Given ``g_L`` (``grad_loc [rows, A]`` or
``grad_values [rows]``):

    for l = L .. 1:   dA[m, i] = sum_j g_l[m, j] W_l[j, i]            the sum from +0 over j in rising order, fused multiply-adds
                      g_{l-1}[m, i] = dA[m, i] * d(hidden[l-1][m, i])  d(y) = y > 0 ? 1 : y + 1
    for every l:      dW_l[j, i] = sum_m g_l[m, j] a_l[m, i]           db_l[j] = sum_m g_l[m, j]
    dA_0 is not formed.

``d`` is ELU's derivative taken from its OUTPUT: the forward stores ``y = expm1(z)`` and ``exp(z) = y + 1`` up to one rounding (torch takes
``exp`` of the saved input; the difference goes into the measured bound of the fixture).

THE SUMS OVER ROWS: rows are cut into chunks of ``CHUNK`` (``GMR_POLICY_BWD_CHUNK``, a multiple of 32).  Inside a chunk the sum is one chain
of fused multiply-adds from +0 over the rows in rising order, in ``dtype`` (``db``: the chain of ``fma(g, 1, .)``, that is of additions);
across chunks the partial sums are added in float64, in rising chunk order, and rounded to ``dtype`` once.

    fma(a, b, c, dtype)                  float32: the exact product and the sum formed in float64 and rounded to float32 (the product of two
                                         float32 is exact in float64; the second rounding differs from a fused one only on a tie of the
                                         float64 sum); float64: a * b + c
    elu_slope(y)                         d(y)
    sweep(layers, hidden, g_out)         -> [g_0, .., g_{L-1}], the ``delta`` list
    row_sums(g, a, rows, chunk)          -> (dW, db) of one layer
    backward(x, layers, hidden, g_out)   -> {"delta", "dW", "db"}
    upstream(rows, cols, stream)         the upstream gradients of the fixture, from a Philox generator written out here
    SEEDED                               the wrong variants the host test must tell from the statement

``dtype=np.float64`` evaluates the same statement in float64 on the same float32 inputs: the yardstick of the device test.  The device sums
the sweep's j in an order of its own (N18 of include/gmr_hip.h) with one rounding per term; both stay within the bound measured from this
mirror's own float32 error.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_mirror as pol  # noqa: E402
import proprio_mirror as pm  # noqa: E402
import tracker_mirror as tm  # noqa: E402

F = np.float32
D = np.float64
CHUNK = 256                              # GMR_POLICY_BWD_CHUNK
MAX_ROWS = 131072                        # GMR_POLICY_BWD_MAX_ROWS
SEEDED = ("slope_y", "untransposed", "priv_obs", "last_chunk", "db_last_tile")


def fma(a, b, c, dtype):
    return (np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D)).astype(dtype)


def elu_slope(y, wrong=None):
    one = np.ones_like(y)
    return np.where(y > 0, one, y if wrong == "slope_y" else y + one).astype(y.dtype)


def sweep(layers, hidden, g_out, dtype=F, wrong=None):
    """``layers``: the ``(W, b)`` pairs of one network, ``hidden``: the forward's list, ``g_out [rows, width[L + 1]]`` -> ``[g_0 .. g_{L-1}]``"""
    L = len(layers) - 1
    g = np.asarray(g_out, F).astype(dtype).reshape(len(g_out), -1)
    delta = [None] * L
    for l in range(L, 0, -1):
        W = np.asarray(layers[l][0], F).astype(dtype)
        if wrong == "untransposed" and W.shape[0] == W.shape[1]:
            W = W.T
        acc = np.zeros((g.shape[0], W.shape[1]), dtype)
        for j in range(W.shape[0]):
            acc = fma(g[:, j:j + 1], W[j][None, :], acc, dtype)
        g = acc * elu_slope(np.asarray(hidden[l - 1], F).astype(dtype), wrong)
        delta[l - 1] = g
    return delta


def chunks(rows, chunk=CHUNK):
    return (rows + chunk - 1) // chunk


def row_sums(g, a, dtype=F, chunk=CHUNK, wrong=None):
    """``g [rows, N]``, ``a [rows, K]`` of ``dtype`` -> ``(dW [N, K], db [N])``"""
    rows = g.shape[0]
    n = chunks(rows, chunk)
    dW, db = np.zeros((g.shape[1], a.shape[1]), D), np.zeros(g.shape[1], D)
    for c in range(n):
        lo, hi = c * chunk, min(rows, (c + 1) * chunk)
        pw, pb = np.zeros(dW.shape, dtype), np.zeros(db.shape, dtype)
        for m in range(lo, hi):
            pw = fma(g[m][:, None], a[m][None, :], pw, dtype)
            if not (wrong == "db_last_tile" and m >= (rows - 1) // pol.TILE * pol.TILE):
                pb = fma(g[m], dtype(1), pb, dtype)
        if wrong == "last_chunk" and c == n - 1 and n > 1:
            continue
        dW, db = dW + pw.astype(D), db + pb.astype(D)                # float64, rising chunk order
    return dW.astype(dtype), db.astype(dtype)


def backward(x, layers, hidden, g_out, dtype=F, chunk=CHUNK, wrong=None):
    """``x [rows, width[0]]``: the input rows (the critic's: ``concatenate([obs, priv], 1)``) -> ``{"delta": [g_0 ..], "dW": [..], "db": [..]}``"""
    L = len(layers) - 1
    delta = sweep(layers, hidden, g_out, dtype, wrong)
    gs = delta + [np.asarray(g_out, F).astype(dtype).reshape(len(g_out), -1)]
    out = {"delta": delta, "dW": [], "db": []}
    for l in range(L + 1):
        a = np.asarray(x if l == 0 else hidden[l - 1], F).astype(dtype)
        dW, db = row_sums(gs[l], a, dtype, chunk, wrong)
        out["dW"].append(dW)
        out["db"].append(db)
    return out


class Backward:
    """The two calls of one tracker on the shapes of a ``policy_mirror.Policy``."""

    def __init__(self, policy, chunk=CHUNK):
        self.p, self.chunk = policy, chunk

    def act(self, params, obs, hidden, grad_loc, wrong=None):
        _, _, layers = pol.split(params, len(self.p.critic))
        return backward(obs, layers, hidden, grad_loc, self.p.T, self.chunk, wrong)

    def values(self, params, obs, priv, hidden, grad_values, wrong=None):
        _, layers, _ = pol.split(params, len(self.p.critic))
        parts = [np.asarray(obs, F)] + ([np.asarray(priv, F)] if self.p.P else [])
        x = np.concatenate(parts[::-1] if wrong == "priv_obs" else parts, axis=1)      # (wrong: the columns of dW_0 in (priv, obs) order)
        return backward(x, layers, hidden, np.asarray(grad_values, F).reshape(-1, 1), self.p.T, self.chunk, wrong)


# ---- the upstream gradients of the fixture (tests/golden/make_policy_bwd_golden.py hands them to torch.autograd.backward) ------------
UPSTREAM_KEY = (20261020, 7)
GOLDEN_STRIDE = 4                        # the fixture keeps rows 0, 4, 8, .. of every dW


def upstream(rows, cols, stream):
    """``f32[rows, cols]`` in [-1, 1) / rows: element i of stream ``stream`` (0: grad_loc, 1: grad_values) is word ``i & 3`` of
    philox4x32((i >> 2, stream, 0, 0), UPSTREAM_KEY), its top 24 bits as a fraction u, (2 u - 1) / rows"""
    n = rows * cols
    out = np.empty(n, F)
    for c in range((n + 3) // 4):
        w = tm.philox4x32((c, stream, 0, 0), UPSTREAM_KEY)
        for j in range(min(4, n - 4 * c)):
            out[4 * c + j] = (F(2.0) * pm.unit(w[j]) - F(1.0)) / F(rows)
    return out.reshape(rows, cols)
