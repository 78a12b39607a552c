"""The PPO loss head of a training iteration on the motion tracker in NumPy: the statement of record of
``csrc/gmr_tracker_loss.hip``.  What the reference's runner does between the outputs of its two networks and its optimiser:
``old_actions_log_prob`` (booster_gym/utils/runner.py:123-125), the value, surrogate, bound and entropy terms and their sum (:146-161,
utils/utils.py:47-52), the backward pass of that sum down to ``loc``, ``logstd`` and ``values`` (what :163 delivers at the outputs of the
networks), the KL between the old and the new policy (:168-174) and the learning-rate rule (:175-178).  Every value is float32 and NumPy
rounds after each operator -- the exp and the log behind the per-column quantities are formed in double and rounded once, the exp of the
row's ratio is the float32 library's --; the sums over rows are float64 in the association stated at :func:`sums`.

    log_prob(loc, logstd, actions)                     runner.py:123-125, one float32 per row
    loss(cfg, lr, loc, logstd, actions, ...)           everything else; ``cfg`` is what :func:`config` returns

``dtype=np.float64`` evaluates the same statement in float64 on the same inputs: the yardstick of the device test.
"""
import math

import numpy as np

F = np.float32
D = np.float64
ROWS = 64                                # rows per group of the partial sums (GMR_LOSS_ROWS)
FOLD = 64                                # groups per block of the second tree level (GMR_LOSS_FOLD)
MAX_ACT = 32                             # GMR_LOSS_MAX_ACT
TERMS = ("value_loss", "actor_loss", "bound_loss", "entropy", "loss", "kl_mean", "learning_rate", "clip_fraction")


def config(bound_coef, entropy_coef, desired_kl, e_clip=0.2, lr_min=1e-5, lr_max=1e-2, lr_factor=1.5):
    return {"bound_coef": float(bound_coef), "entropy_coef": float(entropy_coef), "desired_kl": float(desired_kl), "e_clip": float(e_clip),
            "lr_min": float(lr_min), "lr_max": float(lr_max), "lr_factor": float(lr_factor)}


def _tree(x):
    """x[i] = x[i] + x[i + s] for s = 1, 2, 4, .. along axis 1, whose length is a power of two"""
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def sums(rows):
    """The sum over the rows of ``rows f64[M]`` or, column by column, ``f64[M, K]``: the rows of a group of ROWS consecutive ones (an absent
    row counts +0) by the balanced tree x[i] = x[i] + x[i + s], s = 1, 2, 4, ..; the groups of a block of FOLD consecutive ones (an absent
    group counts +0) by the same tree; the blocks from +0 in rising order.  A function of M alone."""
    rows = np.asarray(rows, D)
    flat = rows.ndim == 1
    x = rows.reshape(rows.shape[0], -1)
    M, K = x.shape
    G = (M + ROWS - 1) // ROWS
    B = (G + FOLD - 1) // FOLD
    pad = np.zeros((B * FOLD * ROWS, K), D)
    pad[:M] = x
    groups = _tree(pad.reshape(B * FOLD, ROWS, K))                   # [B * FOLD, K]
    blocks = _tree(groups.reshape(B, FOLD, K))                       # [B, K]
    S = np.zeros(K, D)
    for b in range(B):
        S = S + blocks[b]
    return S[0] if flat else S


def _row_sum(x, first):
    """over rising a: from the first element (``first``) or from +0"""
    acc = x[:, 0].copy() if first else np.zeros(x.shape[0], x.dtype) + x[:, 0]
    for a in range(1, x.shape[1]):
        acc = acc + x[:, a]
    return acc


def exp_once(x, T):
    """exp of a column quantity with ONE rounding to T: formed in double, rounded once"""
    return np.exp(np.asarray(x, T).astype(D)).astype(T)


def log_once(x, T):
    return np.log(np.asarray(x, T).astype(D)).astype(T)


def columns(logstd, T=F):
    """the per-column quantities: scale, var, log_scale -- the reference takes the log of the exp"""
    scale = exp_once(np.asarray(logstd, F), T)
    return scale, scale * scale, log_once(scale, T)


def _log_prob(loc, logstd, actions, T):
    _, var, log_scale = columns(logstd, T)
    C0 = T(math.log(math.sqrt(2.0 * math.pi)))
    d = actions.astype(T) - loc.astype(T)
    lpe = ((-(d * d)) / (T(2.0) * var) - log_scale) - C0             # torch.distributions.Normal.log_prob
    return d, var, _row_sum(lpe, first=True)


def log_prob(loc, logstd, actions, dtype=F):
    """``loc f32[M, A]``, ``logstd f32[A]``, ``actions f32[M, A]`` -> ``[M]`` (runner.py:123-125)"""
    assert loc.dtype == F and actions.dtype == F and loc.shape == actions.shape and loc.ndim == 2
    with np.errstate(all="ignore"):
        return _log_prob(loc, logstd, actions, dtype)[2]


def step_lr(cfg, lr, kl_mean):
    """runner.py:175-178 in double"""
    lr = float(lr)
    if kl_mean > cfg["desired_kl"] * 2:
        return max(cfg["lr_min"], lr / cfg["lr_factor"])
    if kl_mean < cfg["desired_kl"] / 2:
        return min(cfg["lr_max"], lr * cfg["lr_factor"])
    return lr


def loss(cfg, lr, loc, logstd, actions, old_log_prob, values, returns, advantages, old_loc=None, old_logstd=None, update_lr=False, dtype=F,
         inside_weight=1.0):
    """-> a dict: ``grad_loc [M, A]``, ``grad_logstd [A]``, ``grad_values [M]``, ``log_prob [M]``, ``terms f64[8]`` in the order of TERMS,
    and what the tests look at beside them: ``ratio``, ``w`` and ``learning_rate``.  ``inside_weight`` is 1; the tests hand 0.5 to show
    what the wrong tie rule would give."""
    T = dtype
    M, A = loc.shape
    assert all(np.asarray(x).dtype == F for x in (loc, logstd, actions, old_log_prob, values, returns, advantages))
    assert actions.shape == (M, A) and np.shape(logstd) == (A,) and all(x.shape == (M,) for x in (old_log_prob, values, returns, advantages))
    if (old_loc is None) != (old_logstd is None):
        raise ValueError("old_loc and old_logstd come together")
    if update_lr and old_loc is None:
        raise ValueError("update_lr needs the old policy")
    with np.errstate(all="ignore"):
        Mf = T(M)
        lo, hi = T(1.0 - cfg["e_clip"]), T(1.0 + cfg["e_clip"])
        cb = T(cfg["bound_coef"] / (M * A))
        E0 = T(0.5 + 0.5 * math.log(2.0 * math.pi))
        scale, var, log_scale = columns(logstd, T)
        lc = loc.astype(T)
        d, _, lp = _log_prob(loc, logstd, actions, T)
        # the surrogate (utils.py:47-52) and the weight torch's backward of max and clamp leaves on the row
        ratio = np.exp(lp - old_log_prob.astype(T))
        na = -advantages.astype(T)
        s = na * ratio
        sc = na * np.minimum(np.maximum(ratio, lo), hi)
        surr = np.maximum(s, sc)
        inside = (ratio >= lo) & (ratio <= hi)
        w = np.where(inside, T(inside_weight), np.where(s > sc, T(1.0), np.where(s == sc, T(0.5), T(0.0)))).astype(T)
        glp = (w * s) / Mf
        dv = values.astype(T) - returns.astype(T)
        m1, m2 = np.maximum(lc - T(1.0), T(0.0)), np.minimum(lc + T(1.0), T(0.0))
        out = {"log_prob": lp, "ratio": ratio, "w": w, "grad_values": (T(2.0) * dv) / Mf,
               "grad_loc": glp[:, None] * (d / var) + cb * (T(2.0) * m1 + T(2.0) * m2)}
        q = (d * d) / var - T(1.0)
        S = sums(glp.astype(D)[:, None] * q.astype(D))
        out["grad_logstd"] = (S + D(cfg["entropy_coef"])).astype(T)
        # the terms, in double
        value_loss = sums((dv * dv).astype(D)) / D(M)
        actor_loss = sums(surr.astype(D)) / D(M)
        bound_loss = sums(_row_sum((m1 * m1).astype(D), first=False)) / D(M * A) + sums(_row_sum((m2 * m2).astype(D), first=False)) / D(M * A)
        entropy = D(0.0)
        for a in range(A):
            entropy = entropy + D(E0 + log_scale[a])
        total = value_loss + actor_loss + D(cfg["bound_coef"]) * bound_loss + D(cfg["entropy_coef"]) * entropy
        kl_mean = D(0.0)
        if old_loc is not None:                                        # runner.py:168-174
            assert old_loc.dtype == F and old_loc.shape == (M, A) and np.asarray(old_logstd).dtype == F and np.shape(old_logstd) == (A,)
            old_scale, old_var, _ = columns(old_logstd, T)
            dl = lc - old_loc.astype(T)
            kle = (log_once(scale / old_scale, T) + (T(0.5) * (old_var + dl * dl)) / var) - T(0.5)
            kl_mean = sums(_row_sum(kle, first=True).astype(D)) / D(M)
        new_lr = step_lr(cfg, lr, float(kl_mean)) if update_lr else float(lr)
        clip_fraction = sums((w == 0).astype(D)) / D(M)
        out["terms"] = np.array([value_loss, actor_loss, bound_loss, entropy, total, kl_mean, new_lr, clip_fraction], D)
        out["learning_rate"] = new_lr
    return out
