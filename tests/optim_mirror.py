"""The clip of the gradient norm and the Adam step of a training iteration on the motion tracker in NumPy: the
statement of record of ``csrc/gmr_tracker_optim.hip``.  What the reference's runner does with the gradients of a mini-epoch:
``clip_grad_norm_(model.parameters(), 1.0)`` and ``optimizer.step()`` (booster_gym/utils/runner.py:164-165) of the ``torch.optim.Adam`` of
:33 -- torch's defaults: no weight decay, no amsgrad, not maximising.  Every value is float32 and NumPy rounds after each operator; the sum
of squares and the scalars of a step are float64, the scalars rounded once where torch's kernels take them as float32.

    partials(grads)                      one double per chunk, tensor after tensor: the association stated at :func:`chunk_sum`
    total_norm(grads)                    sqrt of their sum from +0 in rising order
    clip_coef(norm, max_norm)            min(1, max_norm / (norm + 1e-6)), rounded to float32
    adam(p, g, m, v, coef, lr, t, ...)   one tensor, in the operator order of torch's single-tensor path
    Optimizer(sizes, ...).step(params, grads, lr)

``dtype=np.float64`` evaluates the same statement in float64 on the same inputs, no scalar rounded: the yardstick of the device test.
A gradient that is ``None`` leaves its tensor out of the norm and out of the update, like ``p.grad is None``.  The gradients are never
written: the clipped gradient ``g * coef`` exists inside :func:`adam` alone.
"""
import numpy as np

F = np.float32
D = np.float64
CHUNK = 1024                             # elements per chunk (GMR_OPT_CHUNK)
MAX_TENSORS = 32                         # GMR_OPT_MAX_TENSORS
INFO = ("total_norm", "coef", "learning_rate", "step")


def chunk_sum(x):
    """the sum of ``x f64[n]``, ``n <= CHUNK``: the balanced tree x[i] = x[i] + x[i + s], s = 1, 2, 4, .. over the element index, an absent
    element counting +0"""
    pad = np.zeros(CHUNK, D)
    pad[:len(x)] = x
    while len(pad) > 1:
        pad = pad[0::2] + pad[1::2]
    return pad[0]


def partials(grads):
    """``[double per chunk]`` over the tensors in order: a chunk never spans two tensors, the last chunk of a tensor is short; the squares
    are exact in double"""
    out = []
    for g in grads:
        if g is None:
            continue
        q = np.asarray(g, F).reshape(-1).astype(D)
        q = q * q
        out += [chunk_sum(q[i:i + CHUNK]) for i in range(0, len(q), CHUNK)]
    return out


def total_norm(grads):
    total = D(0.0)
    for x in partials(grads):                                        # from +0, in rising order
        total = total + x
    return np.sqrt(total)


def clip_coef(norm, max_norm=1.0, T=F):
    return T(min(D(1.0), D(max_norm) / (D(norm) + D(1e-6))))


def power(beta, t):
    """beta^t as the product of t factors from 1, in double"""
    x = D(1.0)
    for _ in range(int(t)):
        x = x * D(beta)
    return x


def scalars(lr, t, betas=(0.9, 0.999), eps=1e-8, T=F):
    """w1, b2, c2, bc2s, e, ns of step ``t`` (the count after the step): formed in double, rounded once to ``T``"""
    b1, b2 = D(betas[0]), D(betas[1])
    return (T(D(1.0) - b1), T(b2), T(D(1.0) - b2), T(np.sqrt(D(1.0) - power(b2, t))), T(D(eps)), T(-(D(lr) / (D(1.0) - power(b1, t)))))


def adam(p, g, m, v, coef, lr, t, betas=(0.9, 0.999), eps=1e-8, dtype=F):
    """One tensor: ``p``, ``g``, ``m``, ``v`` float32 of one shape, ``coef`` the clip, ``t`` the step count after this step -> the new
    ``(p, m, v)``.  torch/optim/adam.py, the single-tensor path: lerp_, mul_ / addcmul_, sqrt / bias_correction2_sqrt + eps, addcdiv_."""
    T = dtype
    w1, b2, c2, bc2s, e, ns = scalars(lr, t, betas, eps, T)
    with np.errstate(all="ignore"):
        g = np.asarray(g, F).astype(T)
        p, m, v = (np.asarray(x).astype(T) for x in (p, m, v))
        gc = g * T(coef)
        m = m + w1 * (gc - m)
        v = v * b2
        v = v + (c2 * gc) * gc
        den = np.sqrt(v) / bc2s + e
        p = p + (ns * m) / den
    return p, m, v


class Optimizer:
    """The state of one optimiser: ``exp_avg``, ``exp_avg_sq`` per tensor and the step count.  ``step`` takes the rate of THIS step: the
    caller hands the one the rule left at the end of the previous mini-epoch."""

    def __init__(self, sizes, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, dtype=F):
        assert 1 <= len(sizes) <= MAX_TENSORS and all(n >= 1 for n in sizes)
        self.sizes, self.betas, self.eps, self.max_norm, self.T = tuple(sizes), betas, eps, max_norm, dtype
        self.t = 0
        self.m = [np.zeros(n, dtype) for n in sizes]
        self.v = [np.zeros(n, dtype) for n in sizes]

    def step(self, params, grads, lr):
        """-> ``(new params, info f64[4])``; a tensor whose gradient is ``None`` comes back as it went in and keeps its state"""
        assert len(params) == len(grads) == len(self.sizes)
        norm = total_norm(grads)
        coef = clip_coef(norm, self.max_norm, self.T)
        self.t += 1
        out = []
        for k, (p, g) in enumerate(zip(params, grads)):
            if g is None:
                out.append(np.asarray(p).astype(self.T))
                continue
            q, self.m[k], self.v[k] = adam(np.reshape(p, -1), np.reshape(g, -1), self.m[k], self.v[k], coef, lr, self.t, self.betas, self.eps, self.T)
            out.append(q.reshape(np.shape(p)))
        return out, np.array([norm, D(coef), lr, self.t], D)
