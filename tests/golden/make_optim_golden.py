#!/usr/bin/env python3
"""Generate tests/golden/optim_golden.npz: what ``clip_grad_norm_`` and ``optimizer.step()`` (``booster_gym/utils/runner.py:164-165``) read
and deliver, by RUNNING the reference's own ``Runner.__init__`` and one iteration of ``Runner.train`` exactly the way make_ppo_golden.py does
-- its ``run_case``, its settings (four mini-epochs, the rate starting at 3e-5) and make_rollout_golden's stand-in modules and scripted
environment are imported --, case ``a`` only.  Nothing of the reference is restated.

Captured by wrapping, around make_ppo_golden's own wrappers:

    torch.nn.utils.clip_grad_norm_     the parameters it is handed (all 17 tensors of the model, ``logstd`` the first one), their gradients
                                       before the clip, and the value it returns
    torch.optim.Adam.step              the learning rate in the param group at the step; the parameters before and after it; ``exp_avg``,
                                       ``exp_avg_sq`` and ``step`` of the state after it

Part A, per mini-epoch ``m`` (the 152 199-float model does not go into git: the SAMPLE is every element of a tensor of at most 512 elements
and every 251st element, from element 0, of a larger one -- ``a_sample_tensor``, ``a_sample_index``):

    a_total_norm_m f32        the value ``clip_grad_norm_`` returned
    a_ss_m f64[17]            per tensor, the correctly rounded (``math.fsum``) sum of the squares of its gradient before the clip
    a_lr_m f64                the rate in the param group at the step; a_lr_after_m: the rate the rule left after this mini-epoch
    a_grad_m, a_before_m, a_after_m, a_exp_avg_m, a_exp_avg_sq_m f32[sample]

Part B, the unclipped regime (in part A the clip is always active): torch's own ``clip_grad_norm_`` and a fresh ``torch.optim.Adam`` at
torch's defaults, ``lr = B_LR``, on three tensors of 1, 7 and 300 elements made here; gradients in two sets -- ``lo``: total norm about 0.5,
``hi``: about 3 --; three steps; everything in full: ``b_<set>_param_0`` (before), ``b_<set>_grad_<s>``, ``b_<set>_total_norm_<s>``, and after
step ``s`` ``b_<set>_param_<s+1>``, ``b_<set>_exp_avg_<s>``, ``b_<set>_exp_avg_sq_<s>``; each the three tensors end to end.

Asserted here: part A has ``total_norm > 1`` in every mini-epoch and at least two different rates at the steps; the rate at step m + 1 is the
rate the rule left after mini-epoch m; part B has ``coef == 1`` in every step of ``lo`` and ``coef < 1`` in every step of ``hi``.

    python tests/golden/make_optim_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_ppo_golden as mpg  # noqa: E402
import make_rollout_golden as mrg  # noqa: E402

CASE = "a"
SMALL, STRIDE = 512, 251
MAX_NORM = 1.0
B_SEED = 20261020
B_SIZES = (1, 7, 300)
B_LR = 1e-3
B_STEPS = 3
B_NORMS = {"lo": 0.5, "hi": 3.0}


def sample_index(sizes):
    """(tensor, element) of every sampled element, tensor after tensor"""
    tensor, index = [], []
    for k, n in enumerate(sizes):
        idx = np.arange(n) if n <= SMALL else np.arange(0, n, STRIDE)
        tensor.append(np.full(len(idx), k, np.int32))
        index.append(idx.astype(np.int64))
    return np.concatenate(tensor), np.concatenate(index)


def run_part_a(runner, rng):
    (case, H, N), = [c for c in mpg.CASES if c[0] == CASE]
    assert mpg.CASES[0][0] == CASE                                   # the first case: the generator's draws are those of make_ppo_golden
    log, cur = [], {}
    real_clip, real_step = torch.nn.utils.clip_grad_norm_, torch.optim.Adam.step

    def take(tensors, at):
        return np.concatenate([t.detach().reshape(-1).numpy()[at[1][at[0] == k]] for k, t in enumerate(tensors)]).astype(np.float32)

    def clip_grad_norm_(params, max_norm, *a, **kw):
        params = list(params)
        assert max_norm == MAX_NORM and not a and not kw and all(p.grad is not None for p in params)
        cur["sizes"] = np.array([p.numel() for p in params], np.int64)
        at = cur["at"] = sample_index(cur["sizes"])
        cur["grad"] = take([p.grad for p in params], at)
        cur["ss"] = np.array([math.fsum(float(x) * float(x) for x in p.grad.detach().reshape(-1).numpy()) for p in params], np.float64)
        out = real_clip(params, max_norm)
        cur["total_norm"] = out.detach().clone().numpy()
        return out

    def step(self, *a, **kw):
        (group,) = self.param_groups
        assert (group["betas"], group["eps"], group["weight_decay"], group["amsgrad"], group["maximize"]) == ((0.9, 0.999), 1e-8, 0, False, False)
        ps = group["params"]
        assert [p.numel() for p in ps] == list(cur["sizes"])
        cur["lr"] = np.array(float(group["lr"]), np.float64)
        cur["before"] = take(ps, cur["at"])
        out = real_step(self, *a, **kw)
        cur["after"] = take(ps, cur["at"])
        cur["exp_avg"] = take([self.state[p]["exp_avg"] for p in ps], cur["at"])
        cur["exp_avg_sq"] = take([self.state[p]["exp_avg_sq"] for p in ps], cur["at"])
        assert {float(self.state[p]["step"]) for p in ps} == {float(len(log) + 1)}
        log.append(dict(cur))
        cur.clear()
        return out

    torch.nn.utils.clip_grad_norm_, torch.optim.Adam.step = clip_grad_norm_, step
    try:
        torch.manual_seed(mpg.SEED + H)
        ppo = mpg.run_case(runner, rng, case, H, N)
    finally:
        torch.nn.utils.clip_grad_norm_, torch.optim.Adam.step = real_clip, real_step
    assert len(log) == mpg.MINI_EPOCHS
    out = {"a_sizes": log[0]["sizes"], "a_sample_tensor": log[0]["at"][0], "a_sample_index": log[0]["at"][1], "a_learning_rate": np.array(mpg.LEARNING_RATE),
           "a_cols": np.array([mpg.O, mpg.P, mpg.A]), "mini_epochs": np.array(mpg.MINI_EPOCHS), "max_norm": np.array(MAX_NORM)}
    for m, e in enumerate(log):
        for k in ("total_norm", "ss", "lr", "grad", "before", "after", "exp_avg", "exp_avg_sq"):
            out[f"a_{k}_{m}"] = e[k]
        out[f"a_lr_after_{m}"] = ppo[f"{case}_learning_rate_{m}"]
    return out


def run_part_b():
    rng = np.random.default_rng(B_SEED)
    out = {"b_sizes": np.array(B_SIZES, np.int64), "b_lr": np.array(B_LR), "b_steps": np.array(B_STEPS)}
    total = sum(B_SIZES)
    for name, norm in B_NORMS.items():
        params = [torch.nn.Parameter(torch.from_numpy(rng.normal(0, 0.5, n).astype(np.float32))) for n in B_SIZES]
        opt = torch.optim.Adam(params, lr=B_LR)
        flat = lambda ts: np.concatenate([t.detach().reshape(-1).numpy() for t in ts]).astype(np.float32)      # noqa: E731
        out[f"b_{name}_param_0"] = flat(params)
        for s in range(B_STEPS):
            g = rng.normal(0, 1, total)
            g = (g * (norm * (1.0 + 0.1 * s) / np.sqrt((g * g).sum()))).astype(np.float32)
            at = 0
            for p in params:
                p.grad = torch.from_numpy(g[at:at + p.numel()].copy())
                at += p.numel()
            out[f"b_{name}_grad_{s}"] = g
            tn = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            assert flat([p.grad for p in params]).tobytes() == g.tobytes() if name == "lo" else True      # coef == 1 leaves the bits
            opt.step()
            out[f"b_{name}_total_norm_{s}"] = tn.detach().clone().numpy()
            out[f"b_{name}_param_{s + 1}"] = flat(params)
            out[f"b_{name}_exp_avg_{s}"] = flat([opt.state[p]["exp_avg"] for p in params])
            out[f"b_{name}_exp_avg_sq_{s}"] = flat([opt.state[p]["exp_avg_sq"] for p in params])
    return out


def coef_of(total_norm):
    """torch's own clamp, in float32 tensors"""
    return float(torch.clamp(MAX_NORM / (torch.tensor(total_norm) + 1e-6), max=1.0))


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    runner = mrg.reference_runner(ref)
    out = run_part_a(runner, np.random.default_rng(mpg.SEED))
    out.update(run_part_b())
    M = int(out["mini_epochs"])
    rates = [float(out[f"a_lr_{m}"]) for m in range(M)]
    for m in range(M):
        tn = float(out[f"a_total_norm_{m}"])
        print("a", m, "total_norm", tn, "sqrt(sum ss)", math.sqrt(math.fsum(out[f"a_ss_{m}"])), "lr", rates[m], "after", float(out[f"a_lr_after_{m}"]))
        assert tn > 1.0, (m, tn)
        assert rates[m] == (float(out["a_learning_rate"]) if m == 0 else float(out[f"a_lr_after_{m - 1}"])), m
    assert len(set(rates)) >= 2, rates
    for name in B_NORMS:
        coefs = [coef_of(out[f"b_{name}_total_norm_{s}"]) for s in range(B_STEPS)]
        print("b", name, [float(out[f"b_{name}_total_norm_{s}"]) for s in range(B_STEPS)], coefs)
        assert all(c == 1.0 for c in coefs) if name == "lo" else all(c < 1.0 for c in coefs), (name, coefs)
    assert all(v.dtype.kind in "fiu" for v in out.values())
    path = os.path.join(HERE, "optim_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
