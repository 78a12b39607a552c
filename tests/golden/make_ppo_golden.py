#!/usr/bin/env python3
"""Generate tests/golden/ppo_golden.npz by RUNNING the reference's own ``Runner.__init__`` and one iteration of ``Runner.train``
(``booster_gym/utils/runner.py:99-215``) in float32 CPU torch, exactly the way make_rollout_golden.py does -- its stand-in modules, its
``object.__new__`` instance, its scripted environment are imported from there --, and capturing, per mini-epoch, what the loss head of
``:123-125`` and ``:146-180`` reads and what it delivers.  Nothing of the reference is restated.

Captured by wrapping:

    model.act                          ``dist.loc`` of every call (the H calls of the rollout, the old policy of :124, one per mini-epoch) and
                                       ``logstd`` at that moment; a tensor hook on the ``loc`` of a mini-epoch receives its gradient
    model.est_value                    the values of a mini-epoch (the first of its two calls), with a tensor hook for their gradient
    F.mse_loss                         ``returns`` (its second argument) and ``value_loss`` (its result)
    utils.runner.surrogate_loss        ``old_actions_log_prob``, ``actions_log_prob``, the normalised advantages and ``actor_loss``
    optimizer.zero_grad (:162)         called when the loss stands: ``bound_loss``, ``entropy.mean()`` and ``loss`` are read from the
                                       locals of the frame that calls it, which is ``train``
    torch.nn.utils.clip_grad_norm_     ``logstd.grad`` before the clip touches it
    the Recorder's record_statistics   and the next mini-epoch's est_value: ``kl_mean`` of the frame and ``self.learning_rate`` after the rule

The scripted run's settings, chosen so that the assertions at the end hold: Adam's learning rate starts at ``LEARNING_RATE = 3e-5``, four
mini-epochs, ``bound_coef = 0.01``, ``entropy_coef = -0.01``, ``desired_kl`` = ``DESIRED_KL`` per case; the rewards of make_rollout_golden's
script.  In case ``a`` the rule raises the rate after mini-epoch 0 (old == new: kl = 0), and later lowers it; in case ``b`` it keeps it once.
Asserted here: in a later mini-epoch of ``a`` rows inside, above and below the clip interval are present with either sign of the
advantage; the rule takes each of its three branches across the fixture; no row's ratio lies within RATIO_MARGIN of ``1 - e_clip`` or
``1 + e_clip``, so no row is left out of any comparison.

    python tests/golden/make_ppo_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_rollout_golden as mrg  # noqa: E402

SEED = 20261019
MINI_EPOCHS = 4
LEARNING_RATE = 3e-5
BOUND_COEF, ENTROPY_COEF = 0.01, -0.01
DESIRED_KL = {"a": 0.01, "b": 0.05}
OBS_SCALE = 14.0                            # the scripted observations are scaled: larger action means than a fresh network gives
E_CLIP = 0.2                                # the default of utils.surrogate_loss, which the runner does not override
RATIO_MARGIN = 1e-4                         # far above any bound of the host test, in units of the ratio itself
O, P, A = mrg.O, mrg.P, mrg.A
CASES = mrg.CASES


def run_case(runner, rng, case, H, N):
    s = mrg.script(rng, case, H, N)
    # larger action means than a fresh network gives, so that the bound term and its gradient are alive: the observations are scaled
    s["obs"] = (s["obs"] * np.float32(OBS_SCALE)).astype(np.float32)

    class ScriptedEnv:
        num_actions, num_obs, num_privileged_obs, num_envs = A, O, P, N
        mean_lin_vel_level = mean_ang_vel_level = max_lin_vel_level = max_ang_vel_level = 0.0
        curriculum_prob = None

        def __init__(self, cfg):
            self.now = 0

        def reset(self):
            return torch.from_numpy(s["obs"][0]), {"privileged_obs": torch.from_numpy(s["priv"][0])}

        def step(self, act):
            k = self.now
            self.now += 1
            return (torch.from_numpy(s["obs"][k + 1]), torch.from_numpy(s["rew"][k]), torch.from_numpy(s["done"][k]),
                    {"privileged_obs": torch.from_numpy(s["priv"][k + 1]), "time_outs": torch.from_numpy(s["time_outs"][k]), "rew_terms": {}})

    cfg = {"basic": {"task": "ScriptedEnv", "rl_device": "cpu", "max_iterations": 1},
           "runner": {"horizon_length": H, "mini_epochs": MINI_EPOCHS, "save_interval": 1000},
           "algorithm": {"learning_rate": LEARNING_RATE, "gamma": mrg.GAMMA, "lam": mrg.LAM, "bound_coef": BOUND_COEF, "entropy_coef": ENTROPY_COEF,
                         "desired_kl": DESIRED_KL[case]}}
    runner.ScriptedEnv = ScriptedEnv
    R = runner.Runner
    R._get_args = lambda self: None
    R._update_cfg_from_args = lambda self: setattr(self, "cfg", cfg)
    R._set_seed = lambda self: None
    R._load = lambda self: None
    inst = object.__new__(R)
    R.__init__(inst)

    npy = lambda t: t.detach().clone().numpy()                                                  # noqa: E731
    log = {"act": [], "epochs": [], "after": []}
    cur = {}
    real = {"act": inst.model.act, "est_value": inst.model.est_value, "mse_loss": runner.F.mse_loss, "surrogate_loss": runner.surrogate_loss,
            "zero_grad": inst.optimizer.zero_grad, "clip": torch.nn.utils.clip_grad_norm_}

    def after_rule(frame):
        """kl_mean and the learning rate of the mini-epoch that has just ended, from the frame of train"""
        log["after"].append({"kl_mean": npy(frame.f_locals["kl_mean"]), "learning_rate": float(frame.f_locals["self"].learning_rate)})

    def act(obs):
        dist = real["act"](obs)
        log["act"].append({"loc": npy(dist.loc), "logstd": npy(inst.model.logstd).reshape(-1), "grad": dist.loc.requires_grad})
        if dist.loc.requires_grad:
            cur["loc"], cur["logstd"] = log["act"][-1]["loc"], log["act"][-1]["logstd"]
            dist.loc.register_hook(lambda g: cur.__setitem__("grad_loc", g.clone().numpy()))
        return dist

    def est_value(obs, priv):
        v = real["est_value"](obs, priv)
        if v.shape == (H, N) and "values" not in cur:
            frame = sys._getframe(1)
            if "kl_mean" in frame.f_locals:
                after_rule(frame)
            cur["values"] = npy(v)
            v.register_hook(lambda g: cur.__setitem__("grad_values", g.clone().numpy()))
        return v

    def mse_loss(values, returns, *a, **kw):
        out = real["mse_loss"](values, returns, *a, **kw)
        cur["returns"], cur["value_loss"] = npy(returns), npy(out)
        return out

    def surrogate_loss(old, new, advantages, *a, **kw):
        assert not a and not kw                                                                  # e_clip is the default
        out = real["surrogate_loss"](old, new, advantages)
        cur.update(old_log_prob=npy(old), log_prob=npy(new), advantages=npy(advantages), actor_loss=npy(out))
        return out

    def zero_grad(*a, **kw):
        loc = sys._getframe(1).f_locals
        cur.update(bound_loss=npy(loc["bound_loss"]), entropy=npy(loc["entropy"].mean()), loss=npy(loc["loss"]))
        return real["zero_grad"](*a, **kw)

    def clip_grad_norm_(params, *a, **kw):
        cur["grad_logstd"] = npy(inst.model.logstd.grad).reshape(-1)
        log["epochs"].append(dict(cur))
        cur.clear()
        return real["clip"](params, *a, **kw)

    class LastRecorder(mrg.Recorder):
        def record_statistics(self, stats, it):
            after_rule(sys._getframe(1))

    inst.model.act, inst.model.est_value, inst.optimizer.zero_grad = act, est_value, zero_grad
    runner.F.mse_loss, runner.surrogate_loss, torch.nn.utils.clip_grad_norm_, runner.Recorder = mse_loss, surrogate_loss, clip_grad_norm_, LastRecorder
    try:
        inst.train()
    finally:
        runner.F.mse_loss, runner.surrogate_loss, torch.nn.utils.clip_grad_norm_, runner.Recorder = (real["mse_loss"], real["surrogate_loss"],
                                                                                                       real["clip"], mrg.Recorder)
    assert len(log["act"]) == H + 1 + MINI_EPOCHS and len(log["epochs"]) == len(log["after"]) == MINI_EPOCHS
    assert [x["grad"] for x in log["act"]] == [False] * (H + 1) + [True] * MINI_EPOCHS
    out = {f"{case}_actions": inst.buffer["actions"].numpy().copy(), f"{case}_old_loc": log["act"][H]["loc"], f"{case}_old_logstd": log["act"][H]["logstd"],
           f"{case}_rollout_loc": np.stack([x["loc"] for x in log["act"][:H]]), f"{case}_desired_kl": np.array(DESIRED_KL[case])}
    for m, (e, aft) in enumerate(zip(log["epochs"], log["after"])):
        for k in ("loc", "logstd", "values", "returns", "advantages", "old_log_prob", "log_prob", "value_loss", "actor_loss", "bound_loss", "entropy",
                  "loss", "grad_loc", "grad_logstd", "grad_values"):
            out[f"{case}_{k}_{m}"] = e[k]
        out[f"{case}_kl_mean_{m}"] = aft["kl_mean"]
        out[f"{case}_learning_rate_{m}"] = np.array(aft["learning_rate"], np.float64)
    return out


def branch(lr_before, lr_after):
    return 0 if lr_after == lr_before else (1 if lr_after > lr_before else -1)


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    runner = mrg.reference_runner(ref)
    rng = np.random.default_rng(SEED)
    out = {"cols": np.array([O, P, A]), "learning_rate": np.array(LEARNING_RATE), "bound_coef": np.array(BOUND_COEF), "entropy_coef": np.array(ENTROPY_COEF),
           "e_clip": np.array(E_CLIP), "mini_epochs": np.array(MINI_EPOCHS)}
    branches = set()
    for case, H, N in CASES:
        torch.manual_seed(SEED + H)
        out.update(run_case(runner, rng, case, H, N))
        lr = LEARNING_RATE
        for m in range(MINI_EPOCHS):
            after = float(out[f"{case}_learning_rate_{m}"])
            branches.add(branch(lr, after))
            lr = after
            ratio = np.exp(out[f"{case}_log_prob_{m}"].astype(np.float64) - out[f"{case}_old_log_prob_{m}"].astype(np.float64)).reshape(-1)
            assert (np.abs(ratio - (1 - E_CLIP)) > RATIO_MARGIN).all() and (np.abs(ratio - (1 + E_CLIP)) > RATIO_MARGIN).all(), (case, m)
            print(case, m, "kl_mean", float(out[f"{case}_kl_mean_{m}"]), "lr", after, "inside/above/below",
                  int(((ratio >= 1 - E_CLIP) & (ratio <= 1 + E_CLIP)).sum()), int((ratio > 1 + E_CLIP).sum()), int((ratio < 1 - E_CLIP).sum()),
                  "max |loc|", float(np.abs(out[f"{case}_loc_{m}"]).max()))
    assert branches == {-1, 0, 1}, branches
    seen = False
    for m in range(1, MINI_EPOCHS):
        ratio = np.exp(out[f"a_log_prob_{m}"].astype(np.float64) - out[f"a_old_log_prob_{m}"].astype(np.float64)).reshape(-1)
        adv = out[f"a_advantages_{m}"].reshape(-1)
        regimes = [(ratio >= 1 - E_CLIP) & (ratio <= 1 + E_CLIP), ratio > 1 + E_CLIP, ratio < 1 - E_CLIP]
        seen = seen or all((r & (adv > 0)).any() and (r & (adv < 0)).any() for r in regimes)
    assert seen, "no later mini-epoch of case a holds every regime with either sign of the advantage"
    assert (np.abs(out["a_loc_1"]) > 1.0).any() and (out["a_bound_loss_1"] > 0)
    path = os.path.join(HERE, "ppo_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
