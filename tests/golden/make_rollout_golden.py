#!/usr/bin/env python3
"""Generate tests/golden/rollout_golden.npz by RUNNING the reference's own ``Runner.__init__`` from the ActorCritic on
(``booster_gym/utils/runner.py:30-42``: the model, the optimiser, the ``ExperienceBuffer`` and its six ``add_buffer`` calls) and one
iteration of ``Runner.train`` (``:99-215``) with two mini-epochs, in float32 CPU torch: the six ``update_data`` calls of every step
(``:107-108``, ``:115-118``, ``utils/buffer.py:15-16``), the bootstrap of the timed-out rewards (``:135``), ``discount_values``
(``utils/utils.py:33-44``), the returns (``:144``) and the normalisation (``:145``), with the reference's own ``ActorCritic``,
``ExperienceBuffer``, ``discount_values`` and ``surrogate_loss``.  ``runner.py`` imports yaml, imageio, its ``envs`` package (isaacgym) and
its Recorder (tensorboard, wandb), which cannot be imported without a simulator: stand-in modules take their place in ``sys.modules``; the
instance is made with ``object.__new__`` and ``__init__`` runs with ``_get_args``, ``_update_cfg_from_args``, ``_set_seed`` and ``_load``
replaced (they read the command line, a yaml file and a checkpoint); the environment is a scripted one that returns scripted ``obs``,
``privileged_obs``, ``rew``, ``done`` and ``time_outs``.  Nothing of the reference is restated.

Four calls are wrapped to capture the inputs and outputs of each mini-epoch: ``model.est_value`` (values, then last_values),
``utils.runner.discount_values`` (the rewards after the bootstrap, ``dones | time_outs``, the advantages), ``F.mse_loss`` (its second
argument is ``returns``) and ``utils.runner.surrogate_loss`` (its third argument is the normalised advantages).  The optimiser steps
between the mini-epochs, so the second one bootstraps the same time-outs with other values.

Stored, numbers only (``np.savez_compressed``; loadable with allow_pickle=False), for the case ``a`` (H = 6, N = 21) and ``b`` (H = 1,
N = 5), gamma = 0.995, lam = 0.95: the scripted rows of every step, the six buffers after the iteration, and per mini-epoch values,
last_values, the bootstrapped rewards, the advantages, the returns and the normalised advantages.  The flags hold a ``done`` without a
time-out, a time-out without a ``done`` -- what ``T1._check_termination`` produces at a command resample: a time-out and no reset --, both
at once, and in ``a`` a whole step of each.

    python tests/golden/make_rollout_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261019
GAMMA, LAM = 0.995, 0.95
O, P, A = 5, 2, 3
CASES = (("a", 6, 21), ("b", 1, 5))


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    """the stand-in of utils.recorder.Recorder: the runner hands it statistics, nothing comes back"""

    def __init__(self, cfg):
        pass

    def record_episode_statistics(self, *a):
        pass

    def record_statistics(self, *a):
        pass

    def save(self, *a):
        pass


def reference_runner(ref):
    for name in ("yaml", "imageio", "envs", "utils", "utils.recorder", "wandb", "isaacgym"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["utils"].__path__ = []
    sys.modules["utils.recorder"].Recorder = Recorder
    base = os.path.join(ref, "booster_gym", "utils")
    for name in ("model", "buffer", "utils"):
        load(os.path.join(base, name + ".py"), "utils." + name)
    return load(os.path.join(base, "runner.py"), "utils.runner")


def script(rng, case, H, N):
    """the rows the environment hands out: obs and priv of reset() and of every step, the reward and the two flags of every step"""
    F = np.float32
    s = {"obs": rng.normal(0, 1, (H + 1, N, O)).astype(F), "priv": rng.normal(0, 1, (H + 1, N, P)).astype(F), "rew": rng.normal(0.2, 1, (H, N)).astype(F)}
    if case == "a":
        done, to = rng.uniform(size=(H, N)) < 0.15, rng.uniform(size=(H, N)) < 0.15
        done[0, :6] = (False, True, False, True, False, False)          # environment 1: a done alone; 2: a time-out alone (a command
        to[0, :6] = (False, False, True, True, False, False)            # resample, no reset); 3: both at once
        done[2], to[2] = True, False                                     # a whole step of dones
        done[4], to[4] = False, True                                     # a whole step of time-outs
        done[H - 1, 4:8], to[H - 1, 4:8] = (False, True, True, False), (True, False, True, False)      # the last slot: last_values
    else:
        done, to = np.array([[False, True, False, True, False]]), np.array([[False, False, True, True, False]])
    s["done"], s["time_outs"] = done, to
    return s


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    runner = reference_runner(ref)
    rng = np.random.default_rng(SEED)
    out = {"gamma": np.array(GAMMA), "lam": np.array(LAM), "cols": np.array([O, P, A])}
    for case, H, N in CASES:
        torch.manual_seed(SEED + H)
        s = script(rng, case, H, N)

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
               "runner": {"horizon_length": H, "mini_epochs": 2, "save_interval": 1000},
               "algorithm": {"learning_rate": 1e-3, "gamma": GAMMA, "lam": LAM, "bound_coef": 0.01, "entropy_coef": -0.01, "desired_kl": 0.01}}
        runner.ScriptedEnv = ScriptedEnv
        R = runner.Runner
        R._get_args = lambda self: None
        R._update_cfg_from_args = lambda self: setattr(self, "cfg", cfg)
        R._set_seed = lambda self: None
        R._load = lambda self: None
        inst = object.__new__(R)
        R.__init__(inst)
        log = {"est_value": [], "discount_values": [], "returns": [], "normalized": []}
        real = {"est_value": inst.model.est_value, "discount_values": runner.discount_values, "mse_loss": runner.F.mse_loss,
                "surrogate_loss": runner.surrogate_loss}

        def est_value(obs, priv):
            v = real["est_value"](obs, priv)
            log["est_value"].append(v.detach().clone().numpy())
            return v

        def discount_values(rewards, dones, values, last_values, gamma, lam):
            adv = real["discount_values"](rewards, dones, values, last_values, gamma, lam)
            log["discount_values"].append({"rewards": rewards.clone().numpy(), "dones": dones.clone().numpy(), "gamma": gamma, "lam": lam,
                                           "advantages": adv.clone().numpy()})
            return adv

        def mse_loss(values, returns, *a, **kw):
            log["returns"].append(returns.detach().clone().numpy())
            return real["mse_loss"](values, returns, *a, **kw)

        def surrogate_loss(old, new, advantages, *a, **kw):
            log["normalized"].append(advantages.detach().clone().numpy())
            return real["surrogate_loss"](old, new, advantages, *a, **kw)

        inst.model.est_value, runner.discount_values, runner.F.mse_loss, runner.surrogate_loss = est_value, discount_values, mse_loss, surrogate_loss
        try:
            inst.train()
        finally:
            runner.discount_values, runner.F.mse_loss, runner.surrogate_loss = real["discount_values"], real["mse_loss"], real["surrogate_loss"]
        assert len(log["est_value"]) == 4 and len(log["discount_values"]) == len(log["returns"]) == len(log["normalized"]) == 2
        for k in ("obs", "priv", "rew", "done", "time_outs"):
            out[f"{case}_step_{k}"] = s[k]
        for k, name in (("obs", "obses"), ("priv", "privileged_obses"), ("actions", "actions"), ("rewards", "rewards"), ("dones", "dones"),
                        ("time_outs", "time_outs")):
            out[f"{case}_buffer_{k}"] = inst.buffer[name].numpy().copy()
        assert out[f"{case}_buffer_rewards"].dtype == np.float32 and out[f"{case}_buffer_dones"].dtype == np.bool_
        for m in range(2):
            d = log["discount_values"][m]
            assert d["gamma"] == GAMMA and d["lam"] == LAM and (d["dones"] == (s["done"] | s["time_outs"])).all()
            values, last_values = log["est_value"][2 * m], log["est_value"][2 * m + 1]
            assert values.shape == (H, N) and last_values.shape == (N,) and values.dtype == np.float32
            assert (d["rewards"][s["time_outs"]] == values[s["time_outs"]]).all() and (d["rewards"][~s["time_outs"]] == s["rew"][~s["time_outs"]]).all()
            out.update({f"{case}_values_{m}": values, f"{case}_last_values_{m}": last_values, f"{case}_rewards_{m}": d["rewards"],
                        f"{case}_advantages_{m}": d["advantages"], f"{case}_returns_{m}": log["returns"][m], f"{case}_normalized_{m}": log["normalized"][m]})
        assert (out[f"{case}_values_0"] != out[f"{case}_values_1"]).any()                 # the optimiser stepped in between
        assert (out[f"{case}_buffer_rewards"] == out[f"{case}_rewards_1"]).all()          # the buffer keeps the last bootstrap
        if case == "a":
            dn, to = s["done"], s["time_outs"]
            assert (dn & ~to).any() and (to & ~dn).any() and (dn & to).any() and dn[2].all() and to[4].all() and not (dn | to)[1].all()
    path = os.path.join(HERE, "rollout_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
