#!/usr/bin/env python3
"""Generate tests/golden/episode_golden.npz by RUNNING the reference's own ``T1._reset_dofs`` / ``T1._reset_root_states``
(``booster_gym/envs/t1.py:319-340``), ``T1._compute_reward`` (``:560-572``), ``T1Imitation._compute_reward``
(``booster_gym/envs/t1_imitation.py:323-352``) and ``Recorder.record_episode_statistics`` / ``Recorder._mean``
(``booster_gym/utils/recorder.py:36-53``, ``:86-90``) in float32 CPU torch.  The three files import isaacgym, tensorboard, wandb and their own
package, which cannot be imported without a simulator: empty stand-in modules take their place in ``sys.modules`` (``envs.base_task.BaseTask``
is ``object``), ``utils.utils`` and ``utils.terrain`` are the reference's own files, every instance is made with ``object.__new__`` and only
the attributes the methods read are set.  Nothing of the reference is restated except isaacgym's ``quat_from_euler_xyz`` at zero roll and
pitch, which is not there to run: ``(0, 0, sin(yaw / 2), cos(yaw / 2))`` in float32 torch.

Stored, numbers only (``np.savez_compressed``; loadable with allow_pickle=False):

  (a) two resets of listed environments -- ``flat`` on the plane with uniform additive specs, ``slope`` on a sloped height field with a
      gaussian scaling dof spec, a uniform additive xy spec and a gaussian additive velocity spec --: the arrays before and after, and
      the variates of ``rand_like`` / ``randn_like`` / ``rand`` in call order (one dof row per call: ``default_dof_pos`` is ``[1, R]``).
  (b) both ``_compute_reward``s on scripted reward functions whose names are in the library's column order (the six imitation terms,
      then 14 + 8 + 4 + 2 more; two scales are zero): per step the terms, the reward, ``extras["rew_terms"]`` as columns (zero where the
      reference has no entry) and the two totals of the imitation reward.
      ``T1Imitation._prepare_reward_function`` is NOT run: it appends the imitation functions a second time with scales that were not
      multiplied by dt, a third count outside the lines this fixture is about; ``T1._prepare_reward_function`` prepares every instance.
  (c) ``record_episode_statistics`` over 40 scripted steps with a scripted ``done`` (nobody, some, everybody), fed the imitation reward
      and its ``rew_terms`` without the two totals: the finished episodes' steps and sums in the Recorder's order and its ``_mean``s.

    python tests/golden/make_episode_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20251103
DT = 0.02
IMITATION = ("imitation_root_pos", "imitation_root_rot", "imitation_root_vel", "imitation_root_ang_vel", "imitation_dof_pos", "imitation_dof_vel")
PROPRIO = ("lin_vel_z", "ang_vel_xy", "orientation", "torques", "dof_vel", "dof_acc", "root_acc", "action_rate", "dof_pos_limits",
           "dof_vel_limits", "torque_limits", "torque_tiredness", "power", "base_height")
FEET = ("collision", "feet_slip", "feet_vel_z", "feet_roll", "feet_yaw_diff", "feet_yaw_mean", "feet_distance", "feet_swing")
CMD = ("survival", "tracking_lin_vel_x", "tracking_lin_vel_y", "tracking_ang_vel")
EXTRA = ("motion_smoothness", "alive_bonus")
NAMES = IMITATION + PROPRIO + FEET + CMD + EXTRA
LOCOMOTION_WEIGHT, IMITATION_WEIGHT = 0.1, 1.0
FLAT = {"init_dof_pos": {"distribution": "uniform", "operation": "additive", "range": [-0.1, 0.1]},
        "init_base_pos_xy": {"distribution": "uniform", "operation": "additive", "range": [-1.0, 1.0]},
        "init_base_lin_vel_xy": {"distribution": "uniform", "operation": "additive", "range": [-0.5, 0.5]}}
SLOPE = {"init_dof_pos": {"distribution": "gaussian", "operation": "scaling", "range": [1.0, 0.05]},
         "init_base_pos_xy": {"distribution": "uniform", "operation": "additive", "range": [-0.7, 0.3]},
         "init_base_lin_vel_xy": {"distribution": "gaussian", "operation": "additive", "range": [0.0, 0.3]}}
NX, NY, BORDER, HS, VS = 48, 40, 3, 0.25, 0.005


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_modules(ref):
    for name in ("isaacgym", "isaacgym.gymapi", "isaacgym.gymtorch", "isaacgym.gymutil", "isaacgym.torch_utils", "isaacgym.terrain_utils", "envs",
                 "envs.base_task", "utils", "utils.motion_loader", "torch.utils.tensorboard", "wandb"):
        sys.modules[name] = types.ModuleType(name)
    gym = sys.modules["isaacgym"]
    for sub in ("gymapi", "gymtorch", "gymutil", "torch_utils", "terrain_utils"):
        setattr(gym, sub, sys.modules["isaacgym." + sub])
    for name in ("get_axis_params", "to_torch", "quat_rotate_inverse", "quat_from_euler_xyz", "torch_rand_float", "get_euler_xyz", "quat_rotate",
                 "quat_mul", "quat_conjugate"):
        setattr(sys.modules["isaacgym.torch_utils"], name, None)
    sys.modules["isaacgym.gymtorch"].unwrap_tensor = lambda x: x
    sys.modules["envs"].__path__ = []
    sys.modules["envs.base_task"].BaseTask = object
    sys.modules["utils"].__path__ = []
    sys.modules["utils.motion_loader"].MotionLoader = sys.modules["utils.motion_loader"].MotionLibrary = None
    sys.modules["torch.utils.tensorboard"].SummaryWriter = None
    base = os.path.join(ref, "booster_gym")
    load(os.path.join(base, "utils", "utils.py"), "utils.utils")
    terrain = load(os.path.join(base, "utils", "terrain.py"), "utils.terrain")
    t1 = load(os.path.join(base, "envs", "t1.py"), "envs.t1")
    imit = load(os.path.join(base, "envs", "t1_imitation.py"), "envs.t1_imitation")
    recorder = load(os.path.join(base, "utils", "recorder.py"), "utils.recorder")
    # isaacgym's quat_from_euler_xyz at zero roll and pitch, restated
    t1.quat_from_euler_xyz = lambda roll, pitch, yaw: torch.stack([torch.zeros_like(yaw), torch.zeros_like(yaw), torch.sin(yaw * 0.5),
                                                                   torch.cos(yaw * 0.5)], dim=-1)
    return t1, imit, recorder, terrain


class Gym:
    def set_dof_state_tensor_indexed(self, *a):
        pass

    def set_actor_root_state_tensor(self, *a):
        pass


def recorded(log):
    """torch.rand_like / randn_like / rand that write what they return into ``log``"""
    real = {k: getattr(torch, k) for k in ("rand_like", "randn_like", "rand")}

    def wrap(k):
        def f(*a, **kw):
            x = real[k](*a, **kw)
            log.append((k, x.clone().numpy()))
            return x
        return f
    for k in real:
        setattr(torch, k, wrap(k))
    return real


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    t1, imit, recorder, terrain = reference_modules(ref)
    torch.manual_seed(SEED)
    rng = np.random.default_rng(SEED)
    F = np.float32
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731
    out = {"dt": np.array(DT), "names": np.array(NAMES), "locomotion_weight": np.array(LOCOMOTION_WEIGHT), "imitation_weight": np.array(IMITATION_WEIGHT)}

    # ---- (a) _reset_dofs and _reset_root_states ----
    N, R = 12, 23
    field = (7 * np.arange(NX)[:, None] - 4 * np.arange(NY)[None, :] + rng.integers(-2, 3, (NX, NY))).astype(np.int16)
    out.update({"reset_N": N, "reset_R": R, "field": field, "terrain": np.array([HS, VS, BORDER]), "base_init_state": rng.normal(0, 0.3, 13).astype(F),
                "default_dof_pos": rng.uniform(-0.6, 0.6, R).astype(F), "env_origins": rng.uniform(0.5, 4.0, (N, 3)).astype(F)})
    out["base_init_state"][:3] = (F(0.1), F(-0.05), F(0.72))      # with the origins and the xy range every drawn point lies inside the field
    for case, specs, ids in (("flat", FLAT, [0, 3, 4, 7, 11]), ("slope", SLOPE, [10, 2, 5, 6, 1, 9, 8])):
        env = object.__new__(t1.T1)
        env.cfg, env.device, env.gym, env.sim, env.dof_state, env.num_envs = {"randomization": specs}, "cpu", Gym(), None, None, N
        env.default_dof_pos = f32(out["default_dof_pos"]).unsqueeze(0)
        env.base_init_state = f32(out["base_init_state"])
        env.env_origins = f32(out["env_origins"])
        ter = object.__new__(terrain.Terrain)
        ter.device = "cpu"
        if case == "flat":
            ter.type = "plane"
        else:
            ter.type, ter.border_pixels, ter.horizontal_scale, ter.vertical_scale, ter.height_field_raw = "trimesh", BORDER, HS, VS, field
        env.terrain = ter
        before = {"dof_pos": rng.normal(0, 1, (N, R)).astype(F), "dof_vel": rng.normal(0, 1, (N, R)).astype(F),
                  "root_states": rng.normal(0, 1, (N, 13)).astype(F)}
        env.dof_pos, env.dof_vel, env.root_states = (f32(before[k]).clone() for k in ("dof_pos", "dof_vel", "root_states"))
        log = []
        real = recorded(log)
        try:
            env_ids = torch.tensor(ids, dtype=torch.long)
            env._reset_dofs(env_ids)
            env._reset_root_states(env_ids)
        finally:
            for k, f in real.items():
                setattr(torch, k, f)
        kinds = [k for k, _ in log]
        want = [("randn_like" if specs["init_dof_pos"]["distribution"] == "gaussian" else "rand_like"), "rand_like", "rand",
                ("randn_like" if specs["init_base_lin_vel_xy"]["distribution"] == "gaussian" else "rand_like")]
        assert kinds == want, kinds
        assert log[0][1].shape == (1, R) and log[1][1].shape == (len(ids), 2) and log[2][1].shape == (len(ids),) and log[3][1].shape == (len(ids), 2)
        out.update({f"{case}_ids": np.array(ids, dtype=np.int32), f"{case}_var_dof": log[0][1], f"{case}_var_xy": log[1][1], f"{case}_var_yaw": log[2][1],
                    f"{case}_var_vel": log[3][1]})
        for k in before:
            out[f"{case}_{k}_before"] = before[k]
            out[f"{case}_{k}_after"] = getattr(env, k).numpy().copy()
        px = np.floor(BORDER + out[f"{case}_root_states_after"][ids, :2] / HS)
        assert (px >= 0).all() and (px[:, 0] + 1 <= NX - 1).all() and (px[:, 1] + 1 <= NY - 1).all()
        untouched = np.setdiff1d(np.arange(N), ids)
        assert (out[f"{case}_root_states_after"][untouched] == before["root_states"][untouched]).all()
        assert out[f"{case}_root_states_after"].dtype == F

    # ---- (b) the two _compute_reward ----
    N, T, C = 21, 40, len(NAMES)
    scales = rng.uniform(-3.0, 3.0, C).round(2)
    scales[:6] = np.abs(scales[:6]) + 0.5
    scales[NAMES.index("torques")] = 0.0                  # two terms the reference drops (t1.py:281-283)
    scales[NAMES.index("feet_yaw_mean")] = 0.0
    terms = (rng.integers(-512, 513, (T, N, C)) / 256.0).astype(F)          # some sums negative: the clip acts on some environments only
    terms[:, :, :6] = np.abs(terms[:, :, :6])
    out.update({"scales": scales, "terms": terms, "reward_N": N})

    def make(cls, only_positive):
        env = object.__new__(cls)
        env.cfg = {"rewards": {"scales": {k: float(s) for k, s in zip(NAMES, scales)}, "only_positive_rewards": only_positive}}
        env.dt, env.device, env.num_envs = DT, "cpu", N
        env.rew_buf = torch.zeros(N, dtype=torch.float)
        env.extras = {"rew_terms": {}}
        env.locomotion_weight, env.imitation_weight = LOCOMOTION_WEIGHT, IMITATION_WEIGHT
        env.motion_times = torch.zeros(N)
        env._reward_debug_counter = 0                     # (the debug print of step 0 stays off)
        env.now = 0
        for k, name in enumerate(NAMES):
            setattr(env, "_reward_" + name, (lambda k: lambda: f32(terms[env.now][:, k]))(k))
        t1.T1._prepare_reward_function(env)               # (T1's own: every scale times dt, the functions in the order of the scales)
        return env
    assert DT * 1.0 == DT
    out["weights"] = np.array([float(s) * DT for s in scales])             # reward_scales after _prepare_reward_function, as doubles
    for case, cls, pos in (("t1", t1.T1, True), ("imit", imit.T1Imitation, True), ("imit_raw", imit.T1Imitation, False)):
        env = make(cls, pos)
        assert list(env.reward_scales) == [k for k, s in zip(NAMES, scales) if s != 0]
        assert all(env.reward_scales[k] == w for k, w in zip(NAMES, out["weights"]) if w != 0)
        rew, scaled, loc, imi = np.zeros((T, N), F), np.zeros((T, N, C), F), np.zeros((T, N), F), np.zeros((T, N), F)
        for s in range(T):
            env.now = s
            env.extras["rew_terms"] = {}
            env._compute_reward()
            rew[s] = env.rew_buf.numpy()
            for k, name in enumerate(NAMES):
                if name in env.extras["rew_terms"]:
                    scaled[s, :, k] = env.extras["rew_terms"][name].numpy()
            if cls is imit.T1Imitation:
                loc[s], imi[s] = env.extras["rew_terms"]["locomotion_total"].numpy(), env.extras["rew_terms"]["imitation_total"].numpy()
        out[f"{case}_reward"] = rew
        if case == "t1":
            assert (rew == 0).any() and (rew > 0).any()
        if case == "imit":
            out["scaled"], out["imit_locomotion"], out["imit_imitation"] = scaled, loc, imi
            assert (loc == 0).any() and (loc > 0).any()
        if case == "imit_raw":
            assert (scaled == out["scaled"]).all() and (loc < 0).any()
            out["imit_raw_locomotion"] = loc

    # ---- (c) record_episode_statistics ----
    rec = object.__new__(recorder.Recorder)
    rec.cfg, rec.episode_statistics, rec.last_episode, rec.episode_steps = {"runner": {"use_wandb": False}}, {}, {"steps": []}, None
    done = rng.uniform(size=(T, N)) < 0.08
    done[0, :3] = True                   # the very first call: episodes of zero steps
    done[5] = False
    done[17] = True                      # everybody at once
    out["done"] = done
    keys = ["reward"] + [k for k, s in zip(NAMES, scales) if s != 0]
    for s in range(T):
        ep_info = {"reward": f32(out["imit_reward"][s])}
        ep_info.update({k: f32(out["scaled"][s][:, NAMES.index(k)]) for k in keys[1:]})
        rec.record_episode_statistics(torch.from_numpy(done[s]), ep_info, s, False)
    n = len(rec.last_episode["steps"])
    assert n == int(done.sum()) and all(len(rec.last_episode[k]) == n for k in keys)
    fin = np.zeros((n, C + 1), F)            # the finished episodes' sums in the Recorder's order; a dropped term's column stays zero
    means, abs_sum = np.zeros(C + 1), np.zeros(C + 1)
    for k in keys:
        col = 0 if k == "reward" else 1 + NAMES.index(k)
        fin[:, col] = np.array(rec.last_episode[k], dtype=F)
        assert (fin[:, col].astype(np.float64) == np.array(rec.last_episode[k])).all()
        means[col] = rec._mean(rec.last_episode[k])
        abs_sum[col] = np.abs(np.array(rec.last_episode[k])).sum()
    out.update({"fin_steps": np.array(rec.last_episode["steps"], dtype=np.int64), "fin_sums": fin, "mean_steps": np.array(rec._mean(rec.last_episode["steps"])),
                "means": means, "abs_sum": abs_sum, "open_steps": rec.episode_steps.numpy().copy(),
                "open_reward": rec.episode_statistics["reward"].numpy().copy()})
    empty = object.__new__(recorder.Recorder)
    out["mean_of_nothing"] = np.array(empty._mean([]))
    path = os.path.join(HERE, "episode_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", n, "finished episodes")


if __name__ == "__main__":
    main(sys.argv)
