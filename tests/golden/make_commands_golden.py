#!/usr/bin/env python3
"""Generate tests/golden/commands_golden.npz by RUNNING the reference's own ``T1._update_curriculum``, ``T1._resample_commands`` /
``T1._resample_curriculum_commands`` (``booster_gym/envs/t1.py:362-435``) and ``apply_randomization`` (``booster_gym/utils/utils.py:5-30``)
in float32 CPU torch.  ``t1.py`` imports isaacgym and its own package, which cannot be imported without a simulator: empty stand-in modules
take the place of ``isaacgym`` (``gymapi``, ``gymtorch``, ``torch_utils`` with the seven imported names) and of the ``envs`` package
(``envs.base_task.BaseTask`` is ``object``), ``utils.utils`` is the reference's own file, the instance is made with ``object.__new__(T1)``
and only the attributes the three methods read are set.  Nothing of the reference is restated except isaacgym's ``torch_rand_float``, which
is not there to run: ``(upper - lower) * u + lower`` on a recorded uniform ``u``.

Stored, numbers only (``np.savez_compressed``; loadable with allow_pickle=False):

  (a) scripted rounds of ``_update_curriculum`` on a 7 x 5 grid (L = 3, A = 2, update_rate 0.125, so that repeated adds are exact): per
      round the reset environments, their step counts, levels, commands and filtered velocities, and ``curriculum_prob`` after the round.
      Environments succeed at the grid's centre, edges and corners; others miss each of the four conditions by one step or one float32
      ulp; the last round saturates cells at 1.
  (b) both branches of ``_resample_commands`` with ``still_proportion = 0``: the uniforms in call order, the recorded result of
      ``torch.multinomial``, and the resulting ``commands``, ``env_curriculum_level`` and ``gait_frequency``.
  (c) ``apply_randomization`` for the four (operation, distribution) pairs on a kick-shaped tensor and on zeros, with the variate of
      ``randn_like`` / ``rand_like`` recorded.

    python tests/golden/make_commands_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
L, A, RATE = 3, 2, 0.125
TOLER = (0.2, 0.7, 0.3)                    # 0.7 rounds DOWN to float32, 0.2 and 0.3 up: the comparison is shown to be made in float32
RES = (0.2, 0.1, 0.3)
EPISODE_S, DT, LENGTH_TOLER = 1.0, 0.02, 0.1          # success needs more than ceil(50) * 0.9 = 45 steps
RANGES = {"lin_vel_x": (-1.0, 1.3), "lin_vel_y": (-0.4, 0.4), "ang_vel_yaw": (-1.1, 0.9), "gait_frequency": (1.0, 2.2)}
SEED = 20251027


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_modules(ref):
    for name in ("isaacgym", "isaacgym.gymapi", "isaacgym.gymtorch", "isaacgym.gymutil", "isaacgym.torch_utils", "isaacgym.terrain_utils", "envs",
                 "envs.base_task", "utils"):
        sys.modules[name] = types.ModuleType(name)
    gym = sys.modules["isaacgym"]
    for sub in ("gymapi", "gymtorch", "gymutil", "torch_utils", "terrain_utils"):
        setattr(gym, sub, sys.modules["isaacgym." + sub])
    for name in ("get_axis_params", "to_torch", "quat_rotate_inverse", "quat_from_euler_xyz", "torch_rand_float", "get_euler_xyz", "quat_rotate"):
        setattr(sys.modules["isaacgym.torch_utils"], name, None)
    sys.modules["envs"].__path__ = []
    sys.modules["envs.base_task"].BaseTask = object
    sys.modules["utils"].__path__ = []
    utils = load(os.path.join(ref, "booster_gym", "utils", "utils.py"), "utils.utils")
    t1 = load(os.path.join(ref, "booster_gym", "envs", "t1.py"), "envs.t1")
    return t1, utils


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    t1, utils = reference_modules(ref)
    torch.manual_seed(SEED)
    rng = np.random.default_rng(SEED)
    F = np.float32
    out = {"L": L, "A": A, "rate": RATE, "toler": np.array(TOLER), "res": np.array(RES), "episode_length_s": EPISODE_S, "dt": DT,
           "episode_length_toler": LENGTH_TOLER}
    cfg = {"commands": {"curriculum": True, "episode_length_toler": LENGTH_TOLER, "lin_vel_x_toler": TOLER[0], "lin_vel_y_toler": TOLER[1],
                        "ang_vel_yaw_toler": TOLER[2], "lin_vel_levels": L, "ang_vel_levels": A, "update_rate": RATE, "lin_vel_x_resolution": RES[0],
                        "lin_vel_y_resolution": RES[1], "ang_vel_resolution": RES[2], "still_proportion": 0.0, "resampling_time_s": (0.1, 0.5),
                        **{k: list(v) for k, v in RANGES.items()}},
           "rewards": {"episode_length_s": EPISODE_S}}

    # ---- (a) _update_curriculum ----
    N = 24
    env = object.__new__(t1.T1)
    env.cfg, env.dt, env.device = cfg, DT, "cpu"
    env.curriculum_prob = torch.zeros(2 * L + 1, 2 * A + 1)
    env.curriculum_prob[L, A] = 1.0
    # levels: centre, the four edge midpoints, the four corners, then inner cells
    levels = [(0, 0), (3, 0), (-3, 0), (0, 2), (0, -2), (3, 2), (3, -2), (-3, 2), (-3, -2), (1, 1), (-2, -1), (2, 0)]
    levels = np.array(levels + [(0, 0)] * (N - len(levels)), dtype=np.int64)
    tol32 = [F(x) for x in TOLER]
    rounds = []
    for r in range(5):
        steps = np.full(N, 48, np.int64)
        cmd = rng.uniform(-1, 1, (N, 3)).astype(F)
        err = np.zeros((N, 3), F)              # the velocity is cmd + err: within the tolerances
        err[:] = [F(0.5) * t * s for t, s in zip(tol32, (1, -1, 1))]
        ids = np.arange(N)
        if r == 0:                             # everybody succeeds once: centre, edges, corners, inner cells
            ids = np.arange(12)
        elif r == 1:                           # 12..19 miss one condition each by a step or an ulp, 20..23 just make it
            ids = np.arange(12, 24)
            cmd[12:] = 0.0                      # so that |f - c| is the float32 number chosen below, exactly
            err[12:] = 0.0
            steps[12], steps[20] = 45, 46
            for k, (miss, make) in enumerate(((13, 21), (14, 22), (15, 23))):
                err[miss, k], err[make, k] = tol32[k], np.nextafter(tol32[k], F(0))
            err[16, 0], err[17, 1], err[18, 2] = -tol32[0], -tol32[1], -tol32[2]
            err[19, 1] = F(TOLER[1] + 1e-9)    # rounds to (float)tol: a float64 comparison against 0.7 would let 0.69999999 pass
            levels[12:20] = (1, -1)
            levels[20:24] = [(2, 1), (-1, 2), (3, 1), (-3, -1)]
        elif r == 2:                           # a subset again, some of them failing by a wide margin
            ids = np.array([0, 3, 5, 8, 9, 11, 14, 20])
            err[3, 0], steps[9] = F(0.9), 10
        elif r == 3:                           # the same cell many times in one call: 3 x 0.125
            ids = np.arange(9, 24)
            levels[9:12] = (1, 1)
        else:                                  # saturation: ten successes in one cell, five in its neighbour
            levels[:10], levels[10:15] = (-1, 0), (-1, 1)
            ids = np.arange(15)
        vel = (cmd + err).astype(F)
        assert (np.abs(vel - cmd)[12:] == np.abs(err)[12:]).all() or r != 1
        env.episode_length_buf = torch.from_numpy(steps)
        env.commands = torch.from_numpy(cmd)
        env.filtered_lin_vel = torch.from_numpy(np.stack([vel[:, 0], vel[:, 1], np.zeros(N, F)], axis=1))
        env.filtered_ang_vel = torch.from_numpy(np.stack([np.zeros(N, F), np.zeros(N, F), vel[:, 2]], axis=1))
        env.env_curriculum_level = torch.from_numpy(levels.copy())
        env._update_curriculum(torch.from_numpy(ids))
        mask = np.zeros(N, np.int32)
        mask[ids] = 1
        rounds.append({"done": mask, "steps": steps.astype(np.int32), "levels": levels.astype(np.int32).copy(), "commands": cmd,
                       "lin_vel": env.filtered_lin_vel.numpy().copy(), "ang_vel": env.filtered_ang_vel.numpy().copy(),
                       "prob": env.curriculum_prob.numpy().copy()})
    for k in rounds[0]:
        out["a_" + k] = np.stack([r[k] for r in rounds])
    assert (out["a_prob"][-1] == 1.0).sum() >= 3 and out["a_prob"][1].sum() > out["a_prob"][0].sum()

    # ---- (b) _resample_commands, both branches ----
    uniforms, cells = [], []

    def rand_float(lower, upper, shape, device):
        u = torch.rand(*shape)
        uniforms.append(u.numpy().reshape(-1).copy())
        return (upper - lower) * u + lower

    real_multinomial = torch.multinomial

    def multinomial(*args, **kwargs):
        g = real_multinomial(*args, **kwargs)
        cells.append(g.numpy().copy())
        return g

    t1.torch_rand_float = rand_float
    torch.multinomial = multinomial
    try:
        for tag, curriculum, LL, AA in (("b_plain", False, L, A), ("b_cur", True, 3, 3)):
            Nb = 64
            del uniforms[:], cells[:]
            env = object.__new__(t1.T1)
            env.cfg = {"commands": {**cfg["commands"], "curriculum": curriculum, "lin_vel_levels": LL, "ang_vel_levels": AA}, "rewards": cfg["rewards"]}
            env.dt, env.device = DT, "cpu"
            env.episode_length_buf = torch.zeros(Nb, dtype=torch.long)
            env.cmd_resample_time = torch.zeros(Nb, dtype=torch.long)
            env.cmd_resample_time[::5] = 7                       # these do not resample
            env.commands = torch.full((Nb, 3), -9.0)
            env.gait_frequency = torch.full((Nb,), -9.0)
            env.env_curriculum_level = torch.zeros(Nb, 2, dtype=torch.long)
            prob = rng.uniform(0, 1, (2 * LL + 1, 2 * AA + 1)).astype(F)
            prob[rng.uniform(size=prob.shape) < 0.4] = 0.0
            env.curriculum_prob = torch.from_numpy(prob)
            env._resample_commands()
            ids = (env.episode_length_buf == 0).nonzero().flatten().numpy()
            out[tag + "_ids"] = np.nonzero(np.arange(Nb) % 5 != 0)[0].astype(np.int32)
            out[tag + "_uniforms"] = np.stack(uniforms)           # [4][n]: x, y, yaw, gait
            out[tag + "_commands"] = env.commands.numpy().copy()
            out[tag + "_gait_frequency"] = env.gait_frequency.numpy().copy()
            assert len(uniforms) == 4 and len(ids) == Nb
            if curriculum:
                out[tag + "_cells"] = cells[0].astype(np.int32)
                out[tag + "_levels"] = env.env_curriculum_level.numpy().astype(np.int32)
                out[tag + "_prob"] = prob
                out[tag + "_L"], out[tag + "_A"] = LL, AA
                assert (prob.reshape(-1)[cells[0]] > 0).all()
    finally:
        torch.multinomial = real_multinomial

    # ---- (c) apply_randomization ----
    variates = []
    real_randn, real_rand = torch.randn_like, torch.rand_like

    def recorded(fn):
        def wrapped(t):
            v = fn(t)
            variates.append(v.numpy().copy())
            return v
        return wrapped

    torch.randn_like, torch.rand_like = recorded(real_randn), recorded(real_rand)
    try:
        kick = torch.from_numpy(rng.uniform(-2, 2, (16, 3)).astype(F))
        specs = [("additive", "gaussian", (0.0, 0.5)), ("scaling", "gaussian", (1.0, 0.1)), ("additive", "uniform", (-0.3, 0.7)),
                 ("scaling", "uniform", (0.8, 1.25))]
        out["c_input"] = kick.numpy().copy()
        out["c_range"] = np.array([s[2] for s in specs])
        for k, (op, dist, rg) in enumerate(specs):
            for tag, x in (("kick", kick), ("zero", torch.zeros_like(kick))):
                del variates[:]
                y = utils.apply_randomization(x, {"distribution": dist, "operation": op, "range": list(rg)})
                out[f"c_{tag}_{k}_variate"], out[f"c_{tag}_{k}_result"] = variates[0], y.numpy().copy()
    finally:
        torch.randn_like, torch.rand_like = real_randn, real_rand

    path = os.path.join(HERE, "commands_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
