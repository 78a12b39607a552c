"""Every refusal of the tracker's array calls, word for word, without a GPU: one table of ``(call, exception type, full message)`` over
the fifteen host / device twins and the calls that take a listed subset.  The tracker is configured through a stand-in library; the
refused calls then run with ``_lib.lib`` patched to raise, so nothing may reach the library before the refusal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_tracker_tables_host import A, COLS, H, M, N, NB, NSEL, O, R, StandIn, configured_tracker  # noqa: E402

F, I = np.float32, np.int32
NDARRAY = "cannot take a device address from ndarray"        # what a NumPy array handed to a device entry point is told


def z(*shape, dtype=F):
    return np.zeros(shape, dtype)


def small(nbytes):
    """a ``DeviceBuffer`` of ``nbytes`` bytes that owns nothing"""
    from general_motion_retargeting_amd._lib import DeviceBuffer
    b = DeviceBuffer.__new__(DeviceBuffer)
    b.nbytes, b.ptr = nbytes, None
    return b


def refusals(t):
    roots, rows, steps = z(N, 13), z(N, R), z(N, dtype=I)
    body, pos, rot = z(N, NB, 13), z(N, NB, 3), z(N, NB, 4)
    extra = z(N, 1)
    roll = {"obs": z(H, N, O), "priv": z(H, N, 1), "actions": z(H, N, A), "rewards": z(H, N), "dones": z(H, N, dtype=np.uint8),
            "time_outs": z(H, N, dtype=np.uint8)}
    droll = {"obs": 1, "priv": 2, "actions": 3, "rewards": 4, "dones": 5, "time_outs": 6}
    loss = {"loc": z(M, A), "logstd": z(A), "actions": z(M, A), "old_log_prob": z(M), "values": z(M), "returns": z(M), "advantages": z(M)}
    dloss = dict.fromkeys(loss, 1)
    sim_links = sorted(("body_pos", "body_rot", "body_vel", "body_ang_vel"))
    rollout_arrays = sorted(roll)
    loss_inputs = ["loc", "logstd", "actions", "old_log_prob", "values", "returns", "advantages", "old_loc", "old_logstd"]
    return (
        # step
        (lambda: t.step({"base_pos": z(N, 4)}), ValueError, "base_pos: shape (3, 4), (3, 3) needed"),
        (lambda: t.step({"dof_pos": z(2, R)}), ValueError, "dof_pos: shape (2, 2), (3, 2) needed"),
        (lambda: t.step({"base": roots}), TypeError, "step: unknown simulator arrays ['base']"),
        (lambda: t.step_dev({"base": 1}), TypeError, "step_dev: unknown simulator arrays ['base']"),
        (lambda: t.step_dev(reward=1), TypeError, "step_dev: unknown outputs ['reward']"),
        (lambda: t.step_dev(total=z(N)), TypeError, f"total: {NDARRAY}"),
        (lambda: t.step_dev({"dof_vel": rows}), TypeError, f"dof_vel: {NDARRAY}"),
        (lambda: t.step_dev(ref_dof_pos=small(23)), ValueError, "ref_dof_pos: buffer of 23 bytes, 24 needed"),
        (lambda: t.step_dev({"base_quat": small(47)}), ValueError, "base_quat: buffer of 47 bytes, 48 needed"),
        # step_links
        (lambda: t.step_links(links={"body_pos": z(N, NSEL, 4)}), ValueError, "body_pos: shape (3, 2, 4), (3, 2, 3) needed"),
        (lambda: t.step_links(links={"body_rot": z(2, NSEL, 4)}), ValueError, "body_rot: shape (2, 2, 4), (3, 2, 4) needed"),
        (lambda: t.step_links(links={"body_state": z(2, NB, 13)}), ValueError, "body_state: shape (2, 4, 13), (3, nb, 13) needed"),
        (lambda: t.step_links(links={"body_state": z(N, NB, 12)}), ValueError, "body_state: shape (3, 4, 12), (3, nb, 13) needed"),
        (lambda: t.step_links(links={"body_state": z(N, 1, 13)}), ValueError, "sim_bodies reaches body 1, body_state has 1"),
        (lambda: t.step_links({"dof_pos": z(N, 3)}), ValueError, "dof_pos: shape (3, 3), (3, 2) needed"),
        (lambda: t.step_links(links={}), ValueError,
         f"links names none of {sim_links}: pass links=None for a step without the simulator's links"),
        (lambda: t.step_links(links={"body": 1}), TypeError, "step_links: unknown link arrays ['body']"),
        (lambda: t.step_links(links={"body_state": body, "body_pos": pos}), TypeError,
         "links is either {'body_state': [N, nb, 13]} or the four separate arrays"),
        (lambda: t.step_links({"base": 1}), TypeError, "step_links: unknown simulator arrays ['base']"),
        (lambda: t.step_links_dev({"base": 1}), TypeError, "step_links_dev: unknown simulator arrays ['base']"),
        (lambda: t.step_links_dev(reward=1), TypeError, "step_links_dev: unknown outputs ['reward']"),
        (lambda: t.step_links_dev(links={"body_state": 1}), ValueError, "a packed body_state on the device needs num_bodies (or a [N, nb, 13] shape)"),
        (lambda: t.step_links_dev(links={"body_state": 1, "num_bodies": 1}), ValueError, "sim_bodies reaches body 1, body_state has 1"),
        (lambda: t.step_links_dev(links={"body_state": body}), TypeError, f"body_state: {NDARRAY}"),
        (lambda: t.step_links_dev(links={"body_vel": z(N, NSEL, 3)}), TypeError, f"body_vel: {NDARRAY}"),
        (lambda: t.step_links_dev(fail=z(N, dtype=I)), TypeError, f"fail: {NDARRAY}"),
        (lambda: t.step_links_dev(links={"body_state": small(623), "num_bodies": NB}), ValueError, "body_state: buffer of 623 bytes, 624 needed"),
        (lambda: t.step_links_dev(links={"body_rot": small(95)}), ValueError, "body_rot: buffer of 95 bytes, 96 needed"),
        (lambda: t.step_links_dev(ref_body_rot=small(95)), ValueError, "ref_body_rot: buffer of 95 bytes, 96 needed"),
        (lambda: t.step_links_dev(max_dist=small(11)), ValueError, "max_dist: buffer of 11 bytes, 12 needed"),
        # preview (frame "sim")
        (lambda: t.preview({"base_pos": z(N, 4), "base_quat": z(N, 4)}), ValueError, "base_pos: shape (3, 4), (3, 3) needed"),
        (lambda: t.preview({"base_pos": z(N, 3), "base_quat": z(2, 4)}), ValueError, "base_quat: shape (2, 4), (3, 4) needed"),
        (lambda: t.preview(), ValueError, 'frame="sim" needs base_pos and base_quat of the simulator\'s root in sim'),
        (lambda: t.preview({"base_pos": z(N, 3)}), ValueError, 'frame="sim" needs base_pos and base_quat of the simulator\'s root in sim'),
        (lambda: t.preview({"base": 1}), TypeError, "preview: unknown simulator arrays ['base']"),
        (lambda: t.preview_dev({"base": 1}), TypeError, "preview_dev: unknown simulator arrays ['base']"),
        (lambda: t.preview_dev({"base_pos": z(N, 3), "base_quat": 1}), TypeError, f"base_pos: {NDARRAY}"),
        (lambda: t.preview_dev({"base_pos": small(35), "base_quat": 1}), ValueError, "base_pos: buffer of 35 bytes, 36 needed"),
        # targets and torques
        (lambda: t.targets(z(N, 3)), ValueError, "actions: shape (3, 3), (3, 2) needed"),
        (lambda: t.targets(z(2, R)), ValueError, "actions: shape (2, 2), (3, 2) needed"),
        (lambda: t.targets(episode_steps=z(2, dtype=I)), ValueError, "episode_steps: shape (2,), (3,) needed"),
        (lambda: t.targets(episode_steps=z(N)), TypeError, "episode_steps: integers needed, got float32"),
        (lambda: t.targets_dev(actions_clipped=1), ValueError, "targets_dev: actions_clipped needs actions"),
        (lambda: t.targets_dev(rows), TypeError, f"actions: {NDARRAY}"),
        (lambda: t.targets_dev(dof_targets=small(23)), ValueError, "dof_targets: buffer of 23 bytes, 24 needed"),
        (lambda: t.targets_dev(status=small(11)), ValueError, "status: buffer of 11 bytes, 12 needed"),
        (lambda: t.torques(0, z(N, 3), rows, rows, z(R), z(R)), ValueError, "dof_targets: shape (3, 3), (3, 2) needed"),
        (lambda: t.torques(0, rows, z(2, R), rows, z(R), z(R)), ValueError, "dof_pos: shape (2, 2), (3, 2) needed"),
        (lambda: t.torques(0, rows, rows, rows, z(R), None), ValueError, "torques: damping is needed"),
        (lambda: t.torques(0, rows, rows, rows, z(R), z(3)), ValueError,
         "torques: damping has shape (3,), (2,) needed (per_env = False: the three share one shape)"),
        (lambda: t.torques(0, rows, rows, rows, rows, rows, torque_limit=z(3)), ValueError, "torques: torque_limit has shape (3,), (2,) needed"),
        (lambda: t.torques(2, rows, rows, rows, rows, rows), ValueError, "torques: substep = 2 outside [0, 2)"),
        (lambda: t.torques_dev(0, 1, 1, 1, 1, 1, None), ValueError, "torques_dev: dof_torques is needed"),
        (lambda: t.torques_dev(0, 1, None, 1, 1, 1, 1), ValueError, "torques_dev: dof_pos is needed"),
        (lambda: t.torques_dev(0, 1, 1, 1, rows, 1, 1), TypeError, f"stiffness: {NDARRAY}"),
        (lambda: t.torques_dev(0, 1, 1, 1, 1, 1, 1, torque_limit=small(7)), ValueError, "torque_limit: buffer of 7 bytes, 8 needed"),
        (lambda: t.torques_dev(0, 1, 1, 1, small(23), 1, 1), ValueError, "stiffness: buffer of 23 bytes, 24 needed"),
        (lambda: t.torques_dev(0, 1, 1, 1, small(7), 1, 1, per_env=False), ValueError, "stiffness: buffer of 7 bytes, 8 needed"),
        (lambda: t.torques_dev(0, 1, 1, 1, 1, 1, 1, mean_torques=small(23)), ValueError, "mean_torques: buffer of 23 bytes, 24 needed"),
        # proprio (one extra column)
        (lambda: t.proprio(z(N, 12), rows, rows, extra=extra), ValueError, "root_states: shape (3, 12), (3, 13) needed"),
        (lambda: t.proprio(roots, z(2, R), rows, extra=extra), ValueError, "dof_pos: shape (2, 2), (3, 2) needed"),
        (lambda: t.proprio(roots, rows, rows, extra=z(N, 2)), ValueError, "extra: shape (3, 2), (3, 1) needed"),
        (lambda: t.proprio(roots, rows, rows, extra=extra, ground=z(N, 1)), ValueError, "ground: shape (3, 1), (3,) needed"),
        (lambda: t.proprio(roots, rows, rows, extra=extra, episode_steps=z(N)), TypeError, "episode_steps: integers needed, got float32"),
        (lambda: t.proprio(None, rows, rows, extra=extra), ValueError, "proprio: root_states is needed"),
        (lambda: t.proprio(roots, rows, rows), ValueError, "proprio: extra is needed exactly when extra_cols > 0 (extra_cols = 1, extra missing)"),
        (lambda: t.proprio_dev(1, 1, 1), ValueError, "proprio_dev: extra is needed exactly when extra_cols > 0 (extra_cols = 1, extra missing)"),
        (lambda: t.proprio_dev(1, 1, 1, extra=1, reward=1), TypeError, "proprio_dev: unknown outputs ['reward']"),
        (lambda: t.proprio_dev(1, None, 1, extra=1), ValueError, "proprio_dev: dof_pos is needed"),
        (lambda: t.proprio_dev(roots, 1, 1, extra=1), TypeError, f"root_states: {NDARRAY}"),
        (lambda: t.proprio_dev(1, 1, 1, extra=1, done=steps), TypeError, f"done: {NDARRAY}"),
        (lambda: t.proprio_dev(1, 1, 1, extra=small(11)), ValueError, "extra: buffer of 11 bytes, 12 needed"),
        (lambda: t.proprio_dev(1, 1, 1, extra=1, obs=small(155)), ValueError, "obs: buffer of 155 bytes, 156 needed"),
        (lambda: t.proprio_dev(1, 1, 1, extra=1, term=small(167)), ValueError, "term: buffer of 167 bytes, 168 needed"),
        # feet
        (lambda: t.feet({"body_state": z(N, NB, 12)}, roots), ValueError, "body_state: shape (3, 4, 12), (3, 4, 13) needed"),
        (lambda: t.feet({"body_pos": pos, "body_rot": z(2, NB, 4)}, roots), ValueError, "body_rot: shape (2, 4, 4), (3, 4, 4) needed"),
        (lambda: t.feet({"body_state": body}, z(2, 13)), ValueError, "root_states: shape (2, 13), (3, 13) needed"),
        (lambda: t.feet({"body_state": body}, roots, contact_forces=z(N, NB, 2)), ValueError, "contact_forces: shape (3, 4, 2), (3, 4, 3) needed"),
        (lambda: t.feet({"body_state": body}, roots, gait_frequency=z(N, 1)), ValueError, "gait_frequency: shape (3, 1), (3,) needed"),
        (lambda: t.feet({"body_state": body}, None), ValueError, "feet: root_states is needed"),
        (lambda: t.feet({"body_pos": pos}, roots), TypeError, "feet: bodies is either {'body_state': ..} or {'body_pos': .., 'body_rot': ..}, got ['body_pos']"),
        (lambda: t.feet(body, roots), TypeError, "feet: bodies is {'body_state': [N, nb, 13]} or {'body_pos': [N, nb, 3], 'body_rot': [N, nb, 4]}"),
        (lambda: t.feet_dev({"body_state": 1}, 1, reward=1), TypeError, "feet_dev: unknown outputs ['reward']"),
        (lambda: t.feet_dev({"body_state": 1}, None), ValueError, "feet_dev: root_states is needed"),
        (lambda: t.feet_dev({"body_state": body}, 1), TypeError, f"body_state: {NDARRAY}"),
        (lambda: t.feet_dev({"body_pos": 1, "body_rot": rot}, 1), TypeError, f"body_rot: {NDARRAY}"),
        (lambda: t.feet_dev({"body_state": 1}, roots), TypeError, f"root_states: {NDARRAY}"),
        (lambda: t.feet_dev({"body_state": small(623)}, 1), ValueError, "body_state: buffer of 623 bytes, 624 needed"),
        (lambda: t.feet_dev({"body_pos": small(143), "body_rot": 1}, 1), ValueError, "body_pos: buffer of 143 bytes, 144 needed"),
        (lambda: t.feet_dev({"body_state": 1}, 1, contact_forces=small(143)), ValueError, "contact_forces: buffer of 143 bytes, 144 needed"),
        (lambda: t.feet_dev({"body_state": 1}, 1, feet_pos=small(71)), ValueError, "feet_pos: buffer of 71 bytes, 72 needed"),
        # commands
        (lambda: t.commands(steps, lin_vel=z(N, 2)), ValueError, "lin_vel: shape (3, 2), (3, 3) needed"),
        (lambda: t.commands(z(2, dtype=I)), ValueError, "episode_steps: shape (2,), (3,) needed"),
        (lambda: t.commands(None), ValueError, "commands: episode_steps is needed"),
        (lambda: t.commands(steps, done=z(2, dtype=I)), ValueError, "done: shape (2,), (3,) needed"),
        (lambda: t.commands(steps, cmd_obs=(z(N, 3), 1)), ValueError, "cmd_obs: column 1 leaves no three columns in rows of 3"),
        (lambda: t.commands(steps, cmd_obs=z(2, 3)), ValueError, "cmd_obs: a writeable C-contiguous float32 array [N = 3, W] is needed"),
        (lambda: t.commands_dev(1, reward=1), TypeError, "commands_dev: unknown outputs ['reward']"),
        (lambda: t.commands_dev(None), ValueError, "commands_dev: episode_steps is needed"),
        (lambda: t.commands_dev(steps), TypeError, f"episode_steps: {NDARRAY}"),
        (lambda: t.commands_dev(1, commands=z(N, 3)), TypeError, f"commands: {NDARRAY}"),
        (lambda: t.commands_dev(1, ang_vel=small(35)), ValueError, "ang_vel: buffer of 35 bytes, 36 needed"),
        (lambda: t.commands_dev(1, term=small(47)), ValueError, "term: buffer of 47 bytes, 48 needed"),
        (lambda: t.commands_dev(1, cmd_obs=1, cmd_obs_stride=2), ValueError, "commands_dev: cmd_obs_stride = 2, at least 3 floats needed"),
        (lambda: t.commands_dev(1, cmd_obs=small(99), cmd_obs_stride=11), ValueError, "cmd_obs: buffer of 99 bytes, 100 needed"),
        # disturb
        (lambda: t.disturb(0, z(N, 12)), ValueError, "root_states: shape (3, 12), (3, 13) needed"),
        (lambda: t.disturb(0, z(2, 13)), ValueError, "root_states: shape (2, 13), (3, 13) needed"),
        (lambda: t.disturb(-1, roots), ValueError, "disturb: common_step = -1, a step count in [0, 2^32) is needed"),
        (lambda: t.disturb_dev(0), ValueError, "disturb_dev: a kick step needs root_states"),
        (lambda: t.disturb_dev(1, roots), TypeError, f"root_states: {NDARRAY}"),
        (lambda: t.disturb_dev(1, push_obs=small(71)), ValueError, "push_obs: buffer of 71 bytes, 72 needed"),
        (lambda: t.disturb_dev(1, push_force=1, push_force_stride=2), ValueError, "disturb_dev: push_force_stride = 2, at least 3 floats needed"),
        (lambda: t.disturb_dev(1, push_torque=small(107), push_torque_stride=12), ValueError, "push_torque: buffer of 107 bytes, 108 needed"),
        # reset_states
        (lambda: t.reset_states(roots, rows, rows, init_root_states=z(N, 12)), ValueError, "init_root_states: shape (3, 12), (3, 13) needed"),
        (lambda: t.reset_states(roots, rows, rows, env_ids=[0, 2], init_dof_pos=rows), ValueError, "init_dof_pos: shape (3, 2), (2, 2) needed"),
        (lambda: t.reset_states(z(2, 13), rows, rows), ValueError, "root_states: shape (2, 13), (3, 13) needed"),
        (lambda: t.reset_states(roots, rows, z(N, 3)), ValueError, "dof_vel: shape (3, 3), (3, 2) needed"),
        (lambda: t.reset_states(roots, rows, rows, delay_steps=z(N)), TypeError, "delay_steps: integers needed, got float32"),
        (lambda: t.reset_states(roots, rows, rows, env_ids=[1, 1]), ValueError, "reset_states: env_ids names an environment twice"),
        (lambda: t.reset_states(roots, rows, rows, mask=z(2, dtype=I)), ValueError, "mask: shape (2,), (3,) needed"),
        (lambda: t.reset_states(roots, rows, rows, env_ids=[1], mask=z(N, dtype=I)), ValueError, "mask: shape (3,), (1,) needed"),
        (lambda: t.reset_states_dev(1, None, 1), ValueError, "reset_states_dev: root_states, dof_pos and dof_vel are needed"),
        (lambda: t.reset_states_dev(1, 1, 1, env_ids=1), ValueError, "reset_states_dev: env_ids on the device needs n, the length of the list"),
        (lambda: t.reset_states_dev(1, 1, 1, n=2), ValueError, "reset_states_dev: without env_ids every environment is served: n = 2, num_envs = 3"),
        (lambda: t.reset_states_dev(roots, 1, 1), TypeError, f"root_states: {NDARRAY}"),
        (lambda: t.reset_states_dev(1, 1, 1, mask=steps), TypeError, f"mask: {NDARRAY}"),
        (lambda: t.reset_states_dev(1, 1, small(23)), ValueError, "dof_vel: buffer of 23 bytes, 24 needed"),
        (lambda: t.reset_states_dev(1, 1, 1, env_ids=1, n=2, init_dof_pos=small(15)), ValueError, "init_dof_pos: buffer of 15 bytes, 16 needed"),
        (lambda: t.reset_states_dev(1, 1, 1, env_ids=small(7), n=2), ValueError, "env_ids: buffer of 7 bytes, 8 needed"),
        # rewards
        (lambda: t.rewards(term=z(N, 5)), ValueError, "term: shape (3, 5), (3, 6) needed"),
        (lambda: t.rewards(extra=z(2, 1)), ValueError, "extra: shape (2, 1), (3, 1) needed"),
        (lambda: t.rewards(cmd_term=z(2, 4)), ValueError, "cmd_term: shape (2, 4), (3, 4) needed"),
        (lambda: t.rewards(done=z(N)), TypeError, "done: integers needed, got float32"),
        (lambda: t.rewards(flags=z(2, dtype=I)), ValueError, "flags: shape (2,), (3,) needed"),
        (lambda: t.rewards_dev(total=1), TypeError, "rewards_dev: unknown outputs ['total']"),
        (lambda: t.rewards_dev(term=z(N, 6)), TypeError, f"term: {NDARRAY}"),
        (lambda: t.rewards_dev(reset=steps), TypeError, f"reset: {NDARRAY}"),
        (lambda: t.rewards_dev(feet_term=small(95)), ValueError, "feet_term: buffer of 95 bytes, 96 needed"),
        (lambda: t.rewards_dev(scaled=small(4 * N * COLS - 1)), ValueError, f"scaled: buffer of {4 * N * COLS - 1} bytes, {4 * N * COLS} needed"),
        # record and advantages
        (lambda: t.record(0, roll, obs=z(N, 2)), ValueError, "record: obs: shape (3, 2), (3, 3) needed"),
        (lambda: t.record(0, roll, reward=z(2)), ValueError, "record: reward: shape (2,), (3,) needed"),
        (lambda: t.record(0, roll, done=z(2, dtype=I)), ValueError, "done: shape (2,), (3,) needed"),
        (lambda: t.record(0, {}, obs=z(N, O)), ValueError, "record: the rollout array 'obs' is needed"),
        (lambda: t.record(0, {"obs": z(H, N, 4)}, obs=z(N, O)), ValueError, "record: obs: shape (2, 3, 4), (2, 3, 3) needed"),
        (lambda: t.record(0, {"obs": z(H, N, O, dtype=np.float64)}, obs=z(N, O)), TypeError,
         "record: obs is written in place: a writeable C-contiguous float32 array is needed"),
        (lambda: t.record(0, {"values": 1}), ValueError, f"record: unknown rollout arrays ['values'] (known: {rollout_arrays})"),
        (lambda: t.record(H, roll), ValueError, "record: slot n = 2 outside [0, 2)"),
        (lambda: t.record_dev(0, {"values": 1}), ValueError, f"record_dev: unknown rollout arrays ['values'] (known: {rollout_arrays})"),
        (lambda: t.record_dev(0, {}, reward=1), ValueError, "record_dev: the rollout array 'rewards' is needed"),
        (lambda: t.record_dev(0, roll, obs=1), TypeError, f"obs: {NDARRAY}"),
        (lambda: t.record_dev(0, droll, obs=z(N, O)), TypeError, f"obs: {NDARRAY}"),
        (lambda: t.record_dev(0, {**droll, "obs": small(71)}, obs=1), ValueError, "obs: buffer of 71 bytes, 72 needed"),
        (lambda: t.record_dev(0, {**droll, "dones": small(5)}, done=1), ValueError, "dones: buffer of 5 bytes, 6 needed"),
        (lambda: t.record_dev(0, droll, obs=small(35)), ValueError, "obs: buffer of 35 bytes, 36 needed"),
        (lambda: t.record_dev(0, droll, done=small(11)), ValueError, "done: buffer of 11 bytes, 12 needed"),
        (lambda: t.advantages(roll, z(2, 2), z(N)), ValueError, "advantages: values (2, 2) and last_values (3,), (2, 3) and (3,) needed"),
        (lambda: t.advantages(roll, z(H, N), z(2)), ValueError, "advantages: values (2, 3) and last_values (2,), (2, 3) and (3,) needed"),
        (lambda: t.advantages({"dones": roll["dones"]}, z(H, N), z(N)), ValueError, "advantages: the rollout array 'rewards' is needed"),
        (lambda: t.advantages({**roll, "rewards": z(N, H)}, z(H, N), z(N)), ValueError, "advantages: rewards: shape (3, 2), (2, 3) needed"),
        (lambda: t.advantages_dev(droll, 1, 1, {"values": 1}), TypeError, "advantages_dev: unknown outputs ['values']"),
        (lambda: t.advantages_dev(droll, None, 1, {}), ValueError, "advantages_dev: values and last_values are needed"),
        (lambda: t.advantages_dev({}, 1, 1, {}), ValueError, "advantages_dev: the rollout array 'rewards' is needed"),
        (lambda: t.advantages_dev(roll, 1, 1, {}), TypeError, f"rewards: {NDARRAY}"),
        (lambda: t.advantages_dev(droll, 1, 1, {"stats": small(31)}), ValueError, "stats: buffer of 31 bytes, 32 needed"),
        (lambda: t.advantages_dev(droll, 1, 1, {"returns": small(23)}), ValueError, "returns: buffer of 23 bytes, 24 needed"),
        # log_prob and loss
        (lambda: t.log_prob(z(M, 3), z(A), z(M, A)), ValueError, "log_prob: loc: shape (6, 3), (6, 2) needed"),
        (lambda: t.log_prob(z(M, A), z(A), z(5, A)), ValueError, "log_prob: actions: shape (5, 2), (6, 2) needed"),
        (lambda: t.log_prob_dev(1, None, 1, 1), ValueError, "log_prob_dev: loc, logstd, actions and out are needed"),
        (lambda: t.log_prob_dev(z(M, A), 1, 1, 1), TypeError, f"loc: {NDARRAY}"),
        (lambda: t.log_prob_dev(1, 1, 1, small(23)), ValueError, "out: buffer of 23 bytes, 24 needed"),
        (lambda: t.log_prob_dev(1, small(7), 1, 1), ValueError, "logstd: buffer of 7 bytes, 8 needed"),
        (lambda: t.loss({**loss, "loc": z(M, 3)}), ValueError, "loss: loc: shape (6, 3), (6, 2) needed"),
        (lambda: t.loss({**loss, "values": z(5)}), ValueError, "loss: values: shape (5,), (6,) needed"),
        (lambda: t.loss({k: v for k, v in loss.items() if k != "values"}), ValueError, "loss: the input 'values' is needed"),
        (lambda: t.loss({**loss, "old_loc": z(M, A)}), ValueError, "loss: old_loc and old_logstd are given together, or neither"),
        (lambda: t.loss(loss, update_lr=True), ValueError, "loss: update_lr without old_loc and old_logstd: there is no KL to drive the learning rate"),
        (lambda: t.loss({**loss, "value": 1}), TypeError, f"loss: unknown inputs ['value'] (known: {loss_inputs})"),
        (lambda: t.loss_dev(dloss, {"loss": 1}), TypeError, "loss_dev: unknown outputs ['loss']"),
        (lambda: t.loss_dev({**dloss, "value": 1}, {}), TypeError, f"loss_dev: unknown inputs ['value'] (known: {loss_inputs})"),
        (lambda: t.loss_dev({k: 1 for k in loss if k != "returns"}, {}), ValueError, "loss_dev: the input 'returns' is needed"),
        (lambda: t.loss_dev(loss, {}), TypeError, f"loc: {NDARRAY}"),
        (lambda: t.loss_dev(dloss, {"terms": z(8, dtype=np.float64)}), TypeError, f"terms: {NDARRAY}"),
        (lambda: t.loss_dev({**dloss, "actions": small(47)}, {}), ValueError, "actions: buffer of 47 bytes, 48 needed"),
        (lambda: t.loss_dev(dloss, {"terms": small(63)}), ValueError, "terms: buffer of 63 bytes, 64 needed"),
        (lambda: t.loss_dev(dloss, {"grad_logstd": small(7)}), ValueError, "grad_logstd: buffer of 7 bytes, 8 needed"),
        # the listed subset: hold, proprio_reset, set_anchor, anchor_to_root, reset_done (reset_states is above)
        (lambda: t.hold(rows, env_ids=[2, 2]), ValueError, "hold: env_ids names an environment twice"),
        (lambda: t.hold(rows, mask=z(2, dtype=I)), ValueError, "mask: shape (2,), (3,) needed"),
        (lambda: t.hold(rows, env_ids=[0, 1]), ValueError, "dof_pos: shape (3, 2), (2, 2) needed"),
        (lambda: t.hold(rows, mask=z(N)), TypeError, "mask: a mask is bool or integer, got float32"),
        (lambda: t.hold_dev(1, env_ids=1), ValueError, "hold_dev: env_ids on the device needs n, the length of the list"),
        (lambda: t.hold_dev(1, n=2), ValueError, "hold_dev: without env_ids every environment is served: n = 2, num_envs = 3"),
        (lambda: t.hold_dev(None), ValueError, "hold_dev: dof_pos is needed"),
        (lambda: t.hold_dev(1, mask=small(11)), ValueError, "mask: buffer of 11 bytes, 12 needed"),
        (lambda: t.hold_dev(small(15), env_ids=1, n=2), ValueError, "dof_pos: buffer of 15 bytes, 16 needed"),
        (lambda: t.proprio_reset(roots, env_ids=[0, 0]), ValueError, "proprio_reset: env_ids names an environment twice"),
        (lambda: t.proprio_reset(roots, mask=z(4, dtype=I)), ValueError, "mask: shape (4,), (3,) needed"),
        (lambda: t.proprio_reset(roots, env_ids=[1]), ValueError, "root_states: shape (3, 13), (1, 13) needed"),
        (lambda: t.proprio_reset_dev(1, env_ids=1, n=-1), ValueError, "proprio_reset_dev: env_ids on the device needs n, the length of the list"),
        (lambda: t.proprio_reset_dev(1, n=4), ValueError, "proprio_reset_dev: without env_ids every environment is served: n = 4, num_envs = 3"),
        (lambda: t.proprio_reset_dev(None), ValueError, "proprio_reset_dev: root_states is needed"),
        (lambda: t.proprio_reset_dev(small(155)), ValueError, "root_states: buffer of 155 bytes, 156 needed"),
        (lambda: t.set_anchor(pos=z(N, 3), env_ids=[0, 1]), ValueError, "set_anchor: pos has shape (3, 3), (2, 3) needed"),
        (lambda: t.set_anchor(yaw=z(2)), ValueError, "set_anchor: yaw has shape (2,), (3,) needed"),
        (lambda: t.set_anchor_dev(pos=1), ValueError, "set_anchor_dev: anchors are not enabled on this tracker, call enable_anchors() first"),
        (lambda: t.anchor_to_root(z(N, 3), z(N, 4), env_ids=[1, 1, 2]), ValueError, "anchor_to_root: env_ids names an environment twice"),
        (lambda: t.anchor_to_root(z(N, 3), z(N, 4), mask=z(2, dtype=I)), ValueError, "mask: shape (2,), (3,) needed"),
        (lambda: t.anchor_to_root(z(N, 3), z(N, 3)), ValueError, "anchor_to_root: root_quat has shape (3, 3), (3, 4) needed"),
        (lambda: t.anchor_to_root(z(N, 3), z(N, 4), env_ids=[1]), ValueError, "anchor_to_root: root_pos has shape (3, 3), (1, 3) needed"),
        (lambda: t.reset_done(env_ids=[1, 1]), ValueError, "reset_done: env_ids names an environment twice"),
        (lambda: t.reset_done(done=z(2, dtype=I)), ValueError, "done: shape (2,), (3,) needed"),
        (lambda: t.reset_done(failed=z(N, dtype=I), env_ids=[0]), ValueError, "failed: shape (3,), (1,) needed"),
        (lambda: t.reset_done_dev(env_ids=1), ValueError, "reset_done_dev: env_ids on the device needs n, the length of the list"),
        (lambda: t.reset_done_dev(n=2), ValueError, "reset_done_dev: without env_ids the masks cover every environment: n = 2, num_envs = 3"),
        (lambda: t.reset_done_dev(done=steps), TypeError, f"done: {NDARRAY}"),
        (lambda: t.reset_done_dev(failed=small(11)), ValueError, "failed: buffer of 11 bytes, 12 needed"),
    )


def anchored(t):
    """the refusals of the two anchor calls on device memory, which need anchors that are enabled"""
    t._anchors = True
    return (
        (lambda: t.set_anchor_dev(pos=1, env_ids=1), ValueError, "set_anchor_dev: env_ids on the device needs n, the length of the list"),
        (lambda: t.set_anchor_dev(pos=1, n=2), ValueError, "set_anchor_dev: without env_ids every environment is served: n = 2, num_envs = 3"),
        (lambda: t.set_anchor_dev(pos=z(N, 3)), TypeError, f"pos: {NDARRAY}"),
        (lambda: t.set_anchor_dev(pos=small(35)), ValueError, "pos: buffer of 35 bytes, 36 needed"),
        (lambda: t.set_anchor_dev(yaw=small(7), env_ids=1, n=2), ValueError, "yaw: buffer of 7 bytes, 8 needed"),
        (lambda: t.anchor_to_root_dev(1, 1, env_ids=1), ValueError, "anchor_to_root_dev: env_ids on the device needs n, the length of the list"),
        (lambda: t.anchor_to_root_dev(1, 1, n=1), ValueError, "anchor_to_root_dev: without env_ids every environment is served: n = 1, num_envs = 3"),
        (lambda: t.anchor_to_root_dev(1, None), ValueError, "anchor_to_root_dev: root_pos and root_quat are needed"),
        (lambda: t.anchor_to_root_dev(1, z(N, 4)), TypeError, f"root_quat: {NDARRAY}"),
        (lambda: t.anchor_to_root_dev(1, small(47)), ValueError, "root_quat: buffer of 47 bytes, 48 needed"),
        (lambda: t.anchor_to_root_dev(1, 1, mask=small(3), env_ids=1, n=1), ValueError, "mask: buffer of 3 bytes, 4 needed"),
    )


def in_the_call(t):
    """the refusals that fire while the arguments of the library call are formed: the library is loaded by then, and not called"""
    droll = {"rewards": 4, "dones": 5, "time_outs": 6}
    return (
        (lambda: t.preview_dev({"base_pos": 1, "base_quat": 1}, obs=z(N, 2, 5)), TypeError, f"obs: {NDARRAY}"),
        (lambda: t.preview_dev({"base_pos": 1, "base_quat": 1}, obs=small(119)), ValueError, "obs: buffer of 119 bytes, 120 needed"),
        (lambda: t.preview_dev({"base_pos": 1, "base_quat": 1}, valid=small(23)), ValueError, "valid: buffer of 23 bytes, 24 needed"),
        (lambda: t.advantages_dev(droll, z(H, N), 1, {}), TypeError, f"values: {NDARRAY}"),
        (lambda: t.advantages_dev(droll, 1, small(11), {}), ValueError, "last_values: buffer of 11 bytes, 12 needed"),
    )


def test_every_refusal_of_the_array_calls_word_for_word(monkeypatch):
    from general_motion_retargeting_amd import _lib
    L = StandIn()
    monkeypatch.setattr(_lib, "lib", lambda: L)
    t = configured_tracker()
    reached = len(L.calls)

    def no_device():
        raise AssertionError("the library was touched")

    class Loaded:
        def __getattr__(self, name):
            return lambda *args: no_device()

    for table in (refusals, anchored, in_the_call):
        monkeypatch.setattr(_lib, "lib", Loaded if table is in_the_call else no_device)
        for i, (call, exc, message) in enumerate(table(t)):
            with pytest.raises(exc) as e:
                call()
            assert type(e.value) is exc, (table.__name__, i, message, repr(e.value))
            got = e.value.args[0] if e.value.args else ""
            assert got == message, (table.__name__, i, got, message)
    assert len(L.calls) == reached
