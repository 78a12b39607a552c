"""What the tracker's Python side hands the C-ABI, without a GPU: the array tables of ``_lib.py`` against the ctypes structs, the structs
every ``*_dev`` twin builds from raw addresses against literal values worked out by hand, and the arrays of every host twin read back
and written through the addresses the library would get.  ``lib()`` is a stand-in that records its arguments and returns 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_motion_body_state_host import _OfflineLibrary  # noqa: E402

N, R, NB, NSEL, EXTRA = 3, 2, 4, 2, 1
H, O, P, A = 2, 3, 1, 2                       # the rollout: slots, observation, privileged and action columns
M = H * N
COLS = 6 + 4 + 14 + 8 + 4 + 1                 # the reward columns: terms, links, proprio, feet, commands, one caller column
F, I = np.float32, np.int32


class StandIn:
    """``lib()``: every function records ``(name, arguments)``, runs the hook set for its name and returns 0 (a device is visible)"""

    def __init__(self):
        self.calls, self.hooks = [], {}

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name in self.hooks:
                self.hooks[name](args)
            return 1 if name == "gmr_device_count" else 0
        return fn

    def last(self, name):
        assert self.calls and self.calls[-1][0] == name, (name, self.calls[-1:] and self.calls[-1][0])
        return [plain(a) for a in self.calls[-1][1]]


def plain(a):
    """an argument as a literal: a struct behind ``byref`` as the dict of its fields, an address as a number"""
    a = getattr(a, "_obj", a)
    if isinstance(a, C.Structure):
        return {k: getattr(a, k) for k, _ in a._fields_}
    return a.value if isinstance(a, C.c_void_p) else a


def configured_tracker():
    """a tracker of N = 3 environments and R = 2 dofs with every block configured through the public calls; ``_lib.lib`` is a stand-in"""
    from general_motion_retargeting_amd import MotionTracker
    lib = _OfflineLibrary(R, "world")
    lib.num_clips = 1
    t = MotionTracker(lib, N, 0.02)
    t.set_control(np.zeros(R, F), 1.0, 1.0, decimation=2)
    t.set_proprio(np.zeros(R, F), np.stack([-np.ones(R, F), np.ones(R, F)], axis=1), np.ones(R, F), np.ones(R, F), base_height_target=0.7,
                  terminate_vel=50.0, terminate_height=0.3, max_episode_steps=100, extra_cols=EXTRA)
    t.set_feet([0, 1], np.zeros((1, 3), F), NB, feet_distance_ref=0.2, swing_period=0.5)
    t.set_commands((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0), (1.0, 2.0), (10, 20))
    t.set_disturbances(2, 3, 1)
    t.set_reset_states([0, 0, 0.7, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.zeros(R, F))
    t._links = (None, NSEL, np.arange(NSEL, dtype=I), "world")            # what set_links leaves, without a kinematics model
    t._preview = (2, ("root_pos", "dof_pos"), "sim", 0)                   # what set_preview leaves: K = 2 offsets, rows of 3 + R
    t.set_rewards(extra_names=["alive"])
    t.set_rollout(H, O, P, A, 0.99, 0.95)
    t.set_loss(0.0, 0.0, 0.01, 1e-3)
    return t


@pytest.fixture
def standin(monkeypatch):
    from general_motion_retargeting_amd import _lib
    L = StandIn()
    monkeypatch.setattr(_lib, "lib", lambda: L)
    return L


# ---- tables against structs -------------------------------------------------------------------------------------------------------------
TABLES = (("TrackerSim", "TRACKER_SIM"), ("TrackerOut", "TRACKER_OUT"), ("TrackerLinksSim", "TRACKER_LINKS_SIM"), ("TrackerLinksOut", "TRACKER_LINKS_OUT"),
          ("ProprioIn", "PROPRIO_IN"), ("ProprioOut", "PROPRIO_OUT"), ("FeetIn", "FEET_IN"), ("FeetOut", "FEET_OUT"), ("CommandsIn", "CMD_IN"),
          ("CommandsOut", "CMD_OUT"), ("DisturbIo", "DISTURB_IO"), ("ResetIo", "RESET_IO"), ("RewardIn", "REWARD_IN"), ("RewardOut", "REWARD_OUT"),
          ("RolloutIo", "ROLLOUT_IO"), ("RolloutOut", "ROLLOUT_OUT"), ("LossIn", "LOSS_IN"), ("LossOut", "LOSS_OUT"), ("BodyStateOut", "BODY_STATE"))


def test_every_table_names_the_address_fields_of_its_struct_in_order():
    from general_motion_retargeting_amd import _lib
    dims = {"N", "n", "R", "extra_cols", "obs_cols", "nb", "nsel", "C", "E", "H", "O", "P", "A", "M"}
    for struct, table in TABLES:
        rows, cls = getattr(_lib, table), getattr(_lib, struct)
        arrays = [r for r in rows if len(r) == 3]
        assert [r[0] for r in arrays] == [k for k, ct in cls._fields_ if ct is C.c_void_p], struct
        assert [r[0] for r in rows] == [k for k, _ in cls._fields_], struct
        assert tuple(r[0] for r in arrays) == getattr(_lib, table + "_FIELDS"), struct
        for name, dtype, shape in arrays:
            assert np.dtype(dtype).name == dtype and isinstance(shape, tuple), (struct, name)
            assert all(s in dims if isinstance(s, str) else isinstance(s, int) and s > 0 for s in shape), (struct, name, shape)


# ---- the structs of the device twins, literally -----------------------------------------------------------------------------------------
def a(k):
    return 0x1000 * k


def struct(names, **given):
    return {**dict.fromkeys(names), **given}


SIM = ("base_pos", "base_quat", "base_lin_vel", "base_ang_vel", "dof_pos", "dof_vel")
OUT = ("ref_root_pos", "ref_root_rot", "ref_root_vel", "ref_root_ang_vel", "ref_dof_pos", "ref_dof_vel", "err", "term", "total", "status", "finished")
LINKS_OUT = ("ref_body_pos", "ref_body_rot", "ref_body_vel", "ref_body_ang_vel", "link_err", "link_term", "max_dist", "fail")
PROPRIO_IN = ("root_states", "dof_pos", "dof_vel", "actions", "mean_torques", "extra", "ground", "episode_steps")
PROPRIO_OUT = ("base_lin_vel", "base_ang_vel", "projected_gravity", "filtered_lin_vel", "filtered_ang_vel", "obs", "priv", "term", "total", "done")
FEET_IN = ("contact_forces", "root_states", "episode_steps", "gait_frequency")
FEET_OUT = ("feet_pos", "feet_roll", "feet_yaw", "feet_contact", "ground", "gait", "term", "total", "done")
CMD_IN = ("episode_steps", "done", "lin_vel", "ang_vel")
CMD_OUT = ("term", "total", "commands", "gait_frequency", "flags", "cmd_obs")
RESET_IO = ("root_states", "dof_pos", "dof_vel", "delay_steps", "episode_steps", "init_root_states", "init_dof_pos", "init_dof_vel")
REWARD_IN = ("term", "link_term", "proprio_term", "feet_term", "cmd_term", "extra", "done", "flags")
REWARD_OUT = ("reward", "scaled", "group_total", "reset", "time_outs")
ROLLOUT_IO = ("obs", "priv", "actions", "rewards", "dones", "time_outs")
ROLLOUT_OUT = ("advantages", "returns", "normalized", "stats")
LOSS_IN = ("loc", "logstd", "actions", "old_log_prob", "values", "returns", "advantages", "old_loc", "old_logstd")
LOSS_OUT = ("grad_loc", "grad_logstd", "grad_values", "log_prob", "terms")


def links_sim(**given):
    return struct(("body_pos", "body_rot", "body_vel", "body_ang_vel"), **{"env_stride": 0, "body_stride": 0, **given})


def device_calls(t):
    """``(entry point, call, the arguments the library must get)`` for every ``*_dev`` twin, raw addresses ``0x1000 * k`` in"""
    io = {"obs": a(1), "actions": a(2), "rewards": a(3), "dones": a(4), "time_outs": a(5)}
    scan = {k: io[k] for k in ("rewards", "dones", "time_outs")}
    loss_in = {k: a(i + 1) for i, k in enumerate(LOSS_IN)}
    return (
        ("step", lambda: t.step_dev(), [None, None, struct(OUT), None]),
        ("step", lambda: t.step_dev({"base_pos": a(1), "dof_vel": a(2), "base_quat": None}, total=a(3), finished=a(4), err=None),
         [None, struct(SIM, base_pos=a(1), dof_vel=a(2)), struct(OUT, total=a(3), finished=a(4)), None]),
        ("step_links", lambda: t.step_links_dev({"base_pos": a(1), "base_quat": a(2)}, {"body_state": a(3), "num_bodies": NB}, advance=False,
                                                ref_body_pos=a(4), fail=a(5), term=a(6)),
         [None, struct(SIM, base_pos=a(1), base_quat=a(2)),
          links_sim(body_pos=a(3), body_rot=a(3) + 12, body_vel=a(3) + 28, body_ang_vel=a(3) + 40, env_stride=13 * NB, body_stride=13),
          struct(OUT, term=a(6)), struct(LINKS_OUT, ref_body_pos=a(4), fail=a(5)), 1, None]),
        ("step_links", lambda: t.step_links_dev(None, {"body_pos": a(1), "body_rot": a(2), "body_vel": None}, link_err=a(3)),
         [None, None, links_sim(body_pos=a(1), body_rot=a(2)), struct(OUT), struct(LINKS_OUT, link_err=a(3)), 0, None]),
        ("step_links", lambda: t.step_links_dev(status=a(1)), [None, None, None, struct(OUT, status=a(1)), struct(LINKS_OUT), 0, None]),
        ("preview", lambda: t.preview_dev({"base_pos": a(1), "base_quat": a(2)}, obs=a(3), status=a(4)),
         [None, struct(SIM, base_pos=a(1), base_quat=a(2)), a(3), None, a(4), None]),
        ("targets", lambda: t.targets_dev(a(1), a(2), dof_targets=a(3), actions_clipped=a(4), status=a(5)), [None, a(1), a(2), a(3), a(4), a(5), None]),
        ("targets", lambda: t.targets_dev(dof_targets=a(3)), [None, None, None, a(3), None, None, None]),
        ("torques", lambda: t.torques_dev(1, a(1), a(2), a(3), a(4), a(5), a(6), torque_limit=a(7), delay_steps=a(8), mean_torques=a(9)),
         [None, 1, a(1), a(2), a(3), {"stiffness": a(4), "damping": a(5), "friction": None, "torque_limit": a(7), "per_env": 1}, a(8), a(6), a(9), None]),
        ("torques", lambda: t.torques_dev(0, a(1), a(2), a(3), a(4), a(5), a(6), friction=a(7), per_env=False),
         [None, 0, a(1), a(2), a(3), {"stiffness": a(4), "damping": a(5), "friction": a(7), "torque_limit": None, "per_env": 0}, None, a(6), None, None]),
        ("proprio", lambda: t.proprio_dev(a(1), a(2), a(3), actions=a(4), extra=a(5), episode_steps=a(6), noise=False, obs=a(7), done=a(8), priv=None),
         [None, struct(PROPRIO_IN, root_states=a(1), dof_pos=a(2), dof_vel=a(3), actions=a(4), extra=a(5), episode_steps=a(6)), 0,
          struct(PROPRIO_OUT, obs=a(7), done=a(8)), None]),
        ("feet", lambda: t.feet_dev({"body_state": a(1)}, a(2), contact_forces=a(3), gait_frequency=a(4), ground=a(5), feet_contact=a(6)),
         [None, links_sim(body_pos=a(1), body_rot=a(1) + 12, env_stride=13 * NB, body_stride=13),
          struct(FEET_IN, contact_forces=a(3), root_states=a(2), gait_frequency=a(4)), struct(FEET_OUT, ground=a(5), feet_contact=a(6)), None]),
        ("feet", lambda: t.feet_dev({"body_pos": a(1), "body_rot": a(2)}, a(3), episode_steps=a(4), done=a(5)),
         [None, links_sim(body_pos=a(1), body_rot=a(2)), struct(FEET_IN, root_states=a(3), episode_steps=a(4)), struct(FEET_OUT, done=a(5)), None]),
        ("commands", lambda: t.commands_dev(a(1), done=a(2), cmd_obs=a(3), cmd_obs_stride=11, commands=a(4), flags=a(5)),
         [None, struct(CMD_IN, episode_steps=a(1), done=a(2)), struct(CMD_OUT, commands=a(4), flags=a(5), cmd_obs=a(3), cmd_obs_stride=11), None]),
        ("commands", lambda: t.commands_dev(a(1), lin_vel=a(2), ang_vel=a(3), term=a(4)),
         [None, struct(CMD_IN, episode_steps=a(1), lin_vel=a(2), ang_vel=a(3)), struct(CMD_OUT, term=a(4), cmd_obs_stride=0), None]),
        ("disturb", lambda: t.disturb_dev(6, root_states=a(1), push_force=a(2), push_obs=a(3), push_force_stride=3 * NB),
         [None, 6, {"root_states": a(1), "push_force": a(2), "push_torque": None, "push_force_stride": 3 * NB, "push_torque_stride": 0, "push_obs": a(3)},
          None]),
        ("reset_states", lambda: t.reset_states_dev(a(1), a(2), a(3), mask=a(4), env_ids=a(5), n=2, delay_steps=a(6), init_dof_pos=a(7), chain=True),
         [None, 2, a(5), a(4), struct(RESET_IO, root_states=a(1), dof_pos=a(2), dof_vel=a(3), delay_steps=a(6), init_dof_pos=a(7)), 1, None]),
        ("reset_states", lambda: t.reset_states_dev(a(1), a(2), a(3), episode_steps=a(4), init_root_states=a(5), init_dof_vel=a(6)),
         [None, N, None, None, struct(RESET_IO, root_states=a(1), dof_pos=a(2), dof_vel=a(3), episode_steps=a(4), init_root_states=a(5),
                                      init_dof_vel=a(6)), 0, None]),
        ("rewards", lambda: t.rewards_dev(term=a(1), proprio_term=a(2), extra=a(3), done=a(4), reward=a(5), time_outs=a(6)),
         [None, struct(REWARD_IN, term=a(1), proprio_term=a(2), extra=a(3), done=a(4)), struct(REWARD_OUT, reward=a(5), time_outs=a(6)), None]),
        ("record", lambda: t.record_dev(1, io, obs=a(6), actions=a(7), reward=a(8), done=a(9), time_outs=a(10)),
         [None, 1, struct(ROLLOUT_IO, **io), a(6), None, a(7), a(8), a(9), a(10), None]),
        ("advantages", lambda: t.advantages_dev(io, a(6), a(7), {"advantages": a(8), "stats": a(9)}),
         [None, struct(ROLLOUT_IO, **scan), a(6), a(7), struct(ROLLOUT_OUT, advantages=a(8), stats=a(9)), 1, None]),
        ("log_prob", lambda: t.log_prob_dev(a(1), a(2), a(3), a(4)), [None, a(1), a(2), a(3), a(4), None]),
        ("loss", lambda: t.loss_dev(loss_in, {"grad_loc": a(10), "terms": a(11)}, update_lr=True),
         [None, struct(LOSS_IN, **loss_in), struct(LOSS_OUT, grad_loc=a(10), terms=a(11)), 1, None]),
        ("loss", lambda: t.loss_dev({k: loss_in[k] for k in LOSS_IN[:7]}, {"log_prob": a(10)}),
         [None, struct(LOSS_IN, **{k: loss_in[k] for k in LOSS_IN[:7]}), struct(LOSS_OUT, log_prob=a(10)), 0, None]),
    )


def test_every_device_twin_hands_the_library_the_structs_worked_out_by_hand(standin):
    t = configured_tracker()
    for entry, call, want in device_calls(t):
        call()
        got = standin.last(f"gmr_motion_tracker_{entry}_dev")
        assert got == want, (entry, got, want)


# ---- the arrays of the host twins, live -------------------------------------------------------------------------------------------------
def view(address, shape, dtype):
    n = int(np.prod(shape, dtype=np.int64))
    return np.ctypeslib.as_array((C.c_uint8 * (n * np.dtype(dtype).itemsize)).from_address(address)).view(dtype).reshape(shape)


def rand(shape, dtype=F, seed=[0]):
    seed[0] += 1
    rng = np.random.default_rng(seed[0])
    return rng.integers(0, 5, shape).astype(dtype) if np.dtype(dtype).kind in "iu" else rng.standard_normal(shape).astype(dtype)


def host_call(standin, entry, call, ins, outs, at=None):
    """Runs ``call`` with a hook on ``entry`` that finds every name of ``ins`` (the arrays the caller gave, as the library is to see them)
    and of ``outs`` (``name: (shape, dtype)``) among the address fields of the structs and -- by position, ``at[name]`` -- the pointer
    arguments, compares the inputs and writes a counting pattern through the outputs.  Returns what the call returns and the patterns."""
    at, patterns, seen = at or {}, {}, []

    def hook(args):
        where = {}
        for x in args:
            x = getattr(x, "_obj", x)
            if isinstance(x, C.Structure):
                where.update({k: getattr(x, k) for k, ct in x._fields_ if ct is C.c_void_p})
        where.update({k: plain(args[i]) for k, i in at.items()})
        for k, want in ins.items():
            assert where[k], (entry, k)
            got = view(where[k], want.shape, want.dtype)
            assert np.array_equal(got, want), (entry, k)
        for i, (k, (shape, dtype)) in enumerate(outs.items()):
            assert where[k], (entry, k)
            patterns[k] = (np.arange(int(np.prod(shape)), dtype=np.int64) + 100 * (i + 1)).astype(dtype).reshape(shape)
            view(where[k], shape, dtype)[...] = patterns[k]
        seen.append({k for k, v in where.items() if v})

    standin.hooks = {entry: hook}
    got = call()
    assert len(seen) == 1, entry
    assert seen[0] == set(ins) | set(outs), (entry, seen[0] ^ (set(ins) | set(outs)))       # nothing else was handed over
    return got, patterns


def same(got, patterns, keys=None):
    for k in (patterns if keys is None else keys):
        assert isinstance(got[k], np.ndarray) and got[k].dtype == patterns[k].dtype and got[k].shape == patterns[k].shape, k
        assert np.array_equal(got[k], patterns[k]), k
    return True


def test_every_host_twin_hands_over_the_callers_arrays_and_returns_what_the_library_wrote(standin):
    t = configured_tracker()
    P_ = "gmr_motion_tracker_"
    sim = {"base_pos": rand((N, 3)), "base_quat": rand((N, 4)), "base_lin_vel": rand((N, 3)), "base_ang_vel": rand((N, 3)), "dof_pos": rand((N, R)),
           "dof_vel": rand((N, R))}
    step_out = {"ref_root_pos": ((N, 3), F), "ref_root_rot": ((N, 4), F), "ref_root_vel": ((N, 3), F), "ref_root_ang_vel": ((N, 3), F),
                "ref_dof_pos": ((N, R), F), "ref_dof_vel": ((N, R), F), "err": ((N, 6), F), "term": ((N, 6), F), "total": ((N,), F),
                "status": ((N,), I), "finished": ((N,), I)}
    bare = {k: v for k, v in step_out.items() if k not in ("err", "term", "total")}
    # step
    got, pat = host_call(standin, P_ + "step", lambda: t.step(sim), sim, step_out)
    assert same(got, pat) and list(got) == list(step_out)
    got, pat = host_call(standin, P_ + "step", lambda: t.step(), {}, bare)
    assert same(got, pat) and list(got) == list(bare)
    # step_links: the packed tensor (every field an offset into it) and the separate arrays
    ref_links = {"ref_body_pos": ((N, NSEL, 3), F), "ref_body_rot": ((N, NSEL, 4), F), "ref_body_vel": ((N, NSEL, 3), F), "ref_body_ang_vel": ((N, NSEL, 3), F)}
    link_out = {**ref_links, "link_err": ((N, 4), F), "link_term": ((N, 4), F), "max_dist": ((N,), F), "fail": ((N,), I)}
    body = rand((N, NB, 13))
    flat = body.reshape(-1)
    packed = {"body_pos": flat[0:], "body_rot": flat[3:], "body_vel": flat[7:], "body_ang_vel": flat[10:]}
    got, pat = host_call(standin, P_ + "step_links", lambda: t.step_links(sim, {"body_state": body}), {**sim, **packed}, {**step_out, **link_out})
    assert same(got, pat) and list(got) == list(step_out) + list(link_out)
    strides = plain(standin.calls[-1][1][2])
    assert (strides["env_stride"], strides["body_stride"]) == (13 * NB, 13)
    sep = {"body_pos": rand((N, NSEL, 3)), "body_rot": rand((N, NSEL, 4)), "body_vel": rand((N, NSEL, 3)), "body_ang_vel": rand((N, NSEL, 3))}
    got, pat = host_call(standin, P_ + "step_links", lambda: t.step_links(None, sep, advance=False), sep,
                         {**{k: v for k, v in bare.items()}, "total": ((N,), F), **link_out})
    assert same(got, pat) and standin.last(P_ + "step_links")[5] == 1
    got, pat = host_call(standin, P_ + "step_links", lambda: t.step_links(), {}, {**bare, **ref_links})
    assert same(got, pat)
    # preview
    got, pat = host_call(standin, P_ + "preview", lambda: t.preview(sim), {k: sim[k] for k in ("base_pos", "base_quat")},
                         {"obs": ((N, 2, 3 + R), F), "valid": ((N, 2), I), "status": ((N,), I)}, at={"obs": 2, "valid": 3, "status": 4})
    assert same(got, pat) and list(got) == ["obs", "valid", "status"]
    # targets and torques
    act, steps = rand((N, R)), rand((N,), I)
    got, pat = host_call(standin, P_ + "targets", lambda: t.targets(act, steps), {"actions": act, "episode_steps": steps},
                         {"dof_targets": ((N, R), F), "actions_clipped": ((N, R), F), "status": ((N,), I)},
                         at={"actions": 1, "episode_steps": 2, "dof_targets": 3, "actions_clipped": 4, "status": 5})
    assert same(got, pat) and list(got) == ["dof_targets", "status", "actions_clipped"]
    got, pat = host_call(standin, P_ + "targets", lambda: t.targets(), {}, {"dof_targets": ((N, R), F), "status": ((N,), I)},
                         at={"actions": 1, "episode_steps": 2, "dof_targets": 3, "actions_clipped": 4, "status": 5})
    assert same(got, pat)
    tg, q, qd, kp, kd, fr, lim, delay = rand((N, R)), rand((N, R)), rand((N, R)), rand((R,)), rand((R,)), rand((R,)), rand((R,)), rand((N,), I)
    got, pat = host_call(standin, P_ + "torques", lambda: t.torques(1, tg, q, qd, kp, kd, fr, lim, delay),
                         {"dof_targets": tg, "dof_pos": q, "dof_vel": qd, "stiffness": kp, "damping": kd, "friction": fr, "torque_limit": lim, "delay_steps": delay},
                         {"dof_torques": ((N, R), F), "mean_torques": ((N, R), F)},
                         at={"dof_targets": 2, "dof_pos": 3, "dof_vel": 4, "delay_steps": 6, "dof_torques": 7, "mean_torques": 8})
    assert same(got, pat) and plain(standin.calls[-1][1][5])["per_env"] == 0
    # proprio
    pin = {"root_states": rand((N, 13)), "dof_pos": rand((N, R)), "dof_vel": rand((N, R)), "actions": rand((N, R)), "mean_torques": rand((N, R)),
           "extra": rand((N, EXTRA)), "ground": rand((N,)), "episode_steps": rand((N,), I)}
    pout = {"base_lin_vel": ((N, 3), F), "base_ang_vel": ((N, 3), F), "projected_gravity": ((N, 3), F), "filtered_lin_vel": ((N, 3), F),
            "filtered_ang_vel": ((N, 3), F), "obs": ((N, 6 + EXTRA + 3 * R), F), "priv": ((N, 4), F), "term": ((N, 14), F), "total": ((N,), F),
            "done": ((N,), I)}
    got, pat = host_call(standin, P_ + "proprio", lambda: t.proprio(**pin), pin, pout)
    assert same(got, pat) and list(got) == list(pout) and standin.last(P_ + "proprio")[2] == 1
    few = {k: pin[k] for k in ("root_states", "dof_pos", "dof_vel", "extra")}
    got, pat = host_call(standin, P_ + "proprio", lambda: t.proprio(**few, noise=False), few, pout)
    assert same(got, pat)
    # feet: packed (body_rot 12 bytes behind body_pos) and separate
    fin = {"root_states": rand((N, 13)), "contact_forces": rand((N, NB, 3)), "episode_steps": rand((N,), I), "gait_frequency": rand((N,))}
    fout = {"feet_pos": ((N, 2, 3), F), "feet_roll": ((N, 2), F), "feet_yaw": ((N, 2), F), "feet_contact": ((N, 2), I), "ground": ((N,), F),
            "gait": ((N, 2), F), "term": ((N, 8), F), "total": ((N,), F), "done": ((N,), I)}
    got, pat = host_call(standin, P_ + "feet", lambda: t.feet({"body_state": body}, **fin), {**fin, "body_pos": flat[0:], "body_rot": flat[3:]}, fout)
    assert same(got, pat) and list(got) == list(fout)
    strides = plain(standin.calls[-1][1][1])
    assert (strides["env_stride"], strides["body_stride"]) == (13 * NB, 13)
    two = {"body_pos": rand((N, NB, 3)), "body_rot": rand((N, NB, 4))}
    got, pat = host_call(standin, P_ + "feet", lambda: t.feet(two, fin["root_states"]), {**two, "root_states": fin["root_states"]}, fout)
    assert same(got, pat)
    # commands: the done mask arrives as 0 / 1, cmd_obs as the address of its first command column
    done = np.array([0, 3, 0], I)
    lin, ang, rows = rand((N, 3)), rand((N, 3)), rand((N, 7))
    cout = {"term": ((N, 4), F), "total": ((N,), F), "commands": ((N, 3), F), "gait_frequency": ((N,), F), "flags": ((N,), I)}
    got, pat = host_call(standin, P_ + "commands", lambda: t.commands(pin["episode_steps"], done, lin, ang, cmd_obs=(rows, 2)),
                         {"episode_steps": pin["episode_steps"], "done": (done != 0).astype(I), "lin_vel": lin, "ang_vel": ang, "cmd_obs": rows.reshape(-1)[2:]},
                         cout)
    assert same(got, pat) and list(got) == list(cout) and standin.last(P_ + "commands")[2]["cmd_obs_stride"] == 7
    # disturb: a copy of the root states goes in and comes back
    roots = rand((N, 13))
    dout = {"root_states": ((N, 13), F), "push_force": ((N, 3), F), "push_torque": ((N, 3), F), "push_obs": ((N, 6), F)}
    got, pat = host_call(standin, P_ + "disturb", lambda: t.disturb(4, roots), {"root_states": roots}, dout)
    assert got["actions"] == 0 and same(got, pat, ["root_states"]) and got["push_force"] is None and got["root_states"] is not roots
    io = standin.last(P_ + "disturb")[2]
    assert (io["push_force_stride"], io["push_torque_stride"]) == (3, 3)
    # reset_states: copies of the simulator's arrays, the init rows by list position
    rin = {"root_states": rand((N, 13)), "dof_pos": rand((N, R)), "dof_vel": rand((N, R)), "delay_steps": rand((N,), I), "episode_steps": rand((N,), I)}
    init = {"init_root_states": rand((2, 13)), "init_dof_pos": rand((2, R)), "init_dof_vel": rand((2, R))}
    ids, mask = np.array([2, 0], I), np.array([1, 0], I)
    got, pat = host_call(standin, P_ + "reset_states", lambda: t.reset_states(**rin, **init, env_ids=ids, mask=mask, chain=True),
                         {**rin, **init, "env_ids": ids, "mask": mask}, {k: (v.shape, v.dtype.type) for k, v in rin.items()}, at={"env_ids": 2, "mask": 3})
    assert same(got, pat) and got["ignored"] == 0 and list(got) == list(rin) + ["ignored"] and all(got[k] is not rin[k] for k in rin)
    assert standin.last(P_ + "reset_states")[1] == 2 and standin.last(P_ + "reset_states")[5] == 1
    # rewards
    win = {"term": rand((N, 6)), "link_term": rand((N, 4)), "proprio_term": rand((N, 14)), "feet_term": rand((N, 8)), "cmd_term": rand((N, 4)),
           "extra": rand((N, 1)), "done": rand((N,), I), "flags": rand((N,), I)}
    wout = {"reward": ((N,), F), "scaled": ((N, COLS), F), "group_total": ((N, 2), F), "reset": ((N,), I), "time_outs": ((N,), I)}
    got, pat = host_call(standin, P_ + "rewards", lambda: t.rewards(**win), win, wout)
    assert same(got, pat) and list(got) == list(wout)
    # record: the caller's rollout arrays as they lie, the step's rows by position
    roll = {"obs": rand((H, N, O)), "priv": rand((H, N, P)), "actions": rand((H, N, A)), "rewards": rand((H, N)), "dones": rand((H, N), np.uint8),
            "time_outs": rand((H, N), np.uint8)}
    row = {"obs": rand((N, O)), "priv": rand((N, P)), "actions": rand((N, A)), "reward": rand((N,)), "done": rand((N,), I), "time_outs": rand((N,), I)}
    seen = []
    standin.hooks = {P_ + "record": lambda args: seen.append(
        [np.shares_memory(view(plain(args[2])[k], v.shape, v.dtype), v) for k, v in roll.items()]
        + [np.array_equal(view(plain(args[3 + i]), v.shape, v.dtype), v) for i, v in enumerate(row.values())])}
    assert t.record(1, roll, **row) is None and seen == [[True] * 12] and standin.last(P_ + "record")[1] == 1
    # advantages
    values, last = rand((H, N)), rand((N,))
    scan = {k: roll[k] for k in ("rewards", "dones", "time_outs")}
    aout = {"advantages": ((H, N), F), "returns": ((H, N), F), "normalized": ((H, N), F), "stats": ((4,), np.float64)}
    got, pat = host_call(standin, P_ + "advantages", lambda: t.advantages(roll, values, last), {**scan, "values": values, "last_values": last}, aout,
                         at={"values": 2, "last_values": 3})
    assert same(got, pat) and list(got) == list(aout) and standin.last(P_ + "advantages")[5] == 1
    # log_prob and loss
    loc, logstd, actions = rand((M, A)), rand((A,)), rand((H, N, A))
    got, pat = host_call(standin, P_ + "log_prob", lambda: {"out": t.log_prob(loc, logstd, actions)}, {"loc": loc, "logstd": logstd, "actions": actions},
                         {"out": ((M,), F)}, at={"loc": 1, "logstd": 2, "actions": 3, "out": 4})
    assert same(got, pat)
    lin_ = {"loc": loc, "logstd": logstd, "actions": actions, "old_log_prob": rand((M,)), "values": rand((H, N)), "returns": rand((M,)),
            "advantages": rand((M,)), "old_loc": rand((M, A)), "old_logstd": rand((A,))}
    lout = {"grad_loc": ((M, A), F), "grad_logstd": ((A,), F), "grad_values": ((M,), F), "log_prob": ((M,), F), "terms": ((8,), np.float64)}
    got, pat = host_call(standin, P_ + "loss", lambda: t.loss(lin_, update_lr=True), lin_, lout)
    assert same(got, pat) and list(got) == list(lout) and standin.last(P_ + "loss")[3] == 1
