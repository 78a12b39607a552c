"""The tracker's velocity commands, curriculum, kicks and pushes on a real MI355X (csrc/gmr_tracker_commands.hip through motion_tracker.py,
DESIGN.md section 6s): state and outputs are the float32 statement of tests/commands_mirror.py bit for bit -- scripted episodes with and
without the curriculum, both index orders, absent inputs, the command columns inside an observation row, parameter sets enqueued back to
back on a stream of the caller's --, the tracking terms against the float64 evaluation of the exactly formed float32 argument, uniform kicks
and pushes bit for bit and gaussian ones against the float64 evaluation of the same Philox words.  N = 37 environments (no multiple of 16 or
64) on the four-clip library of test_tracker_control.py, 64 guard floats behind every device output; every test makes one pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import commands_mirror as cm  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from test_motion_tracker import STATE, tracker  # noqa: E402
from test_tracker_control import G, SENTINEL, hip, same, world  # noqa: E402,F401
from test_tracker_proprio import GAUSSIAN_BOUND, GAUSSIAN_MEASURED  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
N, DT = 37, 0.02
RANGES = dict(lin_vel_x=(-1.0, 1.3), lin_vel_y=(-0.4, 0.4), ang_vel_yaw=(-1.1, 0.9), gait_frequency=(1.0, 2.2), resample_steps=(3, 9))
PLAIN = dict(still_proportion=0.2, tracking_sigma=0.25, scales={"survival": 0.25, "tracking_lin_vel_x": 1.0, "tracking_ang_vel": 0.5},
             obs_scales=(2.0, 2.0, 0.25))          # tracking_lin_vel_y: weight zero, the term is computed and stays out of the total
COUNTS = {"term": 4, "total": 1, "commands": 3, "gait_frequency": 1, "flags": 1}
CMD_STATE = ("commands", "gait_frequency", "cmd_resample_time", "cmd_draws")
CUR_STATE = CMD_STATE + ("env_level", "curriculum_prob", "hits", "cum")


def curriculum(L=3, A=2, rate=0.125, order="grid", min_success=4):
    return dict(lin_vel_levels=L, ang_vel_levels=A, update_rate=rate, tolerances=(0.2, 0.15, 0.3), resolutions=(0.2, 0.1, 0.3),
                min_success_steps=min_success, index_order=order)


def setup(world, n=N, seed=3, **kw):
    """a tracker on the world's library with commands set, and its mirror"""
    t = tracker(world["lib"], n, DT, world["map"], np.zeros(len(world["map"]), F), seed=seed)
    t.reset()                                             # clips, clocks and draw counters that are not zero
    kw = {**RANGES, **PLAIN, **kw}
    t.set_commands(**kw)
    return t, cm.Commands(cm.config(**kw), n, seed)


def run_dev(hip, t, x, stream=None, want=tuple(COUNTS), obs=None, sync=True):
    """commands_dev into guarded buffers -> the outputs on the host, the guard floats checked; obs: (host rows [n, W], column)"""
    n = t.num_envs
    up = {k: None if a is None else hip.DeviceBuffer.from_host(np.ascontiguousarray(a)) for k, a in x.items()}
    out = {k: hip.DeviceBuffer.from_host(np.full(n * COUNTS[k] + G, SENTINEL, dtype=F)) for k in want}
    kw = {}
    if obs is not None:
        rows, col = obs
        d_obs = hip.DeviceBuffer.from_host(np.concatenate([rows.reshape(-1), np.full(G, SENTINEL, F)]))
        kw = dict(cmd_obs=d_obs.ptr.value + 4 * col, cmd_obs_stride=rows.shape[1])
    t.commands_dev(**up, stream=stream, **out, **kw)

    def collect():
        hip.check(hip.lib().gmr_stream_sync(None if stream is None else stream.ptr))
        got = {}
        for k, b in out.items():
            raw = b.to_host(n * COUNTS[k] + G, F)
            assert (raw[n * COUNTS[k]:] == SENTINEL).all(), k                  # the guard floats
            a = raw[:n * COUNTS[k]]
            got[k] = a.view(np.int32).copy() if k == "flags" else (a.copy() if COUNTS[k] == 1 else a.reshape(n, COUNTS[k]).copy())
        if obs is not None:
            raw = d_obs.to_host(rows.size + G, F)
            assert (raw[rows.size:] == SENTINEL).all(), "cmd_obs"
            got["cmd_obs_rows"] = raw[:rows.size].reshape(rows.shape).copy()
        return got
    return collect() if sync else (collect, up, out)


def check(got, want, t, m, what, keys=CMD_STATE):
    for k in ("commands", "gait_frequency", "flags"):
        if k in got:
            same(got[k], want[k], (what, k))
    if "term" in got:
        print_and_bound_terms(got, want, m, what)
    st, ms = t.command_state(), m.state()
    for k in keys:
        same(st[k], ms[k], (what, k))
    return st


WORST = {"term": 0.0}


def print_and_bound_terms(got, want, m, what):
    """term and total within 2e-6 max(1, |w|) of the float64 evaluation of the exactly formed float32 argument (close_terms of
    tests/test_motion_tracker.py)"""
    for k, w in (("term", want["term64"]), ("total", want["total64"])):
        if k not in got:
            continue
        dev = np.abs(got[k].astype(D) - w) / np.maximum(1.0, np.abs(w))
        WORST["term"] = max(WORST["term"], float(dev.max()))
        assert got[k].dtype == F and (dev <= 2e-6).all(), (what, k, dev.max())


def episode(rng, t, m, hip, steps, n=N, p_done=0.08, vel_scale=0.15, keys=CMD_STATE, stream=None, every=None):
    """a scripted episode: everybody resamples at step 0, then the caller's increment, a scripted done mask, the call, the caller's reset"""
    count = np.zeros(n, np.int32)
    seen = 0
    for s in range(steps):
        if s:
            count += 1
        done = (rng.uniform(size=n) < p_done).astype(np.int32) if s else np.zeros(n, np.int32)
        st = t.command_state() if s else None
        # velocities near the commands, so that tolerances are met by some and missed by others
        base = m.commands if st is None else st["commands"]
        lin = (base + rng.normal(0, vel_scale, (n, 3))).astype(F)
        ang = (base[:, [2, 1, 2]] + rng.normal(0, vel_scale, (n, 3))).astype(F)
        x = {"episode_steps": count, "done": done if s % 7 else done.astype(bool).astype(np.int32) * 5, "lin_vel": lin, "ang_vel": ang}
        if every is not None:
            every(s)
        got = run_dev(hip, t, x, stream=stream)
        want = m.step(count, done, lin, ang)
        state = check(got, want, t, m, s, keys)
        if "hits" in keys:
            assert not state["hits"].any()
        seen |= int(np.bitwise_or.reduce(got["flags"]))
        count[done != 0] = 0
    return seen


# ---- 1. no curriculum ------------------------------------------------------------------------------------------------------------------
def test_sixty_scripted_steps_without_a_curriculum_are_the_mirrors_bits(hip, world):
    rng = np.random.default_rng(71)
    t, m = setup(world)
    before = t.state()
    assert (before["draws"] > 0).all()
    seen = episode(rng, t, m, hip, 60)
    assert seen == cm.BOUNDARY | cm.RESAMPLED                    # no curriculum: the success bit is never set
    st = t.command_state()
    assert st["cmd_draws"].min() >= 5 and (st["commands"][st["gait_frequency"] == 0] == 0).all() and (st["gait_frequency"] == 0).any()
    assert "env_level" not in st
    after = t.state()
    for k in STATE:
        same(before[k], after[k], k)
    print(f"tracking terms: largest deviation from float64 {WORST['term']:.3e} of max(1, |w|) (bound 2e-6)")


# ---- 2. the curriculum -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.125, 0.1])
def test_eighty_steps_with_a_curriculum_are_the_mirrors_bits(hip, world, rate):
    rng = np.random.default_rng(72)
    t, m = setup(world, curriculum=curriculum(rate=rate))
    st = t.command_state()
    assert st["curriculum_prob"].shape == (7, 5) and st["curriculum_prob"][3, 2] == 1 and st["curriculum_prob"].sum() == 1 and not st["cum"].any()
    seen = episode(rng, t, m, hip, 80, p_done=0.12, keys=CUR_STATE)
    assert seen == cm.BOUNDARY | cm.RESAMPLED | cm.SUCCESS
    st = t.command_state()
    assert (st["curriculum_prob"] > 0).sum() > 5 and np.abs(st["env_level"]).max() >= 1
    assert st["max_lin_vel_level"] == np.abs(m.env_level[:, 0]).max() and st["max_ang_vel_level"] == np.abs(m.env_level[:, 1]).max()
    assert st["mean_lin_vel_level"] == float(np.mean(np.abs(m.env_level[:, 0]).astype(F)))
    assert (np.diff(st["cum"]) >= 0).all() and (np.diff(st["cum"])[st["curriculum_prob"].reshape(-1) == 0] == 0).all()


# ---- 3. the reference's index order ----------------------------------------------------------------------------------------------------
def test_the_reference_order_on_a_square_grid_is_the_mirrors_and_the_fixtures(hip, world):
    rng = np.random.default_rng(73)
    t, m = setup(world, curriculum=curriculum(3, 3, order="reference"))
    episode(rng, t, m, hip, 30, p_done=0.2, keys=CUR_STATE)
    st = t.command_state()
    assert (st["env_level"][:, 0] != st["env_level"][:, 1]).any()
    # every level pair the device stored is the one the reference's own run (the fixture) gave the same cell (t1.py:417-418)
    with np.load(os.path.join(GOLDEN, "commands_golden.npz"), allow_pickle=False) as z:
        cells, ids, levels = z["b_cur_cells"], z["b_cur_ids"], z["b_cur_levels"]
        assert int(z["b_cur_L"]) == int(z["b_cur_A"]) == 3
    lin, ang = cm.split_cell(cells, 3, 3, "reference")
    assert (lin == levels[ids, 0]).all() and (ang == levels[ids, 1]).all()
    fixture = {int(g): tuple(int(v) for v in levels[i]) for g, i in zip(cells, ids)}
    device_cells = (st["env_level"][:, 1] + 3) * 7 + (st["env_level"][:, 0] + 3)         # the cell a stored pair came from, "reference" order
    met = [g for g in device_cells.tolist() if g in fixture]
    assert len(met) >= 5
    for e, g in enumerate(device_cells.tolist()):
        if g in fixture:
            assert tuple(st["env_level"][e].tolist()) == fixture[g], (e, g)


# ---- 4. many successes in one cell -----------------------------------------------------------------------------------------------------
def succeed(hip, t, m, n, done, want=()):
    """one call in which every done environment meets every tolerance: the velocities are its commands; steps = 1 > min_success = 0"""
    c = t.command_state()["commands"]
    x = {"episode_steps": np.ones(n, np.int32), "done": done.astype(np.int32), "lin_vel": c, "ang_vel": c}
    got = run_dev(hip, t, x, want=want)
    m.step(x["episode_steps"], x["done"], c, c)
    return got


def everybody_draws(hip, t, m, n):
    zeros = np.zeros((n, 3), F)
    x = {"episode_steps": np.zeros(n, np.int32), "done": None, "lin_vel": zeros, "ang_vel": zeros}
    run_dev(hip, t, x, want=())
    m.step(x["episode_steps"], None, zeros, zeros)


def test_five_thousand_successes_in_the_centre_cell_add_exactly(hip, world):
    n, rate = 5000, 2.0 ** -14                           # rate * hits and every sum of them are exact in float32
    t, m = setup(world, n=n, curriculum=curriculum(rate=rate, min_success=0), still_proportion=0.0)
    everybody_draws(hip, t, m, n)                        # the centre cell: the only one with weight
    st = t.command_state()
    assert not st["env_level"].any() and (st["cmd_draws"] == 1).all()
    got = succeed(hip, t, m, n, np.ones(n, bool), want=("flags",))
    assert (got["flags"] & cm.SUCCESS).all()
    st = check({}, {}, t, m, "stencil", CUR_STATE)
    want = np.zeros((7, 5), F)
    for c in ((2, 2), (4, 2), (3, 1), (3, 3)):
        want[c] = F(rate) * F(n)                         # 5000 / 16384, exactly
    want[3, 2] = 1.0                                     # 1 + 5000 / 16384, clamped
    same(st["curriculum_prob"], want, "stencil")
    assert not st["hits"].any() and st["cum"][-1] == 1.0 + 4 * 5000 / 16384


def test_successes_in_a_corner_cell_reach_its_three_cells_in_the_grid_alone(hip, world):
    """The levels are the tracker's state, so the corner is reached the way a run reaches it: two rounds of successes give its cell weight,
    then it is drawn (3 x 3 grid: the corner lies two cells from the centre)."""
    n, rate = 5000, 2.0 ** -14
    t, m = setup(world, n=n, curriculum=curriculum(1, 1, rate=rate, min_success=0), still_proportion=0.0)
    everybody_draws(hip, t, m, n)
    for _ in range(2):
        succeed(hip, t, m, n, np.ones(n, bool))
    st = check({}, {}, t, m, "walk", CUR_STATE)
    at = (st["env_level"] == (-1, -1)).all(axis=1)       # the corner cell (0, 0)
    k = int(at.sum())
    assert k >= 20, k
    before = st["curriculum_prob"].copy()
    assert (before[[0, 0, 1], [0, 1, 0]] < 0.6).all()    # room to grow below the clamp
    got = succeed(hip, t, m, n, at, want=("flags",))
    assert ((got["flags"] & cm.SUCCESS) != 0).tolist() == at.tolist()
    st = check({}, {}, t, m, "corner", CUR_STATE)
    want = before.copy()
    for c in ((0, 0), (0, 1), (1, 0)):
        want[c] = F(want[c] + F(rate) * F(k))            # exact
    same(st["curriculum_prob"], want, "corner")


# ---- 5. absent inputs ------------------------------------------------------------------------------------------------------------------
def test_absent_inputs_and_outputs(hip, world):
    rng = np.random.default_rng(75)
    t, m = setup(world)
    count = np.zeros(N, np.int32)
    lin, ang = rng.normal(0, 0.3, (N, 3)).astype(F), rng.normal(0, 0.3, (N, 3)).astype(F)
    check(run_dev(hip, t, {"episode_steps": count, "done": None, "lin_vel": lin, "ang_vel": ang}), m.step(count, None, lin, ang), t, m, "no done")
    count += 3
    # no velocities without a curriculum: the three tracking terms are 0 and stay out of the total
    got = run_dev(hip, t, {"episode_steps": count, "done": None, "lin_vel": None, "ang_vel": None})
    check(got, m.step(count, None, None, None), t, m, "no velocities")
    assert (got["term"] == np.array([1, 0, 0, 0], F)).all() and (got["total"] == F(0.25)).all()
    # only the angular velocity
    got = run_dev(hip, t, {"episode_steps": count, "done": None, "lin_vel": None, "ang_vel": ang})
    want = m.step(count, None, None, ang)
    check(got, want, t, m, "ang only")
    assert not got["term"][:, 1:3].any() and (got["term"][:, 3] > 0).all()
    # every output NULL: the state moves all the same
    count[:] = t.command_state()["cmd_resample_time"]
    run_dev(hip, t, {"episode_steps": count, "done": None, "lin_vel": lin, "ang_vel": ang}, want=())
    m.step(count, None, lin, ang)
    st = check({}, {}, t, m, "no outputs")
    assert (st["cmd_resample_time"] > count).all()
    # no velocities with a curriculum: GMR_ERR_ARG
    tc, _ = setup(world, curriculum=curriculum())
    table_in, table_out = hip.CommandsIn(episode_steps=hip.DeviceBuffer.from_host(count).ptr.value), hip.CommandsOut()
    import ctypes as C
    assert hip.lib().gmr_motion_tracker_commands_dev(tc.handle, C.byref(table_in), C.byref(table_out), None) == -1
    assert b"lin_vel" in hip.lib().gmr_last_error()
    with pytest.raises(ValueError, match="curriculum needs"):
        tc.commands(count)
    assert not tc.command_state()["cmd_draws"].any()


# ---- 6. the command columns of an observation row ----------------------------------------------------------------------------------------
def test_cmd_obs_lands_in_columns_six_to_eight_of_a_row_and_nowhere_else(hip, world):
    rng = np.random.default_rng(76)
    t, m = setup(world)
    W = 6 + 5 + 3 * 23
    rows = rng.normal(0, 1, (N, W)).astype(F)
    count = np.zeros(N, np.int32)
    got = run_dev(hip, t, {"episode_steps": count, "done": None, "lin_vel": None, "ang_vel": None}, obs=(rows, 6))
    want = m.step(count, None, None, None)
    same(got["cmd_obs_rows"][:, 6:9], want["cmd_obs"], "cmd_obs")
    same(got["cmd_obs_rows"][:, 6:9], (got["commands"] * np.array([2.0, 2.0, 0.25], F)).astype(F), "commands * scale")
    keep = np.ones(W, bool)
    keep[6:9] = False
    same(got["cmd_obs_rows"][:, keep], rows[:, keep], "the other columns")
    assert got["commands"].any()
    # the synchronous twin writes the same columns of a host array in place
    t2, _ = setup(world)
    host = rows.copy()
    out = t2.commands(count, cmd_obs=(host, 6))
    same(host, got["cmd_obs_rows"], "host rows")
    same(out["commands"], got["commands"], "host commands")


# ---- 7. parameter sets back to back on a stream -----------------------------------------------------------------------------------------
def test_three_parameter_sets_enqueued_back_to_back_each_use_their_own(hip, world):
    rng = np.random.default_rng(77)
    sets = [dict(lin_vel_x=(-1.0, 1.3)), dict(lin_vel_x=(5.0, 6.0), still_proportion=0.0, tracking_sigma=1.0, obs_scales=(1.0, 1.0, 1.0)),
            dict(lin_vel_x=(-9.0, -8.0), gait_frequency=(3.0, 4.0), still_proportion=0.5, resample_steps=(1, 2))]
    (ta, m), (tb, _) = setup(world), setup(world)
    st = hip.Stream()
    count = np.zeros(N, np.int32)
    lin, ang = rng.normal(0, 0.3, (N, 3)).astype(F), rng.normal(0, 0.3, (N, 3)).astype(F)
    pending, host, want = [], [], []
    for s, kw in enumerate(sets):
        kw = {**RANGES, **PLAIN, **kw}
        x = {"episode_steps": count.copy(), "done": None, "lin_vel": lin, "ang_vel": ang}
        tb.set_commands(**kw, keep_state=True)            # replaces the configuration alone: nothing waits for the stream
        pending.append(run_dev(hip, tb, x, stream=st, sync=False))
        ta.set_commands(**kw, keep_state=True)
        host.append(ta.commands(count, None, lin, ang))
        want.append(m.step(count, None, lin, ang, cfg=cm.config(**kw)))
        count[:] = m.cmd_resample_time                    # everybody resamples again in the next call
    for s, (collect, _, _) in enumerate(pending):
        got = collect()
        for k in COUNTS:
            same(got[k], host[s][k], (s, k))              # the synchronous twin gives the same bytes
        for k in ("commands", "gait_frequency", "flags"):
            same(got[k], want[s][k], (s, k))
    lo = [(-1.0, 1.3), (5.0, 6.0), (-9.0, -8.0)]
    for s in range(3):
        c = host[s]["commands"][:, 0]
        live = host[s]["gait_frequency"] != 0
        assert live.any() and (c[live] >= lo[s][0]).all() and (c[live] <= lo[s][1]).all()
    a, b = ta.command_state(), tb.command_state()
    for k in CMD_STATE:
        same(a[k], b[k], k)
        same(a[k], m.state()[k], k)
    tb._commands = ((3, 2),)                              # past the wrapper's own check: the library refuses a change of shape too
    with pytest.raises(hip.GmrHipError, match="keep_state"):
        tb.set_commands(**RANGES, curriculum=curriculum(), keep_state=True)


# ---- 8. one environment; the other halves are untouched --------------------------------------------------------------------------------
def test_one_environment_and_nothing_else_of_the_tracker_moves(hip, world):
    from test_tracker_feet import setup as feet_setup
    (ta, _, _), (tb, _, _) = (feet_setup(world, np.random.default_rng(780), n=1) for _ in range(2))
    kw = {**RANGES, **PLAIN, "curriculum": curriculum()}
    ta.set_commands(**kw)
    ta.set_disturbances(**PERIODS, **UNIFORM)
    m = cm.Commands(cm.config(**kw), 1, 3)
    rng = np.random.default_rng(78)
    count = np.zeros(1, np.int32)
    for s in range(12):
        done = np.array([s in (4, 9)], np.int32)
        lin, ang = (m.commands + rng.normal(0, 0.05, (1, 3))).astype(F), (m.commands + rng.normal(0, 0.05, (1, 3))).astype(F)
        x = {"episode_steps": count, "done": done, "lin_vel": lin, "ang_vel": ang}
        got = run_dev(hip, ta, x) if s % 2 else ta.commands(count, done, lin, ang)
        check(got, m.step(count, done, lin, ang), ta, m, s, CUR_STATE)
        ta.disturb(s, rng.normal(0, 1, (1, 13)).astype(F))
        disturb_dev(hip, ta, s, rng.normal(0, 1, (1, 13)).astype(F), n=1)
        count = np.where(done != 0, 0, count + 1).astype(np.int32)
    for name in ("state", "proprio_state", "feet_state"):
        a, b = getattr(ta, name)(), getattr(tb, name)()
        for k in b:
            if isinstance(b[k], np.ndarray):
                same(a[k], b[k], (name, k))
            else:
                assert a[k] == b[k], (name, k)
    a, b = ta.step(), tb.step()
    assert set(a) == set(b)
    for k in b:
        same(a[k], b[k], ("step", k))


# ---- 9. kicks and pushes ---------------------------------------------------------------------------------------------------------------
UNIFORM = dict(kick_lin_vel={"distribution": "uniform", "operation": "additive", "range": (-0.5, 0.7)},
               kick_ang_vel={"distribution": "uniform", "operation": "scaling", "range": (0.5, 1.5)},
               push_force={"distribution": "uniform", "operation": "additive", "range": (-40.0, 60.0)},
               push_torque={"distribution": "uniform", "operation": "scaling", "range": (0.5, 1.5)})
GAUSS = dict(kick_lin_vel={"distribution": "gaussian", "operation": "additive", "range": (0.0, 0.5)},
             kick_ang_vel={"distribution": "gaussian", "operation": "additive", "range": (0.1, 0.8)},
             push_force={"distribution": "gaussian", "operation": "additive", "range": (0.0, 30.0)},
             push_torque={"distribution": "gaussian", "operation": "additive", "range": (0.0, 5.0)})
PERIODS = dict(kick_every=6, push_every=10, push_duration=3)
NB, BASE = 11, 4


def disturb_dev(hip, t, step, root, n=N, stream=None):
    """disturb_dev with the push landing in guarded [n][NB][3] tensors at body BASE -> (actions, root, forces, torques, push_obs)"""
    d_root = hip.DeviceBuffer.from_host(np.concatenate([root.reshape(-1), np.full(G, SENTINEL, F)]))
    fill = np.full(n * NB * 3 + G, SENTINEL, F)
    d_f, d_t = hip.DeviceBuffer.from_host(fill), hip.DeviceBuffer.from_host(fill)
    d_obs = hip.DeviceBuffer.from_host(np.full(n * 6 + G, SENTINEL, F))
    act = t.disturb_dev(step, d_root, push_force=d_f.ptr.value + 4 * BASE * 3, push_torque=d_t.ptr.value + 4 * BASE * 3, push_obs=d_obs,
                        push_force_stride=NB * 3, push_torque_stride=NB * 3, stream=stream)
    hip.check(hip.lib().gmr_stream_sync(None if stream is None else stream.ptr))
    r, f, q, o = d_root.to_host(n * 13 + G, F), d_f.to_host(n * NB * 3 + G, F), d_t.to_host(n * NB * 3 + G, F), d_obs.to_host(n * 6 + G, F)
    for raw, size in ((r, n * 13), (f, n * NB * 3), (q, n * NB * 3), (o, n * 6)):
        assert (raw[size:] == SENTINEL).all()
    return act, r[:n * 13].reshape(n, 13), f[:n * NB * 3].reshape(n, NB, 3), q[:n * NB * 3].reshape(n, NB, 3), o[:n * 6].reshape(n, 6)


def test_uniform_kicks_and_pushes_are_the_mirrors_bits_and_idle_steps_launch_nothing(hip, world):
    rng = np.random.default_rng(79)
    seed = 11
    t = tracker(world["lib"], N, DT, world["map"], np.zeros(len(world["map"]), F), seed=seed)
    kw = {**PERIODS, **UNIFORM, "scale_push_force": 0.01, "scale_push_torque": 0.1}
    t.set_disturbances(**kw)
    cfg = cm.disturb_config(**kw)
    before = t.state()
    seen = set()
    for step in (0, 1, 3, 6, 10, 13, 30, 7, 2 ** 32 - 6):
        root = rng.normal(0, 1, (N, 13)).astype(F)
        act, r, f, q, o = disturb_dev(hip, t, step, root)
        want_act, wr, wf, wq, wo = cm.disturb(cfg, N, seed, step, root)
        assert act == want_act == t.disturb_actions(step, 6, 10, 3), step
        seen.add(act)
        same(r, wr, (step, "root_states"))                # idle and push-only steps leave it as it was
        others = np.ones(NB, bool)
        others[BASE] = False
        assert (f[:, others] == SENTINEL).all() and (q[:, others] == SENTINEL).all()          # no other body is touched
        if wf is None:
            assert (f == SENTINEL).all() and (q == SENTINEL).all() and (o == SENTINEL).all(), step        # nothing was written
        else:
            same(f[:, BASE], wf, (step, "push_force"))
            same(q[:, BASE], wq, (step, "push_torque"))
            same(o, wo, (step, "push_obs"))
            if act & cm.PUSH_STOP:
                assert not f[:, BASE].any() and not q[:, BASE].any() and not o.any()
            else:
                assert f[:, BASE].all() and not q[:, BASE].any()           # a scaling of zero is zero (utils/utils.py:23)
        host = t.disturb(step, root)                      # the synchronous twin
        assert host["actions"] == act
        same(host["root_states"], wr, (step, "host root"))
        if wf is None:
            assert host["push_force"] is None and host["push_obs"] is None
        else:
            same(host["push_force"], wf, (step, "host force"))
            same(host["push_torque"], wq, (step, "host torque"))
            same(host["push_obs"], wo, (step, "host obs"))
    assert seen == {0, 1, 2, 3, 4}
    after = t.state()
    for k in STATE:
        same(before[k], after[k], k)


def test_a_block_without_a_spec_is_left_alone_and_a_draw_depends_on_seed_environment_and_step_alone(hip, world):
    rng = np.random.default_rng(80)
    seed, big = 12, 5000
    kw = {**PERIODS, "kick_ang_vel": UNIFORM["kick_ang_vel"], "push_torque": UNIFORM["push_force"]}
    small = tracker(world["lib"], N, DT, world["map"], np.zeros(len(world["map"]), F), seed=seed)
    large = tracker(world["lib"], big, DT, world["map"], np.zeros(len(world["map"]), F), seed=seed)
    cfg = cm.disturb_config(**kw)
    root = rng.normal(0, 1, (big, 13)).astype(F)
    out = []
    for t, n in ((small, N), (large, big)):
        t.set_disturbances(**kw)
        act, r, f, q, o = disturb_dev(hip, t, 30, root[:n].copy(), n=n)
        assert act == cm.KICK | cm.PUSH_START
        same(r[:, :10], root[:n, :10], "kick_lin_vel has no spec")
        assert (r[:, 10:] != root[:n, 10:]).all() and not f[:, BASE].any() and q[:, BASE].all() and not o[:, :3].any()
        out.append((r, q, o))
    for a, b in zip(*out):
        same(a, b[:N], "the same draws among 5 000 environments")
    _, wr, wf, wq, wo = cm.disturb(cfg, N, seed, 30, root[:N])
    same(out[0][0], wr, "root_states")
    same(out[0][1][:, BASE], wq, "push_torque")


def test_gaussian_kicks_and_pushes_against_the_float64_evaluation_of_the_same_words(hip, world):
    """Largest deviation met on an MI355X: see DESIGN.md section 6s (the bound is GAUSSIAN_BOUND of tests/test_tracker_proprio.py, four
    times the 1.598e-6 measured there for the same recipe, plus one ulp of the result)."""
    rng = np.random.default_rng(81)
    seed = 13
    t = tracker(world["lib"], N, DT, world["map"], np.zeros(len(world["map"]), F), seed=seed)
    kw = {**PERIODS, **GAUSS, "scale_push_force": 0.01, "scale_push_torque": 0.1}
    t.set_disturbances(**kw)
    cfg = cm.disturb_config(**kw)
    root = rng.normal(0, 1, (N, 13)).astype(F)
    act, r, f, q, o = disturb_dev(hip, t, 60, root)
    assert act == cm.KICK | cm.PUSH_START
    _, wr, wf, wq, wo = cm.disturb(cfg, N, seed, 60, root, wide=True)
    same(r[:, :7], root[:, :7], "pose")
    worst, zmax = 0.0, 0.0
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for i in range(12):
        s = cfg["specs"][i // 3]
        a, b = float(s["a"]), float(s["m"])
        z = np.array([cm.draw(s, key, e, 60, i, wide=True) for e in range(N)])
        got = (r[:, 7 + i] if i < 6 else (f if i < 9 else q)[:, BASE, (i - 6) % 3]).astype(D)
        want = (wr[:, 7 + i] if i < 6 else (wf if i < 9 else wq)[:, (i - 6) % 3])
        x = root[:, 7 + i].astype(D) if i < 6 else 0.0
        assert np.allclose(want, x + a + b * z, rtol=0, atol=1e-12)
        unit = b * np.maximum(1.0, np.abs(z))
        ulp = np.spacing(np.abs(got).astype(F)).astype(D)
        dev = (np.abs(got - want) - ulp) / unit
        worst, zmax = max(worst, float(dev.max())), max(zmax, float(np.abs(z).max()))
        assert (np.abs(got - want) <= GAUSSIAN_BOUND * unit + ulp).all(), (i, dev.max())
    print(f"gaussian kicks and pushes: largest deviation from float64 {worst:.3e} of b max(1, |z|) beyond one ulp of the result "
          f"(measured for the recipe {GAUSSIAN_MEASURED}, bound {GAUSSIAN_BOUND}; a quarter of the bound is {GAUSSIAN_BOUND / 4:.3e})")
    assert zmax > 2.0
    # push_obs is the applied push times its scale, one float32 product
    same(o[:, :3], (f[:, BASE] * F(0.01)).astype(F), "push_obs force")
    same(o[:, 3:], (q[:, BASE] * F(0.1)).astype(F), "push_obs torque")
