"""The tracker's reset states, reward total and episode statistics on a real MI355X (csrc/gmr_tracker_episode.hip through motion_tracker.py,
DESIGN.md section 6t): the simulator's rows, the reward outputs and the statistics are the statement of tests/episode_mirror.py bit for bit
-- except the two yaw components of a reset quaternion, bounded against the float64 evaluation of the exactly formed float32 half angle --,
at N = 37 with R = 23 and R = 5, N = 1 and N = 5 000 (several workgroups: the chain of the partial sums) on the four-clip library of
test_tracker_control.py, 64 guard floats behind every device output; every test makes one pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_mirror as em  # noqa: E402
import feet_mirror as fm  # noqa: E402
from test_motion_tracker import STATE, tracker  # noqa: E402
from test_tracker_commands import PLAIN, RANGES  # noqa: E402
from test_tracker_control import G, SENTINEL, hip, same, world  # noqa: E402,F401
from test_tracker_feet import BORDER, FEET, HS, NB, PENALIZED, SCALES as FEET_SCALES, TERMINATION, VS, edges_of  # noqa: E402
from test_tracker_proprio import SCALES as PROPRIO_SCALES  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
DT = 0.02
YAW_BOUND = 2e-6                        # one libm call of magnitude <= 1 (the bound of section 6s)
ISENT = np.int32(-7725)
SHAPES = [(37, 23), (37, 5), (1, 23), (5000, 23)]
UNI = {"init_dof_pos": {"distribution": "uniform", "operation": "additive", "range": (-0.1, 0.1)},
       "init_base_pos_xy": {"distribution": "uniform", "operation": "scaling", "range": (0.5, 1.5)},
       "init_base_lin_vel_xy": {"distribution": "uniform", "operation": "additive", "range": (-0.5, 0.5)}}
TERM_WEIGHTS = (1.0, 0.5, 0.0, 0.25, 2.0, 0.125)          # root_vel: weight zero
NXF, NYF = 64, 48
WORST = {"yaw": 0.0}


def dmap_of(world, r):
    return world["map"] if r == 23 else world["map"][[0, 1, 2, 4, 5]]


def field_of(rng):
    return (rng.integers(-20, 60, (NXF, NYF)) + 5 * np.arange(NXF)[:, None]).astype(np.int16)


def guarded(a):
    """a device buffer of ``a`` with 64 guard words behind it"""
    from general_motion_retargeting_amd import _lib
    a = np.ascontiguousarray(a)
    tail = np.full(G, SENTINEL, F) if a.dtype == F else np.full(G, ISENT).astype(a.dtype)
    return _lib.DeviceBuffer.from_host(np.concatenate([a.reshape(-1), tail]))


def fetch(buf, like):
    """the array back on the host, the guard words checked"""
    raw = buf.to_host(like.size + G, like.dtype)
    assert (raw[like.size:] == (SENTINEL if like.dtype == F else np.full(1, ISENT).astype(like.dtype)[0])).all(), "guard"
    return raw[:like.size].reshape(like.shape).copy()


def sim_arrays(rng, n, r):
    return {"root_states": rng.normal(0, 1, (n, 13)).astype(F), "dof_pos": rng.normal(0, 1, (n, r)).astype(F), "dof_vel": rng.normal(0, 1, (n, r)).astype(F),
            "delay_steps": rng.integers(50, 60, n).astype(np.int32), "episode_steps": rng.integers(1, 90, n).astype(np.int32)}


def reset_setup(world, rng, n, r, seed=11, terrain=True, control=False, proprio=False, **kw):
    """a tracker with reset states set (and, asked for, terrain, control and proprio), and its mirror"""
    t = tracker(world["lib"], n, DT, dmap_of(world, r), rng.uniform(-0.4, 0.4, r).astype(F), seed=seed)
    t.reset()
    ter = None
    if terrain:
        field = field_of(rng)
        t.set_terrain(field, HS, VS, BORDER)
        ter = fm.terrain(field, HS, VS, BORDER)
    pose = rng.uniform(-0.6, 0.6, r).astype(F)
    if control:
        t.set_control(pose, 0.25, 0.75, 2.0, 0.1, 0.2, decimation=4)
    if proprio:
        set_proprio(t, rng, r)
    base = np.concatenate([[0.3, 0.2, 0.72], [0.0, 0.0, 0.0, 1.0], rng.normal(0, 0.2, 6)]).astype(F)
    args = dict(env_origins=rng.uniform(0.5, 3.0, (n, 2)).astype(F), decimation=7, **{**UNI, **kw})
    t.set_reset_states(base, pose, **args)
    return t, em.Resets(em.reset_config(base, pose, **args), n, r, seed, ter)


def set_proprio(t, rng, r, scales=PROPRIO_SCALES):
    lim = np.sort(rng.uniform(-2.0, 2.0, (r, 2)), axis=1).astype(F)
    lim[:, 1] += F(0.5)
    t.set_proprio(rng.uniform(-0.6, 0.6, r).astype(F), lim, rng.uniform(3, 12, r).astype(F), rng.uniform(10, 60, r).astype(F), base_height_target=0.68,
                  terminate_vel=50.0, terminate_height=0.3, max_episode_steps=30, extra_cols=0, filter_weight=0.1, scales=scales)


def reset_dev(t, sim, mask=None, env_ids=None, chain=False, **init):
    """reset_states_dev on guarded copies of ``sim`` -> the arrays after, and the device root buffer (for the terrain check)"""
    d = {k: guarded(a) for k, a in sim.items()}
    n = None if env_ids is None else len(env_ids)
    extra = {k: guarded(a) for k, a in init.items()}
    t.reset_states_dev(d["root_states"], d["dof_pos"], d["dof_vel"], mask=None if mask is None else guarded(mask.astype(np.int32)),
                       env_ids=None if env_ids is None else guarded(np.asarray(env_ids, np.int32)), n=n, delay_steps=d.get("delay_steps"),
                       episode_steps=d.get("episode_steps"), chain=chain, **extra)
    return {k: fetch(d[k], sim[k]) for k in sim}, d


def same64(a, b, what):
    """the same float64 bits; a NaN matches a NaN at the same position whatever its payload"""
    assert a.dtype == b.dtype == D and a.shape == b.shape, what
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes(), what


def check_reset(got, want, halves, what):
    """bit for bit except the two yaw components of the environments that drew one, which stay within the bound of float64"""
    for k in ("dof_pos", "dof_vel", "delay_steps", "episode_steps"):
        if k in got:
            same(got[k], want[k], (what, k))
    cols = [0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12]
    same(np.ascontiguousarray(got["root_states"][:, cols]), np.ascontiguousarray(want["root_states"][:, cols]), (what, "root_states"))
    drew = np.zeros(len(got["root_states"]), bool)
    for e, half in halves.items():
        drew[e] = True
        s64, c64 = em.yaw64(half)
        dev = max(abs(D(got["root_states"][e, 5]) - s64), abs(D(got["root_states"][e, 6]) - c64))
        WORST["yaw"] = max(WORST["yaw"], float(dev))
        assert dev <= YAW_BOUND, (what, e, dev)
    same(got["root_states"][~drew][:, 5:7], want["root_states"][~drew][:, 5:7], (what, "rows without a yaw draw"))


# ---- 1. reset states -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,r", SHAPES)
def test_a_masked_reset_and_a_list_with_bad_ids_are_the_mirrors_rows(hip, world, n, r):
    rng = np.random.default_rng(100 + n + r)
    t, m = reset_setup(world, rng, n, r)
    before = t.state()
    sim = sim_arrays(rng, n, r)
    mask = rng.uniform(size=n) < (0.15 if n > 100 else 0.5)
    mask[0] = True
    want = {k: a.copy() for k, a in sim.items()}
    dropped, halves = m.reset(want["root_states"], want["dof_pos"], want["dof_vel"], mask=mask, delay_steps=want["delay_steps"],
                              episode_steps=want["episode_steps"])
    got, d = reset_dev(t, sim, mask=mask)
    assert dropped == 0 and t.state()["ignored"] == before["ignored"]
    check_reset(got, want, halves, "mask")
    for k in sim:                                                     # unmasked rows keep their bytes
        assert got[k][~mask].tobytes() == sim[k][~mask].tobytes(), k
    assert (got["episode_steps"][mask] == 0).all() and (got["delay_steps"][mask] < 7).all() and (got["delay_steps"][mask] >= 0).all()
    same(t.reset_state()["reset_draws"], m.reset_draws, "reset_draws")
    # z is the base height plus what terrain_heights_dev returns at the drawn point, bit for bit
    d_h = guarded(np.zeros(n, F))
    t.terrain_heights_dev(d["root_states"], n, d_h, stride=13)
    hip.check(hip.lib().gmr_stream_sync(None))
    h = fetch(d_h, np.zeros(n, F))
    same(got["root_states"][mask, 2], (F(0.72) + h[mask]).astype(F), "z")
    assert len(np.unique(h[mask])) > min(3, mask.sum() - 1)
    # a list: out-of-range ids dropped and counted, a masked-out bad id not counted, the second reset of an environment draws anew
    if n >= 8:
        ids = np.array([n - 1, 3, n, -1, 5, 2 ** 30, 0, n + 7], np.int32)
        lmask = np.array([1, 1, 1, 1, 1, 1, 5, 0], np.int32)
        sim2 = {k: a.copy() for k, a in got.items()}
        want2 = {k: a.copy() for k, a in want.items()}
        want2["root_states"][:, 5:7] = got["root_states"][:, 5:7]       # (the device's own yaw components of the first reset)
        dropped, halves = m.reset(want2["root_states"], want2["dof_pos"], want2["dof_vel"], mask=lmask, env_ids=ids, delay_steps=want2["delay_steps"],
                                  episode_steps=want2["episode_steps"])
        got2, _ = reset_dev(t, sim2, mask=lmask, env_ids=ids)
        assert dropped == 3 and t.state()["ignored"] == before["ignored"] + 3
        check_reset(got2, want2, halves, "list")
        same(t.reset_state()["reset_draws"], m.reset_draws, "reset_draws after the list")
        assert (got2["dof_pos"][0] != got["dof_pos"][0]).any() or not mask[0]
    after = t.state()
    for k in STATE:
        same(before[k], after[k], k)
    print(f"N = {n}, R = {r}: yaw components, largest deviation from float64 {WORST['yaw']:.3e} (bound {YAW_BOUND})")


def test_the_draws_of_an_environment_do_not_depend_on_how_many_there_are(hip, world):
    rows = {}
    for n in (37, 5000):
        rng = np.random.default_rng(7)
        t = tracker(world["lib"], n, DT, world["map"], np.zeros(23, F), seed=99)
        base, pose = np.arange(13, dtype=F), np.linspace(-1, 1, 23).astype(F)
        t.set_reset_states(base, pose, decimation=5, use_terrain=False, **UNI)
        sim = sim_arrays(rng, n, 23)
        mask = np.zeros(n, bool)
        mask[:37] = True
        rows[n], _ = reset_dev(t, sim, mask=mask)
    for k in rows[37]:
        assert rows[37][k].tobytes() == rows[5000][k][:37].tobytes(), k


def test_a_chained_reset_is_the_three_separate_calls(hip, world):
    n, r = 37, 23
    out = []
    for chain in (False, True):
        rng = np.random.default_rng(31)
        t, _ = reset_setup(world, rng, n, r, control=True, proprio=True)
        sim = sim_arrays(rng, n, r)
        mask = rng.uniform(size=n) < 0.5
        # state that is not zero before the reset
        t.hold(rng.normal(0, 1, (n, r)).astype(F))
        t.proprio_reset(rng.normal(0, 1, (n, 13)).astype(F))
        d = {k: guarded(a) for k, a in sim.items()}
        d_mask = guarded(mask.astype(np.int32))
        t.reset_states_dev(d["root_states"], d["dof_pos"], d["dof_vel"], mask=d_mask, delay_steps=d["delay_steps"], episode_steps=d["episode_steps"],
                           chain=chain)
        if not chain:
            mid = (t.control_state(), t.proprio_state())
            t.hold_dev(d["dof_pos"], mask=d_mask)
            t.proprio_reset_dev(d["root_states"], mask=d_mask)
        hip.check(hip.lib().gmr_stream_sync(None))
        out.append(({k: fetch(d[k], sim[k]) for k in sim}, t.control_state(), t.proprio_state(), mask))
    (sim_a, ctl_a, pro_a, mask), (sim_b, ctl_b, pro_b, _) = out
    for k in sim_a:
        assert sim_a[k].tobytes() == sim_b[k].tobytes(), k
    for a, b in ((ctl_a, ctl_b), (pro_a, pro_b)):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    # and the unchained reset had left both states alone
    assert (mid[0]["held"][mask] != ctl_a["held"][mask]).any() and (mid[1]["last_root_vel"][mask] != pro_a["last_root_vel"][mask]).any()
    assert ctl_a["held"][mask].tobytes() == sim_a["dof_pos"][mask].tobytes() and not pro_a["filtered_lin_vel"][mask].any()
    assert pro_a["last_root_vel"][mask].tobytes() == sim_a["root_states"][mask, 7:13].tobytes()


def test_per_entry_init_rows_and_a_block_without_a_spec(hip, world):
    """a list with init_* rows by list position, no yaw range (the given quaternion stays), no dof spec (no draw: the given row as it is), the
    plane; then the synchronous twin gives the same bytes"""
    n, r = 37, 5
    rng = np.random.default_rng(41)
    kw = dict(init_dof_pos=None, yaw_range=None, terrain=False)
    t, m = reset_setup(world, rng, n, r, **kw)
    rng2 = np.random.default_rng(41)
    twin, _ = reset_setup(world, rng2, n, r, **kw)
    sim = sim_arrays(rng, n, r)
    ids = np.array([36, 4, 17, 0, 9], np.int32)
    init = {"init_root_states": rng.normal(0, 1, (5, 13)).astype(F), "init_dof_pos": rng.normal(0, 1, (5, r)).astype(F),
            "init_dof_vel": rng.normal(0, 1, (5, r)).astype(F)}
    want = {k: a.copy() for k, a in sim.items()}
    _, halves = m.reset(want["root_states"], want["dof_pos"], want["dof_vel"], env_ids=ids, delay_steps=want["delay_steps"],
                        episode_steps=want["episode_steps"], **init)
    assert not halves
    got, _ = reset_dev(t, sim, env_ids=ids, **init)
    for k in sim:
        same(got[k], want[k], k)
    same(got["dof_pos"][ids], init["init_dof_pos"], "the given dof rows, undrawn")
    same(got["dof_vel"][ids], init["init_dof_vel"], "the given dof velocities")
    same(np.ascontiguousarray(got["root_states"][ids][:, 3:7]), np.ascontiguousarray(init["init_root_states"][:, 3:7]), "the given quaternions")
    same(np.ascontiguousarray(got["root_states"][ids][:, 9:13]), np.ascontiguousarray(init["init_root_states"][:, 9:13]), "the given velocities")
    assert (got["root_states"][ids, 7:9] != init["init_root_states"][:, 7:9]).all()          # randomised
    sync = twin.reset_states(sim["root_states"], sim["dof_pos"], sim["dof_vel"], env_ids=ids, delay_steps=sim["delay_steps"],
                             episode_steps=sim["episode_steps"], **init)
    assert sync.pop("ignored") == 0
    for k in sim:
        assert sync[k].tobytes() == got[k].tobytes(), k
    same(twin.reset_state()["reset_draws"], t.reset_state()["reset_draws"], "reset_draws")


# ---- 2. the reward and the statistics ----------------------------------------------------------------------------------------------------
def reward_setup(world, rng, n, only_positive=(True, False), stats=True, seed=5):
    """a tracker with control, proprio, feet and commands set and three caller columns, and the reward mirror"""
    r = 23
    t = tracker(world["lib"], n, DT, world["map"], rng.uniform(-0.4, 0.4, r).astype(F), seed=seed)
    t.reset()
    t.set_terms(weights=TERM_WEIGHTS)
    t.set_control(rng.uniform(-0.6, 0.6, r).astype(F), 0.25, 0.75, 2.0, 0.1, 0.2, decimation=4)
    set_proprio(t, rng, r)
    t.set_feet(FEET, edges_of(4), NB, termination_bodies=TERMINATION, penalized_bodies=PENALIZED, feet_distance_ref=0.2, swing_period=0.2, scales=FEET_SCALES)
    t.set_commands(**RANGES, **PLAIN)
    from general_motion_retargeting_amd import motion_tracker as mt
    weights = {"terms": np.array(TERM_WEIGHTS, F), "proprio": np.array([PROPRIO_SCALES.get(k, 0.0) for k in mt.PROPRIO_TERMS], F),
               "feet": np.array([FEET_SCALES.get(k, 0.0) for k in mt.FEET_TERMS], F), "commands": np.array([PLAIN["scales"].get(k, 0.0) for k in mt.CMD_TERMS], F)}
    extra_w = (0.5, 0.0, -1.5)
    kw = dict(group_weight=(0.1, 1.0), only_positive=only_positive, stats=stats)
    layout = t.set_rewards(extra_names=("smooth", "unused", "energy"), extra_weights=extra_w, groups={"dof_pos": 3, "root_pos": 3, "energy": 2, "survival": 0}, **kw)
    C = layout["num_cols"]
    assert C == 6 + 14 + 8 + 4 + 3 and layout["names"][-3:] == ("smooth", "unused", "energy") and layout["blocks"]["feet"] == (20, 8)
    groups = list(layout["groups"])
    assert groups[:6] == [3, 2, 2, 2, 3, 2] and groups[-1] == 2 and groups[28] == 0
    m = em.Rewards(em.reward_config(list(weights), weights, extra_w, groups=groups, **kw), n)
    return t, m, weights


def scripted_terms(rng, n, s):
    x = {"terms": rng.uniform(0, 1, (n, 6)).astype(F), "proprio": rng.uniform(0, 3, (n, 14)).astype(F), "feet": rng.uniform(0, 2, (n, 8)).astype(F),
         "commands": rng.uniform(0, 1, (n, 4)).astype(F), "extra": rng.normal(0, 1, (n, 3)).astype(F)}
    if s % 5 == 3:
        x["feet"] = None                                   # an absent block: its columns stay out
    if s % 7 == 4:
        x["extra"] = None
    if s % 4 == 1:
        x["proprio"][s % n, 4] = np.nan                    # dof_vel: weight zero, the NaN stays out
        x["terms"][(s + 1) % n, 4] = np.nan                # dof_pos, in both groups: the NaN stays, clip or no clip
    return x


NAMES = {"terms": "term", "proprio": "proprio_term", "feet": "feet_term", "commands": "cmd_term", "extra": "extra"}
OUTS = {"reward": (1, F), "scaled": (35, F), "group_total": (2, F), "reset": (1, np.int32), "time_outs": (1, np.int32)}


def rewards_dev(t, x, done, flags, n):
    up = {NAMES[k]: guarded(a) for k, a in x.items() if a is not None}
    like = {k: np.zeros((n, w) if w > 1 else n, dt) for k, (w, dt) in OUTS.items()}
    out = {k: guarded(np.full(a.shape, SENTINEL if a.dtype == F else ISENT, a.dtype)) for k, a in like.items()}
    t.rewards_dev(**up, done=None if done is None else guarded(done), flags=None if flags is None else guarded(flags), **out)
    return {k: fetch(out[k], like[k]) for k in out}


def check_stats(hip, t, m, clear):
    C = m.cfg["C"]
    d_out = guarded(np.zeros(C + 3, np.uint64))
    t.reward_stats_dev(d_out, clear=clear)
    hip.check(hip.lib().gmr_stream_sync(None))
    raw = fetch(d_out, np.zeros(C + 3, np.uint64))
    episodes, steps, sums = m.stats(clear=clear)
    assert (int(raw[0]), int(raw[1])) == (episodes, steps)
    same64(raw[2:].view(D), sums, "fin_sum")
    return episodes


@pytest.mark.parametrize("n,steps,only_positive", [(37, 40, (True, False)), (37, 12, (False, True)), (1, 10, (True, False)), (5000, 4, (True, False))])
def test_scripted_steps_are_the_mirrors_reward_and_statistics(hip, world, n, steps, only_positive):
    rng = np.random.default_rng(200 + n + steps)
    t, m, _ = reward_setup(world, rng, n, only_positive)
    before = {"state": t.state(), "control": t.control_state(), "proprio": t.proprio_state(), "feet": t.feet_state(), "commands": t.command_state()}
    seen = {"clipped": 0, "nan": 0, "episodes": 0, "time_outs": 0}
    for s in range(steps):
        x = scripted_terms(rng, n, s)
        done = (rng.uniform(size=n) < 0.1).astype(np.int32) * rng.integers(1, 16, n).astype(np.int32)
        if s == 0:
            done[0] = 2                                      # the very first call: an episode of zero steps
        if s == 2:
            done[:] = rng.integers(1, 16, n)                 # everybody in one call
        flags = rng.integers(0, 8, n).astype(np.int32)
        dn, fl = (None, None) if s % 6 == 5 else (done, flags)
        got = rewards_dev(t, x, dn, fl, n)
        want = m.step(x, dn, fl)
        for k in OUTS:
            same(got[k], want[k], (s, k))
        st = t.reward_state()
        same(st["ep_steps"], m.ep_steps, (s, "ep_steps"))
        same(st["ep_sum"], m.ep_sum, (s, "ep_sum"))
        seen["clipped"] += sum(int((want["group_total"][:, g] == 0).sum()) for g in (0, 1) if only_positive[g])
        seen["nan"] += int(np.isnan(want["reward"]).sum())
        seen["time_outs"] += int(want["time_outs"].sum())
        if s % 3 == 2 or s == steps - 1:
            seen["episodes"] += check_stats(hip, t, m, clear=s % 2 == 0)
    assert seen["nan"] > 0 and seen["time_outs"] > 0 and seen["episodes"] >= n
    if n >= 37 and only_positive[0]:
        assert seen["clipped"] > 0
    check_stats(hip, t, m, clear=True)
    assert check_stats(hip, t, m, clear=False) == 0           # clear leaves zeros
    raw = t.reward_stats(raw=True)
    assert raw["episodes"] == 0 and raw["steps"] == 0 and not raw["sums"].any() and raw["sums"].tobytes() == bytes(8 * 36)
    z = t.reward_stats()
    assert z["episodes"] == 0 and z["steps"] == 0.0 and z["reward"] == 0.0 and z["energy"] == 0.0
    # a reward call touches no other state of the tracker
    after = {"state": t.state(), "control": t.control_state(), "proprio": t.proprio_state(), "feet": t.feet_state(), "commands": t.command_state()}
    for part in before:
        for k in before[part]:
            if isinstance(before[part][k], np.ndarray):
                same(before[part][k], after[part][k], (part, k))
            else:
                assert before[part][k] == after[part][k], (part, k)


def test_two_runs_and_the_synchronous_twin_give_the_same_bytes(hip, world):
    """N = 5 000 (313 workgroups), every environment done in the second call: two device runs and a run through the host twins"""
    n = 5000
    runs = []
    for mode in ("dev", "dev", "host"):
        rng = np.random.default_rng(77)
        t, m, _ = reward_setup(world, rng, n)
        outs = []
        for s in range(3):
            x = scripted_terms(rng, n, 4 * s)                  # (no NaN here: the means are compared as numbers)
            done = np.full(n, 1, np.int32) if s == 1 else (rng.uniform(size=n) < 0.002).astype(np.int32)
            if mode == "dev":
                outs.append(rewards_dev(t, x, done, None, n))
            else:
                outs.append(t.rewards(**{NAMES[k]: a for k, a in x.items() if a is not None}, done=done))
            m.step(x, done)
        stats = t.reward_stats(clear=False, raw=True)
        runs.append((outs, stats, t.reward_state()))
        assert stats["episodes"] == m.fin_count >= n and stats["steps"] == m.fin_steps
        same64(stats["sums"], m.fin_sum, "fin_sum")
        means = t.reward_stats()
        assert means["episodes"] == stats["episodes"] and means["steps"] == stats["steps"] / stats["episodes"]
        assert means["reward"] == float(stats["sums"][0]) / stats["episodes"] and means["energy"] == float(stats["sums"][-1]) / stats["episodes"]
    for outs, stats, state in runs[1:]:
        for a, b in zip(outs, runs[0][0]):
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), k
        assert stats["sums"].tobytes() == runs[0][1]["sums"].tobytes() and (stats["episodes"], stats["steps"]) == (runs[0][1]["episodes"], runs[0][1]["steps"])
        for k in state:
            assert state[k].tobytes() == runs[0][2][k].tobytes(), k


def test_the_weights_are_read_when_the_call_is_enqueued_and_the_library_checks_the_blocks(hip, world):
    n = 37
    rng = np.random.default_rng(9)
    t, m, weights = reward_setup(world, rng, n, stats=False)
    x = scripted_terms(rng, n, 0)
    same(rewards_dev(t, x, None, None, n)["reward"], m.step(x)["reward"], "before")
    t.set_terms(weights=(0.0, 3.0, 0.0, 0.0, 1.0, 1.0))
    weights["terms"] = np.array((0.0, 3.0, 0.0, 0.0, 1.0, 1.0), F)
    m2 = em.Rewards(em.reward_config(list(weights), weights, (0.5, 0.0, -1.5), groups=list(m.cfg["groups"]), group_weight=(0.1, 1.0),
                                     only_positive=(True, False)), n)
    got, want = rewards_dev(t, x, None, None, n), m2.step(x)
    for k in ("reward", "scaled", "group_total"):
        same(got[k], want[k], k)
    assert t.reward_state() is None
    with pytest.raises(ValueError, match="statistics are off"):
        t.reward_stats()
    # the library checks the blocks again when the Python layer names others than the handle has
    t._commands = None
    with pytest.raises(hip.GmrHipError, match="configured on this tracker"):
        t.set_rewards()
