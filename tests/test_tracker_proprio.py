"""The tracker's proprioception half on a real MI355X (csrc/gmr_tracker_proprio.hip through motion_tracker.py): every
output and the six state arrays are the float32 statement of tests/proprio_mirror.py bit for bit -- noise off, absent inputs, the
termination thresholds, uniform noise, resets, edge shapes, a stream of the caller's --, the gaussian draw against the float64 evaluation
of the same Philox words, and the moments of 94 208 draws.  N = 37 environments (no multiple of 16 or 64) on the four-clip library of
test_tracker_control.py with R = 23 and C = 5 pass-through columns (W = 80), 64 guard floats behind every device output; every test makes
one pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proprio_mirror as pm  # noqa: E402
from test_motion_tracker import STATE, tracker  # noqa: E402
from test_tracker_control import G, NDOF, SENTINEL, hip, same, world  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32
N, R, CX, DT = 37, 23, 5, 0.02
OUTPUTS = ("base_lin_vel", "base_ang_vel", "projected_gravity", "filtered_lin_vel", "filtered_ang_vel", "obs", "priv", "term", "total", "done")
STATE6 = ("filtered_lin_vel", "filtered_ang_vel", "last_root_vel", "last_actions", "last_dof_vel", "noise_tick")
SCALES = {"lin_vel_z": -2.0, "ang_vel_xy": -0.2, "orientation": -5.0, "torques": -2e-4, "dof_acc": -1e-7, "root_acc": -1e-4, "action_rate": -1.0,
          "dof_pos_limits": -1.0, "torque_tiredness": -1e-2, "power": -2e-3, "base_height": -20.0}          # dof_vel and the two *_limits: zero
UNIFORM = {k: {"distribution": "uniform", "operation": op, "range": rng} for k, op, rng in
           (("gravity", "additive", (-0.05, 0.05)), ("ang_vel", "additive", (-0.1, 0.3)), ("dof_pos", "additive", (-0.01, 0.01)),
            ("dof_vel", "scaling", (0.9, 1.15)), ("lin_vel", "scaling", (0.8, 1.2)), ("height", "additive", (-0.02, 0.02)))}
# ang_vel has no spec: its columns must be the clean row's
GAUSSIAN = {k: {"distribution": "gaussian", "operation": op, "range": rng} for k, op, rng in
            (("gravity", "additive", (0.0, 0.05)), ("dof_pos", "additive", (0.01, 0.1)), ("dof_vel", "additive", (0.0, 1.5)),
             ("lin_vel", "additive", (0.0, 0.2)), ("height", "additive", (0.0, 0.05)))}
# The gaussian draw against the float64 evaluation of the same words, in units of s b max(1, |z|) (s: the block's scale, b: its deviation).
# No ulp figures of logf / cosf ship with the ROCm on the test machines, so the bound is four times the largest deviation met on an
# MI355X: a different ROCm may round a few ulp differently.
GAUSSIAN_MEASURED = 1.598e-6
GAUSSIAN_BOUND = 4 * GAUSSIAN_MEASURED


def setup(world, rng, n=N, dmap=None, extra_cols=CX, noise=None, seed=3, scales=SCALES, norm_dof_vel=0.1):
    """a tracker on the world's library with proprio set, and its mirror"""
    dmap = world["map"] if dmap is None else dmap
    r = len(dmap)
    t = tracker(world["lib"], n, DT, dmap, rng.uniform(-0.4, 0.4, r).astype(F), seed=seed)
    t.reset()                                             # clips, clocks and draw counters that are not zero
    pose = rng.uniform(-0.6, 0.6, r).astype(F)
    lim = np.sort(rng.uniform(-2.0, 2.0, (r, 2)), axis=1).astype(F)
    lim[:, 1] += F(0.5)
    vlim, tlim = rng.uniform(3, 12, r).astype(F), rng.uniform(10, 60, r).astype(F)
    kw = dict(base_height_target=0.68, terminate_vel=50.0, terminate_height=0.3, max_episode_steps=30, extra_cols=extra_cols, filter_weight=0.1,
              normalization={"dof_vel": norm_dof_vel, "lin_vel": 2.0, "ang_vel": 0.25}, noise=noise, soft_dof_pos_limit=0.9, soft_dof_vel_limit=0.8,
              soft_torque_limit=0.85, scales=scales)
    t.set_proprio(pose, lim, vlim, tlim, **kw)
    return t, pm.Proprio(pm.config(pose, lim, vlim, tlim, **kw), n, r, DT, seed)


def inputs(rng, n=N, r=R, c=CX, nasty=False):
    quat = rng.standard_normal((n, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    root = np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.uniform(0.2, 0.9, (n, 1)), quat, rng.normal(0, 1.5, (n, 3)), rng.normal(0, 2.0, (n, 3))], axis=1).astype(F)
    x = {"root_states": root, "dof_pos": rng.uniform(-2.2, 2.7, (n, r)).astype(F), "dof_vel": rng.normal(0, 6.0, (n, r)).astype(F),
         "actions": np.clip(rng.normal(0, 0.8, (n, r)), -1, 1).astype(F), "mean_torques": rng.normal(0, 25.0, (n, r)).astype(F),
         "extra": rng.uniform(-1, 1, (n, c)).astype(F) if c else None, "ground": rng.uniform(-0.1, 0.3, n).astype(F),
         "episode_steps": rng.integers(25, 36, n).astype(np.int32)}
    if nasty:
        x["root_states"][1 % n, 3:7] *= F(1.3)                  # not a unit quaternion: used as given
        x["root_states"][2 % n, 3:7] = 0                        # a zero quaternion
        for k, at in (("dof_vel", 1), ("actions", 4)):
            flat = x[k].reshape(-1)
            flat[at % flat.size], flat[(at + 6) % flat.size], flat[-1] = np.nan, np.inf, -np.inf
    return x


def run_dev(hip, t, x, noise, stream=None, want=OUTPUTS):
    """proprio_dev into guarded buffers -> the outputs on the host, the guard floats checked"""
    n = t.num_envs
    _, counts = t._proprio_counts()
    up = {k: None if a is None else hip.DeviceBuffer.from_host(a) for k, a in x.items()}
    out = {k: hip.DeviceBuffer.from_host(np.full(n * counts[k] + G, SENTINEL, dtype=F)) for k in want}
    t.proprio_dev(**up, noise=noise, stream=stream, **out)
    hip.check(hip.lib().gmr_stream_sync(None if stream is None else stream.ptr))
    got = {}
    for k, b in out.items():
        raw = b.to_host(n * counts[k] + G, F)
        assert (raw[n * counts[k]:] == SENTINEL).all(), k                  # the guard floats
        a = raw[:n * counts[k]]
        got[k] = a.view(np.int32).copy() if k == "done" else (a.copy() if k == "total" else a.reshape(n, counts[k]).copy())
    return got


def check(got, want, state, mirror, what):
    for k in got:
        same(got[k], want[k], (what, k))
    ms = mirror.state()
    for k in STATE6:
        same(state[k], ms[k], (what, k))


# ---- 1. noise off ----------------------------------------------------------------------------------------------------------------------
def test_five_steps_without_noise_are_the_mirrors_bits(hip, world):
    rng = np.random.default_rng(61)
    t, m = setup(world, rng, noise=UNIFORM)                   # specs in place, the launches ask for none
    before = t.state()
    assert (before["draws"] > 0).all()
    seen = set()
    for s in range(5):
        x = inputs(rng, nasty=True)
        got = run_dev(hip, t, x, noise=False)
        want = m.step(**x, noise=False)
        check(got, want, t.proprio_state(), m, s)
        seen |= set(got["done"].tolist())
        assert np.isnan(got["term"]).any() and np.isinf(got["term"]).any() and np.isfinite(got["obs"][2]).sum() >= 3 * R
    assert len(seen) >= 4 and not t.proprio_state()["noise_tick"].any()
    after = t.state()
    for k in STATE:
        same(before[k], after[k], k)
    assert before["ignored"] == after["ignored"]
    lay = t.proprio_layout()
    assert lay["width"] == 6 + CX + 3 * R == got["obs"].shape[1] and lay["obs"]["actions"] == (6 + CX + 2 * R, 6 + CX + 3 * R)
    assert np.array_equal(got["obs"][:, 6:6 + CX], x["extra"])


# ---- 2. absent inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actions,torques", [(False, False), (True, False), (False, True)])
def test_absent_inputs_zero_their_terms_and_leave_last_actions(hip, world, actions, torques):
    rng = np.random.default_rng(62)
    t, m = setup(world, rng)
    first = inputs(rng)
    t.proprio(**first, noise=False)
    m.step(**first, noise=False)                              # last_actions is not zero from here on
    x = inputs(rng)
    if not actions:
        x["actions"] = None
    if not torques:
        x["mean_torques"] = None
    x["ground"] = x["episode_steps"] = None
    got = t.proprio(**x, noise=False)
    want = m.step(**x, noise=False)
    st = t.proprio_state()
    check(got, want, st, m, "absent")
    gone = ([] if actions else [7]) + ([] if torques else [3, 10, 11, 12])
    here = [k for k in range(14) if k not in gone]
    assert not got["term"][:, gone].any() and (got["term"][:, here] != 0).any(axis=0).all()
    sc = m.cfg["scale"]
    total = np.zeros(N, F)
    for k in here:
        if sc[k] != 0:
            total = total + sc[k] * got["term"][:, k]
    same(got["total"], total, "total without the absent terms")
    if not actions:
        assert np.array_equal(st["last_actions"], first["actions"]) and not got["obs"][:, -R:].any()
    else:
        assert np.array_equal(st["last_actions"], x["actions"]) and np.array_equal(got["obs"][:, -R:], x["actions"])
    assert not (got["done"] & 4).any()                        # no episode_steps: no time-out


# ---- 3. the termination bits -----------------------------------------------------------------------------------------------------------
def test_done_bits_at_just_under_and_just_over_each_threshold(hip, world):
    rng = np.random.default_rng(63)
    t, m = setup(world, rng)
    x = inputs(rng)
    rs = x["root_states"]
    rs[:, 7:13] = 0
    rs[:, 2] = 0.6
    x["ground"] = None
    x["episode_steps"][:] = 3
    five, th = F(5.0), F(0.3)
    rs[0, 7:9] = five                                          # 25 + 25 = 50 exactly: not above
    rs[1, 7], rs[1, 8] = np.nextafter(five, F(9)), five        # just over
    rs[2, 7], rs[2, 8] = np.nextafter(five, F(0)), five        # just under
    rs[3, 12] = np.nan                                         # a NaN compares false
    rs[4, 2], rs[5, 2], rs[6, 2], rs[7, 2] = th, np.nextafter(th, F(0)), np.nextafter(th, F(1)), np.nan
    x["episode_steps"][8:12] = [30, 31, 29, 2 ** 31 - 1]
    rs[12, 7:9], rs[12, 2], x["episode_steps"][12] = F(6.0), F(0.1), 40
    got = run_dev(hip, t, x, noise=False)
    want = m.step(**x, noise=False)
    check(got, want, t.proprio_state(), m, "done")
    expect = np.zeros(N, np.int32)
    expect[[1, 5, 9, 11, 12]] = [1, 2, 4, 4, 7]
    assert np.array_equal(got["done"], expect)
    # the output is a mask reset_done takes as it lies
    d_done = hip.DeviceBuffer.from_host(got["done"])
    before = t.state()
    t.reset_done_dev(done=d_done)
    hip.check(hip.lib().gmr_stream_sync(None))
    after = t.state()
    assert np.array_equal(after["draws"] != before["draws"], expect != 0)


# ---- 4. uniform noise ------------------------------------------------------------------------------------------------------------------
def test_uniform_noise_is_the_mirrors_and_does_not_depend_on_the_launch_shape(hip, world):
    rng = np.random.default_rng(64)
    t, m = setup(world, rng, noise=UNIFORM, seed=0x1234567887654321)
    x = inputs(rng)
    clean = run_dev(hip, t, x, noise=False, want=("obs", "priv"))
    m.step(**x, noise=False)
    for s in range(2):
        got = run_dev(hip, t, x, noise=True)
        want = m.step(**x, noise=True)
        st = t.proprio_state()
        check(got, want, st, m, ("uniform", s))
        assert (st["noise_tick"] == s + 1).all()
    lay = t.proprio_layout()["obs"]
    plain = np.r_[lay["extra"][0]:lay["extra"][1], lay["actions"][0]:lay["actions"][1]]
    diff = got["obs"] != clean["obs"]
    assert np.array_equal(got["obs"][:, plain], clean["obs"][:, plain]) and np.delete(diff, plain, axis=1).mean() > 0.99
    assert (got["priv"] != clean["priv"]).mean() > 0.99
    # the same seed on 64 environments: the first 37 rows are the same draws; another seed: others
    wide = {k: None if a is None else np.concatenate([a, a[:64 - N]]) for k, a in x.items()}
    for seed, equal in ((0x1234567887654321, True), (0x1234567887654320, False)):
        t2, _ = setup(world, np.random.default_rng(64), n=64, noise=UNIFORM, seed=seed)
        g2 = run_dev(hip, t2, wide, noise=True, want=("obs", "priv"))
        g2 = run_dev(hip, t2, wide, noise=True, want=("obs", "priv"))          # tick 1, as got
        assert np.array_equal(g2["obs"][:N], got["obs"]) == equal and np.array_equal(g2["priv"][:N], got["priv"]) == equal
        assert not np.array_equal(g2["obs"][N:, :6], g2["obs"][:64 - N, :6])          # the same inputs in other environments: other draws


# ---- 5. gaussian noise -----------------------------------------------------------------------------------------------------------------
def test_gaussian_noise_against_the_float64_evaluation_of_the_same_words(hip, world):
    """Largest deviation met on an MI355X: see GAUSSIAN_MEASURED and DESIGN.md section 6q."""
    rng = np.random.default_rng(65)
    t, m = setup(world, rng, noise=GAUSSIAN, seed=77)
    x = inputs(rng)
    clean = run_dev(hip, t, x, noise=False, want=("obs", "priv"))
    mc = m.step(**x, noise=False)
    same(clean["obs"], mc["obs"], "clean obs")
    got = run_dev(hip, t, x, noise=True)
    want = m.step(**x, noise=True, wide=True)
    st = t.proprio_state()
    assert (st["noise_tick"] == 1).all()
    for k in STATE6:
        same(st[k], m.state()[k], k)
    for k in ("base_lin_vel", "base_ang_vel", "projected_gravity", "filtered_lin_vel", "filtered_ang_vel", "term", "total", "done"):
        same(got[k], want[k], k)                                            # nothing but obs and priv sees the noise
    lay = t.proprio_layout()["obs"]
    W = t.proprio_layout()["width"]
    row = np.concatenate([got["obs"], got["priv"]], axis=1).astype(np.float64)
    base = np.concatenate([clean["obs"], clean["priv"]], axis=1).astype(np.float64)
    z = want["z64"]
    nm = m.cfg["norm"]
    worst, drawn = 0.0, np.zeros(W + 4, bool)
    for block, (c0, c1), s in (("gravity", lay["gravity"], nm["gravity"]), ("dof_pos", lay["dof_pos"], nm["dof_pos"]), ("dof_vel", lay["dof_vel"], nm["dof_vel"]),
                               ("lin_vel", (W, W + 3), nm["lin_vel"]), ("height", (W + 3, W + 4), F(1))):
        spec = m.cfg["noise"][block]
        a, b, s = float(spec["a"]), float(spec["m"]), float(s)
        delta64 = (a + b * z[:, c0:c1]) * s                                 # additive: obs - clean
        dev = np.abs((row[:, c0:c1] - base[:, c0:c1]) - delta64) / (s * b * np.maximum(1.0, np.abs(z[:, c0:c1])))
        worst = max(worst, float(dev.max()))
        drawn[c0:c1] = True
    print(f"gaussian draws: largest deviation from float64 {worst:.3e} of s b max(1, |z|) (measured {GAUSSIAN_MEASURED}, bound {GAUSSIAN_BOUND})")
    assert np.array_equal(row[:, ~drawn], base[:, ~drawn]) and (~drawn).sum() == 3 + CX + R          # ang_vel, extra, actions
    assert not z[:, ~drawn].any() and np.abs(z[:, drawn]).max() > 3.0
    assert GAUSSIAN_BOUND is not None and worst <= GAUSSIAN_BOUND


# ---- 6. moments ------------------------------------------------------------------------------------------------------------------------
def test_the_moments_of_a_standard_gaussian_on_dof_vel(hip, world):
    n = 4096
    rng = np.random.default_rng(66)
    spec = {"dof_vel": {"distribution": "gaussian", "operation": "additive", "range": (0.0, 1.0)}}
    t, _ = setup(world, rng, n=n, noise=spec, seed=2025, norm_dof_vel=1.0)
    x = {"root_states": np.zeros((n, 13), F), "dof_pos": np.zeros((n, R), F), "dof_vel": np.zeros((n, R), F), "extra": np.zeros((n, CX), F)}
    got = run_dev(hip, t, x, noise=True, want=("obs",))
    c0, c1 = t.proprio_layout()["obs"]["dof_vel"]
    z = got["obs"][:, c0:c1].astype(np.float64).reshape(-1)
    k = z.size
    assert k == n * R and not got["obs"][:, c1:].any()
    print(f"moments of {k} draws: mean {z.mean():.3e}, variance {z.var():.5f}, largest |z| {np.abs(z).max():.3f}")
    assert abs(z.mean()) <= 5 / np.sqrt(k)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / k)
    assert np.abs(z).max() <= 5.77                                          # sqrt(-2 ln 2^-24)
    assert len(np.unique(z)) > 0.99 * k


# ---- 7. resets -------------------------------------------------------------------------------------------------------------------------
def test_a_masked_reset_with_ids_outside_then_a_step(hip, world):
    rng = np.random.default_rng(67)
    t, m = setup(world, rng, noise=UNIFORM)
    for _ in range(2):
        x = inputs(rng)
        t.proprio(**x, noise=True)
        m.step(**x, noise=True)
    before = t.state()
    ids = np.array([5, N, 9, -3, 0, 2 ** 31 - 1, 30, N - 1], np.int32)
    mask = np.array([1, 1, 0, 1, 1, 0, 1, 1], np.int32)
    rows = rng.normal(0, 1, (len(ids), 13)).astype(F)
    assert t.proprio_reset(rows, mask, ids) == 2 == m.reset(rows, mask, ids)
    after = t.state()
    assert after["ignored"] == before["ignored"] + 2
    for k in STATE:
        same(before[k], after[k], k)
    st = t.proprio_state()
    for k in STATE6:
        same(st[k], m.state()[k], k)
    assert not st["filtered_lin_vel"][[5, 0, 30, N - 1]].any() and st["filtered_ang_vel"][9].any() and np.array_equal(st["last_root_vel"][30], rows[6, 7:13])
    assert st["last_actions"][5].any() and (st["noise_tick"] == 2).all()          # the reset leaves them
    x = inputs(rng)
    got = t.proprio(**x, noise=True)
    check(got, m.step(**x, noise=True), t.proprio_state(), m, "after the reset")
    # every environment by its done flags
    done = rng.uniform(size=N) < 0.5
    rows = rng.normal(0, 1, (N, 13)).astype(F)
    assert t.proprio_reset(rows, done) == 0 == m.reset(rows, done)
    st = t.proprio_state()
    for k in STATE6:
        same(st[k], m.state()[k], k)


# ---- 8. edge shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,r,c", [(N, 1, CX), (N, 64, 16), (1, R, CX), (N, R, 0)])
def test_one_dof_sixty_four_dofs_one_environment_and_no_extra_columns(hip, world, n, r, c):
    rng = np.random.default_rng(70 + n + r + c)
    dmap = world["map"] if r == R else (np.array([5], np.int32) if r == 1 else rng.permutation(np.concatenate([np.arange(NDOF), np.full(r - NDOF, -1)])).astype(np.int32))
    t, m = setup(world, rng, n=n, dmap=dmap, extra_cols=c, noise=UNIFORM)
    assert t.proprio_layout()["width"] == 6 + c + 3 * r
    for s, noise in enumerate((False, True, True)):
        x = inputs(rng, n, r, c, nasty=(s == 0))
        got = run_dev(hip, t, x, noise=noise)
        check(got, m.step(**x, noise=noise), t.proprio_state(), m, (s, noise))
    rows = rng.normal(0, 1, (n, 13)).astype(F)
    assert t.proprio_reset(rows) == 0 == m.reset(rows)
    same(t.proprio_state()["last_root_vel"], m.last_root_vel, "last_root_vel")


# ---- 9. streams ------------------------------------------------------------------------------------------------------------------------
def test_the_device_calls_on_a_stream_of_their_own_give_the_synchronous_bytes(hip, world):
    rng = np.random.default_rng(69)
    (ta, _), (tb, _) = (setup(world, np.random.default_rng(690), noise=UNIFORM) for _ in range(2))
    st = hip.Stream()
    for s in range(2):
        x = inputs(rng)
        host = ta.proprio(**x, noise=True)
        got = run_dev(hip, tb, x, noise=True, stream=st)
        for k in OUTPUTS:
            same(got[k], host[k], (s, k))
        done = (rng.uniform(size=N) < 0.5).astype(np.int32)
        rows = rng.normal(0, 1, (N, 13)).astype(F)
        assert ta.proprio_reset(rows, done) == 0
        d_rows, d_done = hip.DeviceBuffer.from_host(rows), hip.DeviceBuffer.from_host(done)
        tb.proprio_reset_dev(d_rows, d_done, stream=st)
        ids = np.array([3, N + 4, 11], np.int32)
        assert ta.proprio_reset(rows[:3], env_ids=ids) == 1
        d_ids = hip.DeviceBuffer.from_host(ids)
        tb.proprio_reset_dev(d_rows, env_ids=d_ids, n=3, stream=st)
        st.sync()
        a, b = ta.proprio_state(), tb.proprio_state()
        for k in STATE6:
            same(a[k], b[k], (s, k))
    sa, sb = ta.state(), tb.state()
    for k in STATE:
        same(sa[k], sb[k], k)
    assert sa["ignored"] == sb["ignored"] == 2
