"""The tracker's control half on a real MI355X (csrc/gmr_tracker_control.hip through motion_tracker.py): the targets
are the reference row a following step returns, bit for bit, and move nothing; run-phase targets and the clipped actions are the float32
statement of tests/control_mirror.py; start-up targets against the float64 formula on the device's own reference row; bad assignments;
the substep loop of the actuator model against the mirror; the device entry points on a stream of their own.  N = 37 environments (no
multiple of 16 or 64) on four clips of 1, 2, 33 and 70 frames with 21 dofs mapped onto R = 23 (851 elements: a tail of three behind the
16-byte accesses), M = 4 substeps; every test makes one pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_mirror as cm  # noqa: E402
from test_motion_library import _bits, device_library, make_motions  # noqa: E402
from test_motion_tracker import STATE, tracker  # noqa: E402
from test_tracker_anchor import clocks, random_anchors  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
N = 37
R = 23
NDOF = 21
M = 4
DT = 0.02
D = 2.0
G = 64                                   # guard floats behind every device output
SENTINEL = F(-77.25)
START_UP_BOUND = 2e-6                    # x max(1, |x|): start-up targets against the float64 formula (the tracker's bound)


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def world(hip):
    """the library of four clips with the 21 dofs of booster_t1_4dof (built once, never written) and the map onto R = 23"""
    rng = np.random.default_rng(1800)
    motions = make_motions(rng, [1, 2, 33, 70], NDOF, 0)
    for m, fps in zip(motions, (30.0, 50.0, 120.0, 29.97)):
        m["fps"] = fps
    dmap = np.concatenate([rng.permutation(NDOF), [-1, -1]]).astype(np.int32)
    dmap[[3, 22]] = dmap[[22, 3]]                       # the two -1 columns: 3 and 21
    assert (dmap == -1).sum() == 2 and dmap[3] == -1 and dmap[21] == -1
    return {"lib": device_library(hip, motions), "map": dmap}


def control_tracker(world, rng, loop=True, n=N, dmap=None, clip_actions=0.75, startup=D, **kw):
    """a tracker on the world's library with control set, every environment at a clock of its own -> (tracker, mirror configuration)"""
    dmap = world["map"] if dmap is None else dmap
    r = len(dmap)
    default, pose = rng.uniform(-0.4, 0.4, r).astype(F), rng.uniform(-0.6, 0.6, r).astype(F)
    t = tracker(world["lib"], n, DT, dmap, default, loop=loop, **kw)
    clip, time = clocks(rng, world["lib"])
    clip, time = clip[:n].copy(), time[:n].copy()
    if n >= 8:
        time[5], time[6] = F(3.0), F(-0.25)             # past the end (wrapped or clamped) and before the start
    assert t.assign(clip, time) == 0
    t.set_control(pose, 0.25, clip_actions, startup, 0.1, 0.2, decimation=M)
    return t, cm.config(pose, 0.25, clip_actions, M, startup, 0.1, 0.2)


def same(a, b, what):
    """the same bits; a NaN matches a NaN at the same position whatever its payload"""
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if a.dtype != F:
        assert np.array_equal(a, b), what
        return
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan]), what


def same_numbers(a, b, what):
    """numerically equal with NaNs at the same positions"""
    assert a.dtype == b.dtype == F and a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), what


def random_actions(rng, n=N, r=R):
    a = rng.normal(0, 0.8, (n, r)).astype(F)            # a third beyond the clip of 0.75
    flat = a.reshape(-1)
    flat[1 % flat.size], flat[7 % flat.size], flat[-1] = np.nan, np.inf, -np.inf
    return a


# ---- 1. the targets are the step's reference row, and move nothing -------------------------------------------------------------------
@pytest.mark.parametrize("anchors", [False, True])
@pytest.mark.parametrize("loop", [True, False])
def test_plain_targets_are_the_reference_row_of_the_following_step(hip, world, loop, anchors):
    rng = np.random.default_rng(2 + loop + 2 * anchors)
    t, _ = control_tracker(world, rng, loop=loop, seed=3)
    if anchors:
        t.set_anchor(*random_anchors(rng))
    before = t.state()
    got = t.targets()
    after = t.state()
    for k in STATE:
        same(before[k], after[k], k)
    assert before["ignored"] == after["ignored"] and set(got) == {"dof_targets", "status"} and not got["status"].any()
    ref = t.step()
    assert not np.isnan(ref["ref_dof_pos"]).any()
    same(got["dof_targets"], ref["ref_dof_pos"], "dof_targets")
    off = world["map"] < 0
    assert off.sum() == 2 and (got["dof_targets"][:, off] == got["dof_targets"][0, off]).all()          # the two columns on their defaults
    st = t.control_state()
    assert not st["held"].any() and not st["torque_acc"].any()          # set_control leaves zeros, targets writes neither


# ---- 2. the run phase ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip_actions", [0.75, np.inf])
def test_run_phase_targets_and_clipped_actions_are_the_mirrors_bits(hip, world, clip_actions):
    rng = np.random.default_rng(5)
    t, cfg = control_tracker(world, rng, clip_actions=clip_actions)
    actions = random_actions(rng)
    late = rng.integers(100, 5000, N).astype(np.int32)                   # te >= D: 100 * 0.02f is 2.0f exactly
    late[0] = 100
    plain, stepped = t.targets(actions), t.targets(actions, late)
    ref = t.step()["ref_dof_pos"]
    want, clipped, status = cm.targets(cfg, ref, actions, None, DT)
    for got in (plain, stepped):
        same(got["dof_targets"], want, "dof_targets")
        same(got["actions_clipped"], clipped, "actions_clipped")
        assert np.array_equal(got["status"], status)
    assert np.isnan(want).sum() == 1 and (np.isinf(want).sum() == 2) == (clip_actions == np.inf)


# ---- 3. the start-up phase -----------------------------------------------------------------------------------------------------------
def test_startup_targets_against_the_float64_formula_on_the_devices_reference_row(hip, world):
    """Largest deviation met on an MI355X: see DESIGN.md section 6p (the bound is the tracker's, 2e-6 x max(1, |x|))."""
    rng = np.random.default_rng(6)
    t, cfg = control_tracker(world, rng)
    actions = rng.normal(0, 0.8, (N, R)).astype(F)
    steps = np.round(np.linspace(-1, 2 * D / DT, N)).astype(np.int32)       # -1 .. 200: both phases
    steps[[1, 2, 3]] = [100, 99, 0]                                        # the boundary te = D, the step before it, the start
    got = t.targets(actions, steps)
    ref = t.step()["ref_dof_pos"]
    want32, clipped, _ = cm.targets(cfg, ref, actions, steps, DT)
    startup, _ = cm.phase(cfg, steps, DT)
    assert startup.sum() >= 10 and (~startup).sum() >= 10 and not startup[1] and startup[2] and startup[0]
    same(got["actions_clipped"], clipped, "actions_clipped")
    same(got["dof_targets"][~startup], want32[~startup], "the environments outside start-up")
    # float64 on the float32 inputs; the phase is decided by the float32 product, as the kernel decides it
    d64 = np.float64
    te = (steps.astype(F) * F(DT)).astype(d64)
    p = np.clip(te / D, 0.0, 1.0)
    s = (0.5 * (1.0 - np.cos(p * d64(cm.PI_LITERAL))))[:, None]
    base = cfg["default_pos"].astype(d64)[None, :] * (1.0 - s) + ref.astype(d64) * s
    want = base + (d64(cfg["k"]) * clipped.astype(d64)) * d64(cfg["g0"])
    dev = np.abs(got["dof_targets"].astype(d64) - want)[startup] / np.maximum(1.0, np.abs(want[startup]))
    print(f"start-up targets: largest deviation from float64 {dev.max():.3e} of max(1, |x|) (bound 2e-6)")
    assert dev.max() <= START_UP_BOUND
    # at step 0 the target is the default pose plus the action term, whatever the reference says
    zero = got["dof_targets"][3]
    assert np.array_equal(zero, (cfg["default_pos"] * F(1.0) + ref[3] * F(0.0) + (cfg["k"] * clipped[3]) * cfg["g0"]).astype(F))


# ---- 4. bad assignments and the guard rows -------------------------------------------------------------------------------------------
def test_bad_assignments_give_nan_rows_and_nothing_leaves_the_outputs(hip, world):
    rng = np.random.default_rng(7)
    t, cfg = control_tracker(world, rng)
    st = t.state()
    clip, time = st["clip"].copy(), st["time"].copy()
    bad = {3: (7, 0.1), 4: (-1, 0.2), 11: (1, np.nan), 12: (2, np.inf), 36: (4, 0.0)}
    for e, (c, tt) in bad.items():
        clip[e], time[e] = c, tt
    t.assign(clip, time)
    isbad = np.zeros(N, bool)
    isbad[list(bad)] = True
    actions = random_actions(rng)
    steps = rng.integers(-1, 201, N).astype(np.int32)
    steps[3] = 10
    bufs = {k: hip.DeviceBuffer.from_host(np.full(n + G, SENTINEL, dtype=F)) for k, n in (("dof_targets", N * R), ("actions_clipped", N * R), ("status", N))}
    t.targets_dev(hip.DeviceBuffer.from_host(actions), hip.DeviceBuffer.from_host(steps), **bufs)
    hip.check(hip.lib().gmr_stream_sync(None))
    raw = {k: b.to_host(b.nbytes // 4, F) for k, b in bufs.items()}
    for k, n in (("dof_targets", N * R), ("actions_clipped", N * R), ("status", N)):
        assert (raw[k][n:] == SENTINEL).all(), k                          # the guard floats
    targets, clipped = raw["dof_targets"][:N * R].reshape(N, R), raw["actions_clipped"][:N * R].reshape(N, R)
    assert np.array_equal(raw["status"][:N].view(np.int32), isbad.astype(np.int32))
    assert np.isnan(targets[isbad]).all()
    same(clipped, cm.clip_sym(actions, cfg["c"]), "actions_clipped")     # written for a bad assignment too
    host = t.targets(actions, steps)
    same(host["dof_targets"], targets, "the synchronous call")
    ref = t.step()["ref_dof_pos"]
    assert np.isnan(ref[isbad]).all()
    want, _, status = cm.targets(cfg, ref, actions, steps, DT, isbad)
    startup, _ = cm.phase(cfg, steps, DT)
    same(targets[~startup], want[~startup], "the run phase around the bad rows")
    assert np.array_equal(np.isnan(targets), np.isnan(want)) and np.array_equal(host["status"], status)


# ---- 5. the substep loop ---------------------------------------------------------------------------------------------------------------
def actuator_inputs(rng, n, r, per_env, friction, limit, delay):
    shape = (n, r) if per_env else (r,)
    kp, kd = rng.uniform(20, 200, shape).astype(F), rng.uniform(0.5, 5, shape).astype(F)
    fr = lim = ds = None
    if friction:
        fr = rng.uniform(0.0, 3.0, shape).astype(F)
        fr.reshape(-1)[fr.size // 2] = 1e9                              # larger than any |tau|
        if fr.size > 2:
            fr.reshape(-1)[1] = np.nan
    if limit:
        lim = rng.uniform(5, 40, r).astype(F)                           # kp |held - q| reaches 400
    if delay:
        ds = rng.integers(0, M, n).astype(np.int32)
        ds[:min(n, M)] = np.arange(M)[:n]                               # every delay in 0 .. M - 1
        if n > M + 1:
            ds[M], ds[M + 1] = M, -1                                    # and two that never match
    return kp, kd, fr, lim, ds


def substep_loop(t, mirror, rng, tg, kp, kd, fr, lim, ds, expect_clipped=False):
    """M launches against the mirror: dof_torques and held after every substep, mean_torques after the last"""
    n, r = tg.shape
    for i in range(M):
        q, qd = rng.uniform(-1, 1, (n, r)).astype(F), rng.uniform(-4, 4, (n, r)).astype(F)
        q[-1], qd[-1] = (mirror.held[-1] if ds is not None and ds[-1] != i else tg[-1]), 0.0          # zero torques
        q[0, 0] = np.nan                                                   # a NaN torque
        got = t.torques(i, tg, q, qd, kp, kd, fr, lim, ds)
        tau, mean = mirror.torques(i, tg, q, qd, kp, kd, fr, lim, ds)
        same_numbers(got["dof_torques"], tau, ("dof_torques", i))
        state = t.control_state()
        same_numbers(state["held"], mirror.held, ("held", i))
        same_numbers(state["torque_acc"], mirror.acc, ("torque_acc", i))
        assert ("mean_torques" in got) == (i == M - 1)
    same_numbers(got["mean_torques"], mean, "mean_torques")
    finite = ~np.isnan(tau[-1])
    assert np.isnan(tau[0, 0]) and finite.sum() >= max(r - 2, 1) and (tau[-1][finite] == 0).all()
    if expect_clipped:
        assert (np.abs(tau) == lim[None, :]).any()


@pytest.mark.parametrize("per_env,friction,limit,delay", [(True, True, True, True), (False, True, True, True), (True, False, False, False),
                                                          (False, False, True, False), (True, True, False, True), (False, True, False, False)])
def test_a_substep_loop_is_the_mirrors(hip, world, per_env, friction, limit, delay):
    rng = np.random.default_rng(8 + per_env + 2 * friction + 4 * limit)
    t, cfg = control_tracker(world, rng)
    mirror = cm.Actuators(cfg, N, R)
    kp, kd, fr, lim, ds = actuator_inputs(rng, N, R, per_env, friction, limit, delay)
    tg = t.targets(rng.normal(0, 0.5, (N, R)).astype(F))["dof_targets"]
    substep_loop(t, mirror, rng, tg, kp, kd, fr, lim, ds, expect_clipped=limit)
    if delay:
        assert not mirror.held[M].any() and not mirror.held[M + 1].any() and np.array_equal(mirror.held[2], tg[2])
    # a masked hold with ids outside [0, N), then a second loop
    before = t.state()
    ids = np.array([5, N, 9, -3, 0, 2 ** 31 - 1, 30], np.int32)
    mask = np.array([1, 1, 0, 1, 1, 0, 1], np.int32)
    rows = rng.uniform(-1, 1, (len(ids), R)).astype(F)
    assert t.hold(rows, mask, ids) == 2 == mirror.hold(rows, mask, ids)
    after = t.state()
    assert after["ignored"] == before["ignored"] + 2
    for k in STATE:
        same(before[k], after[k], k)
    state = t.control_state()
    same_numbers(state["held"], mirror.held, "held after hold")
    same_numbers(state["torque_acc"], mirror.acc, "torque_acc after hold")
    assert np.array_equal(state["held"][30], rows[6]) and not state["torque_acc"][5].any() and not np.array_equal(state["held"][9], rows[2])
    substep_loop(t, mirror, rng, rng.uniform(-1, 1, (N, R)).astype(F), kp, kd, fr, lim, ds)
    # a hold of every environment by its done flags
    done = rng.uniform(size=N) < 0.5
    rows = rng.uniform(-1, 1, (N, R)).astype(F)
    assert t.hold(rows, done) == 0 == mirror.hold(rows, done)
    same_numbers(t.control_state()["held"], mirror.held, "held after a masked hold of all")


@pytest.mark.parametrize("n,r", [(N, 1), (N, 64), (1, R)])
def test_one_dof_sixty_four_dofs_and_one_environment(hip, world, n, r):
    rng = np.random.default_rng(20 + n + r)
    dmap = world["map"] if r == R else (np.array([5], np.int32) if r == 1 else rng.permutation(np.concatenate([np.arange(NDOF), np.full(r - NDOF, -1)])).astype(np.int32))
    t, cfg = control_tracker(world, rng, n=n, dmap=dmap)
    actions = random_actions(rng, n, r)
    got = t.targets(actions)
    ref = t.step()["ref_dof_pos"]
    want, clipped, _ = cm.targets(cfg, ref, actions, None, DT)
    same(got["dof_targets"], want, "dof_targets")
    same(got["actions_clipped"], clipped, "actions_clipped")
    for per_env in (True, False):
        mirror = cm.Actuators(cfg, n, r)
        rows = rng.uniform(-1, 1, (n, r)).astype(F)
        assert t.hold(rows) == 0 == mirror.hold(rows)
        substep_loop(t, mirror, rng, np.nan_to_num(want), *actuator_inputs(rng, n, r, per_env, True, True, True))


# ---- 6. streams ------------------------------------------------------------------------------------------------------------------------
def test_the_device_calls_on_a_stream_of_their_own_give_the_synchronous_bytes(hip, world):
    rng = np.random.default_rng(9)
    (ta, cfg), (tb, _), (tc, _) = (control_tracker(world, np.random.default_rng(90)) for _ in range(3))
    st = hip.Stream()
    actions, steps = random_actions(rng), rng.integers(-1, 201, N).astype(np.int32)
    kp, kd, fr, lim, ds = actuator_inputs(rng, N, R, True, True, True, True)
    up = lambda a: hip.DeviceBuffer.from_host(a)      # noqa: E731
    guarded = lambda n: hip.DeviceBuffer.from_host(np.full(n + G, SENTINEL, dtype=F))      # noqa: E731
    d_actions, d_steps, d_kp, d_kd, d_fr, d_lim, d_ds = (up(a) for a in (actions, steps, kp, kd, fr, lim, ds))
    out = {k: guarded(N * R) for k in ("dof_targets", "actions_clipped", "dof_torques", "mean_torques")}
    out["status"] = guarded(N)
    # the same loop with dof_pos four bytes off a 16-byte boundary: the kernel without the 16-byte accesses, the same bytes
    shifted = hip.DeviceBuffer((N * R + 1) * 4)
    off_tau = guarded(N * R)
    done = (rng.uniform(size=N) < 0.5).astype(np.int32)
    hold_rows = rng.uniform(-1, 1, (N, R)).astype(F)
    want_hold = ta.hold(hold_rows, done)
    d_hold, d_done = up(hold_rows), up(done)
    tb.hold_dev(d_hold, d_done, stream=st)
    tc.hold(hold_rows, done)
    assert want_hold == 0
    want = ta.targets(actions, steps)
    tb.targets_dev(d_actions, d_steps, out["dof_targets"], out["actions_clipped"], out["status"], stream=st)
    st.sync()
    for k in ("dof_targets", "actions_clipped"):
        raw = out[k].to_host(N * R + G, F)
        same(raw[:N * R].reshape(N, R), want[k], k)
        assert (raw[N * R:] == SENTINEL).all(), k
    raw = out["status"].to_host(N + G, F)
    assert np.array_equal(raw[:N].view(np.int32), want["status"]) and (raw[N:] == SENTINEL).all()
    tg = np.nan_to_num(want["dof_targets"])
    d_tg = up(tg)
    for i in range(M):
        q, qd = rng.uniform(-1, 1, (N, R)).astype(F), rng.uniform(-4, 4, (N, R)).astype(F)
        host = ta.torques(i, tg, q, qd, kp, kd, fr, lim, ds)
        d_q, d_qd = up(q), up(qd)
        tb.torques_dev(i, d_tg, d_q, d_qd, d_kp, d_kd, out["dof_torques"], d_fr, d_lim, d_ds, out["mean_torques"], per_env=True, stream=st)
        st.sync()
        raw = out["dof_torques"].to_host(N * R + G, F)
        same(raw[:N * R].reshape(N, R), host["dof_torques"], ("dof_torques", i))
        assert (raw[N * R:] == SENTINEL).all()
        raw = out["mean_torques"].to_host(N * R + G, F)
        assert (raw[N * R:] == SENTINEL).all()
        if i < M - 1:
            assert (raw == SENTINEL).all()                                 # written by the last substep only
        else:
            same(raw[:N * R].reshape(N, R), host["mean_torques"], "mean_torques")
        hip.check(hip.lib().gmr_memcpy_h2d(shifted.ptr.value + 4, q.ctypes.data, q.nbytes, None))
        tc.torques_dev(i, d_tg, shifted.ptr.value + 4, d_qd, d_kp, d_kd, off_tau, d_fr, d_lim, d_ds, per_env=True)
        hip.check(hip.lib().gmr_stream_sync(None))
        raw = off_tau.to_host(N * R + G, F)
        same(raw[:N * R].reshape(N, R), host["dof_torques"], ("dof_torques off the boundary", i))
        assert (raw[N * R:] == SENTINEL).all()
    a, b, c = ta.control_state(), tb.control_state(), tc.control_state()
    for k in ("held", "torque_acc"):
        same(a[k], b[k], k)
        same(a[k], c[k], k)
    sa, sb = ta.state(), tb.state()
    for k in STATE:
        same(sa[k], sb[k], k)
