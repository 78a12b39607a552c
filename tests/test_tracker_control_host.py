"""The tracker's control half without a GPU: the exports, their ctypes signatures and the layout of
``gmr_tracker_actuator_t`` against the header, every argument check that must fire before a device is touched, and the float32 statement
(tests/control_mirror.py) against an independent statement of the same formulas in float32 torch operations on the CPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header as abi  # noqa: E402
import control_mirror as cm  # noqa: E402
from test_motion_body_state_host import _OfflineLibrary  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTROL_SYMBOLS = ("gmr_motion_tracker_set_control", "gmr_motion_tracker_targets_dev", "gmr_motion_tracker_targets", "gmr_motion_tracker_hold_dev",
                   "gmr_motion_tracker_hold", "gmr_motion_tracker_torques_dev", "gmr_motion_tracker_torques", "gmr_motion_tracker_control_state")
F = np.float32


def test_the_library_exports_the_control_entry_points_with_the_headers_signatures():
    from general_motion_retargeting_amd import _lib
    from general_motion_retargeting_amd import motion_tracker as mt
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmr_hip.h")).read()
    assert "N9: tracker control" in hdr and hdr.index("N9: tracker control") > hdr.index("N8: tracker anchors")
    for sym in CONTROL_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        m = re.search(r"\bint " + sym + r"\(([^;]*)\);", hdr)
        assert m, sym
        params = abi.parameters(hdr, sym)
        res, args = _lib._SIGS[sym]
        assert res is C.c_int and args == params, (sym, params, args)
        # the comment in front of the prototype (a _dev call and its twin share one) cites the reference lines it replaces
        section = hdr[hdr.index("N9: tracker control"):m.start()]
        comment = [c for c in re.findall(r"/\*.*?\*/", section, flags=re.S) if "\n" in c][-1]
        assert re.search(r"t1(_imitation)?\.py:\d+", comment), sym
    # the struct: the same fields in the same order, four pointers and an int32
    body = re.search(r"typedef struct \{([^}]*)\} gmr_tracker_actuator_t", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f for f, _ in _lib.TrackerActuator._fields_]
    assert re.findall(r"\*(\w+)", body) + re.findall(r"int32_t (\w+);", body) == fields == list(_lib.TRACKER_ACTUATOR_FIELDS) + ["per_env"]
    P = C.sizeof(C.c_void_p)
    assert [getattr(_lib.TrackerActuator, f).offset for f in fields] == [0, P, 2 * P, 3 * P, 4 * P]
    assert C.sizeof(_lib.TrackerActuator) == 5 * P and _lib.TrackerActuator.per_env.size == 4
    assert f"#define GMR_CONTROL_MAX_DECIMATION {_lib.CONTROL_MAX_DECIMATION}" in hdr and mt.CONTROL_MAX_DECIMATION == _lib.CONTROL_MAX_DECIMATION
    for name in ("set_control", "targets", "targets_dev", "hold", "hold_dev", "torques", "torques_dev", "control_state"):
        assert callable(getattr(mt.MotionTracker, name)), name
    from general_motion_retargeting_amd import build
    assert "gmr_tracker_control.hip" in build.SOURCES


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def offline_tracker(N=8, R=5):
    from general_motion_retargeting_amd import MotionTracker
    t = MotionTracker.__new__(MotionTracker)
    t._init_state(_OfflineLibrary(R, "world"), N, R)
    return t


def test_control_arguments_are_refused_before_anything_touches_a_device(monkeypatch):
    from general_motion_retargeting_amd import _lib

    def no_device():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    N, R, M = 8, 5, 4
    t = offline_tracker(N, R)
    rows, gains, per_dof = np.zeros((N, R), F), np.ones((N, R), F), np.ones(R, F)
    # control not set: every call says so
    assert t.control_state() is None
    for call in (lambda: t.targets(), lambda: t.targets_dev(dof_targets=1234), lambda: t.hold(rows), lambda: t.hold_dev(1234),
                 lambda: t.torques(0, rows, rows, rows, per_dof, per_dof),
                 lambda: t.torques_dev(0, 1234, 1234, 1234, 1234, 1234, 1234)):
        with pytest.raises(ValueError, match="set_control"):
            call()
    # the configuration
    ok = dict(default_dof_pos=np.zeros(R, F), action_scale=1.0, clip_actions=1.0, decimation=M)
    for kw, match in ((dict(default_dof_pos=np.zeros(R + 1, F)), "default_dof_pos has"), (dict(default_dof_pos=np.full(R, np.nan, F)), "not finite"),
                      (dict(action_scale=np.inf), "must be finite"), (dict(gain_run=np.nan), "must be finite"), (dict(clip_actions=0.0), "clip_actions"),
                      (dict(clip_actions=-1.0), "clip_actions"), (dict(clip_actions=np.nan), "clip_actions"), (dict(startup_seconds=-0.5), "startup_seconds"),
                      (dict(startup_seconds=np.inf), "startup_seconds"), (dict(decimation=0), "decimation"), (dict(decimation=65), "decimation"),
                      (dict(decimation=2.5), "decimation")):
        with pytest.raises(ValueError, match=match):
            t.set_control(**{**ok, **kw})
    assert t._control is None
    assert t._control_setup(np.zeros(R), 1.0, np.inf, 0.0, 0.1, 0.2, 64)[2:4] == (np.inf, 0.0)          # inf: no clipping, 0: no start-up
    t._control = (R, M)
    # shapes and dtypes of targets, hold and torques
    for call, exc, match in ((lambda: t.targets(actions=rows[:, :4]), ValueError, "actions: shape"), (lambda: t.targets(actions=rows[:7]), ValueError, "actions: shape"),
                             (lambda: t.targets(episode_steps=np.zeros(7, np.int32)), ValueError, "episode_steps: shape"),
                             (lambda: t.targets(episode_steps=np.zeros(N, F)), TypeError, "integers"),
                             (lambda: t.targets_dev(actions_clipped=1234), ValueError, "needs actions"),
                             (lambda: t.targets_dev(dof_targets=rows), TypeError, "device address"),
                             (lambda: t.hold(rows[:7]), ValueError, "dof_pos: shape"), (lambda: t.hold(rows[:2], env_ids=[1, 2, 3]), ValueError, "dof_pos: shape"),
                             (lambda: t.hold(rows[:3], env_ids=[1, 2, 1]), ValueError, "twice"), (lambda: t.hold(rows, mask=np.ones(7, bool)), ValueError, "mask: shape"),
                             (lambda: t.hold(rows, mask=np.ones(N, F)), TypeError, "bool or integer"),
                             (lambda: t.hold_dev(1234, env_ids=99), ValueError, "needs n"), (lambda: t.hold_dev(1234, n=7), ValueError, "every environment"),
                             (lambda: t.hold_dev(None), ValueError, "needed"),
                             (lambda: t.torques(0, rows[:, :4], rows, rows, per_dof, per_dof), ValueError, "dof_targets: shape"),
                             (lambda: t.torques(0, rows, rows[:7], rows, per_dof, per_dof), ValueError, "dof_pos: shape"),
                             (lambda: t.torques(0, rows, rows, rows.T, per_dof, per_dof), ValueError, "dof_vel: shape"),
                             (lambda: t.torques(0, rows, rows, rows, per_dof, per_dof, delay_steps=np.zeros(7, np.int32)), ValueError, "delay_steps: shape"),
                             (lambda: t.torques(0, rows, rows, rows, per_dof, per_dof, torque_limit=gains), ValueError, "torque_limit has shape"),
                             (lambda: t.torques(0, rows, rows, rows, per_dof, None), ValueError, "damping is needed")):
        with pytest.raises(exc, match=match):
            call()
    # a substep outside [0, M)
    for i in (-1, M, M + 3, 1.5):
        with pytest.raises(ValueError, match="substep"):
            t.torques(i, rows, rows, rows, per_dof, per_dof)
        with pytest.raises(ValueError, match="substep"):
            t.torques_dev(i, 1234, 1234, 1234, 1234, 1234, 1234)
    # per_env: the three gain arrays share one shape, and it is the one per_env names
    for kw in (dict(stiffness=gains, damping=per_dof), dict(stiffness=per_dof, damping=gains), dict(stiffness=gains, damping=gains, friction=per_dof),
               dict(stiffness=per_dof, damping=per_dof, friction=gains), dict(stiffness=per_dof, damping=per_dof, per_env=True),
               dict(stiffness=gains, damping=gains, per_env=False), dict(stiffness=np.ones((N, R + 1), F), damping=np.ones((N, R + 1), F))):
        with pytest.raises(ValueError, match="per_env"):
            t.torques(0, rows, rows, rows, **kw)
    with pytest.raises(ValueError, match="dof_torques is needed"):
        t.torques_dev(0, 1234, 1234, 1234, 1234, 1234, None)
    # a dof map that changed the number of robot dofs since
    t.nrobot_dof = R + 1
    with pytest.raises(ValueError, match="set_control\\(\\) again"):
        t.targets()
    assert not (t._links or t._preview or t._adaptive or t._anchors)


# ---- the float32 statement against torch on the CPU ---------------------------------------------------------------------------------
def same_numbers(a, b, what):
    """numerically equal with NaNs at the same positions"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype == F and a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), what


def torch_targets(torch, d, k, c, D, g0, g1, dt, ref, actions, steps):
    """section 2 of the issue, line by line in float32 torch"""
    f32 = torch.float32
    te = steps.to(f32) * torch.tensor(dt, dtype=f32)
    startup = te < D
    p = torch.clamp(te / D, 0.0, 1.0)
    s = 0.5 * (1.0 - torch.cos(p * 3.14159))
    eased = d.unsqueeze(0) * (1.0 - s.unsqueeze(1)) + ref * s.unsqueeze(1)
    base = torch.where(startup.unsqueeze(1), eased, ref)
    a = torch.clamp(actions, -c, c) if np.isfinite(c) else actions.clone()
    gain = torch.where(startup, torch.tensor(g0, dtype=f32), torch.tensor(g1, dtype=f32))
    return base + (k * a) * gain.unsqueeze(1), a, startup, s


@pytest.mark.parametrize("clip_actions", [0.75, np.inf])
def test_the_targets_of_the_mirror_are_the_formulas_in_torch(clip_actions):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    N, R, dt, D = 600, 23, 0.02, 2.0
    d = rng.uniform(-0.5, 0.5, R).astype(F)
    ref = rng.uniform(-1.2, 1.2, (N, R)).astype(F)
    actions = rng.normal(0, 1.0, (N, R)).astype(F)
    actions[5, 3], actions[17, 0], actions[100, 22] = np.nan, np.inf, -np.inf
    steps = rng.integers(-1, 201, N).astype(np.int32)          # both phases: te = 2 D at the top
    steps[:6] = [100, 99, 101, -1, 0, -7]                      # te exactly D (100 * 0.02f rounds to 2.0f), its neighbours, negative steps
    assert F(100) * F(dt) == F(D)
    cfg = cm.config(d, 0.25, clip_actions, 4, D, 0.1, 0.2)
    got, clipped, status = cm.targets(cfg, ref, actions, steps, dt)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    want, a, startup, s = torch_targets(torch, tt(d), 0.25, clip_actions, D, 0.1, 0.2, dt, tt(ref), tt(actions), tt(steps))
    want, a, startup, s = want.numpy(), a.numpy(), startup.numpy(), s.numpy()
    assert want.dtype == F and not status.any()
    m_startup, m_s = cm.phase(cfg, steps, dt)
    assert np.array_equal(m_startup, startup) and startup.any() and (~startup).any() and not startup[0] and startup[1] and startup[3]
    same_numbers(clipped, a, "actions_clipped")
    same_numbers(got[~startup], want[~startup], "the run phase")
    # the cos line: two float32 cosines, each good to an ulp or two of a number of size one
    assert np.abs(m_s[startup].astype(np.float64) - s[startup]).max() <= 4 * 2.0 ** -24
    fin = np.isfinite(want) & startup[:, None]
    assert np.array_equal(np.isnan(got[startup]), np.isnan(want[startup])) and np.array_equal(np.isinf(got), np.isinf(want))
    dev = np.abs(got[fin].astype(np.float64) - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    print(f"start-up, mirror against torch: largest deviation {dev.max():.3e} of max(1, |x|)")
    assert dev.max() <= 2e-6
    # without steps every environment runs; without actions the target is the base; a bad assignment is a NaN row
    run, _, _ = cm.targets(cfg, ref, actions, None, dt)
    want_run, _, _, _ = torch_targets(torch, tt(d), 0.25, clip_actions, D, 0.1, 0.2, dt, tt(ref), tt(actions), torch.full((N,), 10 ** 6, dtype=torch.int32))
    same_numbers(run, want_run.numpy(), "no episode_steps")
    base, none, _ = cm.targets(cfg, ref, None, steps, dt)
    assert none is None and np.array_equal(base[~startup], ref[~startup])
    bad = np.zeros(N, bool)
    bad[[2, 9]] = True
    out, clipped2, status = cm.targets(cfg, ref, actions, steps, dt, bad)
    assert np.isnan(out[bad]).all() and np.array_equal(status, bad.astype(np.int32)) and np.array_equal(np.isnan(out[~bad]), np.isnan(got[~bad]))
    same_numbers(clipped2, clipped, "actions_clipped of a bad assignment")
    # D = 0: no start-up phase at a step count that is not negative
    cfg0 = cm.config(d, 0.25, clip_actions, 4, 0.0)
    su0, _ = cm.phase(cfg0, np.array([0, 1, 50], np.int32), dt)
    assert not su0.any()


def torch_torques(torch, i, M, held, acc, tg, q, qd, kp, kd, fr, lim, delay):
    """section 4 of the issue in float32 torch: the reference's own operators"""
    held, acc = held.clone(), acc.clone()
    held[delay == i] = tg[delay == i]
    tau = kp * (held - q) - kd * qd
    if fr is not None:
        tau = tau - torch.min(fr.expand_as(tau), tau.abs()) * torch.sign(tau)
    if lim is not None:
        tau = torch.clip(tau, min=-lim, max=lim)
    if i == 0:
        acc.zero_()
    acc += tau
    return tau, held, acc, (acc / M if i == M - 1 else None)


@pytest.mark.parametrize("per_env", [True, False])
@pytest.mark.parametrize("friction,limit", [(True, True), (False, True), (True, False), (False, False)])
def test_the_substep_loop_of_the_mirror_is_the_formulas_in_torch(per_env, friction, limit):
    torch = pytest.importorskip("torch")
    assert torch.sign(torch.tensor(float("nan"))).item() == 0.0          # the sgn of the issue: +1, -1 or +0
    rng = np.random.default_rng(13 + 2 * per_env + friction)
    N, R, M = 300, 23, 5
    shape = (N, R) if per_env else (R,)
    kp, kd = rng.uniform(20, 200, shape).astype(F), rng.uniform(0.5, 5, shape).astype(F)
    fr = rng.uniform(0.0, 3.0, shape).astype(F) if friction else None
    if friction:
        fr.reshape(-1)[1] = np.nan
        fr.reshape(-1)[2] = 1e9                                    # larger than any |tau|
    lim = rng.uniform(5, 40, R).astype(F) if limit else None
    delay = rng.integers(0, M, N).astype(np.int32)
    delay[:M] = np.arange(M)                                       # every delay in 0 .. M - 1
    delay[M], delay[M + 1] = M, -1                                 # and two that never match
    cfg = cm.config(np.zeros(R, F), 1.0, 1.0, M)
    mirror = cm.Actuators(cfg, N, R)
    start = rng.uniform(-1, 1, (N, R)).astype(F)
    assert mirror.hold(start) == 0
    tt = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy())      # noqa: E731
    held, acc = tt(start), torch.zeros(N, R)
    tg = rng.uniform(-1, 1, (N, R)).astype(F)
    seen = {"zero": False, "nan": False, "friction_wins": False, "clipped": False}
    for i in range(M):
        q, qd = rng.uniform(-1, 1, (N, R)).astype(F), rng.uniform(-4, 4, (N, R)).astype(F)
        q[7], qd[7] = mirror.held[7] if delay[7] != i else tg[7], 0.0          # zero torques
        q[8, 4] = np.nan                                            # NaN torques
        qd[9, :] = 0.0
        q[9, :] = (mirror.held[9] if delay[9] != i else tg[9]) - F(1e-6)          # |tau| <= 200 x 1e-6, below the friction
        tau, mean = mirror.torques(i, tg, q, qd, kp, kd, fr, lim, delay)
        want, held, acc, want_mean = torch_torques(torch, i, M, held, acc, tt(tg), tt(q), tt(qd), tt(kp), tt(kd), tt(fr), tt(lim), tt(delay))
        same_numbers(tau, want.numpy(), ("dof_torques", i))
        same_numbers(mirror.held, held.numpy(), ("held", i))
        same_numbers(mirror.acc, acc.numpy(), ("torque_acc", i))
        assert (mean is None) == (want_mean is None) == (i != M - 1)
        if mean is not None:
            same_numbers(mean, want_mean.numpy(), "mean_torques")
        finite = ~np.isnan(tau[7])                                  # (a NaN friction of a dof makes its column NaN)
        seen["zero"] |= bool(finite.sum() >= R - 1 and (tau[7][finite] == 0).all())
        seen["nan"] |= bool(np.isnan(tau[8, 4]))
        if friction:
            large = np.broadcast_to(fr, (N, R))[9] > 0.01          # (a NaN friction is not)
            seen["friction_wins"] |= bool(large.sum() > R // 2 and (tau[9][large] == 0).all())
        if limit:
            seen["clipped"] |= bool((np.abs(tau) == lim[None, :]).any())
    assert seen["zero"] and seen["nan"] and seen["friction_wins"] == friction and seen["clipped"] == limit
    # the environments whose delay never matches hold what they were given
    assert np.array_equal(mirror.held[M], start[M]) and np.array_equal(mirror.held[M + 1], start[M + 1]) and np.array_equal(mirror.held[2], tg[2])
    # a masked hold with ids outside [0, N)
    rows = rng.uniform(-1, 1, (4, R)).astype(F)
    assert mirror.hold(rows, mask=[1, 0, 1, 1], env_ids=[3, 4, N, -2]) == 2 and mirror.ignored == 2
    assert np.array_equal(mirror.held[3], rows[0]) and not mirror.acc[3].any() and not np.array_equal(mirror.held[4], rows[1])
