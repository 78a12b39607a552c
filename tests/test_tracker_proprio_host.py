"""The tracker's proprioception half without a GPU: the exports, their ctypes signatures and the layout of the four
structs against the header, every argument check that must fire before a device is touched, the float32 statement
(tests/proprio_mirror.py) against the fixture generated from the reference's own ``quat_rotate_inverse`` and ``apply_randomization``
(tests/golden/g_proprio.npz), and the mirror's Philox path."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header as abi  # noqa: E402
import proprio_mirror as pm  # noqa: E402
import tracker_mirror as tm  # noqa: E402
from test_motion_body_state_host import _OfflineLibrary  # noqa: E402
from test_motion_tracker_host import KNOWN_ANSWERS  # noqa: E402

PROPRIO_SYMBOLS = ("gmr_motion_tracker_set_proprio", "gmr_motion_tracker_proprio_dev", "gmr_motion_tracker_proprio", "gmr_motion_tracker_proprio_reset_dev",
                   "gmr_motion_tracker_proprio_reset", "gmr_motion_tracker_proprio_state")
F = np.float32
EPS = 2.0 ** -24


def test_the_library_exports_the_proprio_entry_points_with_the_headers_signatures():
    from general_motion_retargeting_amd import _lib
    from general_motion_retargeting_amd import motion_tracker as mt
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmr_hip.h")).read()
    assert "N10: tracker proprioception" in hdr and hdr.index("N10: tracker proprioception") > hdr.index("N9: tracker control")
    for sym in PROPRIO_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        m = re.search(r"\bint " + sym + r"\(([^;]*)\);", hdr)
        assert m, sym
        params = abi.parameters(hdr, sym)
        res, args = _lib._SIGS[sym]
        assert res is C.c_int and args == params, (sym, params, args)
        # the comment in front of the prototype (a _dev call and its twin share one) cites the reference lines it replaces
        section = hdr[hdr.index("N10: tracker proprioception"):m.start()]
        comment = [c for c in re.findall(r"/\*.*?\*/", section, flags=re.S) if "\n" in c][-1]
        assert re.search(r"t1\.py:\d+", comment), sym
    # the structs: the same fields in the same order
    for name, struct in (("gmr_proprio_noise_t", _lib.ProprioNoise), ("gmr_proprio_config_t", _lib.ProprioConfig), ("gmr_proprio_in_t", _lib.ProprioIn),
                         ("gmr_proprio_out_t", _lib.ProprioOut)):
        assert abi.fields(hdr, name) == [f for f, _ in struct._fields_], name
    P = C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.ProprioNoise) == 24 and C.sizeof(_lib.ProprioIn) == 8 * P and C.sizeof(_lib.ProprioOut) == 10 * P
    assert _lib.ProprioConfig.filter_weight.offset == 5 * P + 8 and _lib.ProprioConfig.noise.offset == 5 * P + 8 + 32 + 32
    assert C.sizeof(_lib.ProprioConfig) == 5 * P + 72 + 6 * 24
    for define, value in (("GMR_PROPRIO_TERMS", len(_lib.PROPRIO_TERMS)), ("GMR_PROPRIO_MAX_EXTRA", _lib.PROPRIO_MAX_EXTRA),
                          ("GMR_PROPRIO_NOISE_BLOCKS", len(_lib.PROPRIO_NOISE_BLOCKS)), ("GMR_NOISE_NONE", _lib.NOISE_DISTRIBUTIONS["none"]),
                          ("GMR_NOISE_GAUSSIAN", _lib.NOISE_DISTRIBUTIONS["gaussian"]), ("GMR_NOISE_UNIFORM", _lib.NOISE_DISTRIBUTIONS["uniform"]),
                          ("GMR_NOISE_ADDITIVE", _lib.NOISE_OPERATIONS["additive"]), ("GMR_NOISE_SCALING", _lib.NOISE_OPERATIONS["scaling"])):
        assert abi.define(hdr, define) == value, define
    assert mt.PROPRIO_TERMS == _lib.PROPRIO_TERMS == pm.TERMS and mt.PROPRIO_NOISE_BLOCKS == _lib.PROPRIO_NOISE_BLOCKS == pm.NOISE_BLOCKS
    assert mt.PROPRIO_MAX_EXTRA == _lib.PROPRIO_MAX_EXTRA and mt.NOISE_DISTRIBUTIONS == _lib.NOISE_DISTRIBUTIONS
    for name in ("set_proprio", "proprio", "proprio_dev", "proprio_reset", "proprio_reset_dev", "proprio_state", "proprio_layout"):
        assert callable(getattr(mt.MotionTracker, name)), name
    from general_motion_retargeting_amd import build
    assert "gmr_tracker_proprio.hip" in build.SOURCES


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def offline_tracker(N=8, R=5):
    from general_motion_retargeting_amd import MotionTracker
    t = MotionTracker.__new__(MotionTracker)
    t._init_state(_OfflineLibrary(R, "world"), N, R)
    return t


def test_proprio_arguments_are_refused_before_anything_touches_a_device(monkeypatch):
    from general_motion_retargeting_amd import _lib

    def no_device():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    N, R = 8, 5
    t = offline_tracker(N, R)
    roots, rows = np.zeros((N, 13), F), np.zeros((N, R), F)
    # proprio not set: every call says so
    assert t.proprio_state() is None
    for call in (lambda: t.proprio(roots, rows, rows), lambda: t.proprio_dev(1234, 1234, 1234, obs=1234), lambda: t.proprio_reset(roots),
                 lambda: t.proprio_reset_dev(1234), lambda: t.proprio_layout()):
        with pytest.raises(ValueError, match="set_proprio"):
            call()
    # the configuration
    lim = np.stack([-np.ones(R, F), np.ones(R, F)], axis=1)
    ok = dict(default_dof_pos=np.zeros(R, F), dof_pos_limits=lim, dof_vel_limits=np.ones(R, F), torque_limits=np.ones(R, F), base_height_target=0.7,
              terminate_vel=50.0, terminate_height=0.3, max_episode_steps=100)
    spec = {"distribution": "gaussian", "operation": "additive", "range": (0.0, 0.1)}
    bad = ((dict(default_dof_pos=np.zeros(R + 1, F)), ValueError, "default_dof_pos has shape"), (dict(default_dof_pos=np.full(R, np.nan, F)), ValueError, "not finite"),
           (dict(dof_pos_limits=lim.T), ValueError, "dof_pos_limits has shape"), (dict(dof_pos_limits=lim[:, ::-1]), ValueError, "upper < lower"),
           (dict(dof_pos_limits=lim * np.inf), ValueError, "not finite"), (dict(soft_dof_pos_limit=-1.5), ValueError, "upper < lower"),
           (dict(dof_vel_limits=np.ones(R - 1, F)), ValueError, "dof_vel_limits has shape"), (dict(torque_limits=np.full(R, np.inf, F)), ValueError, "not finite"),
           (dict(extra_cols=-1), ValueError, "extra_cols"), (dict(extra_cols=17), ValueError, "extra_cols"), (dict(extra_cols=1.5), ValueError, "extra_cols"),
           (dict(max_episode_steps=-1), ValueError, "max_episode_steps"), (dict(max_episode_steps=2.5), ValueError, "max_episode_steps"),
           (dict(filter_weight=np.nan), ValueError, "must be finite"), (dict(soft_torque_limit=np.inf), ValueError, "must be finite"),
           (dict(normalization={"dof_vel": np.inf}), ValueError, "must be finite"), (dict(normalization={"speed": 1.0}), KeyError, "unknown scales"),
           (dict(terminate_vel=np.nan), ValueError, "must be finite"), (dict(base_height_target=np.inf), ValueError, "must be finite"),
           (dict(noise={"wind": spec}), KeyError, "unknown blocks"), (dict(noise={"gravity": {**spec, "distribution": "cauchy"}}), ValueError, "distribution"),
           (dict(noise={"gravity": {**spec, "operation": "xor"}}), ValueError, "operation"), (dict(noise={"height": {**spec, "range": (0.0, -0.1)}}), ValueError, "negative"),
           (dict(noise={"height": {**spec, "range": (0.0, np.nan)}}), ValueError, "not finite"), (dict(noise={"height": {**spec, "range": (0.0,)}}), ValueError, "pair"),
           (dict(noise={"lin_vel": {"distribution": "uniform", "operation": "scaling", "range": (-3e38, 3e38)}}), ValueError, "not finite"),
           (dict(scales=np.ones(13, F)), ValueError, "scales has 13"), (dict(scales={"torques": np.nan}), ValueError, "scales must be finite"),
           (dict(scales={"feet_slip": 1.0}), KeyError, "unknown terms"))
    for kw, exc, match in bad:
        with pytest.raises(exc, match=match):
            t.set_proprio(**{**ok, **kw})
    assert t._proprio is None
    got = t._proprio_setup(**{**dict(extra_cols=0, filter_weight=1.0, normalization=None, noise={"height": None, "gravity": {"distribution": "none"}},
                                    soft_dof_pos_limit=1.0, soft_dof_vel_limit=1.0, soft_torque_limit=1.0, scales=None), **ok})
    assert got["noise"] == [(0, 0, 0.0, 0.0)] * 6 and not got["scales"].any() and got["norm"] == dict.fromkeys(("gravity", "lin_vel", "ang_vel", "dof_pos", "dof_vel"), 1.0)
    t._proprio = (R, 0)
    assert t.proprio_layout() == {"obs": {"gravity": (0, 3), "ang_vel": (3, 6), "extra": (6, 6), "dof_pos": (6, 11), "dof_vel": (11, 16), "actions": (16, 21)},
                                  "width": 21, "priv": {"lin_vel": (0, 3), "height": (3, 4)}, "terms": pm.TERMS}
    # shapes and dtypes of the step and the reset
    for call, exc, match in ((lambda: t.proprio(roots[:, :12], rows, rows), ValueError, "root_states: shape"), (lambda: t.proprio(roots, rows[:7], rows), ValueError, "dof_pos: shape"),
                             (lambda: t.proprio(roots, rows, rows.T), ValueError, "dof_vel: shape"), (lambda: t.proprio(roots, rows, rows, actions=rows[:, :4]), ValueError, "actions: shape"),
                             (lambda: t.proprio(roots, rows, rows, mean_torques=rows[:3]), ValueError, "mean_torques: shape"),
                             (lambda: t.proprio(roots, rows, rows, ground=np.zeros((N, 1), F)), ValueError, "ground: shape"),
                             (lambda: t.proprio(roots, rows, rows, episode_steps=np.zeros(N, F)), TypeError, "integers"),
                             (lambda: t.proprio(roots, rows, rows, episode_steps=np.zeros(N + 1, np.int32)), ValueError, "episode_steps: shape"),
                             (lambda: t.proprio(roots, rows, rows, extra=np.zeros((N, 1), F)), ValueError, "extra is needed exactly"),
                             (lambda: t.proprio_dev(1234, 1234, 1234, extra=1234), ValueError, "extra is needed exactly"),
                             (lambda: t.proprio(None, rows, rows), ValueError, "root_states is needed"), (lambda: t.proprio_dev(1234, None, 1234), ValueError, "dof_pos is needed"),
                             (lambda: t.proprio_dev(1234, 1234, 1234, reward=1234), TypeError, "unknown outputs"),
                             (lambda: t.proprio_dev(roots, 1234, 1234), TypeError, "device address"), (lambda: t.proprio_dev(1234, 1234, 1234, obs=[1]), TypeError, "device address"),
                             (lambda: t.proprio_reset(roots[:7]), ValueError, "root_states: shape"), (lambda: t.proprio_reset(roots[:2], env_ids=[1, 2, 3]), ValueError, "root_states: shape"),
                             (lambda: t.proprio_reset(roots[:3], env_ids=[1, 2, 1]), ValueError, "twice"), (lambda: t.proprio_reset(roots, mask=np.ones(7, bool)), ValueError, "mask: shape"),
                             (lambda: t.proprio_reset(roots, mask=np.ones(N, F)), TypeError, "bool or integer"),
                             (lambda: t.proprio_reset_dev(1234, env_ids=99), ValueError, "needs n"), (lambda: t.proprio_reset_dev(1234, n=7), ValueError, "every environment"),
                             (lambda: t.proprio_reset_dev(None), ValueError, "needed")):
        with pytest.raises(exc, match=match):
            call()
    t._proprio = (R, 3)
    with pytest.raises(ValueError, match="extra is needed exactly"):
        t.proprio(roots, rows, rows)
    with pytest.raises(ValueError, match="extra: shape"):
        t.proprio(roots, rows, rows, extra=np.zeros((N, 2), F))
    # a dof map that changed the number of robot dofs since
    t.nrobot_dof = R + 1
    for call in (lambda: t.proprio(roots, rows, rows), lambda: t.proprio_state(), lambda: t.proprio_reset(roots), lambda: t.proprio_layout()):
        with pytest.raises(ValueError, match="set_proprio\\(\\) again"):
            call()
    assert not (t._links or t._preview or t._adaptive or t._anchors or t._control)


# ---- the mirror against the fixture from the reference's functions ------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(GOLDEN, "g_proprio.npz"), allow_pickle=False)


def golden_config(g, **kw):
    norm = dict(zip(("gravity", "lin_vel", "ang_vel", "dof_pos", "dof_vel"), g["norm"].tolist()))
    ht, tv, th, ms = g["scalars"].tolist()
    soft = g["soft"].tolist()
    return pm.config(g["default_dof_pos"], g["dof_pos_limits"], g["dof_vel_limits"], g["torque_limits"], base_height_target=ht, terminate_vel=tv,
                     terminate_height=th, max_episode_steps=int(ms), extra_cols=g["s_extra"].shape[2], filter_weight=float(g["filter_weight"]),
                     normalization=norm, soft_dof_pos_limit=soft[0], soft_dof_vel_limit=soft[1], soft_torque_limit=soft[2], **kw)


def test_the_rotation_of_the_mirror_is_the_references_within_the_measured_bound():
    g = golden()
    got = pm.rotate_inverse(g["rot_q"], g["rot_v"])
    norm = np.maximum(1.0, np.linalg.norm(g["rot_v"].astype(np.float64), axis=1))[:, None]
    dev = np.abs(got.astype(np.float64) - g["rot_out"]) / norm
    print(f"rotation: largest deviation {dev.max() / EPS:.2f} x 2^-24 max(1, |v|), {np.mean(got == g['rot_out']) * 100:.1f} % bit-equal")
    assert dev.max() <= 8 * EPS


def test_the_mirror_follows_the_scripted_episode_of_the_fixture():
    """Bounds.  A rotated vector lies within d = 8 x 2^-24 max(1, |v|) of the reference's (the issue's bound, measured on the CPU against
    the reference function).  A filtered velocity is a convex combination of the rotated vectors since the last reset, so its bound is the sum
    of their d.  A sum over the dofs lies within R 2^-24 sum|summand| (another order of summation).  The three terms that square a rotated
    or filtered component x carry its deviation on top: |x'^2 - x^2| <= 2 |x| d + d^2 per component."""
    g = golden()
    steps, N, R = g["s_dof_pos"].shape
    cfg = golden_config(g)
    m = pm.Proprio(cfg, N, R, float(g["dt"]))
    resets = {int(s): (g[f"reset{int(s)}_envs"], g[f"reset{int(s)}_roots"]) for s in g["reset_steps"]}
    assert len(resets) == 2
    d64 = np.float64
    d_lin, d_ang = np.zeros(N), np.zeros(N)                  # the accumulated bounds of the filtered velocities
    seen_done, seen_count = set(), 0
    for s in range(steps):
        if s in resets:
            envs, rows = resets[s]
            assert m.reset(rows, env_ids=envs) == 0
            d_lin[envs], d_ang[envs] = 0.0, 0.0
        rs = g["s_root_states"][s]
        out = m.step(rs, g["s_dof_pos"][s], g["s_dof_vel"][s], g["s_actions"][s], g["s_torques"][s], g["s_extra"][s], g["s_ground"][s],
                     g["s_episode_steps"][s], noise=False)
        b_lin = 8 * EPS * np.maximum(1.0, np.linalg.norm(rs[:, 7:10].astype(d64), axis=1))
        b_ang = 8 * EPS * np.maximum(1.0, np.linalg.norm(rs[:, 10:13].astype(d64), axis=1))
        b_g = np.full(N, 8 * EPS)
        for k, b in (("base_lin_vel", b_lin), ("base_ang_vel", b_ang), ("projected_gravity", b_g)):
            assert (np.abs(out[k].astype(d64) - g[f"s_{k}"][s]) <= b[:, None]).all(), (k, s)
        d_lin, d_ang = d_lin + b_lin, d_ang + b_ang
        for k, b in (("filtered_lin_vel", d_lin), ("filtered_ang_vel", d_ang)):
            assert (np.abs(out[k].astype(d64) - g[f"s_{k}"][s]) <= b[:, None]).all(), (k, s)
        want, abs_sum = g["s_term"][s].astype(d64), g["s_abs_sum"][s].astype(d64)
        bound = R * EPS * abs_sum
        bound[:, 0] += 2 * np.abs(g["s_filtered_lin_vel"][s][:, 2]) * d_lin + d_lin ** 2
        bound[:, 1] += (2 * np.abs(g["s_base_ang_vel"][s][:, :2]) * b_ang[:, None] + b_ang[:, None] ** 2).sum(axis=1)
        bound[:, 2] += (2 * np.abs(g["s_projected_gravity"][s][:, :2]) * b_g[:, None] + b_g[:, None] ** 2).sum(axis=1)
        dev = np.abs(out["term"].astype(d64) - want)
        assert (dev <= bound).all(), (s, np.argwhere(dev > bound))
        assert np.array_equal(out["term"][:, 8], g["s_term"][s][:, 8])              # the count of dofs outside their soft limits
        seen_count += int(out["term"][:, 8].sum())
        assert np.array_equal(out["done"], g["s_done"][s]), s
        seen_done |= set(out["done"].tolist())
        # the clean rows: rotated blocks within their bounds, the others the same numbers
        priv = g["s_priv"][s]
        assert (np.abs(out["priv"][:, :3].astype(d64) - priv[:, :3]) <= b_lin[:, None] * float(cfg["norm"]["lin_vel"])).all()
        assert np.array_equal(out["priv"][:, 3], priv[:, 3])
        if s < len(g["s_obs"]):
            obs = g["s_obs"][s]
            assert obs.shape == out["obs"].shape
            assert (np.abs(out["obs"][:, :3].astype(d64) - obs[:, :3]) <= b_g[:, None] * float(cfg["norm"]["gravity"])).all()
            assert (np.abs(out["obs"][:, 3:6].astype(d64) - obs[:, 3:6]) <= b_ang[:, None] * float(cfg["norm"]["ang_vel"])).all()
            assert np.array_equal(out["obs"][:, 6:], obs[:, 6:])
    assert seen_done >= {0, 1, 2, 4} and seen_count > 100
    for k in ("last_root_vel", "last_actions", "last_dof_vel"):
        assert np.array_equal(getattr(m, k), g[f"final_{k}"]), k
    assert not m.noise_tick.any()
    # total: the weighted terms in rising order, a zero scale and an absent input left out
    scales = {"torques": -2e-4, "dof_acc": -1e-7, "action_rate": -1.0, "base_height": -20.0, "dof_pos_limits": -1.0}
    m2 = pm.Proprio(golden_config(g, scales=scales), N, R, float(g["dt"]))
    full = m2.step(g["s_root_states"][0], g["s_dof_pos"][0], g["s_dof_vel"][0], g["s_actions"][0], g["s_torques"][0], g["s_extra"][0])
    sc = m2.cfg["scale"]
    want = np.zeros(N, F)
    for k in (3, 5, 7, 8, 13):
        want = want + sc[k] * full["term"][:, k]
    assert np.array_equal(full["total"], want) and (sc != 0).sum() == 5
    m3 = pm.Proprio(m2.cfg, N, R, float(g["dt"]))
    bare = m3.step(g["s_root_states"][0], g["s_dof_pos"][0], g["s_dof_vel"][0], None, None, g["s_extra"][0])
    want = np.zeros(N, F)
    for k in (5, 8, 13):
        want = want + sc[k] * bare["term"][:, k]
    assert np.array_equal(bare["total"], want) and not bare["term"][:, [3, 7, 10, 11, 12]].any() and not bare["obs"][:, -R:].any()
    assert not m3.last_actions.any() and np.array_equal(m3.last_dof_vel, g["s_dof_vel"][0])


def test_the_noise_application_of_the_mirror_is_the_references_on_its_own_draws():
    g = golden()
    for name, op in (("gaussian", "additive"), ("uniform", "scaling")):
        cfg = pm.config(np.zeros(1), np.zeros((1, 2)), np.zeros(1), np.ones(1), base_height_target=0, terminate_vel=0, terminate_height=0, max_episode_steps=0,
                        noise={"dof_pos": {"distribution": name, "operation": op, "range": g[f"noise_{name}_range"].tolist()}})
        got = pm.apply_noise(g["noise_x"], cfg["noise"]["dof_pos"], g[f"noise_{name}_unit"])
        assert np.array_equal(got, g[f"noise_{name}_result"]), name


# ---- the Philox path of the mirror ----------------------------------------------------------------------------------------------------
def test_the_draw_of_the_mirror_word_for_word(monkeypatch):
    for ctr, key, want in KNOWN_ANSWERS:
        w = tm.philox4x32(ctr, key)
        assert " ".join("%08x" % x for x in w) == want
        assert pm.pair(w, 0) == pm.pair(w, 6) == (w[0], w[1]) and pm.pair(w, 1) == pm.pair(w, 7) == (w[2], w[3])
        for wa, wb in (pm.pair(w, 0), pm.pair(w, 1)):
            u1, u2 = pm.unit_open(wa), pm.unit(wb)
            assert u1 == F(((wa >> 8) + 1) / 2.0 ** 24) and 0 < u1 <= 1 and u2 == F((wb >> 8) / 2.0 ** 24) and 0 <= u2 < 1
            z = pm.gaussian32(wa, wb)
            assert abs(float(z) - pm.gaussian64(wa, wb)) <= 8 * EPS * max(1.0, abs(float(z)))
    # the counter: (environment, tick, element / 2, 1) under the tracker's key; elements 2 k and 2 k + 1 share one call's four words
    seen = []
    real = tm.philox4x32

    def spy(counter, key):
        seen.append((tuple(counter), tuple(key)))
        return real(counter, key)

    monkeypatch.setattr(tm, "philox4x32", spy)
    key = (0x89ABCDEF, 0x01234567)
    a, b = pm.words(key, 5, 9, 12), pm.words(key, 5, 9, 13)
    assert seen == [((5, 9, 6, 1), key)] * 2 and a + b == real((5, 9, 6, 1), key)
    assert pm.Proprio(pm.config(np.zeros(1), np.zeros((1, 2)), np.zeros(1), np.ones(1), base_height_target=0, terminate_vel=0, terminate_height=0,
                                max_episode_steps=0), 1, 1, 0.02, seed=0x0123456789ABCDEF).key == key
    # the ends of the open interval: u1 in (0, 1], so the logarithm is finite and |z| <= sqrt(-2 ln 2^-24) = 5.768
    assert pm.unit_open(0) == F(EPS) and pm.unit_open(0xFFFFFFFF) == F(1.0) and pm.unit(0xFFFFFFFF) < 1
    assert abs(float(pm.gaussian32(0, 0)) - np.sqrt(-2 * np.log(EPS))) < 1e-5 and float(pm.gaussian32(0, 0)) <= 5.77
    assert pm.gaussian32(0xFFFFFFFF, 0x12345678) == 0


def test_noise_off_or_no_spec_moves_no_tick_and_leaves_the_clean_rows():
    g = golden()
    N, R = g["s_dof_pos"].shape[1:]
    spec = {"distribution": "uniform", "operation": "additive", "range": (-0.1, 0.3)}
    args = (g["s_root_states"][0], g["s_dof_pos"][0], g["s_dof_vel"][0], g["s_actions"][0], g["s_torques"][0], g["s_extra"][0], g["s_ground"][0])
    clean = pm.Proprio(golden_config(g), N, R, 0.02, seed=3)
    a = clean.step(*args, noise=True)
    assert not clean.noise_tick.any()
    noisy = pm.Proprio(golden_config(g, noise={"dof_vel": spec, "height": spec}), N, R, 0.02, seed=3)
    b = noisy.step(*args, noise=False)
    assert not noisy.noise_tick.any() and np.array_equal(a["obs"], b["obs"]) and np.array_equal(a["priv"], b["priv"])
    c = noisy.step(*args, noise=True, wide=True)
    assert (noisy.noise_tick == 1).all()
    lay = slice(6 + 5 + R, 6 + 5 + 2 * R)
    diff = c["obs"] != a["obs"]
    assert diff[:, lay].all() and not np.delete(diff, np.arange(lay.start, lay.stop), axis=1).any()
    assert (c["priv"][:, 3] != a["priv"][:, 3]).all() and np.array_equal(c["priv"][:, :3], a["priv"][:, :3])
    u = c["z64"][:, lay]
    assert ((0 <= u) & (u < 1)).all() and 0.3 < u.mean() < 0.7
    d = noisy.step(*args, noise=True)
    assert (noisy.noise_tick == 2).all() and not np.array_equal(c["obs"], d["obs"])          # another tick, another draw
