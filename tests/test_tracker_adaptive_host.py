"""Adaptive start sampling and masked resets of the tracker without a GPU: exports against the header, the bin
tables and the bin of a clock on hand-made libraries, an Adapt on hand-made counts, the statistics of the draw (on the NumPy statement,
tests/adaptive_mirror.py, which the device reproduces bit for bit), the plain masked reset against ``reset`` on the compacted list, and
every argument check that must fire before a device is touched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_mirror as am  # noqa: E402
import motion_mirror as mm  # noqa: E402
import tracker_mirror as tm  # noqa: E402
from test_motion_body_state_host import _OfflineLibrary  # noqa: E402
from test_motion_library import _bits, make_motions  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTIVE_SYMBOLS = ("gmr_motion_tracker_set_adaptive", "gmr_motion_tracker_adapt_dev", "gmr_motion_tracker_adapt", "gmr_motion_tracker_reset_done_dev",
                    "gmr_motion_tracker_reset_done", "gmr_motion_tracker_adaptive_state")
F = np.float32
EPS = 2.0 ** -52


def test_the_library_exports_the_adaptive_entry_points():
    from general_motion_retargeting_amd import _lib
    from general_motion_retargeting_amd import motion_tracker as mt
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gmr_hip.h")).read()
    for sym in ADAPTIVE_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
    assert (mt.ADAPTIVE_MAX_BINS, mt.ADAPTIVE_MAX_LOOKAHEAD) == (am.MAX_BINS, am.MAX_K) == (1 << 22, 16)
    assert set(mt.DEFAULT_ADAPTIVE) == {"bin_seconds", "alpha", "uniform", "lookahead", "gamma"}
    for name in ("set_adaptive", "adapt", "adapt_dev", "reset_done", "reset_done_dev", "adaptive_state"):
        assert callable(getattr(mt.MotionTracker, name)), name


# ---- bins ---------------------------------------------------------------------------------------------------------------------------
def test_bin_tables_of_a_hand_made_library():
    from general_motion_retargeting_amd.motion_tracker import _adaptive_bins
    #       T = 0, T = 1, a multiple of F, F + 1, another fps (F = 15: 2 full bins and one of 7), weight zero
    lens = [0, 1, 90, 31, 37, 60]
    fps = [30.0, 30.0, 30.0, 30.0, 14.6, 30.0]
    seg = np.concatenate([[0], np.cumsum(lens)])
    w = np.array([5.0, 1.0, 2.0, 1.0, 4.0, 0.0])           # (the weight of the empty clip does not enter)
    b = am.Bins(seg, fps, 1.0, w)
    assert b.F.tolist() == [30, 30, 30, 30, 15, 30]          # llround(14.6) = 15
    assert b.bin_start.tolist() == [0, 0, 1, 4, 6, 9, 11] and b.Bt == 11
    assert b.clip.tolist() == [1, 2, 2, 2, 3, 3, 4, 4, 4, 5, 5]
    assert b.first.tolist() == [0, 0, 30, 60, 0, 30, 0, 15, 30, 0, 30]
    assert b.frames.tolist() == [1, 30, 30, 30, 30, 1, 15, 15, 7, 30, 30]
    assert b.last.tolist() == [0, 3, 3, 3, 5, 5, 8, 8, 8, 10, 10]
    assert abs(b.base.sum() - 1.0) <= b.Bt * EPS
    assert np.array_equal(b.base[9:], [0.0, 0.0]) and (b.base[:9] > 0).all()
    assert np.allclose(np.bincount(b.clip, weights=b.base, minlength=6), w * [0, 1, 1, 1, 1, 1] / 8.0, rtol=0, atol=4 * EPS)
    assert b.base[4] == (1.0 / 8.0) * 30.0 / 31.0 and b.base[5] == (1.0 / 8.0) * 1.0 / 31.0
    # without weights: 1 / (number of clips that have frames)
    u = am.Bins(seg, fps, 1.0)
    assert np.allclose(np.bincount(u.clip, weights=u.base, minlength=6), [0, .2, .2, .2, .2, .2], rtol=0, atol=4 * EPS)
    assert abs(u.base.sum() - 1.0) <= u.Bt * EPS
    # the package computes the same tables before it touches a device; half-way cases round away from zero
    for bs in (1.0, 0.5, 0.05, 1.0 / 30.0, 3.0, 100.0):
        got, Fc = _adaptive_bins(seg, fps, bs)
        want = am.Bins(seg, fps, bs)
        assert np.array_equal(got, want.bin_start) and np.array_equal(Fc, want.F), bs
    assert am.round_half_away(2.5) == 3 and am.round_half_away(0.49999999999999994) == 0 and am.round_half_away(0.5) == 1
    assert am.Bins([0, 10], [30.0], 0.001).F.tolist() == [1]                 # never narrower than one frame
    assert am.Bins([0, 10], [30.0], 1e6).bin_start.tolist() == [0, 1]       # one bin for a clip shorter than a bin
    with pytest.raises(ValueError):
        am.Bins([0, 0, 0], [30.0, 30.0], 1.0)                                # no bins at all
    with pytest.raises(ValueError):
        am.Bins(seg, fps, 1.0, [1.0, 0, 0, 0, 0, 0])                         # only the empty clip has weight


def hand_clip(T, fps):
    z = np.zeros((T, 3))
    return {"fps": fps, "root_pos": z, "root_rot": np.tile([0.0, 0.0, 0.0, 1.0], (T, 1)), "dof_pos": z, "local_body_pos": None}


def test_the_bin_of_a_clock():
    T, fps = 9, 64.0                       # duration 9 / 64, the last frame at 8 / 64 = 0.125: all exact in float32
    lib = mm.Library([hand_clip(T, fps), hand_clip(1, fps)], "world")
    last, dur = F(0.125), F(9.0 / 64.0)
    #                 frame 3    the last frame   inside the last   an ulp past the end      negative     T = 1   bad clip   NaN
    times = np.array([3.0 / 64.0, last, np.nextafter(last, F(1)), np.nextafter(dur, F(1)), -1.0 / 64.0, 5.0, 0.0, np.nan], dtype=F)
    clips = np.array([0, 0, 0, 0, 0, 1, 2, 0])
    want = {True: [1, 4, 4, 0, 4, 5, -1, -1],           # loop: past the end wraps to frame 0, a negative time to the last frame
            False: [1, 4, 4, 4, 0, 5, -1, -1]}          # clamp: past the end stays on the last frame, a negative time on frame 0
    for loop in (True, False):
        t = am.AdaptiveTracker(lib, len(times), 0.02, loop=loop)
        t.set_adaptive(2.0 / 64.0)                      # F = 2: bins [0, 2) [2, 4) [4, 6) [6, 8) [8, 9) and the one of clip 1
        assert t.bins.bin_start.tolist() == [0, 5, 6]
        t.assign(clips, times)
        assert [t.bin_of(e) for e in range(len(times))] == want[loop], loop


# ---- Adapt --------------------------------------------------------------------------------------------------------------------------
def test_adapt_on_hand_made_counts():
    seg = np.concatenate([[0], np.cumsum([300, 240, 90, 150])])
    fps = [30.0] * 4
    bins = am.Bins(seg, fps, 1.0, [1.0, 1.0, 0.0, 2.0])      # 10, 8, 3 (weight zero) and 5 bins
    assert bins.bin_start.tolist() == [0, 10, 18, 21, 26]
    zero = np.zeros(bins.Bt)
    # a single failing bin spreads backwards over K - 1 bins with ratios gamma^u
    fail = np.zeros(bins.Bt, np.uint32)
    fail[6] = 5
    ema, s, p, cdf = am.adapt(bins, zero, fail, 0.5, 0.0, 4, 0.5)
    assert ema[6] == 2.5 and not np.delete(ema, 6).any()
    assert np.array_equal(s[3:7], 2.5 * np.array([0.125, 0.25, 0.5, 1.0])) and not np.delete(s, [3, 4, 5, 6]).any()
    assert np.array_equal(p[3:7] / p[6], [0.125, 0.25, 0.5, 1.0]) and abs(p.sum() - 1.0) <= bins.Bt * EPS
    assert cdf[0] == 0.0 and (np.diff(cdf) >= 0).all() and np.array_equal(cdf[:4], np.zeros(4)) and np.array_equal(cdf[7:], np.full(19, cdf[7]))
    # ... and stops at the clip's first bin: it never leaks into the previous clip
    fail[:] = 0
    fail[11] = 3                                             # the second bin of clip 1
    ema, s, p, cdf = am.adapt(bins, zero, fail, 1.0, 0.0, 4, 0.5)
    assert np.array_equal(s[10:12], [1.5, 3.0]) and not s[:10].any() and not s[12:].any()
    # the last bin of a clip stands in for the bins behind it: they would lie in the next clip
    fail[:] = 0
    fail[9] = 1
    fail[10] = 1
    ema, s, p, cdf = am.adapt(bins, zero, fail, 1.0, 0.0, 3, 0.5)
    assert np.array_equal(s[7:10], [0.25, 0.75, 1.75]) and s[10] == 1.0 and not s[:7].any()      # bin 9 counts itself 1 + .5 + .25 times
    # a clip of weight zero keeps s = 0 whatever fails in it
    fail[:] = 0
    fail[19] = 7
    ema, s, p, cdf = am.adapt(bins, zero, fail, 1.0, 0.0, 4, 0.5)
    assert ema[19] == 7.0 and not s.any() and np.array_equal(p, bins.base)          # S = 0 gives base
    fail[4] = 1
    ema, s, p, cdf = am.adapt(bins, zero, fail, 1.0, 0.25, 4, 0.5)
    assert not p[18:21].any() and p[4] > bins.base[4]
    # uniform = 1 gives base; S = 0 gives base
    ema, s, p, cdf = am.adapt(bins, zero, fail, 0.3, 1.0, 4, 0.8)
    assert s.any() and np.array_equal(p, bins.base)
    ema, s, p, cdf = am.adapt(bins, zero, np.zeros(bins.Bt, np.uint32), 0.3, 0.0, 4, 0.8)
    assert np.array_equal(p, bins.base) and np.array_equal(cdf[1:], np.cumsum(bins.base)[:-1])
    # alpha = 1 forgets history, alpha = 0 never learns, in between it decays
    old = np.arange(bins.Bt, dtype=np.float64)
    assert np.array_equal(am.adapt(bins, old, fail, 1.0, 0.5, 2, 0.8)[0], fail.astype(np.float64))
    assert np.array_equal(am.adapt(bins, old, fail, 0.0, 0.5, 2, 0.8)[0], old)
    assert np.array_equal(am.adapt(bins, old, fail, 0.25, 0.5, 2, 0.8)[0], 0.75 * old + 0.25 * fail)
    # on a tracker: the counters are zero afterwards, a fresh configuration samples from base, the same bin_seconds keeps the history
    lib = mm.Library([hand_clip(n, 30.0) for n in (300, 240, 90, 150)], "world")
    t = am.AdaptiveTracker(lib, 4, 0.02, clip_weights=[1.0, 1.0, 0.0, 2.0], loop=False)
    t.set_adaptive(1.0, alpha=0.5, uniform=0.0, lookahead=4, gamma=0.5)
    assert np.array_equal(t.prob, bins.base) and not t.ema.any()
    t.fail_now[6] = 5
    t.adapt()
    assert not t.fail_now.any() and t.ema[6] == 2.5
    t.set_adaptive(1.0, alpha=1.0, uniform=0.0, lookahead=1, gamma=1.0)
    assert t.ema[6] == 2.5 and t.prob[5] > 0                 # nothing ran: the history and the probabilities of the last Adapt
    t.adapt()
    assert not t.ema.any() and np.array_equal(t.prob, bins.base)
    t.fail_now[6] = 1
    t.set_adaptive(2.0)                                      # other bins: everything starts over
    assert t.bins.Bt == 5 + 4 + 2 + 3 and not t.ema.any() and not t.fail_now.any()


# ---- the draw -------------------------------------------------------------------------------------------------------------------------
def test_vector_philox_is_the_trackers():
    key = (0x12345678, 0x9ABCDEF0)
    e = np.array([0, 1, 7, 4999, 2 ** 26 - 1])
    d = np.array([0, 3, 2 ** 32 - 1, 17, 5])
    w0, w1 = am.philox4x32_many(e, d, key)
    for i in range(len(e)):
        assert (int(w0[i]), int(w1[i])) == tm.philox4x32((int(e[i]), int(d[i]), 0, 0), key)[:2]


def test_draw_statistics():
    """n draws from a fixed p: every bin whose expected count is at least 20 within 4 sigma of n p, the mean start of every such bin
    within 4 sigma of the bin's centre, every start inside the frames of its bin.  n = 200 000 and seed 0 were chosen on the CPU (the
    draw is counter-based, so the outcome is deterministic): the rule leaves out under 5 % of the bins with p > 0."""
    rng = np.random.default_rng(0)
    lens = rng.integers(0, 901, size=40)
    fps = rng.choice([30.0, 50.0, 120.0, 29.97], size=40)
    seg = np.concatenate([[0], np.cumsum(lens)])
    bins = am.Bins(seg, fps, 1.0)
    fail = np.zeros(bins.Bt, np.uint32)
    fail[rng.choice(bins.Bt, size=12, replace=False)] = rng.integers(1, 40, size=12)
    _, _, p, cdf = am.adapt(bins, np.zeros(bins.Bt), fail, 0.1, 0.3, 4, 0.8)
    assert cdf[0] == 0.0 and (np.diff(cdf) >= 0).all() and abs(p.sum() - 1.0) <= bins.Bt * EPS
    n, seed = 200_000, 0
    w0, w1 = am.philox4x32_many(np.arange(n), np.zeros(n), (seed & tm.M32, seed >> 32))
    b, c, time = am.bin_draws(bins, cdf, w0, w1)
    assert time.dtype == F and (time >= 0).all() and np.array_equal(c, bins.clip[b])
    # every start lies in the frames of its bin: by the library's own frame arithmetic, in integers
    frame = np.floor(time.astype(np.float64) * bins.fps[c]).astype(np.int64)
    assert ((frame >= bins.first[b]) & (frame < bins.first[b] + bins.frames[b])).all()
    count = np.bincount(b, minlength=bins.Bt)
    assert not count[p == 0].any()
    tested = n * p >= 20
    assert tested.sum() >= 0.95 * (p > 0).sum(), (int(tested.sum()), int((p > 0).sum()))
    sigma = np.sqrt(n * p * (1 - p))
    dev = np.abs(count - n * p)[tested] / sigma[tested]
    print(f"bins {bins.Bt}, tested {int(tested.sum())}, largest count deviation {dev.max():.2f} sigma")
    assert dev.max() <= 4.0
    # starts are uniform inside a bin: the mean of m uniform starts over a span w has sigma w / sqrt(12 m)
    span = bins.frames / bins.fps[bins.clip]
    centre = bins.first / bins.fps[bins.clip] + span / 2
    mean = np.bincount(b, weights=time.astype(np.float64), minlength=bins.Bt) / np.maximum(count, 1)
    dev_t = (np.abs(mean - centre) / (span / np.sqrt(12.0 * np.maximum(count, 1))))[tested]
    print(f"largest deviation of a bin's mean start {dev_t.max():.2f} sigma")
    assert dev_t.max() <= 4.0


def test_tracker_draws_are_the_vector_draws_and_restart_finished_clips_from_the_bins():
    rng = np.random.default_rng(3)
    motions = make_motions(rng, [40, 3, 200, 75, 1, 130], 5, 0)
    t = am.AdaptiveTracker(mm.Library(motions, "world"), 50, 0.05, loop=False, seed=(9 << 32) | 11)
    t.set_adaptive(0.5, alpha=0.5, uniform=0.2, lookahead=3, gamma=0.7)
    t.fail_now[[2, 5, 6]] = [4, 1, 9]
    t.adapt()
    w0, w1 = am.philox4x32_many(np.arange(50), np.zeros(50), t.key)
    _, c, time = am.bin_draws(t.bins, t.bin_cdf, w0, w1)
    assert t.reset_done() == 0
    assert np.array_equal(t.clip, c) and np.array_equal(_bits(t.time), _bits(time)) and (t.draws == 1).all()
    assert np.array_equal(_bits(t.length), _bits(np.array([t.clip_length(int(k)) for k in c], dtype=F)))
    # steps: a finished clip takes clip AND start time from the bins, one draw, nothing recorded
    restarts = 0
    for _ in range(120):
        before = t.state()
        out = t.step()
        fin = out["finished"] == 1
        restarts += int(fin.sum())
        assert np.array_equal(t.draws, before["draws"] + fin)
        w0, w1 = am.philox4x32_many(np.nonzero(fin)[0], before["draws"][fin], t.key)
        _, c, time = am.bin_draws(t.bins, t.bin_cdf, w0, w1)
        assert np.array_equal(t.clip[fin], c) and np.array_equal(_bits(t.time[fin]), _bits(time))
        assert np.array_equal(_bits(t.time[~fin]), _bits((before["time"] + t.dtf).astype(F)[~fin]))
    assert restarts > 50 and (t.time[t.clip == 2] > 0).any() and not t.fail_now.any()


# ---- the plain masked reset -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [True, False])
def test_plain_masked_reset_is_reset_on_the_compacted_list(loop):
    rng = np.random.default_rng(17 + loop)
    motions = make_motions(rng, [30, 2, 90, 55], 4, 0)
    lib = mm.Library(motions, "world")
    kw = dict(loop=loop, seed=77, clip_weights=[1.0, 0.0, 3.0, 2.0])
    a, b = am.AdaptiveTracker(lib, 300, 0.02, **kw), tm.Tracker(lib, 300, 0.02, **kw)
    for frac, resample, rng_t in ((1.0, True, (0.0, 0.0)), (0.02, True, (0.5, 2.0)), (0.0, True, (0.0, 1.0)), (0.3, False, (-1.0, 1.0)), (0.02, True, (0.0, 0.0))):
        done = rng.uniform(size=300) < frac
        failed = rng.uniform(size=300) < 0.5                  # a plain tracker has nowhere to record: ignored
        assert a.reset_done(done, failed, resample=resample, time_offset_range=rng_t) == 0
        if done.any():
            b.reset(np.nonzero(done)[0], resample=resample, time_offset_range=rng_t)
        for k in ("clip", "time", "length", "draws"):
            assert np.array_equal(_bits(a.state()[k]), _bits(b.state()[k])), (k, frac)
        a.step(), b.step()
    # by list: the flags belong to the list positions; ids outside [0, N) count only where the entry is done
    ids = np.array([5, 299, -1, 300, 17, 4])
    done = np.array([1, 0, 1, 0, 1, 1])
    assert a.reset_done(done, None, env_ids=ids) == 1 and b.reset([5, -1, 17, 4]) == 1
    assert all(np.array_equal(_bits(a.state()[k]), _bits(b.state()[k])) for k in ("clip", "time", "length", "draws")) and a.ignored == b.ignored == 1
    # done = None resets every entry
    assert a.reset_done(env_ids=[3, 8]) == 0 and b.reset([3, 8]) == 0 and np.array_equal(a.draws, b.draws)
    assert a.reset_done() == 0 and b.reset() == 0 and np.array_equal(_bits(a.time), _bits(b.time)) and np.array_equal(a.clip, b.clip)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def offline_tracker(lens=(30, 0, 200), fps=(30.0, 50.0, 120.0), N=8):
    from general_motion_retargeting_amd import MotionTracker
    t = MotionTracker.__new__(MotionTracker)
    lib = _OfflineLibrary(5)
    lib.seg_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    lib._fps = np.asarray(fps, dtype=np.float64)
    lib.num_clips = len(fps)
    t._init_state(lib, N, 5)
    return t


def test_adaptive_arguments_are_refused_before_anything_touches_a_device(monkeypatch):
    from general_motion_retargeting_amd import _lib

    def no_device():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    t = offline_tracker()
    for kw, match in ((dict(lookahead=0), "lookahead"), (dict(lookahead=17), "lookahead"), (dict(lookahead=2.5), "lookahead"),
                      (dict(alpha=-0.1), "alpha"), (dict(alpha=1.5), "alpha"), (dict(alpha=np.nan), "alpha"),
                      (dict(uniform=-1e-9), "uniform"), (dict(uniform=1.0000001), "uniform"), (dict(uniform=np.nan), "uniform"),
                      (dict(gamma=0.0), "gamma"), (dict(gamma=1.5), "gamma"), (dict(gamma=np.nan), "gamma"),
                      (dict(bin_seconds=np.nan), "bin_seconds"), (dict(bin_seconds=np.inf), "bin_seconds")):
        with pytest.raises(ValueError, match=match):
            t.set_adaptive(**kw)
    with pytest.raises(ValueError, match="bins"):          # 5 000 000 frames in bins of one frame: more than 2^22
        offline_tracker(lens=(5_000_000,), fps=(30.0,)).set_adaptive(bin_seconds=1.0 / 30.0)
    with pytest.raises(ValueError, match="bins"):          # a library without a frame has no bin
        offline_tracker(lens=(0, 0), fps=(30.0, 30.0)).set_adaptive()
    assert t._adaptive_setup(1.0, 0.0, 1.0, 16, 1.0)[5].tolist() == [0, 1, 1, 3] and t._adaptive is None
    # adaptive calls on a plain tracker
    for call in (t.adapt, t.adapt_dev, t.adaptive_state):
        with pytest.raises(ValueError, match="set_adaptive"):
            call()
    # the masks of a masked reset
    for call in (t.reset_done, t.reset_done_dev):
        with pytest.raises(ValueError, match="finite"):
            call(time_offset_range=(0.0, np.inf))
    for kw, exc, match in ((dict(done=np.ones(7, bool)), ValueError, "done: shape"), (dict(failed=np.ones((8, 1), bool)), ValueError, "failed: shape"),
                           (dict(done=np.ones(8, F)), TypeError, "bool or integer"), (dict(done=np.ones(8, bool), env_ids=[1, 2]), ValueError, "done: shape"),
                           (dict(env_ids=[1, 2, 1]), ValueError, "twice"), (dict(failed=np.ones(3, np.float64), env_ids=[1, 2, 3]), TypeError, "bool or integer")):
        with pytest.raises(exc, match=match):
            t.reset_done(**kw)
    assert t.reset_done(env_ids=[]) == 0                     # nothing listed: nothing to do, and nothing touched
    with pytest.raises(ValueError, match="needs n"):
        t.reset_done_dev(env_ids=1234)
    with pytest.raises(ValueError, match="every environment"):
        t.reset_done_dev(done=1234, n=7)
    with pytest.raises(TypeError, match="device address"):
        t.reset_done_dev(done=np.ones(8, np.int32))
    # an adaptive tracker draws clip and start from its bins: no range, no resample = False
    t._adaptive = (1.0, np.array([0, 1, 1, 3]))
    for call in (t.reset_done, t.reset_done_dev):
        with pytest.raises(ValueError, match="resample=True"):
            call(resample=False)
        with pytest.raises(ValueError, match="time_offset_range"):
            call(time_offset_range=(0.0, 0.5))
        with pytest.raises(ValueError, match="time_offset_range"):
            call(time_offset_range=(0.25, 0.25))
    # the mirror refuses the same
    m = am.AdaptiveTracker(mm.Library([hand_clip(9, 64.0)], "world"), 4, 0.02)
    with pytest.raises(ValueError):
        m.adapt()
    for kw in (dict(lookahead=0), dict(lookahead=17), dict(alpha=1.5), dict(uniform=-0.5), dict(gamma=0.0)):
        with pytest.raises(ValueError):
            m.set_adaptive(**kw)
    m.set_adaptive(1.0)
    with pytest.raises(ValueError):
        m.reset_done(resample=False)
    with pytest.raises(ValueError):
        m.reset_done(time_offset_range=(0.0, 1.0))
