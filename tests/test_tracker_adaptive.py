"""Adaptive start sampling and masked resets of the tracker on a real MI355X (csrc/gmr_tracker_adaptive.hip through motion_tracker.py)
against the NumPy statement (tests/adaptive_mirror.py): the plain masked reset bit-equal to ``reset_dev`` on the compacted list, the
failure counts, an Adapt on tens of thousands of bins, 200 steps of adaptive draws bit-equal to the mirror running on the device's own
``cdf``, a link step whose ``fail`` feeds the reset on one stream, and the lifetime of the configuration.  Every test makes one pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_mirror as am  # noqa: E402
import motion_mirror as mm  # noqa: E402
from test_motion_library import _bits, device_library, make_motions  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
STATE = ("clip", "time", "length", "draws")
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def tracker(lib, *a, **k):
    from general_motion_retargeting_amd import MotionTracker
    return MotionTracker(lib, *a, **k)


def assert_same_state(a, b, what=""):
    """two trackers, or a tracker and a mirror: clip, float32 clock, length, draw counters and ignored ids, bit for bit"""
    x, y = a.state(), b.state()
    for k in STATE:
        assert np.array_equal(_bits(x[k]), _bits(y[k])), (k, what)
    assert x["ignored"] == y["ignored"], what


def mask(hip, a):
    return hip.DeviceBuffer.from_host(np.ascontiguousarray(a, dtype=np.int32))


def plain_clip(rng, n, fps, ndof=2):
    return {"fps": fps, "root_pos": rng.normal(size=(n, 3)), "root_rot": np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)), "dof_pos": rng.normal(size=(n, ndof)),
            "local_body_pos": None}


def adopt_cdf(t, m):
    """the mirror takes the device's cdf after an Adapt: last-bit differences of a float64 sum must not decide an integer"""
    st = t.adaptive_state()
    assert st["cdf"][0] == 0.0 and (np.diff(st["cdf"]) >= 0).all()
    assert np.abs(st["cdf"] - m.bin_cdf).max() <= m.bins.Bt * 2.0 ** -51
    m.bin_cdf = st["cdf"].copy()
    return st


# ---- 1. a plain tracker: the masked reset is reset_dev without the list -----------------------------------------------------------------
@pytest.mark.parametrize("loop", [True, False])
def test_plain_masked_reset_is_reset_dev_on_the_compacted_list(hip, loop):
    rng = np.random.default_rng(100 + loop)
    motions = make_motions(rng, [1, 2, 65, 300] + rng.integers(2, 120, size=12).tolist(), 6, 0)
    lib = device_library(hip, motions)
    N = 5000
    w = rng.uniform(0.0, 1.0, size=lib.num_clips)
    w[3] = 0.0
    kw = dict(loop=loop, seed=(5 << 32) | 1234, clip_weights=w)
    a, b = tracker(lib, N, 0.02, **kw), tracker(lib, N, 0.02, **kw)
    m = am.AdaptiveTracker(mm.Library(motions, "world"), N, 0.02, **kw)
    st = hip.Stream()
    for frac, resample, rng_t in ((1.0, True, (0.0, 0.0)), (0.02, True, (0.25, 3.0)), (0.0, True, (0.0, 1.0)), (0.02, False, (-0.5, 0.5)), (1.0, True, (0.0, 2.0))):
        done = (rng.uniform(size=N) < frac).astype(np.int32) * rng.integers(1, 5, size=N).astype(np.int32)      # any non-zero value is "done"
        failed = rng.integers(0, 2, size=N).astype(np.int32)          # a plain tracker has nowhere to record it
        before = a.state()
        d_done, d_failed = mask(hip, done), mask(hip, failed)
        a.reset_done_dev(done=d_done, failed=d_failed, resample=resample, time_offset_range=rng_t, stream=st)
        ids = np.nonzero(done)[0].astype(np.int32)
        if len(ids):
            d_ids = mask(hip, ids)
            b.reset_dev(len(ids), d_ids, resample=resample, time_offset_range=rng_t, stream=st)
        st.sync()
        m.reset_done(done, failed, resample=resample, time_offset_range=rng_t)
        assert_same_state(a, b, frac)
        assert_same_state(a, m, frac)
        after = a.state()
        idle = done == 0
        for k in STATE:                                   # environments that are not done are untouched and consume no draw
            assert np.array_equal(_bits(after[k][idle]), _bits(before[k][idle])), (k, frac)
        assert (after["draws"][~idle] == before["draws"][~idle] + 1).all()
        for x in (a, b, m):
            x.step()
    # by list, flags by list position, and the host twin; ids outside [0, N) count where the entry is done
    ids = np.array([5, N - 1, -1, N, 17, 4], dtype=np.int32)
    done = np.array([1, 0, 1, 0, 1, 9], dtype=np.int32)
    d_ids, d_done = mask(hip, ids), mask(hip, done)
    a.reset_done_dev(done=d_done, env_ids=d_ids, n=6, time_offset_range=(0.0, 1.0), stream=st)
    st.sync()
    assert b.reset_done(done, None, env_ids=ids, time_offset_range=(0.0, 1.0)) == 1
    assert m.reset_done(done, None, env_ids=ids, time_offset_range=(0.0, 1.0)) == 1
    assert_same_state(a, b, "list")
    assert_same_state(a, m, "list")
    assert a.state()["ignored"] == 1 and not a.state()["adaptive"]
    # done = None: every environment, what reset() does
    assert a.reset_done() == 0 and b.reset() == 0
    assert_same_state(a, b, "all")
    for x in (a, b):
        x.close()


# ---- 2. recording -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", [True, False])
def test_failure_counts_are_the_mirrors(hip, loop):
    rng = np.random.default_rng(200 + loop)
    motions = make_motions(rng, [1, 2, 65, 300, 31, 90, 120, 47], 5, 0)
    lib = device_library(hip, motions)
    N = 3000
    kw = dict(loop=loop, seed=99)
    t = tracker(lib, N, 0.04, **kw)
    m = am.AdaptiveTracker(mm.Library(motions, "world"), N, 0.04, **kw)
    for x in (t, m):
        x.set_adaptive(0.5, alpha=0.3, uniform=0.4, lookahead=3, gamma=0.6)
    assert t.state()["adaptive"]
    first = adopt_cdf(t, m)
    assert np.array_equal(first["bin_start"], m.bins.bin_start) and not first["fail_now"].any() and not first["ema"].any()
    assert np.abs(first["prob"] - m.bins.base).max() <= 4 * EPS
    # clocks all over the clips, past both ends, and a few bad assignments (no bin: never counted)
    clip = rng.integers(0, lib.num_clips, size=N).astype(np.int32)
    time = rng.uniform(-1.0, 12.0, size=N).astype(F)
    clip[:4], time[:4] = [lib.num_clips, -1, 0, 3], [0.5, 0.5, np.nan, np.inf]
    for x in (t, m):
        x.assign(clip, time)
    total = 0
    for s in range(12):
        e = np.arange(N)
        done = ((e * 7 + s * 13) % 5 == 0).astype(np.int32)
        failed = ((e * 3 + s) % 4 != 0).astype(np.int32)              # also set on environments that are not done: not counted
        d_done, d_failed = mask(hip, done), mask(hip, failed)
        t.reset_done_dev(done=d_done, failed=d_failed)
        m.reset_done(done, failed)
        total += int((done != 0).sum())
        for x in (t, m):
            x.step()
    got = t.adaptive_state()
    assert np.array_equal(got["fail_now"], m.fail_now) and 0 < int(m.fail_now.sum()) < total
    assert_same_state(t, m, "scripted")
    # every environment in ONE bin, all of them failing: the count is N
    c, when = 3, F(4.25)
    for x in (t, m):
        x.assign(np.full(N, c), np.full(N, when))
    b = m.bin_of(0)
    before = m.fail_now[b]
    ones = mask(hip, np.ones(N, np.int32))
    t.reset_done_dev(done=ones, failed=ones)
    m.reset_done(np.ones(N, np.int32), np.ones(N, np.int32))
    got = t.adaptive_state()
    assert int(got["fail_now"][b]) == int(before) + N and np.array_equal(got["fail_now"], m.fail_now)
    # failed = None records nothing; the host twin by list
    ids = np.array([9, 2, N + 5, 77], dtype=np.int32)
    assert t.reset_done(env_ids=ids) == 1 and m.reset_done(env_ids=ids) == 1
    assert t.reset_done(done=[1, 0, 1, 1], failed=[1, 1, 1, 0], env_ids=ids) == 1 and m.reset_done([1, 0, 1, 1], [1, 1, 1, 0], env_ids=ids) == 1
    assert np.array_equal(t.adaptive_state()["fail_now"], m.fail_now)
    assert_same_state(t, m, "list")
    # reset() on an adaptive tracker is the plain one: clip weights and the offset range, the bins are not read
    for x in (t, m):
        x.reset(env_ids=np.arange(0, N, 3), time_offset_range=(0.0, 0.3))
    assert_same_state(t, m, "plain reset")
    assert np.array_equal(t.adaptive_state()["fail_now"], m.fail_now)
    t.close()


# ---- 3. Adapt on tens of thousands of bins --------------------------------------------------------------------------------------------------
def test_adapt_on_a_library_of_thousands_of_clips(hip):
    rng = np.random.default_rng(300)
    C = 2300
    lens = rng.integers(1, 1200, size=C)
    lens[:6] = [1, 2, 30, 31, 4095, 64]
    motions = [plain_clip(rng, int(n), float(rng.choice([30.0, 50.0, 120.0, 29.97]))) for n in lens]
    lib = device_library(hip, motions)
    w = rng.uniform(0.1, 1.0, size=C)
    w[rng.choice(C, size=200, replace=False)] = 0.0                   # clips that are never drawn: their bins keep p = 0
    N = 40000
    kw = dict(loop=False, seed=7, clip_weights=w)
    t = tracker(lib, N, 0.02, **kw)
    m = am.AdaptiveTracker(mm.Library(motions, "world"), N, 0.02, **kw)
    params = dict(alpha=0.25, uniform=0.2, lookahead=5, gamma=0.75)
    for x in (t, m):
        x.set_adaptive(0.5, **params)
    Bt = m.bins.Bt
    assert 20000 <= Bt <= 200000, Bt                                  # the scan crosses every boundary: 64-bin chunks, 4096-bin tiles, 64-chunk batches
    adopt_cdf(t, m)
    for rounds in range(3):
        clip = rng.integers(0, C, size=N).astype(np.int32)
        time = rng.uniform(0.0, 30.0, size=N).astype(F)
        hard = rng.choice(C, size=40)                                 # a few clips fail everywhere
        failed = (np.isin(clip, hard) | (rng.uniform(size=N) < 0.05)).astype(np.int32)
        for x in (t, m):
            x.assign(clip, time)
        assert t.reset_done(None, failed) == 0 and m.reset_done(None, failed) == 0
        assert np.array_equal(t.adaptive_state()["fail_now"], m.fail_now) and m.fail_now.sum() > 1000
        if rounds == 1:                                               # new parameters for the Adapts to come; the history stays
            params = dict(alpha=0.6, uniform=0.05, lookahead=16, gamma=0.9)
            for x in (t, m):
                x.set_adaptive(0.5, **params)
        t.adapt()
        m.adapt()
        got = t.adaptive_state()
        assert not got["fail_now"].any()
        assert np.array_equal(got["ema"].view(np.uint64), m.ema.view(np.uint64)), rounds
        rel = np.abs(got["prob"] - m.prob) / np.where(m.prob > 0, m.prob, 1.0)
        print(f"round {rounds}: Bt {Bt}, prob rel {rel.max() / EPS:.1f} eps (bound {Bt}), cdf abs {np.abs(got['cdf'] - m.bin_cdf).max() / EPS:.1f} eps (bound {2 * Bt})")
        assert rel.max() <= Bt * EPS and np.array_equal(got["prob"] == 0, m.prob == 0)
        assert np.abs(got["cdf"] - m.bin_cdf).max() <= Bt * 2.0 ** -51
        assert got["cdf"][0] == 0.0 and (np.diff(got["cdf"]) >= 0).all()
        zero = np.nonzero(got["prob"][:-1] == 0)[0]
        assert len(zero) > 1000 and np.array_equal(got["cdf"][zero + 1], got["cdf"][zero])      # a bin of p = 0 has an empty interval
        assert np.abs(got["clip_prob"] - np.bincount(m.bins.clip, weights=m.prob, minlength=C)).max() <= Bt * EPS
        assert not got["clip_prob"][w == 0].any() and abs(got["clip_prob"].sum() - 1.0) <= Bt * EPS
        adopt_cdf(t, m)
        # and the draws that follow are the mirror's on that cdf: no clip of weight zero among them
        assert t.reset_done() == 0 and m.reset_done() == 0
        assert_same_state(t, m, rounds)
        assert (w[t.state()["clip"]] > 0).all()
    t.close()


# ---- 4. adaptive draws over 200 steps -------------------------------------------------------------------------------------------------------
def run_adaptive(hip, lib, motions, N, steps=200):
    """200 steps with loop off, scripted masks and an Adapt every 40 steps -> the (clip, time bits, draws, finished) history of environment 7"""
    kw = dict(loop=False, seed=(3 << 32) | 21)
    t = tracker(lib, N, 0.05, **kw)
    m = am.AdaptiveTracker(mm.Library(motions, "world"), N, 0.05, **kw)
    for x in (t, m):
        x.set_adaptive(0.4, alpha=0.5, uniform=0.1, lookahead=4, gamma=0.7)
    adopt_cdf(t, m)
    for x in (t, m):
        x.reset_done()
    e = np.arange(N)
    track, finished_total = [], 0
    for s in range(steps):
        out, want = t.step(), m.step()
        assert np.array_equal(out["finished"], want["finished"]), s
        finished_total += int(out["finished"].sum())
        # scripted masks that depend on the environment and the step alone: environment 7 sees the same ones whatever N is
        done = ((e * 5 + s * 3) % 23 == 0).astype(np.int32)
        failed = (((e + s) % 3 != 0) & (e < 64)).astype(np.int32)
        d_done, d_failed = mask(hip, done), mask(hip, failed)
        t.reset_done_dev(done=d_done, failed=d_failed)
        m.reset_done(done, failed)
        if s % 40 == 39:
            assert np.array_equal(t.adaptive_state()["fail_now"], m.fail_now), s
            t.adapt_dev()
            m.adapt()
            st = adopt_cdf(t, m)
            assert np.array_equal(st["ema"].view(np.uint64), m.ema.view(np.uint64)), s
        if s % 10 == 9 or N <= 64:
            assert_same_state(t, m, s)
        st = t.state()
        track.append((int(st["clip"][7]), int(_bits(st["time"])[7]), int(st["draws"][7]), int(out["finished"][7])))
    assert_same_state(t, m, "end")
    assert finished_total > N // 4                    # clips did finish: the redraw from the bins ran
    t.close()
    return track


def test_adaptive_draws_are_the_mirrors_and_do_not_depend_on_the_neighbours(hip):
    rng = np.random.default_rng(400)
    motions = make_motions(rng, rng.integers(20, 160, size=30).tolist() + [1, 2], 4, 0)
    lib = device_library(hip, motions)
    few, many = run_adaptive(hip, lib, motions, 64), run_adaptive(hip, lib, motions, 5000)
    # Only the first 64 environments report failures, and their masks depend on (environment, step) alone: both runs record the same
    # counts, so environment 7 draws from the same distributions and must go through the same sequence among 64 and among 5 000.
    assert few == many
    assert len({x[0] for x in many}) > 3 and many[-1][2] > 10


# ---- 5. a link step on an adaptive tracker ----------------------------------------------------------------------------------------------------
def test_link_step_feeds_the_masked_reset_on_one_stream(hip):
    from test_motion_body_state_host import kinematics
    from test_motion_tracker import random_sim
    from test_tracker_links import random_links
    km = kinematics("unitree_g1")
    rng = np.random.default_rng(500)
    motions = make_motions(rng, [50, 70, 31, 120, 44], km.num_dof, 0)
    lib = device_library(hip, motions)
    N, sel = 700, [12, 4, 33, 20]
    kw = dict(loop=False, seed=8)
    a, b, c = (tracker(lib, N, 0.05, **kw) for _ in range(3))      # a: device loop with links; b: its synchronous twin; c: plain steps
    for x in (a, b, c):
        x.set_adaptive(0.5, alpha=0.5, uniform=0.3, lookahead=3, gamma=0.8)
        x.reset_done()
    for x in (a, b):
        x.set_links(km, bodies=sel)
    ref = b.step_links(advance=False)
    links, sim = random_links(rng, ref, amp=0.1), random_sim(rng, ref)
    md = b.step_links(sim, links, advance=False)["max_dist"]
    for x in (a, b):
        x.set_link_terms(fail_dist=float(np.median(md)))             # about half of the environments fail at the start
    d_links = {k: hip.DeviceBuffer.from_host(v) for k, v in links.items()}
    d_sim = {k: hip.DeviceBuffer.from_host(v) for k, v in sim.items()}
    d_fail, d_fin = mask(hip, np.full(N, -9)), mask(hip, np.full(N, -9))
    st = hip.Stream()
    fails = 0
    for s in range(30):
        # the device loop: fail goes from the link step straight into the reset, nothing comes back to the host in between
        a.step_links_dev(d_sim, d_links, stream=st, fail=d_fail, finished=d_fin)
        a.reset_done_dev(done=d_fail, failed=d_fail, stream=st)
        if s % 10 == 9:
            a.adapt_dev(stream=st)
        out = b.step_links(sim, links)
        fail = out["fail"]
        fails += int(fail.sum())
        b.reset_done(fail, fail)
        plain = c.step()
        assert np.array_equal(plain["finished"], out["finished"]), s
        c.reset_done(fail, fail)
        if s % 10 == 9:
            b.adapt()
            c.adapt()
    st.sync()
    assert fails > N and np.array_equal(d_fail.to_host((N,), np.int32), fail)
    assert_same_state(a, b, "device loop against its synchronous twin")
    assert_same_state(a, c, "link steps against plain steps")
    sa, sb, sc = a.adaptive_state(), b.adaptive_state(), c.adaptive_state()
    for k in ("fail_now", "ema", "prob", "cdf"):
        assert np.array_equal(sa[k], sb[k]) and np.array_equal(sa[k], sc[k]), k
    assert sa["ema"].any()
    for x in (a, b, c):
        x.close()


# ---- 6. lifetime ----------------------------------------------------------------------------------------------------------------------------
def test_parameters_travel_with_the_launch_and_off_is_plain_again(hip):
    rng = np.random.default_rng(600)
    motions = make_motions(rng, [40, 90, 65, 130, 25], 4, 0)
    lib = device_library(hip, motions)
    N = 2000
    kw = dict(loop=False, seed=31, clip_weights=[1.0, 2.0, 0.0, 1.0, 3.0])
    t = tracker(lib, N, 0.05, **kw)
    m = am.AdaptiveTracker(mm.Library(motions, "world"), N, 0.05, **kw)
    sets = (dict(alpha=0.9, uniform=0.5, lookahead=1, gamma=1.0), dict(alpha=0.2, uniform=0.0, lookahead=16, gamma=0.5),
            dict(alpha=0.5, uniform=0.25, lookahead=3, gamma=0.8))
    for x in (t, m):
        x.set_adaptive(0.3, **sets[0])
    adopt_cdf(t, m)
    st = hip.Stream()
    clip, time = rng.integers(0, 5, size=N).astype(np.int32), rng.uniform(0.0, 4.0, size=N).astype(F)
    for x in (t, m):
        x.assign(clip, time)
    failed = (rng.uniform(size=N) < 0.3).astype(np.int32)
    d_failed = mask(hip, failed)
    # three parameter sets enqueued back to back on a stream of its own: every Adapt runs with what it was launched with
    t.reset_done_dev(failed=d_failed, stream=st)
    m.reset_done(None, failed)
    emas = []
    for p in sets:
        t.set_adaptive(0.3, **p)            # the same bins: a host assignment, nothing is synchronised
        t.adapt_dev(stream=st)
        m.set_adaptive(0.3, **p)
        m.adapt()
        emas.append(m.ema.copy())
    st.sync()
    got = t.adaptive_state()
    assert np.array_equal(got["ema"].view(np.uint64), m.ema.view(np.uint64))
    assert not np.array_equal(emas[0], emas[2]) and not got["fail_now"].any()
    rel = np.abs(got["prob"] - m.prob) / np.where(m.prob > 0, m.prob, 1.0)
    assert rel.max() <= m.bins.Bt * EPS
    adopt_cdf(t, m)
    t.reset_done_dev(stream=st)
    st.sync()
    m.reset_done()
    assert_same_state(t, m, "after three Adapts")
    # other bins: everything starts over, synchronously
    for x in (t, m):
        x.set_adaptive(1.0, **sets[2])
    fresh = adopt_cdf(t, m)
    assert not fresh["ema"].any() and len(fresh["prob"]) == m.bins.Bt != len(got["prob"])
    # off: the draws of a plain tracker again, bit for bit -- the mirror without bins is tests/tracker_mirror.py, the statement of the
    # plain tracker (the draw counters travel on: both kinds of draw take one)
    for x in (t, m):
        x.set_adaptive(None)
    assert not t.state()["adaptive"]
    with pytest.raises(ValueError, match="set_adaptive"):
        t.adapt()
    ones = np.ones(N, np.int32)
    d_ones = mask(hip, ones)
    finished = 0
    for step in range(60):
        done = ((np.arange(N) + step) % 17 == 0).astype(np.int32)
        t.reset_done_dev(done=mask(hip, done), failed=d_ones, time_offset_range=(0.0, 0.5), stream=st)
        st.sync()
        m.reset_done(done, ones, time_offset_range=(0.0, 0.5))
        a, b = t.step(), m.step()
        assert np.array_equal(a["finished"], b["finished"])
        finished += int(a["finished"].sum())
        assert (t.state()["time"][a["finished"] == 1] == 0).all()      # a finished clip starts at time 0 again
    assert finished > 100
    assert_same_state(t, m, "off")
    assert t.reset() == 0 and m.reset() == 0
    assert_same_state(t, m, "off, reset")
    t.close()
