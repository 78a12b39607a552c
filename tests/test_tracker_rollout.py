"""The tracker's rollout storage, GAE, returns and normalised advantages on a real MI355X (csrc/gmr_tracker_rollout.hip through
motion_tracker.py): every output of ``record_dev`` and ``advantages_dev``, ``stats`` included, is the statement of
tests/rollout_mirror.py bit for bit, at (H, N, O, P, A) = (1, 37, 5, 0, 3) -- the ``last_values`` branch alone, a partial workgroup, no
privileged observations --, (2, 1, 47, 14, 12) -- two advantages --, (5, 37, 80, 14, 23) and (3, 5000, 4, 2, 2) -- 79 groups: the chain of
the partial sums -- on the four-clip library of test_tracker_control.py, 64 guard words behind every device array; every test makes one
pass."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollout_mirror as rm  # noqa: E402
from test_motion_tracker import tracker  # noqa: E402
from test_tracker_control import G, hip, world  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
DT = 0.02
GAMMA, LAM = 0.995, 0.95
GMR_ERR_ARG = -1
SHAPES = [(1, 37, 5, 0, 3), (2, 1, 47, 14, 12), (5, 37, 80, 14, 23), (3, 5000, 4, 2, 2)]
GUARD = {np.dtype(F): F(-77.25), np.dtype(D): D(-77.25), np.dtype(np.uint8): np.uint8(0xA5), np.dtype(np.int32): np.int32(-7725)}
KEEP = {np.dtype(F): F(-3.5), np.dtype(D): D(-3.5), np.dtype(np.uint8): np.uint8(0x5A)}          # what an array holds before a call


def guarded(a):
    """a device buffer of ``a`` with 64 guard words behind it"""
    from general_motion_retargeting_amd import _lib
    a = np.ascontiguousarray(a)
    return _lib.DeviceBuffer.from_host(np.concatenate([a.reshape(-1), np.full(G, GUARD[a.dtype], a.dtype)]))


def fetch(buf, like):
    """the array back on the host, the guard words checked"""
    raw = buf.to_host(like.size + G, like.dtype)
    assert (raw[like.size:] == GUARD[like.dtype]).all(), "guard"
    return raw[:like.size].reshape(like.shape).copy()


def same(a, b, what):
    """the same bits"""
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def rollout_tracker(world, shape, gamma=GAMMA, lam=LAM):
    H, N, O, P, A = shape
    t = tracker(world["lib"], N, DT, world["map"], np.zeros(23, F), seed=3)
    st = t.set_rollout(H, O, P, A, gamma, lam)
    m = rm.Rollout(H, N, O, P, A, gamma, lam)
    assert st["shapes"] == {k: (None if a is None else a.shape) for k, a in m.io.items()}
    for a in m.io.values():                                         # the arrays hold a pattern, not zeros, before anything is recorded
        if a is not None:
            a[...] = KEEP[a.dtype]
    return t, m


def device_io(m):
    return {k: guarded(a) for k, a in m.io.items() if a is not None}


def fetch_io(d, m):
    return {k: fetch(d[k], m.io[k]) for k in d}


def step_rows(rng, shape, n):
    """what a step hands the rollout: finite rows, the two words as rewards_dev emits them (0 / 1) with other nonzero words among them"""
    H, N, O, P, A = shape
    done = (rng.uniform(size=N) < 0.3).astype(np.int32) * rng.choice(np.array([1, 2, 4, -1, 1 << 30], np.int32), N)
    to = (rng.uniform(size=N) < 0.3).astype(np.int32) * rng.choice(np.array([1, 256, -2], np.int32), N)
    if n == 0:
        done[0], to[0] = 1, 1
    return {"obs": rng.normal(0, 1, (N, O)).astype(F), "priv": rng.normal(0, 1, (N, P)).astype(F) if P else None,
            "actions": rng.normal(0, 1, (N, A)).astype(F), "reward": rng.normal(0.2, 1, N).astype(F), "done": done, "time_outs": to}


def record_dev(t, d, n, rows):
    from general_motion_retargeting_amd import _lib
    up = {k: guarded(a) for k, a in rows.items() if a is not None}
    t.record_dev(n, d, **up)
    _lib.check(_lib.lib().gmr_stream_sync(None))                      # the inputs live until the launch has read them


def advantages_dev(t, d, m, values, last, normalize=True, outputs=("advantages", "returns", "normalized", "stats")):
    """advantages_dev on guarded outputs that hold a pattern -> the outputs on the host"""
    H, N = m.H, m.N
    like = {k: (np.full(4, KEEP[np.dtype(D)], D) if k == "stats" else np.full((H, N), KEEP[np.dtype(F)], F)) for k in outputs}
    out = {k: guarded(a) for k, a in like.items()}
    d_values, d_last = guarded(values), guarded(last)
    t.advantages_dev({k: d[k] for k in ("rewards", "dones", "time_outs")}, d_values, d_last, out, normalize=normalize)
    got = {k: fetch(out[k], like[k]) for k in out}
    fetch(d_values, values)                                           # the inputs are read only
    fetch(d_last, last)
    return got


def values_of(rng, m):
    return rng.normal(0.5, 2.0, (m.H, m.N)).astype(F), rng.normal(0.5, 2.0, m.N).astype(F)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_recorded_rollout_and_two_mini_epochs_are_the_mirrors(hip, world, shape):
    H, N, O, P, A = shape
    rng = np.random.default_rng(300 + H + N)
    t, m = rollout_tracker(world, shape)
    before = t.state()
    d = device_io(m)
    # every slot in the reference's two halves: obs and priv before the step, the rest after it
    for n in range(H):
        rows = step_rows(rng, shape, n)
        first = {k: rows[k] for k in ("obs", "priv")}
        rest = {k: rows[k] for k in ("actions", "reward", "done", "time_outs")}
        record_dev(t, d, n, first)
        m.record(n, **first)
        record_dev(t, d, n, rest)
        m.record(n, **rest)
    got = fetch_io(d, m)
    for k in got:
        same(got[k], m.io[k], ("recorded", k))
    assert set(np.unique(got["dones"])) <= {0, 1} and got["time_outs"][0, 0] == 1 and got["dones"][0, 0] == 1
    flags = m.io["dones"].astype(bool), m.io["time_outs"].astype(bool)
    if N >= 37:
        assert (flags[0] & ~flags[1]).any() and (flags[1] & ~flags[0]).any() and (flags[0] & flags[1]).any() and (~flags[0] & ~flags[1]).any()
    # two mini-epochs on the same arrays: the second overwrites the timed-out rewards again
    for k in range(2):
        values, last = values_of(rng, m)
        out = advantages_dev(t, d, m, values, last)
        want = m.advantages(values, last)
        for name in ("advantages", "returns", "normalized", "stats"):
            same(out[name], want[name], (k, name))
        rewards = fetch(d["rewards"], m.io["rewards"])
        same(rewards, m.io["rewards"], (k, "rewards after the bootstrap"))
        assert (rewards[flags[1]] == values[flags[1]]).all() and np.isfinite(out["stats"]).all()
        assert abs(float(out["normalized"].astype(D).mean())) < 1e-5
    # normalize = 0 leaves normalized and stats as they are, and writes the same advantages and returns
    values, last = values_of(rng, m)
    out = advantages_dev(t, d, m, values, last, normalize=False)
    want = m.advantages(values, last, normalize=False)
    same(out["advantages"], want["advantages"], "advantages, not normalised")
    same(out["returns"], want["returns"], "returns, not normalised")
    assert (out["normalized"] == KEEP[np.dtype(F)]).all() and (out["stats"] == KEEP[np.dtype(D)]).all()
    for k in ("obs", "priv", "actions", "dones", "time_outs"):      # an advantages call writes the rewards alone
        if k in d:
            same(fetch(d[k], m.io[k]), m.io[k], k)
    after = t.state()
    for k in before:
        if isinstance(before[k], np.ndarray):
            assert before[k].tobytes() == after[k].tobytes(), k
        else:
            assert before[k] == after[k], k


def test_only_the_named_slot_is_written_and_an_absent_input_leaves_its_slot(hip, world):
    shape = (5, 37, 80, 14, 23)
    H, N, O, P, A = shape
    rng = np.random.default_rng(17)
    t, m = rollout_tracker(world, shape)
    d = device_io(m)
    for n in (0, H - 1):
        rows = step_rows(rng, shape, n)
        record_dev(t, d, n, rows)
        m.record(n, **rows)
    got = fetch_io(d, m)
    for k in got:
        same(got[k], m.io[k], k)
        assert (got[k][1:H - 1] == KEEP[got[k].dtype]).all(), k      # the slots between keep the pattern
        assert (got[k][0] != KEEP[got[k].dtype]).any() and (got[k][H - 1] != KEEP[got[k].dtype]).any(), k
    # slot 2 with three inputs absent: their slots keep the pattern
    rows = step_rows(rng, shape, 2)
    part = {k: (None if k in ("priv", "reward", "time_outs") else a) for k, a in rows.items()}
    record_dev(t, d, 2, part)
    m.record(2, **part)
    got = fetch_io(d, m)
    for k in got:
        same(got[k], m.io[k], k)
    for k in ("priv", "rewards", "time_outs"):
        assert (got[k][2] == KEEP[got[k].dtype]).all(), k
    for k in ("obs", "actions"):
        same(got[k][2], rows[k], k)
    # nothing at all: no launch, nothing written
    t.record_dev(3, d)
    hip.check(hip.lib().gmr_stream_sync(None))
    for k, a in fetch_io(d, m).items():
        same(a, m.io[k], k)


@pytest.mark.parametrize("shape", [(5, 37, 80, 14, 23), (3, 5000, 4, 2, 2)])
def test_a_call_writes_the_outputs_it_is_given(hip, world, shape):
    """without an advantages array the raw ones pass through the normalised one; stats alone; returns alone -- below and beyond the fold"""
    rng = np.random.default_rng(23 + shape[1])
    t, m = rollout_tracker(world, shape)
    for n in range(m.H):
        m.record(n, **{k: a for k, a in step_rows(rng, shape, n).items() if k not in ("obs", "priv", "actions")})
    d = {k: guarded(m.io[k]) for k in ("rewards", "dones", "time_outs")}
    values, last = values_of(rng, m)
    want = m.advantages(values, last)
    for outputs in (("normalized",), ("stats",), ("returns",), ("normalized", "stats")):
        out = advantages_dev(t, d, m, values, last, outputs=outputs)
        for name in outputs:
            same(out[name], want[name], (outputs, name))
        same(fetch(d["rewards"], m.io["rewards"]), m.io["rewards"], "rewards")


def test_bad_calls_are_refused_by_the_library(hip, world):
    from general_motion_retargeting_amd import _lib
    L = hip.lib()
    t = tracker(world["lib"], 1, DT, world["map"], np.zeros(23, F), seed=3)
    io, out = _lib.RolloutIo(), _lib.RolloutOut()
    held = [np.zeros(64, F) if k in (4, 5) else np.full(64, k + 1.25, F) for k in range(8)]       # (4, 5: the two flag arrays, nothing set)
    bufs = [guarded(a) for a in held]
    for k, b in zip(_lib.ROLLOUT_IO_FIELDS, bufs):
        setattr(io, k, b.ptr.value)
    out.advantages = bufs[6].ptr.value
    src = bufs[7].ptr
    # a call before set_rollout
    assert L.gmr_motion_tracker_record_dev(t.handle, 0, C.byref(io), src, None, None, None, None, None, None) == GMR_ERR_ARG
    assert b"gmr_motion_tracker_set_rollout" in L.gmr_last_error()
    assert L.gmr_motion_tracker_advantages_dev(t.handle, C.byref(io), src, src, C.byref(out), 0, None) == GMR_ERR_ARG
    # a bad configuration
    for args in ((0, 4, 2, 2, GAMMA, LAM), (2, 0, 2, 2, GAMMA, LAM), (2, 4, -1, 2, GAMMA, LAM), (2, 4, 2, 0, GAMMA, LAM), (2, 4, 2, 2, 1.5, LAM),
                 (2, 4, 2, 2, float("nan"), LAM), (2, 4, 2, 2, GAMMA, -0.25), (2, 4, 2, 2, GAMMA, float("inf"))):
        assert L.gmr_motion_tracker_set_rollout(t.handle, *args) == GMR_ERR_ARG, args
    assert L.gmr_motion_tracker_advantages_dev(t.handle, C.byref(io), src, src, C.byref(out), 0, None) == GMR_ERR_ARG      # still not set
    # H = 1, N = 1: slot 1 does not exist, and one advantage has no deviation
    hip.check(L.gmr_motion_tracker_set_rollout(t.handle, 1, 4, 2, 2, GAMMA, LAM))
    assert L.gmr_motion_tracker_record_dev(t.handle, 1, C.byref(io), src, None, None, None, None, None, None) == GMR_ERR_ARG
    assert L.gmr_motion_tracker_record_dev(t.handle, -1, C.byref(io), src, None, None, None, None, None, None) == GMR_ERR_ARG
    assert L.gmr_motion_tracker_advantages_dev(t.handle, C.byref(io), src, src, C.byref(out), 1, None) == GMR_ERR_ARG
    assert b"two advantages" in L.gmr_last_error()
    assert L.gmr_motion_tracker_advantages_dev(t.handle, C.byref(io), src, src, C.byref(out), 2, None) == GMR_ERR_ARG
    hip.check(L.gmr_stream_sync(None))
    for b, a in zip(bufs, held):
        same(fetch(b, a), a, "the refused calls wrote nowhere")
    # the same call without normalize is taken: one advantage, and no other word changes
    hip.check(L.gmr_motion_tracker_advantages_dev(t.handle, C.byref(io), src, src, C.byref(out), 0, None))
    hip.check(L.gmr_stream_sync(None))
    want = rm.advantages(held[3][:1].reshape(1, 1).copy(), np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8), held[7][:1].reshape(1, 1),
                         held[7][:1], GAMMA, LAM, normalize=False)
    held[6][0] = want["advantages"][0, 0]
    assert held[6][0] != F(7.25)
    for b, a in zip(bufs, held):
        same(fetch(b, a), a, "the accepted call")
    # and the Python layer says the same with the method's name
    t._rollout = t._rollout_setup(1, 4, 2, 2, GAMMA, LAM)
    with pytest.raises(ValueError, match="record_dev: slot"):
        t.record_dev(1, {"obs": bufs[0]}, obs=bufs[7])
    with pytest.raises(ValueError, match="advantages_dev: normalize"):
        t.advantages_dev({"rewards": bufs[3], "dones": bufs[4], "time_outs": bufs[5]}, bufs[7], bufs[7], {"advantages": bufs[6]})


def test_the_synchronous_twins_give_the_same_bytes(hip, world):
    shape = (5, 37, 80, 14, 23)
    H, N, O, P, A = shape
    rng = np.random.default_rng(41)
    t, m = rollout_tracker(world, shape)
    io = {k: a.copy() for k, a in m.io.items()}
    io["dones"] = io["dones"].view(np.bool_)                           # a boolean array of the caller's is taken as bytes
    for n in (0, 3):
        rows = step_rows(rng, shape, n)
        if n == 3:
            rows["done"], rows["obs"] = rows["done"] != 0, None        # booleans; an absent input
        t.record(n, io, **rows)
        m.record(n, **rows)
    for k in io:
        assert io[k].tobytes() == m.io[k].tobytes(), k
    values, last = values_of(rng, m)
    for normalize in (True, False):
        out = t.advantages(io, values, last, normalize=normalize)
        want = m.advantages(values, last, normalize=normalize)
        assert set(out) == set(want)
        for k in want:
            same(out[k], want[k], (normalize, k))
        assert io["rewards"].tobytes() == m.io["rewards"].tobytes()
