"""The tracker's PPO loss head on a real MI355X (csrc/gmr_tracker_loss.hip through motion_tracker.py): every output of
``log_prob_dev`` and ``loss_dev`` against a float64 evaluation of the statement of tests/ppo_mirror.py on the same float32 inputs, at
(H, N, A) = (1, 2, 1) -- the smallest case --, (1, 37, 3) -- a partial group --, (5, 37, 23) -- unaligned odd rows across group
boundaries --, (3, 700, 12) -- even A, 33 groups through the fold -- and (1, 4200, 1) -- 66 groups: two blocks of the fold --; the same policy on both
sides at (1, 70000, 1) -- 1094 groups, 18 blocks: more than the fold's sixteen wavefronts take in one round; with as many rows no draw
of two policies keeps every ratio away from the clip interval's ends, the same policy does --, on the four-clip library of test_tracker_control.py, 64 guard words behind every device
array, every output holding a pattern before the call; every test makes one pass."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_mirror as pm  # noqa: E402
from test_motion_tracker import tracker  # noqa: E402
from test_tracker_control import G, hip, world  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
DT = 0.02
EPS32 = float(np.finfo(F).eps)
GMR_ERR_ARG = -1
SHAPES = [(1, 2, 1), (1, 37, 3), (5, 37, 23), (3, 700, 12), (1, 4200, 1)]
# the seed of each shape's inputs, the first of 0, 1, 2, .. for which the mirror holds at least five rows in each of the five regimes and
# no row within the margin of lo or hi (both asserted below, on the mirror, before the device is touched)
SEEDS = {(1, 2, 1): 0, (1, 37, 3): 75, (5, 37, 23): 0, (3, 700, 12): 6, (1, 4200, 1): 8}
LOSS = dict(bound_coef=0.01, entropy_coef=-0.01, desired_kl=0.01, learning_rate=1e-3)
GUARD = {np.dtype(F): F(-77.25), np.dtype(D): D(-77.25)}
KEEP = {np.dtype(F): F(-3.5), np.dtype(D): D(-3.5)}                  # what an output holds before a call
OUTPUTS = ("grad_loc", "grad_logstd", "grad_values", "log_prob", "terms")
# MEASURED[k]: the largest deviation of the FLOAT32 MIRROR from the float64 evaluation of the same statement over SHAPES with the inputs
# below, measured on the CPU, in units of eps32 * max(1, |x|) -- grad_loc: of eps32 * max(1, the largest |entry| of the row) --; the
# bound of the device is four times that.  Never measured from the device.
MEASURED = {"log_prob": 10.290834920480847, "ratio": 24.347130525329316, "grad_loc": 3.0566991358064115, "grad_logstd": 1.115025742299622,
            "grad_values": 0.1621621623635292, "value_loss": 0.14003459815569846, "actor_loss": 0.5153870506037492,
            "bound_loss": 0.07604557275772095, "entropy": 0.23118088059273517, "loss": 0.13946516132496709, "kl_mean": 0.6246731316205114,
            "clip_fraction": 0.0}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
KL_MARGIN = 1e-3                                                      # the KL stays this far, relatively, from both thresholds of the rule
MARGIN = 16.0 * BOUND["ratio"]                                        # no row's ratio within this many units of lo or hi


def make_inputs(shape, seed):
    """drawn as in the CPU check of the weight rule: the old policy a small step away, the actions its samples"""
    H, N, A = shape
    M = H * N
    rng = np.random.default_rng([seed, H, N, A])
    loc = rng.normal(0.0, 0.8, (M, A)).astype(F)
    logstd = rng.normal(-2.0, 0.3, A).astype(F)
    old_loc = (loc + rng.normal(0.0, 0.02, (M, A)).astype(F)).astype(F)
    old_logstd = (logstd + rng.normal(0.0, 0.01, A).astype(F)).astype(F)
    actions = (old_loc + np.exp(old_logstd) * rng.normal(0.0, 1.0, (M, A)).astype(F)).astype(F)
    adv = rng.normal(0.0, 1.0, M).astype(F)
    adv[0], adv[1] = F(0.0), -F(0.0)
    x = {"loc": loc, "logstd": logstd, "actions": actions, "old_log_prob": pm.log_prob(old_loc, old_logstd, actions),
         "values": rng.normal(0.5, 2.0, M).astype(F), "returns": rng.normal(0.5, 2.0, M).astype(F), "advantages": adv, "old_loc": old_loc,
         "old_logstd": old_logstd}
    assert np.signbit(adv[1]) and not np.signbit(adv[0]) and all(np.isfinite(a).all() for a in x.values())
    return x


def units(got, want, unit=None):
    got, want = np.asarray(got, D), np.asarray(want, D)
    unit = EPS32 * np.maximum(1.0, np.abs(want)) if unit is None else unit
    return float((np.abs(got - want) / unit).max())


def deviations(got, ref):
    """the deviation of every output of ``got`` from the float64 evaluation ``ref``, in the units of MEASURED"""
    row = EPS32 * np.maximum(1.0, np.abs(ref["grad_loc"]).max(axis=1, keepdims=True))
    out = {"log_prob": units(got["log_prob"], ref["log_prob"]), "grad_loc": units(got["grad_loc"], ref["grad_loc"], row),
           "grad_logstd": units(got["grad_logstd"], ref["grad_logstd"]), "grad_values": units(got["grad_values"], ref["grad_values"])}
    for i, name in enumerate(pm.TERMS):
        if name != "learning_rate":
            out[name] = units(got["terms"][i], ref["terms"][i])
    return out


@functools.lru_cache(maxsize=None)
def reference(shape):
    """the inputs of a shape, the float32 mirror and the float64 evaluation, made once and never written"""
    x = make_inputs(shape, SEEDS[shape])
    cfg = pm.config(LOSS["bound_coef"], LOSS["entropy_coef"], LOSS["desired_kl"])
    m32 = pm.loss(cfg, LOSS["learning_rate"], **x, update_lr=True)
    m64 = pm.loss(cfg, LOSS["learning_rate"], **x, update_lr=True, dtype=D)
    for a in list(x.values()) + [v for m in (m32, m64) for v in m.values() if isinstance(v, np.ndarray)]:
        a.flags.writeable = False
    return x, cfg, m32, m64


def regimes(shape, m, adv):
    """(rows inside, above with adv > 0, above with adv < 0, below with adv > 0, below with adv < 0), the distance to lo and hi in units"""
    lo, hi = 1.0 - 0.2, 1.0 + 0.2
    ratio = m["ratio"].astype(D)
    inside, above, below = (ratio >= lo) & (ratio <= hi), ratio > hi, ratio < lo
    counts = (int(inside.sum()), int((above & (adv > 0)).sum()), int((above & (adv < 0)).sum()), int((below & (adv > 0)).sum()),
              int((below & (adv < 0)).sum()))
    near = min(float((np.abs(ratio - e) / (EPS32 * np.maximum(1.0, ratio))).min()) for e in (F(lo).astype(D), F(hi).astype(D)))
    return counts, near


def check_inputs(shape):
    """what the comparison rests on, asserted on the mirror before the device is touched: every regime is there, no row is near an edge,
    and the float32 and the float64 evaluation agree on every weight -- so every row is compared"""
    x, cfg, m32, m64 = reference(shape)
    counts, near = regimes(shape, m32, x["advantages"])
    if shape != (1, 2, 1):
        assert min(counts) >= 5, (shape, counts)
    assert near > MARGIN, (shape, near, MARGIN)
    assert (m32["w"] == m64["w"]).all() and units(m32["ratio"], m64["ratio"]) <= MEASURED["ratio"]
    kl = m64["terms"][5]
    assert min(abs(kl / (2 * cfg["desired_kl"]) - 1), abs(kl / (cfg["desired_kl"] / 2) - 1)) > KL_MARGIN      # the rule's branch is not in doubt
    return x, cfg, m32, m64


def guarded(a, front=0):
    """a device buffer of ``a`` with 64 guard words behind it (and ``front`` in front of it)"""
    from general_motion_retargeting_amd import _lib
    a = np.ascontiguousarray(a)
    return _lib.DeviceBuffer.from_host(np.concatenate([np.full(front, GUARD[a.dtype], a.dtype), a.reshape(-1), np.full(G, GUARD[a.dtype], a.dtype)]))


def fetch(buf, like, front=0):
    """the array back on the host, the guard words checked"""
    raw = buf.to_host(front + like.size + G, like.dtype)
    assert (raw[:front] == GUARD[like.dtype]).all() and (raw[front + like.size:] == GUARD[like.dtype]).all(), "guard"
    return raw[front:front + like.size].reshape(like.shape).copy()


def same(a, b, what):
    """the same bits"""
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def loss_tracker(world, shape, **kw):
    H, N, A = shape
    t = tracker(world["lib"], N, DT, world["map"], np.zeros(23, F), seed=3)
    t.set_rollout(H, 4, 0, A, 0.995, 0.95)
    st = t.set_loss(**{**LOSS, **kw})
    assert (st["rows"], st["cols"], st["learning_rate"], st["e_clip"], st["lr_factor"]) == (H * N, A, {**LOSS, **kw}["learning_rate"], 0.2, 1.5)
    return t


def shapes_of(shape):
    H, N, A = shape
    M = H * N
    return {"grad_loc": ((M, A), F), "grad_logstd": ((A,), F), "grad_values": ((M,), F), "log_prob": ((M,), F), "terms": ((8,), D)}


class Call:
    """the device arrays of a shape's inputs, uploaded once per test; ``front`` floats of guard in front of every [M][A] array move it off
    16 bytes"""

    def __init__(self, t, shape, x, front=0):
        self.t, self.shape, self.x, self.front = t, shape, x, front
        self.dev = {k: guarded(a, front if a.ndim == 2 else 0) for k, a in x.items()}

    def address(self, k, buf, like):
        return buf.ptr.value + 4 * self.front if like.ndim == 2 and self.front else buf

    def __call__(self, outputs=OUTPUTS, update_lr=False, old=True):
        """loss_dev with ``outputs`` handed in; all five arrays exist and hold a pattern -> the five arrays on the host"""
        like = {k: np.full(s, KEEP[np.dtype(d)], d) for k, (s, d) in shapes_of(self.shape).items()}
        out = {k: guarded(a, self.front if a.ndim == 2 else 0) for k, a in like.items()}
        inputs = {k: self.address(k, b, self.x[k]) for k, b in self.dev.items() if old or k not in ("old_loc", "old_logstd")}
        self.t.loss_dev(inputs, {k: self.address(k, out[k], like[k]) for k in outputs}, update_lr=update_lr)
        got = {k: fetch(out[k], like[k], self.front if like[k].ndim == 2 else 0) for k in out}
        for k in like:
            if k not in outputs:
                assert (got[k] == KEEP[got[k].dtype]).all(), (k, "an output that was not handed in was written")
        return got

    def inputs_untouched(self):
        for k, b in self.dev.items():
            same(fetch(b, self.x[k], self.front if self.x[k].ndim == 2 else 0), np.asarray(self.x[k]), k)


@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_is_the_statement_within_the_float32_mirrors_own_error(hip, world, shape):
    x, cfg, m32, m64 = check_inputs(shape)
    H, N, A = shape
    M = H * N
    t = loss_tracker(world, shape)
    call = Call(t, shape, x)
    # the log-probability alone, and the old one: the mirror's within the bound
    lp_out = guarded(np.full(M, KEEP[np.dtype(F)], F))
    t.log_prob_dev(call.dev["loc"], call.dev["logstd"], call.dev["actions"], lp_out)
    lp = fetch(lp_out, m32["log_prob"])
    assert units(lp, m64["log_prob"]) <= BOUND["log_prob"]
    # the full call steps the learning rate
    lr0 = LOSS["learning_rate"]
    a = call(update_lr=True)
    same(a["log_prob"], lp, "log_prob of loss_dev and of log_prob_dev")
    dev = deviations(a, m64)
    print(shape, {k: round(v, 4) for k, v in dev.items()})
    for k, v in dev.items():
        assert v <= BOUND[k], (shape, k, v, BOUND[k])
    lr1 = pm.step_lr(cfg, lr0, float(m64["terms"][5]))
    assert a["terms"][6] == lr1 == m32["learning_rate"]              # (lowered at three shapes, kept at (1, 2, 1) and (1, 4200, 1))
    assert t.loss_state()["learning_rate"] == lr1
    # update_lr = 0 leaves the rate alone, and it persists; terms and grad_logstd do not depend on the launch
    b, c = call(), call()
    assert b["terms"][6] == lr1 and t.loss_state()["learning_rate"] == lr1
    for k in OUTPUTS:
        same(b[k], c[k], ("two calls", k))
        if k != "terms":
            same(a[k], b[k], ("with and without update_lr", k))
    same(np.delete(a["terms"], 6), np.delete(b["terms"], 6), "terms with and without update_lr")
    # a second step from the stepped rate
    d = call(outputs=("terms",), update_lr=True)
    assert d["terms"][6] == pm.step_lr(cfg, lr1, float(m64["terms"][5])) == t.loss_state()["learning_rate"]
    call.inputs_untouched()


@pytest.mark.parametrize("shape", [(5, 37, 23), (3, 700, 12)])
def test_a_call_writes_the_outputs_it_is_given_with_the_bits_of_the_full_call(hip, world, shape):
    x, cfg, m32, m64 = check_inputs(shape)
    t = loss_tracker(world, shape)
    call = Call(t, shape, x)
    full = call()
    grad, terms = ("grad_loc", "grad_logstd", "grad_values"), ("terms",)
    for outputs, old in ((grad, True), (terms, True), (OUTPUTS, False), (grad, False), (terms, False), (("grad_loc",), True), (("log_prob",), True),
                         (("grad_values", "log_prob"), False), (("grad_logstd",), True), ((), True)):
        got = call(outputs=outputs, old=old)                          # (checks that the outputs left out keep their pattern)
        for k in outputs:
            if k == "terms" and not old:
                assert got[k][5] == 0.0
                same(np.delete(got[k], 5), np.delete(full[k], 5), (outputs, old, k))
            else:
                same(got[k], full[k], (outputs, old, k))
    assert t.loss_state()["learning_rate"] == LOSS["learning_rate"]
    call.inputs_untouched()


def test_the_same_policy_gives_ratio_one_no_kl_and_the_raised_rate(hip, world):
    shape = (1, 70000, 1)
    H, N, A = shape
    M = H * N
    x = make_inputs(shape, 0)
    t = loss_tracker(world, shape, learning_rate=8e-3)
    lp_out = guarded(np.full(M, KEEP[np.dtype(F)], F))
    first = Call(t, shape, x)
    t.log_prob_dev(first.dev["loc"], first.dev["logstd"], first.dev["actions"], lp_out)
    x.update(old_log_prob=fetch(lp_out, x["old_log_prob"]), old_loc=x["loc"], old_logstd=x["logstd"])
    call = Call(t, shape, x)
    got = call(update_lr=True)
    same(got["log_prob"], x["old_log_prob"], "log_prob")             # ratio = expf(0) = 1 in every row
    adv = x["advantages"].astype(D)
    assert got["terms"][1] == pm.sums(-adv) / D(M)                    # the surrogate is -adv * 1 bit for bit
    dv = x["values"] - x["returns"]
    assert got["terms"][0] == pm.sums((dv * dv).astype(D)) / D(M)     # 18 blocks in the stated order
    assert got["terms"][5] == 0.0 and got["terms"][7] == 0.0          # kl_mean exactly 0, no clipped row
    assert got["terms"][6] == min(1e-2, 8e-3 * 1.5) == 1e-2 == t.loss_state()["learning_rate"]
    again = call(outputs=("terms",), update_lr=True)
    assert again["terms"][6] == 1e-2                                  # lr_max holds
    # w = 1 everywhere: grad_loc and grad_logstd are the float32 mirror's with ratio 1 -- no exp of a row is left in them --, bit for bit
    m32 = pm.loss(pm.config(LOSS["bound_coef"], LOSS["entropy_coef"], LOSS["desired_kl"]), 8e-3, **x)
    assert (m32["ratio"] == 1.0).all() and (m32["w"] == 1.0).all()
    same(got["grad_loc"], m32["grad_loc"], "grad_loc")
    same(got["grad_logstd"], m32["grad_logstd"], "grad_logstd")


def test_arrays_off_16_bytes_take_the_float_path_with_the_same_bits(hip, world):
    shape = (5, 37, 23)
    x, cfg, m32, m64 = check_inputs(shape)
    t = loss_tracker(world, shape)
    aligned, shifted = Call(t, shape, x), Call(t, shape, x, front=1)
    assert shifted.address("loc", shifted.dev["loc"], x["loc"]) % 16 == 4
    want = aligned()
    for outputs, old in ((OUTPUTS, True), (("grad_loc", "terms"), False)):
        got = shifted(outputs=outputs, old=old)
        for k in outputs:
            if k == "terms" and not old:
                same(np.delete(got[k], 5), np.delete(want[k], 5), k)
            else:
                same(got[k], want[k], k)
    M = shape[0] * shape[1]
    lp = guarded(np.full(M, KEEP[np.dtype(F)], F))
    t.log_prob_dev(shifted.address("loc", shifted.dev["loc"], x["loc"]), shifted.dev["logstd"], shifted.address("actions", shifted.dev["actions"], x["actions"]), lp)
    same(fetch(lp, want["log_prob"]), want["log_prob"], "log_prob_dev")
    shifted.inputs_untouched()


def test_the_synchronous_twins_give_the_same_bytes(hip, world):
    shape = (5, 37, 23)
    H, N, A = shape
    x, cfg, m32, m64 = check_inputs(shape)
    t = loss_tracker(world, shape)
    want = Call(t, shape, x)(update_lr=True)
    t2 = loss_tracker(world, shape)
    host = {k: np.array(a) for k, a in x.items()}
    host["actions"] = host["actions"].reshape(H, N, A)                # as the rollout lays it out
    got = t2.loss(host, update_lr=True)
    assert set(got) == set(OUTPUTS)
    for k in OUTPUTS:
        same(got[k], want[k], k)
    same(t2.log_prob(host["loc"], host["logstd"], host["actions"]), want["log_prob"], "log_prob")
    assert t2.loss_state()["learning_rate"] == want["terms"][6]
    nokl = t2.loss({k: v for k, v in host.items() if not k.startswith("old_lo") or k == "old_log_prob"})
    assert nokl["terms"][5] == 0.0 and nokl["terms"][6] == want["terms"][6]
    same(nokl["grad_loc"], want["grad_loc"], "grad_loc without the KL")


def test_bad_calls_are_refused_by_the_library(hip, world):
    from general_motion_retargeting_amd import _lib
    L = hip.lib()
    t = tracker(world["lib"], 3, DT, world["map"], np.zeros(23, F), seed=3)
    good = (0.01, -0.01, 0.01, 1e-3, 0.2, 1e-5, 1e-2, 1.5)
    held = [np.full(64, k + 1.25, F) for k in range(3)] + [np.full(8, 9.5, D)]
    bufs = [guarded(a) for a in held]
    src, dst, terms = bufs[0].ptr, bufs[1].ptr, bufs[3].ptr
    # before set_rollout, and with more columns than the cap
    assert L.gmr_motion_tracker_set_loss(t.handle, *good) == GMR_ERR_ARG and b"gmr_motion_tracker_set_rollout" in L.gmr_last_error()
    hip.check(L.gmr_motion_tracker_set_rollout(t.handle, 2, 4, 0, _lib.LOSS_MAX_ACT + 1, 0.995, 0.95))
    assert L.gmr_motion_tracker_set_loss(t.handle, *good) == GMR_ERR_ARG and b"GMR_LOSS_MAX_ACT" in L.gmr_last_error()
    hip.check(L.gmr_motion_tracker_set_rollout(t.handle, 2, 4, 0, 2, 0.995, 0.95))
    tin, tout = _lib.LossIn(), _lib.LossOut()
    for k in _lib.LOSS_IN_FIELDS[:7]:
        setattr(tin, k, src.value)
    tout.grad_loc, tout.terms = dst.value, terms.value
    # before set_loss
    assert L.gmr_motion_tracker_loss_dev(t.handle, C.byref(tin), C.byref(tout), 0, None) == GMR_ERR_ARG and b"gmr_motion_tracker_set_loss" in L.gmr_last_error()
    assert L.gmr_motion_tracker_log_prob_dev(t.handle, src, src, src, dst, None) == GMR_ERR_ARG
    state = np.zeros(8, D)
    assert L.gmr_motion_tracker_loss_state(t.handle, _lib._ptr(state)) == GMR_ERR_ARG
    # a bad configuration
    nan, inf = float("nan"), float("inf")
    for i, v in ((0, nan), (1, inf), (2, 0.0), (2, nan), (3, 0.0), (3, inf), (4, 0.0), (4, 1.0), (4, nan), (5, 0.0), (5, 2e-2), (6, inf), (7, 0.5), (7, nan)):
        args = list(good)
        args[i] = v
        assert L.gmr_motion_tracker_set_loss(t.handle, *args) == GMR_ERR_ARG, (i, v)
    assert L.gmr_motion_tracker_loss_dev(t.handle, C.byref(tin), C.byref(tout), 0, None) == GMR_ERR_ARG      # still not set
    hip.check(L.gmr_motion_tracker_set_loss(t.handle, *good))
    # update_lr without the old policy, half an old policy, a missing input, a bad flag
    assert L.gmr_motion_tracker_loss_dev(t.handle, C.byref(tin), C.byref(tout), 1, None) == GMR_ERR_ARG and b"update_lr" in L.gmr_last_error()
    assert L.gmr_motion_tracker_loss_dev(t.handle, C.byref(tin), C.byref(tout), 2, None) == GMR_ERR_ARG
    tin.old_loc = src.value
    assert L.gmr_motion_tracker_loss_dev(t.handle, C.byref(tin), C.byref(tout), 0, None) == GMR_ERR_ARG and b"together" in L.gmr_last_error()
    tin.old_loc, tin.returns = None, None
    assert L.gmr_motion_tracker_loss_dev(t.handle, C.byref(tin), C.byref(tout), 0, None) == GMR_ERR_ARG
    tin.returns = src.value
    assert L.gmr_motion_tracker_log_prob_dev(t.handle, src, None, src, dst, None) == GMR_ERR_ARG
    # the rollout set again: the loss no longer fits it
    hip.check(L.gmr_motion_tracker_set_rollout(t.handle, 3, 4, 0, 2, 0.995, 0.95))
    assert L.gmr_motion_tracker_loss_dev(t.handle, C.byref(tin), C.byref(tout), 0, None) == GMR_ERR_ARG and b"set_loss again" in L.gmr_last_error()
    hip.check(L.gmr_stream_sync(None))
    for b, a in zip(bufs, held):
        same(fetch(b, a), a, "the refused calls wrote nowhere")
    # and the accepted call: 9 rows of 2 columns
    hip.check(L.gmr_motion_tracker_set_loss(t.handle, *good))
    hip.check(L.gmr_motion_tracker_loss_dev(t.handle, C.byref(tin), C.byref(tout), 0, None))
    hip.check(L.gmr_stream_sync(None))
    got = fetch(bufs[1], held[1])
    assert (got[:18] != held[1][:18]).all() and (got[18:] == held[1][18:]).all()
    assert fetch(bufs[3], held[3])[6] == 1e-3
    # the Python layer says the same with the method's name
    t._rollout = t._rollout_setup(3, 4, 0, 2, 0.995, 0.95)
    t._loss = t._loss_setup(*good)
    with pytest.raises(ValueError, match="loss_dev: update_lr"):
        t.loss_dev({k: bufs[0] for k in _lib.LOSS_IN_FIELDS[:7]}, {"terms": bufs[3]}, update_lr=True)
