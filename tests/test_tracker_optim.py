"""The tracker's optimiser on a real MI355X (csrc/gmr_tracker_optim.hip through motion_tracker.py): three consecutive
``optimizer_step_dev`` calls against a float64 evaluation of the statement of tests/optim_mirror.py on the same float32 inputs, at
K = 1, n = 1 -- the smallest case --; K = 3 with CHUNK - 1, CHUNK and CHUNK + 1 elements -- a tail of three floats, a full chunk, a chunk
of one --; the 17 tensors of the reference's model at (O, P, A) = (5, 2, 3), 152 199 floats, 159 chunks; K = 32 tensors of 5; and one
tensor of 3 CHUNK + 5 whose addresses are 4 bytes off 16: the float path.  The first step's gradients have a total norm of about 0.5
(coef == 1), the other two of about 3 (coef < 1).  64 guard words behind every device array; every test makes one pass."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_mirror as om  # noqa: E402
from test_motion_tracker import tracker  # noqa: E402
from test_tracker_control import G, hip, world  # noqa: E402,F401
from test_tracker_loss import fetch, guarded, same  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
DT = 0.02
EPS32 = float(np.finfo(F).eps)
CH = om.CHUNK
N_ENVS = 5
LR = 1e-3
STEPS = 3
NORMS = (0.5, 3.0, 3.3)                                              # the total norm of each step's gradients: coef == 1, then coef < 1
# the reference's model at (O, P, A) = (5, 2, 3) in the order of model.parameters(): logstd, the critic, the actor (weight, bias)
MODEL = (3, 256 * 7, 256, 256 * 256, 256, 128 * 256, 128, 128, 1, 256 * 5, 256, 128 * 256, 128, 128 * 128, 128, 3 * 128, 3)
CASES = {"one": (1,), "edges": (CH - 1, CH, CH + 1), "model": MODEL, "many": (5,) * 32, "long": (3 * CH + 5,)}
# MEASURED[k]: the largest deviation of the FLOAT32 MIRROR from the float64 evaluation of the same statement over CASES and the three
# steps with the inputs below, measured on the CPU, in units of eps32 * max(1, |x|); the bound of the device is four times that.  Never
# measured from the device.  (The norm needs none: it is a double in both, and the device's must be the mirror's bit for bit.)
MEASURED = {"param": 1.4154700722319864, "exp_avg": 0.06662982632406056, "exp_avg_sq": 0.0008294107319670729, "coef": 0.10525316186249256}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}


def units(got, want):
    got, want = np.asarray(got, D), np.asarray(want, D)
    return float((np.abs(got - want) / (EPS32 * np.maximum(1.0, np.abs(want)))).max())


def make_inputs(sizes, seed=0, zero=()):
    """parameters and the gradients of every step, scaled to the step's total norm (``zero``: steps whose gradient is all zero)"""
    rng = np.random.default_rng([seed, len(sizes), sum(sizes)])
    params = [rng.normal(0.0, 0.5, n).astype(F) for n in sizes]
    steps = []
    for s in range(STEPS):
        g = [rng.normal(0.0, 1.0, n) for n in sizes]
        scale = NORMS[s] / np.sqrt(sum(float((x * x).sum()) for x in g))
        steps.append([np.zeros(n, F) if s in zero else (x * scale).astype(F) for x, n in zip(g, sizes)])
    return params, steps


def run_mirror(sizes, params, steps, dtype, lr=LR):
    """-> per step (params, exp_avg, exp_avg_sq, info), the statement in ``dtype``"""
    opt = om.Optimizer(sizes, dtype=dtype)
    out = []
    for grads in steps:
        params, info = opt.step(params, grads, lr(len(out)) if callable(lr) else lr)
        out.append(([p.copy() for p in params], [m.copy() for m in opt.m], [v.copy() for v in opt.v], info))
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """the inputs of a case, the float32 mirror and the float64 evaluation, made once and never written"""
    sizes = CASES[case]
    params, steps = make_inputs(sizes)
    m32, m64 = run_mirror(sizes, params, steps, F), run_mirror(sizes, params, steps, D)
    for a in params + [g for s in steps for g in s]:
        a.flags.writeable = False
    return sizes, params, steps, m32, m64


def deviations(got, ref):
    """the deviation of one step's outputs from the float64 evaluation, in the units of MEASURED"""
    return {"param": units(np.concatenate(got[0]), np.concatenate(ref[0])), "exp_avg": units(np.concatenate(got[1]), np.concatenate(ref[1])),
            "exp_avg_sq": units(np.concatenate(got[2]), np.concatenate(ref[2])), "coef": units(got[3][1], ref[3][1])}


def optim_tracker(world, sizes, **kw):
    t = tracker(world["lib"], N_ENVS, DT, world["map"], np.zeros(23, F), seed=3)
    t.set_optimizer(sizes, **{"learning_rate": LR, **kw})
    return t


class Run:
    """the device arrays of a case: the parameters (written in place) and every step's gradients, ``front`` floats of guard in front of
    each so that its address is 4 ``front`` bytes off 256"""

    def __init__(self, t, params, steps, front=0):
        self.t, self.params, self.steps, self.front = t, params, steps, front
        self.p = [guarded(a, front) for a in params]
        self.g = [[None if a is None else guarded(a, front) for a in grads] for grads in steps]
        self.info = guarded(np.full(4, -3.5, D))

    def address(self, buf):
        return None if buf is None else (buf.ptr.value + 4 * self.front if self.front else buf)

    def step(self, s):
        """one optimizer_step_dev -> (params, exp_avg, exp_avg_sq, info) on the host, every guard checked"""
        self.t.optimizer_step_dev([self.address(b) for b in self.p], [self.address(b) for b in self.g[s]], info=self.info)
        params = [fetch(b, a, self.front) for b, a in zip(self.p, self.params)]
        st = self.t.optimizer_state()
        info = fetch(self.info, np.zeros(4, D))
        assert st["step"] == info[3]
        return params, st["exp_avg"], st["exp_avg_sq"], info

    def gradients_untouched(self):
        for bufs, grads in zip(self.g, self.steps):
            for b, a in zip(bufs, grads):
                if a is not None:
                    same(fetch(b, a, self.front), np.asarray(a), "a gradient was written")


def same_step(a, b, what):
    for i, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
        for k, (x, y) in enumerate(zip(a[i], b[i])):
            same(np.asarray(x), np.asarray(y), (what, name, k))
    same(a[3], b[3], (what, "info"))


def test_the_float32_mirror_stays_within_what_was_measured():
    """the yardstick's own error, on the CPU: the bound of the device rests on it"""
    worst = {k: 0.0 for k in MEASURED}
    for case in CASES:
        sizes, params, steps, m32, m64 = reference(case)
        for s in range(STEPS):
            assert m32[s][3][0] == m64[s][3][0]                      # the norm is the same double in both
            for k, v in deviations(m32[s], m64[s]).items():
                worst[k] = max(worst[k], v)
        assert m32[0][3][1] == 1.0 and m32[1][3][1] < 1.0 and m32[2][3][1] < 1.0, case
    print({k: (v, MEASURED[k]) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= MEASURED[k], (k, v, MEASURED[k])


@pytest.mark.parametrize("case", list(CASES))
def test_three_steps_are_the_statement_within_the_float32_mirrors_own_error(hip, world, case):
    sizes, params, steps, m32, m64 = reference(case)
    front = 1 if case == "long" else 0                               # 4 bytes off 16: the float path
    runs = [Run(optim_tracker(world, sizes), params, steps, front) for _ in range(2)]
    for s in range(STEPS):
        got = runs[0].step(s)
        dev = deviations(got, m64[s])
        equal = all(np.asarray(x).tobytes() == y.tobytes() for i in range(3) for x, y in zip(got[i], m32[s][i]))
        print(case, s, {k: round(v, 4) for k, v in dev.items()}, "the float32 mirror's bits" if equal else "not the float32 mirror's bits")
        for k, v in dev.items():
            assert v <= BOUND[k], (case, s, k, v, BOUND[k])
        # the norm is the mirror's double bit for bit; coef, the rate and the step count
        assert got[3][0] == m32[s][3][0], (case, s, got[3][0], m32[s][3][0])
        assert got[3][1] == m32[s][3][1] and (got[3][1] == 1.0) == (s == 0)
        assert got[3][2] == LR and got[3][3] == s + 1
        same_step(got, runs[1].step(s), (case, s, "two identical runs"))
    runs[0].gradients_untouched()
    if case == "long":                                               # the aligned call gives the float path's bits
        aligned = Run(optim_tracker(world, sizes), params, steps)
        assert all(b.ptr.value % 16 == 0 for b in aligned.p + aligned.g[0]) and all(runs[0].address(b) % 16 == 4 for b in runs[0].p + runs[0].g[0])
        for s in range(STEPS):
            last = aligned.step(s)
        same_step(got, last, "aligned and 4 bytes off")


def test_missing_gradients_leave_their_tensors_and_state_alone(hip, world):
    sizes = (CH + 1, 7, 300, 5)
    params, steps = make_inputs(sizes, seed=1)
    steps[1][1] = steps[1][3] = None
    run = Run(optim_tracker(world, sizes), params, steps)
    a = run.step(0)
    b = run.step(1)
    for k in (1, 3):
        for i in range(3):
            same(np.asarray(a[i][k]), np.asarray(b[i][k]), ("a skipped tensor", i, k))
        assert a[1][k].any() and a[2][k].any()                       # (its state was alive)
    assert b[3][0] == om.total_norm(steps[1]) != om.total_norm([steps[1][0], np.zeros(7, F) + 1, steps[1][2], None])
    # the others moved as the mirror's do
    opt = om.Optimizer(sizes)
    want, _ = opt.step(params, steps[0], LR)
    want, info = opt.step(want, steps[1], LR)
    m64 = run_mirror(sizes, params, steps[:2], D)
    assert deviations(b, m64[1])["param"] <= BOUND["param"] and b[3][0] == info[0] and b[3][1] == info[1]
    run.gradients_untouched()


def test_an_all_zero_gradient_has_norm_zero_and_coef_one(hip, world):
    sizes = (CH + 3, 9)
    params, steps = make_inputs(sizes, seed=2, zero=(0,))
    run = Run(optim_tracker(world, sizes), params, steps)
    got = run.step(0)
    assert got[3][0] == 0.0 and got[3][1] == 1.0 and got[3][3] == 1
    for k in range(2):
        same(got[0][k], params[k], "parameters under a zero gradient")
        assert not got[1][k].any() and not got[2][k].any()


def test_the_rate_follows_the_loss_block_one_step_behind(hip, world):
    """INTEGRATION's order: loss_dev(update_lr=True), then the step -- the step runs at the rate the rule left BEFORE this mini-epoch"""
    import ppo_mirror as pm
    H, A = 1, 3
    M = H * N_ENVS
    sizes = (7, A)
    rng = np.random.default_rng(4)
    loc, logstd = rng.normal(0, 0.8, (M, A)).astype(F), rng.normal(-2.0, 0.3, A).astype(F)
    actions = (loc + np.exp(logstd) * rng.normal(0, 1, (M, A)).astype(F)).astype(F)
    x = {"loc": loc, "logstd": logstd, "actions": actions, "old_log_prob": pm.log_prob(loc, logstd, actions), "values": rng.normal(0, 1, M).astype(F),
         "returns": rng.normal(0, 1, M).astype(F), "advantages": rng.normal(0, 1, M).astype(F), "old_loc": loc, "old_logstd": logstd}
    params, steps = make_inputs(sizes, seed=3)
    infos = {}
    for mode, rate in (("follow", None), ("fixed", 2e-4)):
        t = tracker(world["lib"], N_ENVS, DT, world["map"], np.zeros(23, F), seed=3)
        t.set_rollout(H, 4, 0, A, 0.995, 0.95)
        t.set_loss(bound_coef=0.01, entropy_coef=-0.01, desired_kl=0.01, learning_rate=LR)
        t.set_optimizer(sizes, learning_rate=rate)
        dev = {k: guarded(a) for k, a in x.items()}
        terms = guarded(np.zeros(8, D))
        run = Run(t, params, steps)
        t.loss_dev(dev, {"terms": terms}, update_lr=True)              # the same policy on both sides: kl = 0, the rule raises the rate
        assert fetch(terms, np.zeros(8, D))[6] == LR * 1.5 == t.loss_state()["learning_rate"]
        infos[mode] = [run.step(s) for s in range(2)]
    assert infos["follow"][0][3][2] == LR and infos["follow"][1][3][2] == LR * 1.5
    assert infos["fixed"][0][3][2] == infos["fixed"][1][3][2] == 2e-4
    # and the parameters are the mirror's at those rates
    for mode, lr in (("follow", lambda s: (LR, LR * 1.5)[s]), ("fixed", 2e-4)):
        m64 = run_mirror(sizes, params, steps[:2], D, lr=lr)
        for s in range(2):
            assert deviations(infos[mode][s], m64[s])["param"] <= BOUND["param"], (mode, s)
    with pytest.raises(hip.GmrHipError, match="follow"):                # the library refuses follow mode without the loss, too
        t2 = tracker(world["lib"], N_ENVS, DT, world["map"], np.zeros(23, F), seed=3)
        n = np.array(sizes, np.int64)
        hip.check(hip.lib().gmr_motion_tracker_set_optimizer(t2.handle, 2, hip._ptr(n), float("nan"), 0.9, 0.999, 1e-8, 1.0))


def test_a_saved_state_continues_with_the_same_bits(hip, world):
    sizes, params, steps, m32, m64 = reference("edges")
    whole = Run(optim_tracker(world, sizes), params, steps)
    for s in range(STEPS):
        last = whole.step(s)
    first = Run(optim_tracker(world, sizes), params, steps)
    for s in range(STEPS - 1):
        mid = first.step(s)
    state = first.t.optimizer_state()
    assert state["step"] == STEPS - 1 and [len(a) for a in state["exp_avg"]] == list(sizes)
    t = optim_tracker(world, sizes)
    t.load_optimizer_state(state)
    back = t.optimizer_state()
    assert back["step"] == state["step"] and all(a.tobytes() == b.tobytes() for k in ("exp_avg", "exp_avg_sq") for a, b in zip(back[k], state[k]))
    second = Run(t, mid[0], steps)
    same_step(second.step(STEPS - 1), last, "the continued run")
    # the library's own range checks
    n = np.array(sizes, np.int64)
    for args in ((0, n, LR, 0.9, 0.999, 1e-8, 1.0), (33, n, LR, 0.9, 0.999, 1e-8, 1.0), (3, n, -LR, 0.9, 0.999, 1e-8, 1.0), (3, n, LR, 1.0, 0.999, 1e-8, 1.0),
                 (3, n, LR, 0.9, -0.5, 1e-8, 1.0), (3, n, LR, 0.9, 0.999, 0.0, 1.0), (3, n, LR, 0.9, 0.999, 1e-8, float("inf")),
                 (3, np.array([4, 0, 3], np.int64), LR, 0.9, 0.999, 1e-8, 1.0)):
        assert hip.lib().gmr_motion_tracker_set_optimizer(t.handle, args[0], hip._ptr(args[1]), *args[2:]) == -1, args
    t.close()
    assert t.optimizer_state() is None


def test_the_numpy_twin_gives_the_bits_of_the_device_call(hip, world):
    sizes, params, steps, m32, m64 = reference("edges")
    steps = [list(g) for g in steps]
    steps[1][1] = None
    dev = Run(optim_tracker(world, sizes), params, steps)
    t = optim_tracker(world, sizes)
    p = params
    for s in range(STEPS):
        want = dev.step(s)
        before = [a.copy() for a in p]
        new, info = t.optimizer_step(p, steps[s])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(p, before))      # the arrays handed in are not written
        st = t.optimizer_state()
        same_step((new, st["exp_avg"], st["exp_avg_sq"], info), want, ("the NumPy twin", s))
        p = new
