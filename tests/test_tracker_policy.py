"""The tracker's policy block on a real MI355X (csrc/gmr_tracker_policy.hip through motion_tracker.py): ``act_dev`` and
``values_dev`` against a float64 evaluation of the statement of tests/policy_mirror.py on the same float32 inputs.  With T = 32 the row
tile: 1, T - 1, T, T + 1 and 2 T + 3 rows of ``tiny`` -- one input, one hidden layer of 32, one action --, ``odd`` -- five inputs (no multiple
of the eight k of an operand load), two privileged columns, four hidden layers 64, 32, 256, 96, three actions --, ``wide`` -- 512 inputs, no
privileged columns, 32 actions -- and ``model`` -- the reference's model at (O, P, A) = (5, 2, 3) on the fixture's 70 rows, also against the
fixture.  64 guard words behind every device array; every test makes one pass."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_mirror as om  # noqa: E402
import policy_mirror as pol  # noqa: E402
import test_tracker_policy_host as host  # noqa: E402
from test_motion_tracker import tracker  # noqa: E402
from test_tracker_control import G, hip, world  # noqa: E402,F401
from test_tracker_loss import fetch, guarded, same  # noqa: E402
from test_tracker_proprio import GAUSSIAN_BOUND  # noqa: E402  (the gaussian draw against float64: its constant)

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
DT = 0.02
EPS32 = float(np.finfo(F).eps)
T = pol.TILE
SEED = 3
KEEP = F(-3.5)                                                       # what an output holds before a call
ROWS = (1, T - 1, T, T + 1, 2 * T + 3)
# name: (O, P, A, the actor's hidden widths, the critic's, rows of the inputs)
CASES = {"tiny": (1, 0, 1, (32,), (32,), ROWS[-1]), "odd": (5, 2, 3, (64, 32, 256, 96), (64, 32, 256, 96), ROWS[-1]),
         "wide": (512, 0, 32, (256, 128, 128), (32,), ROWS[-1]), "model": pol.GOLDEN_COLS + (pol.ACTOR_HIDDEN, pol.CRITIC_HIDDEN, pol.GOLDEN_ROWS)}
# MEASURED[k]: the largest deviation of the FLOAT32 MIRROR from the float64 evaluation of the same statement over CASES with the inputs
# below (every row, both networks; hidden_l: hidden layer l of either network; actions: one sampling call per case), measured on the CPU, in
# units of eps32 * max(1, |x|); the bound of the device is four times that.  Never measured from the device.
MEASURED = {"loc": 38.887489343993366, "values": 21.04046889487654, "actions": 38.89981472212821, "hidden_0": 36.97692823410034,
            "hidden_1": 75.05559376999736, "hidden_2": 41.08941987971775, "hidden_3": 20.831206876784563}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}


def units(got, want):
    got, want = np.asarray(got, D), np.asarray(want, D)
    return float((np.abs(got - want) / (EPS32 * np.maximum(1.0, np.abs(want)))).max())


def make_inputs(case):
    """-> (params, obs, priv or None): the fixture's for ``model``, drawn otherwise -- weights of about torch's default magnitude, 1.5
    times as wide so that the activations reach both branches of the ELU, logstd about -1"""
    O, P, A, ah, ch, rows = CASES[case]
    if case == "model":
        g = golden()
        return list(host.golden_parameters()), g["obs"], g["priv"]
    rng = np.random.default_rng([20, O, P, A, len(ah)])
    params = []
    for k, shape in enumerate(pol.shapes(O, P, A, ah, ch)):
        if k == 0:
            params.append(rng.normal(-1.0, 0.3, shape).astype(F))
            continue
        fan_in = shape[1] if len(shape) == 2 else pol.shapes(O, P, A, ah, ch)[k - 1][1]
        params.append((rng.normal(0.0, 1.5, shape) / np.sqrt(fan_in)).astype(F))
    return params, rng.normal(0.0, 1.0, (rows, O)).astype(F), rng.normal(0.0, 1.0, (rows, P)).astype(F) if P else None


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(host.GOLDEN, "policy_golden.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def reference(case):
    """the inputs of a case, the float32 mirror and the float64 evaluation -- every row, both networks, one sampling call from count 0 --,
    made once and never written"""
    O, P, A, ah, ch, rows = CASES[case]
    params, obs, priv = make_inputs(case)
    out = {}
    for name, dtype in (("m32", F), ("m64", D)):
        m = pol.Policy(O, P, A, ah, ch, num_envs=rows, seed=SEED, dtype=dtype)
        out[name] = {"act": m.act(params, obs, sample=True), "values": m.values(params, obs, priv)}
    for a in params + [obs] + ([priv] if P else []):
        a.flags.writeable = False
    return params, obs, priv, out["m32"], out["m64"]


def deviations(act, values, ref, rows=None):
    """the deviation of a call's outputs (dicts: loc, actions, hidden; values, hidden) from the float64 evaluation, in the units of MEASURED"""
    r = slice(None, rows)
    out = {}
    if act is not None:
        out["loc"] = units(act["loc"], ref["act"]["loc"][r])
        if act.get("actions") is not None:
            out["actions"] = units(act["actions"], ref["act"]["actions"][r])
    if values is not None:
        out["values"] = units(values["values"], ref["values"]["values"][r])
    for got, want in ((act, ref["act"]), (values, ref["values"])):
        for l, h in enumerate([] if got is None else got.get("hidden") or []):
            if h is not None:
                out[f"hidden_{l}"] = max(out.get(f"hidden_{l}", 0.0), units(h, want["hidden"][l][r]))
    return out


def policy_tracker(world, case, n=None, seed=SEED):
    O, P, A, ah, ch, rows = CASES[case]
    t = tracker(world["lib"], rows if n is None else n, DT, world["map"], np.zeros(23, F), seed=seed)
    t.set_policy(O, P, A, ah, ch)
    return t


class Net:
    """the device arrays of a case: the parameters (``front`` floats of guard in front of each move it 4 ``front`` bytes off 256), the
    inputs, and fresh outputs per call"""

    def __init__(self, t, case, front=0):
        self.t, self.case, self.front = t, case, front
        self.O, self.P, self.A, self.ah, self.ch, self.rows = CASES[case]
        self.params, self.obs, self.priv = reference(case)[:3]
        self.d_params = [guarded(a, front) for a in self.params]
        self.d_obs, self.d_priv = guarded(self.obs), guarded(self.priv) if self.P else None

    def addresses(self):
        return [b.ptr.value + 4 * self.front for b in self.d_params]

    def act(self, rows=None, sample=False, hidden=True, at=0, total=None):
        """one act_dev on rows [at, at + rows) of the inputs -> loc, actions, hidden on the host, [total] rows each: the guards checked
        and the rows the call does not own still KEEP"""
        rows = self.rows if rows is None else rows
        total = rows if total is None else total
        want = [hidden] * len(self.ah) if isinstance(hidden, bool) else list(hidden)
        like = {"loc": np.full((total, self.A), KEEP, F), "actions": np.full((total, self.A), KEEP, F)}
        like.update({f"hidden_{l}": np.full((total, h), KEEP, F) for l, h in enumerate(self.ah) if want[l]})
        bufs = {k: guarded(a) for k, a in like.items()}
        self.t.act_dev(self.addresses(), self.d_obs.ptr.value + 4 * at * self.O, bufs["loc"], bufs["actions"] if sample else None,
                       hidden=[bufs.get(f"hidden_{l}") for l in range(len(self.ah))] if any(want) else None, sample=sample, rows=rows)
        got = {k: fetch(bufs[k], like[k]) for k in bufs}
        for k, a in got.items():
            assert (a[rows:] == KEEP).all() and (sample or k != "actions" or (a == KEEP).all()), (k, "written beyond its rows")
        return {"loc": got["loc"][:rows], "actions": got["actions"][:rows] if sample else None,
                "hidden": [got[f"hidden_{l}"][:rows] if want[l] else None for l in range(len(self.ah))]}

    def values(self, rows=None, hidden=True, at=0, total=None):
        rows = self.rows if rows is None else rows
        total = rows if total is None else total
        want = [hidden] * len(self.ch) if isinstance(hidden, bool) else list(hidden)
        like = {"values": np.full(total, KEEP, F)}
        like.update({f"hidden_{l}": np.full((total, h), KEEP, F) for l, h in enumerate(self.ch) if want[l]})
        bufs = {k: guarded(a) for k, a in like.items()}
        self.t.values_dev(self.addresses(), self.d_obs.ptr.value + 4 * at * self.O, self.d_priv.ptr.value + 4 * at * self.P if self.P else None, bufs["values"],
                          hidden=[bufs.get(f"hidden_{l}") for l in range(len(self.ch))] if any(want) else None, rows=rows)
        got = {k: fetch(bufs[k], like[k]) for k in bufs}
        for k, a in got.items():
            assert (a[rows:] == KEEP).all(), (k, "written beyond its rows")
        return {"values": got["values"][:rows], "hidden": [got[f"hidden_{l}"][:rows] if want[l] else None for l in range(len(self.ch))]}

    def inputs_untouched(self):
        for b, a in zip(self.d_params, self.params):
            same(fetch(b, a, self.front), np.asarray(a), "a parameter was written")
        same(fetch(self.d_obs, self.obs), np.asarray(self.obs), "obs was written")
        if self.P:
            same(fetch(self.d_priv, self.priv), np.asarray(self.priv), "priv was written")


def same_call(a, b, what):
    for k in a:
        for i, (x, y) in enumerate(zip(a[k], b[k]) if k == "hidden" else [(a[k], b[k])]):
            if x is not None and y is not None:
                same(x, y, (what, k, i))


def test_the_float32_mirror_stays_within_what_was_measured():
    """the yardstick's own error, on the CPU: the bound of the device rests on it"""
    worst = {k: 0.0 for k in MEASURED}
    for case in CASES:
        params, obs, priv, m32, m64 = reference(case)
        for k, v in deviations(m32["act"], m32["values"], m64).items():
            worst[k] = max(worst[k], v)
        for net in ("act", "values"):                                # both branches of the ELU in every hidden layer
            assert all((h > 0).any() and (h < 0).any() for h in m64[net]["hidden"]), (case, net)
        assert np.abs(m64["act"]["r"]).max() > (1.5 if case == "tiny" else 2.0)
    print({k: (v, MEASURED[k]) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= MEASURED[k], (k, v, MEASURED[k])


@pytest.mark.parametrize("case", list(CASES))
def test_both_networks_are_the_statement_within_the_float32_mirrors_own_error(hip, world, case):
    params, obs, priv, m32, m64 = reference(case)
    net = Net(policy_tracker(world, case), case)
    st = net.t.policy_state()
    assert (st["obs_cols"], st["priv_cols"], st["act_cols"], st["actor_hidden"], st["critic_hidden"], st["tile"]) == CASES[case][:5] + (T,)
    whole = None
    for rows in sorted(set(ROWS) | {net.rows}):
        if rows > net.rows:
            continue
        a, v = net.act(rows, total=net.rows), net.values(rows, total=net.rows)
        dev = deviations(a, v, m64, rows)
        print(case, rows, {k: round(x, 4) for k, x in dev.items()})
        for k, x in dev.items():
            assert x <= BOUND[k], (case, rows, k, x, BOUND[k])
        if rows == net.rows:
            whole = (a, v)
    # the same bits over two runs, and every row the bits of a call of its own
    same_call(whole[0], net.act(), (case, "act, two runs"))
    same_call(whole[1], net.values(), (case, "values, two runs"))
    for r in range(net.rows):
        a, v = net.act(1, at=r), net.values(1, at=r)
        same_call({k: [h[r:r + 1] for h in x] if k == "hidden" else (None if x is None else x[r:r + 1]) for k, x in whole[0].items()}, a, (case, "act, row", r))
        same_call({k: [h[r:r + 1] for h in x] if k == "hidden" else x[r:r + 1] for k, x in whole[1].items()}, v, (case, "values, row", r))
    net.inputs_untouched()
    assert (net.t.policy_state()["counts"] == 0).all()               # sample off touches no count
    if case == "model":                                              # the reference's own numbers, within the host test's bounds
        g, step = golden(), int(golden()["hidden_stride"])
        got = {"loc": units(whole[0]["loc"], g["loc"]), "values": units(whole[1]["values"], g["values"])}
        for name, r in (("actor", whole[0]), ("critic", whole[1])):
            got.update({f"{name}_hidden_{l}": units(h[:, ::step], g[f"{name}_hidden_{l}"]) for l, h in enumerate(r["hidden"])})
        print("against the fixture", {k: round(x, 4) for k, x in got.items()})
        for k, x in got.items():
            assert x <= host.BOUND[k], (k, x, host.BOUND[k])


def test_the_hidden_outputs_change_no_other_output(hip, world):
    net = Net(policy_tracker(world, "odd"), "odd")
    full_a, full_v = net.act(T + 1), net.values(T + 1)
    for want in (False, (True, False, False, True), (False, True, False, False)):
        same_call(full_a, net.act(T + 1, hidden=want), ("act", want))
        same_call(full_v, net.values(T + 1, hidden=want), ("values", want))


def test_weights_four_bytes_off_sixteen_give_the_aligned_bits(hip, world):
    for case in ("model", "wide"):
        aligned, off = Net(policy_tracker(world, case), case), Net(policy_tracker(world, case), case, front=1)
        assert all(p % 16 == 0 for p in aligned.addresses()) and all(p % 16 == 4 for p in off.addresses())
        same_call(aligned.act(T + 1), off.act(T + 1), (case, "act"))
        same_call(aligned.values(T + 1), off.values(T + 1), (case, "values"))
        off.inputs_untouched()


def test_sampled_actions(hip, world):
    case = "odd"
    params, obs, priv, m32, m64 = reference(case)
    N, A = CASES[case][5], CASES[case][2]
    net = Net(policy_tracker(world, case), case)
    first = net.act(sample=True)
    dev = deviations(first, None, m64)
    print("sampled", {k: round(x, 4) for k, x in dev.items()})
    for k, x in dev.items():
        assert x <= BOUND[k], (k, x, BOUND[k])
    # the draw itself, as the proprio test measures its gaussian noise: against the float64 evaluation of the same words, in units of
    # b max(1, |r|), b = exp(logstd) the deviation
    b = np.exp(np.asarray(params[0], D))[None, :]
    r = m64["act"]["r"]
    worst = float((np.abs((first["actions"].astype(D) - first["loc"].astype(D)) - b * r) / (b * np.maximum(1.0, np.abs(r)))).max())
    print(f"gaussian draws: largest deviation from float64 {worst:.3e} of b max(1, |r|) (bound {GAUSSIAN_BOUND})")
    assert worst <= GAUSSIAN_BOUND and np.abs(r).max() > 2.0
    assert (net.t.policy_state()["counts"] == 1).all()
    # the next call draws again; sample off leaves counts and actions alone
    second = net.act(sample=True)
    same(second["loc"], first["loc"], "loc")
    assert (net.t.policy_state()["counts"] == 2).all() and (second["actions"] != first["actions"]).all()
    m = pol.Policy(*CASES[case][:5], num_envs=N, seed=SEED, dtype=D)
    m.counts += np.uint32(1)
    assert units(second["actions"], m.act(params, obs)["actions"]) <= BOUND["actions"]
    net.act(sample=False)
    net.act(5, sample=False)
    assert (net.t.policy_state()["counts"] == 2).all()
    # the same seed: the same bits; another seed: other bits
    same_call(Net(policy_tracker(world, case), case).act(sample=True), first, "two trackers, one seed")
    other = Net(policy_tracker(world, case, seed=SEED + 1), case).act(sample=True)
    same(other["loc"], first["loc"], "loc")
    assert (other["actions"] != first["actions"]).all()
    # set_policy again zeroes the counts
    net.t.set_policy(*CASES[case][:5])
    assert (net.t.policy_state()["counts"] == 0).all()
    same_call(net.act(sample=True), first, "after set_policy again")
    # two environments with equal obs get different actions; fewer environments than a tile
    t = tracker(world["lib"], 7, DT, world["map"], np.zeros(23, F), seed=SEED)
    t.set_policy(*CASES[case][:5])
    d_params = [guarded(a) for a in params]
    d_obs, loc, act = guarded(np.repeat(obs[:1], 7, axis=0)), guarded(np.zeros((7, A), F)), guarded(np.zeros((7, A), F))
    t.act_dev(d_params, d_obs, loc, act)
    loc, act = fetch(loc, np.zeros((7, A), F)), fetch(act, np.zeros((7, A), F))
    assert (loc == loc[0]).all() and len({row.tobytes() for row in act}) == 7
    same(act[0], first["actions"][0], "environment 0 at count 0: the first call's row")
    with pytest.raises(hip.GmrHipError, match="sampling needs a row per environment"):      # the library refuses it, too
        table = (hip.C.c_void_p * len(d_params))(*(b.ptr.value for b in d_params))
        hip.check(hip.lib().gmr_motion_tracker_act_dev(t.handle, table, 5, d_obs.ptr, guarded(np.zeros((7, A), F)).ptr, guarded(np.zeros((7, A), F)).ptr, None, 1, None))


def test_an_optimizer_step_is_seen_by_the_next_call(hip, world):
    from test_tracker_optim import BOUND as OPT_BOUND
    case = "model"
    params, obs, priv, m32, m64 = reference(case)
    sizes = pol.sizes(*CASES[case][:3])
    net = Net(policy_tracker(world, case), case)
    net.t.set_optimizer(sizes, learning_rate=1e-2)
    rng = np.random.default_rng(9)
    grads = [rng.normal(0.0, 1.0, p.shape).astype(F) for p in params]
    before_a, before_v = net.act(hidden=False), net.values(hidden=False)
    net.t.optimizer_step_dev(net.addresses(), [guarded(g) for g in grads])           # the very list, and no further call
    after_a, after_v = net.act(hidden=False), net.values(hidden=False)
    stepped = [fetch(b, a) for b, a in zip(net.d_params, params)]
    want, _ = om.Optimizer(sizes, dtype=D).step(params, grads, 1e-2)
    assert max(units(x, y) for x, y in zip(stepped, want)) <= OPT_BOUND["param"]
    m = pol.Policy(*CASES[case][:5], num_envs=net.rows, dtype=D)
    assert units(after_a["loc"], m.act(stepped, obs, sample=False)["loc"]) <= BOUND["loc"]
    assert units(after_v["values"], m.values(stepped, obs, priv)["values"]) <= BOUND["values"]
    assert units(after_a["loc"], m64["act"]["loc"]) > 100 * BOUND["loc"] and units(before_a["loc"], m64["act"]["loc"]) <= BOUND["loc"]
    assert (after_v["values"] != before_v["values"]).any()


def test_the_numpy_twins_give_the_bits_of_the_device_calls(hip, world):
    case = "odd"
    params, obs, priv, m32, m64 = reference(case)
    net = Net(policy_tracker(world, case), case)
    t = policy_tracker(world, case)
    a, v = t.act(params, obs, sample=True, hidden=True), t.values(params, obs, priv, hidden=True)
    same_call(net.act(sample=True), a, "act")
    same_call(net.values(), v, "values")
    assert (t.policy_state()["counts"] == 1).all()
    b = t.act(params, obs[:T + 1], sample=False)
    assert set(b) == {"loc"} and b["loc"].tobytes() == a["loc"][:T + 1].tobytes() and (t.policy_state()["counts"] == 1).all()
    same(t.values(params, obs[:3], priv[:3])["values"], v["values"][:3], "values, three rows")
