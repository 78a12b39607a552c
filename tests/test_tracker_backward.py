"""The tracker's backward pass through the two networks on a real MI355X (csrc/gmr_tracker_policy_bwd.hip through motion_tracker.py, DESIGN.md
section 6za): ``act_backward_dev`` and ``values_backward_dev`` against a float64 evaluation of the statement of tests/policy_bwd_mirror.py
on the same float32 inputs.  The four networks of ``test_tracker_policy.CASES`` at 1, T - 1, T, T + 1 and 2 T + 3 rows (T = 32, the tile of
the sweep), ``tiny`` and ``odd`` also at C - 1, C, C + 1 and 2 C + 3 rows (C = 256, the row chunk of the weight gradients); ``model`` also on
the fixture's 70 rows against torch's autograd.  The inputs of a call -- parameters, obs, priv, the hidden activations (the float32 mirror's
forward) and the output gradient, N(0, 1) / rows -- are float32 arrays; 64 guard words behind every device array; every test makes one pass."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_bwd_mirror as bwd  # noqa: E402
import policy_mirror as pol  # noqa: E402
import test_tracker_backward_host as host  # noqa: E402
import test_tracker_policy as tp  # noqa: E402
from test_tracker_control import G, hip, world  # noqa: E402,F401
from test_tracker_loss import fetch, guarded, same  # noqa: E402
from test_tracker_policy import CASES, policy_tracker  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
T, CH = pol.TILE, bwd.CHUNK
ROWS = (1, T - 1, T, T + 1, 2 * T + 3)
BIG = (CH - 1, CH, CH + 1, 2 * CH + 3)
EXTRA = 5                                                            # rows of NaN behind the rows of a call
PATTERN = F(-7.25)                                                   # what a gradient holds before a call
# MEASURED[k]: the largest deviation of the FLOAT32 MIRROR from the float64 evaluation of the same statement over the cases and row counts
# of rows_of() with the inputs below (both networks; delta_l: hidden layer l of either network), measured on the CPU, in units of eps32 *
# the tensor's largest magnitude; the bound of the device is four times that.  Never measured from the device.
MEASURED = {"delta_0": 5.108705155271758, "delta_1": 5.496358165855995, "delta_2": 3.647510704721876, "delta_3": 0.7831086610954895,
            "dW": 17.8427937777556, "db": 13.847819397750742}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
units = host.units


def rows_of(case):
    return ROWS + (BIG if case in ("tiny", "odd") else ()) + ((pol.GOLDEN_ROWS,) if case == "model" else ())


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> params, obs, priv or None, {"actor": hidden, "critic": hidden}, z_loc, z_values: the parameters of the forward test's case, as
    many rows as the largest call of the case takes (``model``: the fixture's 70), the float32 mirror's activations and standard normal
    draws for the output gradients; made once and never written"""
    O, P, A, ah, ch, _ = CASES[case]
    params = tp.reference(case)[0]
    total = max(rows_of(case))
    rng = np.random.default_rng([30, O, P, A, len(ah)])
    if case == "model":
        g = host.golden()
        obs, priv = g["obs"], g["priv"]
    else:
        obs, priv = rng.normal(0.0, 1.0, (total, O)).astype(F), rng.normal(0.0, 1.0, (total, P)).astype(F) if P else None
    m = pol.Policy(O, P, A, ah, ch, num_envs=total)
    hidden = {"actor": m.act(params, obs, sample=False)["hidden"], "critic": m.values(params, obs, priv)["hidden"]}
    z_loc, z_values = rng.normal(0.0, 1.0, (total, A)), rng.normal(0.0, 1.0, total)
    for a in [obs, z_loc, z_values] + ([priv] if P else []) + hidden["actor"] + hidden["critic"]:
        a.flags.writeable = False
    return params, obs, priv, hidden, z_loc, z_values


def upstream(case, rows, fixture=False):
    """g_L of a call: N(0, 1) / rows, or the fixture's"""
    if fixture:
        g = host.golden()
        return g["g_loc"], g["g_values"]
    z_loc, z_values = inputs(case)[4:]
    return (z_loc[:rows] / rows).astype(F), (z_values[:rows] / rows).astype(F)


@functools.lru_cache(maxsize=None)
def reference(case, rows, dtype, fixture=False):
    """the statement on the first ``rows`` rows of the case's inputs -> {"actor": .., "critic": ..}"""
    O, P, A, ah, ch, _ = CASES[case]
    params, obs, priv, hidden, _, _ = inputs(case)
    g_loc, g_values = upstream(case, rows, fixture)
    B = bwd.Backward(pol.Policy(O, P, A, ah, ch, num_envs=rows, dtype=dtype))
    return {"actor": B.act(params, obs[:rows], [h[:rows] for h in hidden["actor"]], g_loc),
            "critic": B.values(params, obs[:rows], priv[:rows] if P else None, [h[:rows] for h in hidden["critic"]], g_values)}


def deviations(got, want):
    """``got``, ``want``: {"delta", "dW", "db"} of one network -> the deviations in the units of MEASURED"""
    out = {"dW": max(units(x, y) for x, y in zip(got["dW"], want["dW"])), "db": max(units(x, y) for x, y in zip(got["db"], want["db"]))}
    for l, (x, y) in enumerate(zip(got["delta"], want["delta"])):
        out[f"delta_{l}"] = units(x, y)
    return out


class Net:
    """the device arrays of a case: parameters, gradients and the inputs of ``total`` rows, NaN in every row beyond ``rows`` of a call;
    ``front`` floats of guard in front of each array move it 4 ``front`` bytes off 256"""

    def __init__(self, t, case, front=0):
        self.t, self.case, self.front = t, case, front
        self.O, self.P, self.A, self.ah, self.ch, _ = CASES[case]
        self.params = inputs(case)[0]
        self.d_params = [guarded(a, front) for a in self.params]
        self.first = {"critic": 1, "actor": 1 + 2 * (len(self.ch) + 1)}

    def addresses(self, bufs):
        return [b.ptr.value + 4 * self.front for b in bufs]

    def call(self, net, rows, extra=0, fill=PATTERN, fixture=False, at=0, of=None):
        """one backward call of ``net`` on rows [at, at + rows) of the inputs of a call of ``of`` rows (default: ``rows``) -> {"delta", "dW",
        "db"}; the arrays hold ``extra`` more rows of NaN; the guards, the inputs and the entries of grads the call does not own are checked"""
        params, obs, priv, hidden, _, _ = inputs(self.case)
        widths = pol.widths(self.O, self.P, self.A, self.ah, self.ch)[net]
        L = len(widths) - 2
        g_out = upstream(self.case, rows if of is None else of, fixture)[0 if net == "actor" else 1]

        def padded(a):
            a = np.asarray(a, F)[at:at + rows]
            return np.concatenate([a, np.full((extra,) + a.shape[1:], np.nan, F)])

        arrays = {"obs": padded(obs), "g": padded(g_out)}
        if net == "critic" and self.P:
            arrays["priv"] = padded(priv)
        for l in range(L):
            arrays[f"hidden_{l}"] = padded(hidden[net][l])
            arrays[f"delta_{l}"] = np.full((rows + extra, widths[l + 1]), np.nan if extra else fill, F)
        bufs = {k: guarded(a, self.front) for k, a in arrays.items()}
        like = [np.full(p.shape, fill, F) for p in params]
        d_grads = [guarded(a, self.front) for a in like]
        ptr = {k: b.ptr.value + 4 * self.front for k, b in bufs.items()}
        hid, dlt = [ptr[f"hidden_{l}"] for l in range(L)], [ptr[f"delta_{l}"] for l in range(L)]
        if net == "actor":
            self.t.act_backward_dev(self.addresses(self.d_params), self.addresses(d_grads), ptr["obs"], hid, ptr["g"], dlt, rows=rows)
        else:
            self.t.values_backward_dev(self.addresses(self.d_params), self.addresses(d_grads), ptr["obs"], ptr.get("priv"), hid, ptr["g"], dlt, rows=rows)
        got = {k: fetch(bufs[k], arrays[k], self.front) for k in bufs}
        for k, a in arrays.items():                                   # the inputs are unchanged, the rows beyond the call untouched
            if not k.startswith("delta"):
                assert got[k].tobytes() == a.tobytes(), (k, "an input was written")
            elif extra:
                assert np.isnan(got[k][rows:]).all(), (k, "written beyond its rows")
        grads = [fetch(b, a, self.front) for b, a in zip(d_grads, like)]
        first = self.first[net]
        own = range(first, first + 2 * (L + 1))
        for k, a in enumerate(grads):
            if k not in own:
                assert (a == fill).all(), (k, "a gradient of the other network or of logstd was written")
        for b, a in zip(self.d_params, params):
            same(fetch(b, a, self.front), np.asarray(a), "a parameter was written")
        return {"delta": [got[f"delta_{l}"][:rows] for l in range(L)], "dW": [grads[first + 2 * l] for l in range(L + 1)],
                "db": [grads[first + 2 * l + 1] for l in range(L + 1)]}


def same_call(a, b, what):
    for k in ("delta", "dW", "db"):
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            same(x, y, (what, k, i))


def backward_tracker(world, case, max_rows=None):
    t = policy_tracker(world, case, n=4)
    st = t.set_backward(max(rows_of(case)) if max_rows is None else max_rows)
    assert st["chunk"] == CH and st["chunks"] == bwd.chunks(st["max_rows"])
    return t


def measure():
    """the float32 mirror against the float64 evaluation over every case and row count -> the figures of MEASURED (CPU only)"""
    worst = {k: 0.0 for k in MEASURED}
    for case in CASES:
        for rows in rows_of(case):
            fixture = case == "model" and rows == pol.GOLDEN_ROWS
            m32, m64 = reference(case, rows, F, fixture), reference(case, rows, D, fixture)
            for net in ("actor", "critic"):
                for k, v in deviations(m32[net], m64[net]).items():
                    worst[k] = max(worst[k], v)
    return worst


def test_the_float32_mirror_stays_within_what_was_measured():
    """the yardstick's own error, on the CPU: the bound of the device rests on it"""
    worst = measure()
    print({k: (v, MEASURED[k]) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= MEASURED[k], (k, v, MEASURED[k])
    for case in CASES:                                                # both branches of the ELU in every hidden layer
        for net in ("actor", "critic"):
            assert all((h > 0).any() and (h < 0).any() for h in inputs(case)[3][net]), (case, net)


@pytest.mark.parametrize("case", list(CASES))
def test_both_networks_are_the_statement_within_the_float32_mirrors_own_error(hip, world, case):
    net = Net(backward_tracker(world, case), case)
    st = net.t.backward_state()
    assert st["max_rows"] == max(rows_of(case)) and st["workspace_bytes"] > 0
    largest = max(rows_of(case))
    whole = {}
    for rows in rows_of(case):
        fixture = case == "model" and rows == pol.GOLDEN_ROWS
        m64 = reference(case, rows, D, fixture)
        for name in ("actor", "critic"):
            got = net.call(name, rows, fixture=fixture)
            dev = deviations(got, m64[name])
            print(case, name, rows, {k: round(x, 4) for k, x in dev.items()})
            for k, x in dev.items():
                assert x <= BOUND[k], (case, name, rows, k, x, BOUND[k])
            if rows == largest:
                whole[name] = got
            if fixture:                                               # torch's autograd through the reference's model, within the host test's bounds
                g = host.golden()
                far = host.against_fixture(got["dW"], got["db"], net.first[name], g)
                print("against the fixture", name, {k: round(x, 4) for k, x in far.items()})
                for k, x in far.items():
                    assert x <= host.BOUND[k[:2]], (k, x, host.BOUND[k[:2]])
    for name in ("actor", "critic"):
        fixture = case == "model"
        # the same bits over two runs; gradients pre-filled with zeros give the bits of those pre-filled with the pattern: overwritten
        same_call(whole[name], net.call(name, largest, fixture=fixture), (case, name, "two runs"))
        same_call(whole[name], net.call(name, largest, fill=F(0.0), fixture=fixture), (case, name, "zeros before the call"))
        # rows beyond the call hold NaN in every array: never read, the gradients finite and the bits of the tight call
        loose = net.call(name, largest, extra=EXTRA, fixture=fixture)
        assert all(np.isfinite(x).all() for k in ("dW", "db", "delta") for x in loose[k])
        same_call(whole[name], loose, (case, name, "NaN beyond the rows"))
        # a delta row of the largest call has the bits of a one-row call on that row
        for r in (0, T - 1, T, largest - 1):
            one = net.call(name, 1, fixture=fixture, at=r, of=largest)
            for l, d in enumerate(one["delta"]):
                same(d, whole[name]["delta"][l][r:r + 1], (case, name, "row", r, "delta", l))


def test_a_shorter_call_on_a_larger_workspace_and_the_chunk_edges(hip, world):
    """max_rows above the rows of a call changes no bit: the association is a function of rows and of the shape alone"""
    case = "odd"
    tight, roomy = Net(backward_tracker(world, case, CH + 1), case), Net(backward_tracker(world, case, 8 * CH), case)
    assert roomy.t.backward_state()["chunks"] == 8
    for name in ("actor", "critic"):
        same_call(tight.call(name, CH + 1), roomy.call(name, CH + 1), name)
        same_call(tight.call(name, T + 1, extra=EXTRA), roomy.call(name, T + 1), name)


def test_arrays_four_bytes_off_sixteen_give_the_aligned_bits(hip, world):
    for case in ("model", "wide"):
        aligned, off = Net(backward_tracker(world, case), case), Net(backward_tracker(world, case), case, front=1)
        assert all(p % 16 == 0 for p in aligned.addresses(aligned.d_params)) and all(p % 16 == 4 for p in off.addresses(off.d_params))
        for name in ("actor", "critic"):
            same_call(aligned.call(name, T + 1), off.call(name, T + 1), (case, name))


def test_the_numpy_twins_give_the_bits_of_the_device_calls(hip, world):
    case = "odd"
    O, P, A, ah, ch, _ = CASES[case]
    params, obs, priv, hidden, _, _ = inputs(case)
    rows = CH + 1
    g_loc, g_values = upstream(case, rows)
    net = Net(backward_tracker(world, case), case)
    t = backward_tracker(world, case)
    a = t.act_backward(params, obs[:rows], [h[:rows] for h in hidden["actor"]], g_loc)
    v = t.values_backward(params, obs[:rows], priv[:rows], [h[:rows] for h in hidden["critic"]], g_values)
    for name, r in (("actor", a), ("critic", v)):
        first, L = net.first[name], len(ah)
        assert sorted(r["grads"]) == list(range(first, first + 2 * (L + 1)))
        twin = {"delta": r["delta"], "dW": [r["grads"][first + 2 * l] for l in range(L + 1)], "db": [r["grads"][first + 2 * l + 1] for l in range(L + 1)]}
        same_call(net.call(name, rows), twin, name)


def test_the_order_of_the_calls(hip, world):
    case = "tiny"
    t = policy_tracker(world, case, n=4)
    assert t.backward_state() is None
    net = Net(t, case)
    with pytest.raises(ValueError, match="call set_backward\\(\\) first"):
        net.call("actor", 3)
    t.set_backward(T)
    net.call("actor", T)
    with pytest.raises(ValueError, match="rows = 33: 1 .. max_rows = 32 are taken"):
        net.call("critic", T + 1)
    # the library refuses both, too
    table = (hip.C.c_void_p * 9)(*net.addresses(net.d_params))
    one = (hip.C.c_void_p * 1)(net.d_params[1].ptr.value)
    with pytest.raises(hip.GmrHipError, match="rows = 33, 1 .. max_rows = 32 are taken"):
        hip.check(hip.lib().gmr_motion_tracker_act_backward_dev(t.handle, table, table, T + 1, net.d_params[1].ptr, one, net.d_params[1].ptr, one, None))
    t.set_policy(*CASES[case][:5])                                   # the very shapes: the plan would still fit, the order is refused all the same
    with pytest.raises(ValueError, match="the policy was set again after the backward pass, call set_backward\\(\\) again"):
        net.call("actor", T)
    t.set_policy(1, 0, 1, (64,), (32,))                              # other shapes: the library's own check
    with pytest.raises(hip.GmrHipError, match="the policy was set again after the backward pass"):
        hip.check(hip.lib().gmr_motion_tracker_act_backward_dev(t.handle, table, table, T, net.d_params[1].ptr, one, net.d_params[1].ptr, one, None))
    t.set_policy(*CASES[case][:5])
    t.set_backward(T)
    net.call("actor", T)
