"""The tracker's policy block without a GPU: the exports, their ctypes signatures and the constants against the
header, every argument check that must fire before the library is loaded, the host's plan of the two networks under plain g++
(tests/cpp/policy_plan_check.cpp), and the NumPy statement (tests/policy_mirror.py) against the fixture recorded by running the reference's
own ``ActorCritic`` in float32 CPU torch (tests/golden/policy_golden.npz, tests/golden/make_policy_golden.py)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header as abi  # noqa: E402
import policy_mirror as pol  # noqa: E402
from test_tracker_proprio_host import offline_tracker  # noqa: E402

SYMBOLS = ("gmr_motion_tracker_set_policy", "gmr_motion_tracker_act_dev", "gmr_motion_tracker_act", "gmr_motion_tracker_values_dev",
           "gmr_motion_tracker_values", "gmr_motion_tracker_policy_state")
F = np.float32
D = np.float64
EPS32 = float(np.finfo(F).eps)
# The mirror cannot be bit-equal to torch: torch's CPU linear sums in the order of its GEMM's blocking with fused multiply-adds, and its ELU
# is a vectorised expm1; the first layer's terms are up to 40 times its result (the observations are scaled by 14).  MEASURED[k] is the largest |mirror - fixture| / (eps32 * max(1, |fixture|)) over the 70 rows of the fixture; the
# bound of each array is four times that (the rule of DESIGN.md sections 6v and 6x).
MEASURED = {"loc": 12.0, "values": 9.223185629453562, "actor_hidden_0": 19.4375, "actor_hidden_1": 22.5, "actor_hidden_2": 21.5, "critic_hidden_0": 36.0,
            "critic_hidden_1": 37.0, "critic_hidden_2": 29.5}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "policy_golden.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def golden_parameters():
    """the parameters of the fixture, rebuilt from the generator's own lines; made once and never written"""
    params = pol.golden_parameters()
    for a in params:
        a.flags.writeable = False
    return tuple(params)


def units(got, want):
    got, want = np.asarray(got, D), np.asarray(want, D)
    return float((np.abs(got - want) / (EPS32 * np.maximum(1.0, np.abs(want)))).max())


def deviations(g, params, obs, priv, n_critic=3):
    """the float32 mirror on the fixture's rows against the fixture, per array, in units"""
    O, P, A = (int(x) for x in g["cols"])
    m = pol.Policy(O, P, A, num_envs=len(obs))
    step = int(g["hidden_stride"])
    a, v = m.act(params, obs, sample=False), m.values(params, obs, priv)
    out = {"loc": units(a["loc"], g["loc"]), "values": units(v["values"], g["values"])}
    for net, r in (("actor", a), ("critic", v)):
        for l, h in enumerate(r["hidden"]):
            assert h.dtype == F
            out[f"{net}_hidden_{l}"] = units(h[:, ::step], g[f"{net}_hidden_{l}"])
    return out


def test_the_library_exports_the_policy_entry_points_with_the_headers_signatures():
    from general_motion_retargeting_amd import _lib, build
    from general_motion_retargeting_amd import motion_tracker as mt
    L = C.CDLL(_lib.LIB_PATH)
    hdr = abi.read()
    assert "N17: tracker policy" in hdr and hdr.index("N17: tracker policy") > hdr.index("N16: tracker optimiser")
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        res, args = _lib._SIGS[sym]
        assert res is C.c_int and args == abi.parameters(hdr, sym), (sym, args)
        m = re.search(r"\bint " + sym + r"\(([^;]*)\);", hdr)
        section = hdr[hdr.index("N17: tracker policy"):m.start()]
        comment = [c for c in re.findall(r"/\*.*?\*/", section, flags=re.S) if "asynchronous" not in c][-1]
        assert re.search(r"model\.py:\d+", comment), sym
    for define, value in (("GMR_POLICY_TILE", _lib.POLICY_TILE), ("GMR_POLICY_MAX_HIDDEN", _lib.POLICY_MAX_HIDDEN), ("GMR_POLICY_WIDTH_STEP", _lib.POLICY_WIDTH_STEP),
                          ("GMR_POLICY_MAX_WIDTH", _lib.POLICY_MAX_WIDTH), ("GMR_POLICY_MAX_IN", _lib.POLICY_MAX_IN), ("GMR_POLICY_MAX_TENSORS", _lib.POLICY_MAX_TENSORS)):
        assert abi.define(hdr, define) == value, define
    assert (_lib.POLICY_TILE, _lib.POLICY_MAX_HIDDEN, _lib.POLICY_WIDTH_STEP, _lib.POLICY_MAX_WIDTH, _lib.POLICY_MAX_IN, _lib.LOSS_MAX_ACT) == \
        (pol.TILE, pol.MAX_HIDDEN, pol.WIDTH_STEP, pol.MAX_WIDTH, pol.MAX_IN, pol.MAX_ACT) == (32, 4, 32, 256, 512, 32)
    assert _lib.POLICY_MAX_TENSORS == 1 + 4 * (_lib.POLICY_MAX_HIDDEN + 1) <= _lib.OPT_MAX_TENSORS          # the list the optimiser takes
    for name in ("set_policy", "act_dev", "act", "values_dev", "values", "policy_state"):
        assert callable(getattr(mt.MotionTracker, name)), name
    assert "gmr_tracker_policy.hip" in build.SOURCES and "gmr_tracker_policy_plan.h" in build.HEADERS
    # the rules of the other blocks hold here: one rounding per operation, no floating-point atomics, no wait for the host behind a launch
    csrc = os.path.join(ROOT, "general_motion_retargeting_amd", "csrc")
    src = open(os.path.join(csrc, "gmr_tracker_policy.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("#include", 1)[1]
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in src
    body = src[src.index("static int policy_launch"):]
    body = body[:body.index("\n}\n")]
    assert "Synchronize" not in body and "hipMemcpy" not in body and "hipMalloc" not in body
    assert body.count("hipLaunchKernelGGL") == 2 and "if (sample) hipLaunchKernelGGL" in body and "else hipLaunchKernelGGL" in body      # ONE launch per call
    # the new counter domain stands next to the other five, and the draw is the tracker's own
    dev = open(os.path.join(csrc, "gmr_tracker_dev.h")).read()
    assert "DRAW_RESET_STATE = 4u, DRAW_ACTION = 5u;" in dev and pol.DRAW_ACTION == 5
    assert "tracker_noise(" in src and "philox4x32(" not in src and "logf(" not in src


def test_the_plan_of_the_two_networks_under_plain_cpp(tmp_path):
    """The stand-alone program, compiled with AddressSanitizer + UBSan where their runtime is installed (the checks of the widths are host
    arithmetic at the edge of int) and plainly where it is not."""
    exe, src = str(tmp_path / "policy_plan_check"), os.path.join(ROOT, "tests", "cpp", "policy_plan_check.cpp")
    cc = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-o", exe, src]
    if subprocess.run(cc + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True).returncode != 0:
        subprocess.check_call(cc)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "ERROR" not in out.stderr, out.stderr[-2000:]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_policy_arguments_are_refused_before_the_library_is_loaded(monkeypatch):
    from general_motion_retargeting_amd import _lib

    def no_device():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    N = 5
    t = offline_tracker(N, 5)
    assert t.policy_state() is None
    for call in (lambda: t.act_dev([1] * 17, 2, 3), lambda: t.values_dev([1] * 17, 2, 3, 4), lambda: t.act([], np.zeros((N, 5), F)),
                 lambda: t.values([], np.zeros((N, 5), F))):
        with pytest.raises(ValueError, match="call set_policy\\(\\) first"):
            call()
    for args, kw, match in (((5, 2, 3), dict(actor_hidden=(256, 100)), r"actor_hidden\[1\] = 100: a multiple of 32 in 32 .. 256"),
                            ((5, 2, 3), dict(critic_hidden=(288,)), r"critic_hidden\[0\] = 288"),
                            ((5, 2, 3), dict(actor_hidden=(0,)), r"actor_hidden\[0\] = 0"),
                            ((5, 2, 3), dict(actor_hidden=(32,) * 5), "actor_hidden names 5 hidden layers, 1 .. 4 are taken"),
                            ((5, 2, 3), dict(critic_hidden=()), "critic_hidden names 0 hidden layers"),
                            ((5, 2, 3), dict(critic_hidden=64), "critic_hidden is a list of widths"),
                            ((5, 2, 33), {}, "act_cols = 33, 1 .. 32 are taken"), ((5, 2, 0), {}, "act_cols = 0"),
                            ((0, 0, 3), {}, "obs_cols = 0 and priv_cols = 0: an input width of 1 .. 512"), ((0, 4, 3), {}, "obs_cols = 0"),
                            ((500, 13, 3), {}, "obs_cols = 500 and priv_cols = 13"), ((513, 0, 3), {}, "obs_cols = 513"), ((5, -1, 3), {}, "obs_cols = 5 and priv_cols = -1")):
        with pytest.raises(ValueError, match="set_policy: " + match):
            t.set_policy(*args, **kw)
    assert t.policy_state() is None
    # the checked configuration: the reference's model at (5, 2, 3) is the 17 tensors the optimiser's test steps
    c = t._policy = t._policy_setup(5, 2, 3, pol.ACTOR_HIDDEN, pol.CRITIC_HIDDEN)
    assert c["sizes"] == pol.sizes(5, 2, 3) == (3, 256 * 7, 256, 256 * 256, 256, 128 * 256, 128, 128, 1, 256 * 5, 256, 128 * 256, 128, 128 * 128, 128, 3 * 128, 3)
    assert c["first"] == {"critic": 1, "actor": 9} and t._policy_setup(512, 0, 32, (32,), (256,) * 4)["sizes"][1] == 256 * 512
    K = len(c["sizes"])
    dev = list(range(1, K + 1))                                      # raw addresses: nothing is dereferenced before the library
    small = _lib.DeviceBuffer.__new__(_lib.DeviceBuffer)
    small.nbytes, small.ptr = 4 * 256 * 7 - 4, None                  # (no allocation: the size alone is looked at)

    class Tensor:
        """what a torch tensor tells about itself"""

        def __init__(self, n, dtype="torch.float32", contiguous=True):
            self.n, self.dtype, self.contiguous = n, dtype, contiguous

        def data_ptr(self):
            return 4096

        def numel(self):
            return self.n

        def is_contiguous(self):
            return self.contiguous

    host = [np.zeros(n, F) for n in c["sizes"]]
    obs, priv = np.zeros((N, 5), F), np.zeros((N, 2), F)
    for call, exc, match in (
            (lambda: t.act_dev(dev[:-1], 2, 3, 4), ValueError, f"act_dev: params names {K - 1} tensors, the policy was set for K = {K}"),
            (lambda: t.values_dev(dev + [9], 2, 3, 4), ValueError, f"values_dev: params names {K + 1} tensors"),
            (lambda: t.act(host[:3], obs), ValueError, "act: params names 3 tensors"),
            (lambda: t.values(host + host, obs, priv), ValueError, f"values: params names {2 * K} tensors"),
            (lambda: t.act_dev(7, 2, 3, 4), ValueError, "params is the list of the model's parameters"),
            (lambda: t.act_dev(dev[:2] + [None] + dev[3:], 2, 3, 4), ValueError, r"params\[2\] is needed"),
            (lambda: t.act_dev([dev[0], small] + dev[2:], 2, 3, 4), ValueError, r"params\[1\]: buffer of 7164 bytes, 7168 needed"),
            (lambda: t.act_dev(dev[:9] + [Tensor(256 * 5, "torch.float64")] + dev[10:], 2, 3, 4), ValueError, r"params\[9\]: dtype torch.float64, float32 needed"),
            (lambda: t.act_dev(dev[:9] + [Tensor(256 * 5, contiguous=False)] + dev[10:], 2, 3, 4), ValueError, r"params\[9\]: not contiguous"),
            (lambda: t.act_dev(dev[:9] + [Tensor(256 * 5 - 1)] + dev[10:], 2, 3, 4), ValueError, r"params\[9\]: 1279 elements, 1280 needed"),
            (lambda: t.act_dev(host, 2, 3, 4), TypeError, "device address"),
            (lambda: t.act(host[:1] + [np.zeros(5, F)] + host[2:], obs), ValueError, r"params\[1\]: 5 elements, 1792 needed"),
            # sampling is per environment
            (lambda: t.act_dev(dev, 2, 3, 4, rows=N + 1), ValueError, f"sample=True draws for the environments.*rows = {N + 1}, num_envs = {N}"),
            (lambda: t.act_dev(dev, 2, 3, 4, rows=1, sample=True), ValueError, "rows = 1, num_envs = 5"),
            (lambda: t.act(host, np.zeros((N - 1, 5), F)), ValueError, "sample=True draws for the environments"),
            (lambda: t.act_dev(dev, 2, 3, None, sample=True), ValueError, "and actions with sample=True"),
            (lambda: t.act_dev(dev, 2, 3, 4, rows=0, sample=False), ValueError, "rows = 0: at least 1"),
            (lambda: t.values_dev(dev, 2, 3, 4, rows=-2), ValueError, "rows = -2"),
            # the arrays of a call
            (lambda: t.act_dev(dev, Tensor(N * 5 - 1), 3, 4), ValueError, "obs: 24 elements, 25 needed"),
            (lambda: t.act_dev(dev, Tensor(N * 5, "torch.float16"), 3, 4), ValueError, "obs: dtype torch.float16"),
            (lambda: t.act_dev(dev, 2, Tensor(N * 3, contiguous=False), 4), ValueError, "loc: not contiguous"),
            (lambda: t.act_dev(dev, 2, 3, Tensor(N * 3 - 1)), ValueError, "actions: 14 elements, 15 needed"),
            (lambda: t.act_dev(dev, 2, 3, sample=False, rows=9, hidden=[Tensor(9 * 256), None, Tensor(9 * 128 - 1)]), ValueError, r"hidden\[2\]: 1151 elements, 1152"),
            (lambda: t.act_dev(dev, 2, 3, 4, hidden=[5, 6]), ValueError, "hidden names 2 layers, the actor has 3 hidden layers"),
            (lambda: t.act_dev(dev, None, 3, 4), ValueError, "obs and loc are needed"),
            (lambda: t.values_dev(dev, 2, None, 4), ValueError, "obs and values are needed, and priv"),
            (lambda: t.values_dev(dev, 2, Tensor(N * 2 - 1), 4), ValueError, "priv: 9 elements, 10 needed"),
            (lambda: t.values_dev(dev, 2, 3, Tensor(N - 1)), ValueError, "values: 4 elements, 5 needed"),
            (lambda: t.values_dev(dev, 2, 3, 4, hidden=[5]), ValueError, "the critic has 3 hidden layers"),
            (lambda: t.act(host, np.zeros((N, 4), F), sample=False), ValueError, r"act: obs: shape \(5, 4\)"),
            (lambda: t.values(host, obs, np.zeros((N, 3), F)), ValueError, r"values: priv: shape \(5, 3\), \(5, 2\) needed"),
            (lambda: t.values(host, obs), ValueError, r"values: priv: shape None")):
        with pytest.raises(exc, match=match):
            call()


# ---- the statement against the reference's own model -----------------------------------------------------------------------------------
def test_the_mirror_is_the_references_model(golden):
    g = golden
    O, P, A = (int(x) for x in g["cols"])
    assert (O, P, A) == pol.GOLDEN_COLS and g["obs"].shape == (pol.GOLDEN_ROWS, O) and g["priv"].shape == (pol.GOLDEN_ROWS, P)
    assert (np.abs(g["loc"]) > 1).any()
    params = golden_parameters()
    assert [p.shape for p in params] == pol.shapes(O, P, A) and sum(p.size for p in params) == 152199
    worst = deviations(g, params, g["obs"], g["priv"])
    for k in MEASURED:
        print(f"{k}: largest deviation {worst[k]!r} units (measured {MEASURED[k]!r}, bound {BOUND[k]!r})")
    for k in MEASURED:
        assert worst[k] <= BOUND[k], (k, worst[k], BOUND[k])
    # what the fixture pins: the layout of W, the order of the critic's input, the order of the parameter list, the ELU
    logstd, critic, actor = pol.split(params, 3)

    def rebuilt(critic=critic, actor=actor):
        return [logstd] + [x for pair in critic for x in pair] + [x for pair in actor for x in pair]

    transposed = rebuilt(actor=[(actor[0][0], actor[0][1]), (actor[1][0], actor[1][1]), (np.ascontiguousarray(actor[2][0].T), actor[2][1]), actor[3]])
    wrong = deviations(g, transposed, g["obs"], g["priv"])
    print(f"a transposed W: loc {wrong['loc']!r} units, actor_hidden_2 {wrong['actor_hidden_2']!r}")
    assert wrong["loc"] > 10 * BOUND["loc"] and wrong["actor_hidden_2"] > 10 * BOUND["actor_hidden_2"] and wrong["actor_hidden_1"] == worst["actor_hidden_1"]
    # (priv, obs): the critic's input put together in the other order
    other = pol.Policy(P, O, A, num_envs=pol.GOLDEN_ROWS).values(params, g["priv"], g["obs"])["values"]
    print(f"(priv, obs): values {units(other, g['values'])!r} units")
    assert units(other, g["values"]) > 10 * BOUND["values"]
    # an ELU with another formula
    relu = np.maximum(pol.Policy(O, P, A).act(params, g["obs"], sample=False)["hidden"][0], 0)
    assert units(relu[:, ::int(g["hidden_stride"])], g["actor_hidden_0"]) > 10 * BOUND["actor_hidden_0"]


def test_the_float64_evaluation_is_the_same_statement(golden):
    """the yardstick of the device test: the same lines in float64 lie closer to the fixture's float32 than its own rounding"""
    g = golden
    O, P, A = (int(x) for x in g["cols"])
    m = pol.Policy(O, P, A, num_envs=pol.GOLDEN_ROWS, dtype=D)
    params = golden_parameters()
    a, v = m.act(params, g["obs"], sample=False), m.values(params, g["obs"], g["priv"])
    assert a["loc"].dtype == D and v["values"].dtype == D
    assert units(a["loc"], g["loc"]) <= BOUND["loc"] and units(v["values"], g["values"]) <= BOUND["values"]


def test_the_draw_and_the_counts():
    rng = np.random.default_rng(5)
    O, P, A, N = 3, 0, 4, 6
    params = [rng.normal(0, 0.3, s).astype(F) for s in pol.shapes(O, P, A, (32,), (32,))]
    obs = np.repeat(rng.normal(0, 1, (1, O)).astype(F), N, axis=0)          # every environment sees the same row
    m = pol.Policy(O, P, A, (32,), (32,), num_envs=N, seed=77)
    a = m.act(params, obs)
    assert (m.counts == 1).all() and a["actions"].dtype == F
    assert (a["loc"] == a["loc"][0]).all() and len({row.tobytes() for row in a["actions"]}) == N      # equal rows, different actions
    assert a["actions"].tobytes() == (a["loc"] + np.exp(params[0])[None, :] * pol.draws(m.key, np.zeros(N, np.uint32), A)[0]).astype(F).tobytes()
    b = m.act(params, obs)
    assert (m.counts == 2).all() and b["loc"].tobytes() == a["loc"].tobytes() and b["actions"].tobytes() != a["actions"].tobytes()
    again = pol.Policy(O, P, A, (32,), (32,), num_envs=N, seed=77)
    assert again.act(params, obs)["actions"].tobytes() == a["actions"].tobytes()
    assert pol.Policy(O, P, A, (32,), (32,), num_envs=N, seed=78).act(params, obs)["actions"].tobytes() != a["actions"].tobytes()
    m.act(params, obs[:2], sample=False)
    assert (m.counts == 2).all()                                     # sample off touches no count and takes any rows
    # the words are the tracker's: element i of environment e at its count, domain 5; elements 2 j and 2 j + 1 share one Philox call
    import proprio_mirror as pm
    import tracker_mirror as tm
    w = tm.philox4x32((3, 1, 1, 5), m.key)
    assert pol.draws(m.key, np.ones(N, np.uint32), A)[0][3, 2] == pm.gaussian32(w[0], w[1])
    assert pol.draws(m.key, np.ones(N, np.uint32), A)[0][3, 3] == pm.gaussian32(w[2], w[3])
