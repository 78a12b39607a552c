"""The tracker's backward pass through the two networks without a GPU: the exports, their ctypes signatures and the
constants against the header, every argument check that must fire before the library is loaded, the host's plan under plain g++
(tests/cpp/policy_bwd_plan_check.cpp), and the NumPy statement (tests/policy_bwd_mirror.py) against the fixture recorded by running
``torch.autograd.backward`` through the reference's own ``ActorCritic`` in float32 CPU torch (tests/golden/policy_bwd_golden.npz,
tests/golden/make_policy_bwd_golden.py)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header as abi  # noqa: E402
import policy_bwd_mirror as bwd  # noqa: E402
import policy_mirror as pol  # noqa: E402
from test_tracker_policy_host import golden_parameters  # noqa: E402
from test_tracker_proprio_host import offline_tracker  # noqa: E402

SYMBOLS = ("gmr_motion_tracker_set_backward", "gmr_motion_tracker_act_backward_dev", "gmr_motion_tracker_act_backward",
           "gmr_motion_tracker_values_backward_dev", "gmr_motion_tracker_values_backward", "gmr_motion_tracker_backward_state")
F = np.float32
D = np.float64
EPS32 = float(np.finfo(F).eps)
# The mirror cannot be bit-equal to torch: torch's CPU GEMMs sum in the order of their blocking, and its ELU backward takes exp of the saved
# input where the statement takes y + 1 from the saved output (one rounding apart).  MEASURED[kind] is the largest |mirror - fixture| /
# (eps32 * max |fixture tensor|) over the tensors of the kind, on the fixture's 70 rows; the bound is four times that (the rule of DESIGN.md
# sections 6v, 6x and 6z).
MEASURED = {"dW": 5.048307414445662, "db": 5.406472421577351}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}


def units(got, want):
    """the largest deviation in units of eps32 times the tensor's largest magnitude"""
    got, want = np.asarray(got, D), np.asarray(want, D)
    return float(np.abs(got - want).max() / (EPS32 * np.abs(want).max()))


@functools.lru_cache(maxsize=None)
def golden():
    """the fixture, the forward fixture's rows and the rebuilt upstream gradients; made once and never written"""
    with np.load(os.path.join(GOLDEN, "policy_bwd_golden.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    with np.load(os.path.join(GOLDEN, "policy_golden.npz"), allow_pickle=False) as z:
        g["obs"], g["priv"] = z["obs"], z["priv"]
    rows, A = int(g["rows"]), int(g["cols"][2])
    g["g_loc"], g["g_values"] = bwd.upstream(rows, A, 0), bwd.upstream(rows, 1, 1)[:, 0]
    for a in g.values():
        a.flags.writeable = False
    return g


def against_fixture(dW, db, first, g):
    """the gradients of one network (lists over its layers) against the fixture -> {tensor name: units}"""
    step = int(g["dw_stride"])
    out = {}
    for l in range(len(dW)):
        out[f"dW_{first + 2 * l}"] = units(np.asarray(dW[l])[::step], g[f"dW_{first + 2 * l}"])
        out[f"db_{first + 2 * l + 1}"] = units(db[l], g[f"db_{first + 2 * l + 1}"])
    return out


def mirror_on_fixture(dtype=F, wrong=None, chunk=bwd.CHUNK):
    g = golden()
    O, P, A = (int(x) for x in g["cols"])
    params = golden_parameters()
    m = pol.Policy(O, P, A, num_envs=int(g["rows"]), dtype=dtype)
    a, v = m.act(params, g["obs"], sample=False), m.values(params, g["obs"], g["priv"])
    B = bwd.Backward(m, chunk)
    ra, rv = B.act(params, g["obs"], a["hidden"], g["g_loc"], wrong), B.values(params, g["obs"], g["priv"], v["hidden"], g["g_values"], wrong)
    assert all(x.dtype == dtype for r in (ra, rv) for k in ("delta", "dW", "db") for x in r[k])
    out = against_fixture(rv["dW"], rv["db"], 1, g)
    out.update(against_fixture(ra["dW"], ra["db"], 9, g))
    return out


def test_the_library_exports_the_backward_entry_points_with_the_headers_signatures():
    from general_motion_retargeting_amd import _lib, build
    from general_motion_retargeting_amd import motion_tracker as mt
    L = C.CDLL(_lib.LIB_PATH)
    hdr = abi.read()
    assert "N18: tracker policy backward" in hdr and hdr.index("N18: tracker policy backward") > hdr.index("N17: tracker policy")
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTED_SYMBOLS
        res, args = _lib._SIGS[sym]
        assert res is C.c_int and args == abi.parameters(hdr, sym), (sym, args)
    for define, value in (("GMR_POLICY_BWD_CHUNK", _lib.POLICY_BWD_CHUNK), ("GMR_POLICY_BWD_MAX_ROWS", _lib.POLICY_BWD_MAX_ROWS)):
        assert abi.define(hdr, define) == value, define
    assert (_lib.POLICY_BWD_CHUNK, _lib.POLICY_BWD_MAX_ROWS) == (bwd.CHUNK, bwd.MAX_ROWS) and bwd.CHUNK % 32 == 0
    # the cap keeps the workspace of the widest admissible networks below 1 GB
    widest = max(sum(pol.sizes(512, 0, 32, (256,) * 4, (256,) * 4)[1:10]), sum(pol.sizes(512, 0, 32, (256,) * 4, (256,) * 4)[11:]))
    assert widest == 336928 and bwd.chunks(bwd.MAX_ROWS) * widest * 4 == 690028544 < 10 ** 9
    for name in ("set_backward", "act_backward_dev", "act_backward", "values_backward_dev", "values_backward", "backward_state"):
        assert callable(getattr(mt.MotionTracker, name)), name
    assert "gmr_tracker_policy_bwd.hip" in build.SOURCES and "gmr_tracker_policy_bwd_plan.h" in build.HEADERS
    # the rules of the other blocks: one rounding per operation, no floating-point atomics, no wait for the host behind a launch
    csrc = os.path.join(ROOT, "general_motion_retargeting_amd", "csrc")
    src = open(os.path.join(csrc, "gmr_tracker_policy_bwd.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("#include", 1)[1]
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in src
    body = src[src.index("static int backward_launch"):]
    body = body[:body.index("\n}\n")]
    assert "Synchronize" not in body and "hipMemcpy" not in body and "hipMalloc" not in body
    assert body.count("hipLaunchKernelGGL") == 3                      # THREE launches per call


def test_the_plan_of_the_backward_pass_under_plain_cpp(tmp_path):
    """The stand-alone program, compiled with AddressSanitizer + UBSan where their runtime is installed and plainly where it is not."""
    exe, src = str(tmp_path / "policy_bwd_plan_check"), os.path.join(ROOT, "tests", "cpp", "policy_bwd_plan_check.cpp")
    cc = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-o", exe, src]
    if subprocess.run(cc + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True).returncode != 0:
        subprocess.check_call(cc)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "ERROR" not in out.stderr, out.stderr[-2000:]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_backward_arguments_are_refused_before_the_library_is_loaded(monkeypatch):
    from general_motion_retargeting_amd import _lib

    def no_device():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_device)
    N = 5
    t = offline_tracker(N, 5)
    assert t.backward_state() is None
    with pytest.raises(ValueError, match="set_backward: the policy is not set on this tracker, call set_policy\\(\\) first"):
        t.set_backward(64)
    p = t._policy = t._policy_setup(5, 2, 3, pol.ACTOR_HIDDEN, pol.CRITIC_HIDDEN)
    K = len(p["sizes"])
    dev = list(range(1, K + 1))                                      # raw addresses: nothing is dereferenced before the library
    for call in (lambda: t.act_backward_dev(dev, dev, 2, [3, 4, 5], 6, [7, 8, 9]), lambda: t.values_backward_dev(dev, dev, 2, 3, [3, 4, 5], 6, [7, 8, 9]),
                 lambda: t.act_backward([], np.zeros((N, 5), F), [], np.zeros((N, 3), F)), lambda: t.values_backward([], np.zeros((N, 5), F), None, [], np.zeros(N, F))):
        with pytest.raises(ValueError, match="call set_backward\\(\\) first"):
            call()
    for rows, match in ((0, "max_rows = 0: a whole number in 1 .. 131072"), (-3, "max_rows = -3"), (131073, "max_rows = 131073"), (2.5, "max_rows = 2.5"),
                        (1 << 40, "max_rows = 1099511627776")):
        with pytest.raises(ValueError, match="set_backward: " + match):
            t.set_backward(rows)
    assert t._backward is None
    c = t._backward = t._backward_setup(64)
    assert c["max_rows"] == 64 and c["policy"] is p

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

    host = [np.zeros(s, F) for s in pol.shapes(5, 2, 3)]
    obs, priv = np.zeros((N, 5), F), np.zeros((N, 2), F)
    ha, hc = [np.zeros((N, h), F) for h in pol.ACTOR_HIDDEN], [np.zeros((N, h), F) for h in pol.CRITIC_HIDDEN]
    h3 = [3, 4, 5]
    for call, exc, match in (
            (lambda: t.act_backward_dev(dev, dev, 2, h3, 6, h3, rows=65), ValueError, "act_backward_dev: rows = 65: 1 .. max_rows = 64 are taken"),
            (lambda: t.values_backward_dev(dev, dev, 2, 3, h3, 6, h3, rows=0), ValueError, "values_backward_dev: rows = 0: 1 .. max_rows = 64"),
            (lambda: t.act_backward(host, np.zeros((65, 5), F), ha, np.zeros((65, 3), F)), ValueError, "act_backward: rows = 65"),
            (lambda: t.act_backward_dev(dev[:-1], dev, 2, h3, 6, h3), ValueError, f"params names {K - 1} tensors, the policy was set for K = {K}"),
            (lambda: t.act_backward_dev(dev, dev[:-1], 2, h3, 6, h3), ValueError, f"grads names {K - 1} tensors, the policy was set for K = {K}"),
            (lambda: t.act_backward_dev(dev, 7, 2, h3, 6, h3), ValueError, "grads is the list of the gradients"),
            (lambda: t.act_backward_dev(dev, dev[:9] + [None] + dev[10:], 2, h3, 6, h3), ValueError, r"grads\[9\] is needed: the actor's gradients"),
            (lambda: t.values_backward_dev(dev, [None] + dev[1:3] + [None] + dev[4:], 2, 3, h3, 6, h3), ValueError, r"grads\[3\] is needed: the critic's"),
            (lambda: t.act_backward_dev(dev, dev[:9] + [Tensor(256 * 5 - 1)] + dev[10:], 2, h3, 6, h3), ValueError, r"grads\[9\]: 1279 elements, 1280 needed"),
            (lambda: t.act_backward_dev(dev, dev[:9] + [Tensor(256 * 5, "torch.float64")] + dev[10:], 2, h3, 6, h3), ValueError, r"grads\[9\]: dtype torch.float64"),
            (lambda: t.act_backward_dev(dev, host, 2, h3, 6, h3), TypeError, "device address"),
            (lambda: t.act_backward_dev(dev, dev, 2, h3[:2], 6, h3), ValueError, "hidden names 2 layers, the actor has 3 hidden layers"),
            (lambda: t.act_backward_dev(dev, dev, 2, h3, 6, h3 + [9]), ValueError, "delta names 4 layers, the actor has 3 hidden layers"),
            (lambda: t.act_backward_dev(dev, dev, 2, [3, None, 5], 6, h3), ValueError, r"hidden\[1\] is needed: the backward pass takes every layer"),
            (lambda: t.act_backward_dev(dev, dev, 2, h3, 6, [3, 4, None]), ValueError, r"delta\[2\] is needed"),
            (lambda: t.act_backward_dev(dev, dev, 2, h3, 6, 7), ValueError, "delta is a list with one array per hidden layer"),
            (lambda: t.act_backward_dev(dev, dev, 2, h3, 6, [3, 4, Tensor(N * 128 - 1)]), ValueError, r"delta\[2\]: 639 elements, 640 needed"),
            (lambda: t.values_backward_dev(dev, dev, 2, 3, [Tensor(N * 256), Tensor(N * 256 - 1), 5], 6, h3), ValueError, r"hidden\[1\]: 1279 elements, 1280"),
            (lambda: t.act_backward_dev(dev, dev, None, h3, 6, h3), ValueError, "obs and grad_loc are needed"),
            (lambda: t.act_backward_dev(dev, dev, 2, h3, None, h3), ValueError, "obs and grad_loc are needed"),
            (lambda: t.act_backward_dev(dev, dev, 2, h3, Tensor(N * 3 - 1), h3), ValueError, "grad_loc: 14 elements, 15 needed"),
            (lambda: t.values_backward_dev(dev, dev, 2, None, h3, 6, h3), ValueError, "obs and grad_values are needed, and priv"),
            (lambda: t.values_backward_dev(dev, dev, 2, 3, h3, Tensor(N - 1), h3), ValueError, "grad_values: 4 elements, 5 needed"),
            (lambda: t.values_backward_dev(dev, dev, 2, Tensor(N * 2 - 1), h3, 6, h3), ValueError, "priv: 9 elements, 10 needed"),
            (lambda: t.act_backward(host, np.zeros((N, 4), F), ha, np.zeros((N, 3), F)), ValueError, r"act_backward: obs: shape \(5, 4\)"),
            (lambda: t.act_backward(host, obs, ha[:2], np.zeros((N, 3), F)), ValueError, "hidden names 2 layers, the actor has 3"),
            (lambda: t.act_backward(host, obs, [ha[0], ha[1][:, :-1], ha[2]], np.zeros((N, 3), F)), ValueError, r"hidden\[1\]: shape \(5, 127\), \(5, 128\) needed"),
            (lambda: t.act_backward(host, obs, ha, np.zeros((N, 2), F)), ValueError, "the output gradient: 10 elements, 15 needed"),
            (lambda: t.act_backward(host[:3], obs, ha, np.zeros((N, 3), F)), ValueError, "params names 3 tensors"),
            (lambda: t.values_backward(host, obs, None, hc, np.zeros(N, F)), ValueError, "values_backward: priv: shape None"),
            (lambda: t.values_backward(host, obs, priv, hc, np.zeros(N + 1, F)), ValueError, "the output gradient: 6 elements, 5 needed")):
        with pytest.raises(exc, match=match):
            call()
    # a set_policy after set_backward: every call is refused until set_backward runs again
    t._policy = t._policy_setup(5, 2, 3, pol.ACTOR_HIDDEN, pol.CRITIC_HIDDEN)
    for call in (lambda: t.act_backward_dev(dev, dev, 2, h3, 6, h3), lambda: t.values_backward_dev(dev, dev, 2, 3, h3, 6, h3),
                 lambda: t.act_backward(host, obs, ha, np.zeros((N, 3), F)), lambda: t.values_backward(host, obs, priv, hc, np.zeros(N, F))):
        with pytest.raises(ValueError, match="the policy was set again after the backward pass, call set_backward\\(\\) again"):
            call()


# ---- the statement against torch's autograd through the reference's own model -----------------------------------------------------------
def test_the_mirror_is_autograd_through_the_references_model():
    g = golden()
    assert tuple(int(x) for x in g["cols"]) == pol.GOLDEN_COLS and int(g["rows"]) == pol.GOLDEN_ROWS and int(g["dw_stride"]) == bwd.GOLDEN_STRIDE
    shapes = pol.shapes(*pol.GOLDEN_COLS)
    for k in range(1, len(shapes)):
        if len(shapes[k]) == 2:
            assert g[f"dW_{k}"].shape == (-(-shapes[k][0] // bwd.GOLDEN_STRIDE), shapes[k][1]), k
        else:
            assert g[f"db_{k}"].shape == shapes[k], k
    assert np.abs(g["g_loc"]).max() < 1.0 / pol.GOLDEN_ROWS and g["g_loc"].dtype == F
    worst = {"dW": 0.0, "db": 0.0}
    # the association across chunks is part of the statement, not of its agreement with torch: one chunk, three chunks
    for chunk in (bwd.CHUNK, 32):
        got = mirror_on_fixture(chunk=chunk)
        for k, v in got.items():
            worst[k[:2]] = max(worst[k[:2]], v)
    for k in MEASURED:
        print(f"{k}: largest deviation {worst[k]!r} units (measured {MEASURED[k]!r}, bound {BOUND[k]!r})")
    for k in MEASURED:
        assert worst[k] <= BOUND[k], (k, worst[k], BOUND[k])
    # the float64 evaluation is the same statement: the yardstick of the device test
    for k, v in mirror_on_fixture(D).items():
        assert v <= BOUND[k[:2]], (k, v)
    right = mirror_on_fixture(chunk=32)
    # every seeded wrong variant lies more than ten bounds outside, in the tensors it touches, and nowhere else
    touched = {"slope_y": {1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14},     # everything below a last layer
               "untransposed": {1, 2, 9, 10, 11, 12},                # the critic's W_1 (256 x 256) and the actor's W_2 (128 x 128) are square
               "priv_obs": {1},
               "last_chunk": set(range(1, 17)),
               "db_last_tile": {2, 4, 6, 8, 10, 12, 14, 16}}
    assert set(touched) == set(bwd.SEEDED)
    for wrong, where in touched.items():
        got = mirror_on_fixture(wrong=wrong, chunk=32)
        far = {int(k[3:]) for k, v in got.items() if v > 10 * BOUND[k[:2]]}
        print(wrong, "smallest deviation where it shows:", min(got[k] for k in got if int(k[3:]) in where))
        assert far == where, (wrong, far, where)
        assert all(got[k] == right[k] for k in got if int(k[3:]) not in where), wrong


def test_the_chunks_of_the_statement():
    """one chunk is a float32 chain in rising row order; the chunks are added in float64 and rounded once"""
    rng = np.random.default_rng(11)
    g, a = rng.normal(0, 1, (70, 3)).astype(F), rng.normal(0, 1, (70, 5)).astype(F)
    dW, db = bwd.row_sums(g, a, F, chunk=32)
    parts, pb = [], []
    for lo in (0, 32, 64):
        acc, accb = np.zeros((3, 5), F), np.zeros(3, F)
        for m in range(lo, min(70, lo + 32)):
            acc = (g[m].astype(D)[:, None] * a[m].astype(D)[None, :] + acc.astype(D)).astype(F)
            accb = accb + g[m]
        parts.append(acc)
        pb.append(accb)
    assert dW.tobytes() == ((parts[0].astype(D) + parts[1].astype(D)) + parts[2].astype(D)).astype(F).tobytes()
    assert db.tobytes() == ((pb[0].astype(D) + pb[1].astype(D)) + pb[2].astype(D)).astype(F).tobytes()
    assert [bwd.chunks(r) for r in (1, bwd.CHUNK - 1, bwd.CHUNK, bwd.CHUNK + 1, 2 * bwd.CHUNK + 3)] == [1, 1, 1, 2, 3]
    y = np.array([-0.75, 0.0, 2.0], F)
    assert bwd.elu_slope(y).tolist() == [0.25, 1.0, 1.0]
