"""The reference of the body-weight tests (tests/test_ik_body_weights_host.py on the CPU, tests/test_ik_body_weights.py on the
GPU): the loop of vel_limit_mirror.retarget_stream, built from the untouched oracle, with one multiplier m[t, b] per frame and
human body on the cost side.  Per frame:

    1. the rows of missing bodies (m == 0, not the human root) are set to NaN;
    2. the packed task set is copied with w_pos[st, :K] and w_rot[st, :K] multiplied by m[task_human] -- one product each;
    3. oracle.preprocess runs on that copy (its own NaN rule keeps missing feet out of the lowest-foot search);
    4. the missing rows of the targets get a finite stand-in (the identity pose; no result depends on it);
    5. the residual norm of the stop rule is sqrt(sum(e[keep] ** 2)) over the rows of oracle.stage_error with m != 0;
    6. build_qp on the copy, either CPU solver, integrate, and the stop rule as in vel_limit_mirror; the two velocity clamps of
       frame_limit_mirror are composed onto the box where a case sets them.

With weights of ones the copy is the task set, nothing is missing, and the loop with the oracle's solver is
oracle.retarget_streams in qpos and solve counts.

Weights of a case: LEVELS[rng(100 + seed).choice(4, size=(S, T, nhuman), p=(0.3, 0.2, 0.3, 0.2))]; with offset_to_ground a frame
in which every foot is missing gets 1.0 on its first foot (every foot missing is out of the feature's scope).

Seeds: every case runs its stated seed; none had to be replaced (the figures are in tests/test_ik_body_weights_host.py).
"""
import dataclasses

import numpy as np

import bpp_mirror
import frame_limit_mirror as fm
import vel_limit_mirror as vm

TOL = vm.TOL
LEVELS = np.array((0.0, 0.25, 1.0, 2.5))
LEVEL_P = (0.3, 0.2, 0.3, 0.2)
STAND_IN = np.array((0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0))
G1, T1, HEIGHTS = vm.G1, vm.T1, vm.HEIGHTS


def missing_rows(ts, m):
    """bool[nhuman]: bodies missing under the multipliers m[nhuman] -- weight 0 and not the human root"""
    nh = int(ts["nhuman"][0])
    return (np.asarray(m)[:nh] == 0.0) & (np.arange(nh) != int(ts["human_root"][0]))


def weighted_taskset(ts, m):
    """a copy of the packed task set with the weights of both tables multiplied by the multiplier of each task's human body"""
    tw = ts.copy()
    for st in range(2):
        K = int(ts["ntask"][0][st])
        th = ts["task_human"][0][st, :K]
        tw["w_pos"][0][st, :K] = ts["w_pos"][0][st, :K] * m[th]
        tw["w_rot"][0][st, :K] = ts["w_rot"][0][st, :K] * m[th]
    return tw


def frame_targets(oracle, ts, human_t, m, offset_to_ground):
    """(weighted task set, targets with the stand-in in the missing rows, missing) of one frame"""
    miss = missing_rows(ts, m)
    h = np.array(human_t, dtype=np.float64)
    h[miss] = np.nan
    tw = weighted_taskset(ts, m)
    tgt = oracle.preprocess(tw, h, offset_to_ground)
    tgt[miss] = STAND_IN
    return tw, tgt, miss


def masked_norm(oracle, model, tw, ts, stage, q, tgt, m):
    K = int(ts["ntask"][0][stage])
    keep = m[ts["task_human"][0][stage, :K]] != 0.0
    e = oracle.stage_error(model, tw, stage, q, tgt)[0]
    return float(np.sqrt(np.sum(e[keep] ** 2)))


def masked_errors(oracle, model, ts, q, human_t, m, offset_to_ground=False):
    """f64[2]: what err_out holds for a frame that ends at q (0 for a stage the config does not use)"""
    tw, tgt, _ = frame_targets(oracle, ts, human_t, m, offset_to_ground)
    return np.array([masked_norm(oracle, model, tw, ts, st, q, tgt, m) if int(ts["use_stage"][0][st]) else 0.0 for st in range(2)])


@dataclasses.dataclass
class Run:
    q: np.ndarray                # [T, nq]
    nsolve: np.ndarray           # [T, 2]
    err: np.ndarray              # [T, 2]: the masked norms at the configuration each frame ends with
    margin: float                # smallest |curr - next - tol| over all solves
    rounds: list                 # per solve: pivoting rounds (bpp) / empty (oracle solver)


def retarget_stream(oracle, model, ts, q0, human, weight, solver="bpp", offset_to_ground=False, vmax_solve=None, vmax_frame=None,
                    frame_dt=fm.FRAME_DT, first_bounded=False):
    """One stream through the reference's loop under the body weights weight[T, nhuman], with `solver` in ("oracle", "bpp")."""
    T = human.shape[0]
    tol, max_iter = float(ts["tol"][0]), int(ts["max_iter"][0])
    nv = int(model["nv"][0])
    vdt = vm.vdt_of(model, np.inf if vmax_solve is None else vmax_solve)
    w = fm.window_of(model, np.inf if vmax_frame is None else vmax_frame, frame_dt)
    q = np.array(q0, dtype=np.float64)
    lower = upper = 0
    out = Run(np.empty((T, len(q))), np.zeros((T, 2), dtype=np.int32), np.zeros((T, 2)), np.inf, [])
    for t in range(T):
        m = np.asarray(weight[t], dtype=np.float64)
        theta0 = np.zeros(nv)
        theta0[6:] = q[7:]
        bounded = vmax_frame is not None and (t > 0 or first_bounded)
        tw, tgt, _ = frame_targets(oracle, ts, human[t], m, offset_to_ground)
        for stage in range(2):
            if not int(ts["use_stage"][0][stage]):
                continue
            curr = masked_norm(oracle, model, tw, ts, stage, q, tgt, m)
            num_iter = 0
            while True:
                H, c, lo, hi = oracle.build_qp(model, tw, stage, q, tgt)
                if vmax_solve is not None:
                    lo, hi = vm.clamp_box(lo, hi, vdt)
                if bounded:
                    theta = np.zeros(nv)
                    theta[6:] = q[7:]
                    lo, hi, _, _ = fm.clamp_window(lo, hi, theta0, theta, w)
                if solver == "bpp":
                    log = []
                    x, lower, upper = bpp_mirror.bpp_solve(H, c, lo, hi, lower, upper, log)
                    out.rounds.append(len(log))
                else:
                    x, rc = oracle.solve_box_qp(H, c, lo, hi)
                    assert rc > 0, rc
                q = oracle.integrate(model, q, x)
                nxt = masked_norm(oracle, model, tw, ts, stage, q, tgt, m)
                out.nsolve[t, stage] += 1
                if out.nsolve[t, stage] > 1:
                    num_iter += 1
                out.margin = min(out.margin, abs(curr - nxt - tol))
                if not (curr - nxt > tol and num_iter < max_iter):
                    break
                curr = nxt
        out.q[t] = q
        for stage in range(2):
            if int(ts["use_stage"][0][stage]):
                out.err[t, stage] = masked_norm(oracle, model, tw, ts, stage, q, tgt, m)
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str                    # (the inputs are cached by name in vel_limit_mirror: every name here starts with "w_")
    robot: object                # a get_setup key or "dense"
    S: int
    T: int
    seed: int
    heights: tuple = None
    vmax_solve: float = None     # the per-solve velocity limit on top (rad/s, every hinge)
    vmax_frame: float = None     # the frame velocity limit on top (rad/s, every hinge, at frame_limit_mirror.FPS)
    start: str = "qpos0"


CASES = {c.name: c for c in (
    Case("w_g1", G1, 4, 6, 9),
    Case("w_t1", T1, 2, 4, 5),
    Case("w_dense", "dense", 2, 4, 9),          # (seed 5 has a stop margin of 1.2e-6, too close to the floor)
    Case("w_g1_heights", G1, 4, 6, 9, heights=HEIGHTS),
    Case("w_g1_both", G1, 4, 6, 9, vmax_solve=vm.THREE_PI, vmax_frame=fm.VMAX),
)}
GROUND_CASES = ("w_g1", "w_t1")                 # both variants of offset_to_ground

make_input = vm.make_input
stream_tasksets = vm.stream_tasksets
setup_of = vm.setup_of

_weights, _runs = {}, {}


def make_weights(case, ground=False):
    """f64[S, T, nhuman] of a case, read-only and shared"""
    key = (case.name, bool(ground))
    if key not in _weights:
        su = setup_of(case.robot)
        nh = int(su.ts["nhuman"][0])
        m = LEVELS[np.random.default_rng(100 + case.seed).choice(4, size=(case.S, case.T, nh), p=LEVEL_P)]
        if ground:
            feet = np.nonzero(su.ts["is_foot"][0][:nh])[0]
            none = (m[..., feet] == 0.0).all(axis=-1)
            m[none, feet[0]] = 1.0
        m.setflags(write=False)
        _weights[key] = m
    return _weights[key]


def limits_of(case):
    """(vmax_solve f64[nhinge] or None, vmax_frame f64[nhinge] or None) of a case"""
    nh = len(setup_of(case.robot).model.joint_names)
    return (None if case.vmax_solve is None else np.full(nh, case.vmax_solve),
            None if case.vmax_frame is None else np.full(nh, case.vmax_frame))


def mirror_runs(oracle, case, solver="bpp", ground=False, weight=None):
    """[Run per stream] of a case under its own weights (or `weight`), computed once per (case, solver, ground, weights)."""
    w = make_weights(case, ground) if weight is None else np.asarray(weight, dtype=np.float64)
    key = (case.name, solver, bool(ground), w.tobytes())
    if key not in _runs:
        su = setup_of(case.robot)
        human, q0 = make_input(case)
        tss = stream_tasksets(case)
        vs, vf = limits_of(case)
        runs = [retarget_stream(oracle, su.mb, tss[s], q0[s], human[s], w[s], solver, ground, vs, vf) for s in range(case.S)]
        for r in runs:
            for a in (r.q, r.nsolve, r.err):
                a.setflags(write=False)
        _runs[key] = runs
    return _runs[key]


def stacked(runs):
    return np.stack([r.q for r in runs]), np.stack([r.nsolve for r in runs])


def with_missing_rows(case, human, weight, fill):
    """a copy of human[S, T, nhuman, 7] with the rows of the missing bodies set to `fill`"""
    su = setup_of(case.robot)
    h = np.array(human)
    for s in range(h.shape[0]):
        for t in range(h.shape[1]):
            h[s, t, missing_rows(su.ts, weight[s, t])] = fill
    return h
