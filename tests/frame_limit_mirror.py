"""The reference of the frame-velocity-limit tests (tests/test_ik_frame_limits_host.py on the CPU, tests/test_ik_frame_limits.py
on the GPU): the loop of vel_limit_mirror.retarget_stream with BOTH clamps applied to oracle.build_qp's box, the per-solve
clamp first and the frame window last,

    w_h  = vmax_frame_h * frame_dt                 (dof 6 + h; the six dofs of the free joint: +inf)
    lf   = (theta0 - w) - theta,  hf = (theta0 + w) - theta
    lo   = min(max(lo_prev, lf), hf),  hi = min(max(hi_prev, lf), hf)

in exactly that association (the kernels round alike), theta0 taken at the top of each frame: the previous frame's result,
or q0 for frame 0, which is bounded only with `first_bounded`.  Either QP solver sits behind it, as in vel_limit_mirror.
With w = +inf both lines return lo_prev / hi_prev themselves.

Also here: the cases both test files use and their mirror runs, computed once and read-only.  Every case was checked under
the two conditions of tests/test_ik_frame_limits_host.py (at most 20 pivoting rounds in any solve, smallest stop-rule margin
at least 1e-6) before its seed was fixed; seeds tried and dropped are named next to the case.
"""
import dataclasses

import numpy as np

import bpp_mirror
import vel_limit_mirror as vm

TOL = vm.TOL
BOUND_EPS = vm.BOUND_EPS
FPS = 30.0
FRAME_DT = 1.0 / FPS
VMAX = 0.6                       # rad/s: w = 0.02 rad per frame at 30 fps, a twentieth of the unbounded steps of these inputs
VMAX_LARGE = 12.0                # rad/s: w = 0.4 rad per frame, about the largest unbounded step: rarely active


def window_of(model, vmax, frame_dt=FRAME_DT):
    """f64[nv]: the per-dof frame window of a packed model blob; vmax f64[nhinge] or a scalar (rad/s).  inf stays inf."""
    nv, nh = int(model["nv"][0]), int(model["nhinge"][0])
    w = np.full(nv, np.inf)
    v = np.broadcast_to(np.asarray(vmax, dtype=np.float64), (nh,))
    w[6:] = np.where(np.isfinite(v), v * frame_dt, np.inf)
    return w


def clamp_window(lo, hi, theta0, theta, w):
    lf, hf = (theta0 - w) - theta, (theta0 + w) - theta
    return np.minimum(np.maximum(lo, lf), hf), np.minimum(np.maximum(hi, lf), hf), lf, hf


@dataclasses.dataclass
class Run:
    q: np.ndarray                # [T, nq]
    nsolve: np.ndarray           # [T, 2]
    margin: float                # smallest |curr - next - tol| over all solves
    rounds: list                 # per solve: pivoting rounds (bpp) / empty (oracle solver)
    on_frame: list               # per solve: (frame, variables on a frame bound)


def retarget_stream(oracle, model, ts, q0, human, vmax_frame, frame_dt=FRAME_DT, vmax_solve=None, first_bounded=False, solver="bpp",
                    offset_to_ground=False):
    """One stream through the reference's loop under the frame limit `vmax_frame` at `frame_dt` (and the per-solve limit
    `vmax_solve`, None = none), with `solver` in ("oracle", "bpp")."""
    T = human.shape[0]
    tol, max_iter = float(ts["tol"][0]), int(ts["max_iter"][0])
    nv = int(model["nv"][0])
    vdt = vm.vdt_of(model, np.inf if vmax_solve is None else vmax_solve)
    w = window_of(model, vmax_frame, frame_dt)
    finite = np.isfinite(w)
    q = np.array(q0, dtype=np.float64)
    lower = upper = 0
    out = Run(np.empty((T, len(q))), np.zeros((T, 2), dtype=np.int32), np.inf, [], [])
    for t in range(T):
        theta0 = np.zeros(nv)
        theta0[6:] = q[7:]
        bounded = t > 0 or first_bounded
        tgt = oracle.preprocess(ts, human[t], offset_to_ground)
        for stage in range(2):
            if not int(ts["use_stage"][0][stage]):
                continue
            curr = oracle.stage_error(model, ts, stage, q, tgt)[1]
            num_iter = 0
            while True:
                H, c, lo, hi = oracle.build_qp(model, ts, stage, q, tgt)
                lo, hi = vm.clamp_box(lo, hi, vdt)
                at = np.zeros(nv, dtype=bool)
                if bounded:
                    theta = np.zeros(nv)
                    theta[6:] = q[7:]
                    lo, hi, lf, hf = clamp_window(lo, hi, theta0, theta, w)
                if solver == "bpp":
                    log = []
                    x, lower, upper = bpp_mirror.bpp_solve(H, c, lo, hi, lower, upper, log)
                    out.rounds.append(len(log))
                else:
                    x, rc = oracle.solve_box_qp(H, c, lo, hi)
                    assert rc > 0, rc                      # (the number of factorisations; < 0 = failure)
                if bounded:
                    at = finite & (((np.abs(x - lo) <= BOUND_EPS) & (lo == lf)) | ((np.abs(x - hi) <= BOUND_EPS) & (hi == hf)))
                out.on_frame.append((t, int(at.sum())))
                q = oracle.integrate(model, q, x)
                nxt = oracle.stage_error(model, ts, stage, q, tgt)[1]
                out.nsolve[t, stage] += 1
                if out.nsolve[t, stage] > 1:
                    num_iter += 1
                out.margin = min(out.margin, abs(curr - nxt - tol))
                if not (curr - nxt > tol and num_iter < max_iter):
                    break
                curr = nxt
        out.q[t] = q
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------
G1, T1, HEIGHTS = vm.G1, vm.T1, vm.HEIGHTS


def mixed_table(model):
    """The non-uniform frame table, indexed by hinge: 0.6 / 12 / none in turn, and 0.6 on every hinge WITHOUT a range (the
    window is the only bound such a hinge has: a kernel that skipped it would show)."""
    nh = len(model.joint_names)
    v = np.array([(VMAX, VMAX_LARGE, np.inf)[h % 3] for h in range(nh)])
    v[np.asarray(model.limited[:nh]) == 0] = VMAX
    return v


@dataclasses.dataclass
class Case:
    name: str                    # (the inputs are cached by name in vel_limit_mirror: every name here starts with "f_")
    robot: object                # a get_setup key or "dense"
    S: int
    T: int
    seed: int
    table: str = "uniform"       # "uniform" (0.6 rad/s) | "mixed"
    start: str = "qpos0"         # "outside": vel_limit_mirror.OUTSIDE
    heights: tuple = None
    vmax_solve: float = None     # the per-solve limit next to the frame limit
    first_bounded: bool = False  # GMR_FLAG_FRAME_LIMIT_FIRST

    def vmax(self):
        su = vm.setup_of(self.robot)
        return np.full(len(su.model.joint_names), VMAX) if self.table == "uniform" else mixed_table(su.model)


# G1 seed 9 (the seed of the per-solve tests) has a stop margin of 3.4e-7 at w = 0.02: not used here.
CASES = {c.name: c for c in (
    Case("f_g1", G1, 4, 6, 5),
    Case("f_t1", T1, 2, 5, 9),
    Case("f_g1_mixed", G1, 4, 6, 5, "mixed"),
    Case("f_t1_mixed", T1, 2, 5, 9, "mixed"),
    Case("f_dense_mixed", "dense", 2, 4, 5, "mixed"),
    Case("f_g1_first", G1, 4, 6, 5, first_bounded=True),
    Case("f_g1_outside", G1, 4, 6, 5, start="outside", first_bounded=True),
    Case("f_g1_scaled", G1, 4, 6, 5, heights=HEIGHTS),
    Case("f_g1_both", G1, 4, 6, 5, vmax_solve=vm.THREE_PI),
)}


make_input = vm.make_input
stream_tasksets = vm.stream_tasksets
setup_of = vm.setup_of
stacked = vm.stacked

_runs = {}


def mirror_runs(oracle, case, solver="bpp", vmax=None, first_bounded=None):
    """[Run per stream] of a case under its own table (or `vmax`), computed once per (case, solver, table, first frame)."""
    v = case.vmax() if vmax is None else np.asarray(vmax, dtype=np.float64)
    fb = case.first_bounded if first_bounded is None else first_bounded
    key = (case.name, solver, v.tobytes(), fb)
    if key not in _runs:
        su = setup_of(case.robot)
        human, q0 = make_input(case)
        tss = stream_tasksets(case)
        runs = [retarget_stream(oracle, su.mb, tss[s], q0[s], human[s], v, FRAME_DT, case.vmax_solve, fb, solver) for s in range(case.S)]
        for r in runs:
            r.q.setflags(write=False)
            r.nsolve.setflags(write=False)
        _runs[key] = runs
    return _runs[key]


WALK_FRAMES = 2                  # frames of the outside start in which both hinges are still so far out (0.1 and 0.07 rad against
#                                  w = 0.02) that the range's own bound, gain * distance with a gain of at most 1, lies beyond the window


def walk_back_error(q, q0, h, d):
    """largest |theta_h(t) - (theta_h(q0) -+ (t + 1) w)| over the first WALK_FRAMES frames: hinge h, d beyond its range,
    comes back by exactly w per frame, q0 being the frame before frame 0"""
    w = VMAX * FRAME_DT
    want = q0[:, None, 7 + h] - np.sign(d) * w * np.arange(1, WALK_FRAMES + 1)
    return float(np.abs(q[:, :WALK_FRAMES, 7 + h] - want).max())


def excess(q, q0, w, first_bounded=False):
    """[S, T, nhinge]: |theta_t - theta_{t-1}| - w * (1 + 1e-12) over the bounded frames (frame 0: against q0, only when it
    is bounded; else -inf)."""
    th = np.concatenate([q0[:, None, 7:], q[..., 7:]], axis=1)
    e = np.abs(np.diff(th, axis=1)) - w[6:] * (1.0 + 1e-12)
    if not first_bounded:
        e[:, 0] = -np.inf
    return e
