"""-m gpu: the three IK kernels off the shipped line -- solver parameters other than the defaults and stage tables that
differ between the stages -- against the CPU oracle.

The variants, their inputs and tolerances are in tests/ik_variants.py; tests/test_ik_variants_host.py shows on the CPU
that the inputs are fit for the comparison and which kernel instance each case reaches.  Every variant runs in the
latency shape (set_waves(4): ik_streams_kernel<class, 4>), the throughput shape (set_waves(1): gmr_ik_wide.hip) and the
one-wavefront shape (set_waves(1) on a solver created under GMR_IK_NO_WIDE=1: ik_streams_kernel<class, 1>); `sixteen`
does not fit the throughput kernel and runs <48, 4> and <48, 1>.

Tolerances (ik_variants.BASE_TOL / DERIVED_TOL; amplification = the oracle's own deviation under rounding-sized noise
relative to the shipped parameters', measured on the CPU):
    smooth input 1e-9, scattered input 1e-8                      every variant but the four below
    damping=0.05     amplification 0.99  -> 1e-9
    damping=0.25     amplification 0.99  -> 1e-9
    lm_damping=0.1   amplification 0.69  -> 1e-9
    lm_damping=10.0  amplification 8.37  -> 1e-8
"""
import numpy as np
import pytest

import ik_variants as iv
from conftest import ALL_CONFIGS, get_setup

pytestmark = pytest.mark.gpu

SHAPES_AGREE = 1e-12            # as test_launch_shapes_agree: the same algorithm in another launch shape
ERR_TOL = 1e-10                 # error1 / error2 at the kernel's own output, as test_gpu_parity.py compares them


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _solver(hip, monkeypatch, mb, ts, shape):
    """A solver that serves `shape`.  GMR_IK_NO_WIDE is read by gmr_solver_create: set before, removed after."""
    if shape == "onewave":
        monkeypatch.setenv("GMR_IK_NO_WIDE", "1")
    try:
        sol = hip.Solver(mb, ts)
    finally:
        monkeypatch.delenv("GMR_IK_NO_WIDE", raising=False)
    sol.set_waves(4 if shape == "latency" else 1)
    return sol


def _check(tag, out, ref, tol):
    q_h, ns_h, st_h = out[:3]
    q_o, ns_o = ref[:2]
    assert (st_h == 0).all(), (tag, st_h)
    assert np.array_equal(ns_h, ns_o), f"{tag}: solve counts differ from the oracle's"
    err = float(np.abs(q_h - q_o).max())
    print(f"{tag}: max |q - q_oracle| = {err:.3e} (tolerance {tol:g})")
    assert err <= tol, (tag, err)
    return err


def _run_shapes(hip, oracle, monkeypatch, v, **kw):
    human, q0 = iv.make_input(v)
    ref = iv.oracle_run(oracle, v)
    assert (ref[2] == 0).all()
    flags = hip.FLAG_OFFSET_TO_GROUND if v.ground else 0
    outs = {}
    for shape in iv.shapes_of(v):
        sol = _solver(hip, monkeypatch, v.mb, v.ts, shape)
        outs[shape] = sol.retarget_streams(q0, human, flags=flags, **kw)
        sol.close()
        _check(f"{v.name} {shape}", outs[shape], ref, v.tol)
    if not v.derived:
        first, *others = outs
        for shape in others:
            out = outs[shape]
            assert np.array_equal(out[1], outs[first][1]), (v.name, shape)
            d = float(np.abs(out[0] - outs[first][0]).max())
            print(f"{v.name}: max |q_{shape} - q_{first}| = {d:.3e}")
            assert d <= SHAPES_AGREE, (v.name, shape, d)
    return outs, ref


@pytest.mark.parametrize("name", iv.variant_names("param"))
def test_parameter_variant_matches_oracle_in_every_shape(hip, oracle, monkeypatch, name):
    """One field of (damping, lm_damping, tol, max_iter, limit_gain, ground_offset, model timestep) off its default:
    status, solve counts and q against the oracle.  A kernel that hard-coded the field fails here: the oracle's result
    moves by more than 1e-4 for every one of them (test_ik_variants_host.py)."""
    v = iv.all_variants()[name]
    outs, ref = _run_shapes(hip, oracle, monkeypatch, v)
    if name.startswith("max_iter="):
        k = int(v.ts["max_iter"][0])
        for shape, (q, ns, st) in outs.items():
            assert (ns >= 1).all() and (ns <= k + 1).all(), (shape, int(ns.max()))       # both stages are enabled
            if k == 0:
                assert (ns == 1).all(), shape


@pytest.mark.parametrize("name", iv.variant_names("stage"))
def test_stage_variant_matches_oracle_in_every_shape(hip, oracle, monkeypatch, name):
    """Stage tables the shipped configurations do not have: one stage only, other task order, fewer tasks in one stage
    (K[0] != K[1]), the same pairs in both, an H pattern of stage 2 that is a strict subset of stage 1's, and 16 tasks with
    179 pairs (size class 48 on a full-size robot)."""
    v = iv.all_variants()[name]
    want_errors = name in ("only2", "no_left_arm_2")
    outs, ref = _run_shapes(hip, oracle, monkeypatch, v, want_errors=want_errors)
    enabled = v.ts["use_stage"][0] != 0
    human, q0 = iv.make_input(v)
    for shape, out in outs.items():
        ns = out[1]
        assert (ns[..., ~enabled] == 0).all() and (ns[..., enabled] >= 1).all(), shape
        if not want_errors:
            continue
        q_h, err_h = out[0], out[4]
        worst = 0.0
        for s in range(iv.S):
            for t in range(iv.T):
                tgt = oracle.preprocess(v.ts, human[s, t])
                for stage in range(2):
                    E = oracle.stage_error(v.mb, v.ts, stage, q_h[s, t], tgt)[1] if enabled[stage] else 0.0
                    worst = max(worst, abs(err_h[s, t, stage] - E))
        print(f"{name} {shape}: max |error - oracle stage error| = {worst:.3e}")
        assert worst <= ERR_TOL, (shape, worst)
        assert (err_h[..., ~enabled] == 0).all(), shape


@pytest.mark.parametrize("src,robot", ALL_CONFIGS)
def test_one_wavefront_kernel_all_configs(hip, oracle, monkeypatch, src, robot):
    """ik_streams_kernel<28 | 32 | 36, 1, QP_TREE_SMALL>: what every shipped robot runs under GMR_IK_NO_WIDE=1, on
    scattered targets (joint limits active), S=3, T=6."""
    from general_motion_retargeting_amd import synth
    su = get_setup(src, robot, 1.7)
    human, q0 = synth.make_streams(su.model, su.tt, 3, 6, seed=iv.SEED)
    human = iv.scatter(human)
    q_o, ns_o, st_o = oracle.retarget_streams(su.mb, su.ts, q0, human)
    assert (st_o == 0).all()
    sol = _solver(hip, monkeypatch, su.mb, su.ts, "onewave")
    out = sol.retarget_streams(q0, human)
    sol.close()
    _check(f"{src}/{robot} onewave", out, (q_o, ns_o), iv.BASE_TOL["scatter"])


@pytest.mark.parametrize("name", iv.QUEUED)
def test_queued_dispatch_with_unequal_stages(hip, oracle, name):
    """The device-side queue saves and restores a stream's state between items: with K[0] != K[1] (and with the second
    stage stopping after one solve, lm_damping=0.1) the bits are still those of one workgroup per stream."""
    v = iv.all_variants()[name]
    bh, bq = iv.make_input(v, S_=iv.QUEUED_BASE, T_=iv.QUEUED_T)
    pick = np.arange(iv.QUEUED_S) % iv.QUEUED_BASE
    human, q0 = bh[pick].copy(), bq[pick].copy()
    sol = hip.Solver(v.mb, v.ts)
    sol.set_waves(1)
    sol.set_dispatch(0)
    q_d, ns_d, st_d = sol.retarget_streams(q0, human)
    sol.set_dispatch(2)
    q_q, ns_q, st_q = sol.retarget_streams(q0, human)
    sol.close()
    assert (st_d == 0).all() and np.array_equal(st_d, st_q) and np.array_equal(ns_d, ns_q) and np.array_equal(q_d, q_q)
    ref = iv.oracle_run(oracle, v, S_=iv.QUEUED_BASE, T_=iv.QUEUED_T)
    n = iv.QUEUED_BASE
    _check(f"{name} queued", (q_q[-n:], ns_q[-n:], st_q[-n:]), (ref[0][pick[-n:]], ref[1][pick[-n:]]), v.tol)


def test_shim_damping_reaches_the_kernel(hip, oracle):
    """GeneralMotionRetargeting(..., damping=0.25): the public argument, through the packed task set, to the kernel."""
    from general_motion_retargeting_amd import GeneralMotionRetargeting, synth
    v = iv.all_variants()["damping=0.25"]
    human, q0 = iv.make_input(v)
    frames = synth.streams_to_dicts(v.tt, human[0])
    g = GeneralMotionRetargeting(*iv.BASE[:2], actual_human_height=iv.BASE[2], damping=0.25)
    assert float(g._taskset_blob["damping"][0]) == 0.25
    clip = g.retarget_clip(frames)
    q_o = iv.oracle_run(oracle, v)[0][0]
    err = float(np.abs(clip - q_o).max())
    print(f"shim damping=0.25: max |q - q_oracle| = {err:.3e} (tolerance {v.tol:g})")
    assert err <= v.tol, err
    default = GeneralMotionRetargeting(*iv.BASE[:2], actual_human_height=iv.BASE[2]).retarget_clip(frames)
    assert np.abs(default - iv.oracle_run(oracle, iv.all_variants()["default"])[0][0]).max() <= iv.BASE_TOL["smooth"]
    assert np.abs(default - clip).max() > 1e-4
