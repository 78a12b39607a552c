"""-m gpu: the IK kernels at their compile-time capacities, against the CPU oracle.

The robots, their inputs, the figures the oracle gives on them and the tolerances are in tests/ik_capacity.py;
tests/test_ik_capacity_host.py shows on the CPU that the inputs are fit for the comparison and which kernel instance every
(case, shape) reaches:

    wide160      the throughput kernel at WD_P = 160 / WD_K / WD_NB / WD_NH / WD_NHUM, <36, 4> and <36, 1> at p = 160
    wide161      one pair more: <48, 4> and <48, 1> with the small tree solver
    deepwide     five FK rounds in the throughput kernel, <36, 4> and <36, 1>
    tree48       <48, 4> with the large tree solver at K = 16, P = 264; <48, 1> dense
    two_chains   <48, 1> dense, five FK rounds, 40 hinges, depth 19, P = 332
    at_abi_caps  <48, 1> dense at K = 16, P = 384
    bodies48     <48, 1> dense with 48 bodies

Every launch is S = 3 streams of T = 6 frames.  A robot that does not decompose is served by <48, 1> whatever shape is
requested; both requests run.  The one-wavefront shape of a case that fits the throughput kernel needs GMR_IK_NO_WIDE at
solver creation and runs in ONE child process for all such cases (tests/ik_capacity_child.py).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ik_capacity as ic
import ik_variants as iv

pytestmark = pytest.mark.gpu

SHAPES_AGREE = 1e-12            # as test_launch_shapes_agree: the same algorithm in another launch shape
ERR_TOL = 1e-12                 # as test_per_frame_errors, per unit of the residual norm (norms here reach 10)

CASE_SHAPES = [(n, s) for n in ic.case_names() for s in iv.shapes_of(ic.all_cases()[n])]


@pytest.fixture(scope="module")
def hip():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


@pytest.fixture(scope="module")
def onewave(hip, tmp_path_factory):
    """The child's results: {"<case>/<input>/<q | ns | st | err>[2]": array}."""
    out = tmp_path_factory.mktemp("ikc") / "onewave.npz"
    env = dict(os.environ, GMR_IK_NO_WIDE="1")
    run = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ik_capacity_child.py"), str(out)],
                         env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    return dict(np.load(out))


_results = {}


def _launch(hip, onewave, c, shape, inp):
    """(q, ns, st, err) of two launches of (case, shape, input), computed once."""
    key = (c.name, shape, inp)
    if key not in _results:
        if shape == "onewave":
            _results[key] = [tuple(onewave[f"{c.name}/{inp}/{f}{tag}"] for f in ("q", "ns", "st", "err")) for tag in ("", "2")]
        else:
            human, q0 = ic.make_input(c, inp)
            sol = hip.Solver(c.mb, c.ts)
            sol.set_waves(4 if shape == "latency" else 1)
            runs = []
            for _ in range(2):
                q, ns, st, _, err = sol.retarget_streams(q0, human, want_errors=True)
                runs.append((q, ns, st, err))
            sol.close()
            _results[key] = runs
    return _results[key]


def _stage_errors(oracle, c, q, human):
    tgt = oracle.preprocess(c.ts, human)
    return np.array([[[oracle.stage_error(c.mb, c.ts, stage, q[s, t], tgt[s, t])[1] for stage in (0, 1)]
                      for t in range(q.shape[1])] for s in range(q.shape[0])])


@pytest.mark.parametrize("name,shape", CASE_SHAPES)
def test_capacity_case_matches_oracle(hip, oracle, onewave, name, shape):
    """Status 0, the oracle's solve counts, q within the derived tolerance of the case and input, and error1 / error2 of
    every frame equal to the oracle's stage errors at the kernel's own output."""
    c = ic.all_cases()[name]
    for inp in c.inputs:
        q_o, ns_o, st_o, _ = ic.oracle_run(oracle, c, inp)
        assert (st_o == 0).all()
        q, ns, st, err = _launch(hip, onewave, c, shape, inp)[0]
        tag = f"{name} {shape} {inp}"
        assert (st == 0).all(), (tag, st)
        dev = float(np.abs(q - q_o).max())
        print(f"{tag}: max |q - q_oracle| = {dev:.3e} (tolerance {c.tol(inp):g})")
        assert np.array_equal(ns, ns_o), f"{tag}: solve counts differ from the oracle's"
        assert dev <= c.tol(inp), (tag, dev)
        exp = _stage_errors(oracle, c, q, ic.make_input(c, inp)[0])
        d = float((np.abs(err - exp) / np.maximum(1.0, exp)).max())
        print(f"{tag}: max |error - oracle stage error| / max(1, error) = {d:.3e}")
        assert d <= ERR_TOL, (tag, d)


@pytest.mark.parametrize("name,shape", CASE_SHAPES)
def test_two_launches_give_the_same_bytes(hip, onewave, name, shape):
    c = ic.all_cases()[name]
    for inp in c.inputs:
        a, b = _launch(hip, onewave, c, shape, inp)
        for x, y, what in zip(a, b, ("q", "nsolve", "status", "errors")):
            assert x.tobytes() == y.tobytes(), (name, shape, inp, what)


@pytest.mark.parametrize("name", ["wide160", "deepwide"])
def test_throughput_kernel_and_one_wavefront_instance_agree(hip, onewave, name):
    """The neighbours at p = 160: the throughput kernel and <36, 1> (and <36, 4>) are the same algorithm: equal solve counts,
    q equal to 1e-12."""
    c = ic.all_cases()[name]
    for inp in c.inputs:
        q_w, ns_w = _launch(hip, onewave, c, "throughput", inp)[0][:2]
        for other in ("onewave", "latency"):
            q_1, ns_1 = _launch(hip, onewave, c, other, inp)[0][:2]
            d = float(np.abs(q_w - q_1).max())
            print(f"{name} {inp}: max |q_throughput - q_{other}| = {d:.3e}")
            assert np.array_equal(ns_w, ns_1), (inp, other)
            assert d <= SHAPES_AGREE, (inp, other, d)


def test_one_pair_more_lands_in_class_48(hip, oracle, onewave):
    """wide161 is wide160 with one pair more: the LDS report is class 48's instead of class 36's, and the result is that
    of its OWN oracle run."""
    a, b = ic.all_cases()["wide160"], ic.all_cases()["wide161"]
    sol_a, sol_b = hip.Solver(a.mb, a.ts), hip.Solver(b.mb, b.ts)
    assert sol_a.lds_bytes == a.expect["smem"][1] and sol_b.lds_bytes == b.expect["smem"][1]
    sol_a.close()
    sol_b.close()
    q_b = _launch(hip, onewave, b, "throughput", "scatter5")[0][0]
    assert np.abs(q_b - ic.oracle_run(oracle, b, "scatter5")[0]).max() <= b.tol("scatter5")


@pytest.mark.parametrize("name", ["deepwide", "two_chains"])
def test_fifth_fk_round_residuals(hip, oracle, name):
    """GMR_FLAG_EVAL_ONLY at bent configurations: no solve, so nothing can absorb a wrong body pose.  error1 / error2 hold
    the residuals of the tasks on bodies with 16 and more ancestors, which only the fifth pointer-jumping round completes;
    displacing just those bodies by 1 cm moves the norm by 4e-4 and more (test_deep_tasks_matter_to_the_oracle)."""
    c = ic.all_cases()[name]
    q, human = ic.eval_input(c)
    tgt = oracle.preprocess(c.ts, human)
    exp = np.array([[[oracle.stage_error(c.mb, c.ts, stage, q[s], tgt[s, 0])[1] for stage in (0, 1)]] for s in range(ic.S)])
    for shape in iv.shapes_of(c)[:2]:
        sol = hip.Solver(c.mb, c.ts)
        sol.set_waves(4 if shape == "latency" else 1)
        q_h, ns, st, tg, err = sol.retarget_streams(q, human, flags=hip.FLAG_EVAL_ONLY, want_targets=True, want_errors=True)
        sol.close()
        assert (st == 0).all() and (ns == 0).all() and np.abs(q_h[:, 0] - q).max() <= 1e-15
        assert np.abs(tg - tgt).max() <= 1e-14
        d = float((np.abs(err - exp) / np.maximum(1.0, exp)).max())
        print(f"{name} {shape}: max |error - oracle stage error| / max(1, error) = {d:.3e} (errors {exp.min():.3f} .. {exp.max():.3f})")
        assert d <= ERR_TOL, (shape, d)


@pytest.mark.parametrize("name", ["deepwide", "two_chains"])
def test_deep_tasks_steer_the_solve(hip, oracle, onewave, name):
    """The same launch with the weights of the tasks on the deep bodies at zero matches ITS oracle run and is far from the
    weighted result: the parity of the weighted run is a statement about those bodies' poses, not about the others'."""
    c = ic.all_cases()[name]
    z = ic.without_deep_tasks(c)
    human, q0 = ic.make_input(c, "scatter5")
    q_zo, ns_zo, st_zo, _ = oracle.retarget_streams_audit(z.mb, z.ts, q0, human)
    assert (st_zo == 0).all()
    tol = iv.derive_tolerance(ic.BASE_TOL["scatter5"], ic.noise_deviation(oracle, z.mb, z.ts, q0, human) / ic.g1_noise_deviation(oracle, "scatter5"))
    for shape in iv.shapes_of(c)[:2]:
        sol = hip.Solver(z.mb, z.ts)
        sol.set_waves(4 if shape == "latency" else 1)
        q_z, ns_z, st_z = sol.retarget_streams(q0, human)
        sol.close()
        assert (st_z == 0).all() and np.array_equal(ns_z, ns_zo), shape
        dev = float(np.abs(q_z - q_zo).max())
        far = float(np.abs(q_z - _launch(hip, onewave, c, shape, "scatter5")[0][0]).max())
        print(f"{name} {shape}: deep weights zero: max |q - q_oracle| = {dev:.3e} (tolerance {tol:g}), max |q - q_weighted| = {far:.3e}")
        assert dev <= tol, (shape, dev)
        assert far > 1e-3, (shape, far)


def test_task_set_at_the_abi_limits_is_served(hip, oracle, onewave):
    """K = 16, P = 384 on a robot that does not decompose: created, served by <48, 1> under either request with the same
    bytes, and the LDS report names the layout that runs."""
    c = ic.all_cases()["at_abi_caps"]
    sol = hip.Solver(c.mb, c.ts)
    assert sol.lds_bytes == ic.SMEM_48_1
    sol.close()
    for inp in c.inputs:
        a = _launch(hip, onewave, c, "latency", inp)[0]
        b = _launch(hip, onewave, c, "throughput", inp)[0]
        assert (a[2] == 0).all()
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), inp
    for name in ("two_chains", "bodies48", "tree48"):
        d = ic.all_cases()[name]
        sol = hip.Solver(d.mb, d.ts)
        assert sol.lds_bytes == (d.expect["smem"][1] if d.expect["tree_ok"] else ic.SMEM_48_1), name
        sol.close()
