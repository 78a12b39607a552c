"""CPU side of tests/test_ik_variants.py: what the host code decides for every variant of tests/ik_variants.py (stage
switches, tasks and pairs per stage, size class, throughput-kernel fit), which kernel instances the GPU cases reach, and
that the inputs of those cases are fit for a comparison at 1e-9: the oracle solves them with status 0, no stop decision
sits within 1e-7 of its threshold, every parameter variant really changes the result, and the tolerances of the weakly
regularised variants are what the oracle's own sensitivity to rounding-sized noise gives."""
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ik_variants as iv
from conftest import ALL_CONFIGS, get_setup

MIN_MARGIN = 1e-7


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("ikv")
    exes = {}
    for name in ("layout_check", "tree_dump"):
        exes[name], cc = iv.build_cpp(d, name)
        assert cc.returncode == 0, cc.stderr

    def run(name, mb, ts):
        blob = d / "blob.bin"
        iv.write_blob(blob, mb, ts)
        return subprocess.run([exes[name], str(blob)], capture_output=True, text=True)
    return run


def _dump(tools, mb, ts):
    out = tools("tree_dump", mb, ts)
    assert out.returncode == 0, out.stderr
    return iv.parse_tree_dump(out.stdout)


@pytest.mark.parametrize("name", iv.variant_names())
def test_layout_of_every_variant(tools, name):
    """layout_check (schedules, decomposition, LDS layout, stage flags) passes, and use0 / use1 / K / P / size class /
    wide_fits are the expected ones; a parameter variant keeps the shipped structure."""
    v = iv.all_variants()[name]
    exp = v.expect or dict(use0=1, use1=3, K=(14, 14), P=(124, 154), cls=36, wide_fits=1)
    out = tools("layout_check", v.mb, v.ts)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("ok") and "tree=1" in out.stdout and "limbs=4" in out.stdout, out.stdout
    assert out.stdout.strip().endswith(f" use1={exp['use1']}"), out.stdout
    d = _dump(tools, v.mb, v.ts)
    got = dict(use0=d["tree_use0"], use1=d["tree_use1"], K=tuple(d["K"]), P=tuple(d["P"]), cls=d["tree_class"],
               wide_fits=d["tree_wide_fits"])
    assert got == exp, (got, exp)
    assert d["tree_ok"] == 1 and d["tree_small"] == 1
    # the packed task set says the same
    assert tuple(int(x) for x in v.ts["ntask"][0]) == exp["K"] and tuple(int(x) for x in v.ts["npair"][0]) == exp["P"]
    assert tuple(int(x) for x in v.ts["use_stage"][0]) == (exp["use0"], int(exp["use1"] != 0))


def test_layout_code_is_clean_under_sanitizers_for_every_variant(tmp_path):
    """The stand-alone AddressSanitizer + UBSan build of layout_check (as test_host_cpp.py runs it over the shipped
    configurations) over every variant: class 48 with 179 pairs, a disabled first stage and stages of different size
    walk parts of the host-side builders that no shipped configuration reaches."""
    exe, cc = iv.build_cpp(tmp_path, "layout_check", sanitize=True)
    if cc.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + cc.stderr[-200:])
    def run(item):
        i, (name, v) = item
        blob = tmp_path / f"blob{i}.bin"
        iv.write_blob(blob, v.mb, v.ts)
        return name, subprocess.run([exe, str(blob)], capture_output=True, text=True)
    with ThreadPoolExecutor(max_workers=4) as pool:          # (the instrumented checker takes over a second per task set)
        for name, out in pool.map(run, enumerate(iv.all_variants().items())):
            assert out.returncode == 0 and "runtime error" not in out.stderr and "ERROR" not in out.stderr, (name, out.stderr[-2000:])


def test_gpu_cases_reach_every_kernel_instance(tools):
    """The union of the cases of tests/test_ik_variants.py: the helper shape of class 36, the throughput kernel, the
    one-wavefront instances of classes 28 / 32 / 36 (every shipped configuration under GMR_IK_NO_WIDE=1), and both shapes
    of class 48 with the small tree solver (`sixteen`: a full-size robot, not the 16-dof toy)."""
    reached = {}
    for name, v in iv.all_variants().items():
        d = _dump(tools, v.mb, v.ts)
        for shape in iv.shapes_of(v):
            reached.setdefault(iv.instance(d, shape), []).append(f"{name}/{shape}")
    for src, robot in ALL_CONFIGS:
        su = get_setup(src, robot, 1.7)
        d = _dump(tools, su.mb, su.ts)
        assert d["tree_wide_fits"] == 1, (src, robot)          # so set_waves(1) alone never leaves the throughput kernel
        reached.setdefault(iv.instance(d, "onewave"), []).append(f"{src}/{robot}/onewave")
    want = {"<36,4,TREE_SMALL>", "wide", "<28,1,TREE_SMALL>", "<32,1,TREE_SMALL>", "<36,1,TREE_SMALL>", "<48,1,TREE_SMALL>",
            "<48,4,TREE_SMALL>"}
    assert want <= set(reached), sorted(want - set(reached))
    assert reached["<48,1,TREE_SMALL>"] == ["sixteen/throughput"] and reached["<48,4,TREE_SMALL>"] == ["sixteen/latency"]


@pytest.mark.parametrize("name", iv.variant_names())
def test_oracle_solves_every_variant_away_from_the_stop_threshold(oracle, name):
    """A condition on the INPUTS of the GPU cases, over all frames: status 0, and the stop rule's smallest margin is at
    least 1e-7 -- a kernel that differs from the oracle by rounding takes the same number of iterations."""
    v = iv.all_variants()[name]
    q, ns, st, mg = iv.oracle_run(oracle, v)
    assert (st == 0).all(), st
    print(f"{name}: smallest stop-rule margin {mg[..., 0].min():.3e}")
    assert mg[..., 0].min() >= MIN_MARGIN, float(mg[..., 0].min())
    enabled = v.ts["use_stage"][0] != 0
    assert (ns[..., ~enabled] == 0).all() and (ns[..., enabled] >= 1).all()
    k = int(v.ts["max_iter"][0])
    assert (ns <= k + 1).all()


def test_oracle_margins_of_the_further_gpu_inputs(oracle):
    """The same condition for the inputs of the other GPU tests: every shipped configuration (S=3, T=6, scattered), the
    base streams of the queued-dispatch test, and the scattered / grounded runs of the shipped parameters."""
    from general_motion_retargeting_amd import synth
    worst = np.inf
    for src, robot in ALL_CONFIGS:
        su = get_setup(src, robot, 1.7)
        human, q0 = synth.make_streams(su.model, su.tt, 3, 6, seed=iv.SEED)
        q, ns, st, mg = oracle.retarget_streams_audit(su.mb, su.ts, q0, iv.scatter(human))
        assert (st == 0).all() and mg[..., 0].min() >= MIN_MARGIN, (src, robot, float(mg[..., 0].min()))
        worst = min(worst, mg[..., 0].min())
    V = iv.all_variants()
    for name in iv.QUEUED:
        q, ns, st, mg = iv.oracle_run(oracle, V[name], S_=iv.QUEUED_BASE, T_=iv.QUEUED_T)
        assert (st == 0).all() and mg[..., 0].min() >= MIN_MARGIN, (name, float(mg[..., 0].min()))
        worst = min(worst, mg[..., 0].min())
    for name in ("limit_gain=0.3", "ground_offset=0.25"):
        q, ns, st, mg = iv.oracle_run(oracle, iv.default_for(V[name]))
        assert (st == 0).all() and mg[..., 0].min() >= MIN_MARGIN, (name, float(mg[..., 0].min()))
        worst = min(worst, mg[..., 0].min())
    print(f"smallest stop-rule margin {worst:.3e}")


@pytest.mark.parametrize("name", iv.variant_names("param"))
def test_parameter_variants_change_the_oracle_output(oracle, name):
    """A parameter whose variant gave the shipped parameters' result would test nothing.  Halving the model's timestep
    is the exception: velocity * dt is the same product, bit for bit."""
    v = iv.all_variants()[name]
    q = iv.oracle_run(oracle, v)[0]
    q_d = iv.oracle_run(oracle, iv.default_for(v))[0]
    d = float(np.abs(q - q_d).max())
    print(f"{name}: max |q - q_default| = {d:.3e}")
    if v.changes_output:
        assert d > 1e-4, d                       # far above every tolerance of the GPU cases
    else:
        assert np.array_equal(q, q_d)


def test_derived_tolerances_follow_the_oracle(oracle):
    """The tolerance table of ik_variants.py, recomputed: the deviation under qp_noise = 1e-11 relative to the shipped
    parameters' on the same input, through derive_tolerance.  The variants that keep the base tolerance are printed."""
    V = iv.all_variants()
    base = {}
    for name, v in V.items():
        key = (v.inp, v.ground)
        if key not in base:
            base[key] = iv.noise_deviation(oracle, iv.default_for(v))
        ratio = iv.noise_deviation(oracle, v) / base[key]
        print(f"{name}: amplification {ratio:.2f}, tolerance {v.tol:g}")
        if v.derived:
            assert v.tol == iv.derive_tolerance(iv.BASE_TOL[v.inp], ratio), (name, ratio)
        else:
            assert v.tol == iv.BASE_TOL[v.inp]
    assert {n for n, v in V.items() if v.derived} == {"damping=0.05", "damping=0.25", "lm_damping=0.1", "lm_damping=10.0"}


def test_derive_tolerance_rule():
    assert iv.derive_tolerance(1e-9, 0.7) == 1e-9 and iv.derive_tolerance(1e-9, 1.0) == 1e-9
    assert iv.derive_tolerance(1e-9, 8.4) == 1e-8 and iv.derive_tolerance(1e-9, 10.0) == 1e-8
    assert iv.derive_tolerance(1e-9, 11.0) == 1e-7 and iv.derive_tolerance(1e-9, 5000.0) == 1e-7
    assert iv.derive_tolerance(1e-8, 1.2) == 1e-7
