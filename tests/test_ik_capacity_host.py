"""CPU side of tests/test_ik_capacity.py: what the host code decides for every case of tests/ik_capacity.py (sizes, size
class, decomposition, throughput-kernel fit, LDS bytes of both launch shapes), which kernel instances the device cases
reach, that their inputs are fit for a comparison with the oracle, the tolerances that follow from the oracle's own
sensitivity, what really bounds a task set (the LDS of the 4-wavefront layout of a robot that decomposes; nothing but
the ABI limits for one that does not), and that one past every ABI limit is refused."""
import ctypes as C
import itertools
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ik_capacity as ic
import ik_variants as iv
from test_ik_variants_host import MIN_MARGIN

NAMES = ic.case_names()


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = tmp_path_factory.mktemp("ikc")
    exes = {}
    for name in ("layout_check", "tree_dump"):
        exes[name], cc = iv.build_cpp(d, name)
        assert cc.returncode == 0, cc.stderr
    count = itertools.count()

    def run(name, mb, ts):
        blob = d / f"blob{next(count)}.bin"
        iv.write_blob(blob, mb, ts)
        return subprocess.run([exes[name], str(blob)], capture_output=True, text=True)
    return run


def _dump(tools, mb, ts):
    out = tools("tree_dump", mb, ts)
    assert out.returncode == 0, out.stderr
    return iv.parse_tree_dump(out.stdout)


@pytest.mark.parametrize("name", NAMES)
def test_expected_table(tools, name):
    """Every number of ik_capacity.EXPECT is what csrc/gmr_ik_layout.h and gmr_ik_wide_layout.h compute, and the packed
    blobs say the same."""
    c = ic.all_cases()[name]
    d = _dump(tools, c.mb, c.ts)
    got = dict(nbody=d["tree_nbody"], nhinge=d["tree_nhinge"], maxd=d["tree_maxd"], nhop=d["tree_nhop"], K=tuple(d["K"]),
               P=tuple(d["P"]), nhuman=d["tree_nhuman"], cls=d["tree_class"], tree_ok=d["tree_ok"], tree_small=d["tree_small"],
               wide_fits=d["tree_wide_fits"], smem=(d["tree_smem1"], d["tree_smem4"]))
    exp = dict(c.expect)
    assert got == exp, (got, exp)
    assert int(c.mb["nbody"][0]) == exp["nbody"] and int(c.mb["nhinge"][0]) == exp["nhinge"]
    assert int(c.mb["depth"][0].max()) + 1 == exp["maxd"] and exp["nhop"] == int(np.ceil(np.log2(exp["maxd"])))
    assert tuple(int(x) for x in c.ts["ntask"][0]) == exp["K"] and tuple(int(x) for x in c.ts["npair"][0]) == exp["P"]
    assert int(c.ts["nhuman"][0]) == exp["nhuman"]
    # the layout that runs fits the LDS: the one-wavefront one always, the 4-wavefront one where the robot decomposes
    assert got["smem"][0] <= ic.LDS_LIMIT
    if exp["tree_ok"]:
        assert exp["smem"][1] <= ic.LDS_LIMIT
    if not exp["tree_ok"]:
        assert exp["smem"][0] == ic.SMEM_48_1


def test_cases_sit_on_the_edges():
    """The point of the cases: exactly at, and exactly one past, the capacities."""
    from general_motion_retargeting_amd import ik_config
    E = ic.EXPECT
    w = E["wide160"]
    assert (w["nbody"], w["nhinge"], w["K"], w["P"], w["nhuman"]) == (40, 30, (16, 16), (160, 160), 16)   # WD_NB, WD_NH, WD_K, WD_P, WD_NHUM
    assert E["wide161"]["P"] == (161, 161) and E["wide161"]["cls"] == 48 and w["cls"] == 36
    assert E["deepwide"]["maxd"] == 17 and E["deepwide"]["nhop"] == 5 and E["deepwide"]["wide_fits"] == 1
    assert E["two_chains"]["maxd"] == ik_config.MAX_DEPTH and E["two_chains"]["nhinge"] == ik_config.MAX_HINGES
    a = E["at_abi_caps"]
    assert a["P"] == (ik_config.MAX_PAIRS,) * 2 and a["K"] == (ik_config.MAX_TASKS,) * 2 and a["nhuman"] == ik_config.MAX_HUMAN
    assert E["bodies48"]["nbody"] == ik_config.MAX_BODIES
    assert E["tree48"]["tree_ok"] == 1 and E["tree48"]["tree_small"] == 0 and E["tree48"]["K"] == (16, 16)


@pytest.mark.parametrize("name", ic.served())
def test_layout_check_passes(tools, name):
    """tests/cpp/layout_check.cpp (schedules for 64 and 192 lanes, decomposition, LDS layouts, throughput-kernel tables)
    on every case that is served."""
    c = ic.all_cases()[name]
    out = tools("layout_check", c.mb, c.ts)
    assert out.returncode == 0, out.stderr
    e = c.expect
    assert out.stdout.startswith(f"ok nv={e['nhinge'] + 6} tree={e['tree_ok']} "), out.stdout
    assert f" lds1={e['smem'][0]} " in out.stdout, out.stdout


def test_layout_code_is_clean_under_sanitizers_at_the_capacities(tmp_path):
    """The stand-alone AddressSanitizer + UBSan build of layout_check over every case: the host-side builders write the
    last slot of every region of the class-36, class-48 and throughput-kernel images here."""
    exe, cc = iv.build_cpp(tmp_path, "layout_check", sanitize=True)
    if cc.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + cc.stderr[-200:])

    def run(item):
        i, name = item
        c = ic.all_cases()[name]
        blob = tmp_path / f"blob{i}.bin"
        iv.write_blob(blob, c.mb, c.ts)
        return name, subprocess.run([exe, str(blob)], capture_output=True, text=True)
    with ThreadPoolExecutor(max_workers=4) as pool:
        for name, out in pool.map(run, enumerate(ic.served())):
            assert out.returncode == 0 and "runtime error" not in out.stderr and "ERROR" not in out.stderr, (name, out.stderr[-2000:])


def test_device_cases_reach_the_instances_at_their_edges(tools):
    """The instances no earlier test reaches: the throughput kernel at WD_P / WD_K / WD_NB / WD_NH / WD_NHUM and with five
    FK rounds; <36, 1> and <36, 4> at p = 160; <48, 4> with the large tree solver at K = 16; <48, 1> dense with five FK
    rounds, at 48 bodies and at P = 384."""
    reached = {}
    for name, c in ic.all_cases().items():
        d = _dump(tools, c.mb, c.ts)
        for shape in iv.shapes_of(c):
            reached.setdefault(iv.instance(d, shape), []).append(f"{name}/{shape}")
    assert {"wide160/throughput", "deepwide/throughput"} == set(reached["wide"])
    assert {"wide160/onewave", "deepwide/onewave"} == set(reached["<36,1,TREE_SMALL>"])
    assert {"wide160/latency", "deepwide/latency"} == set(reached["<36,4,TREE_SMALL>"])
    assert reached["<48,4,TREE>"] == ["tree48/latency"]
    assert reached["<48,4,TREE_SMALL>"] == ["wide161/latency"] and reached["<48,1,TREE_SMALL>"] == ["wide161/throughput"]
    dense = set(reached["<48,1,DENSE>"])
    assert {"two_chains/latency", "two_chains/throughput", "at_abi_caps/latency", "at_abi_caps/throughput", "bodies48/latency",
            "bodies48/throughput", "tree48/throughput"} == dense


@pytest.mark.parametrize("name", NAMES)
def test_oracle_solves_every_case_away_from_the_stop_threshold(oracle, name):
    """Conditions on the INPUTS of the device cases, from the oracle alone: status 0 on every frame; the stop rule's
    smallest margin is at least MIN_MARGIN, so a kernel that differs by rounding takes the same number of solves; and at
    least half of the (frame, stage) runs end by the rule -- for one that ran into max_iter + 1 solves the margin says
    nothing.  The table of ik_capacity.py holds the same figures."""
    c = ic.all_cases()[name]
    k = int(c.ts["max_iter"][0])
    for inp in c.inputs:
        q, ns, st, mg = ic.oracle_run(oracle, c, inp)
        assert (st == 0).all(), (inp, st)
        margin, frac = float(mg[..., 0].min()), ic.stopped_by_rule(c, ns)
        print(f"{name} {inp}: smallest stop-rule margin {margin:.3e}, stopped by the rule {frac:.3f}, mean solves {ns.mean():.2f} of {k + 1}")
        assert margin >= MIN_MARGIN, (inp, margin)
        assert (ns >= 1).all() and (ns <= k + 1).all()
        assert frac >= 0.5, (inp, frac)
        rec = ic.MEASURED[name][inp]
        assert abs(margin - rec[0]) <= 0.01 * rec[0] and abs(frac - rec[1]) <= 1e-3, (inp, margin, frac, rec)


def test_derived_tolerances_follow_the_oracle(oracle):
    """The tolerances of ik_capacity.MEASURED, recomputed: the deviation under qp_noise = 1e-11 (seeds 1..3) relative to the
    shipped G1's on the same kind of input, through ik_variants.derive_tolerance."""
    for name, c in ic.all_cases().items():
        for inp in c.inputs:
            ratio = ic.amplification(oracle, c, inp)
            rec = ic.MEASURED[name][inp]
            print(f"{name} {inp}: amplification {ratio:.2f}, tolerance {rec[3]:g}")
            assert rec[3] == iv.derive_tolerance(ic.BASE_TOL[inp], ratio) <= iv.TOL_CAP, (name, inp, ratio)
            assert abs(ratio - rec[2]) <= 0.02 * rec[2] + 0.01, (name, inp, ratio, rec[2])


@pytest.mark.parametrize("name", ["deepwide", "two_chains"])
def test_deep_tasks_matter_to_the_oracle(oracle, name):
    """The five-hop device tests rest on two facts about the INPUT: the residual norm at the start configuration moves by
    far more than its tolerance when only the bodies deeper than 16 are displaced (what an FK that stopped after four
    rounds would do to them), and the solve with the deep tasks' weights at zero is a sound input whose result is far from
    the weighted one."""
    c = ic.all_cases()[name]
    deep = ic.deep_bodies(c)
    assert len(deep) >= 1 and set(ic.deep_tasks(c)) and int(c.mb["depth"][0][deep].min()) >= 16
    q, human = ic.eval_input(c)
    tgt = oracle.preprocess(c.ts, human)
    mb = c.mb.copy()
    mb["body_pos"][0][deep] += 0.01
    for stage in (0, 1):
        E = [oracle.stage_error(m, c.ts, stage, q[s], tgt[s, 0])[1] for s in range(ic.S) for m in (c.mb, mb)]
        d = np.abs(np.array(E[0::2]) - np.array(E[1::2]))
        print(f"{name} stage {stage + 1}: the residual norm moves by {d.min():.3e} .. {d.max():.3e}")
        assert d.min() > 1e-6, d
    z = ic.without_deep_tasks(c)
    hq = ic.make_input(c, "scatter5")
    qz, ns, st, mg = oracle.retarget_streams_audit(z.mb, z.ts, hq[1], hq[0])
    assert (st == 0).all() and mg[..., 0].min() >= MIN_MARGIN and ic.stopped_by_rule(z, ns) >= 0.5
    far = float(np.abs(qz - ic.oracle_run(oracle, c, "scatter5")[0]).max())
    print(f"{name}: max |q(deep weights = 0) - q| = {far:.3e}")
    assert far > 1e-3, far


# ---- the real capacity ------------------------------------------------------------------------------------------------
def _placements():
    """Task placements on the largest robot the tree solver takes: K = 16 on 16 different bodies.  The schedule of the
    4-wavefront layout grows with the terms of H, that is with how many tasks share how many dofs: all tasks deep in the
    limbs (tree48 itself), all in one limb plus the trunk, spread evenly, with and without position weights, and
    random draws."""
    bodies = ic.tree_extreme_bodies()                          # base, w0..w3, la0..la7, ra0.., ll0.., rl0..
    limb = {p: [f"{p}{i}" for i in range(8)] for p in ("la", "ra", "ll", "rl")}
    out = {"tips4x4": [b for p in limb for b in limb[p][4:]]}
    out["two_limbs"] = limb["la"] + limb["ra"]
    out["trunk_and_tips"] = ["base", "w0", "w1", "w2", "w3"] + limb["la"][5:] + limb["ra"][5:] + limb["ll"][5:] + limb["rl"][6:]
    out["one_limb_deep"] = limb["la"] + limb["ra"][6:] + limb["ll"][5:] + limb["rl"][5:]
    out["tips_5_5_3_3"] = limb["la"][3:] + limb["ra"][3:] + limb["ll"][5:] + limb["rl"][5:]
    rng = np.random.default_rng(0)
    for i in range(12):
        out[f"random{i}"] = [bodies[j] for j in sorted(rng.choice(len(bodies), 16, replace=False))]
    return out


def test_tree_capable_extreme_fits_the_lds_for_every_placement(tools):
    """Host test of the real bound: trunk 10, limbs 8, K = 16.  P is at most 16 * 18 = 288 by construction (a task lists
    the 6 base dofs, the 4 waist hinges and one limb); over the sweep the 4-wavefront layout stays under the limit, the
    largest being the figure quoted in include/gmr_types.h."""
    worst = (0, None, None)
    for tag, frames in _placements().items():
        assert len(set(frames)) == 16, tag
        for weights in ("pos", "mixed"):
            tasks = [(f, (50 if weights == "pos" or i % 2 == 0 else 0), 10) for i, f in enumerate(frames)]
            model, tt, mb, ts = ic.tree_extreme(tasks)
            d = _dump(tools, mb, ts)
            assert d["tree_ok"] == 1 and d["tree_small"] == 0 and d["tree_class"] == 48 and d["K"] == [16, 16], (tag, d)
            assert max(d["P"]) <= 288
            assert d["tree_smem1"] == ic.SMEM_48_1
            assert d["tree_smem4"] <= ic.LDS_LIMIT, (tag, weights, d["tree_smem4"])
            worst = max(worst, (d["tree_smem4"], tag, max(d["P"])))
    print(f"largest 4-wavefront layout of the sweep: {worst[0]} B ({worst[1]}, P = {worst[2]}) of {ic.LDS_LIMIT}")
    assert worst[0] == ic.TREE_EXTREME_SMEM4, worst


def test_a_robot_that_does_not_decompose_is_bounded_by_the_abi_alone(tools):
    """Its only layout is the one-wavefront one of class 48, whose size does not depend on the task set: 66 112 B at
    P = 332 and at P = 384 alike, while the 4-wavefront layout it never runs would need more than the LDS."""
    for name in ("two_chains", "at_abi_caps", "bodies48"):
        e = ic.EXPECT[name]
        assert e["tree_ok"] == 0 and e["smem"][0] == ic.SMEM_48_1 <= ic.LDS_LIMIT
    assert ic.EXPECT["at_abi_caps"]["smem"][1] > ic.LDS_LIMIT


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ic.OVER_LIMIT)
def test_one_past_each_limit_is_refused_when_packing(which):
    bodies, tasks, nhuman = ic.over_limit(which)
    with pytest.raises(ValueError):
        ic.build("over", bodies, tasks, nhuman)


BLOB_EDITS = {
    "P=385": ("ts", lambda t: t["npair"].__setitem__((0, 0), 385), "npair out of range"),
    "K=17": ("ts", lambda t: t["ntask"].__setitem__((0, 1), 17), "ntask out of range"),
    "nhuman=17": ("ts", lambda t: t["nhuman"].__setitem__(0, 17), "nhuman/human_root out of range"),
    "depth=20": ("mb", None, "depth["),
    "nbody=49": ("mb", lambda m: m["nbody"].__setitem__(0, 49), "nbody out of range"),
    "nhinge=41": ("mb", lambda m: m["nhinge"].__setitem__(0, 41), "nhinge out of range"),
}


@pytest.mark.parametrize("which", ic.OVER_LIMIT)
def test_library_refuses_a_blob_one_past_each_limit(which):
    """validate() of gmr_solver_create runs before the device is looked for: a valid blob edited by one to each limit's
    first refused value answers GMR_ERR_ARG with the matching message, on a machine without a GPU too."""
    from general_motion_retargeting_amd import _lib
    try:
        L = _lib.lib()
    except (OSError, _lib.GmrHipError) as e:
        pytest.skip(f"the library does not load here: {e}")
    c = ic.all_cases()["two_chains"]                           # depth 19, 40 hinges: every field one below its refusal
    mb, ts = c.mb.copy(), c.ts.copy()
    what, edit, message = BLOB_EDITS[which]
    if which == "depth=20":
        tip = int(np.argmax(mb["depth"][0]))
        assert mb["depth"][0][tip] == 19
        mb["depth"][0][tip] = 20
    else:
        edit(mb if what == "mb" else ts)
    h = C.c_void_p()
    rc = L.gmr_solver_create(mb.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p), C.byref(h))
    msg = L.gmr_last_error().decode()
    assert rc == -1 and not h.value, (rc, msg)                 # GMR_ERR_ARG
    assert message in msg, msg
