"""CPU: the reference of the body-weight tests is fit for its job, the Python side checks its arguments before the device, and
the staging of the weight array moves the right bytes.

tests/body_weight_mirror.py is vel_limit_mirror's loop with the task weights multiplied by one multiplier per (frame, human
body), missing bodies (multiplier 0) out of the targets and out of the residual norm.  Shown here: with weights of ones that
loop IS oracle.retarget_streams; on every case of tests/test_ik_body_weights.py the oracle's active-set solver and the kernels'
pivoting (bpp_mirror.bpp_solve) agree to 1e-12 with equal solve counts and no stop decision is closer than 1e-6 to its tolerance
(device and mirror differ by about 1e-14, so equal solve counts on the device are a fair demand); a frame whose bodies are all
missing leaves q where it is with one solve per stage.

Figures of the cases (bpp solver; every case runs the seed it was given, none had to be replaced):

    case                 |q_bpp - q_active_set|  rounds  margin   |q - q_unweighted|  solve counts that differ
    w_g1                       3.7e-13              3    2.2e-5        3.16                 27 of 48
    w_g1 ground                1.4e-13              4    3.4e-5        3.18                 28 of 48
    w_t1                       2.3e-14              2    5.9e-5        0.76                  9 of 16
    w_t1 ground                4.8e-14              2    6.7e-5        0.76                 10 of 16
    w_dense                    1.0e-13              1    8.4e-5        0.94                  6 of 16
    w_g1_heights               9.3e-14              3    8.7e-6        3.13                 27 of 48
    w_g1_both                  4.4e-16              5    9.7e-5        0.40                 31 of 48
"""
import os
import subprocess

import numpy as np
import pytest

import body_weight_mirror as bw
from conftest import ROOT
from general_motion_retargeting_amd import _lib

SOLVERS_AGREE = 1e-12
MIN_MARGIN = 1e-6                # tests/test_ik_frame_limits_host.py

VARIANTS = [(n, g) for n in bw.CASES for g in ((False, True) if n in bw.GROUND_CASES else (False,))]


@pytest.mark.parametrize("name,ground", VARIANTS)
def test_case_is_fit_for_the_device_comparison(oracle, name, ground):
    case = bw.CASES[name]
    bpp, act = bw.mirror_runs(oracle, case, "bpp", ground), bw.mirror_runs(oracle, case, "oracle", ground)
    (q_b, ns_b), (q_a, ns_a) = bw.stacked(bpp), bw.stacked(act)
    d = float(np.abs(q_b - q_a).max())
    margin = min(min(r.margin for r in bpp), min(r.margin for r in act))
    q_u, ns_u = bw.stacked(bw.mirror_runs(oracle, case, "bpp", ground, weight=np.ones_like(bw.make_weights(case, ground))))
    print(f"{name} ground={ground}: |q_bpp - q_active_set| = {d:.2e}, at most {max(max(r.rounds) for r in bpp)} rounds, smallest stop margin "
          f"{margin:.2e}, |q - q_unweighted| = {np.abs(q_b - q_u).max():.2f}, {int((ns_b != ns_u).sum())} of {ns_b.size} solve counts differ")
    assert np.array_equal(ns_b, ns_a)
    assert d <= SOLVERS_AGREE, d
    assert margin >= MIN_MARGIN, margin
    assert (ns_b > 0).all()
    # a kernel that ignored the array could not pass: the weights move the result and the iteration counts
    assert np.abs(q_b - q_u).max() > 0.1 and (ns_b != ns_u).any()


def test_weights_of_a_case_are_the_stated_pattern():
    case = bw.CASES["w_g1"]
    m, mg = bw.make_weights(case), bw.make_weights(case, ground=True)
    nh = int(bw.setup_of(case.robot).ts["nhuman"][0])
    assert m.shape == (case.S, case.T, nh) and set(np.unique(m)) == set(bw.LEVELS)
    assert np.array_equal(m, bw.LEVELS[np.random.default_rng(100 + case.seed).choice(4, size=m.shape, p=(0.3, 0.2, 0.3, 0.2))])
    feet = np.nonzero(bw.setup_of(case.robot).ts["is_foot"][0][:nh])[0]
    assert len(feet) >= 2 and (mg[..., feet] != 0).any(axis=-1).all()
    changed = np.argwhere(m != mg)
    assert all(b == feet[0] and (m[s, t, feet] == 0).all() for s, t, b in changed)


@pytest.mark.parametrize("name", ["w_g1", "w_t1", "w_dense", "w_g1_heights"])
def test_ones_are_the_oracle(oracle, name):
    """weights of ones: the copy of the task set is the task set, nothing is missing, and the loop with the oracle's solver
    returns oracle.retarget_streams bit for bit (qpos and solve counts), stream by stream with its own task set, both ground
    variants where the robot has feet."""
    case = bw.CASES[name]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    ones = np.ones_like(bw.make_weights(case))
    for ground in ((False, True) if name in bw.GROUND_CASES else (False,)):
        runs = bw.mirror_runs(oracle, case, "oracle", ground, weight=ones)
        for s, ts in enumerate(bw.stream_tasksets(case)):
            q_o, ns_o, st_o = oracle.retarget_streams(su.mb, ts, q0[s:s + 1], human[s:s + 1], offset_to_ground=ground)
            assert st_o[0] == 0
            assert np.array_equal(runs[s].nsolve, ns_o[0]) and np.array_equal(runs[s].q, q_o[0]), (name, ground, s)


@pytest.mark.parametrize("solver", ["bpp", "oracle"])
def test_a_frame_with_every_body_missing_is_a_plain_damped_solve(oracle, solver):
    case = bw.CASES["w_g1"]
    w = np.array(bw.make_weights(case))
    w[:, 2] = 0.0
    for r in bw.mirror_runs(oracle, case, solver, weight=w):
        assert np.abs(r.q[2] - r.q[1]).max() == 0.0 and r.nsolve[2].tolist() == [1, 1] and (r.err[2] == 0.0).all()


def test_missing_rows_do_not_reach_the_mirror(oracle):
    """the mirror sets the missing rows to NaN itself: garbage there changes nothing"""
    case = bw.CASES["w_t1"]
    su = bw.setup_of(case.robot)
    human, q0 = bw.make_input(case)
    w = bw.make_weights(case)
    junk = bw.with_missing_rows(case, human, w, 1e300)
    assert not np.array_equal(junk, human)
    for s in range(case.S):
        a = bw.retarget_stream(oracle, su.mb, su.ts, q0[s], human[s], w[s])
        b = bw.retarget_stream(oracle, su.mb, su.ts, q0[s], junk[s], w[s])
        assert a.q.tobytes() == b.q.tobytes() and np.array_equal(a.nsolve, b.nsolve)


# ---- argument checks that need no device ----------------------------------------------------------------------------------------------
class _NoDevice:
    """stands in for the library: any call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def _fake_solver(nq=36, nhuman=14):
    sol = _lib.Solver.__new__(_lib.Solver)
    sol.handle, sol.nq, sol.nhuman = None, nq, nhuman
    return sol


def test_check_weights():
    assert _lib.check_weights(None, 3, 2, 14) is None
    a = _lib.check_weights(np.ones((3, 2, 14), dtype=np.float32)[:, :, ::1], 3, 2, 14)
    assert a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (3, 2, 14)
    assert _lib.check_weights(np.zeros((3, 2, 14), dtype=int), 3, 2, 14).dtype == np.float64
    for bad in (np.ones((2, 2, 14)), np.ones((3, 2, 13)), np.ones((3, 14)), np.ones(84)):
        with pytest.raises(ValueError, match=r"\[3,2,14\]"):
            _lib.check_weights(bad, 3, 2, 14)
    for v in (-1.0, np.nan, np.inf, -np.inf):
        w = np.ones((3, 2, 14))
        w[2, 1, 5] = v
        with pytest.raises(ValueError, match="stream 2, frame 1, body 5"):
            _lib.check_weights(w, 3, 2, 14)
    with pytest.raises(TypeError):
        _lib.check_weights(np.full((3, 2, 14), "a"), 3, 2, 14)
    # rows at or beyond a stream's length are padding: not looked at
    w = np.ones((3, 2, 14))
    w[0, 1, 5] = np.nan
    assert _lib.check_weights(w, 3, 2, 14, lens=np.array([1, 2, 2], np.int32)) is not None
    with pytest.raises(ValueError, match="stream 0, frame 1, body 5"):
        _lib.check_weights(w, 3, 2, 14, lens=np.array([2, 2, 2], np.int32))


def test_weights_are_checked_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())
    sol = _fake_solver()
    human, q0 = np.zeros((3, 2, 14, 7)), np.zeros((3, 36))
    with pytest.raises(ValueError, match=r"\[3,2,14\]"):
        sol.retarget_streams(q0, human, weights=np.ones((3, 14)))
    w = np.ones((3, 2, 14))
    w[1, 0, 3] = -0.5
    with pytest.raises(ValueError, match="stream 1, frame 0, body 3"):
        sol.retarget_streams(q0, human, weights=w)
    with pytest.raises(ValueError, match="job 0: weights: stream 1, frame 0, body 3"):
        _lib.retarget_group([{"solver": sol, "human": human, "q0": q0, "weights": w}])
    with pytest.raises(ValueError, match="one entry per job"):
        _lib.retarget_group_dev([(sol, 3, 2) + (None,) * 6], weights=[None, None])


def test_python_argument_errors_raise_before_any_library_call(monkeypatch):
    from general_motion_retargeting_amd import GeneralMotionRetargeting, chunking, dataset
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())
    g = GeneralMotionRetargeting(*bw.G1[:2], actual_human_height=bw.G1[2])
    names = g.human_body_names
    nh = len(names)
    row = g.body_weight_row({names[1]: 0.0, names[2]: 2.5})
    assert row.shape == (nh,) and row[1] == 0.0 and row[2] == 2.5 and row.sum() == nh - 2 + 2.5
    assert g.body_weight_row(None) is None
    with pytest.raises(KeyError):
        g.body_weight_row({"no_such_body": 1.0})
    for bad in ({names[1]: -1.0}, {names[1]: np.nan}, {names[1]: np.inf}, np.ones(nh + 1)):
        with pytest.raises(ValueError):
            g.body_weight_row(bad)
    frames = np.zeros((4, nh, 7))
    with pytest.raises(ValueError, match="chunk"):
        g.retarget_clip(frames, chunk="auto", body_weights=np.ones((4, nh)))
    with pytest.raises(ValueError, match=rf"\[1,4,{nh}\]"):
        g.retarget_clip(frames, body_weights=np.ones((3, nh)))
    with pytest.raises(ValueError, match="one dict per frame"):
        g.retarget_clip([{}] * 4, body_weights=[{}] * 3)
    with pytest.raises(ValueError, match="chunk"):
        dataset.retarget_clips(*bw.G1[:2], [frames], [30.0], chunk=chunking.ChunkSpec(frames=100), body_weights=[np.ones((4, nh))])
    with pytest.raises(ValueError, match="body_weights for 1 clips"):
        dataset.ClipRetargeter(*bw.G1[:2])([frames], [30.0], body_weights=[None, None])
    assert g._solver is None


def test_a_frame_may_lack_a_task_body_only_with_weight_zero():
    from general_motion_retargeting_amd import GeneralMotionRetargeting, synth
    g = GeneralMotionRetargeting(*bw.G1[:2], actual_human_height=bw.G1[2])
    human, _ = bw.make_input(bw.CASES["w_g1"])
    hd = synth.streams_to_dicts(g._tables, human[0])[0]
    task_bodies = [n for n in g._tables.stages[0].human_names if n != g.human_root_name]
    gone = task_bodies[0]
    lacking = {n: v for n, v in hd.items() if n != gone}
    with pytest.raises(KeyError, match=gone):
        g.pack_frame(dict(lacking))
    with pytest.raises(KeyError, match=gone):
        g.pack_frame(dict(lacking), g.body_weight_row({gone: 0.5}))
    frame = g.pack_frame(dict(lacking), g.body_weight_row({gone: 0.0}))
    assert np.isnan(frame[g.human_body_names.index(gone)]).all()
    no_root = {n: v for n, v in hd.items() if n != g.human_root_name}
    with pytest.raises(KeyError, match=g.human_root_name):
        g.pack_frame(no_root, g.body_weight_row({g.human_root_name: 0.0}))


def test_body_weights_from_missing():
    import general_motion_retargeting_amd as gmr
    h = np.zeros((2, 3, 5, 7))
    h[0, 1, 2, 6] = np.nan
    h[1, 2, 4, 0] = np.inf
    w = gmr.body_weights_from_missing(h)
    assert w.shape == (2, 3, 5) and w.dtype == np.float64 and w.sum() == 28 and w[0, 1, 2] == 0 and w[1, 2, 4] == 0
    assert gmr.body_weights_from_missing(h[0, 1]).tolist() == [1, 1, 0, 1, 1]
    with pytest.raises(ValueError):
        gmr.body_weights_from_missing(np.zeros((3, 6)))


def test_packer_drop_mode_needs_no_device():
    from general_motion_retargeting_amd import GeneralMotionRetargeting
    from general_motion_retargeting_amd.utils import optitrack
    g = GeneralMotionRetargeting("fbx", "unitree_g1", actual_human_height=1.6)
    pk = optitrack.RigidBodyPacker(g)
    ids = np.arange(1, 52)
    pos, rot = np.random.default_rng(0).normal(size=(51, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (51, 1))
    frame = pk.pack(ids, pos, rot)
    f2, w = pk.pack(ids, pos, rot, missing="drop")
    assert np.array_equal(frame, f2, equal_nan=True) and (w == 1).all()
    gone = [r for r in pk._required if r != pk._root][0]
    keep = ids != 1 + optitrack.FBX_SKELETON_NAMES.index(pk.names[gone])
    with pytest.raises(KeyError, match=pk.names[gone]):
        pk.pack(ids[keep], pos[keep], rot[keep])
    f3, w3 = pk.pack(ids[keep], pos[keep], rot[keep], missing="drop")
    assert w3[gone] == 0 and w3.sum() == len(w3) - 1 and np.isnan(f3[gone]).all()
    no_root = ids != 1 + optitrack.FBX_SKELETON_NAMES.index(pk.names[pk._root])
    with pytest.raises(KeyError, match=pk.names[pk._root]):
        pk.pack(ids[no_root], pos[no_root], rot[no_root], missing="drop")
    with pytest.raises(ValueError, match="missing"):
        pk.pack(ids, pos, rot, missing="skip")
    with pytest.raises(ValueError, match="missing"):
        optitrack.StreamingRetargeter(g, missing="skip")
    assert g._solver is None


def test_signatures_and_header():
    new = ["gmr_retarget_streams_weighted", "gmr_retarget_streams_weighted_dev", "gmr_retarget_group_weighted_dev",
           "gmr_retarget_group_weighted_window_dev", "gmr_retarget_group_weighted"]
    assert set(new) <= set(_lib._SIGS) and set(new) <= set(_lib.EXPORTED_SYMBOLS)
    import abi_header
    hdr = abi_header.read()
    for sym in new:
        assert abi_header.parameters(hdr, sym) == _lib._SIGS[sym][1], sym
    # the _scaled pair plus one pointer in front of the flags; the group entry points plus one behind njobs
    assert len(_lib._SIGS["gmr_retarget_streams_weighted"][1]) == len(_lib._SIGS["gmr_retarget_streams_scaled"][1]) + 1
    assert len(_lib._SIGS["gmr_retarget_group_weighted_window_dev"][1]) == len(_lib._SIGS["gmr_retarget_group_window_dev"][1]) + 1


@pytest.mark.parametrize("sanitize", [False, True])
def test_weight_array_carve_slices_and_windows(tmp_path, sanitize):
    """csrc/gmr_ik_weight_stage.h on literal values, as a stand-alone program (plain, and under AddressSanitizer + UBSan): the
    carve of the weight array in front of a job's arrays, its slice copies and its strided window copies applied with memcpy,
    for a job with the array and for one without."""
    name = "ik_weight_stage_check"
    exe = str(tmp_path / (name + ("_asan" if sanitize else "")))
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    if sanitize:      # is the sanitizer runtime there at all?  Asked with a trivial program, so that an error of the check itself is not skipped
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        pc = subprocess.run(["g++", "-std=c++17"] + extra + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
        if pc.returncode != 0:
            pytest.skip("sanitizer runtime not available: " + pc.stderr[-200:])
    cc = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "cpp", name + ".cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0 and "warning" not in cc.stderr, cc.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok" and "runtime error" not in out.stderr and "ERROR" not in out.stderr, (out.stdout, out.stderr[-2000:])
