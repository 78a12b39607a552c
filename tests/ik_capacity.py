"""Robots and task sets at the compile-time capacities of the IK kernels, for tests/test_ik_capacity_host.py (CPU) and
tests/test_ik_capacity.py (GPU).

The capacities: include/gmr_types.h (48 bodies, 40 hinges, depth below 20, 16 tasks and 16 human bodies per stage, 384
(task, dof) pairs per stage), csrc/gmr_ik_layout.h (`ik_caps`: classes 28 / 32 / 36 hold 160 pairs, class 48 the ABI
limits) and csrc/gmr_ik_wide_layout.h (WD_NB = 40, WD_NH = 30, WD_K = 16, WD_P = 160, WD_NHUM = 16).  Every case is a
synthetic MJCF robot built like `_synthetic_robot` of tests/test_gpu_parity.py, extended by bodies without a joint:

  wide160      trunk = base + 2 waist hinges, four limbs of 7 hinges on the second waist body, two jointless leaves on
               every limb tip and a jointless head: 40 bodies, 30 hinges, 16 tasks, 16 human bodies, P = 160 in both
               stages -- every capacity of the throughput kernel and of class 36 at once
  wide161      the same robot, one rotation-only task moved one body down its limb: P = 161, the first task set that
               class 36 and the throughput kernel do not hold
  deepwide     the same trunk; one limb carries a jointless body after every hinge, so that its last body is the 17th
               on its path: the FK's fifth pointer-jumping round (nhop = 5) in the throughput kernel and in class 36
  tree48       4 waist hinges and four limbs of 8 hinges (trunk 10, limbs 8: the large tree solver), 16 tasks
  two_chains   two chains of 19 hinges and one of 2: 40 hinges, depth 19, 16 tasks, P = 332, does not decompose
  at_abi_caps  a chain of 18 hinges with 16 hinged leaves at its tip and a chain of 6: K = 16 and P = 384 exactly
  bodies48     two_chains plus 7 jointless leaves: 48 bodies

Weights follow `_synthetic_robot`: the second table has position weight 2w + 1 and rotation weight max(w / 2, 1), but a
zero position weight stays zero in both tables (such a task lists no base-translation pair, ik_config.pack_taskset).

EXPECT states, per case, what the host code is to decide; tests/test_ik_capacity_host.py recomputes every number of it
from the headers (tests/cpp/tree_dump.cpp, layout_check.cpp).  MEASURED holds what the oracle gives on the cases'
inputs (S = 3, T = 6): the smallest stop-rule margin, the fraction of frames a stage ends by the rule rather than at
max_iter + 1 solves, the amplification of rounding-sized noise relative to the shipped G1 on the same kind of input,
the tolerance that follows (ik_variants.derive_tolerance) and the largest deviation seen on an MI355X.
"""
import dataclasses

import numpy as np

import ik_variants as iv

S, T = 3, 6
LDS_LIMIT = 160 * 1024 - 1024                       # what gmr_solver_create allows a workgroup
SMEM_48_1 = 66112                                   # the one-wavefront layout of class 48: no schedule in LDS, so no
                                                    # dependence on the task set

# input kinds: the smooth synthetic streams; the same plus the 5 cm scatter of test_generic_topologies (some joints end
# on their limits); the far scatter of ik_variants.scatter (targets outside the reachable set).  The 5 cm kind counts as
# smooth input: the shipped G1 moves by 1.4e-11 under rounding-sized noise on smooth input, by 3.5e-11 with the 5 cm
# scatter and by 3.9e-10 with the far one (g1_noise_deviation below), so it gets the base of 1e-9, not the 1e-8 of
# scattered input.
BASE_TOL = {"smooth": 1e-9, "scatter5": 1e-9, "scatter": 1e-8}
INPUTS = {"wide160": ("smooth", "scatter5", "scatter"), "tree48": ("smooth", "scatter5", "scatter")}
DEFAULT_INPUTS = ("smooth", "scatter5")


def _limb(prefix, parent, n, pos, interleave=False):
    """n hinged bodies <prefix>0 .. below `parent`; interleave: a jointless body <prefix>{i}x after every hinge."""
    out = []
    for i in range(n):
        out.append((f"{prefix}{i}", parent, True, pos if i == 0 else "0.02 0 -0.09"))
        parent = f"{prefix}{i}"
        if interleave:
            out.append((f"{prefix}{i}x", parent, False, "0.01 0 -0.03"))
            parent = f"{prefix}{i}x"
    return out


def _leaves(names, parent, hinged=False):
    return [(n, parent, hinged, f"{0.03 * (i % 4 - 1.5):.3f} {0.02 * (i // 4 - 1.5):.3f} -0.04") for i, n in enumerate(names)]


def _wide_bodies():
    b = _limb("w", "base", 2, "0 0 0.1")
    for p, pos in (("la", "0 0.2 0.2"), ("ra", "0 -0.2 0.2"), ("ll", "0 0.1 -0.3"), ("rl", "0 -0.1 -0.3")):
        b += _limb(p, "w1", 7, pos) + _leaves([f"{p}f", f"{p}g"], f"{p}6")
    return b + [("head", "w1", False, "0 0 0.3")]


def _wide_tasks(moved):
    t = [("base", 100, 10), ("w1", 0, 10), ("head", 0, 10)]
    for p in ("la", "ra", "ll", "rl"):
        t += [(f"{p}6", 50, 10), (f"{p}3", 10, 5), (f"{p}1" if p == moved else f"{p}0", 0, 10)]
    return t + [("laf", 0, 5)]


def _deepwide():
    b = _limb("w", "base", 2, "0 0 0.1") + _limb("la", "w1", 7, "0 0.2 0.2", interleave=True)
    for p, pos in (("ra", "0 -0.2 0.2"), ("ll", "0 0.1 -0.3"), ("rl", "0 -0.1 -0.3")):
        b += _limb(p, "w1", 7, pos)
    t = [("base", 100, 10), ("w1", 0, 10), ("la6x", 50, 10), ("la3x", 10, 5), ("la1x", 0, 10)]
    for p in ("ra", "ll", "rl"):
        t += [(f"{p}6", 50, 10), (f"{p}3", 10, 5)]
    return b, t


def _tree48():
    b = _limb("w", "base", 4, "0 0 0.1")
    t = []
    for p, pos in (("la", "0 0.2 0.2"), ("ra", "0 -0.2 0.2"), ("ll", "0 0.1 -0.3"), ("rl", "0 -0.1 -0.3")):
        b += _limb(p, "w3", 8, pos)
        t += [(f"{p}{i}", w, 10) for i, w in ((7, 50), (6, 20), (5, 10), (4, 10))]
    return b, t


def _two_chains(extra_leaves=0):
    b = _limb("a", "base", 19, "0 0.1 0") + _limb("b", "base", 19, "0 -0.1 0") + _limb("c", "base", 2, "0 0 0.2")
    b += _leaves([f"x{i}" for i in range(extra_leaves)], "c1")
    t = [("base", 100, 10)] + [(f"a{i}", 50 if i == 18 else 10, 5) for i in range(18, 11, -1)]
    t += [(f"b{i}", 50 if i == 18 else 10, 5) for i in range(18, 10, -1)]
    return b, t


def _at_abi_caps(c_task="c2"):
    b = _limb("a", "base", 18, "0 0.1 0") + _leaves([f"f{i}" for i in range(16)], "a17", hinged=True)
    b += _limb("c", "base", 6, "0 -0.1 0")
    t = [(c_task, 100, 10)] + [(f"f{i}", 20, 5) for i in range(15)]
    return b, t


def _cases():
    return {
        "wide160": (_wide_bodies(), _wide_tasks(None)),
        "wide161": (_wide_bodies(), _wide_tasks("rl")),
        "deepwide": _deepwide(),
        "tree48": _tree48(),
        "two_chains": _two_chains(),
        "at_abi_caps": _at_abi_caps(),
        "bodies48": _two_chains(extra_leaves=7),
    }


# What the host code decides.  maxd = bodies on the longest root -> leaf path, nhop = ceil(log2(maxd)); smem = LDS bytes of
# (the one-wavefront layout, the 4-wavefront layout); a robot that does not decompose has no 4-wavefront layout: its smem4
# is what make_ik_layout would ask for, and may exceed LDS_LIMIT (at_abi_caps: the refusal before this table existed).
EXPECT = {
    "wide160":     dict(nbody=40, nhinge=30, maxd=11, nhop=4, K=(16, 16), P=(160, 160), nhuman=16, cls=36, tree_ok=1, tree_small=1, wide_fits=1, smem=(40624, 69040)),
    "wide161":     dict(nbody=40, nhinge=30, maxd=11, nhop=4, K=(16, 16), P=(161, 161), nhuman=16, cls=48, tree_ok=1, tree_small=1, wide_fits=0, smem=(66112, 94528)),
    "deepwide":    dict(nbody=38, nhinge=30, maxd=17, nhop=5, K=(11, 11), P=(126, 126), nhuman=11, cls=36, tree_ok=1, tree_small=1, wide_fits=1, smem=(40624, 69040)),
    "tree48":      dict(nbody=37, nhinge=36, maxd=13, nhop=4, K=(16, 16), P=(264, 264), nhuman=16, cls=48, tree_ok=1, tree_small=0, wide_fits=0, smem=(66112, 119104)),
    "two_chains":  dict(nbody=41, nhinge=40, maxd=20, nhop=5, K=(16, 16), P=(332, 332), nhuman=16, cls=48, tree_ok=0, tree_small=0, wide_fits=0, smem=(66112, 155968)),
    "at_abi_caps": dict(nbody=41, nhinge=40, maxd=20, nhop=5, K=(16, 16), P=(384, 384), nhuman=16, cls=48, tree_ok=0, tree_small=0, wide_fits=0, smem=(66112, 217408)),
    "bodies48":    dict(nbody=48, nhinge=40, maxd=20, nhop=5, K=(16, 16), P=(332, 332), nhuman=16, cls=48, tree_ok=0, tree_small=0, wide_fits=0, smem=(66112, 155968)),
}

# seed of synth.make_streams per case (the first, from 5 on, at which every input of the case meets the conditions of
# test_ik_capacity_host.py) and the standard deviation of the "scatter5" kind (0.05 unless more than half of the frames
# ran into max_iter + 1 solves with it)
SEED = {n: 5 for n in EXPECT}
SCATTER5 = {n: 0.05 for n in EXPECT}

# case -> input -> (smallest stop-rule margin, fraction of (frame, stage) that stop by the rule, amplification,
# tolerance, largest |q - q_oracle| seen on an MI355X over all shapes)
MEASURED = {
    "wide160":     {"smooth": (5.52e-05, 0.889, 1.98, 1e-08, 9.0e-15), "scatter5": (2.89e-04, 0.861, 1.38, 1e-08, 5.0e-15), "scatter": (2.33e-03, 0.611, 0.37, 1e-08, 2.7e-15)},
    "wide161":     {"smooth": (5.38e-06, 0.889, 2.02, 1e-08, 2.6e-14), "scatter5": (1.64e-05, 0.861, 1.38, 1e-08, 4.7e-15)},
    "deepwide":    {"smooth": (6.40e-05, 0.722, 8.78, 1e-08, 1.8e-14), "scatter5": (1.27e-04, 0.694, 3.63, 1e-08, 5.9e-15)},
    "tree48":      {"smooth": (3.21e-05, 0.972, 7.42, 1e-08, 3.3e-14), "scatter5": (4.51e-05, 0.806, 2.96, 1e-08, 1.1e-14), "scatter": (5.64e-04, 0.528, 0.25, 1e-08, 1.6e-15)},
    "two_chains":  {"smooth": (1.41e-04, 0.917, 6.91, 1e-08, 7.8e-14), "scatter5": (1.06e-04, 0.778, 3.27, 1e-08, 2.0e-14)},
    "at_abi_caps": {"smooth": (8.64e-05, 0.972, 6.50, 1e-08, 3.1e-14), "scatter5": (8.68e-05, 0.917, 2.87, 1e-08, 5.7e-15)},
    "bodies48":    {"smooth": (1.41e-04, 0.917, 6.91, 1e-08, 7.8e-14), "scatter5": (1.06e-04, 0.778, 3.27, 1e-08, 2.0e-14)},
}


@dataclasses.dataclass
class Case:
    name: str
    model: object
    tt: object
    mb: np.ndarray
    ts: np.ndarray
    tasks: list
    expect: dict
    seed: int
    ground: bool = False

    @property
    def inputs(self):
        return INPUTS.get(self.name, DEFAULT_INPUTS)

    def tol(self, inp):
        return MEASURED[self.name][inp][3]


def robot_xml(name, bodies):
    """MJCF text of `bodies` = [(name, parent, hinged, pos)], each parent listed before its children."""
    axes = ["1 0 0", "0 1 0", "0 0 1"]
    children = {}
    for i, (nm, parent, hinged, pos) in enumerate(bodies):
        children.setdefault(parent, []).append((i, nm, hinged, pos))

    def emit(parent):
        out = ""
        for i, nm, hinged, pos in children.get(parent, []):
            out += f'<body name="{nm}" pos="{pos}" quat="0.98 0.1 0.05 0.12">'
            if hinged:
                out += f'<joint name="j_{nm}" axis="{axes[(i + len(nm)) % 3]}" range="-1.3 1.1"/>'
            out += emit(nm) + "</body>"
        return out
    return ('<mujoco model="%s"><compiler angle="radian"/><worldbody><body name="base" pos="0 0 1"><freejoint/>%s'
            '</body></worldbody></mujoco>' % (name, emit("base")))


def task_config(tasks, nhuman=None):
    """The ik_config dict of `tasks` = [(frame, w_pos, w_rot)]; nhuman > len(tasks) adds unused human bodies."""
    names = [f"h{i}" for i in range(len(tasks))]
    tbl1 = {f: [h, wp, wr, [0.01, 0, 0], [1, 0, 0, 0]] for (f, wp, wr), h in zip(tasks, names)}
    tbl2 = {f: [h, wp * 2 + 1 if wp else 0, max(wr / 2, 1), [0, 0, 0], [1, 0, 0, 0]] for (f, wp, wr), h in zip(tasks, names)}
    scale = {n: 0.9 for n in names + [f"h{i}" for i in range(len(tasks), nhuman or 0)]}
    return {"robot_root_name": "base", "human_root_name": "h0", "ground_height": 0.0, "human_height_assumption": 1.8,
            "use_ik_match_table1": True, "use_ik_match_table2": True, "human_scale_table": scale,
            "ik_match_table1": tbl1, "ik_match_table2": tbl2}


def compile_robot(name, bodies):
    import os
    import tempfile
    from general_motion_retargeting_amd.mjcf import compile_mjcf
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, f"{name}.xml")
        with open(p, "w") as f:
            f.write(robot_xml(name, bodies))
        return compile_mjcf(p)


def build(name, bodies, tasks, nhuman=None):
    """(model, task tables, packed model, packed task set); raises what pack_model / pack_taskset raise."""
    from general_motion_retargeting_amd.ik_config import build_task_tables, pack_model, pack_taskset
    model = compile_robot(name, bodies)
    tt = build_task_tables(task_config(tasks, nhuman), 1.7)
    return model, tt, pack_model(model), pack_taskset(model, tt)


_all = None


def all_cases():
    global _all
    if _all is None:
        _all = {}
        for name, (bodies, tasks) in _cases().items():
            model, tt, mb, ts = build(name, bodies, tasks)
            mb.setflags(write=False)
            ts.setflags(write=False)
            _all[name] = Case(name, model, tt, mb, ts, tasks, EXPECT[name], SEED[name])
    return _all


def case_names():
    return list(EXPECT)


def served():
    """Every case runs on the device (at_abi_caps since gmr_solver_create builds the 4-wavefront layout only for a robot
    that decomposes)."""
    return case_names()


def tree_extreme(tasks):
    """The largest robot the tree solver takes (trunk 10 = base + 4 waist hinges, four limbs of 8) under `tasks`."""
    return build("tree_extreme", _tree48()[0], tasks)


def tree_extreme_bodies():
    return ["base"] + [b[0] for b in _tree48()[0]]


# ---- refusals: one past each ABI limit -------------------------------------------------------------------------------
def over_limit(which):
    """(bodies, tasks, nhuman) of a robot / task set one past the limit `which`."""
    if which == "P=385":
        return (*_at_abi_caps("c3"), None)
    if which == "K=17":
        b, t = _tree48()
        return b, t + [("w3", 10, 5)], None
    if which == "nhuman=17":
        return (*_tree48(), 17)
    if which == "depth=20":
        return _limb("a", "base", 20, "0 0.1 0"), [("base", 100, 10), ("a19", 50, 10)], None
    if which == "nbody=49":
        return _leaves([f"x{i}" for i in range(48)], "base"), [("base", 100, 10), ("x3", 50, 10)], None
    if which == "nhinge=41":
        b = _limb("a", "base", 11, "0 0.1 0")
        for p in "bcd":
            b += _limb(p, "base", 10, "0 -0.1 0")
        return b, [("base", 100, 10), ("a10", 50, 10)], None
    raise KeyError(which)


OVER_LIMIT = ("P=385", "K=17", "nhuman=17", "depth=20", "nbody=49", "nhinge=41")


# ---- inputs and oracle runs, computed once -----------------------------------------------------------------------------
_inputs, _runs = {}, {}


def make_input(c, inp, seed=None, sigma=None):
    """(human, q0) of a case: synth.make_streams with the case's own tables, read-only and shared."""
    from general_motion_retargeting_amd import synth
    seed = c.seed if seed is None else seed
    sigma = SCATTER5[c.name] if sigma is None else sigma
    key = (c.name, inp, seed, sigma)
    if key not in _inputs:
        human, q0 = synth.make_streams(c.model, c.tt, S, T, seed=seed)
        if inp == "scatter5":
            rng = np.random.default_rng(1)
            human[..., :3] += rng.normal(0, sigma, size=human[..., :3].shape)
        elif inp == "scatter":
            human = iv.scatter(human)
        human.setflags(write=False)
        q0.setflags(write=False)
        _inputs[key] = (human, q0)
    return _inputs[key]


def oracle_run(oracle, c, inp, seed=None, sigma=None):
    """(q, nsolve, status, margins) of retarget_streams_audit without noise, read-only."""
    human, q0 = make_input(c, inp, seed, sigma)
    key = (c.name, inp, seed, sigma)
    if key not in _runs:
        out = oracle.retarget_streams_audit(c.mb, c.ts, q0, human)
        for a in out:
            a.setflags(write=False)
        _runs[key] = out
    return _runs[key]


def noise_deviation(oracle, mb, ts, q0, human):
    """max over the noise seeds of |q(qp_noise) - q| (ik_variants.noise_deviation on any input)."""
    q = oracle.retarget_streams_audit(mb, ts, q0, human)[0]
    return max(float(np.abs(oracle.retarget_streams_audit(mb, ts, q0, human, qp_noise=iv.NOISE, seed=s)[0] - q).max())
               for s in iv.NOISE_SEEDS)


_g1_base = {}


def g1_noise_deviation(oracle, inp):
    """The same quantity for the shipped G1 (ik_variants.BASE) on the same kind of input, S = 3, T = 6, seed 5."""
    if inp not in _g1_base:
        from general_motion_retargeting_amd import synth
        from conftest import get_setup
        su = get_setup(*iv.BASE)
        human, q0 = synth.make_streams(su.model, su.tt, S, T, seed=iv.SEED)
        if inp == "scatter5":
            human[..., :3] += np.random.default_rng(1).normal(0, 0.05, size=human[..., :3].shape)
        elif inp == "scatter":
            human = iv.scatter(human)
        _g1_base[inp] = noise_deviation(oracle, su.mb, su.ts, q0, human)
    return _g1_base[inp]


def amplification(oracle, c, inp):
    human, q0 = make_input(c, inp)
    return noise_deviation(oracle, c.mb, c.ts, q0, human) / g1_noise_deviation(oracle, inp)


def stopped_by_rule(c, ns):
    """Fraction of (frame, stage) solves counts below max_iter + 1: stages that ended by the stop rule."""
    return float((ns < int(c.ts["max_iter"][0]) + 1).mean())


# ---- five FK rounds: the bodies only the fifth round reaches ---------------------------------------------------------------
def deep_bodies(c):
    """Bodies with 16 or more ancestors: after four pointer-jumping rounds a body holds the product of its last 16 path
    transforms, so these are the ones the fifth round completes."""
    return np.nonzero(c.mb["depth"][0][: int(c.mb["nbody"][0])] >= 16)[0]


def deep_tasks(c, stage=0):
    deep = set(int(b) for b in deep_bodies(c))
    return [k for k in range(int(c.ts["ntask"][0][stage])) if int(c.ts["task_body"][0][stage][k]) in deep]


def eval_input(c):
    """(q[S, nq], human[S, 1, nhuman, 7]) for GMR_FLAG_EVAL_ONLY: bent configurations (every hinge off zero, so that a deep
    body's pose depends on each of its ancestors' joints) under the first frames of the scatter5 input."""
    human, q0 = make_input(c, "scatter5")
    rng = np.random.default_rng(11)
    q = q0.copy()
    q[:, 7:] = rng.uniform(-0.9, 0.9, size=q[:, 7:].shape)
    q[:, :3] += rng.normal(0, 0.05, size=(S, 3))
    quat = rng.normal(size=(S, 4))
    q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    return q, np.ascontiguousarray(human[:, :1])


_without = {}


def without_deep_tasks(c):
    """The case with both weights of every task on a deep body set to zero in both stages (the pairs stay listed)."""
    if c.name not in _without:
        ts = c.ts.copy()
        for stage in (0, 1):
            for k in deep_tasks(c, stage):
                ts["w_pos"][0][stage][k] = ts["w_rot"][0][stage][k] = 0.0
        ts.setflags(write=False)
        _without[c.name] = dataclasses.replace(c, name=c.name + "/no_deep", ts=ts)
    return _without[c.name]


# the largest 4-wavefront layout over the task placements of test_tree_capable_extreme_fits_the_lds_for_every_placement
TREE_EXTREME_SMEM4 = 119104
