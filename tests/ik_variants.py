"""Task sets and solver parameters off the shipped line, for tests/test_ik_variants_host.py (CPU) and
tests/test_ik_variants.py (GPU).

Everything is built on smplx -> unitree_g1 at height 1.7 from the shipped config dict: a STAGE variant edits a deep copy
of the dict and goes through build_task_tables / pack_taskset; a PARAMETER variant copies the packed blob of the
shipped tables and sets one field.  The expected (use1, K, P, size class, wide_fits) of every variant is stated here
and checked on the CPU against what csrc/gmr_ik_layout.h computes; so is which kernel instance a launch request ends
in (`instance`), a restatement of gmr_retarget_streams_dev / gmr_launch_ik_streams.
"""
import copy
import dataclasses
import math

import numpy as np

from conftest import get_setup

BASE = ("smplx", "unitree_g1", 1.7)
S, T, SEED = 4, 8, 5

LEFT_ARM = ("left_shoulder_yaw_link", "left_elbow_link", "left_wrist_yaw_link")
LEGS = ("left_hip_roll_link", "left_knee_link", "left_toe_link", "right_hip_roll_link", "right_knee_link", "right_toe_link")

# Tolerances on max |q_gpu - q_oracle|.  BASE_TOL is the project's established pair: 1e-9 on smooth input, 1e-8 on the
# scattered input of test_ik_bound_path._scatter.  It holds wherever the regularisation is at least the default one
# (tol, max_iter, limit_gain, ground_offset, timestep, damping >= 0.5, every stage structure).  Where it is weaker the
# tolerance is DERIVED FROM THE ORACLE ALONE (test_ik_variants_host.py::test_derived_tolerances_follow_the_oracle):
#   amplification = max over seeds 1..3 of |q(qp_noise = 1e-11) - q|  /  the same quantity for the shipped parameters
#   tolerance     = BASE_TOL * max(1, amplification) rounded up to a power of ten, at most 1e-7  (contract: 1e-4)
# Amplification measured with S=4, T=8, seed=5 on the CPU (noise seeds 1..3), and the tolerance that follows:
#   damping=0.05      0.99   -> 1e-9
#   damping=0.25      0.99   -> 1e-9
#   lm_damping=0.1    0.69   -> 1e-9
#   lm_damping=10.0   8.37   -> 1e-8
# (the same ratio for the variants that keep BASE_TOL: 0.77 .. 2.9, the largest for max_iter=0 and no_legs_1)
BASE_TOL = {"smooth": 1e-9, "scatter": 1e-8}
TOL_CAP = 1e-7
DERIVED_TOL = {"damping=0.05": 1e-9, "damping=0.25": 1e-9, "lm_damping=0.1": 1e-9, "lm_damping=10.0": 1e-8}
NOISE, NOISE_SEEDS = 1e-11, (1, 2, 3)

# the queued-dispatch test: more streams than resident wavefronts, tiled from QUEUED_BASE generated ones
QUEUED = ("no_left_arm_2", "lm_damping=0.1")
QUEUED_BASE, QUEUED_S, QUEUED_T = 24, 2600, 5


def derive_tolerance(base, amplification):
    """BASE_TOL * max(1, amplification), rounded up to a power of ten and capped (the rule above)."""
    decades = math.ceil(math.log10(max(1.0, float(amplification))) - 1e-12)
    return min(TOL_CAP, float(f"1e{round(math.log10(base)) + decades}"))


@dataclasses.dataclass
class Variant:
    name: str
    kind: str                      # "param" | "stage"
    model: object
    tt: object
    mb: np.ndarray
    ts: np.ndarray
    inp: str = "smooth"            # "smooth" | "scatter"
    ground: bool = False           # FLAG_OFFSET_TO_GROUND
    seed: int = SEED
    expect: dict = None            # stage variants: use0, use1, K, P, cls, wide_fits
    changes_output: bool = True    # parameter variants: the oracle's output differs from the shipped parameters'

    @property
    def derived(self):
        return self.name in DERIVED_TOL

    @property
    def tol(self):
        return DERIVED_TOL.get(self.name, BASE_TOL[self.inp])


def scatter(human):
    """The scatter of test_ik_bound_path._scatter (targets far outside the reachable set), on a copy."""
    from general_motion_retargeting_amd import synth
    human = human.copy()
    rng = np.random.default_rng(0)
    human[..., :3] += rng.normal(0, 0.3, size=human[..., :3].shape)
    rv = rng.normal(0, 1.0, size=human.shape[:-1] + (3,))
    human[..., 3:] = synth.quat_mul(human[..., 3:], synth.rotvec_quat(rv))
    return human


_inputs = {}


def make_input(v, inp=None, S_=S, T_=T):
    """(human, q0) of a variant: synth.make_streams with the variant's OWN task tables, read-only and shared."""
    from general_motion_retargeting_amd import synth
    inp = inp or v.inp
    key = (v.name, inp, S_, T_)
    if key not in _inputs:
        human, q0 = synth.make_streams(v.model, v.tt, S_, T_, seed=v.seed)
        if inp == "scatter":
            human = scatter(human)
        human.setflags(write=False)
        q0.setflags(write=False)
        _inputs[key] = (human, q0)
    return _inputs[key]


# ---- stage structures -------------------------------------------------------------------------------------------------
def _raise_pos(table, least=5.0):
    for e in table.values():
        e[1] = max(float(e[1]), least)


def _edit_only1(c):
    c["use_ik_match_table2"] = False


def _edit_only2(c):
    c["use_ik_match_table1"] = False


def _edit_reorder2(c):
    c["ik_match_table2"] = dict(reversed(list(c["ik_match_table2"].items())))


def _edit_no_left_arm_2(c):
    for f in LEFT_ARM:
        del c["ik_match_table2"][f]


def _edit_no_legs_1(c):
    for f in LEGS:
        c["ik_match_table1"][f][1] = c["ik_match_table1"][f][2] = 0.0


def _edit_same(c):
    c["ik_match_table2"] = copy.deepcopy(c["ik_match_table1"])


def _edit_allpos1(c):
    _raise_pos(c["ik_match_table1"])


def _edit_sixteen(c):
    for t in ("ik_match_table1", "ik_match_table2"):
        tbl = c[t]
        _raise_pos(tbl)
        # two more tasks on bodies of the scale table; the offsets are those of the knee entries, so that the table-1
        # offsets of that human body stay what they were
        for side in ("left", "right"):
            knee = tbl[f"{side}_knee_link"]
            tbl[f"{side}_ankle_pitch_link"] = [f"{side}_knee", 5.0, 5.0, list(knee[3]), list(knee[4])]


STAGE_VARIANTS = {
    #  name            edit                  use0 use1  K         P           class wide_fits
    "only1":         (_edit_only1,         dict(use0=1, use1=0, K=(14, 14), P=(124, 154), cls=36, wide_fits=1)),
    "only2":         (_edit_only2,         dict(use0=0, use1=1, K=(14, 14), P=(124, 154), cls=36, wide_fits=1)),
    "reorder2":      (_edit_reorder2,      dict(use0=1, use1=1, K=(14, 14), P=(124, 154), cls=36, wide_fits=1)),
    "no_left_arm_2": (_edit_no_left_arm_2, dict(use0=1, use1=1, K=(14, 11), P=(124, 113), cls=36, wide_fits=1)),
    "no_legs_1":     (_edit_no_legs_1,     dict(use0=1, use1=1, K=(8, 14), P=(76, 154), cls=36, wide_fits=1)),
    "same":          (_edit_same,          dict(use0=1, use1=7, K=(14, 14), P=(124, 124), cls=36, wide_fits=1)),
    "allpos1":       (_edit_allpos1,       dict(use0=1, use1=3, K=(14, 14), P=(157, 154), cls=36, wide_fits=1)),
    "sixteen":       (_edit_sixteen,       dict(use0=1, use1=7, K=(16, 16), P=(179, 179), cls=48, wide_fits=0)),
}

# ---- parameters: (field, value, input, ground flag) ---------------------------------------------------------------------
PARAM_VARIANTS = (
    [("damping", x, "smooth", False) for x in (0.05, 0.25, 4.0)]
    + [("lm_damping", x, "smooth", False) for x in (0.1, 10.0)]
    + [("tol", x, "smooth", False) for x in (1e-6, 1e-2, 0.1)]
    + [("max_iter", x, "smooth", False) for x in (0, 1, 3, 40)]
    + [("limit_gain", x, "scatter", False) for x in (0.3, 1.0)]      # on smooth input 1.0 equals 0.95 bit for bit
    + [("ground_offset", 0.25, "smooth", True)]                      # without the flag the field has no effect
)

_variants = None


def all_variants():
    """name -> Variant, in a fixed order; `default` (shipped tables and parameters) comes first."""
    global _variants
    if _variants is not None:
        return _variants
    from general_motion_retargeting_amd.ik_config import build_task_tables, pack_taskset
    su = get_setup(*BASE)
    out = {"default": Variant("default", "param", su.model, su.tt, su.mb, su.ts, changes_output=False)}
    for field, value, inp, ground in PARAM_VARIANTS:
        ts = su.ts.copy()
        ts[field] = value
        name = f"{field}={value}"
        out[name] = Variant(name, "param", su.model, su.tt, su.mb, ts, inp=inp, ground=ground)
    mb = su.mb.copy()
    mb["timestep"] = su.mb["timestep"] / 2                           # the oracle's result is unchanged bit for bit
    out["timestep/2"] = Variant("timestep/2", "param", su.model, su.tt, mb, su.ts, changes_output=False)
    for name, (edit, expect) in STAGE_VARIANTS.items():
        cfg = copy.deepcopy(su.cfg)
        edit(cfg)
        tt = build_task_tables(cfg, BASE[2])
        out[name] = Variant(name, "stage", su.model, tt, su.mb, pack_taskset(su.model, tt), expect=expect)
    for v in out.values():
        v.ts.setflags(write=False)
        v.mb.setflags(write=False)
    _variants = out
    return out


def variant_names(kind=None):
    return [n for n, v in all_variants().items() if kind is None or v.kind == kind]


def default_for(v):
    """The shipped parameters under the input and ground flag of `v` (what a parameter variant is compared with)."""
    d = all_variants()["default"]
    return dataclasses.replace(d, name=f"default[{v.inp},{int(v.ground)}]", inp=v.inp, ground=v.ground, seed=v.seed)


# ---- which kernel a launch ends in --------------------------------------------------------------------------------------
SHAPES = ("latency", "throughput", "onewave")


def shapes_of(v):
    """Launch shapes a variant runs in.  A task set that does not fit the throughput kernel has no separate one-wave run:
    for it set_waves(1) already is <class, 1, ...>."""
    return ("latency", "throughput") if v.expect and not v.expect["wide_fits"] else SHAPES


def instance(dump, shape):
    """The kernel a request ends in, from tree_dump's fields: gmr_retarget_streams_dev takes the helper shape when the
    robot decomposes and four wavefronts are asked for, else the throughput kernel when the task set fits it and
    GMR_IK_NO_WIDE is unset, else the one-wavefront instance of the size class."""
    qp = "TREE_SMALL" if dump["tree_small"] else ("TREE" if dump["tree_ok"] else "DENSE")
    if shape == "latency" and dump["tree_ok"]:
        return f"<{dump['tree_class']},4,{qp}>"
    if shape == "throughput" and dump["tree_wide_fits"]:
        return "wide"
    return f"<{dump['tree_class']},1,{'TREE_SMALL' if dump['tree_small'] else 'DENSE'}>"


def write_blob(path, mb, ts):
    with open(path, "wb") as f:
        f.write(mb.tobytes())
        f.write(ts.tobytes())


def build_cpp(out_dir, name, sanitize=False):
    """Compile tests/cpp/<name>.cpp (plain C++ over the product headers); returns (exe, compiler result)."""
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(str(out_dir), name + ("_asan" if sanitize else ""))
    cmd = ["g++", "-O1", "-std=c++17", "-Wall"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cc = subprocess.run(cmd + ["-o", exe, os.path.join(ROOT, "tests", "cpp", name + ".cpp")], capture_output=True, text=True)
    return exe, cc


def parse_tree_dump(stdout):
    """tree_dump's line as a dict: `tree_*` fields are integers, every other field a list of integers."""
    kv = dict(w.split("=") for w in stdout.split())
    return {k: (int(v) if k.startswith("tree_") else [int(x) for x in v.split(",") if x]) for k, v in kv.items()}


# ---- the oracle on a variant's input, computed once -----------------------------------------------------------------------
_oracle_runs = {}


def oracle_run(oracle, v, inp=None, S_=S, T_=T):
    """(q, nsolve, status, margins) of retarget_streams_audit without noise (bit-equal to retarget_streams), read-only."""
    key = (v.name, inp or v.inp, v.ground, S_, T_)
    if key not in _oracle_runs:
        human, q0 = make_input(v, inp, S_, T_)
        out = oracle.retarget_streams_audit(v.mb, v.ts, q0, human, offset_to_ground=v.ground)
        for a in out:
            a.setflags(write=False)
        _oracle_runs[key] = out
    return _oracle_runs[key]


def noise_deviation(oracle, v):
    """max over the noise seeds of |q(qp_noise) - q| on the variant's input: how far rounding-sized perturbations of
    every QP solution move the result."""
    human, q0 = make_input(v)
    q = oracle_run(oracle, v)[0]
    return max(float(np.abs(oracle.retarget_streams_audit(v.mb, v.ts, q0, human, offset_to_ground=v.ground, qp_noise=NOISE,
                                                          seed=s)[0] - q).max()) for s in NOISE_SEEDS)
