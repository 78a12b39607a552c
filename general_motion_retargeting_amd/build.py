"""Build libgmrhip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

Every source is compiled to its own object (cached under build/obj by source + header mtimes and flags), then
linked: editing one kernel file rebuilds that file only.  ``build_variant(name, defines)`` produces
``libgmrhip_<name>.so`` for A/B measurements through ``GMR_HIP_LIBRARY`` (diagnostic builds; never loaded by default).
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libgmrhip.so")
OBJ = os.path.join(os.path.dirname(HERE), "build", "obj")
SOURCES = ["gmr_ik.hip", "gmr_ik_wide.hip", "gmr_fk.hip", "gmr_post.hip", "gmr_smplx.hip", "gmr_bvh.hip", "gmr_chunk.hip", "gmr_motion.hip", "gmr_body_state.hip", "gmr_tracker.hip", "gmr_tracker_links.hip", "gmr_tracker_preview.hip", "gmr_tracker_adaptive.hip", "gmr_tracker_anchor.hip", "gmr_tracker_control.hip", "gmr_tracker_proprio.hip", "gmr_tracker_feet.hip", "gmr_tracker_commands.hip", "gmr_tracker_episode.hip", "gmr_tracker_rollout.hip", "gmr_tracker_loss.hip", "gmr_tracker_optim.hip", "gmr_tracker_policy.hip", "gmr_tracker_policy_bwd.hip", "gmr_comm.hip", "gmr_ik_host.hip", "gmr_abi.hip"]
HEADERS = ["gmr_ik_wide_item.inc", "gmr_ik_wide_kernels.inc", "gmr_device_math.h", "gmr_ik_layout.h", "gmr_ik_weight_stage.h", "gmr_ik_wide_layout.h", "gmr_ik_prof.h", "gmr_ik_tree.h",
           "gmr_fk_tree.h", "gmr_fk_walk.h", "gmr_fk_handle.h", "gmr_launch.h", "gmr_ik_stage.h", "gmr_motion_sample.h", "gmr_philox.h", "gmr_tracker_dev.h", "gmr_tracker_host.h", "gmr_tracker_policy_plan.h", "gmr_tracker_policy_bwd_plan.h", "gmr_terrain.h", "gmr_link_plan.h", "gmr_smplx_prog.h", "gmr_bvh_prog.h", "gmr_handles.h", "gmr_post.h", "gmr_internal.h", "gmr_workspace.h", "../../include/gmr_hip.h", "../../include/gmr_types.h"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC"]
# The throughput kernel must stay within 256 registers (two wavefronts per SIMD; since round 3: 168, three).  Machine-LICM hoists every FP64
# literal and lane predicate of the (fully inlined) frame loop into registers that live for the whole kernel; they
# then spill to scratch and are RELOADED inside the loop (99 spilled VGPRs, 336 B of scratch per lane).  Without it
# and with sinking enabled: 226 VGPRs, no scratch, +13 % frames/s (profiles/r02_*).
PER_SOURCE_FLAGS = {"gmr_ik_wide.hip": ["-mllvm", "-disable-machine-licm", "-mllvm", "-sink-insts-to-avoid-spills=1"]}


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (set HIPCC)")


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def _object(src: str, defines, force: bool, verbose: bool) -> str:
    os.makedirs(OBJ, exist_ok=True)
    per_source = [] if os.environ.get("GMR_BUILD_NO_PER_SOURCE_FLAGS") else PER_SOURCE_FLAGS.get(src, [])   # (A/B builds)
    defines = per_source + list(defines)
    tag = hashlib.sha1(" ".join(FLAGS + defines).encode()).hexdigest()[:10]
    obj = os.path.join(OBJ, f"{os.path.splitext(src)[0]}.{tag}.o")
    deps = [os.path.join(CSRC, src)] + [os.path.join(CSRC, h) for h in HEADERS]
    if force or verbose or not os.path.exists(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in deps):
        cmd = [_hipcc()] + FLAGS + list(defines) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            cmd.append("-Rpass-analysis=kernel-resource-usage")
        subprocess.check_call(cmd, cwd=CSRC)
    return obj


def _link(objs, out: str) -> str:
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out + ".tmp"] + objs + ["-ldl"])
    os.replace(out + ".tmp", out)
    return out


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    return _link([_object(s, [], force, verbose) for s in SOURCES], LIB)


# The test-only probe of gmr_device_math.h (tests/hip/math_probe.hip): one shared object per flag set the shipped library
# compiles that header under.  Libraries of their own -- nothing of the probe is linked into libgmrhip.so.
PROBE_SRC = os.path.join(os.path.dirname(HERE), "tests", "hip", "math_probe.hip")
PROBE_LIBS = {"flags": os.path.join(os.path.dirname(PROBE_SRC), "libgmr_math_probe.so"),
              "wide": os.path.join(os.path.dirname(PROBE_SRC), "libgmr_math_probe_wide.so")}


def _build_probe_libs(src: str, libs: dict, force: bool) -> dict:
    deps = [src, os.path.join(CSRC, "gmr_device_math.h"), os.path.abspath(__file__)]
    extra = {"flags": [], "wide": PER_SOURCE_FLAGS["gmr_ik_wide.hip"]}
    for name, out in libs.items():
        if force or not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call([_hipcc()] + FLAGS + extra[name] + ["-shared", "-o", out + ".tmp", src])
            os.replace(out + ".tmp", out)
    return dict(libs)


def build_probe(force: bool = False) -> dict:
    """Both probe libraries, rebuilt when the probe source or the header is newer (the libraries are cached on those mtimes)."""
    return _build_probe_libs(PROBE_SRC, PROBE_LIBS, force)


# The probe of se3_jlinv_coef5 / se3_jlinv_apply5 (tests/hip/jlinv_apply_probe.hip, tests/test_jlinv_apply.py): the same two flag sets.
JLINV_PROBE_SRC = os.path.join(os.path.dirname(PROBE_SRC), "jlinv_apply_probe.hip")
JLINV_PROBE_LIBS = {"flags": os.path.join(os.path.dirname(PROBE_SRC), "libgmr_jlinv_apply_probe.so"),
                    "wide": os.path.join(os.path.dirname(PROBE_SRC), "libgmr_jlinv_apply_probe_wide.so")}


def build_jlinv_probe(force: bool = False) -> dict:
    return _build_probe_libs(JLINV_PROBE_SRC, JLINV_PROBE_LIBS, force)


# The probe of the split evaluation (tests/hip/split_eval_probe.hip, tests/test_split_eval.py): the split forms of se3_log_rel5 /
# se3_jlinv_coef5 and the latency kernel's two walks, under the library's own flags.
SPLIT_PROBE_SRC = os.path.join(os.path.dirname(PROBE_SRC), "split_eval_probe.hip")
SPLIT_PROBE_LIB = os.path.join(os.path.dirname(PROBE_SRC), "libgmr_split_eval_probe.so")


def build_split_probe(force: bool = False) -> str:
    deps = [SPLIT_PROBE_SRC, os.path.abspath(__file__)] + [os.path.join(CSRC, h) for h in ["gmr_ik.hip"] + HEADERS]
    out = SPLIT_PROBE_LIB
    if force or not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call([_hipcc()] + FLAGS + ["-shared", "-o", out + ".tmp", SPLIT_PROBE_SRC])
        os.replace(out + ".tmp", out)
    return out


# The probe of the folded row broadcasts and of div_const (tests/hip/rowfma_probe.hip, tests/test_row_bcast_fma.py), under the
# library's own flags.
ROWFMA_PROBE_SRC = os.path.join(os.path.dirname(PROBE_SRC), "rowfma_probe.hip")
ROWFMA_PROBE_LIB = os.path.join(os.path.dirname(PROBE_SRC), "libgmr_rowfma_probe.so")


def build_rowfma_probe(force: bool = False) -> str:
    return _build_probe_libs(ROWFMA_PROBE_SRC, {"flags": ROWFMA_PROBE_LIB}, force)["flags"]


# The probe of the hazard-complete solver statements (tests/hip/filled_probe.hip, tests/test_filled_waits.py), under the
# library's own flags.
FILLED_PROBE_SRC = os.path.join(os.path.dirname(PROBE_SRC), "filled_probe.hip")
FILLED_PROBE_LIB = os.path.join(os.path.dirname(PROBE_SRC), "libgmr_filled_probe.so")


def build_filled_probe(force: bool = False) -> str:
    return _build_probe_libs(FILLED_PROBE_SRC, {"flags": FILLED_PROBE_LIB}, force)["flags"]


def build_variant(name: str, defines=(), verbose: bool = False) -> str:
    """libgmrhip_<name>.so with extra -D flags on every source (objects cached per flag set)."""
    out = os.path.join(HERE, f"libgmrhip_{name}.so")
    return _link([_object(s, list(defines), False, verbose) for s in SOURCES], out)


def build_ik_variant(name: str, defines=(), sources=("gmr_ik.hip",), force: bool = False) -> str:
    """libgmrhip_<name>.so with extra -D flags on `sources` ONLY, linked with the default objects of every other source:
    a switch of the latency kernel (-DGMR_QP_CARRIED_START) costs one compilation, not twenty-two.  A profile build
    (-DGMR_IK_PROFILE) names gmr_ik_host.hip as well: its entry point lives there.  Cached on the mtimes of sources and headers."""
    out = os.path.join(HERE, f"libgmrhip_{name}.so")
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    return _link([_object(s, list(defines) if s in sources else [], False, False) for s in SOURCES], out)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--variant":
        print(build_variant(sys.argv[2], sys.argv[3:], verbose=False))
    else:
        print(build(force=True, verbose=True))
