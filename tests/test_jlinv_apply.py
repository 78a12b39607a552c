"""-m gpu: se3_jlinv_coef5 / se3_jlinv_apply5 of csrc/gmr_device_math.h on the GPU (tests/hip/jlinv_apply_probe.hip, built
by build.build_jlinv_probe()) on the inputs of tests/test_jlinv_apply_host.py, against the same multiprecision values and
under the same bound (see that module's docstring).  Both compilations of the probe agree bit for bit.

GMR_MATH_ULP_DUMP=<file> writes the observed maximum next to the bound as JSON, as tests/test_device_math.py does (into
<file>.jlinv_apply.json, so that the two dumps do not overwrite each other).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import jlinv_apply_mirror as mirror
import test_jlinv_apply_host as host

pytestmark = pytest.mark.gpu


def _run(path, e, aux, jl, ja):
    L = C.CDLL(path)
    n = len(e)
    ins = [np.ascontiguousarray(a, dtype=np.float64) for a in (e, aux, jl, ja)]
    coef, out = np.empty((n, 8)), np.empty((n, 6))
    rc = L.gmr_probe_jlinv_apply(C.c_int(n), *[a.ctypes.data_as(C.c_void_p) for a in ins + [coef, out]])
    assert rc == 0, f"gmr_probe_jlinv_apply: HIP error {rc}"
    return coef, out


@pytest.fixture(scope="module")
def results():
    """the inputs, their multiprecision values and both compilations' (coef, [top; bot]); a GPU host without the probe is a
    failure, not a skip"""
    from general_motion_retargeting_amd import _lib, build
    _lib.require_gpu()
    try:
        libs = build.build_jlinv_probe()
    except Exception as exc:   # noqa: BLE001
        pytest.fail(f"the Jl^-1 apply probe is missing and could not be built: {exc}")
    e, aux, ident, jl, ja = mirror.cases()
    truth = host.truth_mp(e, ident, jl, ja)
    return (e, aux, ident, jl, ja, truth), {k: _run(p, e, aux, jl, ja) for k, p in libs.items()}


def test_device_apply_against_multiprecision(results):
    (e, aux, ident, jl, ja, truth), outs = results
    coef, out = outs["flags"]
    idz = ident == 1
    assert np.array_equal(coef[idz], np.broadcast_to([0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], coef[idz].shape))
    worst, ratio = host.check(out, e, ident, jl, ja, truth)
    print(f"device: max error {worst:.2f} ulp, max error / allowed {ratio:.3f}")
    dump = os.environ.get("GMR_MATH_ULP_DUMP")
    if dump:
        with open(dump + ".jlinv_apply.json", "w") as f:
            json.dump({"se3_jlinv_apply5": {"observed_max": worst, "observed_max_over_allowed": ratio, "n": int((~idz).sum()),
                                            "bound": "_jl_bound(32, t) + 8"}}, f, indent=1, sort_keys=True)
    assert ratio <= 1.0, (worst, ratio)


def test_both_compilations_are_bit_identical(results):
    _, outs = results
    for u, v in zip(outs["flags"], outs["wide"]):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
