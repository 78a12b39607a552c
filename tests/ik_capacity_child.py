"""Child process of tests/test_ik_capacity.py: the cases that fit the throughput kernel, served by the one-wavefront
instance of their size class instead.  GMR_IK_NO_WIDE is read by gmr_solver_create, so the parent sets it for this
process alone.

    python ik_capacity_child.py <out.npz>

out.npz: for every such case and input, `<case>/<input>/q`, `/ns`, `/st`, `/err` of two launches (`/q2`, ... for the second).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    assert os.environ.get("GMR_IK_NO_WIDE") == "1"
    import ik_capacity as ic
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    out = {}
    for name, c in ic.all_cases().items():
        if not c.expect["wide_fits"]:
            continue
        sol = _lib.Solver(c.mb, c.ts)
        sol.set_waves(1)
        for inp in c.inputs:
            human, q0 = ic.make_input(c, inp)
            for tag in ("", "2"):
                q, ns, st, _, err = sol.retarget_streams(q0, human, want_errors=True)
                out.update({f"{name}/{inp}/q{tag}": q, f"{name}/{inp}/ns{tag}": ns, f"{name}/{inp}/st{tag}": st, f"{name}/{inp}/err{tag}": err})
        sol.close()
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
