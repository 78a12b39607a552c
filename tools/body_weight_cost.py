"""What per-frame body weights cost when they are on: the launch of two inputs -- the headline shape (100 streams x
100 frames, seed 0: the latency kernel) and 16 384 x 8, seed 1 (the throughput kernel, queued) -- without weights, with weights
of ones and with the pattern of the tests (levels 0 / 0.25 / 1 / 2.5 with probabilities 0.3 / 0.2 / 0.3 / 0.2, the rows of missing
bodies set to NaN), timed by device events around the launch on device buffers: ten steps after three.

    python tools/body_weight_cost.py [--steps 10] [--warmup 3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = np.array((0.0, 0.25, 1.0, 2.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import general_motion_retargeting_amd as pkg
    from general_motion_retargeting_amd import _lib, synth
    _lib.require_gpu()
    g = pkg.GeneralMotionRetargeting("smplx", "unitree_g1")
    sol = g.hip_solver
    root = g.human_body_names.index(g.human_root_name)
    st = _lib.Stream()
    e0, e1 = _lib.Event(), _lib.Event()
    for S, T, seed in ((100, 100, 0), (16384, 8, 1)):
        human, q0 = synth.make_streams(g.model, g._tables, S, T, seed=seed)
        nh = human.shape[2]
        pattern = LEVELS[np.random.default_rng(100 + seed).choice(4, size=(S, T, nh), p=(0.3, 0.2, 0.3, 0.2))]
        holes = np.array(human)
        miss = pattern == 0.0
        miss[..., root] = False
        holes[miss] = np.nan
        d_q0 = _lib.DeviceBuffer.from_host(np.ascontiguousarray(q0))
        d_q, d_ns, d_st = _lib.DeviceBuffer(S * T * sol.nq * 8), _lib.DeviceBuffer(S * T * 8), _lib.DeviceBuffer(S * 4)
        for tag, h, w in (("no weights", human, None), ("ones", human, np.ones((S, T, nh))), ("pattern", holes, pattern), ("no weights again", human, None)):
            d_h = _lib.DeviceBuffer.from_host(np.ascontiguousarray(h))
            d_w = None if w is None else _lib.DeviceBuffer.from_host(np.ascontiguousarray(w))
            ms = []
            for i in range(a.warmup + a.steps):
                e0.record(st)
                sol.retarget_streams_dev(S, T, d_q0, d_h, None, 0, d_q, d_ns, d_st, stream=st, d_weight=d_w)
                e1.record(st)
                st.sync()
                if i >= a.warmup:
                    ms.append(e0.elapsed_ms(e1))
            ns = d_ns.to_host((S, T, 2), np.int32)
            status = d_st.to_host((S,), np.int32)
            print(f"{S} x {T} seed {seed}, {tag}: {min(ms):.2f} / {np.mean(ms):.2f} / {max(ms):.2f} ms per launch (min / mean / max), "
                  f"{S * T / np.mean(ms) * 1e3:,.0f} frames/s, {ns.sum() / (S * T):.2f} solves per frame, failed streams {int((status != 0).sum())}")
            d_h.free()
            if d_w is not None:
                d_w.free()
        for b in (d_q0, d_q, d_ns, d_st):
            b.free()


if __name__ == "__main__":
    main()
