"""A whole training iteration on a real MI355X as one chain of device calls (tests/tracker_chain.py): the listing of
INTEGRATION.md "A whole iteration" on a torch stream of the test's own -- torch operations and library launches interleaved, no
synchronisation and no read-back between the first call and the last -- against the same iteration from the NumPy mirrors, replayed step by
step against the downloaded slabs.  Every output is compared the way its own block's test compares it; N = 37 with R = 23, H = 6, M = 4
and two iterations around a stage switch, then N = 1 and N = 300, two trackers on two streams, and the documented alternatives of the
reset.  What the run rests on -- its coverage, its distance from every discontinuity -- is asserted on the CPU by
tests/test_tracker_chain_host.py."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_chain as tc  # noqa: E402
from test_tracker_control import hip, world  # noqa: E402,F401

pytestmark = pytest.mark.gpu

N, H, ITERS = 37, 6, 2


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def enqueue(torch, world, cfg, iterations, **kw):
    """a tracker, its device side on a stream of its own, ``iterations`` iterations enqueued with the stage switch between them and no
    synchronisation -> (tracker, device side)"""
    t = tc.build_tracker(world, cfg)
    dev = tc.Device(torch, cfg, torch.cuda.Stream())
    assert dev.stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    for it in range(iterations):
        if it:
            tc.stage_switch(t, cfg, it)
        tc.device_iteration(t, dev, it, **kw)
    return t, dev


def replay(world, cfg, got, iterations, first_cdf):
    mir = tc.Mirror(cfg, root_ang_vel=world["lib"].array("root_ang_vel"), first_cdf=first_cdf)
    for it in range(iterations):
        if it:
            mir.stage_switch(it)
        tc.mirror_iteration(mir, it, got, "listing")
    return mir


def report(mir):
    for k, v in sorted(mir.worst.items()):
        print(f"largest deviation met, {k}: {v:.3e}")


@pytest.fixture(scope="module")
def first(torch, hip, world):
    """the run of test 1: enqueued, synchronised once, downloaded; made once and never written"""
    cfg = tc.Config(N, H, ITERS)
    t, dev = enqueue(torch, world, cfg, ITERS)
    dev.stream.synchronize()
    got = dev.download()
    for a in got.values():
        a.flags.writeable = False
    return cfg, got, tc.device_state(t), t.first_cdf


def first_iteration(cfg, got):
    """the bytes of iteration 0 of a run"""
    out = {k: got[k][:cfg.H] for k in list(tc.STEP_SLABS) + ["dof_torques"]}
    out.update({k: a[0] for k, a in got.items() if k.startswith(("kept_", "ep_")) or k in ("stats", "old_loc", "old_lp")})
    return out


def test_two_iterations_around_a_stage_switch_are_the_mirrors(hip, world, first):
    cfg, got, state, first_cdf = first
    mir = replay(world, cfg, got, ITERS, first_cdf)
    tc.check_states(state, mir, "after two iterations")
    tc.no_sentinel_left(got, cfg)
    report(mir)


@pytest.mark.parametrize("n", [1, 300])
def test_one_iteration_at_the_edge_sizes(torch, hip, world, n):
    """N = 300: two 256-thread workgroups of the one-lane-per-environment kernels, 19 groups of the 16-per-workgroup kernels, a partial
    group in the reward and advantage sums"""
    cfg = tc.Config(n, 3, 1)
    t, dev = enqueue(torch, world, cfg, 1)
    dev.stream.synchronize()
    got = dev.download()
    mir = replay(world, cfg, got, 1, t.first_cdf)
    tc.check_states(tc.device_state(t), mir, f"N = {n}")
    tc.no_sentinel_left(got, cfg)
    report(mir)


def test_two_trackers_on_two_streams_share_nothing_writable(torch, hip, world, first):
    cfg, want, _, _ = first
    pairs = []
    for _ in range(2):
        pairs.append((tc.build_tracker(world, cfg), tc.Device(torch, cfg, torch.cuda.Stream())))
    assert pairs[0][1].stream.cuda_stream != pairs[1][1].stream.cuda_stream
    for _ in itertools.zip_longest(*[tc.iteration_calls(t, dev, 0) for t, dev in pairs]):          # call by call, alternately, both to their end
        pass
    for _, dev in pairs:
        dev.stream.synchronize()
    want0 = first_iteration(cfg, want)
    for i, (_, dev) in enumerate(pairs):
        got = first_iteration(cfg, dev.download())
        for k, a in want0.items():
            assert got[k].tobytes() == a.tobytes(), (i, k)


def test_the_documented_alternatives_are_the_same_episode(torch, hip, world, first):
    """hold_dev and proprio_reset_dev after an unchained reset_states_dev, and reset_done_dev on the compacted list with the failed flags by
    list position (made on the host from the downloaded masks of the first run) in place of the masks themselves: on an adaptive tracker
    reset_dev draws from the plain distribution and is no alternative"""
    cfg, want, _, _ = first
    t = tc.build_tracker(world, cfg)
    dev = tc.Device(torch, cfg, torch.cuda.Stream())
    lists = []
    for s in range(cfg.H):
        ids = np.nonzero(want["reset"][s])[0].astype(np.int32)
        failed = np.ascontiguousarray(want["fail"][s][ids])
        lists.append((torch.from_numpy(ids).to(dev.dev), torch.from_numpy(failed).to(dev.dev), len(ids)))
    assert sum(n for _, _, n in lists) > 0
    torch.cuda.synchronize()
    tc.device_iteration(t, dev, 0, chain=False, reset_lists=lists)
    dev.stream.synchronize()
    got, want0 = first_iteration(cfg, dev.download()), first_iteration(cfg, want)
    for k, a in want0.items():
        assert got[k].tobytes() == a.tobytes(), k
