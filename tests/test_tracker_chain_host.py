"""The chain of a whole training iteration on the mirrors alone (tests/tracker_chain.py): what the device test of
tests/test_tracker_chain.py rests on, asserted without a GPU -- the run it makes meets every branch of the coverage list and stays clear of
every discontinuity behind a bound; the reference's line order and the order of the INTEGRATION.md listing differ in exactly the documented
rows and columns; every column of the observation row and of the privileged row has one writer; no two draws share a Philox counter; and
every line of the toy simulator, the policy and the critic rounds once."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import commands_mirror as cmm  # noqa: E402
import tracker_chain as tc  # noqa: E402
import tracker_mirror as tm  # noqa: E402

F = np.float32
N, H, ITERS = 37, 6, 2


def fork(mir):
    """a mirror that goes on from the same state on its own (the configuration is shared, it is never written)"""
    new = copy.copy(mir)
    for k, v in vars(mir).items():
        if k not in ("cfg", "o"):
            setattr(new, k, copy.deepcopy(v))
    return new


def run(n=N, horizon=H, iterations=ITERS, order="listing", ops=None, loss_seed=None):
    cfg = tc.Config(n, horizon, iterations, loss_seed)
    mir = tc.Mirror(cfg, ops=ops)
    steps, after = [], []
    for it in range(iterations):
        if it:
            mir.stage_switch(it)
        a, b = tc.mirror_iteration(mir, it, None, order)
        steps += a
        after.append(b)
    return cfg, mir, steps, after


@pytest.fixture(scope="module")
def chain():
    """the run the device test makes, on the mirrors alone, made once and never written"""
    return run()


def test_the_run_meets_every_branch_of_the_coverage_list(chain):
    cfg, mir, steps, after = chain
    S = len(steps)
    assert S == H * ITERS
    pdone = np.stack([r["proprio_done"] for r in steps])
    for bit in (1, 2, 4):
        assert (pdone & bit).any(), f"proprio done bit {bit}"
    assert (np.stack([r["feet_done"] for r in steps]) == 8).any(), "the feet contact bit"
    assert any((r["feet_term"][:, 0] > 0).any() for r in steps), "a collision"
    assert np.stack([r["finished"] for r in steps]).any(), "a finished clip with its redraw"
    s, e = cfg.events["link_fail"]
    fail = np.stack([r["fail"] for r in steps])
    assert fail[s, e] == 1 and (np.stack([r["reset"] for r in steps])[fail != 0] != 0).all(), "a link fail, and it resets"
    assert mir.trk.ema.any(), "the failure reached the bins and an Adapt folded it in"
    # the anchors of the environments that were reset moved to their robots, the others are the identity still; the preview looks past
    # the end of some clips and inside others
    moved = np.abs(mir.anchor["pos"][:, :2]).sum(axis=1) > 0
    ever = (np.stack([r["reset"] for r in steps]) != 0).any(axis=0)
    assert moved[ever].all() and not moved[~ever].any() and not mir.anchor["pos"][:, 2].any() and (mir.anchor["yaw_zw"] == (0, 1)).all()
    valid = np.stack([r["pre_valid"] for r in steps])
    assert (valid == 1).any() and (valid == 0).any()
    flags = np.stack([r["flags"] for r in steps])
    for bit, what in ((cmm.BOUNDARY, "a CMD_BOUNDARY"), (cmm.RESAMPLED, "a command resample"), (cmm.SUCCESS, "a curriculum success")):
        assert (flags & bit).any(), what
    acts = [r["disturb"] for r in steps]
    assert any(a & cmm.KICK for a in acts) and any(a & cmm.PUSH_START for a in acts) and any(a & cmm.PUSH_STOP for a in acts)
    inside = [s for s in range(1, S) if acts[s - 1] & cmm.PUSH_START and not acts[s] & (cmm.PUSH_START | cmm.PUSH_STOP)]
    assert inside and all(np.abs(steps[s]["push_force"]).max() > 0 for s in inside), "a step inside a push window"
    startup = np.stack([r["startup"] for r in steps])
    assert startup.any() and (~startup).any() and (~startup[0]).any(), "start-up phase and run phase"
    reset = np.stack([r["reset"] for r in steps]) != 0
    assert reset[0].any() and reset[H - 1].any(), "a reset at the first and at the last step of a horizon"
    per_env = reset.sum(axis=0)
    assert (per_env == 0).any() and (per_env >= 2).any(), "an environment that is never reset, one that is reset twice"
    # a time-out that rewrites a recorded reward: the rollout's buffer holds the critic's value there after the advantages
    seen = 0
    for it in range(ITERS):
        to = after[it]["buf"]["time_outs"] != 0
        values = after[it]["epochs"][-1]["values"]
        assert (after[it]["buf"]["rewards"][to] == values[to]).all()
        rewards = np.stack([r["reward"] for r in steps[it * H:(it + 1) * H]])
        seen += int((rewards[to] != values[to]).sum())
    assert seen > 0
    time_outs = np.stack([r["time_outs"] for r in steps]) != 0
    assert (time_outs & ~(pdone & 4).astype(bool)).any(), "a time-out that comes from a command boundary alone"
    # episodes finished and counted in both iterations
    assert all(a["stats"][0] > 0 for a in after)
    # the scripted events did what they were scripted for
    for name, bit in (("velocity", 1), ("height", 2), ("second_reset", 2)):
        s, e = cfg.events[name]
        assert pdone[s, e] & bit, name
    s, e = cfg.events["contact"]
    assert steps[s]["feet_done"][e] == 8


def test_the_run_stays_clear_of_every_discontinuity_behind_a_bound(chain):
    """the feet test's bounds hold 1e-5 from the contact clearance and 1e-3 rad from the angles' seams (its ``check``), the loss test's where
    no ratio lies within its MARGIN of the clip interval's ends, and the learning-rate rule is decided where the float64 KL is away from
    both thresholds by more than the loss test asks (1e-3, relative)"""
    cfg, mir, steps, after = chain
    for s, r in enumerate(steps):
        assert r["feet_margins"]["clearance"] > tc.CLEARANCE_MARGIN and r["feet_margins"]["angle"] > tc.ANGLE_MARGIN, (s, r["feet_margins"])
        assert r["cdf_margin"] > tc.CDF_MARGIN, (s, r["cdf_margin"])
        assert (np.abs(r["max_dist"] - tc.FAIL_DIST) > 1e-3).all(), (s, "a link at the failure distance")
    moves = []
    for it, a in enumerate(after):
        for ep, e in enumerate(a["epochs"]):
            assert e["near"] > tc.MARGIN and e["weights_agree"], (it, ep, e["near"])
            assert e["kl_margin"] > tc.KL_MARGIN, (it, ep, e["kl"])
            assert e["own_error"] <= tc.LOSS_OWN_ERROR, (it, ep, e["own_error"])      # the loss test's bounds carry over to these inputs
            moves.append(np.sign(e["m64"]["terms"][6] - e["lr_before"]))
    assert -1 in moves and 1 in moves and 0 in moves, moves       # the rule lowers, raises and keeps the rate in this run


@pytest.mark.parametrize("n", [1, 300])
def test_the_edge_sizes_stay_clear_too(n):
    """the runs of the device test at N = 1 and N = 300 (H = 3, one iteration)"""
    cfg, mir, steps, after = run(n, 3, 1)
    for s, r in enumerate(steps):
        assert r["feet_margins"]["clearance"] > tc.CLEARANCE_MARGIN and r["feet_margins"]["angle"] > tc.ANGLE_MARGIN, (s, r["feet_margins"])
        assert r["cdf_margin"] > tc.CDF_MARGIN, (s, r["cdf_margin"])
        assert (np.abs(r["max_dist"] - tc.FAIL_DIST) > 1e-3).all(), (s, "a link at the failure distance")
    for ep, e in enumerate(after[0]["epochs"]):
        assert e["near"] > tc.MARGIN and e["weights_agree"] and e["kl_margin"] > tc.KL_MARGIN, (ep, e["near"], e["kl"])
        assert e["own_error"] <= tc.LOSS_OWN_ERROR, (ep, e["own_error"])
    assert np.stack([r["reset"] for r in steps]).any()


def test_the_two_orders_differ_in_the_documented_rows_and_columns_and_nowhere_else():
    """Step by step from a common state: the listing's order against the reference's line order (t1.py:437-497).  They differ
      * in the rows with ``reset`` set: the dof_pos and dof_vel columns of the observation row the step leaves, and ``last_dof_vel`` (so the
        dof_acc term of the one step that follows) -- the reference forms the row and rolls over after the reset, proprio_dev before it;
      * on a kick step, in every row: the root_acc term, what the reward makes of it, and, in the rows that are not reset,
        ``last_root_vel`` (so the root_acc term of the one step that follows) -- the reference kicks before its termination check and its
        reward, disturb_dev comes after proprio_dev;
    and nowhere else.  No reordering of the existing calls removes either: proprio_dev forms terms, row and roll-over in one launch.  The
    reference side is tracker_chain.ReferenceProprio, the proprio statement cut into the reference's own pieces and called in its line order;
    nothing of it is copied from the listing's run, so an equality found here is one of two computations."""
    cfg = tc.Config(N, H, ITERS)
    mir = tc.Mirror(cfg)
    d0, d1 = tc.obs_block("dof_pos")[0], tc.obs_block("dof_vel")[1]
    ROOT_ACC = 6
    col = 10 + ROOT_ACC                                     # the proprio block follows the six tracking and four link terms in the reward's columns
    met = {"obs": 0, "last_dof_vel": 0, "root_acc": 0, "last_root_vel": 0}
    for s in range(cfg.S):
        if s == H:
            mir.stage_switch(1)
        other = fork(mir)
        a, b = tc.mirror_step(mir, s, None, "listing"), tc.mirror_step(other, s, None, "reference")
        reset = a["reset"] != 0
        kick = bool(a["disturb"] & cmm.KICK)
        allowed = {"obs": np.zeros((N, tc.W), bool), "obs_row": np.zeros((N, tc.OW), bool)}
        allowed["obs"][reset, d0:d1] = allowed["obs_row"][reset, d0:d1] = True
        if kick:
            allowed["proprio_term"] = np.zeros((N, 14), bool)
            allowed["proprio_term"][:, ROOT_ACC] = True
            allowed["scaled"] = np.zeros((N, tc.NC), bool)
            allowed["scaled"][:, col] = True
            allowed["group_total"] = np.zeros((N, 2), bool)
            allowed["group_total"][:, 0] = True
            allowed["proprio_total"] = allowed["reward"] = np.ones(N, bool)
        for k, x in a.items():
            if not isinstance(x, np.ndarray):
                continue
            y = b[k]
            diff = ~((x == y) | ((x != x) & (y != y)))
            assert not (diff & ~allowed.get(k, np.zeros(x.shape, bool))).any(), (s, k)
            if k == "obs":
                met["obs"] += int(diff.sum())
            if k == "proprio_term":
                met["root_acc"] += int(diff.sum())
        sa, sb = mir.state(), other.state()
        for part in sa:
            if part == "learning_rate":
                continue
            for k, x in sa[part].items():
                diff = x != sb[part][k]
                ok = np.zeros(x.shape, bool)
                if (part, k) == ("proprio", "last_dof_vel"):
                    ok[reset] = True
                    met["last_dof_vel"] += int(diff.sum())
                if kick and (part, k) == ("proprio", "last_root_vel"):
                    ok[~reset] = True
                    met["last_root_vel"] += int(diff.sum())
                if kick and (part, k) == ("rewards", "ep_sum"):
                    ok[~reset, 0] = ok[~reset, 1 + col] = True
                assert not (diff & ~ok).any(), (s, part, k)
        for k in ("obs", "rewards"):
            diff = mir.roll.io[k] != other.roll.io[k]
            assert not diff.any() or k == "rewards" and kick, (s, "rollout", k)
    assert all(v > 0 for v in met.values()), met


def test_every_column_of_the_two_rows_has_one_writer():
    from general_motion_retargeting_amd import MotionTracker
    t = MotionTracker.__new__(MotionTracker)
    t._init_state(None, N, tc.R)
    t._proprio = (tc.R, tc.CX)
    lay = t.proprio_layout()
    t._preview = (tc.PK, tc.PRE_BLOCKS, "reference", 0)
    obs, priv = tc.row_writers(lay, t.preview_layout)
    assert t.preview_layout["row_width"] == tc.PD
    assert tc.partitions(obs, tc.OW) and tc.partitions(priv, tc.P), (obs, priv)
    assert lay["obs"]["extra"] == (tc.CMD_COL, tc.CMD_COL + tc.CX) and lay["width"] == tc.W
    assert all(tc.obs_block(k) == lay["obs"][k] for k in lay["obs"])
    # the same statement fails when two calls claim a column, or none does
    assert not tc.partitions(obs + [("commands_dev:again", tc.CMD_COL, tc.CMD_COL + 3)], tc.OW)
    assert not tc.partitions([r for r in priv if not r[0].startswith("caller")], tc.P)
    # the reward's columns: the four blocks of the chain in fixed order, thirty-two of them
    t._commands, t._feet, t._links = (None,), (tc.NB, 4), (None, 6, None, "world")
    t._rewards = t._rewards_setup(None, None, tc.GROUPS, tc.REWARD_KW["group_weight"], tc.REWARD_KW["only_positive"], True)
    rl = t.reward_layout()
    assert rl["blocks"] == {"terms": (0, 6), "links": (6, 4), "proprio": (10, 14), "feet": (24, 8), "commands": (28 + 4, 4), "extra": (tc.NC, 0)}
    assert list(rl["groups"]) == tc.Config(1, 1, loss_seed=0).reward_groups()
    # and the mirror's rows are laid out by it
    cfg, mir, steps, _ = run(3, 2, 1, loss_seed=0)
    r = steps[-1]
    a, b = lay["obs"]["actions"]
    assert r["obs"][:, a:b].tobytes() == r["actions_clipped"].tobytes()
    assert r["obs"][:, tc.CMD_COL:tc.CMD_COL + 3].tobytes() == (r["commands"] * np.array(tc.PLAIN["obs_scales"], F)).astype(F).tobytes()
    assert r["priv"][:, tc.PRIV_PUSH:].tobytes() == r["push_obs"].tobytes() and r["priv"][:, 0:1].tobytes() == cfg.mass.tobytes()


def test_no_two_draws_share_a_counter(monkeypatch):
    """every Philox call of the run, by the function that made it: a counter belongs to one draw site, its fourth word is that site's
    domain, and a site uses a counter once -- twice where an element pair shares the four words of one call"""
    calls = []
    scalar, many = tm.philox4x32, cmm.philox_np

    def rec_scalar(counter, key, rounds=10):
        f = sys._getframe(1)
        calls.append((tuple(int(x) for x in counter), tuple(key), os.path.basename(f.f_code.co_filename) + ":" + f.f_code.co_name))
        return scalar(counter, key, rounds)

    def rec_many(e, n, j, domain, key):
        f = sys._getframe(1)
        site = os.path.basename(f.f_code.co_filename) + ":" + f.f_code.co_name
        for a, b in zip(np.asarray(e).reshape(-1).tolist(), np.broadcast_to(np.asarray(n), np.shape(e)).reshape(-1).tolist()):
            calls.append(((int(a), int(b), int(j), int(domain)), tuple(key), site))
        return many(e, n, j, domain, key)

    import adaptive_mirror as am
    bins = am.philox4x32_many

    def rec_bins(c0, c1, key):
        f = sys._getframe(1)
        if f.f_code.co_name == "reset_done":               # (tracker_chain.cdf_margin looks ahead with the same function: no draw)
            for a, b in zip(np.asarray(c0).reshape(-1).tolist(), np.asarray(c1).reshape(-1).tolist()):
                calls.append(((int(a), int(b), 0, 0), tuple(key), "adaptive_mirror.py:reset_done"))
        return bins(c0, c1, key)

    monkeypatch.setattr(am, "philox4x32_many", rec_bins)
    monkeypatch.setattr(tm, "philox4x32", rec_scalar)
    monkeypatch.setattr(cmm, "philox_np", rec_many)
    run()
    domains = {"tracker_mirror.py:draw": 0, "adaptive_mirror.py:draw_bin": 0, "adaptive_mirror.py:reset_done": 0, "proprio_mirror.py:words": 1, "commands_mirror.py:step": 2, "commands_mirror.py:draw": 3,
               "episode_mirror.py:reset_words": 4}
    pairs = {"proprio_mirror.py:words", "commands_mirror.py:draw", "episode_mirror.py:reset_words"}
    assert {c[2] for c in calls} == set(domains), {c[2] for c in calls}
    owner, uses = {}, {}
    # the redraw of a finished clip: the adaptive mirror lets its parent draw, takes that draw back and draws from the bins on the same
    # counter -- one draw of the device, two calls of the mirror
    taken_back = set()
    for i, (counter, key, site) in enumerate(calls):
        if site == "adaptive_mirror.py:draw_bin":
            j = max(k for k in range(i) if calls[k][0] == counter and calls[k][2] == "tracker_mirror.py:draw")
            taken_back.add(j)
    assert taken_back
    calls = [(c, k, "tracker" if domains[s] == 0 else s) for i, (c, k, s) in enumerate(calls) if i not in taken_back]
    domains["tracker"] = 0
    for counter, key, site in calls:
        assert counter[3] == domains[site], (counter, site)
        assert owner.setdefault((counter, key), site) == site, (counter, site, owner[(counter, key)])
        uses[(counter, key)] = uses.get((counter, key), 0) + 1
    for (counter, key), n in uses.items():
        assert n <= (2 if owner[(counter, key)] in pairs else 1), (counter, owner[(counter, key)], n)
    assert len(calls) > 10000 and len({c[1] for c in calls}) == 1


def test_the_twins_round_once_per_line():
    ops = tc.CheckedOps()
    run(N, 3, 1, ops=ops, loss_seed=0)
    assert ops.lines > 100
