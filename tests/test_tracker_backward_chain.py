"""Two mini-epochs of the torch-free chain on a real MI355X (INTEGRATION.md "A mini-epoch without torch"):

    act_dev(hidden=) -> values_dev(hidden=) -> advantages_dev -> loss_dev -> act_backward_dev -> values_backward_dev -> optimizer_step_dev

at ``(H, N) = (1, 37)`` on the network ``odd`` of tests/test_tracker_policy.py, every array a device buffer, no call of torch.  Each link is
judged on what the device itself handed it, so that no accumulated rounding is judged through Adam's sign-like first step: the gradients
against the float64 backward of the device's own forward outputs and output gradients (the bounds of tests/test_tracker_backward.py), the
parameters against what ``optim_mirror`` makes of the device's own gradients (the comparison of DESIGN.md section 6x), and the second
mini-epoch's ``loc`` and ``values`` against the forward mirror on the stepped parameters (the bounds of section 6z)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_mirror as om  # noqa: E402
import policy_bwd_mirror as bwd  # noqa: E402
import policy_mirror as pol  # noqa: E402
import ppo_mirror as pm  # noqa: E402
import test_tracker_backward as tb  # noqa: E402
import test_tracker_policy as tp  # noqa: E402
from test_tracker_control import hip, world  # noqa: E402,F401
from test_tracker_loss import LOSS, fetch, guarded  # noqa: E402
from test_tracker_optim import BOUND as OPT_BOUND  # noqa: E402
from test_tracker_optim import units as opt_units  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
H, N = 1, 37
CASE = "odd"
LR = 1e-3


def test_two_mini_epochs_without_torch(hip, world):
    O, P, A, ah, ch, _ = tp.CASES[CASE]
    M = H * N
    params0 = tb.inputs(CASE)[0]
    sizes = pol.sizes(O, P, A, ah, ch)
    K = len(sizes)
    t = tp.policy_tracker(world, CASE, n=N)
    t.set_rollout(H, O, P, A, 0.995, 0.95)
    t.set_loss(**LOSS)
    t.set_optimizer(sizes, learning_rate=LR)
    assert t.set_backward(M)["chunks"] == 1
    # the rollout of the iteration: what the old policy saw and did
    rng = np.random.default_rng(41)
    obs, priv = rng.normal(0.0, 1.0, (M, O)).astype(F), rng.normal(0.0, 1.0, (M, P)).astype(F)
    old = pol.Policy(O, P, A, ah, ch, num_envs=M).act(params0, obs, sample=False)["loc"]
    logstd0 = np.asarray(params0[0], F).reshape(-1)
    actions = (old + np.exp(logstd0)[None, :] * rng.normal(0.0, 1.0, (M, A))).astype(F)
    host = {"obs": obs, "priv": priv, "actions": actions, "old_loc": old, "old_logstd": logstd0.copy(), "old_log_prob": pm.log_prob(old, logstd0, actions),
            "rewards": rng.normal(0.5, 1.0, M).astype(F), "dones": (rng.random(M) < 0.1).astype(np.uint8), "time_outs": np.zeros(M, np.uint8),
            "last_values": rng.normal(0.5, 1.0, N).astype(F)}
    dev = {k: guarded(a) if a.dtype == F else hip.DeviceBuffer.from_host(a) for k, a in host.items()}      # (the two u8 arrays: no guard words)
    widths = pol.widths(O, P, A, ah, ch)
    like = {"loc": np.zeros((M, A), F), "values": np.zeros(M, F), "advantages": np.zeros(M, F), "returns": np.zeros(M, F), "normalized": np.zeros(M, F),
            "grad_loc": np.zeros((M, A), F), "grad_logstd": np.zeros(A, F), "grad_values": np.zeros(M, F)}
    for net in ("actor", "critic"):
        for l, h in enumerate(widths[net][1:-1]):
            like[f"{net}_hidden_{l}"] = np.zeros((M, h), F)
            like[f"{net}_delta_{l}"] = np.zeros((M, h), F)
    out = {k: guarded(a) for k, a in like.items()}
    d_params = [guarded(a) for a in params0]
    d_grads = [out["grad_logstd"]] + [guarded(np.full(p.shape, tb.PATTERN, F)) for p in params0[1:]]      # logstd's gradient is the loss head's
    layers = {net: [out[f"{net}_hidden_{l}"] for l in range(len(widths[net]) - 2)] for net in widths}
    deltas = {net: [out[f"{net}_delta_{l}"] for l in range(len(widths[net]) - 2)] for net in widths}

    def mini_epoch():
        """the chain: seven calls, ten launches or so, no torch and no synchronisation between them"""
        t.act_dev(d_params, dev["obs"], out["loc"], hidden=layers["actor"], sample=False, rows=M)
        t.values_dev(d_params, dev["obs"], dev["priv"], out["values"], hidden=layers["critic"], rows=M)
        t.advantages_dev({k: dev[k] for k in ("rewards", "dones", "time_outs")}, out["values"], dev["last_values"],
                         {k: out[k] for k in ("advantages", "returns", "normalized")})
        t.loss_dev({"loc": out["loc"], "logstd": d_params[0], "actions": dev["actions"], "old_log_prob": dev["old_log_prob"], "values": out["values"],
                    "returns": out["returns"], "advantages": out["normalized"], "old_loc": dev["old_loc"], "old_logstd": dev["old_logstd"]},
                   {k: out[k] for k in ("grad_loc", "grad_logstd", "grad_values")})
        t.act_backward_dev(d_params, d_grads, dev["obs"], layers["actor"], out["grad_loc"], deltas["actor"], rows=M)
        t.values_backward_dev(d_params, d_grads, dev["obs"], dev["priv"], layers["critic"], out["grad_values"], deltas["critic"], rows=M)
        t.optimizer_step_dev(d_params, d_grads)

    opt = om.Optimizer(sizes, dtype=D)
    params = [np.asarray(p, F) for p in params0]
    first = {"critic": 1, "actor": 1 + 2 * (len(ch) + 1)}
    for epoch in range(2):
        mini_epoch()
        got = {k: fetch(out[k], like[k]) for k in out}
        grads = [got["grad_logstd"]] + [fetch(b, p) for b, p in zip(d_grads[1:], params[1:])]
        stepped = [fetch(b, p) for b, p in zip(d_params, params)]
        assert all(np.isfinite(g).all() for g in grads) and all((g != tb.PATTERN).all() for g in grads[1:])
        # the forward on the parameters the epoch started from (the first epoch's: the forward test's own ground)
        m = pol.Policy(O, P, A, ah, ch, num_envs=M, dtype=D)
        fa, fv = m.act(params, obs, sample=False), m.values(params, obs, priv)
        dev_f = tp.deviations({"loc": got["loc"], "hidden": [got[f"actor_hidden_{l}"] for l in range(len(ah))]},
                              {"values": got["values"], "hidden": [got[f"critic_hidden_{l}"] for l in range(len(ch))]}, {"act": fa, "values": fv})
        print("epoch", epoch, "forward", {k: round(v, 3) for k, v in dev_f.items()})
        for k, v in dev_f.items():
            assert v <= tp.BOUND[k], (epoch, k, v, tp.BOUND[k])
        # the gradients: the float64 backward of the device's own forward outputs and output gradients
        B = bwd.Backward(m)
        want = {"actor": B.act(params, obs, [got[f"actor_hidden_{l}"] for l in range(len(ah))], got["grad_loc"]),
                "critic": B.values(params, obs, priv, [got[f"critic_hidden_{l}"] for l in range(len(ch))], got["grad_values"])}
        for net in ("actor", "critic"):
            L = len(widths[net]) - 2
            mine = {"delta": [got[f"{net}_delta_{l}"] for l in range(L)], "dW": [grads[first[net] + 2 * l] for l in range(L + 1)],
                    "db": [grads[first[net] + 2 * l + 1] for l in range(L + 1)]}
            dev_b = tb.deviations(mine, want[net])
            print("epoch", epoch, net, {k: round(v, 3) for k, v in dev_b.items()})
            for k, v in dev_b.items():
                assert v <= tb.BOUND[k], (epoch, net, k, v, tb.BOUND[k])
        assert np.abs(got["grad_loc"]).max() > 0 and np.abs(got["grad_values"]).max() > 0
        # the step: what the optimiser's mirror makes of the device's own gradients
        new, info = opt.step(params, grads, LR)
        worst = max(opt_units(x, y) for x, y in zip(stepped, new))
        print("epoch", epoch, "parameters", round(worst, 3), "norm", info[0], "coef", info[1])
        assert worst <= OPT_BOUND["param"], (epoch, worst)
        assert all((x != y).any() for x, y in zip(stepped, params)), "a tensor was not stepped"
        params = stepped
    assert K == len(d_params) == len(d_grads)
