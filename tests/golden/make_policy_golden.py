#!/usr/bin/env python3
"""Generate tests/golden/policy_golden.npz: what the reference's own ``ActorCritic(A, O, P)`` (``booster_gym/utils/model.py``) computes, by
RUNNING it in float32 CPU torch at ``(O, P, A) = (5, 2, 3)`` on 70 rows.  Nothing of the reference is restated: the module is loaded from
the reference root and called -- ``model.act(obs).loc`` and ``model.est_value(obs, priv)`` -- with forward hooks on every ``torch.nn.ELU``.

The parameters are neither torch's initialisation nor a library's random stream: ``policy_mirror.golden_parameters`` writes the generator
out (the project's Philox4x32 mirror mapped to floats of about the magnitude of torch's default initialisation), this script fills the
``state_dict`` with them in the order of ``model.parameters()``, and the tests rebuild them bit for bit from the same lines -- the 152 199
floats do not go into git.

    obs f32[70, 5], priv f32[70, 2]      standard normal draws of a seeded NumPy generator, scaled by make_ppo_golden's OBS_SCALE so that
                                         some |loc| pass 1
    loc f32[70, 3], values f32[70]
    actor_hidden_l, critic_hidden_l      the output of ELU l of either network, every second column from column 0 (``hidden_stride``):
                                         f32[70, h_l / 2]

Asserted here: the order and the shapes of ``model.parameters()`` are the ones ``policy_mirror.shapes`` states; both branches of the ELU
occur in every hidden layer; some ``|loc| > 1``.

    python tests/golden/make_policy_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_ppo_golden as mpg  # noqa: E402
import make_rollout_golden as mrg  # noqa: E402
import policy_mirror as pol  # noqa: E402

SEED = 20261021
HIDDEN_STRIDE = 2


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    O, P, A = pol.GOLDEN_COLS
    rows = pol.GOLDEN_ROWS
    module = mrg.load(os.path.join(ref, "booster_gym", "utils", "model.py"), "policy_golden_model")
    model = module.ActorCritic(A, O, P)
    params = pol.golden_parameters(O, P, A)
    listed = list(model.parameters())
    assert [tuple(p.shape) for p in listed] == [(1, A)] + pol.shapes(O, P, A)[1:], [tuple(p.shape) for p in listed]
    with torch.no_grad():
        for p, a in zip(listed, params):
            p.copy_(torch.from_numpy(a).reshape(p.shape))
    rng = np.random.default_rng(SEED)
    obs = (rng.normal(0.0, 1.0, (rows, O)) * mpg.OBS_SCALE).astype(np.float32)
    priv = (rng.normal(0.0, 1.0, (rows, P)) * mpg.OBS_SCALE).astype(np.float32)
    seen = {"actor": [], "critic": []}
    for net in seen:
        for m in getattr(model, net):
            if isinstance(m, torch.nn.ELU):
                m.register_forward_hook(lambda mod, inp, out, net=net: seen[net].append((inp[0].detach().clone().numpy(), out.detach().clone().numpy())))
    with torch.no_grad():
        loc = model.act(torch.from_numpy(obs)).loc.numpy()
        values = model.est_value(torch.from_numpy(obs), torch.from_numpy(priv)).numpy()
    out = {"cols": np.array([O, P, A]), "hidden_stride": np.array(HIDDEN_STRIDE), "obs": obs, "priv": priv, "loc": loc.astype(np.float32),
           "values": values.astype(np.float32)}
    w = pol.widths(O, P, A)
    for net, calls in seen.items():
        assert [c[1].shape for c in calls] == [(rows, h) for h in w[net][1:-1]], net
        for l, (z, y) in enumerate(calls):
            assert (z > 0).any() and (z < 0).any(), (net, l)                      # both branches of the ELU
            print(net, l, "positive", float((z > 0).mean()), "largest", float(np.abs(y).max()))
            out[f"{net}_hidden_{l}"] = y[:, ::HIDDEN_STRIDE].astype(np.float32)
    print("loc: largest", float(np.abs(loc).max()), "above 1:", int((np.abs(loc) > 1).sum()), "values: largest", float(np.abs(values).max()))
    assert (np.abs(loc) > 1).any() and loc.shape == (rows, A) and values.shape == (rows,)
    assert all(v.dtype.kind in "fiu" for v in out.values())
    path = os.path.join(HERE, "policy_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "optim_golden.npz"))


if __name__ == "__main__":
    main(sys.argv)
