#!/usr/bin/env python3
"""Generate tests/golden/policy_bwd_golden.npz: the gradients torch's autograd computes through the reference's own ``ActorCritic(A, O, P)``
(``booster_gym/utils/model.py``), by RUNNING it in float32 CPU torch at ``(O, P, A) = (5, 2, 3)`` on the 70 rows of policy_golden.npz with
the parameters of ``policy_mirror.golden_parameters``.  Nothing of the reference is restated: the module is loaded from the reference root,
``loc = model.act(obs).loc`` and ``values = model.est_value(obs, priv)`` are formed with autograd on, and

    torch.autograd.backward((loc, values), (g_loc, g_values))

fills ``p.grad`` of every weight and bias.  The upstream gradients are not stored: ``policy_bwd_mirror.upstream`` writes their generator
out (Philox words mapped to [-1, 1) / rows) and the tests rebuild them bit for bit.

    cols i64[3], rows, dw_stride         (O, P, A), 70, 4
    db_<k> f32[width]                    the gradient of bias tensor k of the parameter list, whole
    dW_<k> f32[ceil(width / 4), in]      rows 0, 4, 8, .. of the gradient of weight tensor k (``dw_stride``)

Asserted here: both branches of the ELU occur in every hidden layer of the 70 rows; logstd gets no gradient (the distribution's scale is
not part of either output); the file stays below g_pre.npz.

    python tests/golden/make_policy_bwd_golden.py <reference root>        # or GMR_REFERENCE_ROOT
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_rollout_golden as mrg  # noqa: E402
import policy_bwd_mirror as bwd  # noqa: E402
import policy_mirror as pol  # noqa: E402


def main(argv):
    ref = argv[1] if len(argv) > 1 else os.environ.get("GMR_REFERENCE_ROOT")
    if not ref:
        raise SystemExit(__doc__)
    O, P, A = pol.GOLDEN_COLS
    rows = pol.GOLDEN_ROWS
    with np.load(os.path.join(HERE, "policy_golden.npz"), allow_pickle=False) as z:
        obs, priv = z["obs"], z["priv"]
    assert obs.shape == (rows, O) and priv.shape == (rows, P)
    module = mrg.load(os.path.join(ref, "booster_gym", "utils", "model.py"), "policy_bwd_golden_model")
    model = module.ActorCritic(A, O, P)
    params = pol.golden_parameters(O, P, A)
    listed = list(model.parameters())
    assert [tuple(p.shape) for p in listed] == [(1, A)] + pol.shapes(O, P, A)[1:]
    with torch.no_grad():
        for p, a in zip(listed, params):
            p.copy_(torch.from_numpy(a).reshape(p.shape))
    seen = {"actor": [], "critic": []}
    for net in seen:
        for m in getattr(model, net):
            if isinstance(m, torch.nn.ELU):
                m.register_forward_hook(lambda mod, inp, out, net=net: seen[net].append(inp[0].detach().clone().numpy()))
    loc = model.act(torch.from_numpy(obs)).loc
    values = model.est_value(torch.from_numpy(obs), torch.from_numpy(priv))
    g_loc, g_values = bwd.upstream(rows, A, 0), bwd.upstream(rows, 1, 1)
    torch.autograd.backward((loc, values), (torch.from_numpy(g_loc).reshape(loc.shape), torch.from_numpy(g_values).reshape(values.shape)))
    for net, calls in seen.items():
        assert len(calls) == 3, net
        for l, z in enumerate(calls):
            assert (z > 0).any() and (z < 0).any(), (net, l)                      # both branches of the ELU
    assert listed[0].grad is None or not listed[0].grad.any()
    out = {"cols": np.array([O, P, A]), "rows": np.array(rows), "dw_stride": np.array(bwd.GOLDEN_STRIDE)}
    for k, p in enumerate(listed):
        if k == 0:
            continue
        g = p.grad.detach().numpy().astype(np.float32)
        assert np.isfinite(g).all() and np.abs(g).max() > 0, k
        print(k, tuple(g.shape), "largest", float(np.abs(g).max()))
        if g.ndim == 2:
            out[f"dW_{k}"] = np.ascontiguousarray(g[::bwd.GOLDEN_STRIDE])
        else:
            out[f"db_{k}"] = g
    path = os.path.join(HERE, "policy_bwd_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "g_pre.npz"))


if __name__ == "__main__":
    main(sys.argv)
