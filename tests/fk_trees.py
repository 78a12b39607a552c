"""Synthetic kinematic trees for the float32 FK kernels (csrc/gmr_fk.hip, plan in csrc/gmr_fk_tree.h) and a float64 walk
written from the definition of the operation.  NumPy only; used by tests/test_fk_trees_host.py (CPU) and
tests/test_fk_trees.py (GPU).

A tree is the dict ``FkHandle`` takes: ``parent`` (i32, ``parent[b] < b``, -1 for the root), ``local_translation`` (f32),
``local_rotation`` (f32 xyzw, NOT normalised), ``dof_idx`` (i32, -1: no hinge), ``dof_dim`` (i32), ``axis`` (f64, any length),
plus ``name`` and ``family``.

Families (``FAMILIES``): single body; 2, 3, 5 and 7 bodies (below 8 a tree is never split; with 1, 2, 3, 5 and 7 bodies the
float count of a block's output is no multiple of 4 for some of B = 1, 63, 65, 130, which sends the flush through its scalar
tail); a chain of depth exactly 24; a star of 63 leaves; a comb (each trunk body carries one leaf); a binary tree of 63
bodies; a broom (long trunk, a fan of leaves at its end); two brooms from the root; humanoid-like trees with random limbs;
uniformly random trees (``parent[b]`` uniform below ``b``) and deep random trees (``parent[b]`` among the last few bodies),
both resampled to respect the depth limit.  Across all families: bodies without a hinge, dof indices in body order or
permuted, local rotations that are exactly the identity / unit / rounded to three decimals as robot descriptions have them
(norm off by 1e-3), hinge axes exactly +-e_k (both signs) or general and of any length, translation components exactly zero.

``GPU_TREES`` is the fixed list the GPU tests walk; ``sweep(n, seed)`` yields as many trees as asked for the CPU checks of
the plan.  What the plan makes of the GPU list (checked in tests/test_fk_trees_host.py from the output of
tests/cpp/fk_plan_check.cpp, four wavefronts allowed): trees that end with 2, 3 and 4 wavefronts, trees with and without a
shared trunk, with extra angle columns, with the register spare slot only, with private LDS slots beyond it, trees that
fall back to one wavefront (more than 32 parked angles in a list), and trees below 8 bodies.  No listed plan feature is out
of reach of the generator.
"""
import numpy as np

F = np.float32
MAX_BODIES, MAX_DEPTH = 64, 24


# ---------------------------------------------------------------------------------------------------------------------------
# topologies
# ---------------------------------------------------------------------------------------------------------------------------
def depth_of(parent):
    d = np.zeros(len(parent), dtype=np.int64)
    for b in range(1, len(parent)):
        d[b] = d[parent[b]] + 1
    return d


def _chain(n):
    return [-1] + list(range(n - 1))


def _star(n):
    return [-1] + [0] * (n - 1)


def _comb(trunk):
    par = [-1]
    last = 0
    for _ in range(trunk):
        par.append(last)                 # the next trunk body ...
        last = len(par) - 1
        par.append(last)                 # ... and its leaf
    return par


def _binary(n):
    return [-1] + [(b - 1) // 2 for b in range(1, n)]


def _broom(trunk, leaves, start=0, par=None):
    par = [-1] if par is None else par
    last = start
    for _ in range(trunk):
        par.append(last)
        last = len(par) - 1
    par.extend([last] * leaves)
    return par


def _humanoid(rng):
    par = [-1]
    torso = [0]
    for _ in range(int(rng.integers(1, 4))):
        par.append(torso[-1])
        torso.append(len(par) - 1)
    for limb in range(int(rng.integers(4, 6))):
        last = torso[0] if limb < 2 else torso[-1]       # legs from the pelvis, arms and head from the chest
        for _ in range(int(rng.integers(2, 9))):
            if len(par) >= MAX_BODIES:
                break
            par.append(last)
            last = len(par) - 1
        if rng.random() < 0.5 and len(par) + 3 <= MAX_BODIES:      # a hand: a few fingers on the limb's end
            par.extend([last] * int(rng.integers(2, 4)))
    return par


def _random(rng, n, window=None):
    par, depth = [-1], [0]
    for b in range(1, n):
        ok = [p for p in range(b) if depth[p] + 2 <= MAX_DEPTH]                  # parents that respect the depth limit
        near = [p for p in ok if window is None or p >= b - window]
        p = int(rng.choice(near or ok))
        par.append(p)
        depth.append(depth[p] + 1)
    return par


def _topology(family, rng):
    if family == "single":
        return [-1]
    if family.startswith("small"):
        return _random(rng, int(family[5:]))
    if family == "chain24":
        return _chain(MAX_DEPTH)
    if family == "star":
        return _star(MAX_BODIES)
    if family == "comb":
        return _comb(int(rng.integers(8, MAX_DEPTH - 1)))
    if family == "binary":
        return _binary(63)
    if family == "broom":
        trunk = int(rng.integers(10, MAX_DEPTH - 1))
        return _broom(trunk, int(rng.integers(30, MAX_BODIES - trunk)))
    if family == "brooms2":
        t1, t2 = int(rng.integers(6, 20)), int(rng.integers(6, 20))
        l1 = int(rng.integers(3, (MAX_BODIES - 1 - t1 - t2) // 2 + 1))
        l2 = int(rng.integers(3, MAX_BODIES - t1 - t2 - l1))
        return _broom(t2, l2, 0, _broom(t1, l1))
    if family == "humanoid":
        return _humanoid(rng)
    if family == "random":
        return _random(rng, int(rng.integers(8, MAX_BODIES + 1)))
    if family == "deep":
        return _random(rng, int(rng.integers(20, MAX_BODIES + 1)), window=int(rng.integers(2, 6)))
    raise ValueError(family)


FAMILIES = ("single", "small2", "small3", "small5", "small7", "chain24", "star", "comb", "binary", "broom", "brooms2", "humanoid",
            "random", "deep")


# ---------------------------------------------------------------------------------------------------------------------------
# a whole tree
# ---------------------------------------------------------------------------------------------------------------------------
def make_tree(family, seed):
    rng = np.random.default_rng([FAMILIES.index(family), seed])
    return tree_from_parents(_topology(family, rng), family, seed, rng)


def tree_from_parents(parent, family, seed, rng=None, name=None):
    """the hinges, dof order, local rotations, axes and translations of ``make_tree`` on a given parent list.  ``rng``: the
    generator that drew the topology (``make_tree`` goes on with it); without one the tree draws from its own"""
    if rng is None:
        rng = np.random.default_rng([FAMILIES.index(family), seed, len(parent)])
    par = np.array(parent, dtype=np.int32)
    nb = len(par)
    assert 1 <= nb <= MAX_BODIES and depth_of(par).max() + 1 <= MAX_DEPTH and all(par[b] < b for b in range(nb))
    # hinges: all bodies, most bodies, or half of them; dofs in body order or permuted
    p_hinge = (1.0, 0.85, 0.5)[seed % 3]
    hinge = rng.random(nb) < p_hinge
    hinge[0] = False
    ndof = int(hinge.sum())
    order = rng.permutation(ndof) if (seed // 3) % 2 else np.arange(ndof)
    dof_idx = np.full(nb, -1, dtype=np.int32)
    dof_idx[hinge] = order
    # local rotations: identity / unit / three decimals
    q = rng.normal(size=(nb, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    kind = rng.integers(0, 3, size=nb)
    q[kind == 0] = [0.0, 0.0, 0.0, 1.0]
    q[kind == 2] = np.round(q[kind == 2], 3)
    # hinge axes: +-e_k or anything
    axis = rng.normal(size=(nb, 3)) * rng.uniform(0.3, 3.0, size=(nb, 1))
    aligned = rng.random(nb) < 0.5
    axis[aligned] = np.eye(3)[rng.integers(0, 3, size=int(aligned.sum()))] * rng.choice([-1.0, 1.0], size=(int(aligned.sum()), 1))
    # translations with exact zeros
    t = rng.normal(0.0, 0.1, size=(nb, 3))
    t[rng.random((nb, 3)) < 0.3] = 0.0
    return {"name": name or f"{family}-{seed}", "family": family, "parent": par, "local_translation": t.astype(F), "local_rotation": q.astype(F),
            "dof_idx": dof_idx, "dof_dim": hinge.astype(np.int32), "axis": axis}


def sweep(n, seed=0):
    """``n`` trees, the families in turn"""
    for i in range(n):
        yield make_tree(FAMILIES[i % len(FAMILIES)], seed + i // len(FAMILIES))


# (family, seed): the trees the GPU tests walk.  Every family; tests/test_fk_trees_host.py asserts what the plan makes of them.
GPU_LIST = (("single", 0), ("small2", 0), ("small3", 0), ("small5", 1), ("small7", 0), ("small7", 4),
            ("chain24", 0), ("chain24", 1), ("star", 0), ("star", 2), ("comb", 0), ("comb", 1), ("comb", 5),
            ("binary", 0), ("binary", 1), ("broom", 0), ("broom", 1), ("broom", 2), ("brooms2", 0), ("brooms2", 1), ("brooms2", 2),
            ("humanoid", 0), ("humanoid", 1), ("humanoid", 2), ("humanoid", 3), ("humanoid", 4), ("humanoid", 5),
            ("random", 0), ("random", 1), ("random", 2), ("random", 3), ("random", 4), ("random", 5),
            ("deep", 0), ("deep", 1), ("deep", 2), ("deep", 3), ("deep", 4), ("deep", 5), ("deep", 6))


def gpu_trees():
    return [make_tree(f, s) for f, s in GPU_LIST]


def small_family_trees():
    """a comb with a trunk of 8 (17 bodies) and a binary tree of 15 bodies: the two families whose listed trees all park more
    parents than the per-body state kernel (csrc/gmr_body_state.hip) has LDS for, at a size it takes"""
    return [tree_from_parents(_comb(8), "comb", 0, name="comb8-0"), tree_from_parents(_binary(15), "binary", 0, name="binary15-0")]


def body_state_lds(tree):
    """(ndof, parked parents, bytes of LDS per workgroup) of ``gmr_motion_body_state`` on a tree, as csrc/gmr_body_state.hip lays
    it out: 64 rows of dof_pos | dof_vel (odd stride), 13 floats x 64 per parked parent (a parent with a child that does not
    follow it immediately, at least one slot, as gmr_fk_create counts them), staging rows of 3, 4, 3, 3 floats x 4 bodies + 1 and
    four query scalars"""
    par = tree["parent"]
    ndof = int((tree["dof_dim"] > 0).sum())
    nslot = max(1, len({int(par[b]) for b in range(1, len(par)) if par[b] != b - 1}))
    return ndof, nslot, 4 * (64 * ((2 * ndof) | 1) + nslot * 13 * 64 + 64 * (3 * 13 + 17) + 4 * 64)


BODY_STATE_LDS_LIMIT = 64 * 1024


def checker_line(tree):
    """a tree as tests/cpp/fk_plan_check.cpp reads it"""
    return " ".join([tree["name"], str(len(tree["parent"]))] + [str(int(x)) for x in tree["parent"]] + [str(int(x)) for x in tree["dof_idx"]])


def parse_checker(stdout):
    """{(name, maxw, share): {field: int}} from the checker's lines"""
    out = {}
    for line in stdout.splitlines():
        w = line.split()
        if len(w) < 3 or "=" not in w[1]:
            continue
        kv = {k: int(v) for k, v in (x.split("=") for x in w[1:])}
        out[(w[0], kv["maxw"], kv["share"])] = kv
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(tree, B, seed=0):
    """(root_pos [B, 3], root_rot [B, 4] xyzw unit, dof [B, ndof]) float32: angles in +-3 rad with exact zeros, the exact identity
    among the roots.  Row 0 is a general frame (B = 1 walks it)."""
    rng = np.random.default_rng([seed, B, len(tree["parent"])])
    ndof = int((tree["dof_dim"] > 0).sum())
    dof = rng.uniform(-3.0, 3.0, size=(B, ndof))
    dof[rng.random((B, ndof)) < 0.03] = 0.0
    rq = rng.normal(size=(B, 4))
    rq /= np.linalg.norm(rq, axis=1, keepdims=True)
    rp = rng.normal(size=(B, 3))
    if B > 1:
        rq[1] = [0, 0, 0, 1]; dof[1] = 0.0
    if B > 2:
        rq[2] = [0, 0, 0, 1]
    if B > 3:
        dof[3] = 0.0
    return rp.astype(F), rq.astype(F), dof.astype(F)


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 walk
# ---------------------------------------------------------------------------------------------------------------------------
def _rotate(q, v):
    """R(q) v as the reference's quat_rotate defines it (torch_utils.py:65-75): for a unit q the rotation matrix of q applied to
    v; the reference applies the same expression to the un-normalised product of un-normalised local rotations, so that
    expression is the operation"""
    u, w = q[..., :3], q[..., 3:]
    return v * (2.0 * w ** 2 - 1.0) + 2.0 * w * np.cross(u, v) + 2.0 * u * np.sum(u * v, axis=-1, keepdims=True)


def _mul(a, b):
    """Hamilton product, xyzw: (w_a w_b - u_a . u_b,  w_a u_b + w_b u_a + u_a x u_b)"""
    ua, wa, ub, wb = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return np.concatenate([wa * ub + wb * ua + np.cross(ua, ub), wa * wb - np.sum(ua * ub, axis=-1, keepdims=True)], axis=-1)


def fk_f64(tree, root_pos, root_rot, dof):
    """pos_j = pos_p + R_p t_j,  rot_j = rot_p . r_j . axis-angle(axis_j, theta_j) in float64 on the float32 inputs.  Normalised is
    what KinematicsModel normalises: the hinge axis (axis / max(|axis|, 1e-9)) and the joint quaternion (quat_unit); neither the
    local rotations nor any product."""
    par, nb = tree["parent"], len(tree["parent"])
    rp, rq, dof = (np.asarray(x, dtype=np.float64) for x in (root_pos, root_rot, dof))
    B = len(rp)
    t = np.asarray(tree["local_translation"], dtype=F).astype(np.float64)
    r = np.asarray(tree["local_rotation"], dtype=F).astype(np.float64)
    axis = np.asarray(tree["axis"], dtype=np.float64)
    pos, rot = np.zeros((B, nb, 3)), np.zeros((B, nb, 4))
    pos[:, 0], rot[:, 0] = rp, rq
    for j in range(1, nb):
        p, d = int(par[j]), int(tree["dof_idx"][j])
        pos[:, j] = pos[:, p] + _rotate(rot[:, p], np.broadcast_to(t[j], (B, 3)))
        local = np.broadcast_to(r[j], (B, 4))
        if d >= 0:
            half = dof[:, d:d + 1] / 2.0
            n = axis[j] / max(np.linalg.norm(axis[j]), 1e-9)
            jq = np.concatenate([n * np.sin(half), np.cos(half)], axis=1)
            jq = jq / np.maximum(np.linalg.norm(jq, axis=1, keepdims=True), 1e-9)
            local = _mul(local, jq)
        rot[:, j] = _mul(rot[:, p], local)
    return pos, rot


def bound(e_ref, ref):
    """what the kernel may deviate from the float64 walk: twice the error of the reference's own float32 operation order plus one
    float32 spacing at the largest magnitude of the output (the factor 2: the kernel's own sin / cos instead of libm's, a couple
    of ulp per joint along a chain)"""
    return 2.0 * e_ref + float(np.spacing(F(np.abs(ref).max())))
