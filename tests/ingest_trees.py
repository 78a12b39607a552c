"""One catalogue of skeletons for the clip ingest kernels (csrc/gmr_smplx.hip, csrc/gmr_bvh.hip): a fixed, named list of
topologies from the generators of tests/fk_trees.py, each with a deterministic selection, plus the sweep of generated cases the
stand-alone checker (tests/cpp/ingest_prog_check.cpp) replays.  NumPy only; used by tests/test_ingest_prog_host.py (CPU) and
tests/test_smplx_trees.py, tests/test_bvh_trees.py (GPU).

What the walk programs make of the catalogue (asserted from the checker's output in tests/test_ingest_prog_host.py):
  SMPL-X  single, pair, small3, small5    J = 1, 2, 3, 5
          chain64        depth 64: align LDS 64 x 2048 = 131 072 B, nslot 1 (nothing parked)
          star64         nslot 1: the root lives in the register slot only and is reloaded 62 times
          binary63       nslot 5: four LDS slots live at once under the register slot
          comb43, humanoid, random21      nslot 2 .. 4
          caterpillar27  J = 55, nslot 27: joints LDS 26 x 6144 = 159 744 B, the largest accepted
          caterpillar28  J = 57, nslot 28: 165 888 B, refused ("tree too deep")
          chain65        J = 65, refused
  batch   chain22, star22, humanoid22, binary22, nested22   batch_nslot 1, 1, 2, 3, 4 in front of the pose tile
          caterpillar22  nslot 10: batch joints LDS 9 x 6144 + 16 128 = 71 424 B (above 48 KB)
  BVH     the accepted trees above with a (position, orientation) selection, and
          wide256        J = 256, fifteen chains interleaved in joint order; the three highest tips: closure 52, slots reused
          chain64_tip    closure exactly 64 (bit 63 of the flip mask); chain65_tip: refused
          star45_sel44   nsel + nslot = 45: 161 280 B, accepted; star46_sel45: 164 864 B, refused
"""
import numpy as np

import fk_trees as ft

SX_MAX_JOINTS, BVH_MAX_JOINTS, BVH_MAX_STEPS, BVH_MAX_ROWS, BODY_JOINTS = 64, 256, 64, 64, 22
LDS_LIMIT = 160 * 1024 - 1024
LDS_DEFAULT = 48 * 1024


# ---------------------------------------------------------------------------------------------------------------------------
# topologies
# ---------------------------------------------------------------------------------------------------------------------------
def caterpillar(spine):
    """a spine of ``spine`` joints with two children each: the first continues the spine, the second is a leaf"""
    par, s = [-1], 0
    for _ in range(spine):
        par.extend([s, s])
        s = len(par) - 2
    return par


def interleaved_chains(nchain, length):
    """``nchain`` chains of ``length`` joints under the root, numbered level by level: consecutive joints belong to different
    chains, so in joint order (the BVH walk) no parent is the previous step"""
    par = [-1]
    for lvl in range(length):
        for c in range(nchain):
            par.append(0 if lvl == 0 else 1 + c + nchain * (lvl - 1))
    return par


def humanoid22():
    """pelvis, two spine joints, legs of four and three from the pelvis, two arms of three with two fingers each and a neck +
    head from the chest: pelvis, chest and a wrist are parked at once"""
    par = [-1, 0, 1]
    for start, n, fingers in ((0, 4, 0), (0, 3, 0), (2, 3, 2), (2, 3, 2), (2, 2, 0)):
        last = start
        for _ in range(n):
            par.append(last)
            last = len(par) - 1
        par.extend([last] * fingers)
    return par


def cut(parent, J):
    """the first ``J`` joints of a tree (parents precede children, so this is a tree)"""
    return list(parent[:J])


def closure(parent, joints):
    keep = set()
    for j in joints:
        while j >= 0 and j not in keep:
            keep.add(j)
            j = int(parent[j])
    return keep


# ---------------------------------------------------------------------------------------------------------------------------
# selections
# ---------------------------------------------------------------------------------------------------------------------------
def smplx_selection(parent, rng, nsel=None, must=()):
    """``nsel`` distinct joints in random order (about a third of the tree by default), ``must`` among them"""
    J = len(parent)
    nsel = max(1, len(must), J // 3) if nsel is None else nsel
    rest = [j for j in rng.permutation(J) if j not in must]
    sel = list(must) + [int(j) for j in rest[: nsel - len(must)]]
    return [int(sel[i]) for i in rng.permutation(len(sel))]


def bvh_selection(parent, rng, nsel, pool=None, max_steps=BVH_MAX_STEPS):
    """(sel_pos, sel_rot): rows of one joint (j, j), rows whose position and orientation joints are unrelated, one joint used by
    four rows and the root as an orientation-only partner, all drawn from ``pool`` while the ancestor closure stays within
    ``max_steps`` joints"""
    J = len(parent)
    pool = list(range(J)) if pool is None else list(pool)
    keep, sp, sr = set(), [], []

    def take(a, b):
        new = closure(parent, [a, b]) | keep
        if len(new) > max_steps:
            return False
        keep.update(new)
        sp.append(int(a)); sr.append(int(b))
        return True

    star = int(pool[int(rng.integers(len(pool)))])
    for r in range(200 * nsel):
        if len(sp) >= nsel:
            break
        a, b = (int(pool[int(i)]) for i in rng.integers(len(pool), size=2))
        kind = len(sp) % 4 if len(sp) >= 4 else -1
        if len(sp) < 2:
            take(star, star)                       # the joint of four rows: twice as (j, j) ...
        elif len(sp) == 2:
            take(star, a)                          # ... once as a position ...
        elif len(sp) == 3:
            take(a, star)                          # ... once as an orientation
        elif kind == 0:
            take(a, 0)                             # the root: orientation of a row whose position is elsewhere
        elif kind == 1:
            take(a, b)                             # unrelated
        else:
            take(a, a)
    if not keep:
        keep.add(0)
    while len(sp) < nsel:                          # (a closure at its limit: repeat joints already walked)
        j = sorted(keep)[int(rng.integers(len(keep)))]
        sp.append(j); sr.append(j)
    return sp, sr


# ---------------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng([ord(c) for c in name])


def _entry(name, parent, sel=None, bvh=None, batch=False, smplx=True, refused=None):
    return {"name": name, "parent": np.array(parent, dtype=np.int32), "sel": sel, "bvh": bvh, "batch": batch, "smplx": smplx, "refused": refused}


def _build():
    out = []

    def add(name, parent, nsel=None, must=(), bvh_nsel=None, **kw):
        rng = _rng(name)
        sel = smplx_selection(parent, rng, nsel, must) if kw.get("smplx", True) and len(parent) <= SX_MAX_JOINTS else None
        bvh = None
        if bvh_nsel:
            bvh = bvh_selection(parent, rng, bvh_nsel)
        out.append(_entry(name, parent, sel, bvh, **kw))

    add("single", [-1], bvh_nsel=1)
    add("pair", [-1, 0], nsel=2, bvh_nsel=3)
    add("small3", ft._random(_rng("small3"), 3), bvh_nsel=4)
    add("small5", ft._random(_rng("small5"), 5), nsel=3, bvh_nsel=7)
    add("chain64", ft._chain(64), nsel=9, must=(63,))
    add("star64", ft._star(64), nsel=20, bvh_nsel=20)
    add("binary63", ft._binary(63), nsel=21, bvh_nsel=24)
    add("comb43", ft._comb(21), bvh_nsel=16)
    add("humanoid", ft._humanoid(_rng("humanoid")), bvh_nsel=14)
    add("random21", ft._random(_rng("random21"), 21), bvh_nsel=12)
    add("caterpillar27", caterpillar(27), nsel=14, must=(54,), bvh_nsel=20)
    add("caterpillar28", caterpillar(28), nsel=14, refused="tree too deep")
    add("chain65", ft._chain(65), smplx=True, refused="1 <= J <= 64")
    # the batch entry points read joints 0 .. 21
    add("chain22", ft._chain(22), nsel=6, must=(21,), batch=True)
    add("star22", ft._star(22), nsel=9, batch=True)
    add("binary22", ft._binary(22), nsel=22, batch=True)
    add("humanoid22", humanoid22(), nsel=22, batch=True)
    add("nested22", caterpillar(5) + list(range(9, 20)), nsel=22, batch=True)
    add("caterpillar22", caterpillar(10) + [0], nsel=22, batch=True)
    # BVH only
    wide = interleaved_chains(15, 17)
    rng = _rng("wide256")
    out.append(_entry("wide256", wide, bvh=bvh_selection(wide, rng, 12, pool=[253, 254, 255, 238, 239, 240, 223, 224, 225]), smplx=False))
    c64, c65 = ft._chain(64), ft._chain(65)
    out.append(_entry("chain64_tip", c64, bvh=([63, 63, 31, 63, 0, 17], [63, 0, 63, 62, 63, 17]), smplx=False))
    out.append(_entry("chain65_tip", c65, bvh=([64, 3], [64, 0]), smplx=False, refused="more than 64 joints"))
    out.append(_entry("star45_sel44", ft._star(45), bvh=(list(range(1, 45)), [0] + list(range(2, 45))), smplx=False))
    out.append(_entry("star46_sel45", ft._star(46), bvh=(list(range(1, 46)), [0] + list(range(2, 46))), smplx=False, refused="do not fit the LDS"))
    return out


CATALOGUE = _build()
BY_NAME = {e["name"]: e for e in CATALOGUE}


def smplx_trees(accepted=True):
    return [e for e in CATALOGUE if e["smplx"] and (e["refused"] is None) == accepted]


def batch_trees():
    return [e for e in CATALOGUE if e["batch"]]


def bvh_trees(accepted=True):
    return [e for e in CATALOGUE if e["bvh"] is not None and (e["refused"] is None) == accepted]


# ---------------------------------------------------------------------------------------------------------------------------
# the checker's cases
# ---------------------------------------------------------------------------------------------------------------------------
def _ints(xs):
    return " ".join(str(int(x)) for x in xs)


def smplx_line(name, parent, sel=None):
    sel = [] if sel is None else list(sel)
    return f"S {name} {len(parent)} {_ints(parent)} {len(sel)} {_ints(sel)}".rstrip()


def bvh_line(name, parent, sel_pos, sel_rot):
    return f"B {name} {len(parent)} {_ints(parent)} {len(sel_pos)} {_ints(sel_pos)} {_ints(sel_rot)}"


def catalogue_lines():
    """every catalogue entry as the checker reads it: the all-joints handle and the selection for SMPL-X, the pair selection for
    BVH (``name``, ``name/sel``, ``name/bvh``)"""
    lines = []
    for e in CATALOGUE:
        if e["smplx"]:
            lines.append(smplx_line(e["name"], e["parent"]))
            if e["sel"] is not None:
                lines.append(smplx_line(e["name"] + "/sel", e["parent"], e["sel"]))
        if e["bvh"] is not None:
            lines.append(bvh_line(e["name"] + "/bvh", e["parent"], *e["bvh"]))
    return lines


def _sweep_topology(i, seed, limit):
    """the families of fk_trees.py in turn, cut to ``limit`` joints, and for BVH (limit 256) every fourth tree grown beyond 64
    joints by grafting further family trees under random joints"""
    fam = ft.FAMILIES[i % len(ft.FAMILIES)]
    rng = np.random.default_rng([ft.FAMILIES.index(fam), seed + i // len(ft.FAMILIES), limit])
    par = list(ft._topology(fam, rng))
    if limit > SX_MAX_JOINTS and i % 4 == 3:
        while len(par) < limit:
            sub = ft._topology(ft.FAMILIES[int(rng.integers(len(ft.FAMILIES)))], rng)
            at, base = int(rng.integers(len(par))), len(par)
            par.extend(at if p < 0 else base + p for p in sub)
    return cut(par, int(rng.integers(1, limit + 1)) if i % 5 == 4 else limit), rng


def sweep_lines(n, seed=0):
    """``n`` generated cases, SMPL-X and BVH in turn: random selections of 1 .. min(J, 64) rows (for SMPL-X every seventh the
    all-joints handle, every eleventh with a duplicate; for BVH position / orientation pairs that repeat joints, the closure
    unbounded -- many are refused for their steps or their LDS)"""
    lines = []
    for i in range(n):
        if i % 2 == 0:
            par, rng = _sweep_topology(i // 2, seed, SX_MAX_JOINTS)
            J = len(par)
            sel = None if i % 14 == 0 else smplx_selection(par, rng, int(rng.integers(1, J + 1)))
            if sel is not None and i % 22 == 2 and len(sel) >= 2:
                sel[-1] = sel[0]
            lines.append(smplx_line(f"s{i}", par, sel))
        else:
            par, rng = _sweep_topology(i // 2, seed, BVH_MAX_JOINTS)
            J = len(par)
            nsel = int(rng.integers(1, min(J, BVH_MAX_ROWS) + 1))
            if i % 3 == 0:                      # anything: the closure is what it is
                sp, sr = rng.integers(J, size=nsel), rng.integers(J, size=nsel)
            else:                               # a closure at or below a random limit up to 64 steps
                sp, sr = bvh_selection(par, rng, nsel, max_steps=int(rng.integers(1, BVH_MAX_STEPS + 1)))
            lines.append(bvh_line(f"b{i}", par, sp, sr))
    return lines


def parse_checker(stdout):
    """{name: {field: int}} from the checker's lines (``kind`` as the letter)"""
    out = {}
    for line in stdout.splitlines():
        w = line.split()
        if len(w) < 2 or "=" not in w[1]:
            continue
        kv = dict(x.split("=") for x in w[1:])
        out[w[0]] = {k: (v if k == "kind" else int(v)) for k, v in kv.items()}
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# inputs of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
FRAME_COUNTS = (1, 2, 63, 64, 65, 130)


def smplx_inputs(entry, N, seed=0):
    """(j_rest f64[J, 3], full_pose f32[N, J, 3], transl f32[N, 3]): poses a random walk around N(0, 0.6) rad; rest offsets
    scaled by the tree's depth so that no joint lies further than about 2.5 from the root (chain64: 64 offsets of 0.03).  In
    ``small5`` joint 1 is held at exact zeros and joint 2 at |v| = 1e-5."""
    par = entry["parent"]
    J = len(par)
    rng = np.random.default_rng([seed, N, J] + [ord(c) for c in entry["name"]])
    depth = int(ft.depth_of(par).max()) + 1
    s = min(0.15, 2.0 / (1.7 * depth))
    j_rest = np.zeros((J, 3))
    j_rest[0] = rng.normal(0, 0.2, size=3)
    for j in range(1, J):
        j_rest[j] = j_rest[par[j]] + rng.normal(0, s, size=3)
    pose = (rng.normal(0, 0.6, size=(1, J, 3)) + np.cumsum(rng.normal(0, 0.05, size=(N, J, 3)), axis=0)).astype(np.float32)
    if entry["name"] == "small5":
        pose[:, 1] = 0.0
        pose[:, 2] = np.float32(1e-5) * np.array([0.6, 0.0, -0.8], dtype=np.float32)
    transl = rng.normal(0, 0.3, size=(N, 3)).astype(np.float32)
    return j_rest, pose, transl


def target_times(N):
    """the alignments of a clip of N frames: None (frame by frame) and np.linspace(0, N - 1, Nout) for Nout in {1, N // 4, N}"""
    outs = [None]
    if N >= 2:
        outs += [np.linspace(0, N - 1, n) for n in sorted({1, N // 4, N}) if n >= 1]
    return outs
