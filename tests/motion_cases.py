"""Libraries, clips and queries at the edges of the motion library's kernels (csrc/gmr_motion.hip, csrc/gmr_motion_sample.h), and
the high-precision evaluations they are compared with.  NumPy and mpmath only; used by tests/test_motion_edges_host.py (CPU) and
tests/test_motion_edges.py (GPU).

* ``width_motions(ndof)``: ragged batches with empty clips whose column count 3 + ndof reaches every group width of
  motion_stats_kernel, ``ncol == G``, ``ncol == G + 1``, exactly 64 columns and two and three column sweeps;
* ``offset_motion()``, ``NAN_PLACES``: one clip of 300 frames and 66 columns whose values sit far from zero (a one-pass or float32
  variance loses every digit of the std there), and where a single NaN goes for the four fills that follow its carry;
* ``stats_reference``: mean and unbiased std by mpmath on the float32 data;
* ``angvel_clip()``, ``angvel_reference(mode)``: frame pairs at the edges of the quaternion log and mpmath's
  ``rotvec(q_i q_{i-1}^-1) / dt`` of the float32 quaternions;
* ``slerp_motions()``, ``slerp_queries()``, ``slerp_f64``: frame pairs at the switches of the float32 slerp and the float64
  evaluation of the same statement.

Every builder is deterministic; the references are computed once per process and handed out read-only."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_mirror as mm  # noqa: E402

F = np.float32
FPS = (30.0, 50.0, 120.0, 29.97)

# ---------------------------------------------------------------------------------------------------------------------------
# A. fill and stats at every width
# ---------------------------------------------------------------------------------------------------------------------------
WIDTH_NDOF = (0, 1, 2, 5, 6, 13, 29, 61, 62, 63, 130)         # ncol = 3, 4, 5, 8, 9, 16, 32, 64, 65, 66, 133
WIDTH_LENS = (1, 2, 0, 63, 64, 65, 0, 129, 3, 0)             # empty clips in the middle, next to a one-frame clip, and last
WIDTH_NBODY = (0, 1, 3)


def group_width(ncol):
    """the G of motion_stats_kernel and the number of column sweeps"""
    G = 4
    while G < ncol and G < 64:
        G <<= 1
    return G, (ncol + 63) // 64


def quat_track(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    for i in range(1, n):          # thirds: a random jump, a small step, a larger step; every fifth in the other hemisphere
        if i % 3:
            q[i] = q[i - 1] + rng.normal(size=4) * (3e-3 if i % 3 == 1 else 0.2)
            q[i] /= np.linalg.norm(q[i])
            if i % 5 == 0:
                q[i] = -q[i]
    return q


def width_motions(ndof):
    """float64 clips of WIDTH_LENS frames with ``ndof`` dofs; neighbouring clips differ in fps, so a velocity that takes the dt of the
    wrong clip shows"""
    rng = np.random.default_rng([41, ndof])
    nbody = WIDTH_NBODY[WIDTH_NDOF.index(ndof) % 3]
    return [{"fps": FPS[c % 4], "root_pos": rng.normal(0, 0.5, size=(n, 3)) + np.array([0.3, -0.2, 0.8]), "root_rot": quat_track(rng, n),
             "dof_pos": rng.uniform(-1.2, 1.2, size=(n, ndof)),
             "local_body_pos": rng.normal(size=(n, nbody, 3)).astype(F) if nbody else None} for c, n in enumerate(WIDTH_LENS)]


OFFSET_NDOF, OFFSET_FRAMES = 63, 300                          # 66 columns: a full sweep of 64 and a second one of 2
OFFSET_COLUMN = 64                                            # (of the stats row: dof 61, in the second sweep)
# (row, column of the stats row) of the single NaN of each fill.  With 66 columns G = 64: a wavefront takes a row per
# instruction, wavefront w the rows t = w (mod 4).  Wavefront 0 lane 0; the last row (wavefront 3); wavefront 1 at a column of
# the first sweep; the second sweep (wavefront 2).
NAN_PLACES = ((0, 0), (299, 2), (5, 7), (150, 65))


def offset_motion(nan_at=None):
    rng = np.random.default_rng(43)
    n = OFFSET_FRAMES
    m = {"fps": 50.0, "root_pos": 1000.0 + rng.uniform(-1e-3, 1e-3, size=(n, 3)), "root_rot": quat_track(rng, n),
         "dof_pos": rng.uniform(-1.2, 1.2, size=(n, OFFSET_NDOF)), "local_body_pos": None}
    m["dof_pos"][:, OFFSET_COLUMN - 3] = -500.0 + rng.uniform(-1e-3, 1e-3, size=n)
    if nan_at is not None:
        row, col = nan_at
        (m["root_pos"] if col < 3 else m["dof_pos"])[row, col if col < 3 else col - 3] = np.nan
    return m


def stats_reference(root_pos, dof_pos):
    """(mean, std) float64 [3 + ndof] of float32 rows: the sum, the squared deviations from the exact mean and the square root in
    mpmath (80 digits), rounded once to float64.  std is NaN for one frame, both are NaN for none."""
    import mpmath as mp
    import mp_lie  # noqa: F401  (sets the working precision)
    x = np.concatenate([np.asarray(root_pos, dtype=F), np.asarray(dof_pos, dtype=F)], axis=1)
    T, n = x.shape
    mean, std = np.full(n, np.nan), np.full(n, np.nan)
    for j in range(n if T else 0):
        col = [mp.mpf(float(v)) for v in x[:, j]]
        m = mp.fsum(col) / T
        mean[j] = float(m)
        if T > 1:
            std[j] = float(mp.sqrt(mp.fsum([(v - m) ** 2 for v in col]) / (T - 1)))
    return mean, std


@functools.lru_cache(maxsize=None)
def library_stats_reference(ndof):
    """per clip of ``width_motions(ndof)`` (``ndof`` in WIDTH_NDOF) or of the offset clip (``ndof = 'offset'``): mean and std
    [C, 3 + ndof]"""
    motions = [offset_motion()] if ndof == "offset" else width_motions(ndof)
    res = [stats_reference(np.asarray(m["root_pos"]).astype(F), np.asarray(m["dof_pos"]).astype(F)) for m in motions]
    out = np.array([r[0] for r in res]), np.array([r[1] for r in res])
    for a in out:
        a.setflags(write=False)
    return out


def spacings_off(got, ref):
    """|got - ref| in float32 spacings of ``ref`` (float64 reference of a float32 result); where the reference is NaN the result has to
    be NaN too (inf otherwise)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    with np.errstate(invalid="ignore"):
        u = np.abs(got - ref) / np.spacing(np.abs(np.where(nan, 0.0, ref)).astype(F)).astype(np.float64)
    return np.where(nan, np.where(np.isnan(got), 0.0, np.inf), np.where(np.isnan(got), np.inf, u))


# ---------------------------------------------------------------------------------------------------------------------------
# B1. angular velocity
# ---------------------------------------------------------------------------------------------------------------------------
ANGVEL_FPS = 50.0
ANGVEL_KINDS = ("same", "adjacent", "1e-6", "1e-3", "0.2", "norm0.5", "norm2")
ANGVEL_PI_KINDS = ("pi-", "pi+", "reset", "pi")               # "reset" leaves the exact identity in front of the exact half turn
ANGVEL_PAIRS = 399


def _angvel_schedule():
    sched = [(k, twin) for twin in (False, True) for k in ANGVEL_KINDS + ANGVEL_PI_KINDS]
    cycle = 0
    while len(sched) < ANGVEL_PAIRS:                          # the pairs at pi stay few: their sign is arbitrary (see angvel_reference)
        sched += [(k, bool(cycle % 2)) for k in ANGVEL_KINDS + ("jump",)]
        cycle += 1
    return sched[:ANGVEL_PAIRS]


@functools.lru_cache(maxsize=None)
def _angvel_rot():
    rng = np.random.default_rng(97)
    q = [np.array([0.3, -0.2, 0.1, 0.9]) / np.linalg.norm([0.3, -0.2, 0.1, 0.9])]

    def step(prev, angle):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        d = np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])
        return mm.qmul_xyzw(d[None], prev[None])[0]          # d * prev: the world-frame step of frame i is d

    for kind, twin in _angvel_schedule():
        last = q[-1].astype(F)
        prev = last.astype(np.float64) / np.linalg.norm(last.astype(np.float64))
        if kind == "same":
            nxt = last.astype(np.float64)
        elif kind == "adjacent":                              # one component moved by one float32 spacing
            nxt = last.copy()
            k = int(rng.integers(4))
            nxt[k] = np.nextafter(nxt[k], F(np.inf) if rng.random() < 0.5 else F(-np.inf))
            nxt = nxt.astype(np.float64)
        elif kind in ("1e-6", "1e-3", "0.2"):
            nxt = step(prev, float(kind))
        elif kind in ("norm0.5", "norm2"):
            nxt = step(prev, 0.05) * float(kind[4:])
        elif kind in ("pi-", "pi+"):
            nxt = step(prev, np.pi + (6e-7 if kind == "pi+" else -6e-7))
        elif kind == "reset":
            nxt = np.array([0.0, 0.0, 0.0, 1.0])
        elif kind == "pi":
            nxt = np.array([1.0, 0.0, 0.0, 0.0])
        else:
            nxt = step(prev, float(rng.uniform(0.3, 2.5)))
        q.append(-nxt if twin else nxt)
    rot = np.array(q)
    rot.setflags(write=False)
    return rot


def angvel_clip():
    """one clip of 400 frames whose consecutive quaternions are: identical, float32 neighbours, steps of 1e-6, 1e-3 and 0.2 rad,
    of norm 0.5 and 2, within 1e-6 of a half turn on both sides and exactly a half turn, each also with the second quaternion
    negated"""
    rot = _angvel_rot()
    rng = np.random.default_rng(98)
    n = len(rot)
    return {"fps": ANGVEL_FPS, "root_pos": rng.normal(size=(n, 3)), "root_rot": rot.copy(), "dof_pos": rng.uniform(-1, 1, size=(n, 1)),
            "local_body_pos": None}


@functools.lru_cache(maxsize=None)
def angvel_reference(mode):
    """(root_ang_vel float64 [T, 3], near_pi bool [T], side float64 [T]) of ``angvel_clip()``: mpmath's rotvec(q_i q_{i-1}^-1) / dt on the float32
    quaternions (mp_lie.so3_log: angle * axis with the angle folded into (-pi, pi], no normalisation needed), dt = 1.0 / fps as
    the float64 the library divides by; row 0 copies row 1.  ``near_pi``: the angle is within 1e-6 of pi, where the side of the
    shortest arc -- the sign of the whole vector -- hangs on the last bit of the product's scalar part; ``side`` is the unfolded
    angle 2 atan2(|v|, w) minus pi."""
    import mpmath as mp
    import mp_lie as ml
    q = _angvel_rot().astype(F)
    dt = mp.mpf(1.0 / ANGVEL_FPS)
    order = {"world": (3, 0, 1, 2), "reference": (2, 3, 0, 1)}[mode]      # wxyz of what each mode reads
    ref, near, side = np.zeros((len(q), 3)), np.zeros(len(q), dtype=bool), np.full(len(q), -np.pi)
    for i in range(1, len(q)):
        a, b = ([mp.mpf(float(q[j][k])) for k in order] for j in (i - 1, i))
        d = ml.qmul(b, [a[0], -a[1], -a[2], -a[3]])
        ref[i] = [float(c / dt) for c in ml.so3_log(d)]
        n = mp.sqrt(d[1] ** 2 + d[2] ** 2 + d[3] ** 2)
        if n != 0:
            side[i] = float(2 * mp.atan2(n, d[0]) - mp.pi)
        near[i] = abs(side[i]) < 1e-6
    ref[0], near[0], side[0] = ref[1], near[1], side[1]
    for a in (ref, near, side):
        a.setflags(write=False)
    return ref, near, side


def angvel_floor_needed(got, mode):
    """How ``got`` (float32 [T, 3]) sits against the reference.  The bound of a component is one float32 spacing of the reference
    value or, where that is smaller, an absolute floor c 2^-52 / dt; returned is the largest c any component needs that is more
    than a spacing off (0.0: every component is within its spacing), and the number of rows compared up to the sign of the whole
    vector (``near_pi``)."""
    ref, near, _ = angvel_reference(mode)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    unit = 2.0 ** -52 * ANGVEL_FPS

    def need(g):
        err = np.abs(g - ref)
        return np.where(err <= np.spacing(np.abs(ref).astype(F)).astype(np.float64), 0.0, err / unit).max(axis=1)

    c = np.where(near, np.minimum(need(got), need(-got)), need(got))
    return float(c.max()), int(near.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# B2. the float32 slerp of the sampler
# ---------------------------------------------------------------------------------------------------------------------------
SLERP_DOTS = (0.9995, 0.0, 1.0)
SLERP_DELTAS = (-1e-6, -3e-7, -1e-7, 0.0, 1e-7, 3e-7, 1e-6)
SLERP_REPEATS = 4
# blend: 0; the smallest positive double, whose float32 image is 0 while the frame pair is still blended; a half; 1 - 2^-24
SLERP_BLENDS = (0.0, 5e-324, 0.5, 1.0 - 2.0 ** -24)


@functools.lru_cache(maxsize=None)
def slerp_pairs():
    """float32 unit quaternion pairs [P, 2, 4] (xyzw) whose dot lies within 1e-6 of 0.9995 (the switch between the normalised
    lerp and the slerp), of 0 (the hemisphere flip) and of 1, on both sides, then q2 = -q1 exactly; and each of them again with
    q2 negated"""
    rng = np.random.default_rng(131)
    pairs = []
    for d0 in SLERP_DOTS:
        for delta in SLERP_DELTAS:
            for _ in range(SLERP_REPEATS):
                c = min(d0 + delta, 1.0)
                q1 = rng.normal(size=4)
                q1 /= np.linalg.norm(q1)
                u = rng.normal(size=4)
                u -= q1 * (u @ q1)
                u /= np.linalg.norm(u)
                pairs.append((q1, c * q1 + np.sqrt(max(0.0, 1.0 - c * c)) * u))
    q1 = np.array([0.5, -0.1, 0.7, 0.2]) / np.linalg.norm([0.5, -0.1, 0.7, 0.2])
    pairs.append((q1.astype(F).astype(np.float64), -q1.astype(F).astype(np.float64)))
    pairs += [(a, -b) for a, b in pairs]
    out = np.array(pairs).astype(F)
    out.setflags(write=False)
    return out


def slerp_motions():
    """one clip of two frames per pair, 1 frame per second: a time in [0, 1) is the blend itself"""
    rng = np.random.default_rng(132)
    return [{"fps": 1.0, "root_pos": rng.normal(size=(2, 3)), "root_rot": p.astype(np.float64), "dof_pos": rng.uniform(-1, 1, size=(2, 3)),
             "local_body_pos": None} for p in slerp_pairs()]


def slerp_queries():
    P = len(slerp_pairs())
    return np.repeat(np.arange(P), len(SLERP_BLENDS)).astype(np.int32), np.tile(np.array(SLERP_BLENDS), P)


def slerp_f64(mirror, clip, time, loop):
    """root_rot [N, 4] xyzw of a ``motion_mirror.Library``'s sampler, the statement of csrc/gmr_motion_sample.h evaluated in float64
    on the float32 rows and the float32 weights.  WHICH side of a switch a query is on (the hemisphere, dot > 0.9995) is decided
    as the statement decides it, from its float32 dot: the two sides are different functions, and only the chosen one is
    evaluated here."""
    ok, lo, hi, blend = mirror.frames(clip, time, loop)
    assert ok.all()
    w0, w1 = (1.0 - blend).astype(F), blend.astype(F)
    q1, q2 = mirror.root_rot[lo][:, [3, 0, 1, 2]], mirror.root_rot[hi][:, [3, 0, 1, 2]]
    dot = q1[:, 0] * q2[:, 0]
    for k in (1, 2, 3):
        dot = dot + q1[:, k] * q2[:, k]
    sgn = np.where(dot < 0, F(-1), F(1))
    near = np.clip(sgn * dot, F(-1), F(1)) > F(0.9995)
    a, b = q1.astype(np.float64), sgn.astype(np.float64)[:, None] * q2.astype(np.float64)
    w0, w1 = w0.astype(np.float64)[:, None], w1.astype(np.float64)[:, None]
    d = np.clip((a * b).sum(axis=1), -1.0, 1.0)[:, None]
    lin = w0 * a + w1 * b
    with np.errstate(invalid="ignore", divide="ignore"):
        nlerp = lin / np.linalg.norm(lin, axis=1, keepdims=True)
        th0 = np.arccos(d)
        th = th0 * w1
        slerp = (np.cos(th) - d * np.sin(th) / np.sin(th0)) * a + np.sin(th) / np.sin(th0) * b
    r = np.where((lo == hi)[:, None], a, np.where(near[:, None], nlerp, slerp))
    return r[:, [1, 2, 3, 0]]
