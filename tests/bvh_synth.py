"""Synthetic BVH material for the tests of the raw-BVH path (test_bvh_frames.py, test_bvh_raw_host.py): raw clips built
in memory on the topology of tests/golden/synthetic.bvh, the host reference of a raw clip, and a small BVH text writer."""
import os

import numpy as np

GOLDEN_BVH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthetic.bvh")


def golden_raw():
    from general_motion_retargeting_amd.utils import lafan1
    return lafan1.read_bvh_raw(GOLDEN_BVH)


def all_names(raw):
    return list(raw.names) + ["LeftFootMod", "RightFootMod"]


def make_raw(T, seed=0, channels=3, order="zyx", toggles=(), base=None, offset_scale=1.0, pos_scale=20.0):
    """A clip of T frames on the golden topology: smooth Euler angles that wrap through +-180 degrees (every wrap of a
    rotation channel flips the sign of the joint's quaternion) plus, at the frames in ``toggles``, a 360 degree step of
    every joint's first rotation channel (a flip of every joint at exactly that frame).  ``base``: another skeleton
    (:func:`skeleton_raw`); ``pos_scale``: the spread of the translation channels in centimetres."""
    from general_motion_retargeting_amd.utils import lafan1
    base = golden_raw() if base is None else base        # (an empty clip is falsy)
    rng = np.random.default_rng(seed)
    J = len(base.parents)
    t = np.arange(T, dtype=np.float64)[:, None, None]
    rate = rng.uniform(-7.0, 7.0, size=(1, J, 3))
    eul = rng.uniform(-180, 180, size=(1, J, 3)) + rate * t + 25.0 * np.sin(0.05 * t * rng.uniform(0.5, 2.0, size=(1, J, 3)))
    eul = (eul + 180.0) % 360.0 - 180.0
    step = np.zeros(T)
    for f in toggles:
        if 0 <= f < T:
            step[f:] = 360.0 - step[f:]
    eul[:, :, 0] += step[:, None]
    pos = rng.normal(size=(T, J, 3)) * pos_scale
    if channels == 3:
        rows = np.concatenate([pos[:, 0], eul.reshape(T, J * 3)], axis=1)
    else:
        rows = np.concatenate([pos, eul], axis=2).reshape(T, J * 6)
    offsets = base.offsets * offset_scale + rng.normal(size=base.offsets.shape) * 0.5
    return lafan1.BvhRaw(base.names, base.parents, offsets, channels, order, base.frametime, np.ascontiguousarray(rows))


def host_packed(raw, body_names):
    from general_motion_retargeting_amd.utils import lafan1
    return lafan1.packed_from_raw(raw, body_names)


def skeleton_raw(parents, seed=0, offset_sd=10.0):
    """An empty clip on any topology (joints ``j000`` ...), rest offsets N(0, offset_sd) centimetres: the ``base`` of
    :func:`make_raw` for skeletons that have no feet to name."""
    from general_motion_retargeting_amd.utils import lafan1
    J = len(parents)
    rng = np.random.default_rng([seed, J])
    return lafan1.BvhRaw([f"j{j:03d}" for j in range(J)], np.asarray(parents, dtype=np.int32), rng.normal(0.0, offset_sd, size=(J, 3)), 3, "zyx",
                         1.0 / 30.0, np.zeros((0, 3 + 3 * J)))


def host_packed_sel(raw, sel_pos, sel_rot):
    """:func:`host_packed` for rows given as (position joint, orientation joint) pairs -- what ``gmr_bvh_create`` takes --: the
    functions ``lafan1.packed_from_raw`` goes through (``bvh_from_raw``, ``quat_fk``, its Y-up cm -> Z-up m step) without the two
    ``FootMod`` rows, which need joints called LeftFoot, LeftToe, RightFoot and RightToe."""
    from general_motion_retargeting_amd.utils import lafan1
    data = lafan1.bvh_from_raw(raw)
    grot, gpos = lafan1.quat_fk(data.quats, data.pos, data.parents)
    orient = lafan1._quat_mul(np.broadcast_to(lafan1._ROT_QUAT, grot.shape), grot)
    position = gpos @ lafan1._ROT.T / 100
    return np.concatenate([position[:, list(sel_pos)], orient[:, list(sel_rot)]], axis=-1)


def write_bvh(path, names, parents, offsets, rows, frametime=1.0 / 30.0):
    """BVH text with LAFAN1's layout: six channels at the root, three ZYX rotations per joint, an End Site per leaf."""
    J = len(names)
    kids = [[j for j in range(J) if parents[j] == i] for i in range(J)]
    out = ["HIERARCHY"]

    def emit(j, d):
        ind = "\t" * d
        out.append(f"{ind}{'ROOT' if parents[j] < 0 else 'JOINT'} {names[j]}")
        out.append(ind + "{")
        out.append(f"{ind}\tOFFSET {float(offsets[j][0])!r} {float(offsets[j][1])!r} {float(offsets[j][2])!r}")
        if parents[j] < 0:
            out.append(f"{ind}\tCHANNELS 6 Xposition Yposition Zposition Zrotation Yrotation Xrotation")
        else:
            out.append(f"{ind}\tCHANNELS 3 Zrotation Yrotation Xrotation")
        for k in kids[j]:
            emit(k, d + 1)
        if not kids[j]:
            out.extend([f"{ind}\tEnd Site", ind + "\t{", f"{ind}\t\tOFFSET 0.0 0.0 0.0", ind + "\t}"])
        out.append(ind + "}")

    emit(0, 0)
    out += ["MOTION", f"Frames: {len(rows)}", f"Frame Time: {frametime:.6f}"]
    out += [" ".join(repr(float(v)) for v in r) for r in rows]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
