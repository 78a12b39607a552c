"""The BVH ingest kernels (csrc/gmr_bvh.hip) off the 22-joint LAFAN1 topology: every accepted BVH skeleton of
tests/ingest_trees.py -- up to 256 joints, closures of exactly 64 steps (bit 63 of the flip mask), slots that are reused,
rows whose position and orientation joints are unrelated, nsel + nslot at the LDS limit -- against the NumPy host path
(bvh_synth.host_packed_sel: lafan1.bvh_from_raw, quat_fk and the Y-up -> Z-up step), with the bound and the sign check of
tests/test_bvh_frames.py.  tests/test_ingest_prog_host.py proves the programs' slot indices in bounds and asserts which paths
this list reaches."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_synth  # noqa: E402
import fk_trees as ft  # noqa: E402
import ingest_trees as it  # noqa: E402
from test_bvh_frames import _close, _one  # noqa: E402

pytestmark = pytest.mark.gpu
TOGGLES = (1, 63, 64, 65, 129)


def _scales(e):
    """rest offsets and translation channels in centimetres, so that no position leaves about 4 m: a joint lies at most
    depth x (|offset| or |translation|) from the root, each about 1.7 x the scale"""
    depth = int(ft.depth_of(e["parent"]).max()) + 1
    s = min(10.0, 300.0 / (1.7 * depth))
    return s, s


def _raw(e, T, seed, channels, order, toggles):
    off, pos = _scales(e)
    base = bvh_synth.skeleton_raw(e["parent"], seed=seed, offset_sd=off)
    return bvh_synth.make_raw(T, seed=seed, channels=channels, order=order, toggles=toggles, base=base, pos_scale=pos)


def _handle(lib, e, channels, order, sel=None):
    sp, sr = e["bvh"] if sel is None else sel
    return lib.BvhHandle(e["parent"], channels, order, sp, sr)


@pytest.fixture(scope="module")
def lib():
    from general_motion_retargeting_amd import _lib
    _lib.require_gpu()
    return _lib


def _ids(entries):
    return [e["name"] for e in entries]


@pytest.mark.parametrize("e", it.bvh_trees(), ids=_ids(it.bvh_trees()))
def test_every_skeleton_both_layouts_two_orders(lib, e):
    """T = 130 with a flip of every joint at frames 1, 63, 64, 65 and 129, channels 3 and 6, Euler orders zyx and xzy"""
    sp, sr = e["bvh"]
    for channels in (3, 6):
        for order in ("zyx", "xzy"):
            raw = _raw(e, 130, 5 + channels, channels, order, TOGGLES)
            ref = bvh_synth.host_packed_sel(raw, sp, sr)
            assert np.abs(ref[..., :3]).max() < 4.0, np.abs(ref[..., :3]).max()
            out = _one(_handle(lib, e, channels, order), raw)
            print(f"{e['name']} ch={channels} {order}: |pos| {np.abs(ref[..., :3]).max():.2f} err {np.abs(out - ref).max():.3e}")
            _close(out, ref)
    # the toggles did flip every walked joint at those frames
    from general_motion_retargeting_amd.utils import lafan1
    q = lafan1.euler_to_quat(np.radians(lafan1.bvh_from_raw(raw).eulers), raw.order)
    flips = np.sum(q[:-1] * q[1:], axis=-1) < 0
    walked = sorted(it.closure(e["parent"], list(sp) + list(sr)))
    assert flips[:, walked].any(axis=0).all()


@pytest.mark.parametrize("name", ["chain64_tip", "wide256"])
def test_long_clip_carries_bit_63_across_scan_blocks(lib, name):
    """600 frames, flips of every joint at the last and first rows of the 252-row scan blocks: the de-flip carry crosses two
    block boundaries with every bit of the mask in use (chain64_tip: bits 0 .. 63)"""
    e = it.BY_NAME[name]
    raw = _raw(e, 600, 17, 3, "zyx", (251, 252, 253, 503, 504, 505))
    _close(_one(_handle(lib, e, 3, "zyx"), raw), bvh_synth.host_packed_sel(raw, *e["bvh"]))


@pytest.mark.parametrize("name", ["binary63", "wide256"])
def test_ragged_call_into_a_padded_batch(lib, name):
    """9 clips of 0 .. 253 frames into a sentinel-filled padded batch with guard words: bit-identical to the single-clip calls,
    padding and guards untouched (the method of test_ragged_batch_into_padded_batch_and_ik_ignores_padding on other trees)"""
    e = it.BY_NAME[name]
    lens = [0, 1, 2, 63, 64, 65, 251, 252, 253]
    raws = [_raw(e, n, 40 + i, 6, "yzx", (n // 3, n // 3 + 1, n // 2)) for i, n in enumerate(lens)]
    h = _handle(lib, e, 6, "yzx")
    S, T, W = len(raws), 256, h.rows * 7
    rows = np.concatenate([r.rows for r in raws])
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    offsets = np.stack([r.offsets for r in raws])
    SENT, GUARD = -12345.678, 7.0e77
    host = np.full((S * T * W + 2 * 64,), GUARD)
    host[64:-64] = SENT
    d_h = lib.DeviceBuffer.from_host(host)
    d_rows, d_seg, d_off = lib.DeviceBuffer.from_host(rows), lib.DeviceBuffer.from_host(seg), lib.DeviceBuffer.from_host(offsets)
    st = lib.Stream()
    h.frames_dev(S, len(rows), d_rows, d_seg, d_off, T, C.c_void_p(d_h.ptr.value + 64 * 8), st)
    st.sync()
    back = d_h.to_host(host.shape, np.float64)
    assert np.all(back[:64] == GUARD) and np.all(back[-64:] == GUARD)
    human = back[64:-64].reshape(S, T, h.rows, 7)
    for i, r in enumerate(raws):
        n = lens[i]
        assert np.all(human[i, n:] == SENT)
        if n:
            assert np.array_equal(human[i, :n], _one(h, r))
            _close(human[i, :n], bvh_synth.host_packed_sel(r, *e["bvh"]))


def test_unrelated_position_and_orientation_joints(lib):
    """random (position, orientation) pairs, a joint used by four rows, the root as an orientation-only row"""
    e = it.BY_NAME["humanoid"]
    J = len(e["parent"])
    rng = np.random.default_rng(8)
    raw = _raw(e, 65, 3, 3, "zyx", (7, 64))
    for trial in range(4):
        n = int(rng.integers(3, 20))
        sp, sr = [int(x) for x in rng.integers(1, J, size=n)], [int(x) for x in rng.integers(1, J, size=n)]
        star = int(rng.integers(1, J))
        sp[:2] = [star, star]; sr[1:3] = [star, star]       # four uses of one joint
        sr[-1] = 0                                          # the root: an orientation only
        assert 0 not in sp
        _close(_one(_handle(lib, e, 3, "zyx", (sp, sr)), raw), bvh_synth.host_packed_sel(raw, sp, sr))


def test_refusals_are_error_returns_and_the_process_goes_on(lib):
    by = it.BY_NAME
    with pytest.raises(lib.GmrHipError, match="needs more than 64 joints"):
        _handle(lib, by["chain65_tip"], 3, "zyx")
    with pytest.raises(lib.GmrHipError, match="45 rows and 1 parked joints do not fit the LDS"):
        _handle(lib, by["star46_sel45"], 3, "zyx")
    with pytest.raises(lib.GmrHipError, match="1 <= nsel <= 64"):
        lib.BvhHandle(by["star64"]["parent"].tolist() + [0, 0], 3, "zyx", list(range(65)), list(range(65)))
    e = by["star45_sel44"]
    raw = _raw(e, 65, 2, 3, "zyx", (1, 64))
    _close(_one(_handle(lib, e, 3, "zyx"), raw), bvh_synth.host_packed_sel(raw, *e["bvh"]))
