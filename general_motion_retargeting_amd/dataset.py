"""Dataset harness: what the reference's ``process_file`` does after loading a clip
(``scripts/smplx_to_robot_dataset.py:78-146`` and ``scripts/bvh_to_robot_dataset.py:86-152``;
SURVEY.md H10), for MANY clips per launch.

Per clip: retarget every frame from ``qpos0`` (a fresh ``GeneralMotionRetargeting`` per file,
:79-87) -> split qpos, root quaternion wxyz -> xyzw (:97-102) -> ``local_body_pos`` = FK with
identity root (:106-112) -> optional height adjust ``root_z -= min_{t,b} z`` over the world FK
(:118-126) -> optional ``root_xy -= root_xy[0]`` (:128-131) -> the pkl dict (:134-141).
The SMPL-X script has both adjustments on, the BVH script both off (``bvh_to_robot_dataset.py:128``).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import os
import threading
import time
import weakref
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib, chunking
from .data_loader import motion_dict
from .kinematics_model import KinematicsModel
from .motion_retarget import GeneralMotionRetargeting


def postprocess_clip(qpos: np.ndarray, km: KinematicsModel, fps: float, height_adjust: bool = True,
                     root_origin_offset: bool = True, ground_offset: float = 0.0) -> Dict:
    """qpos f64[T, nq] of one clip -> motion dict (App. D)."""
    qpos = np.array(qpos, dtype=np.float64, copy=True)
    root_pos = qpos[:, :3].copy()
    root_rot = qpos[:, [4, 5, 6, 3]].copy()          # wxyz -> xyzw
    dof_pos = qpos[:, 7:].copy()
    T = qpos.shape[0]
    ident_pos = np.zeros((T, 3), dtype=np.float32)
    ident_rot = np.zeros((T, 4), dtype=np.float32)
    ident_rot[:, 3] = 1.0
    local_body_pos, _ = km.forward_kinematics(ident_pos, ident_rot, dof_pos.astype(np.float32))
    if height_adjust and T > 0:
        _, _, lowest = km.forward_kinematics(root_pos.astype(np.float32), root_rot.astype(np.float32),
                                             dof_pos.astype(np.float32), return_min_z=True)
        root_pos[:, 2] = root_pos[:, 2] - lowest + ground_offset
    if root_origin_offset and T > 0:
        root_pos[:, :2] -= root_pos[0, :2]
    return motion_dict(fps, root_pos, root_rot, dof_pos, np.asarray(local_body_pos), km.body_names)


def postprocess_clips(qpos_list: Sequence[np.ndarray], km: KinematicsModel, fps: Sequence[float], height_adjust: bool = True,
                      root_origin_offset: bool = True, ground_offset: float = 0.0) -> List[Dict]:
    """:func:`postprocess_clip` for MANY clips with two FK launches in total instead of one or two per clip: the frames
    of all clips are concatenated, ``local_body_pos`` comes from one launch with identity roots, the per-clip minimum of
    the world FK's z from one launch + a segmented reduction on the device (``gmr_fk_batch_segments``).  Same values."""
    lens = np.array([len(q) for q in qpos_list], dtype=np.int64)
    if len(lens) == 0:
        return []
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    B = int(seg[-1])
    allq = np.concatenate([np.asarray(q, dtype=np.float64).reshape(-1, km.num_dof + 7) for q in qpos_list]) if B else np.zeros((0, km.num_dof + 7))
    root_pos = allq[:, :3].copy()
    root_rot = allq[:, [4, 5, 6, 3]].copy()           # wxyz -> xyzw
    dof_pos = allq[:, 7:].copy()
    dof32 = dof_pos.astype(np.float32)
    ident = np.zeros((B, 4), dtype=np.float32)
    ident[:, 3] = 1.0
    fk = km.hip_handle
    local_body_pos = fk.fk_segments(np.zeros((B, 3), dtype=np.float32), ident, dof32, np.array([0, B]))[0] if B else \
        np.zeros((0, km.num_joint, 3), np.float32)
    if height_adjust and B:
        _, lowest = fk.fk_segments(root_pos.astype(np.float32), root_rot.astype(np.float32), dof32, seg, want_pos=False)
        root_pos[:, 2] = root_pos[:, 2] - np.repeat(lowest.astype(np.float64), lens) + ground_offset
    out = []
    for i in range(len(lens)):
        a, b = int(seg[i]), int(seg[i + 1])
        rp = root_pos[a:b].copy()
        if root_origin_offset and b > a:
            rp[:, :2] -= rp[0, :2]
        out.append(motion_dict(fps[i], rp, root_rot[a:b].copy(), dof_pos[a:b].copy(), local_body_pos[a:b].copy(), km.body_names))
    return out


# ----------------------------------------------------------------------------------------------
# The same post-processing ON THE DEVICE (``gmr_postprocess_clips_dev``): the IK launch's output never leaves the GPU, the
# five pkl arrays of the whole batch come back in one asynchronous copy into page-locked memory, and the motion dicts are
# VIEWS of that block.  ``GMR_DATASET_POST=host`` (or no GPU) keeps :func:`postprocess_clips`; the bytes are the same.
# ----------------------------------------------------------------------------------------------
def post_path() -> str:
    """``"device"`` or ``"host"``: which post-processing the drivers take (environment switch ``GMR_DATASET_POST``)."""
    if os.environ.get("GMR_DATASET_POST", "device").strip().lower() == "host":
        return "host"
    try:
        return "device" if _lib.lib().gmr_device_count() > 0 else "host"
    except Exception:  # noqa: BLE001 -- no library, no device: the host path says so itself
        return "host"


def bvh_path() -> str:
    """``"device"`` or ``"host"``: where the BVH drivers turn raw channel rows into packed frames.  ``"device"``
    (``gmr_bvh_frames_dev`` in front of the IK launch, the loaders only parse text) needs a GPU and the device post-processing
    (:func:`post_path`); ``GMR_DATASET_BVH=host`` keeps the NumPy functions of ``utils/lafan1.py`` in the loaders."""
    if os.environ.get("GMR_DATASET_BVH", "device").strip().lower() == "host":
        return "host"
    return post_path()


def smplx_path() -> str:
    """``"device"`` or ``"host"``: where the SMPL-X drivers compute the packed frames of a batch.  ``"device"`` (the raw arrays of
    all clips uploaded ragged, ONE ``gmr_smplx_batch_frames_dev`` call in front of the IK launch) needs a GPU and the device
    post-processing (:func:`post_path`); ``GMR_DATASET_SMPLX=host`` keeps one ``gmr_smplx_frames`` call per clip."""
    if os.environ.get("GMR_DATASET_SMPLX", "device").strip().lower() == "host":
        return "host"
    return post_path()


def heights_path() -> str:
    """``"merged"`` or ``"groups"``: how a batch of clips of several human heights reaches the IK kernels.  Merged (the default):
    ONE solver built from the unscaled config and ONE job, the heights travel as per-stream scale rows
    (``ik_config.scale_rows``).  ``GMR_DATASET_HEIGHTS=groups`` keeps one solver and one job per height, for A/B; the bytes
    are the same."""
    if os.environ.get("GMR_DATASET_HEIGHTS", "merged").strip().lower() == "groups":
        return "groups"
    return "merged"


class PinnedPool:
    """Page-locked output blocks for batches whose results are handed out as views.  A block is taken for one batch; it
    comes back when the LAST array viewing it has died (a finalizer on the buffer the arrays are views of), so a dict kept
    by the caller or waiting for a writer thread never aliases memory a later batch writes.  A new block is locked only
    when no free one is large enough.  ``alloc(nbytes)`` -> object with ``.ptr`` (``c_void_p``) and ``.nbytes``."""

    def __init__(self, alloc=None, keep: int = 8):
        self._alloc, self._keep = alloc, int(keep)
        self._free: List = []
        self._lock = threading.Lock()
        self.blocks_allocated = 0

    def take(self, nbytes: int):
        """a ``ctypes`` char buffer of at least ``nbytes`` bytes; ``np.frombuffer`` views of it keep the block out of the pool"""
        import ctypes as C
        need = max(int(nbytes), 8)
        with self._lock:
            fit = [o for o in self._free if o.nbytes >= need]
            owner = min(fit, key=lambda o: o.nbytes) if fit else None
            if owner is not None:
                self._free.remove(owner)
        if owner is None:
            if self._alloc is None:
                self._alloc = _lib._PinnedOwner
            owner = self._alloc(need + need // 4)
            self.blocks_allocated += 1
        buf = (C.c_char * owner.nbytes).from_address(owner.ptr.value)
        weakref.finalize(buf, self._give_back, owner).atexit = False      # (the finalizer holds the owner, not the buffer)
        return buf

    def _give_back(self, owner) -> None:
        with self._lock:
            if len(self._free) < self._keep:
                self._free.append(owner)            # (beyond `keep` free blocks the owner dies here and unlocks its pages)

    @property
    def free_blocks(self) -> int:
        with self._lock:
            return len(self._free)


@dataclasses.dataclass
class BlockPlan:
    """The output block of one :meth:`DevicePost.run` (:func:`plan_block`): which rows every clip gets, which post-processing
    calls write them, and where the five arrays lie in the block's bytes."""
    perms: List[Optional[np.ndarray]]     # per job: device position -> clip of the job (None: the job's own order)
    dlens: List[np.ndarray]               # per job: the clip lengths in device order
    spans: List[List[tuple]]              # per job: (first row, end row) of every clip, in device order
    calls: List[tuple]                    # per post-processing call: (first job, first row, seg_start i32[clips of the call + 1])
    rows: int
    nclip: int
    arrays: Dict[str, tuple]              # name -> (byte offset, bytes per row, dtype, shape)
    total: int

    def to_job_order(self, i: int, x):
        """``x`` (one entry per clip of job i, in device order) in the job's own clip order"""
        if self.perms[i] is None:
            return x
        inv = np.argsort(self.perms[i])
        return x[inv] if isinstance(x, np.ndarray) else [x[k] for k in inv.tolist()]

    def at(self, base: int, name: str, row: int = 0) -> C.c_void_p:
        """the address of ``row`` of array ``name`` in a block that starts at ``base``"""
        off, stride = self.arrays[name][:2]
        return C.c_void_p(base + off + row * stride)

    def views(self, buf):
        """``(root_pos, root_rot, dof_pos, local_body_pos, status)`` of a host copy of the block: four views and a copy"""
        v = [np.frombuffer(buf, dtype=dt, count=int(np.prod(shape)), offset=off).reshape(shape) for off, _, dt, shape in self.arrays.values()]
        return v[0], v[1], v[2], v[3], v[4].copy()


def plan_block(lens_per_job: Sequence, perms: Sequence, ndof: int, nb: int) -> BlockPlan:
    """The sources of one post-processing call are at most 8 jobs: more jobs -> more calls, each over its own dense range of
    rows that starts at a multiple of 4 (so that its ``local_body_pos`` starts 16-byte aligned).  ``perms[i]`` orders the clips
    of job i on the device (raw BVH jobs: the clips of one topology are consecutive streams), ``None`` leaves them."""
    dlens = [np.asarray(l, dtype=np.int64) if p is None else np.asarray(l, dtype=np.int64)[p] for l, p in zip(lens_per_job, perms)]
    calls, spans, row = [], [], 0
    for c0 in range(0, len(dlens), 8):
        seg = [0]
        for lens in dlens[c0:c0 + 8]:
            starts = row + seg[-1] + np.concatenate([[0], np.cumsum(lens)])
            spans.append([(int(a), int(b)) for a, b in zip(starts[:-1], starts[1:])])
            seg.extend((seg[-1] + np.cumsum(lens)).tolist())
        calls.append((c0, row, np.asarray(seg, dtype=np.int32)))
        row = (row + seg[-1] + 3) // 4 * 4
    rows, nclip = max(row, 1), sum(len(l) for l in dlens)
    arrays, total = {}, 0
    for name, dt, shape in (("root_pos", np.float64, (rows, 3)), ("root_rot", np.float64, (rows, 4)), ("dof_pos", np.float64, (rows, ndof)),
                            ("local_body_pos", np.float32, (rows, nb, 3)), ("status", np.int32, (nclip,))):
        stride = int(np.prod(shape[1:])) * np.dtype(dt).itemsize
        arrays[name] = (total, stride, dt, shape)
        total += _lib.align256(shape[0] * stride)
    return BlockPlan(list(perms), dlens, spans, calls, rows, nclip, arrays, total)


def _bvh_perm(job: Dict) -> Optional[np.ndarray]:
    """a raw BVH job's clips in the order they take on the device: topology by topology, then the packed ones"""
    if "bvh" not in job:
        return None
    perm = np.array([i for g in job["bvh"] for i in g["clips"]] + [i for i, _ in job.get("packed", ())], dtype=np.int64)
    assert sorted(perm.tolist()) == list(range(len(job["lens"])))
    return perm


class DevicePost:
    """IK and post-processing of one batch without a host round trip in between: page-locked ``human`` -> H2D -> one group
    launch -> ``gmr_postprocess_clips_dev`` over all jobs -> ONE D2H of the five arrays and the status words -> one stream
    synchronisation.  Device buffers and the input staging are grow-only and reused from batch to batch; output blocks come
    from a :class:`PinnedPool`."""

    def __init__(self, pool: Optional[PinnedPool] = None):
        self.pool = pool if pool is not None else PinnedPool()
        self._stream = None
        self._bufs = _lib.NamedBuffers()          # device blocks and input staging
        self._events = None
        self._chunker = None
        self.chunk_reports: List = []             # per job of the last run: per-clip chunk reports (chunking.clip_report), or None
        self.library = None                       # the motion library of the last run that asked for one (run(..., library=))

    def _d(self, name: str, nbytes: int):
        return self._bufs.device(name, nbytes)

    def pinned(self, name: str, shape, dtype) -> np.ndarray:
        return self._bufs.pinned(name, shape, dtype)

    def _stage_smplx(self, jobs: Sequence[Dict]):
        """The raw SMPL-X clips of all jobs that carry ``"smplx"``, per handle: one page-locked block (poses, translations, the
        two tables, flags, rest joints and the per-clip destination addresses inside the jobs' ``human_{i}`` device buffers)
        that goes up in ONE copy.  Returns ``({job index: human buffer}, H2D copies, frame calls)`` like the other two stages."""
        groups: Dict[int, tuple] = {}
        d_human: Dict[int, object] = {}
        for i, j in enumerate(jobs):
            if "smplx" not in j:
                continue
            sx, sol = j["smplx"], j["solver"]
            S, T = len(j["lens"]), max(int(j["T"]), 1)
            assert len(sx["clips"]) == S and sx["handle"].rows == sol.nhuman and sx["handle"].batch_takes
            d_human[i] = self._d(f"human_{i}", S * T * sol.nhuman * 56)
            groups.setdefault(id(sx["handle"]), (sx["handle"], []))[1].extend((i, k, T, e) for k, e in enumerate(sx["clips"]))
        copies, calls = [], []
        for gi, (h, members) in enumerate(groups.values()):
            n, frame_bytes = len(members), h.rows * 56
            B = sum(e["N"] for _, _, _, e in members)
            fields = (("ro", np.float32, (B, 3)), ("pb", np.float32, (B, 63)), ("tr", np.float32, (B, 3)), ("seg", np.int32, (n + 1,)),
                      ("nout", np.int32, (n,)), ("align", np.uint8, (n,)), ("jrest", np.float64, (n, h.J, 3)), ("tab", np.uint64, (n,)))
            offs, total = {}, 0
            for k, dt, shape in fields:
                offs[k] = total
                total += _lib.align256(int(np.prod(shape)) * np.dtype(dt).itemsize)
            stage = self.pinned(f"smplx_in_{gi}", (total,), np.uint8)
            v = {k: stage[offs[k]: offs[k] + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape) for k, dt, shape in fields}
            a = 0
            v["seg"][0] = 0
            for m, (i, k, T, e) in enumerate(members):
                N = e["N"]
                assert 0 <= e["nout"] <= min(N, T) and int(jobs[i]["lens"][k]) == e["nout"] and (e["align"] or e["nout"] == N)
                v["ro"][a:a + N] = e["root_orient"]
                v["pb"][a:a + N] = e["pose_body"]
                v["tr"][a:a + N] = e["trans"]
                a += N
                v["seg"][m + 1] = a
                v["nout"][m], v["align"][m], v["jrest"][m] = e["nout"], e["align"], e["j_rest"]
                v["tab"][m] = d_human[i].ptr.value + k * T * frame_bytes
            d_in = self._d(f"smplx_in_{gi}", total)
            copies.append((d_in.ptr, stage))
            calls.append(functools.partial(h.batch_frames_dev, n, B, *(C.c_void_p(d_in.ptr.value + offs[k]) for k, _, _ in fields)))
        return d_human, copies, calls

    def run(self, jobs: Sequence[Dict], km: KinematicsModel, ik_flags: int = 0, height_adjust: bool = True,
            root_origin_offset: bool = True, ground_offset: float = 0.0, timing: Optional[Dict[str, float]] = None, chunk=None,
            library: Optional[Dict] = None):
        """``library`` (``None`` | ``{"fps": [per job: fps per clip], "ang_vel": "world" | "reference"}``): also fill a
        ``motion_library.MotionLibrary`` from the post-processed block where it lies on the device (no second upload), on this
        object's stream and before the block is reused; it is left in ``self.library``.  What is returned does not change.
        ``chunk`` (``None`` | ``chunking.ChunkSpec`` | ``"auto"``): jobs with a clip longer than the spec's ``frames`` run chunked
        (:class:`chunking.ChunkRunner` in place of the one IK launch: NOT parity, ``chunk_reports`` says how far off); the
        post-processing reads the stitched clip-major output unchanged.
        ``jobs`` = ``[{"solver", "human": f64[S,T,nhuman,7] (page-locked for an asynchronous copy), "lens": i32[S],
        "q0": f64[nq], optional "scales": f64[S,nhuman] (a human scale table per clip in place of the solver's; not with a
        chunk spec that takes effect: the slots of a chunk job are not streams), optional "weights": f64[S,T,nhuman] (per-frame
        body weights, 0 = the body is missing in that frame; not with a chunk spec that takes effect either)}]``, all for the robot of ``km``.  A job of raw BVH clips carries, instead of ``"human"``, ``"T"`` and
        ``"bvh"`` = ``[{"handle": _lib.BvhHandle, "rows": f64[B,ncol] (page-locked), "offsets": f64[n,J,3], "clips": [index in
        lens, ...], "lens": [...]}]`` (one entry per topology) and optionally ``"packed"`` = ``[(index, f64[n,nhuman,7])]``: the
        raw rows are uploaded ragged and ``gmr_bvh_frames_dev`` writes ``human`` on the device, on the same stream, in front
        of the IK launch (inside the batch the clips are ordered by topology; the results come back in the job's order).  A job
        of raw SMPL-X clips carries ``"T"`` and ``"smplx"`` = ``{"handle": _lib.SmplxHandle, "clips": [utils.smpl.smplx_raw_clip
        entry per clip of lens]}``: the arrays of ALL such jobs go up as one ragged block and one ``gmr_smplx_batch_frames_dev``
        call per handle writes every job's ``human`` through a table of per-clip addresses.  Returns ``(root_pos, root_rot, dof_pos, local_body_pos, spans, status)``:
        the four arrays are views of one pool block, ``spans[j][k] = (a, b)`` are the rows of clip k of job j, ``status[j]``
        the IK status words of job j."""
        if self._stream is None:
            self._stream = _lib.Stream()
            self._events = [_lib.Event() for _ in range(6)]
        st, ev = self._stream, self._events
        fk = km.hip_handle
        block = plan_block([j["lens"] for j in jobs], [_bvh_perm(j) for j in jobs], fk.ndof, fk.nbody)
        d_out = self._d("out", block.total)
        base = d_out.ptr.value
        sx_human, sx_copies, sx_calls = self._stage_smplx(jobs)
        ev[0].record(st)
        launch, bvh_calls, clip, d_weights = [], [], 0, []
        for i, j in enumerate(jobs):
            if "bvh" in j:
                d_h, copies, calls = self._stage_bvh(i, j, block.dlens[i])
            elif "smplx" in j:
                d_h, copies, calls = sx_human[i], [], []          # (frames at or beyond a clip's nout stay stale: never read)
            else:
                d_h, copies, calls = self._stage_packed(i, j)
            job, more, d_w = self._stage_job(i, j, d_h, block, block.at(base, "status", clip))
            for dst, src in copies + more:
                self._h2d(dst, src)
            launch.append(job)
            d_weights.append(d_w)
            bvh_calls += calls
            clip += job.S
        for dst, src in sx_copies:
            self._h2d(dst, src)
        ev[1].record(st)
        for call in bvh_calls + sx_calls:
            call(st)
        ev[5].record(st)
        self.chunk_reports = self._ik(launch, block, chunk, ik_flags, d_weights)
        ev[2].record(st)
        self._post(block, base, launch, fk, height_adjust, root_origin_offset, ground_offset)
        ev[3].record(st)
        self.library = self._library(block, base, km, library)
        buf = self._read_back(block, d_out)
        ev[4].record(st)
        st.sync()
        if timing is not None:
            for k, a, b in (("h2d", 0, 1), ("frames", 1, 5), ("ik", 5, 2), ("post", 2, 3), ("d2h", 3, 4)):
                if k != "frames" or bvh_calls or sx_calls:
                    timing[k] = timing.get(k, 0.0) + ev[a].elapsed_ms(ev[b]) * 1e-3
        rp, rr, dp, lbp, status = block.views(buf)
        first = np.cumsum([0] + [len(l) for l in block.dlens])
        return (rp, rr, dp, lbp, [block.to_job_order(i, sp) for i, sp in enumerate(block.spans)],
                [block.to_job_order(i, status[a:b]) for i, (a, b) in enumerate(zip(first[:-1], first[1:]))])

    def _h2d(self, dst, src: np.ndarray) -> None:
        _lib.check(_lib.lib().gmr_memcpy_h2d(dst, src.ctypes.data_as(C.c_void_p), src.nbytes, self._stream.ptr))

    def _stage_packed(self, i: int, j: Dict):
        """job i with its frames packed on the host: one copy of the padded batch"""
        human, sol = j["human"], j["solver"]
        assert human.dtype == np.float64 and human.flags.c_contiguous and human.shape[2:] == (sol.nhuman, 7)
        d_h = self._d(f"human_{i}", human.nbytes)
        return d_h, [(d_h.ptr, human)], []

    def _stage_bvh(self, i: int, j: Dict, dlens: np.ndarray):
        """job i of raw BVH clips: per topology the ragged rows, their segment starts and joint offsets go up and one
        ``gmr_bvh_frames_dev`` call writes the clips' padded frames; clips packed on the host go straight into theirs"""
        sol, S, T, copies, calls = j["solver"], len(dlens), max(int(j["T"]), 1), [], []
        frame_bytes = sol.nhuman * 7 * 8
        d_h = self._d(f"human_{i}", S * T * frame_bytes)       # (rows at or beyond a clip's length stay stale: never read)
        pos = 0
        for gi, g in enumerate(j["bvh"]):
            rows, n = g["rows"], len(g["clips"])
            assert rows.dtype == np.float64 and rows.flags.c_contiguous and rows.shape[1] == g["handle"].ncol
            seg = self.pinned(f"bvhseg_{i}_{gi}", (n + 1,), np.int32)
            seg[0] = 0
            seg[1:] = np.cumsum(g["lens"])
            assert int(seg[-1]) == rows.shape[0] and len(g["lens"]) == n
            off = self.pinned(f"bvhoff_{i}_{gi}", (n, g["handle"].J, 3), np.float64)
            off[:] = g["offsets"]
            d_rows, d_seg, d_off = (self._d(f"bvh{k}_{i}_{gi}", a.nbytes) for k, a in (("rows", rows), ("seg", seg), ("off", off)))
            copies += [(d_rows.ptr, rows), (d_seg.ptr, seg), (d_off.ptr, off)]
            calls.append(functools.partial(g["handle"].frames_dev, n, rows.shape[0], d_rows, d_seg, d_off, T,
                                           C.c_void_p(d_h.ptr.value + pos * T * frame_bytes)))
            pos += n
        packed = j.get("packed", ())
        if packed:      # clips the device path does not take, computed on the host
            stage = self.pinned(f"bvhpacked_{i}", (sum(len(p) for _, p in packed), sol.nhuman, 7), np.float64)
            a = 0
            for _, p in packed:
                stage[a:a + len(p)] = p
                if len(p):
                    copies.append((C.c_void_p(d_h.ptr.value + pos * T * frame_bytes), stage[a:a + len(p)]))
                a += len(p)
                pos += 1
        return d_h, copies, calls

    def _stage_job(self, i: int, j: Dict, d_h, block: BlockPlan, d_status):
        """what every kind of job needs besides its frames: start poses, clip lengths (device order), the IK outputs and the
        scale rows and body weights it may carry.  Returns ``(DevJob, H2D copies, the weights on the device or None)``."""
        sol, dlens = j["solver"], block.dlens[i]
        S, T = j["human"].shape[:2] if "human" in j else (len(dlens), max(int(j["T"]), 1))
        q0 = self.pinned(f"q0_{i}", (S, sol.nq), np.float64)
        q0[:] = j["q0"]
        lens = self.pinned(f"len_{i}", (S,), np.int32)
        lens[:] = dlens
        d_q0, d_len = self._d(f"q0_{i}", q0.nbytes), self._d(f"len_{i}", lens.nbytes)
        d_q, d_ns = self._d(f"q_out_{i}", S * T * sol.nq * 8), self._d(f"nsolve_{i}", S * T * 8)
        copies, d_sc = [], None
        if j.get("scales") is not None:
            rows = _lib.check_scales(j["scales"], S, sol.nhuman, f"job {i}: scales")
            sc = self.pinned(f"scale_{i}", (S, sol.nhuman), np.float64)
            sc[:] = rows if block.perms[i] is None else rows[block.perms[i]]
            d_sc = self._d(f"scale_{i}", sc.nbytes)
            copies.append((d_sc.ptr, sc))
        d_w = None
        if j.get("weights") is not None:
            rows = _lib.check_weights(j["weights"], S, T, sol.nhuman, f"job {i}: weights", j["lens"])
            w = self.pinned(f"weight_{i}", (S, T, sol.nhuman), np.float64)
            w[:] = rows if block.perms[i] is None else rows[block.perms[i]]
            d_w = self._d(f"weight_{i}", w.nbytes)
            copies.append((d_w.ptr, w))
        return _lib.DevJob(sol, S, T, d_q0, d_h, d_len, d_q, d_ns, d_status, d_sc), copies + [(d_q0.ptr, q0), (d_len.ptr, lens)], d_w

    def _ik(self, launch: List, block: BlockPlan, chunk, ik_flags: int, d_weights: Optional[List] = None) -> List:
        """the IK launch of all jobs (``d_weights``: per job its body weights on the device, or None), chunked where the spec
        takes effect; returns the chunk reports per job, in job order"""
        total_frames = int(sum(int(l.sum()) for l in block.dlens))
        specs = [chunking.resolve_any(chunk, l, total_frames) for l in block.dlens]
        weighted = d_weights is not None and any(w is not None for w in d_weights)
        if all(sp is None for sp in specs):
            _lib.retarget_group_dev(launch, ik_flags, self._stream, weights=d_weights if weighted else None)
            return [None] * len(launch)
        if weighted:
            raise ValueError(chunking.BODY_WEIGHTS_REFUSAL)
        if any(job.scale is not None for job in launch):
            raise ValueError("per-clip scales do not go with a chunk spec that takes effect: run the heights as groups")
        if self._chunker is None:
            self._chunker = chunking.ChunkRunner()
        reports = self._chunker.run(launch, block.dlens, specs, ik_flags, self._stream)
        return [r if r is None else block.to_job_order(i, r) for i, r in enumerate(reports)]

    def _post(self, block: BlockPlan, base: int, launch: List, fk, height_adjust: bool, root_origin_offset: bool, ground_offset: float):
        sources = [(job.S, job.T, job.q_out, job.len) for job in launch]
        for n, (c0, r0, seg) in enumerate(block.calls):
            hseg = self.pinned(f"seg_{n}", seg.shape, np.int32)
            hseg[:] = seg
            d_seg = self._d(f"seg_{n}", seg.nbytes)
            self._h2d(d_seg.ptr, hseg)
            fk.postprocess_clips_dev(sources[c0:c0 + 8], d_seg, len(seg) - 1, int(seg[-1]), block.at(base, "root_pos", r0),
                                     block.at(base, "root_rot", r0), block.at(base, "dof_pos", r0), block.at(base, "local_body_pos", r0),
                                     None, height_adjust, root_origin_offset, ground_offset, self._stream)

    def _library(self, block: BlockPlan, base: int, km: KinematicsModel, library: Optional[Dict]):
        if library is None:
            return None
        # the block is clip-contiguous from row 0 when one post-processing call covered it, in the jobs' own clip order
        if len(block.calls) != 1 or any(p is not None and not np.array_equal(p, np.arange(len(p))) for p in block.perms):
            raise ValueError("a motion library takes the clips of at most 8 jobs in the order they were handed over")
        from .motion_library import MotionLibrary
        fk = km.hip_handle
        lib_ = MotionLibrary.from_device(
            block.calls[0][2], np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1) for f in library["fps"]]), fk.ndof, fk.nbody,
            block.at(base, "root_pos"), block.at(base, "root_rot"), block.at(base, "dof_pos"), block.at(base, "local_body_pos"),
            ang_vel=library.get("ang_vel", "world"), stream=self._stream, link_body_lists=[km.body_names] * block.nclip)
        lib_._kinematics = km         # the robot of these clips: body_state() needs no kinematics argument
        return lib_

    def _read_back(self, block: BlockPlan, d_out):
        """the whole block into a pool block, asynchronously; returns the buffer the views are taken of"""
        buf = self.pool.take(block.total)
        # (the address, not ctypes.cast: a cast leaves the buffer referring to itself, and only the cycle collector would
        #  hand the block back)
        _lib.check(_lib.lib().gmr_memcpy_d2h(C.c_void_p(C.addressof(buf)), d_out.ptr, block.total, self._stream.ptr))
        return buf


def _run_batch(jobs: Sequence[Dict], km: KinematicsModel, ik_flags: int, height_adjust: bool, root_origin_offset: bool, chunk,
               library: Optional[str], timing: Optional[Dict[str, float]], post: Optional[DevicePost], outs=None):
    """The tail of every driver: IK, status check, post-processing, motion dicts, motion library.  ``jobs`` as
    :meth:`DevicePost.run` takes them, each with ``"idxs"`` (its clips' indices in the caller's order) and ``"fps"`` (per
    clip); with a ``post`` everything runs on the device, without one through ``_lib.retarget_group`` (or the chunked host
    entry) and :func:`postprocess_clips` (``"human"`` jobs only; ``outs()`` -> the page-locked outputs of the plain launch).
    ``library``: ``None`` | ``"world"`` | ``"reference"``.  Returns ``(motions in the caller's order, library, chunk reports per job)``."""
    from .motion_library import MotionLibrary
    t0 = time.perf_counter()
    fps = {i: f for j in jobs for i, f in zip(j["idxs"], j["fps"])}
    out: List[Optional[Dict]] = [None] * len(fps)

    def check(j, status):
        if (status != 0).any():
            raise RuntimeError(f"IK failed for clips {[j['idxs'][k] for k in np.nonzero(status)[0]]}")

    def add(key: str, seconds: float):
        if timing is not None:
            timing[key] = timing.get(key, 0.0) + seconds

    if post is not None:
        rp, rr, dp, lbp, spans, status = post.run(jobs, km, ik_flags, height_adjust, root_origin_offset, 0.0, timing, chunk=chunk,
                                                  library=None if library is None else
                                                  {"fps": [list(j["fps"]) for j in jobs], "ang_vel": library})
        t1 = time.perf_counter()
        for j, sp, stt in zip(jobs, spans, status):
            check(j, stt)
            for i, (a, b) in zip(j["idxs"], sp):
                out[i] = motion_dict(fps[i], rp[a:b], rr[a:b], dp[a:b], lbp[a:b], km.body_names)
        add("dicts", time.perf_counter() - t1)
        return out, post.library, post.chunk_reports
    total_frames = int(sum(int(np.sum(j["lens"])) for j in jobs))
    specs = [chunking.resolve_any(chunk, j["lens"], total_frames) for j in jobs]
    results, reports = [None] * len(jobs), [None] * len(jobs)
    plain = [n for n, sp in enumerate(specs) if sp is None]
    if plain:
        group = [{**jobs[n], "q0": np.broadcast_to(jobs[n]["q0"], (len(jobs[n]["lens"]), jobs[n]["solver"].nq))} for n in plain]
        for n, r in zip(plain, _lib.retarget_group(group, ik_flags, 0, outs=outs() if outs is not None and len(plain) == len(jobs) else None)):
            results[n] = r
    for n, (j, sp) in enumerate(zip(jobs, specs)):
        if sp is not None:
            assert j.get("scales") is None          # (the slots of a chunk job are not streams)
            if j.get("weights") is not None:
                raise ValueError(chunking.BODY_WEIGHTS_REFUSAL)
            *results[n], reports[n] = chunking.retarget_chunked_host(j["solver"], j["human"], j["q0"], j["lens"], ik_flags, sp)
    t1 = time.perf_counter()
    qpos: List[Optional[np.ndarray]] = [None] * len(out)
    for j, (q, _, status) in zip(jobs, results):
        check(j, status)
        for k, i in enumerate(j["idxs"]):
            qpos[i] = q[k, : j["lens"][k]]
    out = postprocess_clips(qpos, km, [fps[i] for i in range(len(out))], height_adjust, root_origin_offset)
    add("ik", t1 - t0)
    add("post", time.perf_counter() - t1)
    lib_ = None
    if library is not None:      # (host post-processing: the arrays are on the host, so they go up once)
        lib_ = MotionLibrary.from_motions(out, library)
        lib_._kinematics = km
    return out, lib_, reports


class ClipRetargeter:
    """Many clips of one (source, robot, height) per call, ONE IK launch each: the per-batch step of the dataset drivers.
    What does not depend on the batch is built once -- the solver, the ``KinematicsModel`` -- and the padded input /
    output arrays live in page-locked memory that is reused from batch to batch (locking pages costs more than
    retargeting them), so the copies of a large batch run asynchronously, slice by slice, under its kernels."""

    _seen_raw = False            # this object has staged raw BVH clips: its batches are raw batches from then on
    _raw_index: Optional[Dict[tuple, int]] = None        # topology key -> number of its page-locked rows block
    chunk = None                 # chunked retargeting of long clips: off
    chunk_report: Optional[List[Dict]] = None
    _library_mode: Optional[str] = None       # hand the batch to a motion library: off
    library = None
    _per_clip = False            # one height per clip, travelling as scale rows: off
    _heights: Optional[np.ndarray] = None
    _frame_limit = None          # velocity limits between frames: off

    def __init__(self, src_human: str, tgt_robot: str, actual_human_height=None, height_adjust: bool = True,
                 root_origin_offset: bool = True, offset_to_ground: bool = False, chunk=None, library=False,
                 velocity_limit=None, frame_velocity_limit=None):
        """``velocity_limit`` (default None: off): per-joint velocity limits of every solve, a scalar in rad/s, an array
        ``[nhinge]`` or a dict ``{joint name: rad/s}`` (``GeneralMotionRetargeting.set_velocity_limit``: a bound per solve, not
        on the velocity between frames).
        ``frame_velocity_limit`` (default None: off): per-joint velocity limits BETWEEN FRAMES, in the same three forms
        (``GeneralMotionRetargeting.set_frame_velocity_limit``); the frames are ``1 / fps`` apart, the fps of the batch, so a
        batch whose clips disagree on fps raises ``ValueError`` while it is on; every clip starts free (from ``qpos0``).  It
        does not go with ``chunk`` (``ValueError``).
        ``actual_human_height``: one height for every clip (a number or None: the solver is built for it, as ever), or a
        sequence with one height per clip of a call (``add(clip, height=)`` in the staged protocol): the solver is built from
        the unscaled config and every clip carries its height as a scale row of the ONE job, the bits of a retargeter built
        for that height.  Per-clip heights do not go with a ``chunk`` spec that takes effect (the slots of a chunk job are
        not streams; :func:`retarget_clips` then runs the heights as groups).
        ``library`` (``False`` | ``True`` | ``"world"`` | ``"reference"``): every batch also leaves a
        ``motion_library.MotionLibrary`` of its clips in ``self.library`` -- on the device post-processing path filled from the
        block the post-processing wrote, without a second upload (``True`` = ``"world"``).  The motion dicts do not change.
        ``chunk``: ``None`` (default: one stream per clip, as ever), a ``chunking.ChunkSpec`` or ``"auto"``: clips longer than the
        spec's ``frames`` are cut into chunks that run as independent streams (NOT parity with the sequential run; DESIGN.md
        section 6g).  ``chunk_report`` then holds, per clip of the last batch, K, ``seam_max``, seams repaired / left bad, passes
        and ``warm_solves``; ``chunk_summary`` the totals over all batches."""
        self._per_clip = actual_human_height is not None and np.ndim(actual_human_height) > 0
        self._heights = np.asarray(actual_human_height, dtype=np.float64).reshape(-1) if self._per_clip else None
        self.gmr = GeneralMotionRetargeting(src_human, tgt_robot, actual_human_height=None if self._per_clip else actual_human_height,
                                            velocity_limit=velocity_limit)
        self._frame_limit = frame_velocity_limit
        _refuse_chunk_under_frame_limit(self.gmr, frame_velocity_limit, chunk)      # (and the limit is parsed once, here)
        self.height_adjust, self.root_origin_offset, self.offset_to_ground = height_adjust, root_origin_offset, offset_to_ground
        self.chunk = chunk
        self._library_mode = None if not library else ("world" if library is True else str(library))
        self.library = None
        self.chunk_report: Optional[List[Dict]] = None
        self.chunk_summary: Dict = {}
        self._km: Optional[KinematicsModel] = None
        self._pin = _lib.NamedBuffers()
        self._dev_post: Optional[DevicePost] = None
        self.timing: Dict[str, float] = {}

    def _buf(self, name: str, shape, dtype) -> np.ndarray:
        """a [shape] view of this object's page-locked block ``name`` (grown by half when too small)"""
        return self._pin.pinned(name, shape, dtype)

    # ---- staged protocol (DatasetPipeline): clips are copied into the padded, page-locked batch AS THEY ARRIVE from the
    # loaders -- the time this thread would otherwise spend waiting for them -- instead of when the batch is launched
    def reserve(self, frames_budget: int, row_doubles: int = 0) -> None:
        """Lock the pages of a batch of ``frames_budget`` padded frames now (e.g. while the loaders are starting up);
        ``row_doubles`` > 0: of ``frames_budget`` raw BVH rows of that many columns instead (the device path of :meth:`add`)."""
        sol = self.gmr.hip_solver
        if row_doubles > 0:
            self._buf("rows_0", (frames_budget, row_doubles), np.float64)
        else:
            self._buf("human", (frames_budget, sol.nhuman, 7), np.float64)
            self._buf("q_out", (frames_budget, sol.nq), np.float64)
            self._buf("nsolve", (frames_budget, 2), np.int32)
        if self._km is None:
            self._km = KinematicsModel(self.gmr.xml_file)
            self._km.hip_handle

    def begin(self, longest: int, max_clips: int, frames_budget: int) -> None:
        """A batch whose longest clip has ``longest`` frames (the drivers hand the clips over largest first)."""
        sol = self.gmr.hip_solver
        self._T = max(int(longest), 1)
        self._cap = max(1, min(int(max_clips), int(frames_budget) // self._T))
        self._human = None                                # the padded batch: locked when the first packed clip arrives
        self._lens = np.zeros(self._cap, dtype=np.int32)
        self._hts = np.full(self._cap, np.nan)            # per-clip heights (NaN = none: the unscaled table)
        self._wts = None                                  # per-frame body weights of the batch: locked when the first clip that has some arrives
        self._n = 0
        # a batch of raw BVH clips (device path): per topology the rows of its clips, concatenated in page-locked memory
        self._raw_mode = self._seen_raw
        self._bvh_device = bvh_path() == "device"         # (asked once per batch, not per clip)
        self._raw: Dict[tuple, Dict] = {}
        self._packed: List = []

    def _add_raw(self, clip) -> bool:
        """one raw BVH clip of a device-path batch: only its rows are copied"""
        from .utils import lafan1
        n = len(clip)
        if self._n >= self._cap or n > self._T:
            return False
        key = lafan1.topology_key(clip)
        if self._raw_index is None:
            self._raw_index = {}
        g = self._raw.get(key)
        if g is None:
            handle = lafan1.BVH_FRAMES.handle(clip, self.gmr.human_body_names)
            g = self._raw[key] = {"handle": handle, "index": self._raw_index.setdefault(key, len(self._raw_index)), "buf": None,
                                  "cap": 0, "used": 0, "clips": [], "lens": [], "offsets": []}
        if g["used"] + n > g["cap"]:
            # the first topology gets what the padded batch would have taken (cap x T rows); others grow as they fill
            cap = max(g["used"] + n, 2 * g["cap"], self._cap * self._T if g["index"] == 0 and self._cap * self._T < (1 << 40) else 0)
            keep = g["buf"][: g["used"]].copy() if g["used"] else None
            g["buf"], g["cap"] = self._buf(f"rows_{g['index']}", (cap, g["handle"].ncol), np.float64), cap
            if keep is not None:
                g["buf"][: g["used"]] = keep
        g["buf"][g["used"]: g["used"] + n] = clip.rows
        g["used"] += n
        g["clips"].append(self._n)
        g["lens"].append(n)
        g["offsets"].append(np.asarray(clip.offsets, dtype=np.float64))
        self._lens[self._n] = n
        self._n += 1
        self._raw_mode = self._seen_raw = True
        return True

    def add(self, clip, height: Optional[float] = None, body_weights=None) -> bool:
        """Copy one clip into the batch; False when it does not fit (batch full, or the clip is longer than the batch's
        rows): the caller finishes this batch and begins another.  ``height``: this clip's ``actual_human_height`` (only a
        retargeter built with per-clip heights takes one).  ``body_weights`` (``[T_i, nhuman]`` or one dict ``{body: m}`` per
        frame): this clip's per-frame body weights, packed into the batch beside its frames (clips without: ones); 0 = the body
        is missing in that frame.  Not for raw BVH clips (the device-side reader produces no dropouts) and not with ``chunk``.  A raw BVH clip (``lafan1.BvhRaw``) joins a batch whose
        frames are computed on the device (:func:`bvh_path`): only its rows are copied.  On the host path, for a file the
        device path does not take, or in a batch that already holds packed clips, its frames are computed here."""
        from .utils import lafan1
        t0 = time.perf_counter()
        if height is not None:
            if not self._per_clip:
                raise ValueError("this retargeter was built for one height: build it with a sequence of heights")
            if self._n < self._cap:
                self._hts[self._n] = height               # (kept only if the clip is: a refused clip leaves _n where it is)
        w = None
        if body_weights is not None:
            if self.chunk is not None:
                raise ValueError(chunking.BODY_WEIGHTS_REFUSAL)
            if isinstance(clip, lafan1.BvhRaw) or self._raw_mode:
                raise ValueError("body weights go with packed clips, not with raw BVH clips")
            w = self.gmr.clip_body_weights(body_weights, len(clip))
        if isinstance(clip, lafan1.BvhRaw):
            if self._bvh_device and lafan1.device_takes(clip) and (self._raw_mode or self._n == 0):
                ok = self._add_raw(clip)
                self.timing["pack"] = self.timing.get("pack", 0.0) + time.perf_counter() - t0
                return ok
            clip = lafan1.packed_from_raw(clip, self.gmr.human_body_names)
        p = clip if isinstance(clip, np.ndarray) else self.gmr.pack_frames(clip, w)
        if self._n >= self._cap or p.shape[0] > self._T:
            return False
        if w is not None:
            if self._wts is None:
                self._wts = self._buf("weights", (self._cap, self._T, self.gmr.hip_solver.nhuman), np.float64)
                self._wts[:] = 1.0
            self._wts[self._n, : w.shape[0]] = w
        if self._raw_mode and self._bvh_device:
            self._packed.append((self._n, np.asarray(p, dtype=np.float64)))      # uploaded into its padded rows by DevicePost
        else:
            self._raw_mode = False
            if self._human is None:
                self._human = self._buf("human", (self._cap, self._T, self.gmr.hip_solver.nhuman, 7), np.float64)
            self._human[self._n, : p.shape[0]] = p      # (rows beyond a clip's length are never read by the kernel)
        self._lens[self._n] = p.shape[0]
        self._n += 1
        self.timing["pack"] = self.timing.get("pack", 0.0) + time.perf_counter() - t0
        return True

    def _scales(self, S: int):
        """the scale rows of the batch's clips (None for a retargeter of one height)"""
        if not self._per_clip:
            return None
        from .ik_config import scale_rows
        return scale_rows(self.gmr._ik_config, self._hts[:S])

    def finish(self, fps: Sequence[float]) -> List[Dict]:
        S = self._n
        if S == 0:
            return []
        lens = self._lens[:S].copy()
        if self._per_clip and chunking.resolve_any(self.chunk, lens) is not None:
            raise ValueError("per-clip heights do not go with a chunk spec that takes effect: run the heights as groups")
        if self._frame_limit is not None:           # (this object's own retargeter: without a limit it never had one)
            _set_batch_frame_limit([self.gmr], self._frame_limit, list(fps)[:S])
        return self._finish_device(fps, lens) if post_path() == "device" else self._finish(fps, lens, None)

    def _finish_device(self, fps: Sequence[float], lens: np.ndarray) -> List[Dict]:
        """:meth:`finish` with the post-processing on the device: ``q_out`` and ``nsolve`` never cross the bus.  ``timing`` gets
        ``h2d`` / ``ik`` / ``post`` / ``d2h`` from device events of the one stream everything runs on (none of them overlaps
        another) and ``dicts``, the host time to wrap the views."""
        if self._dev_post is None:
            self._dev_post = DevicePost()
        return self._finish(fps, lens, self._dev_post)

    def _finish(self, fps: Sequence[float], lens: np.ndarray, post: Optional[DevicePost]) -> List[Dict]:
        """the batch as ONE job of :func:`_run_batch`, on the device with a ``post``"""
        S, T, gmr = self._n, self._T, self.gmr
        sol = gmr.hip_solver
        if self._km is None:
            self._km = KinematicsModel(gmr.xml_file)
        job = {"solver": sol, "lens": lens, "q0": gmr.model.qpos0, "scales": self._scales(S), "idxs": list(range(S)), "fps": list(fps)[:S]}
        if self._raw_mode:
            job.update(T=T, packed=self._packed,
                       bvh=[{"handle": g["handle"], "rows": g["buf"][: g["used"]], "offsets": np.stack(g["offsets"]), "clips": g["clips"],
                             "lens": g["lens"]} for g in self._raw.values()])
        else:
            job["human"] = self._human[:S]
        if self._wts is not None:
            job["weights"] = self._wts[:S]
        outs = None
        if post is None:        # the start poses and the outputs of the plain launch stay in this object's page-locked memory
            job["q0"] = self._buf("q0", (S, sol.nq), np.float64)
            job["q0"][:] = gmr.model.qpos0
            outs = lambda: [(self._buf("q_out", (S, T, sol.nq), np.float64), self._buf("nsolve", (S, T, 2), np.int32), np.zeros(S, np.int32))]   # noqa: E731
        self._n = 0
        out, self.library, (self.chunk_report,) = _run_batch([job], self._km, gmr._flags(self.offset_to_ground), self.height_adjust,
                                                             self.root_origin_offset, self.chunk, self._library_mode, self.timing, post, outs)
        if self.chunk_report is not None:
            chunking.summarize(self.chunk_report, self.chunk_summary)
        return out

    def __call__(self, clips: Sequence, fps: Sequence[float], body_weights: Optional[Sequence] = None) -> List[Dict]:
        """``body_weights``: None, or one entry per clip, each None or that clip's ``[T_i, nhuman]`` (see :meth:`add`)."""
        from .utils.lafan1 import BvhRaw
        if body_weights is not None and len(body_weights) != len(clips):
            raise ValueError(f"{len(body_weights)} body_weights for {len(clips)} clips")
        if body_weights is not None and self.chunk is not None and any(w is not None for w in body_weights):
            raise ValueError(chunking.BODY_WEIGHTS_REFUSAL)
        bw = [None] * len(clips) if body_weights is None else [None if w is None else self.gmr.clip_body_weights(w, len(c))
                                                               for w, c in zip(body_weights, clips)]
        packed = [c if isinstance(c, (np.ndarray, BvhRaw)) else self.gmr.pack_frames(c, w) for c, w in zip(clips, bw)]
        if not packed:
            return []
        if self._per_clip and len(self._heights) != len(packed):
            raise ValueError(f"{len(self._heights)} heights for {len(packed)} clips")
        self.begin(max(len(p) for p in packed), len(packed), 1 << 62)
        for k, p in enumerate(packed):
            assert self.add(p, float(self._heights[k]) if self._per_clip else None, bw[k])
        return self.finish(fps)


def _refuse_chunk_under_frame_limit(gmr: GeneralMotionRetargeting, frame_velocity_limit, chunk) -> None:
    """``chunk=`` and a finite frame velocity limit do not go together (chunking.FRAME_LIMIT_REFUSAL); parses the limit."""
    table, _ = gmr._frame_limit_table(frame_velocity_limit, 1.0)
    if chunk is not None and table is not None and np.isfinite(table).any():
        raise ValueError(chunking.FRAME_LIMIT_REFUSAL)


def _set_batch_frame_limit(gmrs, frame_velocity_limit, fps) -> None:
    """The frame velocity limit of one batch on the retargeters that serve it (None: cleared -- a kept retargeter serves every
    batch).  One ``frame_dt = 1 / fps`` per solver, so the clips of a batch under a limit must agree on their fps."""
    f = None
    if frame_velocity_limit is not None:
        distinct = sorted({float(x) for x in fps})
        if len(distinct) > 1:
            raise ValueError(f"frame_velocity_limit: the clips of a batch must share one fps (frame_dt = 1 / fps), got {distinct}")
        f = distinct[0] if distinct else None
        if f is None:
            return
    for g in gmrs:
        g.set_frame_velocity_limit(frame_velocity_limit, f)


def retarget_clips(src_human: str, tgt_robot: str, clips: Sequence, fps: Sequence[float],
                   actual_human_height=None, height_adjust: bool = True,
                   root_origin_offset: bool = True, offset_to_ground: bool = False, chunk=None, report: Optional[List] = None,
                   library=False, velocity_limit=None, frame_velocity_limit=None, body_weights=None):
    """Retarget many clips of one (source, robot, height) in ONE IK launch.  ``body_weights``: None, or one entry per clip, each
    None or ``[T_i, nhuman]`` per-frame body weights (0 = the body is missing in that frame: :meth:`GeneralMotionRetargeting.retarget_streams`),
    packed into the batch beside the frames; refused (``ValueError``) together with ``chunk``.  ``velocity_limit``, ``frame_velocity_limit``: see :class:`ClipRetargeter`.  ``library`` (``True`` | ``"world"`` | ``"reference"``;
    default off): returns ``(motions, motion_library.MotionLibrary)``, the library filled on the device from the post-processed
    batch; ``motions`` are the same bytes as without it.  ``chunk`` (``chunking.ChunkSpec`` or ``"auto"``; default
    off) cuts long clips into independently running chunks -- NOT parity; the per-clip chunk reports are appended to ``report``.

    ``clips[i]`` is a list of ``human_data`` dicts or an array ``[T_i, nhuman, 7]`` (ragged lengths
    are fine: streams are padded and the kernel stops each stream at its own length).
    Returns one motion dict per clip, identical to processing the clips one by one.

    ``actual_human_height``: a number (or None) for all clips, or one height per clip: still ONE solver and ONE IK launch, the
    heights travel as per-stream scale rows, and the motions are the bytes of one call per height.  Scale rows are not
    gathered into chunk jobs: with a ``chunk`` spec that takes effect the heights run as groups, one call per height as before
    (and no ``library``).
    """
    if body_weights is not None and chunk is not None:
        raise ValueError(chunking.BODY_WEIGHTS_REFUSAL)
    if actual_human_height is not None and np.ndim(actual_human_height) > 0:
        heights = [float(h) for h in np.asarray(actual_human_height, dtype=np.float64).reshape(-1)]
        if len(heights) != len(clips):
            raise ValueError(f"{len(heights)} heights for {len(clips)} clips")
        if heights_groups_needed(chunk, [len(c) for c in clips]):
            if library:
                raise ValueError("a motion library takes one job: chunked clips of several heights run as height groups")
            out: List = [None] * len(clips)
            for h in dict.fromkeys(heights):
                idxs = [i for i, x in enumerate(heights) if x == h]
                for i, md in zip(idxs, retarget_clips(src_human, tgt_robot, [clips[i] for i in idxs], [fps[i] for i in idxs], h, height_adjust,
                                                      root_origin_offset, offset_to_ground, chunk=chunk, report=report,
                                                      velocity_limit=velocity_limit, frame_velocity_limit=frame_velocity_limit)):
                    out[i] = md
            return out
    rt = ClipRetargeter(src_human, tgt_robot, actual_human_height, height_adjust, root_origin_offset, offset_to_ground, chunk=chunk,
                        library=library, velocity_limit=velocity_limit, frame_velocity_limit=frame_velocity_limit)
    out = rt(clips, fps) if body_weights is None else rt(clips, fps, body_weights)
    if report is not None and rt.chunk_report is not None:
        report.extend(rt.chunk_report)
    return (out, rt.library) if library else out


def heights_groups_needed(chunk, lens) -> bool:
    """Whether a batch of these clip lengths whose heights would travel as scale rows has to run as one job per height
    instead: a chunk spec takes effect on it (some clip is longer than the spec's ``frames``).  The slots of a chunk job are
    not streams, and their scale rows are not gathered (DESIGN.md section 6g names that as the follow-up)."""
    return chunking.resolve_any(chunk, np.asarray(lens, dtype=np.int64)) is not None


def retarget_mixed(groups: Sequence[Dict], offset_to_ground: bool = False, slices: int = 0, pinned_outputs: bool = False):
    """Mixed-robot batch (BASELINE.json configs[3]; SURVEY.md section 8d "one kernel with per-stream model index"): every
    group = one (source, robot, height) with its own streams; ALL groups form one scheduling domain on the device --
    the robots of the throughput kernel's size class (every shipped one) share a resident grid and one queue of
    (robot, stream, chunk) items (``gmr_retarget_group``) -- and the host buffers are cut into slices whose copies
    overlap the kernels.  Bit-identical to retargeting every group by itself.

    ``groups[i]`` = ``{"src_human", "tgt_robot", "human": f64[S,T,nhuman,7], optional "lens", "weights" (f64[S,T,nhuman]
    per-frame body weights of the group's streams),
    "actual_human_height", "velocity_limit", "frame_velocity_limit", "fps"}`` (the limits as in ``GeneralMotionRetargeting``: they
    are the group's own, each job launches with its solver's tables; a frame limit needs the group's ``fps``), the height a number for the group or one per stream (``f64[S]``: the group's solver is built
    from the unscaled config and the heights travel as scale rows); arrays allocated with ``_lib.pinned_empty`` are copied asynchronously.
    Returns a list of ``(qpos[S,T,nq], nsolve[S,T,2], status[S])``.
    """
    jobs, keep = [], []
    for g in groups:
        h = g.get("actual_human_height")
        per_stream = h is not None and np.ndim(h) > 0
        gmr = GeneralMotionRetargeting(g["src_human"], g["tgt_robot"], actual_human_height=None if per_stream else h,
                                       velocity_limit=g.get("velocity_limit"),
                                       frame_velocity_limit=g.get("frame_velocity_limit"), fps=g.get("fps"))
        keep.append(gmr)
        jobs.append({"solver": gmr.hip_solver, "human": g["human"], "lens": g.get("lens"),
                     "scales": gmr.stream_scales(len(g["human"]), heights=h) if per_stream else None, "weights": g.get("weights")})
    flags = _lib.FLAG_OFFSET_TO_GROUND if offset_to_ground else 0
    return _lib.retarget_group(jobs, flags, slices, out_pinned=pinned_outputs)   # (rows beyond a stream's length: zeros)


def retarget_bvh_files(bvh_files: Sequence[str], tgt_robot: str, fps: float = 30.0, height_adjust: bool = False,
                       root_origin_offset: bool = False, chunk=None, report: Optional[List] = None, velocity_limit=None,
                       frame_velocity_limit=None) -> List[Dict]:
    """``scripts/bvh_to_robot_dataset.py:60-152`` for a list of files: every BVH clip becomes one
    stream of ONE launch (LAFAN1: 77 ragged clips).  Both adjustments default to off like that script
    (``HEIGHT_ADJUST = False``, :128); the loader's hard-coded height 1.75 is used (lafan1.py:39).
    On the device path (:func:`bvh_path`) only the text is parsed here: the raw rows are uploaded and ``gmr_bvh_frames_dev``
    writes the packed frames into the IK batch (files of several skeletons: one call per topology)."""
    from .utils.lafan1 import load_lafan1_packed, read_bvh_raw
    gmr = GeneralMotionRetargeting("bvh", tgt_robot, actual_human_height=1.75)
    if bvh_path() == "device":
        clips = [read_bvh_raw(f) for f in bvh_files]
    else:
        clips = [load_lafan1_packed(f, gmr.human_body_names)[0] for f in bvh_files]
    return retarget_clips("bvh", tgt_robot, clips, [fps] * len(clips), actual_human_height=1.75,
                          height_adjust=height_adjust, root_origin_offset=root_origin_offset, chunk=chunk, report=report,
                          velocity_limit=velocity_limit, frame_velocity_limit=frame_velocity_limit)


def retarget_smplx_files(smplx_files: Sequence[str], smplx_body_model_path: str, tgt_robot: str, tgt_fps: int = 30,
                         height_adjust: bool = True, root_origin_offset: bool = True,
                         skip_errors: bool = True, chunk=None, report: Optional[List] = None,
                         velocity_limit=None, frame_velocity_limit=None) -> List[Optional[Dict]]:
    """``scripts/smplx_to_robot_dataset.py:39-146`` (``process_file``) for a list of AMASS-style SMPL-X
    files, everything after the file read on the device: joints-only body model + fps alignment
    (utils/smpl.py) -> packed frames -> IK (one group launch for all heights) -> FK post-processing.
    Returns one motion dict per file in input order (``None`` for a file that failed to load when
    ``skip_errors`` -- the script prints and skips, :62-76)."""
    raws, ok = [], []
    for i, f in enumerate(smplx_files):
        try:
            raws.append(_load_smplx_raw(f))
            ok.append(i)
        except Exception as e:  # noqa: BLE001 - mirrors the script's print-and-skip
            if not skip_errors:
                raise
            print(f"Error loading {f}: {e}")
    out: List[Optional[Dict]] = [None] * len(smplx_files)
    for i, md in zip(ok, retarget_smplx_loaded(raws, smplx_body_model_path, tgt_robot, tgt_fps, height_adjust, root_origin_offset,
                                               chunk=chunk, report=report, velocity_limit=velocity_limit,
                                               frame_velocity_limit=frame_velocity_limit)):
        out[i] = md
    return out


def retarget_single_clip(retargeter: GeneralMotionRetargeting, frames: Sequence, fps: float,
                         skip_first_frame: bool = True) -> Dict:
    """The save path of the single-clip scripts (``scripts/smplx_to_robot.py:104-161``,
    ``scripts/bvh_to_robot.py`` alike): one ``retarget()`` per displayed frame, then a pkl dict with
    ``root_rot`` xyzw, ``local_body_pos = None`` and ``link_body_list = None`` (:146-158).  Their loop
    increments the index BEFORE the first use (:104-111), so frame 0 is never retargeted; that is the default
    here too.  One launch instead of one call per frame; continues from ``retargeter``'s configuration."""
    seq = frames[1:] if skip_first_frame else frames
    qpos = retargeter.retarget_clip(seq)
    return motion_dict(fps, qpos[:, :3].copy(), qpos[:, [4, 5, 6, 3]].copy(), qpos[:, 7:].copy(), None, None)


# ----------------------------------------------------------------------------------------------
# the dataset drivers with the reference's FILE semantics
#   python -m general_motion_retargeting_amd.dataset --source smplx|bvh --src_folder ... --tgt_folder ... --robot ...
# (scripts/smplx_to_robot_dataset.py:171-242, scripts/bvh_to_robot_dataset.py:16-157): same folder walk, same
# skip-if-exists / --override rule, same exclusion lists, one pkl per input -- but the files of a batch share ONE IK
# launch (and one FK launch per clip) instead of one process per file.
# ----------------------------------------------------------------------------------------------
EXCLUDE_FILE_CONTENT = ["BMLrub", "EKUT", "crawl", "_lie", "upstairs", "downstairs"]    # smplx_to_robot_dataset.py:218


def natural_key(name: str):
    """Sort key of ``natsort.natsorted`` (default algorithm: runs of digits compare as unsigned integers)."""
    import re
    parts = re.split(r"(\d+)", name)
    return [int(p) if p.isdigit() else p for p in parts if p != ""]


def _natsorted(names):
    try:                                   # the reference uses natsort; not installed here -> same order from natural_key
        from natsort import natsorted
        return natsorted(names)
    except ImportError:
        def key(n):
            return [(0, p, "") if isinstance(p, int) else (1, 0, p) for p in natural_key(n)]
        return sorted(names, key=key)


def load_hard_motions(paths) -> List[str]:
    """Names listed in the ``assets/hard_motions/*.txt`` reports (``Motion: <name>.pkl, Difficulty: ...``;
    smplx_to_robot_dataset.py:196-205)."""
    import os
    out = []
    for p in paths:
        if not os.path.exists(p):
            continue
        with open(p, "r") as f:
            for line in f:
                if "Motion:" not in line:
                    continue
                motion_path = line.split(":")[1].strip()
                out.append(motion_path.split(",")[0].strip().split(".")[0])
    return out


def list_smplx_jobs(src_folder: str, tgt_folder: str, override: bool = False, hard_motions: Sequence[str] = (),
                    exclude: Sequence[str] = tuple(EXCLUDE_FILE_CONTENT)):
    """(source file, target pkl) pairs in the reference's order and with its filters (:208-228): natsorted walk,
    ``*_stagei.npz`` skipped, ``.pkl`` / ``.npz`` accepted, existing targets skipped unless ``override``, hard and
    infeasible motions removed."""
    import os
    jobs = []
    for dirpath, _, filenames in os.walk(src_folder):
        for filename in _natsorted(filenames):
            if filename.endswith("_stagei.npz"):
                continue
            if filename.endswith((".pkl", ".npz")):
                src = os.path.join(dirpath, filename)
                tgt = src.replace(src_folder, tgt_folder).replace(".npz", ".pkl")
                if not os.path.exists(tgt) or override:
                    jobs.append((src, tgt))
    hard = set(hard_motions)
    kept = []
    for src, tgt in jobs:
        motion_name = src.split("/")[-1].split(".")[0]
        if motion_name in hard or any(c in motion_name for c in exclude):
            continue
        kept.append((src, tgt))
    return jobs, kept


def list_bvh_jobs(src_folder: str, tgt_folder: str, override: bool = False, verbose: bool = True):
    """(bvh file, target pkl) pairs of ``bvh_to_robot_dataset.py:60-73``: sorted walk, ``.bvh`` only, existing targets
    skipped (with the script's message) unless ``override``."""
    import os
    jobs = []
    for dirpath, _, filenames in os.walk(src_folder):
        for filename in sorted(filenames):
            if not filename.endswith(".bvh"):
                continue
            src = os.path.join(dirpath, filename)
            tgt = src.replace(src_folder, tgt_folder).replace(".bvh", ".pkl")
            if os.path.exists(tgt) and not override:
                if verbose:
                    print(f"Skipping {src} because {tgt} exists")
                continue
            jobs.append((src, tgt))
    return jobs


def _dump(tgt: str, motion: Dict, key_order: Sequence[str]) -> None:
    import os
    import pickle
    os.makedirs(os.path.dirname(tgt) or ".", exist_ok=True)
    with open(tgt, "wb") as f:
        pickle.dump({k: motion[k] for k in key_order}, f)


SMPLX_KEYS = ("fps", "root_pos", "root_rot", "dof_pos", "local_body_pos", "link_body_list")      # :134-141
BVH_KEYS = ("root_pos", "root_rot", "dof_pos", "local_body_pos", "fps", "link_body_list")        # bvh script :141-148


# ----------------------------------------------------------------------------------------------
# The pipeline behind both drivers: loading, retargeting and writing overlap, and a batch
# is sized for the throughput shape of the kernel -- a budget of (padded) frames, thousands of clips -- instead of a
# fixed number of files.
#
#   loader pool (processes / threads)   load(src) -> clip          batch k + 1, k + 2 are being read and parsed ...
#   this thread (the GPU)               retarget(batch) -> dicts   ... while batch k is on the device ...
#   writer threads                      pickle.dump                ... and batch k - 1 is written.
#
# The GPU call releases the GIL (ctypes), so the pools keep running underneath it.  Output files are independent of
# each other, so the jobs may be processed in any order: the drivers sort them by cost (largest first), which keeps
# the padding of a ragged batch small and is also the order LPT sharding over ranks wants.
# ----------------------------------------------------------------------------------------------
class DatasetPipeline:
    def __init__(self, load, retarget, frames_of, key_order, frames_budget: int = 1 << 19, max_clips: int = 16384,
                 loader=None, prefetch_clips: int = 4096, writers: int = 4, verbose: bool = True, label: str = ""):
        """``load(src)`` -> clip (any object; runs in ``loader``, a ``concurrent.futures`` executor, or inline when None);
        ``frames_of(clip)`` -> frames of the clip; ``retarget(clips, srcs)`` -> one motion dict (or None) per clip, on
        this thread; ``frames_budget`` bounds ``len(batch) * longest clip`` (the padded batch the kernel is given).
        A ``retarget`` object with ``begin / add / finish`` (:class:`ClipRetargeter` via :class:`_Staged`) is handed every
        clip when it arrives, so that packing the batch happens while this thread would wait for the loaders anyway."""
        self.load, self.retarget, self.frames_of, self.key_order = load, retarget, frames_of, tuple(key_order)
        self.frames_budget, self.max_clips = max(int(frames_budget), 1), max(int(max_clips), 1)
        self.loader, self.prefetch_clips, self.writers = loader, max(int(prefetch_clips), 1), max(int(writers), 1)
        self.verbose, self.label = verbose, label
        self.stats = {"clips": 0, "frames": 0, "batches": 0, "load_errors": 0, "seconds_gpu": 0.0, "seconds_waiting_for_loads": 0.0,
                      "seconds_waiting_for_writes": 0.0, "seconds_total": 0.0}

    def _submit(self, src):
        import concurrent.futures as cf
        if self.loader is not None:
            return self.loader.submit(self.load, src)
        f = cf.Future()
        try:
            f.set_result(self.load(src))
        except Exception as e:  # noqa: BLE001
            f.set_exception(e)
        return f

    def run(self, jobs: Sequence, after_submit=None) -> int:
        """``jobs`` = (src, tgt) pairs.  Returns the number of files written.  ``after_submit()`` runs on this thread once
        the first window of loads has been handed to the pool (work that can hide under the loaders' start-up)."""
        import collections
        import concurrent.futures as cf
        import time
        t_start = time.perf_counter()
        jobs = list(jobs)
        todo = collections.deque(jobs)
        inflight = collections.deque()           # (src, tgt, future) in job order
        done = 0
        writes = collections.deque()
        with cf.ThreadPoolExecutor(self.writers) as wpool:
            batch, longest = [], 0

            staged = hasattr(self.retarget, "add")

            def flush():
                nonlocal batch, longest, done
                if not batch:
                    return
                t0 = time.perf_counter()
                if staged:
                    motions = self.retarget.finish([s for s, _, _ in batch])
                else:
                    motions = self.retarget([c for _, _, c in batch], [s for s, _, _ in batch])
                self.stats["seconds_gpu"] += time.perf_counter() - t0
                self.stats["batches"] += 1
                for (src, tgt, clip), md in zip(batch, motions):
                    if md is None:
                        continue
                    writes.append(wpool.submit(_dump, tgt, md, self.key_order))
                    done += 1
                    self.stats["clips"] += 1
                    self.stats["frames"] += int(clip) if staged else int(self.frames_of(clip))
                    if self.verbose:
                        print(f"Processed {done}/{len(jobs)}: {tgt}")
                while len(writes) > 4 * self.max_clips:          # bound the dicts waiting for the writers
                    writes.popleft().result()
                batch, longest = [], 0

            while todo or inflight:
                while todo and len(inflight) < self.prefetch_clips:
                    src, tgt = todo.popleft()
                    inflight.append((src, tgt, self._submit(src)))
                if after_submit is not None:
                    after_submit()
                    after_submit = None
                src, tgt, fut = inflight.popleft()
                try:
                    t_w = time.perf_counter()
                    clip = fut.result()
                    self.stats["seconds_waiting_for_loads"] += time.perf_counter() - t_w
                except Exception as e:  # noqa: BLE001 -- the scripts print and skip (smplx_to_robot_dataset.py:62-76)
                    print(f"Error loading {src}: {e}")
                    self.stats["load_errors"] += 1
                    continue
                n = int(self.frames_of(clip))
                if staged:
                    if not batch:
                        self.retarget.begin(n, self.max_clips, self.frames_budget)
                    if not self.retarget.add(clip):
                        flush()
                        self.retarget.begin(n, self.max_clips, self.frames_budget)
                        if not self.retarget.add(clip):
                            raise RuntimeError(f"{src}: clip does not fit an empty batch")
                    batch.append((src, tgt, n))           # (the frames now live in the staged batch)
                    longest = max(longest, n)
                    continue
                if batch and ((len(batch) + 1) * max(longest, n) > self.frames_budget or len(batch) >= self.max_clips):
                    flush()
                batch.append((src, tgt, clip))
                longest = max(longest, n)
            flush()
            t_w = time.perf_counter()
            for w in writes:
                w.result()                                        # a failed write raises here
            self.stats["seconds_waiting_for_writes"] = time.perf_counter() - t_w
        self.stats["seconds_total"] = time.perf_counter() - t_start
        return done


class _Staged:
    """:class:`ClipRetargeter` behind the staged protocol of :class:`DatasetPipeline` with a fixed fps per clip."""

    def __init__(self, rt: "ClipRetargeter", fps: float):
        self.rt, self.fps = rt, fps

    def begin(self, longest, max_clips, frames_budget):
        self.rt.begin(longest, max_clips, frames_budget)

    def add(self, clip):
        return self.rt.add(clip)

    def finish(self, files):
        return self.rt.finish([self.fps] * len(files))


def job_cost(src: str) -> int:
    """Cheap proxy of a file's frame count, the same on every rank: BVH -- the ``Frames:`` line of its header; anything
    else -- the file size.  Used to order the jobs and to shard them over ranks (LPT)."""
    import os
    if src.endswith(".bvh"):
        try:
            with open(src, "r", errors="replace") as f:
                for i, line in enumerate(f):
                    if line.lstrip().startswith("Frames:"):
                        return int(line.split(":")[1])
                    if i > 4000:
                        break
        except (OSError, ValueError):
            pass
    try:
        return int(os.path.getsize(src))
    except OSError:
        return 0


def shard_jobs(jobs: Sequence, rank: int = 0, world: int = 1, cost=job_cost):
    """This rank's jobs, largest first: ``sharding.lpt_partition`` on the cost of every job (deterministic: every rank
    computes the same partition from the same folder walk)."""
    from .sharding import lpt_partition
    jobs = list(jobs)
    costs = [int(cost(s)) for s, _ in jobs]
    mine = lpt_partition(costs, world)[rank] if world > 1 else list(range(len(jobs)))
    mine = sorted(mine, key=lambda i: (-costs[i], i))
    return [jobs[i] for i in mine]


def _skip_existing(jobs, override: bool, verbose: bool):
    """skip-if-exists of the scripts (bvh_to_robot_dataset.py:66-70, smplx_to_robot_dataset.py:213-215) on a job list"""
    import os
    if override:
        return list(jobs)
    kept = []
    for src, tgt in jobs:
        if os.path.exists(tgt):
            if verbose:
                print(f"Skipping {src} because {tgt} exists")
            continue
        kept.append((src, tgt))
    return kept


def _loader_pool(kind: str, workers: int):
    """Process pool (BVH: pure-Python parsing holds the GIL) or thread pool (npz: the reads release it).  Processes are
    SPAWNED, never forked: this process may already have initialised the GPU."""
    import concurrent.futures as cf
    import multiprocessing as mp
    if workers <= 0:
        return None
    if kind == "process":
        return cf.ProcessPoolExecutor(workers, mp_context=mp.get_context("spawn"))
    return cf.ThreadPoolExecutor(workers)


def default_workers(world: int = 1) -> int:
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 4)
    return max(1, min(16, n // max(world, 1)))


# ---- BVH ---------------------------------------------------------------------------------------------------------------
def _load_bvh_clip(args):
    """(file, body names[, raw]) -> packed frames f64[T, nhuman, 7], or with ``raw`` the parsed text alone
    (``lafan1.BvhRaw``: less to compute here and less to pickle back; the frames are computed on the device) unless the
    device path does not take the file; module-level: runs in spawned worker processes."""
    from .utils import lafan1
    f, names = args[0], args[1]
    if len(args) > 2 and args[2]:
        raw = lafan1.read_bvh_raw(f)
        if lafan1.device_takes(raw):
            lafan1.selection(raw.names, names)             # an unknown body is this file's error, as on the host path
            lafan1._global_poses_names(raw.names)
            lafan1.topology_key(raw)                       # (computed here, kept on the clip)
            return raw
        return lafan1.packed_from_raw(raw, names)
    return lafan1.load_lafan1_packed(f, names)[0]


def run_bvh_dataset(src_folder: str, tgt_folder: str, robot: str, override: bool = False, batch_files: int = 0,
                    retarget=None, verbose: bool = True, frames_budget: int = 1 << 19, loader_workers: int = -1,
                    rank: int = 0, world: int = 1, load=None, stats: Optional[Dict] = None, chunk=None, velocity_limit=None,
                    frame_velocity_limit=None) -> int:
    """``bvh_to_robot_dataset.py`` (:60-157) on the pipeline above.  ``velocity_limit``, ``frame_velocity_limit`` (at the 30 fps of the clips): see :class:`ClipRetargeter`.  ``chunk``: see :class:`ClipRetargeter` (``stats["chunk"]`` gets the totals).  ``batch_files`` > 0 additionally caps the clips of a
    launch (0: only the frames budget does).  ``retarget(clips, files)`` and ``load(file)`` are injectable (tests)."""
    # the partition is computed on ALL source files (a rank that starts later must not see another partition because
    # some targets exist by then); skip-if-exists is applied to the rank's own shard
    workers = default_workers(world) if loader_workers < 0 else loader_workers
    pool = _loader_pool("process" if load is None else "thread", workers)     # first: the workers start up under what follows
    jobs = _skip_existing(shard_jobs(list_bvh_jobs(src_folder, tgt_folder, True, False), rank, world), override, verbose)
    gmr = None
    if load is None or retarget is None:
        gmr = GeneralMotionRetargeting("bvh", robot, actual_human_height=1.75)
    names = gmr.human_body_names if gmr is not None else None
    rt = None
    if retarget is None:
        rt = ClipRetargeter("bvh", robot, 1.75, height_adjust=False, root_origin_offset=False, chunk=chunk,    # HEIGHT_ADJUST = False, :128
                            velocity_limit=velocity_limit, frame_velocity_limit=frame_velocity_limit)
        retarget = _Staged(rt, 30)
    raw = rt is not None and bvh_path() == "device"        # the loaders only parse; gmr_bvh_frames_dev computes the frames
    try:
        pipe = DatasetPipeline((lambda f: _load_bvh_clip((f, names, raw))) if (load is None and pool is None) else (load or _BvhLoad(names, raw)),
                               retarget, len, BVH_KEYS, frames_budget, batch_files if batch_files > 0 else 16384, pool,
                               verbose=verbose, label="bvh")

        def reserve():
            row_doubles = 0
            if raw:
                try:                                       # columns of a motion row, from the first file's hierarchy
                    from .utils import lafan1
                    hdr = lafan1.read_bvh_raw(jobs[0][0], header_only=True)
                    row_doubles = {3: 3 + 3 * len(hdr.parents), 6: 6 * len(hdr.parents)}.get(hdr.channels, 0)
                except Exception:  # noqa: BLE001 -- a broken first file: the batch locks its pages when it knows
                    return
                if row_doubles == 0:
                    return
            rt.reserve(min(frames_budget, 420 * len(jobs)), row_doubles)
        # lock the pages of the first batch while the loader processes start up and parse the first files
        warm = reserve if (rt is not None and len(jobs) > 64) else None
        done = pipe.run(jobs, warm)
    finally:
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)
    if stats is not None:
        stats.update(pipe.stats)
        if rt is not None:
            stats["seconds_gpu_parts"] = dict(rt.timing)
            if rt.chunk_summary:
                stats["chunk"] = dict(rt.chunk_summary)
    if verbose:
        print("Done. saved to ", tgt_folder)
    return done


class _BvhLoad:
    """Picklable ``load`` for the process pool."""

    def __init__(self, names, raw: bool = False):
        self.names, self.raw = list(names), bool(raw)

    def __call__(self, f):
        return _load_bvh_clip((f, self.names, self.raw))


# ---- SMPL-X ---------------------------------------------------------------------------------------------------------------
def _load_smplx_raw(f):
    """The arrays ``load_smplx_file`` reads from an AMASS-style file (utils/smpl.py:12-41), nothing computed: runs in the
    loader threads."""
    with np.load(f, allow_pickle=False) as z:
        return {k: np.asarray(z[k]) for k in ("gender", "betas", "root_orient", "pose_body", "trans", "mocap_frame_rate")}


def retarget_smplx_loaded(raws: Sequence[Dict], smplx_body_model_path: str, tgt_robot: str, tgt_fps: int = 30,
                          height_adjust: bool = True, root_origin_offset: bool = True,
                          timing: Optional[Dict[str, float]] = None, chunk=None, report: Optional[List] = None,
                          library=False, velocity_limit=None, frame_velocity_limit=None):
    """``process_file`` (smplx_to_robot_dataset.py:39-146) for many already-read files: joints-only body model and fps
    alignment on the device, ONE solver (built from the unscaled config, kept from batch to batch) and ONE IK job for the
    whole batch -- a file's height comes from its betas (:36-39) and travels as that clip's scale row
    (``ik_config.scale_rows``), so a motion library of the batch is not limited by the count of heights -- and two FK launches
    for the post-processing of all clips together.  ``GMR_DATASET_HEIGHTS=groups`` (:func:`heights_path`) keeps one solver and
    one job per height in one group launch; the bytes are the same.  Scale rows are not gathered into chunk jobs: with a
    ``chunk`` spec that takes effect the batch runs as height groups whatever the switch says.  On the device path (:func:`smplx_path`, and every
    body model of the batch one that ``utils.smpl.smplx_device_takes``) the files' arrays go up as they are and ONE
    ``gmr_smplx_batch_frames_dev`` call writes the packed frames of all clips where the IK kernels read them; otherwise one
    ``gmr_smplx_frames`` call per clip and a padded upload -- the same bits.  ``timing`` accumulates the seconds of the stages.
    ``library`` (``True`` | ``"world"`` | ``"reference"``; default off): returns ``(motions, motion_library.MotionLibrary)`` as
    :func:`retarget_clips` does, the clips in the order of ``raws``; the batch must then be one job (the merged path).
    ``frame_velocity_limit``: see :class:`ClipRetargeter`; ``frame_dt`` is ``1 / `` the aligned fps of the batch (``tgt_fps``,
    unless the files are slower), and files whose aligned fps differ raise ``ValueError``."""
    from .utils import smpl
    t0 = time.perf_counter()
    from .ik_config import scale_rows
    packed, fps_of, height, bms = {}, {}, {}, {}
    for i, d in enumerate(raws):
        bms[i] = smpl.body_model_for(smplx_body_model_path, str(d["gender"]))
        betas = np.asarray(d["betas"])
        height[i] = float(1.66 + 0.1 * (betas[0] if betas.ndim == 1 else betas[0, 0]))
    # merged: the frame counts decide below whether a chunk spec takes effect; they need no solver (AMASS files say them)
    merged = heights_path() == "merged" and bool(raws)
    if merged and chunk is not None:
        merged = not heights_groups_needed(chunk, [smpl.smplx_frame_count(d, tgt_fps) for d in raws])
    gmr_of: Dict[Optional[float], GeneralMotionRetargeting] = {}
    if merged:
        gmr_of[None] = _smplx_base_retargeter(tgt_robot)
        gmr_of[None].set_velocity_limit(velocity_limit)      # (the kept retargeter serves every batch: this batch's limit, or none)
    else:
        for h in height.values():
            if h not in gmr_of:
                gmr_of[h] = GeneralMotionRetargeting("smplx", tgt_robot, actual_human_height=h, velocity_limit=velocity_limit)
    group_of = {i: (None if merged else height[i]) for i in height}
    if gmr_of:
        _refuse_chunk_under_frame_limit(next(iter(gmr_of.values())), frame_velocity_limit, chunk)
    device = post_path() == "device" and bool(raws)
    any_g = next(iter(gmr_of.values()), None)
    raw = device and smplx_path() == "device" and all(smpl.smplx_device_takes(bm, any_g) for bm in {id(b): b for b in bms.values()}.values())
    for i, d in enumerate(raws):
        if raw:         # nothing per frame on the host: the arrays as float32, the frame counts, the subject's rest joints
            packed[i] = smpl.smplx_raw_clip(d, bms[i], tgt_fps)
            fps_of[i] = packed[i]["aligned_fps"]
        else:
            packed[i], fps_of[i] = smpl.smplx_frames_packed_fused(gmr_of[group_of[i]], d, bms[i], tgt_fps=tgt_fps)      # body model + alignment, one call
    _set_batch_frame_limit(gmr_of.values(), frame_velocity_limit, fps_of.values())     # (the kept retargeter: this batch's limit, or none)
    t1 = time.perf_counter()
    dp = _smplx_device_post(any_g.xml_file) if device else None
    jobs = []
    for n, (h, g) in enumerate(gmr_of.items()):
        idxs = [i for i in range(len(raws)) if group_of[i] == h]
        lens = np.array([packed[i]["nout"] if raw else packed[i].shape[0] for i in idxs], dtype=np.int32)
        T = max(int(lens.max()), 1)
        job = {"solver": g.hip_solver, "lens": lens, "q0": g.model.qpos0, "idxs": idxs, "fps": [fps_of[i] for i in idxs],
               "scales": scale_rows(g._ik_config, [height[i] for i in idxs]) if merged else None}
        jobs.append(job)
        if raw:
            job.update(T=T, smplx= {"handle": smpl.smplx_batch_handle(bms[idxs[0]], g), "clips": [packed[i] for i in idxs]})
            continue
        shape = (len(idxs), T, len(g.human_body_names), 7)
        human = dp[1].pinned(f"human_{n}", shape, np.float64) if device else np.empty(shape)
        human[..., :3] = 0.0
        human[..., 3] = 1.0
        human[..., 4:] = 0.0
        for k, i in enumerate(idxs):
            human[k, : lens[k]] = packed[i]
        job["human"] = human
    if timing is not None:
        timing["prepare"] = timing.get("prepare", 0.0) + t1 - t0
        timing["pack"] = timing.get("pack", 0.0) + time.perf_counter() - t1
        # counts, not seconds: batches, their IK jobs, and the batches wide enough (more than 300 streams in all) for the
        # throughput shape of the IK kernel; the others run the latency shape job by job
        for k, v in (("n_batches", 1), ("n_ik_jobs", len(jobs)), ("n_batches_throughput_shape", int(len(raws) > 300))):
            timing[k] = timing.get(k, 0) + v
    lib_mode = None if not library else ("world" if library is True else str(library))
    if not raws:
        return ([], None) if library else []
    if lib_mode is not None and len(jobs) != 1:
        raise ValueError("a motion library takes the clips in the order they were handed over: one job (the merged heights path)")
    km, post = dp if device else (KinematicsModel(any_g.xml_file), None)
    out, lib_, reports = _run_batch(jobs, km, 0, height_adjust, root_origin_offset, chunk, lib_mode, timing, post)
    if report is not None:
        report.extend(r for rs in reports if rs is not None for r in rs)
    return (out, lib_) if library else out


_SMPLX_DEVICE_POST: Dict[str, tuple] = {}
_SMPLX_BASE: Dict[str, GeneralMotionRetargeting] = {}


def _smplx_base_retargeter(tgt_robot: str) -> GeneralMotionRetargeting:
    """The retargeter of a robot built from the UNSCALED config, kept for the batches of a run: every height is a scale row
    of its one solver, so a batch builds nothing."""
    if tgt_robot not in _SMPLX_BASE:
        _SMPLX_BASE[tgt_robot] = GeneralMotionRetargeting("smplx", tgt_robot)
    return _SMPLX_BASE[tgt_robot]


def _smplx_device_post(xml_file: str):
    """(KinematicsModel, DevicePost) of a robot, kept for the batches of a run: the FK handle owns the device scratch of the
    post-processing, the DevicePost the device buffers and the page-locked staging."""
    key = str(xml_file)
    if key not in _SMPLX_DEVICE_POST:
        _SMPLX_DEVICE_POST[key] = (KinematicsModel(xml_file), DevicePost())
    return _SMPLX_DEVICE_POST[key]


def run_smplx_dataset(src_folder: str, tgt_folder: str, robot: str, smplx_folder: str, override: bool = False,
                      hard_motion_files: Sequence[str] = (), batch_files: int = 0, retarget=None, verbose: bool = True,
                      frames_budget: int = 1 << 19, loader_workers: int = -1, rank: int = 0, world: int = 1, load=None,
                      stats: Optional[Dict] = None, chunk=None, velocity_limit=None, frame_velocity_limit=None) -> int:
    """``smplx_to_robot_dataset.py:main`` (:171-242) on the pipeline above.  ``retarget(raws, files)`` defaults to
    :func:`retarget_smplx_loaded`, ``load(file)`` to the npz reader (tests inject stand-ins).  Returns the number of pkl
    files this rank wrote."""
    hard = load_hard_motions(hard_motion_files)
    all_jobs, jobs = list_smplx_jobs(src_folder, tgt_folder, override, hard)
    if verbose and rank == 0:
        print("full args_list:", len(all_jobs))
        print("new args_list:", len(jobs))
        print(f"Total number of files to process: {len(jobs)}")
    if world > 1:      # partition ALL files (see run_bvh_dataset), then drop what exists from this rank's shard
        jobs = _skip_existing(shard_jobs(list_smplx_jobs(src_folder, tgt_folder, True, hard)[1], rank, world), override, False)
    else:
        jobs = shard_jobs(jobs, rank, world)
    timing: Dict[str, float] = {}
    chunk_summary: Dict = {}
    if retarget is None:
        def retarget(raws, files):
            rep: List = []
            out = retarget_smplx_loaded(raws, smplx_folder, robot, timing=timing, chunk=chunk, report=rep, velocity_limit=velocity_limit,
                                        frame_velocity_limit=frame_velocity_limit)
            if rep:
                chunking.summarize(rep, chunk_summary)
            return out
    workers = default_workers(world) if loader_workers < 0 else loader_workers
    pool = _loader_pool("thread", workers if len(jobs) > 1 else 0)
    try:
        pipe = DatasetPipeline(load or _load_smplx_raw, retarget, lambda d: len(d["trans"]) if isinstance(d, dict) else len(d),
                               SMPLX_KEYS, frames_budget, batch_files if batch_files > 0 else 16384, pool, verbose=verbose,
                               label="smplx")
        done = pipe.run(jobs)
    finally:
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)
    if stats is not None:
        stats.update(pipe.stats)
        if timing:
            stats["seconds_gpu_parts"] = dict(timing)
        if chunk_summary:
            stats["chunk"] = dict(chunk_summary)
    if verbose:
        print("Done. Saved to ", tgt_folder)
    return done


def _retarget_bvh_skipping_errors(bvh_files: Sequence[str], tgt_robot: str) -> List[Optional[Dict]]:
    """:func:`retarget_bvh_files` with the script's print-and-skip for files that fail to load (:77-82)."""
    from .utils.lafan1 import load_lafan1_packed
    gmr = GeneralMotionRetargeting("bvh", tgt_robot, actual_human_height=1.75)
    ok, clips = [], []
    for i, f in enumerate(bvh_files):
        try:
            clips.append(load_lafan1_packed(f, gmr.human_body_names)[0])
            ok.append(i)
        except Exception as e:  # noqa: BLE001 - mirrors the script
            print(f"Error loading {f}: {e}")
    out: List[Optional[Dict]] = [None] * len(bvh_files)
    if clips:
        res = retarget_clips("bvh", tgt_robot, clips, [30] * len(clips), actual_human_height=1.75,
                             height_adjust=False, root_origin_offset=False)
        for i, md in zip(ok, res):
            out[i] = md
    return out


def main(argv=None) -> int:
    import argparse
    import json
    import os
    import pathlib
    import sys
    import time
    ap = argparse.ArgumentParser(description="Retarget a folder of SMPL-X (AMASS) or BVH (LAFAN1) motions to a robot: "
                                             "the reference's dataset scripts on the MI355X kernels")
    ap.add_argument("--source", choices=["smplx", "bvh"], default="smplx")
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--src_folder", type=str, required=True)
    ap.add_argument("--tgt_folder", type=str, required=True)
    ap.add_argument("--override", default=False, action="store_true")
    ap.add_argument("--num_cpus", default=-1, type=int, help="loader workers per rank (the reference's mp.Pool size; default: "
                                                             "this rank's share of the host's cores, at most 16)")
    ap.add_argument("--target_fps", default=30, type=int, help="accepted for compatibility (the BVH script ignores it too)")
    ap.add_argument("--smplx_folder", type=str, default=None, help="SMPL-X body models (default: <assets>/body_models)")
    ap.add_argument("--hard_motions", nargs="*", default=None, help="difficulty reports (default: <assets>/hard_motions/{0,1}.txt)")
    ap.add_argument("--batch_files", type=int, default=0, help="cap on the clips of one IK launch (0: the frames budget alone)")
    ap.add_argument("--frames_budget", type=int, default=1 << 19, help="padded frames (clips x longest clip) of one IK launch")
    ap.add_argument("--gpus", type=int, default=1, help="ranks = GPUs of this node; the files are LPT-sharded over them")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--velocity_limit", type=float, default=None, metavar="RAD_PER_S",
                    help="per-joint velocity limit of every IK solve on every motor joint (upstream's use_velocity_limit: 9.42 = 3 pi); "
                         "a bound per solve, not on the velocity between frames (default: none)")
    ap.add_argument("--frame_velocity_limit", type=float, default=None, metavar="RAD_PER_S",
                    help="per-joint velocity limit between consecutive frames of every retargeted clip, on every motor joint, at the "
                         "fps of the clips; not with --chunk_frames (default: none)")
    chunking.add_cli_arguments(ap)
    a = ap.parse_args(argv)
    chunk = chunking.spec_from_args(a)
    from . import launcher
    if a.gpus > 1 and not launcher.is_rank_process():
        # become the launcher: one rank process per GPU, nothing of the GPU is touched here
        cmd = [sys.executable, "-m", "general_motion_retargeting_amd.dataset"] + list(sys.argv[1:] if argv is None else argv)
        return launcher.self_launch(a.gpus, cmd, "GMR_DATASET_TIMEOUT", 86400.0)
    from . import _lib, comm as gcomm, sharding
    rank, local_rank, world = gcomm.env_rank_world()
    cm = None
    if world > 1:
        L = _lib.lib()
        _lib.require_gpu()
        _lib.check(L.gmr_set_device(local_rank % max(L.gmr_device_count(), 1)))
        cm = gcomm.create()
        # the ONE collective of the path: rank 0's compiled (robot, task set) to every rank; a rank whose own plugin files
        # compile to other bytes would silently produce other motions -- that is an error, not a fallback
        g0 = GeneralMotionRetargeting(a.source, a.robot)
        mb, ts = sharding.broadcast_blobs(g0._model_blob if rank == 0 else None, g0._taskset_blob if rank == 0 else None, rank, cm)
        if not (np.array_equal(mb.view(np.uint8), g0._model_blob.view(np.uint8))):
            raise SystemExit(f"rank {rank}: the robot model compiled here differs from rank 0's")
    t0 = time.perf_counter()
    stats: Dict = {}
    if a.source == "bvh":
        n = run_bvh_dataset(a.src_folder, a.tgt_folder, a.robot, a.override, a.batch_files, verbose=not a.quiet,
                            frames_budget=a.frames_budget, loader_workers=a.num_cpus, rank=rank, world=world, stats=stats, chunk=chunk,
                            velocity_limit=a.velocity_limit, frame_velocity_limit=a.frame_velocity_limit)
    else:
        from .params import ASSET_ROOT
        if ASSET_ROOT is None and (a.smplx_folder is None or a.hard_motions is None):
            raise SystemExit("no assets directory: give --smplx_folder and --hard_motions (or set GMR_ASSET_ROOT)")
        assets = pathlib.Path(ASSET_ROOT) if ASSET_ROOT is not None else None      # (only the defaults need it)
        smplx_folder = a.smplx_folder or str(assets / "body_models")
        hard = a.hard_motions if a.hard_motions is not None else [str(assets / "hard_motions" / "0.txt"),
                                                                    str(assets / "hard_motions" / "1.txt")]
        n = run_smplx_dataset(a.src_folder, a.tgt_folder, a.robot, smplx_folder, a.override, hard, a.batch_files,
                              verbose=not a.quiet, frames_budget=a.frames_budget, loader_workers=a.num_cpus, rank=rank,
                              world=world, stats=stats, chunk=chunk, velocity_limit=a.velocity_limit,
                              frame_velocity_limit=a.frame_velocity_limit)
    dt = time.perf_counter() - t0
    if chunk is not None:        # one line per rank: the mode is not parity, so what it did to the seams is always said
        print(json.dumps({"chunk_summary": {"rank": rank, **stats.get("chunk", {"clips_split": 0})}}))
    frames = float(stats.get("frames", 0))
    if cm is not None:
        tot = cm.allgather(frames)
        files = cm.allgather(float(n))
        dt = cm.allreduce_max(dt)
        cm.barrier()
        cm.close()
        frames, n_all = sum(tot), int(sum(files))
    else:
        n_all = n
    if rank == 0:
        print(json.dumps({"dataset_summary": {"files_written": n_all, "frames": int(frames), "seconds": dt,
                                              "frames_per_s": frames / dt if dt > 0 else 0.0, "ranks": world,
                                              "rank0": {k: stats.get(k) for k in ("batches", "seconds_gpu", "seconds_waiting_for_loads",
                                                                                    "seconds_waiting_for_writes", "load_errors", "seconds_gpu_parts")}}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
