"""Chunked retargeting of long clips (opt-in, NOT parity with the sequential run).

Frames of a clip depend on each other (warm start), so the unit of parallelism is the clip, and a dataset of few, long
clips (LAFAN1: 77 clips of up to 9 855 frames) leaves most of the device idle.  With a :class:`ChunkSpec` a clip longer
than ``frames`` is cut into chunks that run as independent IK streams; chunk k >= 1 starts from ``qpos0`` and first runs
``warmup`` frames whose results are dropped.  The frame in front of a chunk is computed twice, so the mode measures its own
error (the seam residual) on the device, re-runs the chunks whose seam is over ``tol`` from their predecessor's final state
(at most ``max_passes`` repair passes) and reports what is left (:class:`ChunkRunner`, ``ClipRetargeter.chunk_report``).

The IK kernels are untouched: a pass is ``gmr_chunk_gather_dev`` -> ``gmr_retarget_group_dev`` on the chunk job ->
``gmr_chunk_stitch_dev`` -> ``gmr_chunk_seams_dev`` and ONE 4-byte read-back (the number of seams over the tolerance).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import re
from typing import Dict, List, Optional, Sequence

import numpy as np

PASS0, REPAIR = 0, 1
# how these were chosen (seam residual against warm-up on long synthetic clips, CPU reference)
DEFAULT_WARMUP = 30
DEFAULT_TOL = 1e-3
DEFAULT_PASSES = 2
AUTO_FLOOR = 120            # "auto" never cuts below this many frames: warm-up is then at most a quarter of a chunk's work
WIDE_STREAMS_PER_CU = 9     # resident streams of the throughput shape (gmr_solver_set_dispatch)


@dataclasses.dataclass(frozen=True)
class ChunkSpec:
    """``frames``: longest run of frames one chunk owns (L); ``warmup``: frames run in front of a chunk and dropped (W);
    ``tol``: a seam is bad when its residual (rad / m / rad) exceeds this; ``max_passes``: repair passes after pass 0
    (0 = report only, ``None`` = until no seam is bad, which ends after at most max K passes)."""
    frames: int
    warmup: int = DEFAULT_WARMUP
    tol: float = DEFAULT_TOL
    max_passes: Optional[int] = DEFAULT_PASSES

    def __post_init__(self):
        if int(self.frames) < 1 or int(self.warmup) < 1:
            raise ValueError("ChunkSpec: frames >= 1 and warmup >= 1")
        if not float(self.tol) >= 0.0:
            raise ValueError("ChunkSpec: tol is a number >= 0")
        if self.max_passes is not None and int(self.max_passes) < 0:
            raise ValueError("ChunkSpec: max_passes >= 0, or None for no bound")


def device_streams() -> int:
    """streams the device holds in the throughput shape: 9 per CU (256 CUs when no device answers)"""
    cus = 256
    try:
        from . import _lib
        m = re.search(r"CUs=(\d+)", _lib.lib().gmr_backend_info().decode())
        if m and int(m.group(1)) > 0:
            cus = int(m.group(1))
    except Exception:  # noqa: BLE001 -- no library / no device: the nominal MI355X
        pass
    return WIDE_STREAMS_PER_CU * cus


def auto_frames(total_frames: int, streams: Optional[int] = None) -> int:
    """L of ``chunk="auto"``: the batch's frames over the streams the device holds, so that the batch has about as many chunks
    as resident wavefronts and every one of them works for the whole launch; never below :data:`AUTO_FLOOR`."""
    streams = device_streams() if streams is None else int(streams)
    return max(AUTO_FLOOR, -(-int(total_frames) // max(streams, 1)))


def resolve(chunk, lens: Sequence[int], total_frames: Optional[int] = None) -> Optional[ChunkSpec]:
    """``None`` | :class:`ChunkSpec` | ``"auto"`` | ``dict`` -> the spec a batch of these clip lengths runs with, or ``None`` when
    no clip is longer than its ``frames`` (the batch then takes the ordinary launch: the bytes it produces today)."""
    if chunk is None:
        return None
    lens = np.asarray(lens, dtype=np.int64)
    if isinstance(chunk, str):
        if chunk.strip().lower() != "auto":
            raise ValueError(f"chunk = {chunk!r}: a ChunkSpec, 'auto' or None")
        chunk = ChunkSpec(auto_frames(int(lens.sum()) if total_frames is None else total_frames))
    elif isinstance(chunk, dict):
        chunk = ChunkSpec(**chunk)
    elif not isinstance(chunk, ChunkSpec):
        raise TypeError(f"chunk = {chunk!r}: a ChunkSpec, 'auto' or None")
    if len(lens) == 0 or int(lens.max()) <= int(chunk.frames):
        return None
    return chunk


def add_cli_arguments(ap) -> None:
    ap.add_argument("--chunk_frames", type=str, default=None, help="cut clips longer than this many frames into chunks that run as "
                    "independent streams ('auto': sized to fill the device); NOT parity with the sequential run; default off")
    ap.add_argument("--chunk_warmup", type=int, default=DEFAULT_WARMUP, help="warm-up frames in front of every chunk")
    ap.add_argument("--chunk_tol", type=float, default=DEFAULT_TOL, help="seam residual (rad / m) above which a chunk is re-run")
    ap.add_argument("--chunk_passes", type=int, default=DEFAULT_PASSES, help="repair passes (0: report only; -1: until no seam is bad)")


def spec_from_args(a):
    """``--chunk_*`` -> ``None`` (off), ``"auto"``-like spec holder or :class:`ChunkSpec`"""
    if a.chunk_frames is None:
        return None
    passes = None if a.chunk_passes < 0 else a.chunk_passes
    if str(a.chunk_frames).strip().lower() == "auto":
        return _Auto(a.chunk_warmup, a.chunk_tol, passes)
    return ChunkSpec(int(a.chunk_frames), a.chunk_warmup, a.chunk_tol, passes)


class _Auto:
    """``"auto"`` with the other three fields given (the CLI)"""

    def __init__(self, warmup, tol, max_passes):
        self.warmup, self.tol, self.max_passes = warmup, tol, max_passes
        ChunkSpec(1, warmup, tol, max_passes)            # (validates)


def resolve_any(chunk, lens, total_frames=None) -> Optional[ChunkSpec]:
    if isinstance(chunk, _Auto):
        lens = np.asarray(lens, dtype=np.int64)
        n = int(lens.sum()) if total_frames is None else int(total_frames)
        chunk = ChunkSpec(auto_frames(n), chunk.warmup, chunk.tol, chunk.max_passes)
    return resolve(chunk, lens, total_frames)


@dataclasses.dataclass
class ChunkPlan:
    chunk: np.ndarray         # i32 [nchunk, 4]: clip, first source frame (warm-up included), warm, owned
    clip_first: np.ndarray    # i32 [nclip + 1]
    Tc: int

    @property
    def nchunk(self) -> int:
        return int(self.chunk.shape[0])


def plan(lens: Sequence[int], frames: int, warmup: int) -> ChunkPlan:
    """``gmr_chunk_plan`` (host code of the library, no GPU needed): two calls, sizing first."""
    from . import _lib
    L = _lib.lib()
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    n, Tc = C.c_int(), C.c_int()
    first = np.zeros(len(lens) + 1, dtype=np.int32)
    _lib.check(L.gmr_chunk_plan(len(lens), _lib._ptr(lens), int(frames), int(warmup), 0, None, None, C.byref(n), C.byref(Tc)))
    table = np.zeros((n.value, 4), dtype=np.int32)
    _lib.check(L.gmr_chunk_plan(len(lens), _lib._ptr(lens), int(frames), int(warmup), n.value, _lib._ptr(table), _lib._ptr(first),
                                C.byref(n), C.byref(Tc)))
    return ChunkPlan(table, first, int(Tc.value))


def over_tol(resid: np.ndarray, tol: float) -> np.ndarray:
    """bool per chunk: a residual component above ``tol`` or not finite"""
    return ~np.all(resid <= tol, axis=-1)


def clip_report(p: ChunkPlan, spec: ChunkSpec, resid0, resid, warm_solves, chunk_status, passes: int) -> List[Dict]:
    """per clip: K, seam_max[3] (after the last pass), seam_max_pass0[3], seams over the tolerance after pass 0, repaired, left bad,
    repair passes of the batch, warm-up solves"""
    bad0, bad = over_tol(resid0, spec.tol), over_tol(resid, spec.tol)
    out = []
    for c in range(len(p.clip_first) - 1):
        a, b = int(p.clip_first[c]), int(p.clip_first[c + 1])
        behind_failed = np.zeros(b - a, dtype=bool)
        behind_failed[1:] = chunk_status[a:b - 1] != 0
        left = bad[a:b] | behind_failed
        smax = lambda r: [float(np.nan if np.isnan(r[a:b, i]).any() else r[a:b, i].max()) for i in range(3)]   # noqa: E731
        out.append({"K": b - a, "seam_max": smax(resid), "seam_max_pass0": smax(resid0), "seams_bad_pass0": int(bad0[a:b].sum()),
                    "seams_repaired": int((bad0[a:b] & ~left).sum()), "seams_left_bad": int(left.sum()), "passes": int(passes),
                    "warm_solves": int(warm_solves[c])})
    return out


def summarize(reports: Sequence[Dict], into: Optional[Dict] = None) -> Dict:
    """totals of per-clip reports (accumulated ``into`` a running summary): what the CLI prints as one line"""
    s = into if into is not None else {}
    for k in ("clips", "clips_split", "chunks", "seams", "seams_bad_pass0", "seams_repaired", "seams_left_bad", "warm_solves"):
        s.setdefault(k, 0)
    s.setdefault("seam_max", [0.0, 0.0, 0.0])
    s.setdefault("passes_max", 0)
    for r in reports:
        s["clips"] += 1
        s["clips_split"] += int(r["K"] > 1)
        s["chunks"] += r["K"]
        s["seams"] += r["K"] - 1
        for k in ("seams_bad_pass0", "seams_repaired", "seams_left_bad", "warm_solves"):
            s[k] += r[k]
        s["seam_max"] = [float(np.nan if (np.isnan(a) or np.isnan(b)) else max(a, b)) for a, b in zip(s["seam_max"], r["seam_max"])]
        s["passes_max"] = max(s["passes_max"], r["passes"])
    return s


# Every chunk starts from qpos0 behind a warm-up and a bad seam is repaired by re-running the chunk from its predecessor's last
# frame: neither the warm-up's first frame nor a seam before its repair carries |theta(t) - theta(t - 1)| <= w, and a repair
# that does may no longer reach the frames the unbounded pass found.  No half version: the two do not go together.
FRAME_LIMIT_REFUSAL = ("chunked retargeting does not carry the frame velocity limit across chunk seams: "
                       "drop chunk= or clear the limit (set_frame_velocity_limit(None))")


# A chunk's warm-up frames and a repaired seam re-run frames of the clip under a chunk-local frame index, and the chunk entry
# points take no weight array: the weights would have to be gathered and re-indexed with the frames.  No half version.
BODY_WEIGHTS_REFUSAL = ("chunked retargeting does not take per-frame body weights: drop chunk= or the weights")


class ChunkRunner:
    """The pass loop on one HIP stream.  Device buffers are grow-only and reused from batch to batch::

        pass 0 : gather(all) -> IK(chunk jobs) -> stitch -> seams -> n_bad            (4 bytes back per job, ONE synchronisation)
        repair : while n_bad and passes < max_passes:
                     gather(bad list, repair mode) -> IK -> stitch(bad list) -> seams -> n_bad

    A repaired chunk starts from its predecessor's current last frame without warm-up, so its residual is exactly 0 until the
    predecessor itself changes; after pass p every chunk with index <= p in its clip is final, so the loop ends after at most
    max K passes.  A repair pass is as long as one chunk whatever the number of bad chunks: passes cost, bad chunks do not."""

    def __init__(self):
        from . import _lib
        self._bufs = _lib.NamedBuffers()
        self._events = None
        self.pass_ms: List[Dict[str, float]] = []      # per pass of the last run: gather / ik / stitch / seams (device events)

    def run(self, launch: Sequence[tuple], lens: Sequence[np.ndarray], specs: Sequence[Optional[ChunkSpec]], flags: int, stream,
            timed: bool = False) -> List[Optional[List[Dict]]]:
        """``launch[i]`` = a :class:`_lib.DevJob` (or the plain tuple of its fields) as :func:`_lib.retarget_group_dev` takes
        them (clip-major device buffers), ``lens[i]`` the host copy of its clip lengths, ``specs[i]`` its
        :class:`ChunkSpec` or ``None`` (that job is launched as it is, in the group of pass 0).  Everything goes to ``stream``;
        returns one list of per-clip reports per job (``None`` for a job without a spec).  ``timed``: record device events
        around the four steps of every pass (``pass_ms``)."""
        from . import _lib
        L = _lib.lib()
        st = _lib._s(stream)
        if timed and self._events is None:
            self._events = [_lib.Event() for _ in range(5)]
        ev = self._events if timed else None
        self.pass_ms = []
        h2d = lambda dst, src: _lib.check(L.gmr_memcpy_h2d(dst.ptr, _lib._ptr(src), src.nbytes, st))     # noqa: E731
        d2h = lambda dst, src, n: _lib.check(L.gmr_memcpy_d2h(_lib._ptr(dst), src.ptr, n, st))            # noqa: E731
        mark = lambda i: ev[i].record(stream) if ev else None                                              # noqa: E731
        launch = [_lib.dev_job(job, i) for i, job in enumerate(launch)]
        jobs = []
        for i, (job, spec) in enumerate(zip(launch, specs)):
            if spec is None:
                continue
            sol, S, T = job.solver, int(job.S), max(int(job.T), 1)
            if np.isfinite(sol.frame_velocity_limit()[0]).any():
                raise ValueError(FRAME_LIMIT_REFUSAL)
            p = plan(np.asarray(lens[i], dtype=np.int32), spec.frames, spec.warmup)
            n, Tc, nq, nh = p.nchunk, p.Tc, sol.nq, sol.nhuman
            j = {"i": i, "src": job, "spec": spec, "plan": p, "S": S, "T": T, "n": n, "sol": sol}
            for name, nbytes in (("chunk", n * 16), ("first", (S + 1) * 4), ("human_c", n * Tc * nh * 56), ("len_c", n * 4),
                                 ("q0_c", n * nq * 8), ("q_out_c", n * Tc * nq * 8), ("nsolve_c", n * Tc * 8), ("status_c", n * 4),
                                 ("chunk_status", n * 4), ("q_seam", n * nq * 8), ("resid", n * 24), ("bad", n * 4), ("nbad", 4),
                                 ("seam_max", S * 24), ("warm", S * 4)):
                j[name] = self._bufs.device(f"{name}_{i}", max(nbytes, 8))
            for name, shape, dt in (("h_nbad", (1,), np.int32), ("h_resid", (n, 3), np.float64), ("h_resid0", (n, 3), np.float64),
                                    ("h_warm", (S,), np.int32), ("h_cst", (n,), np.int32)):
                j[name] = self._bufs.pinned(f"{name}_{i}", shape, dt)
            h2d(j["chunk"], p.chunk)
            h2d(j["first"], p.clip_first)
            jobs.append(j)

        def dims(j):
            return j["S"], j["T"], j["sol"].nq, j["n"], j["plan"].Tc, j["src"]

        def one_pass(active, mode, extra=()):
            mark(0)
            for j in active:
                S, T, nq, n, Tc, src = dims(j)
                lst, nl = (j["bad"].ptr, int(j["h_nbad"][0])) if mode == REPAIR else (None, 0)
                j["slots"] = nl if mode == REPAIR else n
                _lib.check(L.gmr_chunk_gather_dev(S, T, j["sol"].nhuman, nq, n, Tc, j["chunk"].ptr, lst, nl, mode, _lib._d(src.human), _lib._d(src.q0),
                                                  _lib._d(src.q_out), j["human_c"].ptr, j["len_c"].ptr, j["q0_c"].ptr, j["q_seam"].ptr, st))
            mark(1)
            _lib.retarget_group_dev([_lib.DevJob(j["sol"], j["slots"], j["plan"].Tc, j["q0_c"], j["human_c"], j["len_c"], j["q_out_c"],
                                                 j["nsolve_c"], j["status_c"]) for j in active] + list(extra), flags, stream)
            mark(2)
            for j in active:
                S, T, nq, n, Tc, src = dims(j)
                lst, nl = (j["bad"].ptr, j["slots"]) if mode == REPAIR else (None, 0)
                _lib.check(L.gmr_chunk_stitch_dev(S, T, nq, n, Tc, j["chunk"].ptr, j["first"].ptr, lst, nl, mode, j["q_out_c"].ptr,
                                                  j["nsolve_c"].ptr, j["status_c"].ptr, _lib._d(src.q_out), _lib._d(src.nsolve), j["chunk_status"].ptr,
                                                  _lib._d(src.status), j["q_seam"].ptr, j["warm"].ptr, st))
            mark(3)
            for j in active:
                S, T, nq, n, Tc, src = dims(j)
                _lib.check(L.gmr_chunk_seams_dev(S, T, nq, n, Tc, j["chunk"].ptr, j["first"].ptr, _lib._d(src.q_out), j["q_seam"].ptr,
                                                 j["chunk_status"].ptr, float(j["spec"].tol), j["resid"].ptr, j["bad"].ptr, j["nbad"].ptr,
                                                 j["seam_max"].ptr, st))
            mark(4)
            for j in active:
                d2h(j["h_nbad"], j["nbad"], 4)
                d2h(j["h_resid0"] if mode == PASS0 else j["h_resid"], j["resid"], j["n"] * 24)
                d2h(j["h_cst"], j["chunk_status"], j["n"] * 4)
                if mode == PASS0:
                    d2h(j["h_warm"], j["warm"], j["S"] * 4)
            _lib.check(L.gmr_stream_sync(st))                     # the one synchronisation of a pass
            if ev:
                self.pass_ms.append({"slots": sum(j["slots"] for j in active),
                                     **{k: ev[a].elapsed_ms(ev[a + 1]) for a, k in enumerate(("gather", "ik", "stitch", "seams"))}})

        one_pass(jobs, PASS0, [launch[i] for i, s in enumerate(specs) if s is None])
        for j in jobs:
            j["h_resid"][:] = j["h_resid0"]
            j["passes"] = 0
        passes = 0
        while True:
            active = [j for j in jobs if int(j["h_nbad"][0]) > 0 and (j["spec"].max_passes is None or passes < j["spec"].max_passes)
                      and passes <= int(np.diff(j["plan"].clip_first).max())]
            if not active:
                break
            one_pass(active, REPAIR)
            passes += 1
            for j in active:
                j["passes"] = passes
        out: List[Optional[List[Dict]]] = [None] * len(launch)
        for j in jobs:
            out[j["i"]] = clip_report(j["plan"], j["spec"], j["h_resid0"].copy(), j["h_resid"].copy(), j["h_warm"].copy(), j["h_cst"].copy(),
                                      j["passes"])
        return out


def retarget_chunked_host(solver, human: np.ndarray, q0: np.ndarray, lens, flags: int, spec: ChunkSpec, runner: Optional[ChunkRunner] = None,
                          timed: bool = False):
    """Host arrays in and out around :class:`ChunkRunner`: ``human f64[S,T,nhuman,7]``, ``q0 f64[S,nq]`` ->
    ``(q_out[S,T,nq], nsolve[S,T,2], status[S], per-clip reports)``; rows at or beyond a clip's length come back as zeros."""
    from . import _lib
    human = np.ascontiguousarray(human, dtype=np.float64)
    S, T = human.shape[:2]
    if human.ndim != 4 or human.shape[2:] != (solver.nhuman, 7):
        raise ValueError(f"human must be [S,T,{solver.nhuman},7], got {human.shape}")
    q0 = np.ascontiguousarray(np.broadcast_to(q0, (S, solver.nq)), dtype=np.float64)
    lens = np.full(S, T, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    runner = runner if runner is not None else ChunkRunner()
    st = _lib.Stream()
    d_h, d_q0, d_len = (_lib.DeviceBuffer.from_host(a, st) for a in (human, q0, lens))
    d_q, d_ns, d_st = _lib.DeviceBuffer(max(S * T * solver.nq * 8, 8)), _lib.DeviceBuffer(max(S * T * 8, 8)), _lib.DeviceBuffer(max(S * 4, 8))
    for b in (d_q, d_ns, d_st):
        _lib.check(_lib.lib().gmr_memset(b.ptr, 0, b.nbytes, st.ptr))
    reports, = runner.run([_lib.DevJob(solver, S, T, d_q0, d_h, d_len, d_q, d_ns, d_st)], [lens], [spec], flags, st, timed)
    q_out = d_q.to_host((S, T, solver.nq), np.float64, st)
    nsolve = d_ns.to_host((S, T, 2), np.int32, st)
    status = d_st.to_host((S,), np.int32, st)
    for b in (d_h, d_q0, d_len, d_q, d_ns, d_st):
        b.free()
    return q_out, nsolve, status, reports
