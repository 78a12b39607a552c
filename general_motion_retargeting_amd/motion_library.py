"""Device-resident motion library: the training-side consumer of the motion pkl files.

What the reference's ``booster_gym/utils/motion_loader.py:100-247`` does per clip and per query in Python -- statistics,
finite-difference velocities, the angular velocity through one pair of scipy ``Rotation`` objects per frame, and
``get_motion_state`` one time at a time -- for MANY clips held in one block of device memory (``csrc/gmr_motion.hip``):
derivatives and statistics are computed by two kernels when the library is filled, and :meth:`MotionLibrary.sample` answers
N ``(clip, time)`` queries in one launch.

* :class:`MotionLibrary` -- the batched interface (``from_motions``, ``from_files``, ``sample``, ``sample_dev``, ``body_state``,
  ``body_state_dev``, ``clip``), and
  with a directory as its argument the reference's class of the same name (``sample_motion``, ``get_motion_names``);
* :class:`MotionLoader` -- the reference's per-file class (attribute and method names kept, NumPy instead of torch), a one-clip
  library underneath.

``ang_vel``: ``"world"`` is the physical world-frame angular velocity; ``"reference"`` reproduces the reference's numbers, whose
``root_ang_vel`` is the log of another rotation (:131-135 reorder the quaternion to wxyz and hand it to a scalar-last
constructor).  The batched interface defaults to the former, :class:`MotionLoader` to the latter.

No GPU framework is imported here: results are NumPy arrays, and :meth:`MotionLibrary.sample_dev` writes into device memory the
caller names -- ``_lib.DeviceBuffer``, a raw address, or anything with ``data_ptr()`` (a tensor of a ROCm build of PyTorch).
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import _dev_ptr  # noqa: F401  (the tracker and callers take it from here)
from .data_loader import motion_arrays

ANGVEL = {"world": 0, "reference": 1}
LOOP = 1
ARRAY_IDS = {"root_pos": 0, "root_rot": 1, "dof_pos": 2, "local_body_pos": 3, "root_vel": 4, "root_ang_vel": 5, "dof_vel": 6,
             "stats": 7, "seg_start": 8, "fps": 9}
STAT_ROWS = ("mean", "std", "min", "max")
SAMPLE_FIELDS = ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel", "local_body_pos")
STATE_FIELDS = SAMPLE_FIELDS[:6]                                        # what body_state shares with sample
BODY_FIELDS = {"body_pos": 3, "body_rot": 4, "body_vel": 3, "body_ang_vel": 3}      # floats per body


class ClipView:
    """One clip of a library on the host: the attributes the reference's ``MotionLoader`` computes when it loads a file."""

    def __init__(self, lib: "MotionLibrary", k: int):
        k = int(k)
        if not 0 <= k < lib.num_clips:
            raise IndexError(f"clip {k} of {lib.num_clips}")
        a, b = int(lib.seg_start[k]), int(lib.seg_start[k + 1])
        self.index = k
        self.fps = lib.fps_list[k]
        self.dt = 1.0 / self.fps
        self.num_frames = b - a
        self.motion_duration = self.num_frames / self.fps
        self.link_body_list = lib.link_body_lists[k]
        for name in ("root_pos", "root_rot", "dof_pos", "root_vel", "root_ang_vel", "dof_vel"):
            setattr(self, name, lib.array(name)[a:b])
        self.local_body_pos = lib.array("local_body_pos")[a:b] if lib.has_local_body_pos else None
        st = lib.array("stats")[k]
        for i, s in enumerate(STAT_ROWS):
            setattr(self, f"root_pos_{s}", st[i, :3])
            setattr(self, f"dof_pos_{s}", st[i, 3:])


class MotionLibrary:
    """Many clips in one block of device memory.

    ``MotionLibrary(motion_dir, motion_files=None)`` loads every ``*.pkl`` of a directory (or the files named), as the reference's
    ``MotionLibrary`` does -- one upload and one fill instead of one loader per file; files that do not load are reported and
    skipped, as there.  :meth:`from_motions` / :meth:`from_files` build one from pkl dicts / paths."""

    def __init__(self, motion_dir: str, device=None, motion_files: Optional[Sequence[str]] = None, ang_vel: str = "world"):
        self.device, self.motion_dir = device, motion_dir
        if motion_files is None:
            motion_files = sorted(f for f in os.listdir(motion_dir) if f.endswith(".pkl"))
        motions, names = [], []
        for f in motion_files:
            try:
                with open(os.path.join(motion_dir, f), "rb") as fh:
                    m = pickle.load(fh)
                motion_arrays(m)
            except Exception as e:  # noqa: BLE001 -- the reference's loop reports and goes on (motion_loader.py:287-293)
                print(f"Failed to load motion {f}: {e}")
                continue
            motions.append(m)
            names.append(os.path.splitext(f)[0])
        if not motions:
            raise ValueError(f"No valid motion files found in {motion_dir}")
        self._build(motions, ang_vel, names)

    # ---- construction -------------------------------------------------------------------------------------------------
    @classmethod
    def from_motions(cls, motions: Sequence[Dict], ang_vel: str = "world", names: Optional[Sequence[str]] = None) -> "MotionLibrary":
        """``motions``: pkl dicts of either variant (ndarray- or list-valued), all of one robot."""
        self = cls.__new__(cls)
        self.device = self.motion_dir = None
        self._build(list(motions), ang_vel, names)
        return self

    @classmethod
    def from_files(cls, paths: Sequence[str], ang_vel: str = "world") -> "MotionLibrary":
        motions = []
        for p in paths:
            with open(p, "rb") as f:
                motions.append(pickle.load(f))
        return cls.from_motions(motions, ang_vel, [os.path.splitext(os.path.basename(p))[0] for p in paths])

    @staticmethod
    def host_inputs(motions: Sequence[Dict]):
        """What a fill reads, from pkl dicts: ``(seg_start i32[C+1], fps f64[C], root_pos f64[B,3], root_rot f64[B,4], dof_pos
        f64[B,ndof], local_body_pos f32[B,nbody,3] or None, link_body_lists)``.  The values are the loader's float32 arrays
        (``data_loader.motion_arrays``), widened: the fill rounds them back to the same float32."""
        if not motions:
            raise ValueError("a motion library needs at least one clip")
        arrs = [motion_arrays(m) for m in motions]
        ndof = {a["dof_pos"].shape[1] if a["dof_pos"].ndim == 2 else -1 for a in arrs}
        if len(ndof) != 1 or -1 in ndof:
            raise ValueError(f"the clips of one library share one robot: dof_pos widths {sorted(ndof)}")
        for i, a in enumerate(arrs):
            n = a["num_frames"]
            if n < 1 or a["root_pos"].shape != (n, 3) or a["root_rot"].shape != (n, 4) or len(a["dof_pos"]) != n:
                raise ValueError(f"clip {i}: root_pos {a['root_pos'].shape}, root_rot {a['root_rot'].shape}, dof_pos {a['dof_pos'].shape}")
        seg = np.concatenate([[0], np.cumsum([a["num_frames"] for a in arrs])]).astype(np.int32)
        fps = np.array([float(a["fps"]) for a in arrs], dtype=np.float64)
        cat = lambda k: np.ascontiguousarray(np.concatenate([a[k] for a in arrs]), dtype=np.float64)   # noqa: E731
        lbp = None
        shapes = {None if a["local_body_pos"] is None else a["local_body_pos"].shape[1:] for a in arrs}
        if len(shapes) == 1 and None not in shapes and all(len(a["local_body_pos"]) == a["num_frames"] for a in arrs):
            lbp = np.ascontiguousarray(np.concatenate([a["local_body_pos"] for a in arrs]), dtype=np.float32).reshape(int(seg[-1]), -1, 3)
        return seg, fps, cat("root_pos"), cat("root_rot"), cat("dof_pos"), lbp, [list(a["link_body_list"]) for a in arrs]

    def _build(self, motions, ang_vel, names):
        seg, fps, rp, rr, dp, lbp, links = self.host_inputs(motions)
        self._create(seg, fps, dp.shape[1], 0 if lbp is None else lbp.shape[1], ang_vel, names, links)
        # ONE upload: the four arrays in one host block (every part starts 256-byte aligned)
        parts = [rp, rr, dp] + ([lbp] if lbp is not None else [])
        offs, total = [], 0
        for a in parts:
            offs.append(total)
            total += _lib.align256(a.nbytes)
        host = np.zeros(max(total, 8), dtype=np.uint8)
        for a, o in zip(parts, offs):
            host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        d = _lib.DeviceBuffer.from_host(host)
        at = lambda i: C.c_void_p(d.ptr.value + offs[i])   # noqa: E731
        self.fill_dev(at(0), at(1), at(2), at(3) if lbp is not None else None)
        _lib.check(_lib.lib().gmr_stream_sync(None))
        d.free()

    def _create(self, seg_start, fps, ndof, nbody, ang_vel, names=None, link_body_lists=None):
        if ang_vel not in ANGVEL:
            raise ValueError(f"ang_vel must be one of {sorted(ANGVEL)}, got {ang_vel!r}")
        _lib.require_gpu()
        self.seg_start = np.ascontiguousarray(seg_start, dtype=np.int32)
        self._fps = np.ascontiguousarray(fps, dtype=np.float64)
        if self.seg_start.ndim != 1 or self._fps.shape != (len(self.seg_start) - 1,):
            raise ValueError("seg_start is [C + 1], fps [C]")
        self.num_clips, self.num_frames = len(self._fps), int(self.seg_start[-1])
        self.ndof, self.nbody, self.ang_vel = int(ndof), int(nbody), ang_vel
        self.fps_list = [float(f) for f in self._fps]
        self.motion_names = list(names) if names is not None else [f"clip{k}" for k in range(self.num_clips)]
        self.link_body_lists = list(link_body_lists) if link_body_lists is not None else [[] for _ in range(self.num_clips)]
        self.has_local_body_pos = False
        self._kinematics = self._fk = None          # attach_kinematics(): the robot body_state() walks
        self._host: Dict[str, np.ndarray] = {}
        self._views: Dict[int, ClipView] = {}
        self._loaders: Dict[str, "MotionLoader"] = {}
        h = C.c_void_p()
        _lib.check(_lib.lib().gmr_motion_lib_create(self.num_clips, self.num_frames, self.ndof, self.nbody, _lib._ptr(self.seg_start),
                                                    _lib._ptr(self._fps), C.byref(h)))
        self.handle = h

    @classmethod
    def from_device(cls, seg_start, fps, ndof: int, nbody: int, d_root_pos, d_root_rot, d_dof_pos, d_local_body_pos=None,
                    ang_vel: str = "world", stream=None, names=None, link_body_lists=None) -> "MotionLibrary":
        """A library filled from float64 arrays that already lie on the device, as ``gmr_postprocess_clips_dev`` leaves them
        (``seg_start`` and ``fps`` are host arrays).  The fill is enqueued on ``stream``; the caller synchronises it before the
        library is sampled from another stream and before the inputs are reused."""
        self = cls.__new__(cls)
        self.device = self.motion_dir = None
        self._create(seg_start, fps, ndof, nbody if d_local_body_pos is not None else 0, ang_vel, names, link_body_lists)
        self.fill_dev(d_root_pos, d_root_rot, d_dof_pos, d_local_body_pos, stream)
        return self

    def fill_dev(self, d_root_pos, d_root_rot, d_dof_pos, d_local_body_pos=None, stream=None) -> None:
        B = self.num_frames
        _lib.check(_lib.lib().gmr_motion_lib_fill_dev(self.handle, _dev_ptr(d_root_pos, "root_pos", "float64", B * 3),
                                                      _dev_ptr(d_root_rot, "root_rot", "float64", B * 4),
                                                      _dev_ptr(d_dof_pos, "dof_pos", "float64", B * self.ndof),
                                                      _dev_ptr(d_local_body_pos, "local_body_pos", "float32", B * self.nbody * 3),
                                                      ANGVEL[self.ang_vel], _lib._s(stream)))
        self.has_local_body_pos = d_local_body_pos is not None and self.nbody > 0
        self._host.clear()
        self._views.clear()

    # ---- the arrays ---------------------------------------------------------------------------------------------------
    def _shape(self, name):
        B, C_ = self.num_frames, self.num_clips
        return {"root_pos": ((B, 3), np.float32), "root_rot": ((B, 4), np.float32), "dof_pos": ((B, self.ndof), np.float32),
                "local_body_pos": ((B, self.nbody, 3), np.float32), "root_vel": ((B, 3), np.float32),
                "root_ang_vel": ((B, 3), np.float32), "dof_vel": ((B, self.ndof), np.float32),
                "stats": ((C_, len(STAT_ROWS), 3 + self.ndof), np.float32), "seg_start": ((C_ + 1,), np.int32),
                "fps": ((C_,), np.float64)}[name]

    def device_array(self, name: str):
        """``(address, bytes)`` of one array of the library on the device"""
        p, n = C.c_void_p(), C.c_size_t()
        _lib.check(_lib.lib().gmr_motion_lib_array(self.handle, ARRAY_IDS[name], C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def array(self, name: str) -> np.ndarray:
        """One array of the library on the host (downloaded on first use; synchronises the device)."""
        a = self._host.get(name)
        if a is None:
            if name == "local_body_pos" and not self.has_local_body_pos:
                raise KeyError("this library holds no local_body_pos")
            shape, dtype = self._shape(name)
            a = np.empty(shape, dtype=dtype)
            addr, nbytes = self.device_array(name)
            assert nbytes == a.nbytes, (name, nbytes, a.nbytes)
            L = _lib.lib()
            _lib.check(L.gmr_stream_sync(None))
            if a.nbytes:
                _lib.check(L.gmr_memcpy_d2h(_lib._ptr(a), C.c_void_p(addr), a.nbytes, None))
                _lib.check(L.gmr_stream_sync(None))
            a.setflags(write=False)
            self._host[name] = a
        return a

    def clip(self, k: int) -> ClipView:
        v = self._views.get(int(k))
        if v is None:
            v = self._views[int(k)] = ClipView(self, k)
        return v

    # ---- sampling -----------------------------------------------------------------------------------------------------
    def sample(self, clip_ids, times, loop: bool = True, local_body_pos: bool = False) -> Dict[str, np.ndarray]:
        """N queries in one launch, host arrays in and out: ``root_pos [N,3]``, ``root_rot [N,4]`` xyzw, ``root_vel``,
        ``root_ang_vel``, ``dof_pos [N,ndof]``, ``dof_vel`` (and ``local_body_pos [N,nbody,3]`` when asked for), plus ``status
        i32[N]``: 1 where the clip id is out of range or the time not finite -- those rows are NaN."""
        times = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        clip_ids = np.ascontiguousarray(np.broadcast_to(np.asarray(clip_ids), times.shape), dtype=np.int32)
        N = len(times)
        if local_body_pos and not self.has_local_body_pos:
            raise KeyError("this library holds no local_body_pos")
        widths = {"root_pos": (3,), "root_rot": (4,), "root_vel": (3,), "root_ang_vel": (3,), "dof_pos": (self.ndof,),
                  "dof_vel": (self.ndof,), "local_body_pos": (self.nbody, 3)}
        out = {k: np.empty((N,) + widths[k], dtype=np.float32) for k in SAMPLE_FIELDS if k != "local_body_pos" or local_body_pos}
        out["status"] = np.zeros(N, dtype=np.int32)
        _lib.check(_lib.lib().gmr_motion_sample(self.handle, N, _lib._ptr(clip_ids), _lib._ptr(times), LOOP if loop else 0,
                                                *[_lib._ptr(out.get(k)) for k in SAMPLE_FIELDS], _lib._ptr(out["status"])))
        return out

    def sample_dev(self, N: int, d_clip, d_time, loop: bool = True, root_pos=None, root_rot=None, root_vel=None, root_ang_vel=None,
                   dof_pos=None, dof_vel=None, local_body_pos=None, status=None, stream=None) -> None:
        """The same on device memory, asynchronous on ``stream``: ``d_clip i32[N]``, ``d_time f64[N]`` and whichever outputs are
        wanted (float32, row-major; ``status`` int32).  Each may be a ``_lib.DeviceBuffer``, a raw address or an object with
        ``data_ptr()``; what such an object says about its dtype, contiguity and size is checked."""
        N = int(N)
        given = dict(root_pos=root_pos, root_rot=root_rot, root_vel=root_vel, root_ang_vel=root_ang_vel, dof_pos=dof_pos,
                     dof_vel=dof_vel, local_body_pos=local_body_pos)
        count = {"root_pos": 3, "root_rot": 4, "root_vel": 3, "root_ang_vel": 3, "dof_pos": self.ndof, "dof_vel": self.ndof,
                 "local_body_pos": self.nbody * 3}
        ptrs = [_dev_ptr(given[k], k, "float32", N * count[k]) for k in SAMPLE_FIELDS]
        _lib.check(_lib.lib().gmr_motion_sample_dev(self.handle, N, _dev_ptr(d_clip, "clip", "int32", N), _dev_ptr(d_time, "time", "float64", N),
                                                    LOOP if loop else 0, *ptrs, _dev_ptr(status, "status", "int32", N), _lib._s(stream)))

    # ---- per-body state --------------------------------------------------------------------------------
    def attach_kinematics(self, kinematics) -> "MotionLibrary":
        """The robot of this library, a ``KinematicsModel`` or an ``_lib.FkHandle``: :meth:`body_state` walks its tree when it is
        not handed one.  A library handed over by the dataset driver has it attached."""
        ndof = kinematics.num_dof if hasattr(kinematics, "body_names") else kinematics.ndof
        if int(ndof) != self.ndof:
            raise ValueError(f"the kinematics has {int(ndof)} dofs, the library {self.ndof}")
        self._kinematics = kinematics
        return self

    def _resolve_kinematics(self, kinematics):
        """``(fk handle, body names or None)`` of ``kinematics`` or of the attached one; the checks that need no device"""
        if self.ang_vel != "world":
            raise ValueError(f'body_state needs a library built with ang_vel="world": the root_ang_vel of ang_vel="{self.ang_vel}" is '
                             "not a physical angular velocity (DESIGN.md section 6h) and cannot be carried through the tree")
        km = self._kinematics if kinematics is None else kinematics
        if km is None:
            raise ValueError("body_state needs the robot: pass kinematics= (a KinematicsModel or an _lib.FkHandle) or call "
                             "attach_kinematics() once")
        names = getattr(km, "body_names", None)
        ndof = km.num_dof if names is not None else km.ndof
        if int(ndof) != self.ndof:
            raise ValueError(f"the kinematics has {int(ndof)} dofs, the library {self.ndof}")
        return km, (list(names) if names is not None else None)

    @staticmethod
    def _body_selection(bodies, names, nbody: int):
        """``bodies`` (``None`` | indices | names) -> ``(i32 array or None, nsel)``"""
        if bodies is None:
            return None, nbody
        sel = []
        for b in bodies:
            if isinstance(b, str):
                if names is None or b not in names:
                    raise KeyError(f"unknown body {b!r}")
                sel.append(names.index(b))
            else:
                sel.append(int(b))
        if not 1 <= len(sel) <= _lib.FK_MAX_BODIES:
            raise ValueError(f"a selection holds 1 to {_lib.FK_MAX_BODIES} bodies, got {len(sel)}")
        for b in sel:
            if not 0 <= b < nbody:
                raise ValueError(f"body {b} outside [0, {nbody})")
        if len(set(sel)) != len(sel):
            raise ValueError("a selection names every body once")
        return np.array(sel, dtype=np.int32), len(sel)

    def _body_state_setup(self, kinematics, bodies):
        km, names = self._resolve_kinematics(kinematics)
        nbody = len(names) if names is not None else km.nbody
        sel, nsel = self._body_selection(bodies, names, nbody)
        fk = km.hip_handle if names is not None else km
        return fk, sel, nsel

    def body_state(self, clip_ids, times, kinematics=None, loop: bool = True, bodies=None, state: bool = True) -> Dict[str, np.ndarray]:
        """N queries in one launch -> world-frame ``body_pos [N,nsel,3]``, ``body_rot [N,nsel,4]`` xyzw, ``body_vel``,
        ``body_ang_vel [N,nsel,3]`` of every body (``bodies=None``) or of the bodies named by index or by name, in that order, plus
        ``status``; with ``state`` also the six arrays of :meth:`sample` (same bits).  The pose is the float32 FK of the sampled
        state, the velocities are the library's ``root_vel / root_ang_vel / dof_vel`` carried through the tree."""
        fk, sel, nsel = self._body_state_setup(kinematics, bodies)
        times = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        clip_ids = np.ascontiguousarray(np.broadcast_to(np.asarray(clip_ids), times.shape), dtype=np.int32)
        N = len(times)
        widths = {"root_pos": (3,), "root_rot": (4,), "root_vel": (3,), "root_ang_vel": (3,), "dof_pos": (self.ndof,), "dof_vel": (self.ndof,)}
        out = {k: np.empty((N,) + widths[k], dtype=np.float32) for k in STATE_FIELDS} if state else {}
        for k, w in BODY_FIELDS.items():
            out[k] = np.empty((N, nsel, w), dtype=np.float32)
        out["status"] = np.zeros(N, dtype=np.int32)
        table = _lib.BodyStateOut(**{k: out[k].ctypes.data for k in out})
        _lib.check(_lib.lib().gmr_motion_body_state(self.handle, fk.handle, N, _lib._ptr(clip_ids), _lib._ptr(times), LOOP if loop else 0,
                                                    _lib._ptr(sel), nsel, C.byref(table)))
        return out

    def body_state_dev(self, N: int, d_clip, d_time, kinematics=None, loop: bool = True, bodies=None, stream=None, **outputs) -> None:
        """The same on device memory, asynchronous on ``stream``: ``outputs`` names whichever of ``root_pos, root_rot, root_vel,
        root_ang_vel, dof_pos, dof_vel, body_pos, body_rot, body_vel, body_ang_vel, status`` are wanted, each a ``_lib.DeviceBuffer``, a
        raw address or an object with ``data_ptr()``, checked as :meth:`sample_dev` checks them."""
        fk, sel, nsel = self._body_state_setup(kinematics, bodies)
        N = int(N)
        rows = _lib.resolve(_lib.BODY_STATE, N=N, R=self.ndof, nsel=nsel)
        table = _lib.device_struct(_lib.BodyStateOut, rows, outputs, "body_state_dev")
        _lib.check(_lib.lib().gmr_motion_body_state_dev(self.handle, fk.handle, N, _dev_ptr(d_clip, "clip", "int32", N),
                                                        _dev_ptr(d_time, "time", "float64", N), LOOP if loop else 0, _lib._ptr(sel), nsel,
                                                        C.byref(table), _lib._s(stream)))

    # ---- the reference's MotionLibrary surface (motion_loader.py:300-312) ----------------------------------------------------
    def sample_motion(self, motion_name: Optional[str] = None) -> "MotionLoader":
        if motion_name is None:
            motion_name = np.random.choice(self.motion_names)
        elif motion_name not in self.motion_names:
            raise ValueError(f"Motion {motion_name} not found in library")
        ld = self._loaders.get(motion_name)
        if ld is None:
            ld = self._loaders[motion_name] = MotionLoader._of(self, self.motion_names.index(motion_name))
        return ld

    def get_motion_names(self) -> List[str]:
        return list(self.motion_names)

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h:
            _lib.lib().gmr_motion_lib_destroy(h)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MotionLoader:
    """The reference's ``MotionLoader`` (motion_loader.py:9-247) on a one-clip :class:`MotionLibrary`: same attribute and method
    names, NumPy arrays where the reference has torch tensors.  ``ang_vel`` defaults to ``"reference"``, so that
    ``root_ang_vel`` has the numbers a policy trained against the reference's loader saw."""

    def __init__(self, motion_file: str, device=None, loop: bool = True, motion_time_offset: float = 0.0, ang_vel: str = "reference"):
        if not os.path.exists(motion_file):
            raise FileNotFoundError(f"Motion file not found: {motion_file}")
        self._init(MotionLibrary.from_files([motion_file], ang_vel), 0, device, loop, motion_time_offset)

    @classmethod
    def _of(cls, library: MotionLibrary, k: int, loop: bool = True, motion_time_offset: float = 0.0) -> "MotionLoader":
        self = cls.__new__(cls)
        self._init(library, k, library.device, loop, motion_time_offset)
        return self

    def _init(self, library, k, device, loop, motion_time_offset):
        self.library, self.clip_index = library, int(k)
        self.device, self.loop, self.motion_time_offset = device, loop, motion_time_offset
        self.current_frame, self.motion_time = 0, 0.0
        v = library.clip(k)
        for name, val in vars(v).items():
            if name != "index":
                setattr(self, name, val)

    def get_motion_state(self, time: float) -> Dict[str, np.ndarray]:
        """root_pos (3,), root_rot xyzw (4,), root_vel, root_ang_vel, dof_pos, dof_vel at ``time + motion_time_offset``."""
        out = self.library.sample([self.clip_index], [time + self.motion_time_offset], self.loop)
        return {k: out[k][0] for k in SAMPLE_FIELDS if k in out}

    def get_motion_length(self) -> float:
        return self.motion_duration

    def reset(self, time_offset: float = 0.0):
        self.motion_time_offset = time_offset
        self.current_frame = 0
        self.motion_time = 0.0
