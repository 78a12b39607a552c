"""``GeneralMotionRetargeting`` with the reference's constructor / ``retarget()`` surface, backed by
the HIP kernels behind the C-ABI (no CPU fallback: without ``libgmrhip.so`` and a GPU every
numerical entry point raises).

Mirrors reference ``general_motion_retargeting/motion_retarget.py``:

* ``__init__``                      :13-72   (same signature, same public attributes)
* ``update_targets`` / ``retarget`` :117-185 (same in-place ``to_numpy`` mutation of the caller's
  dict, same ``KeyError`` behaviour, returns a fresh float64 ``qpos`` copy)
* ``scaled_human_data``, ``error1`` / ``error2`` :118-124, :188-200 -- served from what the kernel computed for the
  last frame (its ``tgt_out`` / ``err_out``); after ``update_targets()`` alone, from a solve-free launch
* ``scale_human_data`` / ``offset_human_data`` / ``offset_human_data_to_ground`` / ``to_numpy``
  :203-270 (NumPy helpers kept for callers; the retargeting path preprocesses on the device)

plus the batched entry points that the per-frame API cannot express (``retarget_clip``,
``retarget_streams``): many frames / many independent streams per launch, time loop on device.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .ik_config import TaskTables, build_task_tables, pack_model, pack_taskset, scale_rows, velocity_limit_table
from .models import load_ik_config, load_robot
from .params import IK_CONFIG_DICT, ROBOT_XML_DICT


class TargetNotSet(Exception):
    """A frame task has no target (mirrors mink.TargetNotSet for duplicated human bodies)."""


class _Data:
    def __init__(self, qpos):
        self.qpos = qpos


class _Configuration:
    """Minimal stand-in for ``mink.Configuration``: holds ``q`` (``data.qpos``) and the model."""

    def __init__(self, model, q):
        self.model = model
        self.data = _Data(q)

    @property
    def q(self):
        return self.data.qpos.copy()

    def update(self, q=None):
        if q is not None:
            self.data.qpos = np.asarray(q, dtype=np.float64).copy()


def _quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _quat_rotate(q, v):
    qv = np.concatenate([[0.0], v])
    return _quat_mul(_quat_mul(q, qv), q * np.array([1.0, -1.0, -1.0, -1.0]))[1:]


def body_weights_from_missing(human) -> np.ndarray:
    """Body weights ``f64[..., nhuman]`` of packed frames ``human[..., nhuman, 7]``: 1 where all seven entries of a body's row
    are finite, 0 (the body is missing in that frame) where one is not -- what ``retarget_streams(weights=)`` takes for a
    capture with dropouts."""
    human = np.asarray(human, dtype=np.float64)
    if human.ndim < 2 or human.shape[-1] != 7:
        raise ValueError(f"packed frames [..., nhuman, 7] needed, got {human.shape}")
    return np.isfinite(human).all(axis=-1).astype(np.float64)


class GeneralMotionRetargeting:
    """General Motion Retargeting (GMR), MI355X-native backend."""

    def __init__(
        self,
        src_human: str,
        tgt_robot: str,
        actual_human_height: float = None,
        solver: str = "daqp",
        damping: float = 5e-1,
        verbose: bool = False,
        use_velocity_limit: bool = False,
        velocity_limit=None,
        frame_velocity_limit=None,
        fps: Optional[float] = None,
    ) -> None:
        """``use_velocity_limit`` / ``velocity_limit``: per-joint velocity limits in the QP of every solve (upstream's
        ``use_velocity_limit=True`` = ``mink.VelocityLimit`` at 3 pi rad/s on every motor joint); see
        :meth:`set_velocity_limit`.  Off by default.
        ``frame_velocity_limit`` / ``fps``: per-joint velocity limits of the retargeted motion itself, between consecutive
        frames ``1 / fps`` apart; see :meth:`set_frame_velocity_limit`.  Off by default."""
        self.xml_file = str(ROBOT_XML_DICT[tgt_robot])
        if verbose:
            print("Use robot model: ", self.xml_file)
        self.model = load_robot(self.xml_file)

        ik_config_path = IK_CONFIG_DICT[src_human][tgt_robot]
        ik_config = load_ik_config(ik_config_path)
        if verbose:
            print("Use IK config: ", ik_config_path)

        self._ik_config = ik_config       # unscaled: the scale rows of retarget_streams(heights=) come from it
        self._tables: TaskTables = build_task_tables(ik_config, actual_human_height, damping)
        tt = self._tables
        # same public attributes as the reference (:47-59)
        self.ik_match_table1 = ik_config["ik_match_table1"]
        self.ik_match_table2 = ik_config["ik_match_table2"]
        self.human_root_name = tt.human_root_name
        self.robot_root_name = tt.robot_root_name
        self.use_ik_match_table1 = tt.use_stage[0]
        self.use_ik_match_table2 = tt.use_stage[1]
        self.human_scale_table = dict(tt.scale_table)
        self.ground = tt.ground_height * np.array([0, 0, 1])
        self.max_iter = tt.max_iter
        self.solver = solver          # kept for signature compatibility; the device QP is exact
        self.damping = damping
        self.pos_offsets1 = {k: v.copy() for k, v in tt.pos_offsets1.items()}
        self.rot_offsets1 = {k: v.copy() for k, v in tt.rot_offsets1.items()}   # wxyz, normalised
        self._raw_frame = None
        self._scaled_cache = None

        self._human_names: List[str] = tt.human_names
        self._model_blob = pack_model(self.model)
        self._taskset_blob = pack_taskset(self.model, tt)
        self._solver: Optional[_lib.Solver] = None
        self.use_velocity_limit = bool(use_velocity_limit) or velocity_limit is not None
        self._velocity_limit = velocity_limit_table(self.model, use_velocity_limit, velocity_limit)
        self._frame_velocity_limit, self._frame_fps = self._frame_limit_table(frame_velocity_limit, fps)
        self.setup_retarget_configuration()

    # ------------------------------------------------------------------ #
    def setup_retarget_configuration(self):
        """Fresh configuration at ``qpos0`` (reference :74-75); tasks live in the packed task set."""
        self.configuration = _Configuration(self.model, self.model.qpos0.copy())
        self._frames_done = 0         # frames retargeted into the configuration: from the second call on it IS the previous frame

    @property
    def hip_solver(self) -> _lib.Solver:
        if self._solver is None:
            self._solver = _lib.Solver(self._model_blob, self._taskset_blob)   # raises without GPU/library
            if self._velocity_limit is not None:
                self._solver.set_velocity_limit(self._velocity_limit)
            if self._frame_velocity_limit is not None:
                self._solver.set_frame_velocity_limit(self._frame_velocity_limit, 1.0 / self._frame_fps)
        return self._solver

    def set_velocity_limit(self, velocity_limit=None, use_velocity_limit: bool = False) -> None:
        """Per-joint velocity limits for every later call of this object (all entry points: they launch from its solver).
        ``velocity_limit``: a scalar in rad/s for every hinge, an array ``[nhinge]`` in ``model.joint_names`` order, or a
        dict ``{joint name: rad/s}`` (joints not named: none); ``use_velocity_limit=True`` alone: 3 pi on every hinge;
        neither: no limit.  Every solve then keeps ``|dq_h| <= vmax_h * model.timestep`` next to the joint ranges, as
        ``mink.VelocityLimit`` does.  NOTE: that bounds ONE ``solve_ik`` call, as in mink; a frame runs up to 22 solves
        (two stages of ``max_iter + 1``), so a joint may move up to 22 times that far between two frames -- this is not a
        limit on the joint velocity of the retargeted clip (that is :meth:`set_frame_velocity_limit`).  The floating base is
        never bounded."""
        table = velocity_limit_table(self.model, use_velocity_limit, velocity_limit)
        same = (table is None and self._velocity_limit is None) or \
            (table is not None and self._velocity_limit is not None and np.array_equal(table, self._velocity_limit))
        self._velocity_limit = table
        self.use_velocity_limit = table is not None
        if self._solver is not None and not same:
            self._solver.set_velocity_limit(table)

    @property
    def velocity_limit(self) -> Optional[np.ndarray]:
        """The table in force: ``f64[nhinge]`` rad/s (``inf`` = none for that hinge) or None."""
        return None if self._velocity_limit is None else self._velocity_limit.copy()

    def _frame_limit_table(self, limit, fps):
        """(table f64[nhinge] or None, fps or None) of the two arguments; raises before anything reaches the device."""
        table = velocity_limit_table(self.model, False, limit)
        if table is None:
            return None, None
        if fps is None or not (np.isfinite(float(fps)) and float(fps) > 0.0):
            raise ValueError(f"frame_velocity_limit needs fps > 0 (the frames are 1 / fps apart), got fps = {fps!r}")
        return table, float(fps)

    def set_frame_velocity_limit(self, limit=None, fps: Optional[float] = None) -> None:
        """Per-joint velocity limits of the retargeted MOTION, for every later call of this object: every frame keeps
        ``|theta_h(t) - theta_h(t - 1)| <= limit_h / fps`` for every hinge, next to the joint ranges and the per-solve limit of
        :meth:`set_velocity_limit`, inside the QP of every solve -- the other joints compensate for one that saturates, and a
        joint that starts outside its range walks back by ``limit_h / fps`` per frame.  ``limit``: a scalar in rad/s for
        every hinge, an array ``[nhinge]`` in ``model.joint_names`` order, or a dict ``{joint name: rad/s}`` (joints not
        named: none); ``None``: no limit.  ``fps`` is required with a limit.  The first frame after construction or
        :meth:`setup_retarget_configuration` is free (the configuration is ``qpos0`` then, not a pose of the motion); every
        later frame of :meth:`retarget`, :meth:`retarget_packed` and :meth:`retarget_clip` is bounded around the frame
        before it, so a per-frame loop equals one ``retarget_clip`` call.  The floating base is never bounded.  Does not go
        with ``chunk=`` (chunks start from ``qpos0`` and seams are repaired by re-running: a seam would not carry the bound)."""
        table, fps = self._frame_limit_table(limit, fps)
        old = self._frame_velocity_limit
        same = fps == self._frame_fps and ((table is None and old is None) or
                                           (table is not None and old is not None and np.array_equal(table, old)))
        self._frame_velocity_limit, self._frame_fps = table, fps
        if self._solver is not None and not same:
            self._solver.set_frame_velocity_limit(table, 0.0 if table is None else 1.0 / fps)

    @property
    def frame_velocity_limit(self) -> Optional[np.ndarray]:
        """The frame table in force: ``f64[nhinge]`` rad/s (``inf`` = none for that hinge) or None."""
        return None if self._frame_velocity_limit is None else self._frame_velocity_limit.copy()

    def _frame_limit_on(self) -> bool:
        return self._frame_velocity_limit is not None and bool(np.isfinite(self._frame_velocity_limit).any())

    @property
    def human_body_names(self) -> List[str]:
        """Order of the bodies in the packed ``[nhuman, 7]`` frame layout."""
        return list(self._human_names)

    # ------------------------------------------------------------------ #
    # packing of the reference's dict format (App. D) into the C-ABI layout
    # ------------------------------------------------------------------ #
    def body_weight_row(self, body_weights) -> Optional[np.ndarray]:
        """``{body: m}`` (names not given: 1) or an array ``[nhuman]`` as the packed row ``f64[nhuman]`` of one frame's body
        weights; None stays None.  Raises for a name that is no body of the packed layout and for a value that is not finite and
        not negative, before anything reaches the device."""
        if body_weights is None:
            return None
        if isinstance(body_weights, dict):
            row = np.ones(len(self._human_names))
            for n, m in body_weights.items():
                if n not in self._human_names:
                    raise KeyError(n)
                row[self._human_names.index(n)] = float(m)
        else:
            row = np.asarray(body_weights, dtype=np.float64)
        return _lib.check_weights(row[None, None], 1, 1, len(self._human_names), "body_weights")[0, 0]

    def _check_names(self, human_data: Dict, weights: Optional[np.ndarray] = None) -> None:
        """``weights`` (a packed row): a task body with weight 0 may be absent from the frame; the human root may not."""
        tt = self._tables
        if tt.human_root_name not in human_data:
            raise KeyError(tt.human_root_name)
        # bodies that survive scale_human_data must have table-1 offsets (reference :241)
        for n in human_data.keys():
            if n in tt.scale_table and n not in tt.pos_offsets1:
                raise KeyError(n)
        for s in range(2):
            if not tt.use_stage[s]:
                continue
            hs = tt.stages[s].human_names
            if len(set(hs)) != len(hs):
                raise TargetNotSet("two robot frames are mapped to one human body: a task has no target")
            for n in hs:
                if n not in tt.scale_table:
                    raise KeyError(n)
                if n not in human_data and not (weights is not None and weights[self._human_names.index(n)] == 0.0):
                    raise KeyError(n)

    def pack_frame(self, human_data: Dict, weights: Optional[np.ndarray] = None) -> np.ndarray:
        """dict{name: (pos, quat_wxyz)} -> f64[nhuman, 7]; bodies absent from the dict become NaN rows.  ``weights`` (the
        frame's packed body weights): a task body whose weight is 0 may be absent."""
        self._check_names(human_data, weights)
        out = np.full((len(self._human_names), 7), np.nan)
        for i, n in enumerate(self._human_names):
            if n in human_data:
                out[i, :3] = human_data[n][0]
                out[i, 3:] = human_data[n][1]
        return out

    def pack_frames(self, frames: Sequence[Dict], weights: Optional[np.ndarray] = None) -> np.ndarray:
        return np.stack([self.pack_frame(self.to_numpy(f), None if weights is None else weights[i]) for i, f in enumerate(frames)]) \
            if len(frames) else np.zeros((0, len(self._human_names), 7))

    # ------------------------------------------------------------------ #
    # reference API
    # ------------------------------------------------------------------ #
    def update_targets(self, human_data, offset_to_ground=False, body_weights=None):
        human_data = self.to_numpy(human_data)
        w = self.body_weight_row(body_weights)
        self._set_frame(self.pack_frame(human_data, w), offset_to_ground, list(human_data.keys()), w)

    def _set_frame(self, frame, offset_to_ground, key_order=None, weights=None):
        """New targets (a packed frame and, or None, its packed body weights): everything derived from the previous ones is stale."""
        self._raw_frame = frame
        self._raw_weights = weights
        self._ground_flag = bool(offset_to_ground)
        self._key_order = key_order
        self._targets = None          # f64[nhuman, 7]: the kernel's preprocessed frame (tgt_out)
        self._errors = None           # (error1, error2) at self._errors_q
        self._errors_q = None
        self._scaled_cache = None

    def _flags(self, offset_to_ground):
        return _lib.FLAG_OFFSET_TO_GROUND if offset_to_ground else 0

    def _evaluate(self):
        """Targets and residual norms of the current (frame, configuration) WITHOUT a solve: the device runs the
        preprocessing and both tables' residuals (GMR_FLAG_EVAL_ONLY) -- update_targets() followed by
        scaled_human_data / error1() / error2() in the reference (:117-136, :188-200)."""
        if getattr(self, "_raw_frame", None) is None:
            raise TargetNotSet("retarget()/update_targets() has not been called")
        q = self.configuration.data.qpos
        _, _, status, tg, er = self.hip_solver.retarget_streams(
            q[None], self._raw_frame[None, None], flags=self._flags(self._ground_flag) | _lib.FLAG_EVAL_ONLY,
            want_targets=True, want_errors=True, weights=None if self._raw_weights is None else self._raw_weights[None, None])
        if status[0] != 0:
            raise RuntimeError(f"evaluation failed (status {int(status[0])})")
        self._targets, self._errors, self._errors_q = tg[0, 0], er[0, 0], q.copy()
        self._scaled_cache = None

    @property
    def scaled_human_data(self):
        """``{name: [pos, quat_wxyz]}`` after scale / offset / ground (reference :118-124), exactly the values the
        IK kernel computed for the last frame (its ``tgt_out``), in the reference's dict order."""
        if self._scaled_cache is None:
            if getattr(self, "_raw_frame", None) is None:
                return None
            if self._targets is None:
                self._evaluate()
            names = self._human_names
            w = self._raw_weights          # a body missing in this frame (weight 0, not the root) is dropped like an absent one
            rows = {n: self._targets[i] for i, n in enumerate(names) if not np.isnan(self._raw_frame[i, 0])
                    and not (w is not None and w[i] == 0.0 and n != self.human_root_name)}
            order = [self.human_root_name] + [n for n in (self._key_order or names) if n != self.human_root_name]
            self._scaled_cache = {n: [rows[n][:3].copy(), rows[n][3:].copy()] for n in order if n in rows}
        return self._scaled_cache

    @scaled_human_data.setter
    def scaled_human_data(self, value):
        self._scaled_cache = value

    def _run(self, human, offset_to_ground, key_order=None, weights=None):
        """One launch over ``human[T, nhuman, 7]`` (``weights[T, nhuman]``: its body weights, or None) continuing from the
        current configuration; keeps the last frame's targets and residual norms so that scaled_human_data / error1() /
        error2() refer to it."""
        q_out, nsolve, status, tg, er = self.hip_solver.retarget_streams(
            self.configuration.data.qpos[None], human[None],
            flags=self._flags(offset_to_ground) | (_lib.FLAG_FRAME_LIMIT_FIRST if self._frames_done else 0),
            want_targets=True, want_errors=True, weights=None if weights is None else weights[None])
        if status[0] != 0:
            raise RuntimeError(f"IK failed (status {int(status[0])}): QP not solvable / non-finite input")
        self._set_frame(human[-1], offset_to_ground, key_order, None if weights is None else weights[-1])
        self.configuration.data.qpos = q_out[0, -1].copy()
        self._frames_done += human.shape[0]
        self._targets, self._errors, self._errors_q = tg[0, -1], er[0, -1], q_out[0, -1].copy()
        return q_out[0], nsolve[0]

    def retarget(self, human_data, offset_to_ground=False, body_weights=None):
        """One frame (reference :139-185): warm-started from the previous call, returns qpos f64[nq].  ``body_weights``
        ``{body: m}``: a multiplier on the cost of every task bound to that human body in this frame (names not given: 1);
        ``m == 0``: the body is missing -- it may be absent from ``human_data`` or hold anything (the human root is always
        needed), and ``scaled_human_data`` drops it."""
        human_data = self.to_numpy(human_data)
        w = self.body_weight_row(body_weights)
        frame = self.pack_frame(human_data, w)
        q, ns = self._run(frame[None], offset_to_ground, list(human_data.keys()), None if w is None else w[None])
        self.last_num_solves = ns[0].copy()
        return q[0].copy()

    def retarget_packed(self, frame: np.ndarray, offset_to_ground=False, weights=None) -> np.ndarray:
        """:meth:`retarget` for a frame that is already packed (``f64[nhuman, 7]``, rows in
        ``human_body_names`` order, NaN rows = absent bodies): the streaming path (utils/optitrack.py).  ``weights``
        ``f64[nhuman]``: the frame's body weights in the same order (0 = the body is missing, its row may hold anything)."""
        frame = np.ascontiguousarray(frame, dtype=np.float64)
        if frame.shape != (len(self._human_names), 7):
            raise ValueError(f"packed frame must be [{len(self._human_names)}, 7], got {frame.shape}")
        w = self.body_weight_row(weights)
        q, ns = self._run(frame[None], offset_to_ground, None, None if w is None else w[None])
        self.last_num_solves = ns[0].copy()
        return q[0].copy()

    def clip_body_weights(self, body_weights, T: int) -> Optional[np.ndarray]:
        """A clip's body weights -- a sequence of T dicts ``{body: m}`` or an array ``[T, nhuman]`` -- as ``f64[T, nhuman]``;
        None stays None.  Checked before anything reaches the device."""
        if body_weights is None:
            return None
        if not isinstance(body_weights, np.ndarray) and len(body_weights) and isinstance(body_weights[0], dict):
            if len(body_weights) != T:
                raise ValueError(f"body_weights: one dict per frame needed, got {len(body_weights)} for {T} frames")
            return np.stack([self.body_weight_row(w) for w in body_weights])
        return _lib.check_weights(np.asarray(body_weights)[None], 1, T, len(self._human_names), "body_weights")[0]

    def retarget_clip(self, frames, offset_to_ground=False, chunk=None, body_weights=None) -> np.ndarray:
        """All frames of one clip in ONE launch (time loop on device); continues from the current
        configuration exactly like calling :meth:`retarget` per frame.  ``frames`` is a sequence of
        ``human_data`` dicts or an array ``[T, nhuman, 7]``.  Returns ``qpos f64[T, nq]``.
        ``chunk`` (a ``chunking.ChunkSpec`` or ``"auto"``; default off): a clip longer than the spec's ``frames`` runs as
        independent chunks with warm-up -- NOT parity with the per-frame loop; ``self.chunk_report`` says how far off.
        ``chunk`` is refused (``ValueError``) while a finite frame velocity limit is set, and together with ``body_weights``.
        ``body_weights``: a list of T dicts ``{body: m}`` or an array ``[T, nhuman]`` (see :meth:`retarget`)."""
        key_order = None
        weights = self.clip_body_weights(body_weights, len(frames))
        if isinstance(frames, np.ndarray):
            human = np.ascontiguousarray(frames, dtype=np.float64)
        else:
            human = self.pack_frames(frames, weights)
            key_order = list(frames[-1].keys()) if len(frames) else None
        if human.shape[0] == 0:
            return np.zeros((0, self.model.nq))
        from . import chunking
        if chunk is not None and self._frame_limit_on():
            raise ValueError(chunking.FRAME_LIMIT_REFUSAL)
        if chunk is not None and weights is not None:
            raise ValueError(chunking.BODY_WEIGHTS_REFUSAL)
        spec = chunking.resolve_any(chunk, [human.shape[0]])
        self.chunk_report = None
        if spec is not None:
            q, ns, status, self.chunk_report = chunking.retarget_chunked_host(
                self.hip_solver, human[None], self.configuration.data.qpos[None], None, self._flags(offset_to_ground), spec)
            if status[0] != 0:
                raise RuntimeError(f"IK failed (status {int(status[0])}): QP not solvable / non-finite input")
            self._set_frame(human[-1], offset_to_ground, key_order)
            self.configuration.data.qpos = q[0, -1].copy()
            self._frames_done += human.shape[0]
            self._targets, self._errors, self._errors_q = None, None, None      # (evaluated on demand: tgt_out / err_out are not chunked)
            self.last_num_solves = ns[0].copy()
            return q[0]
        q, ns = self._run(human, offset_to_ground, key_order, weights)
        self.last_num_solves = ns.copy()
        return q

    def stream_scales(self, S: int, heights=None, scales=None) -> Optional[np.ndarray]:
        """The per-stream human scale tables ``f64[S, nhuman]`` of ``heights[S]`` (``actual_human_height`` per stream: the
        table of an object built for that height, whatever height THIS object was built for) or of ``scales`` itself; at
        most one of the two, None for neither.  Raises before anything reaches the device."""
        if heights is not None and scales is not None:
            raise ValueError("give heights or scales, not both")
        if heights is not None:
            heights = np.asarray(heights, dtype=np.float64)
            if heights.shape != (S,):
                raise ValueError(f"heights must be [{S}], got {heights.shape}")
            return scale_rows(self._ik_config, heights)
        return _lib.check_scales(scales, S, len(self._human_names))

    def retarget_streams(self, human: np.ndarray, q0: Optional[np.ndarray] = None, lens=None,
                         offset_to_ground=False, heights=None, scales=None, want_targets: bool = False,
                         want_errors: bool = False, q0_is_previous_frame: bool = False, weights=None):
        """Many independent streams ``human[S, T, nhuman, 7]`` (each from ``q0[s]``, default
        ``qpos0`` = a fresh object per clip as the dataset scripts do).  Does not touch this object's
        configuration.  Returns ``(qpos[S, T, nq], nsolve[S, T, 2], status[S])``, with ``want_targets`` /
        ``want_errors`` also ``targets[S, T, nhuman, 7]`` (every frame's ``scaled_human_data``) and ``errors[S, T, 2]``
        (``error1()`` / ``error2()``).  ``heights[S]`` (one ``actual_human_height`` per stream) or ``scales[S, nhuman]``
        (one human scale table per stream: per-subject limb scaling) let subjects of different sizes share this object and
        the launch; stream ``s`` then gets the bits of an object built for ``heights[s]``.
        ``q0_is_previous_frame`` (callers that resume streams): ``q0[s]`` is the pose of the frame before ``human[s, 0]``, so
        the frame velocity limit (:meth:`set_frame_velocity_limit`) bounds frame 0 around it; by default frame 0 is free.
        ``weights[S, T, nhuman]``: a multiplier per (stream, frame, human body) on the cost of every task bound to that body;
        0 = the body is missing in that frame, its ``human`` row may hold anything (NaN included) and its ``targets`` row comes
        back as NaN (:func:`body_weights_from_missing` builds such an array from the NaN rows of ``human``)."""
        S = human.shape[0]
        scales = self.stream_scales(S, heights, scales)
        if q0 is None:
            q0 = np.broadcast_to(self.model.qpos0, (S, self.model.nq)).copy()
        flags = self._flags(offset_to_ground) | (_lib.FLAG_FRAME_LIMIT_FIRST if q0_is_previous_frame else 0)
        return self.hip_solver.retarget_streams(q0, human, lens=lens, flags=flags, scales=scales,
                                                want_targets=want_targets, want_errors=want_errors, weights=weights)

    # ---- errors (reference :188-200): evaluated by the kernel ------------------------------
    def _error(self, stage: int) -> float:
        if getattr(self, "_raw_frame", None) is None:
            raise TargetNotSet("retarget()/update_targets() has not been called")
        if not self._tables.use_stage[stage]:
            raise ValueError("need at least one array to concatenate")    # the reference's empty task list (:190,:197)
        if self._errors is None or not np.array_equal(self._errors_q, self.configuration.data.qpos):
            self._evaluate()
        return float(self._errors[stage])

    def error1(self):
        return self._error(0)

    def error2(self):
        return self._error(1)

    # ---- preprocessing helpers (reference :203-270) ----------------------------------------------
    # Public-by-convention NumPy methods of the reference class, kept for callers that use them directly.  The
    # retargeting path does not: the kernel preprocesses the raw packed frame (and scaled_human_data above is
    # its output).
    def to_numpy(self, human_data):
        for body_name in human_data.keys():
            human_data[body_name] = [np.asarray(human_data[body_name][0]), np.asarray(human_data[body_name][1])]
        return human_data

    def scale_human_data(self, human_data, human_root_name, human_scale_table):
        root_pos, root_quat = human_data[human_root_name]
        scaled_root_pos = human_scale_table[human_root_name] * root_pos
        out = {human_root_name: (scaled_root_pos, root_quat)}
        for name in human_data.keys():
            if name not in human_scale_table or name == human_root_name:
                continue
            local = (human_data[name][0] - root_pos) * human_scale_table[name]
            out[name] = (local + scaled_root_pos, human_data[name][1])
        return out

    def offset_human_data(self, human_data, pos_offsets, rot_offsets):
        """Rotation offset first, then the position offset in the updated local frame."""
        out = {}
        for name in human_data.keys():
            pos, quat = human_data[name]
            q = np.asarray(quat, dtype=np.float64)
            q = q / np.linalg.norm(q)
            qo = np.asarray(rot_offsets[name], dtype=np.float64)
            uq = _quat_mul(q, qo / np.linalg.norm(qo))
            uq = uq / np.linalg.norm(uq)
            out[name] = [pos + _quat_rotate(uq, np.asarray(pos_offsets[name], dtype=np.float64)), uq]
        return out

    def offset_human_data_to_ground(self, human_data):
        ground_offset = self._tables.ground_offset
        lowest = np.inf
        for name in human_data.keys():
            if "Foot" not in name and "foot" not in name:
                continue
            if human_data[name][0][2] < lowest:
                lowest = human_data[name][0][2]
        out = {}
        for name in human_data.keys():
            pos, quat = human_data[name]
            out[name] = [pos - np.array([0, 0, lowest]) + np.array([0, 0, ground_offset]), quat]
        return out
