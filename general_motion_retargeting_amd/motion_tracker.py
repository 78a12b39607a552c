"""Motion tracker: the reference source of an imitation environment, on the device.

What the reference's ``booster_gym/envs/t1_imitation.py`` does per environment and per step in Python -- ``_update_reference_motion``
(:103-200: one ``get_motion_state`` per environment, the map of the motion's dofs onto the robot's, the clock advance),
``_reset_finished_motions`` / ``_reset_idx`` (:201-235) and the six ``_reward_imitation_*`` terms (:249-309) -- for N environments
bound to one :class:`MotionLibrary`: every environment's clip and float32 clock live on the device, and :meth:`MotionTracker.step`
is ONE kernel launch (``csrc/gmr_tracker.hip``).  Random draws are counter-based (Philox4x32-10 keyed by the seed, counter =
environment and draw number), so a run is reproducible whatever the number of environments around it.  :meth:`MotionTracker.preview` is
the observation half: the reference at every environment's clock plus a few offsets, packed as observation rows in
one launch (``csrc/gmr_tracker_preview.hip``) that moves no clock.  :meth:`MotionTracker.reset_done` resets from done / failed masks in one
launch and :meth:`MotionTracker.set_adaptive` draws episode starts where episodes recently failed (DESIGN.md section 6n,
``csrc/gmr_tracker_adaptive.hip``).  :meth:`MotionTracker.set_anchor` and :meth:`MotionTracker.anchor_to_root` place the reference of every
environment in the simulator's world: a yaw and a translation per environment that every world-frame output goes through (DESIGN.md
section 6o, ``csrc/gmr_tracker_anchor.hip``).  :meth:`MotionTracker.targets` and :meth:`MotionTracker.torques` are the control half of the step
(``csrc/gmr_tracker_control.hip``): the PD targets -- the reference's joint row eased in from the default pose, plus
the clipped action -- in one launch, and the actuator model in one launch per physics substep.  :meth:`MotionTracker.proprio` is what
follows the physics (``csrc/gmr_tracker_proprio.hip``): the body-frame base state, the proprioceptive observation row
with sensor noise, the regularisation penalties, the state-based termination and the roll-over of the ``last_*`` arrays, in one launch.
:meth:`MotionTracker.set_terrain`, :meth:`MotionTracker.terrain_heights` and :meth:`MotionTracker.feet` close the step (DESIGN.md section 6r,
``csrc/gmr_tracker_feet.hip``): the bilinear terrain height the reference interpolates on the host, the feet pose and edge contacts, the gait
clock, the contact-force termination, ``collision`` and the seven ``feet_*`` terms, in one launch.  :meth:`MotionTracker.commands` and
:meth:`MotionTracker.disturb` take what was left of the step (``csrc/gmr_tracker_commands.hip``): the velocity commands
with their resampling and curriculum, the command-tracking terms, and the kicks and pushes.  On the learner's side
:meth:`MotionTracker.record` / :meth:`MotionTracker.advantages` (6u), :meth:`MotionTracker.loss` (6v) and
:meth:`MotionTracker.optimizer_step` (6x, ``csrc/gmr_tracker_optim.hip``: the clip of the gradient norm and the Adam step in three
launches) leave the networks and their backward pass as the only part of a training iteration that is not a call of this class.
:meth:`MotionTracker.act` and :meth:`MotionTracker.values` (6z, ``csrc/gmr_tracker_policy.hip``) are the forward pass of those networks
without autograd -- the ELU MLPs of the reference's ``model.py`` on the FP32 matrix instructions, one launch each, with the sampled action.

No GPU framework is imported here: :meth:`MotionTracker.step` takes and returns NumPy arrays, :meth:`MotionTracker.step_dev` reads
and writes device memory the caller names -- ``_lib.DeviceBuffer``, a raw address, or anything with ``data_ptr()``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (CMD_BOUNDARY, CMD_INDEX_ORDERS, CMD_MAX_LEVELS, CMD_RESAMPLED, CMD_SUCCESS, CMD_TERMS, CONTROL_MAX_DECIMATION, DISTURB_KICK,  # noqa: F401
                   DISTURB_PUSH_START, DISTURB_PUSH_STOP, DISTURB_SPECS, FEET_DONE_CONTACT, FEET_MAX_BODIES, FEET_MAX_EDGES, FEET_TERMS,
                   NOISE_DISTRIBUTIONS, NOISE_OPERATIONS, PREVIEW_MAX_BODIES, PREVIEW_MAX_OFFSETS, PROPRIO_MAX_EXTRA, PROPRIO_NOISE_BLOCKS,
                   PROPRIO_TERMS, RESET_SPECS, REWARD_BLOCKS, REWARD_IMITATION, REWARD_LOCOMOTION, REWARD_MAX_EXTRA, _dev_ptr)
from .motion_library import LOOP, MotionLibrary

# what the library's ABI fixes -- term names in column order, limits, flag bits -- is defined once, in _lib.py, and bound here under the same name
TERMS = ("root_pos", "root_rot", "root_vel", "root_ang_vel", "dof_pos", "dof_vel")
DEFAULT_SCALES = (0.5, 0.5, 2.0, 1.0, 1.0, 0.1)           # T1Imitation.yaml:327-332
MAX_DOF = _lib.TRACKER_MAX_DOF
LINK_TERMS = ("link_pos", "link_rot", "link_vel", "link_ang_vel")
DEFAULT_LINK_SCALES = (0.3, 0.8, 2.0, 4.0)               # m, rad, m/s, rad/s: a choice of this library, the reference has no link terms
FRAMES = {"world": 0, "heading": 1}
PREVIEW_BLOCKS = tuple(_lib.PREVIEW_BLOCKS)               # row order
PREVIEW_SAMPLER_BLOCKS = ("root_pos", "root_quat", "root_vel", "root_ang_vel", "dof_pos", "dof_vel")
PREVIEW_FRAMES = {"raw": 0, "reference": 1, "sim": 2}
ADAPTIVE_MAX_BINS, ADAPTIVE_MAX_LOOKAHEAD = 1 << 22, 16
# failure-driven start sampling: a choice of this library, the reference starts every motion at time 0
DEFAULT_ADAPTIVE = {"bin_seconds": 1.0, "alpha": 0.1, "uniform": 0.3, "lookahead": 4, "gamma": 0.8}
# t1_imitation.py:388, :414: two seconds of start-up, the action gain during it and afterwards
DEFAULT_CONTROL = {"startup_seconds": 2.0, "gain_startup": 0.1, "gain_run": 0.2}
PROPRIO_NORMALIZATION = ("gravity", "lin_vel", "ang_vel", "dof_pos", "dof_vel")
PROPRIO_STATE = ("filtered_lin_vel", "filtered_ang_vel", "last_root_vel", "last_actions", "last_dof_vel", "noise_tick")
FEET_STATE = ("last_feet_pos", "gait_process")
DEFAULT_FEET = {"force_threshold": 1.0, "contact_clearance": 0.01}          # t1.py:553, :629 and :545
COMMAND_STATE = ("commands", "gait_frequency", "cmd_resample_time", "cmd_draws", "env_level", "curriculum_prob", "hits", "cum")
LINK_SIM = {"body_pos": (0, 3), "body_rot": (3, 4), "body_vel": (7, 3), "body_ang_vel": (10, 3)}      # offset and width in a packed row of 13


def _dof_tables(ndof: int, dof_map, dof_default, dof_weight):
    """``(R, map i32[R] or None, default f32[R] or None, weight f32[R] or None)``, checked as the library checks them"""
    m = None if dof_map is None else np.ascontiguousarray(dof_map, dtype=np.int32).reshape(-1)
    R = ndof if m is None else len(m)
    if not 1 <= R <= MAX_DOF:
        raise ValueError(f"a tracker serves 1 to {MAX_DOF} robot dofs, got {R}")
    if m is not None and ((m < -1) | (m >= ndof)).any():
        raise ValueError(f"dof_map entries lie in [-1, {ndof}): {m.tolist()}")
    out = [R, m]
    for name, a in (("dof_default", dof_default), ("dof_weight", dof_weight)):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
            if len(a) != R:
                raise ValueError(f"{name} has {len(a)} entries, the robot {R} dofs")
            if not np.isfinite(a).all():
                raise ValueError(f"{name} is not finite")
        out.append(a)
    return tuple(out)


def _clip_weights(num_clips: int, clip_weights):
    if clip_weights is None:
        return None
    w = np.ascontiguousarray(clip_weights, dtype=np.float64).reshape(-1)
    if len(w) != num_clips:
        raise ValueError(f"clip_weights has {len(w)} entries, the library {num_clips} clips")
    if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("clip_weights must be finite, not negative and not all zero")
    return w


def _adaptive_bins(seg_start, fps, bin_seconds: float):
    """``(bin_start i32[C + 1], frames i64[C])`` of the library under ``bin_seconds``: ``F_c = max(1, round-half-away(bin_seconds fps_c))``
    frames per bin and ``ceil(T_c / F_c)`` bins per clip, as ``gmr_motion_tracker_set_adaptive`` builds them"""
    seg = np.asarray(seg_start, dtype=np.int64)
    T = np.diff(seg)
    f = np.minimum(float(bin_seconds) * np.asarray(fps, dtype=np.float64), 2147483647.0)
    whole = np.floor(f)
    F = np.maximum((whole + (f - whole >= 0.5)).astype(np.int64), 1)
    nb = -(-T // F)
    return np.concatenate([[0], np.cumsum(nb)]), F


def _mask(a, what: str, n: int):
    """a done / failed mask of ``n`` entries as ``i32[n]`` (bool or integer in), or None"""
    if a is None:
        return None
    a = np.asarray(a)
    if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{what}: a mask is bool or integer, got {a.dtype}")
    if a.shape != (n,):
        raise ValueError(f"{what}: shape {a.shape}, {(n,)} needed")
    return np.ascontiguousarray(a != 0, dtype=np.int32)


def _terms(scales, weights, names=TERMS, default_scales=DEFAULT_SCALES):
    out = []
    for name, a, positive in (("scales", scales, True), ("weights", weights, False)):
        if a is not None:
            if isinstance(a, dict):
                unknown = sorted(set(a) - set(names))
                if unknown:
                    raise KeyError(f"{name}: unknown terms {unknown} (known: {list(names)})")
                base = default_scales if positive else (1.0,) * len(names)
                a = [a.get(k, b) for k, b in zip(names, base)]
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
            if len(a) != len(names):
                raise ValueError(f"{name} has {len(a)} entries, there are {len(names)} terms: {list(names)}")
            if not np.isfinite(a).all() or (positive and not (a > 0).all()):
                raise ValueError(f"{name} must be finite" + (" and positive" if positive else ""))
        out.append(a)
    return out


class MotionTracker:
    """``num_envs`` environments on one library.  ``dof_map[j]`` is the library column robot dof ``j`` follows, or -1 for
    ``dof_default[j]`` at velocity zero (identity by default); ``dof_weight`` weighs the dofs inside the two dof terms (ones: the
    reference's formula); ``scales`` / ``weights`` are six numbers or a dict over :data:`TERMS`; ``clip_weights`` bias the random
    choice of a clip.  A new tracker has every environment on clip 0 at time 0: call :meth:`reset` or :meth:`assign`.

    A tracker is single-stream: its ``*_dev`` calls go to one stream, or the caller orders them."""

    def __init__(self, library: MotionLibrary, num_envs: int, dt: float, dof_map=None, dof_default=None, dof_weight=None, loop: bool = True,
                 scales=None, weights=None, clip_weights=None, seed: int = 0):
        self._init_state(library, num_envs)
        self.dt, self.loop, self.seed = float(dt), bool(loop), int(seed)
        if self.num_envs < 1:
            raise ValueError(f"num_envs = {num_envs}")
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed is a 64-bit unsigned number")
        R, m, d, w = _dof_tables(library.ndof, dof_map, dof_default, dof_weight)
        cw = _clip_weights(library.num_clips, clip_weights)
        sc, wt = _terms(scales, weights)
        _lib.require_gpu()
        h = C.c_void_p()
        _lib.check(_lib.lib().gmr_motion_tracker_create(library.handle, self.num_envs, self.dt, LOOP if loop else 0, R, _lib._ptr(m), _lib._ptr(d),
                                                        _lib._ptr(w), _lib._ptr(cw), self.seed, C.byref(h)))
        self.handle, self.nrobot_dof = h, R
        if sc is not None or wt is not None:
            self.set_terms(sc, wt)

    # The private state of a tracker on which nothing is configured yet, stated once: a ``set_*`` call replaces an entry on the instance.
    _links = None            # (fk, nsel, sim_body, frame) once set_links has attached a selection
    _preview = None          # (K, blocks in row order, frame, nsel) once set_preview has configured one
    _adaptive = None         # (bin_seconds, bin_start i64[C + 1]) once set_adaptive has built the bins
    _anchors = False         # whether the per-environment anchors are enabled
    _control = None          # (R, decimation) once set_control has configured the control half
    _proprio = None          # (R, extra_cols) once set_proprio has configured the proprioception half
    _feet = None             # (num_bodies, num_edges) once set_feet has configured the feet
    _commands = None         # ((L, A) or None,) once set_commands has configured the velocity commands
    _resets = None           # (R, decimation) once set_reset_states has configured the reset states
    _rewards = None          # the checked configuration once set_rewards has laid the reward columns out
    _rollout = None          # the checked configuration once set_rollout has configured the rollout
    _loss = None             # the checked configuration, with its rows and columns, once set_loss has configured the loss head
    _optim = None            # the checked configuration (sizes, rate or None: follow, betas, eps, max_norm) once set_optimizer has run
    _policy = None           # the checked shapes of the two networks and the sizes of their parameter list once set_policy has run
    _backward = None         # max_rows and the policy configuration it was planned for once set_backward has run
    _disturb = None          # (kick_every, push_every, push_duration) once set_disturbances has configured kicks and pushes

    def _init_state(self, library, num_envs, nrobot_dof=None) -> None:
        """What a tracker holds before a handle exists, beside the class's "nothing configured" entries above: needs no device"""
        self.library, self.num_envs, self.nrobot_dof, self.handle = library, int(num_envs), nrobot_dof, None

    def _rows_of(self, table, **dims):
        """the arrays of a table of ``_lib.py`` as ``{name: (dtype, shape, count)}`` under ``N = num_envs`` and ``dims``"""
        return _lib.resolved(table, N=self.num_envs, **dims)

    def _subset(self, what: str, env_ids, mask=None, n=None, device: bool = False, once: bool = True, all_envs: str = "every environment is served"):
        """``env_ids`` / ``mask`` / ``n`` of a call that serves a listed subset -> ``(n, ids, mask)``: host arrays ``i32[n]`` or ``None``
        (``once``: a list that names an environment twice is refused), or -- ``device`` -- device addresses, where a list needs ``n``"""
        if device:
            if env_ids is None:
                if n is not None and int(n) != self.num_envs:
                    raise ValueError(f"{what}: without env_ids {all_envs}: n = {n}, num_envs = {self.num_envs}")
                n = self.num_envs
            elif n is None or int(n) < 0:
                raise ValueError(f"{what}: env_ids on the device needs n, the length of the list")
            n = int(n)
            return n, _dev_ptr(env_ids, "env_ids", "int32", n), _dev_ptr(mask, "mask", "int32", n)
        ids, n = None, self.num_envs
        if env_ids is not None:
            ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
            n = len(ids)
            if once and len(np.unique(ids)) != n:
                raise ValueError(f"{what}: env_ids names an environment twice")
        return n, ids, _mask(mask, "mask", n)

    def _bodies(self, bodies, names, width: int, nb=None, reach=None, device: bool = False):
        """The simulator's rigid bodies as a ``gmr_tracker_links_sim_t`` -> ``(struct, arrays to keep alive)``.  ``bodies`` is
        ``{"body_state": the packed [N, nb, 13] tensor}`` -- the fields ``names`` become offsets into it, with its two strides; ``nb=None``
        reads the count off a host array; ``reach``, the largest body index that will be read, must lie inside -- or ``{name: [N, width, k]}``,
        the separate arrays."""
        N = self.num_envs
        if "body_state" not in bodies:
            rows = self._rows_of(_lib.TRACKER_LINKS_SIM, nsel=width)
            return (_lib.device_struct(_lib.TrackerLinksSim, rows, bodies), []) if device else _lib.host_inputs(_lib.TrackerLinksSim, rows, bodies)
        a = bodies["body_state"]
        if not device:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 3 or a.shape[0] != N or a.shape[2] != 13 or nb not in (None, a.shape[1]):
                raise ValueError(f"body_state: shape {a.shape}, ({N}, {'nb' if nb is None else nb}, 13) needed")
            nb = a.shape[1]
        if reach is not None and reach >= nb:
            raise ValueError(f"sim_bodies reaches body {reach}, body_state has {nb}")
        base = _dev_ptr(a, "body_state", "float32", N * nb * 13).value if device else a.ctypes.data
        ls = _lib.TrackerLinksSim(env_stride=13 * nb, body_stride=13)
        for k in names:
            setattr(ls, k, base + 4 * LINK_SIM[k][0])
        return ls, [a]

    # ---- tables ---------------------------------------------------------------------------------------------------------
    def set_dof_map(self, dof_map=None, dof_default=None, dof_weight=None) -> None:
        """Replaces the three dof tables (a curriculum changes them between stages); steps already enqueued keep theirs."""
        R, m, d, w = _dof_tables(self.library.ndof, dof_map, dof_default, dof_weight)
        _lib.check(_lib.lib().gmr_motion_tracker_set_dof_map(self.handle, R, _lib._ptr(m), _lib._ptr(d), _lib._ptr(w)))
        self.nrobot_dof = R

    def set_terms(self, scales=None, weights=None) -> None:
        """``term = exp(-err / scale)``, ``total = sum of weight * term`` over the terms whose weight is not zero; what is ``None``
        is kept."""
        sc, wt = _terms(scales, weights)
        _lib.check(_lib.lib().gmr_motion_tracker_set_terms(self.handle, _lib._ptr(sc), _lib._ptr(wt)))

    # ---- clip assignment and clocks ---------------------------------------------------------------------------------------
    def reset(self, env_ids=None, resample: bool = True, time_offset_range: Sequence[float] = (0.0, 0.0)) -> int:
        """``_reset_idx`` (:215-235) for ``env_ids`` (all by default): a new clip when ``resample``, and the clock at a uniformly
        random point of ``time_offset_range``.  Returns how many ids lay outside ``[0, num_envs)`` (they are ignored)."""
        lo, hi = (float(x) for x in time_offset_range)
        ids, n = None, 0
        if env_ids is not None:
            ids = np.unique(np.asarray(env_ids, dtype=np.int32).reshape(-1))        # every environment once
            n = len(ids)
            if n == 0:
                return 0
        ignored = C.c_int()
        _lib.check(_lib.lib().gmr_motion_tracker_reset(self.handle, n, _lib._ptr(ids), 1 if resample else 0, lo, hi, C.byref(ignored)))
        return int(ignored.value)

    def assign(self, clip_ids, times, env_ids=None) -> int:
        """Sets ``(clip, time)`` of ``env_ids`` (all, in order, by default) explicitly; returns the number of ignored ids."""
        n = self.num_envs if env_ids is None else int(np.size(env_ids))
        ids = None if env_ids is None else np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
        clip = np.ascontiguousarray(np.broadcast_to(np.asarray(clip_ids, dtype=np.int32), (n,)))
        time = np.ascontiguousarray(np.broadcast_to(np.asarray(times, dtype=np.float32), (n,)))
        ignored = C.c_int()
        _lib.check(_lib.lib().gmr_motion_tracker_assign(self.handle, n, _lib._ptr(ids), _lib._ptr(clip), _lib._ptr(time), C.byref(ignored)))
        return int(ignored.value)

    def reset_dev(self, n: int = 0, d_env_ids=None, resample: bool = True, time_offset_range: Sequence[float] = (0.0, 0.0), stream=None) -> None:
        """:meth:`reset` with the ids (``i32[n]``, every environment once) on the device, asynchronous on ``stream``.  A list that names
        an environment twice gives that environment one of two outcomes (one draw or two) and touches no other; the masked form,
        :meth:`reset_done_dev`, takes the flags themselves and cannot have that problem."""
        lo, hi = (float(x) for x in time_offset_range)
        _lib.check(_lib.lib().gmr_motion_tracker_reset_dev(self.handle, int(n), _dev_ptr(d_env_ids, "env_ids", "int32", int(n)),
                                                           1 if resample else 0, lo, hi, _lib._s(stream)))

    def assign_dev(self, n: int, d_clip, d_time, d_env_ids=None, stream=None) -> None:
        """:meth:`assign` on device memory (``clip i32[n]``, ``time f32[n]``, ``env_ids i32[n]`` or None with n = num_envs)"""
        n = int(n)
        _lib.check(_lib.lib().gmr_motion_tracker_assign_dev(self.handle, n, _dev_ptr(d_env_ids, "env_ids", "int32", n),
                                                            _dev_ptr(d_clip, "clip", "int32", n), _dev_ptr(d_time, "time", "float32", n),
                                                            _lib._s(stream)))

    def state(self) -> Dict[str, np.ndarray]:
        """``clip i32[N]``, ``time f32[N]``, ``length f32[N]``, ``draws u32[N]``, ``ignored``, the ids outside ``[0, N)`` met so far, and
        ``adaptive``: whether :meth:`set_adaptive` has bins in place"""
        N = self.num_envs
        out = {"clip": np.empty(N, np.int32), "time": np.empty(N, np.float32), "length": np.empty(N, np.float32), "draws": np.empty(N, np.uint32)}
        ign = C.c_uint32()
        _lib.check(_lib.lib().gmr_motion_tracker_state(self.handle, *[_lib._ptr(out[k]) for k in ("clip", "time", "length", "draws")], C.byref(ign)))
        out["ignored"] = int(ign.value)
        out["adaptive"] = self._adaptive is not None
        return out

    # ---- adaptive sampling and masked resets ---------------------------------------------------------
    def _adaptive_setup(self, bin_seconds, alpha, uniform, lookahead, gamma):
        """the checks of :meth:`set_adaptive`, all of them before a device is touched -> ``(bin_seconds, alpha, uniform, K, gamma,
        bin_start)``"""
        bin_seconds, alpha, uniform, gamma = float(bin_seconds), float(alpha), float(uniform), float(gamma)
        if not np.isfinite(bin_seconds) or not bin_seconds > 0:
            raise ValueError(f"bin_seconds = {bin_seconds}, must be positive and finite (None turns adaptive sampling off)")
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"alpha = {alpha} outside [0, 1]")
        if not 0.0 <= uniform <= 1.0:
            raise ValueError(f"uniform = {uniform} outside [0, 1]")
        if int(lookahead) != lookahead or not 1 <= int(lookahead) <= ADAPTIVE_MAX_LOOKAHEAD:
            raise ValueError(f"lookahead = {lookahead} outside 1 to {ADAPTIVE_MAX_LOOKAHEAD} bins")
        if not 0.0 < gamma <= 1.0:
            raise ValueError(f"gamma = {gamma} outside (0, 1]")
        bin_start, _ = _adaptive_bins(self.library.seg_start, self.library._fps, bin_seconds)
        if not 1 <= int(bin_start[-1]) <= ADAPTIVE_MAX_BINS:
            raise ValueError(f"bin_seconds = {bin_seconds} cuts the library into {int(bin_start[-1])} bins, 1 to {ADAPTIVE_MAX_BINS} are served")
        return bin_seconds, alpha, uniform, int(lookahead), gamma, bin_start

    def set_adaptive(self, bin_seconds: Optional[float] = DEFAULT_ADAPTIVE["bin_seconds"], alpha: float = DEFAULT_ADAPTIVE["alpha"],
                     uniform: float = DEFAULT_ADAPTIVE["uniform"], lookahead: int = DEFAULT_ADAPTIVE["lookahead"],
                     gamma: float = DEFAULT_ADAPTIVE["gamma"]) -> None:
        """Failure-driven start sampling.  Every clip is cut into bins of ``bin_seconds``; :meth:`reset_done` counts the failures per
        bin, :meth:`adapt` folds the counts into a history (``ema = (1 - alpha) ema + alpha count``) and turns it into start
        probabilities: a failure raises its own bin and, discounted by ``gamma`` per bin, the ``lookahead - 1`` bins in front of it
        inside its clip, and ``uniform`` is the share that stays "clip by weight, start uniform over the clip".  A fresh configuration
        draws from that base distribution.  The same ``bin_seconds`` again replaces the four parameters and keeps the history;
        ``bin_seconds=None`` (or ``<= 0``) turns adaptive sampling off.  From then on :meth:`reset_done` and the redraw of a finished clip
        (``loop=False``) take clip and start time from the bins; :meth:`reset` and :meth:`assign` do not change.  The defaults
        (:data:`DEFAULT_ADAPTIVE`) are a choice of this library."""
        if bin_seconds is None or (np.isfinite(float(bin_seconds)) and float(bin_seconds) <= 0):
            _lib.check(_lib.lib().gmr_motion_tracker_set_adaptive(self.handle, 0.0, 0.0, 1.0, 1, 1.0))
            self._adaptive = None
            return
        bin_seconds, alpha, uniform, K, gamma, bin_start = self._adaptive_setup(bin_seconds, alpha, uniform, lookahead, gamma)
        _lib.check(_lib.lib().gmr_motion_tracker_set_adaptive(self.handle, bin_seconds, alpha, uniform, K, gamma))
        self._adaptive = (bin_seconds, bin_start)

    def _need_adaptive(self, what: str):
        if self._adaptive is None:
            raise ValueError(f"{what}: adaptive sampling is not configured, call set_adaptive() first")
        return self._adaptive

    def adapt(self) -> None:
        """One Adapt (typically once per rollout): the failure counts enter the history and are cleared, the start probabilities and
        their CDF are rebuilt.  Synchronous."""
        self._need_adaptive("adapt")
        _lib.check(_lib.lib().gmr_motion_tracker_adapt(self.handle))

    def adapt_dev(self, stream=None) -> None:
        """:meth:`adapt`, asynchronous on ``stream`` (three launches)"""
        self._need_adaptive("adapt_dev")
        _lib.check(_lib.lib().gmr_motion_tracker_adapt_dev(self.handle, _lib._s(stream)))

    def _check_reset_done(self, what: str, resample: bool, time_offset_range):
        lo, hi = (float(x) for x in time_offset_range)
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"{what}: time_offset_range {(lo, hi)} is not finite")
        if self._adaptive is not None and (not resample or lo != 0.0 or hi != 0.0):
            raise ValueError(f"{what}: an adaptive tracker draws clip and start time from its bins, so resample=True and "
                             f"time_offset_range=(0, 0) are the only choice (got {resample}, {(lo, hi)}); reset() serves a range")
        return lo, hi

    def reset_done(self, done=None, failed=None, env_ids=None, resample: bool = True, time_offset_range: Sequence[float] = (0.0, 0.0)) -> int:
        """The masked reset, host arrays in.  Without ``env_ids``: environment ``e`` is reset iff ``done[e]`` (``[N]``, bool or integer;
        ``None``: every one).  With ``env_ids`` (every environment at most once): the listed ones, ``done`` / ``failed`` indexed by list
        position.  On a plain tracker a done environment gets what :meth:`reset` gives it, bit for bit, and one that is not done consumes
        no draw.  On an adaptive tracker the bin of every done environment with ``failed`` set is counted first -- at the clock it has
        now -- and clip and start time come from the bins.  Returns how many ids of done entries lay outside ``[0, num_envs)``."""
        lo, hi = self._check_reset_done("reset_done", resample, time_offset_range)
        n, ids, _ = self._subset("reset_done", env_ids)
        d, f = _mask(done, "done", n), _mask(failed, "failed", n)
        if n == 0:
            return 0
        ignored = C.c_int()
        _lib.check(_lib.lib().gmr_motion_tracker_reset_done(self.handle, n, _lib._ptr(ids), _lib._ptr(d), _lib._ptr(f), 1 if resample else 0, lo, hi,
                                                            C.byref(ignored)))
        return int(ignored.value)

    def reset_done_dev(self, done=None, failed=None, env_ids=None, n: Optional[int] = None, resample: bool = True,
                       time_offset_range: Sequence[float] = (0.0, 0.0), stream=None) -> None:
        """:meth:`reset_done` on device memory, asynchronous on ``stream``: ONE launch, no allocation, no synchronisation, no
        read-back.  ``done`` / ``failed`` are ``i32`` masks as a step leaves them (``finished``, ``fail``) or as the simulator keeps them;
        with ``env_ids`` (``i32[n]``) they are indexed by list position and ``n`` is mandatory."""
        lo, hi = self._check_reset_done("reset_done_dev", resample, time_offset_range)
        n, p_ids, _ = self._subset("reset_done_dev", env_ids, n=n, device=True, all_envs="the masks cover every environment")
        p_done, p_failed = _dev_ptr(done, "done", "int32", n), _dev_ptr(failed, "failed", "int32", n)
        _lib.check(_lib.lib().gmr_motion_tracker_reset_done_dev(self.handle, n, p_ids, p_done, p_failed, 1 if resample else 0, lo, hi,
                                                                _lib._s(stream)))

    def adaptive_state(self) -> Dict[str, np.ndarray]:
        """``bin_start i32[C + 1]``, ``fail_now u32[Bt]`` (failures since the last Adapt), ``ema``, ``prob``, ``cdf`` (``f64[Bt]``) and
        ``clip_prob f64[C]``, the sum of ``prob`` over the bins of every clip.  Synchronous."""
        _, bin_start = self._need_adaptive("adaptive_state")
        Bt, Cn = int(bin_start[-1]), len(bin_start) - 1
        out = {"bin_start": np.empty(Cn + 1, np.int32), "fail_now": np.empty(Bt, np.uint32), "ema": np.empty(Bt, np.float64),
               "prob": np.empty(Bt, np.float64), "cdf": np.empty(Bt, np.float64)}
        _lib.check(_lib.lib().gmr_motion_tracker_adaptive_state(self.handle, *[_lib._ptr(out[k]) for k in ("bin_start", "fail_now", "ema", "prob", "cdf")]))
        assert np.array_equal(out["bin_start"], bin_start), "the library's bins differ from the ones computed here"
        out["clip_prob"] = np.bincount(np.repeat(np.arange(Cn), np.diff(bin_start)), weights=out["prob"], minlength=Cn)
        return out

    # ---- anchors -------------------------------------------------------------------------------------
    def _anchor_yaw_allowed(self, what: str) -> None:
        if self.library.ang_vel != "world":
            raise ValueError(f'{what}: a yaw anchor needs a library built with ang_vel="world": the root_ang_vel of '
                             f'ang_vel="{self.library.ang_vel}" is not a physical angular velocity and cannot be rotated')

    def _need_anchors(self, what: str) -> None:
        if not self._anchors:
            raise ValueError(f"{what}: anchors are not enabled on this tracker, call enable_anchors() first")

    def enable_anchors(self, on: bool = True) -> None:
        """Per-environment anchors: a yaw about the vertical, then a translation, applied to every world-frame quantity the tracker emits
        or compares -- the four root rows and root terms of :meth:`step` / :meth:`step_links`, the ``frame="world"`` link rows and terms,
        the root blocks of a ``"raw"`` preview and the reference of a ``"sim"`` one.  ``frame="heading"`` links and a ``"reference"``
        preview do not see them.  Enabling allocates the two arrays once and fills them with the identity (synchronous; a tracker that
        has them keeps them as they are); ``on=False`` frees them and the tracker runs the plain code path again."""
        _lib.check(_lib.lib().gmr_motion_tracker_enable_anchors(self.handle, 1 if on else 0))
        self._anchors = bool(on)

    def _anchor_setup(self, what, pos, yaw, env_ids, n=None):
        """the checks of :meth:`set_anchor`, all of them before a device is touched -> ``(n, ids i32[n] or None, pos f32[n,3] or None, yaw
        f32[n] or None)``"""
        n, ids, _ = self._subset(what, env_ids, once=False)
        if pos is not None:
            pos = np.ascontiguousarray(pos, dtype=np.float32)
            if pos.shape != (n, 3):
                raise ValueError(f"{what}: pos has shape {pos.shape}, {(n, 3)} needed")
            if not np.isfinite(pos).all():
                raise ValueError(f"{what}: pos is not finite")
        if yaw is not None:
            self._anchor_yaw_allowed(what)
            yaw = np.ascontiguousarray(yaw, dtype=np.float32)
            if yaw.shape != (n,):
                raise ValueError(f"{what}: yaw has shape {yaw.shape}, {(n,)} needed")
            if not np.isfinite(yaw).all():
                raise ValueError(f"{what}: yaw is not finite")
        return n, ids, pos, yaw

    def set_anchor(self, pos=None, yaw=None, env_ids=None) -> int:
        """Sets the anchors of ``env_ids`` (all, in order, by default): ``pos [n,3]`` metres and / or ``yaw [n]`` radians; what is ``None``
        is kept.  Enables anchors when they are not.  Returns how many ids lay outside ``[0, num_envs)`` (they are ignored)."""
        n, ids, pos, yaw = self._anchor_setup("set_anchor", pos, yaw, env_ids)
        ignored = C.c_int()
        _lib.check(_lib.lib().gmr_motion_tracker_set_anchor(self.handle, n, _lib._ptr(ids), _lib._ptr(pos), _lib._ptr(yaw), C.byref(ignored)))
        self._anchors = True
        return int(ignored.value)

    def set_anchor_dev(self, pos=None, yaw=None, env_ids=None, n: Optional[int] = None, stream=None) -> None:
        """:meth:`set_anchor` on device memory (``pos f32[n*3]``, ``yaw f32[n]`` radians, ``env_ids i32[n]`` with ``n``, or None for all),
        asynchronous on ``stream``: one launch.  Anchors must be enabled."""
        self._need_anchors("set_anchor_dev")
        if yaw is not None:
            self._anchor_yaw_allowed("set_anchor_dev")
        n, p_ids, _ = self._subset("set_anchor_dev", env_ids, n=n, device=True)
        p_pos, p_yaw = _dev_ptr(pos, "pos", "float32", n * 3), _dev_ptr(yaw, "yaw", "float32", n)
        _lib.check(_lib.lib().gmr_motion_tracker_set_anchor_dev(self.handle, n, p_ids, p_pos, p_yaw, _lib._s(stream)))

    def anchor_to_root(self, root_pos, root_quat, mask=None, env_ids=None, yaw: bool = True, z: bool = False) -> int:
        """Anchors the reference to where the robot is: for every environment whose ``mask`` is set (``None``: all), the anchor that
        carries the reference root at the environment's own ``(clip, time)`` onto ``root_pos [n,3]`` / ``root_quat [n,4]`` xyzw in x, y and
        -- with ``yaw`` -- heading, and -- with ``z`` -- height; what is not asked for is kept.  Without ``env_ids`` the three arrays
        cover every environment; with it (every environment at most once) they are indexed by list position, as the masks of
        :meth:`reset_done` are.  A bad assignment or a root that is not finite leaves that environment's anchor as it was.  Enables
        anchors when they are not.  Returns how many ids of masked entries lay outside ``[0, num_envs)``."""
        if yaw:
            self._anchor_yaw_allowed("anchor_to_root")
        n, ids, m = self._subset("anchor_to_root", env_ids, mask)
        rp, rq = np.ascontiguousarray(root_pos, dtype=np.float32), np.ascontiguousarray(root_quat, dtype=np.float32)
        if rp.shape != (n, 3):
            raise ValueError(f"anchor_to_root: root_pos has shape {rp.shape}, {(n, 3)} needed")
        if rq.shape != (n, 4):
            raise ValueError(f"anchor_to_root: root_quat has shape {rq.shape}, {(n, 4)} needed")
        ignored = C.c_int()
        _lib.check(_lib.lib().gmr_motion_tracker_anchor_to_root(self.handle, n, _lib._ptr(ids), _lib._ptr(m), _lib._ptr(rp), _lib._ptr(rq),
                                                                (_lib.ANCHOR_YAW if yaw else 0) | (_lib.ANCHOR_Z if z else 0), C.byref(ignored)))
        self._anchors = True
        return int(ignored.value)

    def anchor_to_root_dev(self, root_pos, root_quat, mask=None, env_ids=None, n: Optional[int] = None, yaw: bool = True, z: bool = False,
                           stream=None) -> None:
        """:meth:`anchor_to_root` on device memory, asynchronous on ``stream``: ONE launch, no allocation, no synchronisation, no
        read-back.  ``mask`` is an ``i32`` mask as a step leaves it (``finished``) or as :meth:`reset_done_dev` takes it; ``root_pos
        f32[n*3]``, ``root_quat f32[n*4]``; with ``env_ids`` (``i32[n]``) ``n`` is mandatory.  Anchors must be enabled."""
        self._need_anchors("anchor_to_root_dev")
        if yaw:
            self._anchor_yaw_allowed("anchor_to_root_dev")
        n, p_ids, p_mask = self._subset("anchor_to_root_dev", env_ids, mask, n, device=True)
        if root_pos is None or root_quat is None:
            raise ValueError("anchor_to_root_dev: root_pos and root_quat are needed")
        p_pos, p_quat = _dev_ptr(root_pos, "root_pos", "float32", n * 3), _dev_ptr(root_quat, "root_quat", "float32", n * 4)
        _lib.check(_lib.lib().gmr_motion_tracker_anchor_to_root_dev(self.handle, n, p_ids, p_mask, p_pos, p_quat,
                                                                    (_lib.ANCHOR_YAW if yaw else 0) | (_lib.ANCHOR_Z if z else 0), _lib._s(stream)))

    def anchor_state(self) -> Optional[Dict[str, np.ndarray]]:
        """``pos f32[N,3]`` and ``yaw_zw f32[N,2]``, the ``(z, w)`` of the yaw's unit quaternion, or ``None`` when anchors are off.
        Synchronous."""
        if not self._anchors:
            return None
        out = {"pos": np.empty((self.num_envs, 3), np.float32), "yaw_zw": np.empty((self.num_envs, 2), np.float32)}
        _lib.check(_lib.lib().gmr_motion_tracker_anchor_state(self.handle, _lib._ptr(out["pos"]), _lib._ptr(out["yaw_zw"])))
        return out

    # ---- control -------------------------------------------------------------------------------------
    def _control_setup(self, default_dof_pos, action_scale, clip_actions, startup_seconds, gain_startup, gain_run, decimation):
        """the checks of :meth:`set_control`, all of them before a device is touched -> ``(default f32[R], k, c, D, g0, g1, M)``"""
        R = self.nrobot_dof
        d = np.ascontiguousarray(default_dof_pos, dtype=np.float32).reshape(-1)
        if len(d) != R:
            raise ValueError(f"default_dof_pos has {len(d)} entries, the robot {R} dofs")
        if not np.isfinite(d).all():
            raise ValueError("default_dof_pos is not finite")
        k, c, D, g0, g1 = (float(np.float32(x)) for x in (action_scale, clip_actions, startup_seconds, gain_startup, gain_run))
        if not (np.isfinite(k) and np.isfinite(g0) and np.isfinite(g1)):
            raise ValueError(f"action_scale = {k}, gain_startup = {g0} and gain_run = {g1} must be finite")
        if not c > 0:
            raise ValueError(f"clip_actions = {c}, must be positive (inf: no clipping)")
        if not (np.isfinite(D) and D >= 0):
            raise ValueError(f"startup_seconds = {D}, must be finite and not negative (0: no start-up phase)")
        if int(decimation) != decimation or not 1 <= int(decimation) <= CONTROL_MAX_DECIMATION:
            raise ValueError(f"decimation = {decimation} outside 1 to {CONTROL_MAX_DECIMATION} substeps")
        return d, k, c, D, g0, g1, int(decimation)

    def set_control(self, default_dof_pos, action_scale: float, clip_actions: float, startup_seconds: float = DEFAULT_CONTROL["startup_seconds"],
                    gain_startup: float = DEFAULT_CONTROL["gain_startup"], gain_run: float = DEFAULT_CONTROL["gain_run"], *, decimation: int) -> None:
        """Configures the control half: ``default_dof_pos [R]``, the robot's default joint angles from which :meth:`targets` eases in (a
        table of its own, not the ``dof_default`` of the dof map), ``action_scale`` and ``clip_actions`` (``inf``: no clipping) of the
        policy action, the ``startup_seconds`` of the easing (0: none) with the action gain during it and afterwards, and ``decimation``,
        the physics substeps per step.  Allocates ``held`` and ``torque_acc`` (``[N, R]``, zeros).  Synchronous; call it again after
        :meth:`set_dof_map` has changed the number of robot dofs."""
        d, k, c, D, g0, g1, M = self._control_setup(default_dof_pos, action_scale, clip_actions, startup_seconds, gain_startup, gain_run, decimation)
        _lib.check(_lib.lib().gmr_motion_tracker_set_control(self.handle, _lib._ptr(d), k, c, D, g0, g1, M))
        self._control = (self.nrobot_dof, M)

    def _need_control(self, what: str):
        ctl = self._control
        if ctl is None:
            raise ValueError(f"{what}: control is not set on this tracker, call set_control() first")
        if ctl[0] != self.nrobot_dof:
            raise ValueError(f"{what}: control was set for {ctl[0]} robot dofs, the dof map now has {self.nrobot_dof}: call set_control() again")
        return ctl

    def _rows(self, a, what: str, n: Optional[int] = None):
        """``a`` as ``f32[n, R]`` (n = num_envs by default), its shape checked"""
        n = self.num_envs if n is None else n
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != (n, self.nrobot_dof):
            raise ValueError(f"{what}: shape {a.shape}, {(n, self.nrobot_dof)} needed")
        return a

    def _per_env_ints(self, a, what: str):
        if a is None:
            return None
        a = np.asarray(a)
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"{what}: integers needed, got {a.dtype}")
        if a.shape != (self.num_envs,):
            raise ValueError(f"{what}: shape {a.shape}, {(self.num_envs,)} needed")
        return np.ascontiguousarray(a, dtype=np.int32)

    def targets(self, actions=None, episode_steps=None) -> Dict[str, np.ndarray]:
        """The PD targets of the next physics step, host arrays in and out: ``dof_targets [N,R]`` -- the reference's joint row at every
        environment's present clock (what a following :meth:`step` returns as ``ref_dof_pos``, bit for bit), eased in from the default
        pose with a cosine S-curve while ``episode_steps [N] * dt`` (the simulator's episode length counter; ``None``: no start-up) is
        below ``startup_seconds``, plus ``action_scale * clip(actions) * gain`` --, ``status i32[N]`` (1: a bad assignment, its row is
        NaN) and, with ``actions [N,R]``, ``actions_clipped``.  One launch; clocks, clips and draw counters stay as they are."""
        self._need_control("targets")
        N, R = self.num_envs, self.nrobot_dof
        a = None if actions is None else self._rows(actions, "actions")
        st = self._per_env_ints(episode_steps, "episode_steps")
        out = {"dof_targets": np.empty((N, R), np.float32), "status": np.empty(N, np.int32)}
        if a is not None:
            out["actions_clipped"] = np.empty((N, R), np.float32)
        _lib.check(_lib.lib().gmr_motion_tracker_targets(self.handle, _lib._ptr(a), _lib._ptr(st), _lib._ptr(out["dof_targets"]),
                                                         _lib._ptr(out.get("actions_clipped")), _lib._ptr(out["status"])))
        return out

    def targets_dev(self, actions=None, episode_steps=None, dof_targets=None, actions_clipped=None, status=None, stream=None) -> None:
        """:meth:`targets` on device memory, asynchronous on ``stream``: ``actions f32[N*R]`` and ``episode_steps i32[N]`` (each may be
        ``None``) in, whichever of ``dof_targets f32[N*R]``, ``actions_clipped f32[N*R]``, ``status i32[N]`` are wanted out."""
        self._need_control("targets_dev")
        N, R = self.num_envs, self.nrobot_dof
        if actions_clipped is not None and actions is None:
            raise ValueError("targets_dev: actions_clipped needs actions")
        ptrs = (_dev_ptr(actions, "actions", "float32", N * R), _dev_ptr(episode_steps, "episode_steps", "int32", N),
                _dev_ptr(dof_targets, "dof_targets", "float32", N * R), _dev_ptr(actions_clipped, "actions_clipped", "float32", N * R),
                _dev_ptr(status, "status", "int32", N))
        _lib.check(_lib.lib().gmr_motion_tracker_targets_dev(self.handle, *ptrs, _lib._s(stream)))

    def hold(self, dof_pos, mask=None, env_ids=None) -> int:
        """After a reset: the actuators of every environment whose ``mask`` is set (``None``: all) hold ``dof_pos [n,R]`` and its running
        torque sum is cleared.  Without ``env_ids`` the arrays cover every environment; with it (every environment at most once) they are
        indexed by list position, as the masks of :meth:`reset_done` are.  Returns how many ids of masked entries lay outside
        ``[0, num_envs)``."""
        self._need_control("hold")
        n, ids, m = self._subset("hold", env_ids, mask)
        q = self._rows(dof_pos, "dof_pos", n)
        if n == 0:
            return 0
        ignored = C.c_int()
        _lib.check(_lib.lib().gmr_motion_tracker_hold(self.handle, n, _lib._ptr(ids), _lib._ptr(m), _lib._ptr(q), C.byref(ignored)))
        return int(ignored.value)

    def hold_dev(self, dof_pos, mask=None, env_ids=None, n: Optional[int] = None, stream=None) -> None:
        """:meth:`hold` on device memory, asynchronous on ``stream``: ONE launch.  ``dof_pos f32[n*R]``, ``mask i32[n]`` as a step leaves
        it (``finished``) or as :meth:`reset_done_dev` takes it; with ``env_ids`` (``i32[n]``) ``n`` is mandatory."""
        self._need_control("hold_dev")
        n, p_ids, p_mask = self._subset("hold_dev", env_ids, mask, n, device=True)
        if dof_pos is None:
            raise ValueError("hold_dev: dof_pos is needed")
        p_pos = _dev_ptr(dof_pos, "dof_pos", "float32", n * self.nrobot_dof)
        _lib.check(_lib.lib().gmr_motion_tracker_hold_dev(self.handle, n, p_ids, p_mask, p_pos, _lib._s(stream)))

    def _check_substep(self, what: str, substep) -> int:
        _, M = self._need_control(what)
        if int(substep) != substep or not 0 <= int(substep) < M:
            raise ValueError(f"{what}: substep = {substep} outside [0, {M})")
        return int(substep)

    def _actuator(self, what: str, stiffness, damping, friction, torque_limit, per_env):
        """the actuator arrays of :meth:`torques` as float32, their shapes checked -> ``(per_env, kp, kd, fr or None, lim or None)``"""
        N, R = self.num_envs, self.nrobot_dof
        kp = np.ascontiguousarray(stiffness, dtype=np.float32)
        if per_env is None:
            per_env = kp.ndim == 2
        shape = (N, R) if per_env else (R,)
        out = [bool(per_env)]
        for name, a in (("stiffness", kp), ("damping", damping), ("friction", friction)):
            if a is None:
                if name != "friction":
                    raise ValueError(f"{what}: {name} is needed")
                out.append(None)
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"{what}: {name} has shape {a.shape}, {shape} needed (per_env = {bool(per_env)}: the three share one shape)")
            out.append(a)
        lim = None
        if torque_limit is not None:
            lim = np.ascontiguousarray(torque_limit, dtype=np.float32)
            if lim.shape != (R,):
                raise ValueError(f"{what}: torque_limit has shape {lim.shape}, {(R,)} needed")
        return tuple(out) + (lim,)

    def torques(self, substep: int, dof_targets, dof_pos, dof_vel, stiffness, damping, friction=None, torque_limit=None, delay_steps=None,
                per_env: Optional[bool] = None) -> Dict[str, np.ndarray]:
        """The actuator model of physics substep ``substep`` (0 to ``decimation - 1``), host arrays in and out: an environment whose
        ``delay_steps [N]`` (``None``: 0) equals the substep takes ``dof_targets [N,R]`` into ``held``; ``tau = stiffness * (held -
        dof_pos) - damping * dof_vel``, less ``min(friction, |tau|) * sign(tau)``, clipped to ``torque_limit [R]``.  ``stiffness``,
        ``damping`` and ``friction`` are all ``[N,R]`` (``per_env``) or all ``[R]``; ``per_env=None`` reads it off ``stiffness``.  Returns
        ``dof_torques [N,R]`` and, after the last substep, ``mean_torques``, the mean over the step's substeps.  One launch."""
        i = self._check_substep("torques", substep)
        N, R = self.num_envs, self.nrobot_dof
        tg, q, qd = self._rows(dof_targets, "dof_targets"), self._rows(dof_pos, "dof_pos"), self._rows(dof_vel, "dof_vel")
        pe, kp, kd, fr, lim = self._actuator("torques", stiffness, damping, friction, torque_limit, per_env)
        ds = self._per_env_ints(delay_steps, "delay_steps")
        act = _lib.TrackerActuator(*[None if a is None else a.ctypes.data for a in (kp, kd, fr, lim)], 1 if pe else 0)
        out = {"dof_torques": np.empty((N, R), np.float32)}
        if i == self._control[1] - 1:
            out["mean_torques"] = np.empty((N, R), np.float32)
        _lib.check(_lib.lib().gmr_motion_tracker_torques(self.handle, i, _lib._ptr(tg), _lib._ptr(q), _lib._ptr(qd), C.byref(act), _lib._ptr(ds),
                                                         _lib._ptr(out["dof_torques"]), _lib._ptr(out.get("mean_torques"))))
        return out

    def torques_dev(self, substep: int, dof_targets, dof_pos, dof_vel, stiffness, damping, dof_torques, friction=None, torque_limit=None,
                    delay_steps=None, mean_torques=None, per_env: bool = True, stream=None) -> None:
        """:meth:`torques` on device memory, asynchronous on ``stream``: ONE launch.  Every array is a ``_lib.DeviceBuffer``, a raw address
        or an object with ``data_ptr()``; ``per_env`` says whether ``stiffness``, ``damping`` and ``friction`` hold ``N*R`` or ``R``
        floats.  ``mean_torques`` is written by the last substep only."""
        i = self._check_substep("torques_dev", substep)
        N, R = self.num_envs, self.nrobot_dof
        for name, x in (("dof_targets", dof_targets), ("dof_pos", dof_pos), ("dof_vel", dof_vel), ("stiffness", stiffness), ("damping", damping),
                        ("dof_torques", dof_torques)):
            if x is None:
                raise ValueError(f"torques_dev: {name} is needed")
        g = N * R if per_env else R
        act = _lib.TrackerActuator()
        for name, x, count in (("stiffness", stiffness, g), ("damping", damping, g), ("friction", friction, g), ("torque_limit", torque_limit, R)):
            p = _dev_ptr(x, name, "float32", count)
            setattr(act, name, None if p is None else p.value)
        act.per_env = 1 if per_env else 0
        rows = [_dev_ptr(x, name, "float32", N * R) for name, x in (("dof_targets", dof_targets), ("dof_pos", dof_pos), ("dof_vel", dof_vel))]
        p_delay, p_tau = _dev_ptr(delay_steps, "delay_steps", "int32", N), _dev_ptr(dof_torques, "dof_torques", "float32", N * R)
        p_mean = _dev_ptr(mean_torques, "mean_torques", "float32", N * R)
        _lib.check(_lib.lib().gmr_motion_tracker_torques_dev(self.handle, i, *rows, C.byref(act), p_delay, p_tau, p_mean, _lib._s(stream)))

    def control_state(self) -> Optional[Dict[str, np.ndarray]]:
        """``held f32[N,R]``, the targets the actuators hold, and ``torque_acc f32[N,R]``, the running torque sum of the current step, or
        ``None`` when control is not set.  Synchronous."""
        if self._control is None:
            return None
        self._need_control("control_state")
        out = {"held": np.empty((self.num_envs, self.nrobot_dof), np.float32), "torque_acc": np.empty((self.num_envs, self.nrobot_dof), np.float32)}
        _lib.check(_lib.lib().gmr_motion_tracker_control_state(self.handle, _lib._ptr(out["held"]), _lib._ptr(out["torque_acc"])))
        return out

    # ---- proprioception ------------------------------------------------------------------------------
    def _proprio_setup(self, default_dof_pos, dof_pos_limits, dof_vel_limits, torque_limits, extra_cols, filter_weight, normalization, noise,
                       soft_dof_pos_limit, soft_dof_vel_limit, soft_torque_limit, base_height_target, terminate_vel, terminate_height,
                       max_episode_steps, scales):
        """the checks of :meth:`set_proprio`, all of them before a device is touched -> a dict of the checked values"""
        R = self.nrobot_dof
        tables = {}
        for name, a, shape in (("default_dof_pos", default_dof_pos, (R,)), ("dof_pos_limits", dof_pos_limits, (R, 2)),
                               ("dof_vel_limits", dof_vel_limits, (R,)), ("torque_limits", torque_limits, (R,))):
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"{name} has shape {a.shape}, {shape} needed (the robot has {R} dofs)")
            if not np.isfinite(a).all():
                raise ValueError(f"{name} is not finite")
            tables[name] = a
        if int(extra_cols) != extra_cols or not 0 <= int(extra_cols) <= PROPRIO_MAX_EXTRA:
            raise ValueError(f"extra_cols = {extra_cols} outside 0 to {PROPRIO_MAX_EXTRA} pass-through columns")
        if int(max_episode_steps) != max_episode_steps or not 0 <= int(max_episode_steps) < 2 ** 31:
            raise ValueError(f"max_episode_steps = {max_episode_steps}, a whole number of steps that is not negative is needed")
        fw, sp, sv, st = (float(x) for x in (filter_weight, soft_dof_pos_limit, soft_dof_vel_limit, soft_torque_limit))
        if not all(np.isfinite(x) for x in (fw, sp, sv, st)):
            raise ValueError(f"filter_weight = {fw} and the soft factors {(sp, sv, st)} must be finite")
        norm = dict.fromkeys(PROPRIO_NORMALIZATION, 1.0)
        if normalization is not None:
            unknown = sorted(set(normalization) - set(norm))
            if unknown:
                raise KeyError(f"normalization: unknown scales {unknown} (known: {list(PROPRIO_NORMALIZATION)})")
            norm.update(normalization)
        norm = {k: float(np.float32(v)) for k, v in norm.items()}
        scalars = {k: float(np.float32(v)) for k, v in (("base_height_target", base_height_target), ("terminate_vel", terminate_vel),
                                                        ("terminate_height", terminate_height))}
        for k, v in {**norm, **scalars}.items():
            if not np.isfinite(v):
                raise ValueError(f"{k} = {v} must be finite")
        noise = {} if noise is None else dict(noise)
        unknown = sorted(set(noise) - set(PROPRIO_NOISE_BLOCKS))
        if unknown:
            raise KeyError(f"noise: unknown blocks {unknown} (known: {list(PROPRIO_NOISE_BLOCKS)})")
        specs = [self._noise_spec(f"noise[{k!r}]", noise.get(k)) for k in PROPRIO_NOISE_BLOCKS]
        if scales is None:
            sc = np.zeros(len(PROPRIO_TERMS), np.float32)
        else:
            if isinstance(scales, dict):
                unknown = sorted(set(scales) - set(PROPRIO_TERMS))
                if unknown:
                    raise KeyError(f"scales: unknown terms {unknown} (known: {list(PROPRIO_TERMS)})")
                scales = [scales.get(k, 0.0) for k in PROPRIO_TERMS]
            sc = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
            if len(sc) != len(PROPRIO_TERMS):
                raise ValueError(f"scales has {len(sc)} entries, there are {len(PROPRIO_TERMS)} terms: {list(PROPRIO_TERMS)}")
            if not np.isfinite(sc).all():
                raise ValueError("scales must be finite")
        # the soft position limits as the library forms them (t1.py:665-670), to refuse upper < lower here
        lim = tables["dof_pos_limits"]
        half = np.float32(0.5 * (1.0 - sp))
        span = lim[:, 1] - lim[:, 0]
        lower, upper = lim[:, 0] + half * span, lim[:, 1] - half * span
        soft = (lower, upper, tables["dof_vel_limits"] * np.float32(sv), tables["torque_limits"] * np.float32(st))
        if not all(np.isfinite(x).all() for x in soft):
            raise ValueError("the soft limits are not finite in float32")
        if (upper < lower).any():
            raise ValueError(f"dof_pos_limits: upper < lower at dofs {np.nonzero(upper < lower)[0].tolist()}")
        return {**tables, "scales": sc, "extra_cols": int(extra_cols), "max_episode_steps": int(max_episode_steps), "filter_weight": fw,
                "soft": (sp, sv, st), "norm": norm, **scalars, "noise": specs}

    def set_proprio(self, default_dof_pos, dof_pos_limits, dof_vel_limits, torque_limits, *, base_height_target: float, terminate_vel: float,
                    terminate_height: float, max_episode_steps: int, extra_cols: int = 0, filter_weight: float = 1.0, normalization=None,
                    noise=None, soft_dof_pos_limit: float = 1.0, soft_dof_vel_limit: float = 1.0, soft_torque_limit: float = 1.0,
                    scales=None) -> None:
        """Configures the proprioception half: ``default_dof_pos [R]`` (a table of its own, independent of :meth:`set_control`),
        ``dof_pos_limits [R,2]``, ``dof_vel_limits [R]`` and ``torque_limits [R]`` with their three soft factors, ``extra_cols`` pass-through
        columns (0 to 16) of the observation row, the ``filter_weight`` of the low-pass filtered velocities, ``normalization`` -- a dict
        over ``gravity, lin_vel, ang_vel, dof_pos, dof_vel`` (1 by default) --, ``noise`` -- a dict over :data:`PROPRIO_NOISE_BLOCKS` of
        ``{"distribution": "gaussian" | "uniform" | "none", "operation": "additive" | "scaling", "range": (a, b)}`` as the reference's
        configuration writes them --, ``base_height_target``, the thresholds ``terminate_vel`` and ``terminate_height``,
        ``max_episode_steps`` (``ceil(episode_length_s / dt)``) and ``scales``, fourteen numbers or a dict over :data:`PROPRIO_TERMS` that
        weigh ``total`` (zero, the default: the term stays out).  Allocates the six state arrays (zeros).  Synchronous; call it again
        after :meth:`set_dof_map` has changed the number of robot dofs."""
        c = self._proprio_setup(default_dof_pos, dof_pos_limits, dof_vel_limits, torque_limits, extra_cols, filter_weight, normalization, noise,
                                soft_dof_pos_limit, soft_dof_vel_limit, soft_torque_limit, base_height_target, terminate_vel, terminate_height,
                                max_episode_steps, scales)
        cfg = _lib.ProprioConfig()
        for k in _lib.PROPRIO_CONFIG_TABLES:
            setattr(cfg, k, c[k].ctypes.data)
        cfg.extra_cols, cfg.max_episode_steps, cfg.filter_weight = c["extra_cols"], c["max_episode_steps"], c["filter_weight"]
        cfg.soft_dof_pos_limit, cfg.soft_dof_vel_limit, cfg.soft_torque_limit = c["soft"]
        for k in PROPRIO_NORMALIZATION:
            setattr(cfg, "scale_" + k, c["norm"][k])
        cfg.base_height_target, cfg.terminate_vel, cfg.terminate_height = c["base_height_target"], c["terminate_vel"], c["terminate_height"]
        for i, (dist, op, a, b) in enumerate(c["noise"]):
            cfg.noise[i].distribution, cfg.noise[i].operation, cfg.noise[i].a, cfg.noise[i].b = dist, op, a, b
        _lib.check(_lib.lib().gmr_motion_tracker_set_proprio(self.handle, C.byref(cfg)))
        self._proprio = (self.nrobot_dof, c["extra_cols"])

    def _need_proprio(self, what: str):
        p = self._proprio
        if p is None:
            raise ValueError(f"{what}: proprio is not set on this tracker, call set_proprio() first")
        if p[0] != self.nrobot_dof:
            raise ValueError(f"{what}: proprio was set for {p[0]} robot dofs, the dof map now has {self.nrobot_dof}: call set_proprio() again")
        return p

    def proprio_layout(self) -> Dict[str, object]:
        """The column ranges ``(first, end)`` of ``obs`` -- ``gravity, ang_vel, extra, dof_pos, dof_vel, actions`` --, its ``width``, the
        ranges of ``priv`` (``lin_vel, height``) and ``terms``, the names of the columns of ``term``"""
        R, Cx = self._need_proprio("proprio_layout")
        edges = np.cumsum([0, 3, 3, Cx, R, R, R])
        names = ("gravity", "ang_vel", "extra", "dof_pos", "dof_vel", "actions")
        return {"obs": {k: (int(edges[i]), int(edges[i + 1])) for i, k in enumerate(names)}, "width": int(edges[-1]),
                "priv": {"lin_vel": (0, 3), "height": (3, 4)}, "terms": PROPRIO_TERMS}

    def _proprio_counts(self):
        R, Cx = self._proprio
        return _lib.widths(_lib.PROPRIO_IN, R=R, extra_cols=Cx), _lib.widths(_lib.PROPRIO_OUT, obs_cols=6 + Cx + 3 * R)

    def _proprio_rows(self):
        R, Cx = self._proprio
        return self._rows_of(_lib.PROPRIO_IN, R=R, extra_cols=Cx), self._rows_of(_lib.PROPRIO_OUT, obs_cols=6 + Cx + 3 * R)

    def _check_extra(self, what: str, extra) -> None:
        if (extra is not None) != (self._proprio[1] > 0):
            raise ValueError(f"{what}: extra is needed exactly when extra_cols > 0 (extra_cols = {self._proprio[1]}, extra "
                             f"{'given' if extra is not None else 'missing'})")

    def proprio(self, root_states, dof_pos, dof_vel, actions=None, mean_torques=None, extra=None, ground=None, episode_steps=None,
                noise: bool = True) -> Dict[str, np.ndarray]:
        """What follows the physics of a step, host arrays in and out: from ``root_states [N,13]`` (position, xyzw quaternion, world linear
        and angular velocity, the simulator's tensor as it lies), ``dof_pos``, ``dof_vel`` ``[N,R]`` and, each optional, the clipped
        ``actions [N,R]`` of :meth:`targets`, the ``mean_torques [N,R]`` of :meth:`torques`, ``extra [N,extra_cols]``, ``ground [N]``
        (terrain height under the base; ``None``: 0) and ``episode_steps i32[N]`` -- ``base_lin_vel``, ``base_ang_vel``,
        ``projected_gravity``, ``filtered_lin_vel``, ``filtered_ang_vel`` ``[N,3]``, ``obs [N,W]`` (see :meth:`proprio_layout`), ``priv
        [N,4]``, ``term [N,14]`` in the order of :data:`PROPRIO_TERMS`, ``total [N]`` and ``done i32[N]`` (bit 0: velocity, bit 1: height,
        bit 2: time-out).  A term without its input is 0 and stays out of ``total``.  Then ``last_actions`` (with actions),
        ``last_dof_vel`` and ``last_root_vel`` roll over, and with ``noise`` and a noise spec every environment's tick moves by one.
        One launch; clocks, clips and draw counters stay as they are."""
        self._need_proprio("proprio")
        self._check_extra("proprio", extra)
        ins, outs = self._proprio_rows()
        given = {"root_states": root_states, "dof_pos": dof_pos, "dof_vel": dof_vel, "actions": actions, "mean_torques": mean_torques, "extra": extra,
                 "ground": ground, "episode_steps": episode_steps}
        st, keep = _lib.host_inputs(_lib.ProprioIn, ins, given, "proprio", required=("root_states", "dof_pos", "dof_vel"))
        table, out = _lib.host_outputs(_lib.ProprioOut, outs)
        _lib.check(_lib.lib().gmr_motion_tracker_proprio(self.handle, C.byref(st), 1 if noise else 0, C.byref(table)))
        return out

    def proprio_dev(self, root_states, dof_pos, dof_vel, actions=None, mean_torques=None, extra=None, ground=None, episode_steps=None,
                    noise: bool = True, stream=None, **outputs) -> None:
        """:meth:`proprio` on device memory, asynchronous on ``stream``: ONE launch.  ``outputs`` names whichever of the arrays of
        :meth:`proprio` are wanted; every array is a ``_lib.DeviceBuffer``, a raw address or an object with ``data_ptr()``."""
        self._need_proprio("proprio_dev")
        self._check_extra("proprio_dev", extra)
        ins, outs = self._proprio_rows()
        table = _lib.device_struct(_lib.ProprioOut, outs, outputs, "proprio_dev")
        given = {"root_states": root_states, "dof_pos": dof_pos, "dof_vel": dof_vel, "actions": actions, "mean_torques": mean_torques, "extra": extra,
                 "ground": ground, "episode_steps": episode_steps}
        st = _lib.device_struct(_lib.ProprioIn, ins, given, "proprio_dev", required=("root_states", "dof_pos", "dof_vel"))
        _lib.check(_lib.lib().gmr_motion_tracker_proprio_dev(self.handle, C.byref(st), 1 if noise else 0, C.byref(table), _lib._s(stream)))

    def proprio_reset(self, root_states, mask=None, env_ids=None) -> int:
        """After a reset: every environment whose ``mask`` is set (``None``: all) gets filtered velocities of zero and ``last_root_vel =
        root_states[i, 7:13]`` (``root_states [n,13]``); ``last_actions`` and ``last_dof_vel`` stay, as in the reference.  Without
        ``env_ids`` the arrays cover every environment; with it (every environment at most once) they are indexed by list position, as
        the arrays of :meth:`hold` are.  Returns how many ids of masked entries lay outside ``[0, num_envs)``."""
        self._need_proprio("proprio_reset")
        n, ids, m = self._subset("proprio_reset", env_ids, mask)
        rs = np.ascontiguousarray(root_states, dtype=np.float32)
        if rs.shape != (n, 13):
            raise ValueError(f"root_states: shape {rs.shape}, {(n, 13)} needed")
        if n == 0:
            return 0
        ignored = C.c_int()
        _lib.check(_lib.lib().gmr_motion_tracker_proprio_reset(self.handle, n, _lib._ptr(ids), _lib._ptr(m), _lib._ptr(rs), C.byref(ignored)))
        return int(ignored.value)

    def proprio_reset_dev(self, root_states, mask=None, env_ids=None, n: Optional[int] = None, stream=None) -> None:
        """:meth:`proprio_reset` on device memory, asynchronous on ``stream``: ONE launch.  ``root_states f32[n*13]``, ``mask i32[n]`` as a
        step leaves it (``done``) or as :meth:`reset_done_dev` takes it; with ``env_ids`` (``i32[n]``) ``n`` is mandatory."""
        self._need_proprio("proprio_reset_dev")
        n, p_ids, p_mask = self._subset("proprio_reset_dev", env_ids, mask, n, device=True)
        if root_states is None:
            raise ValueError("proprio_reset_dev: root_states is needed")
        p_roots = _dev_ptr(root_states, "root_states", "float32", n * 13)
        _lib.check(_lib.lib().gmr_motion_tracker_proprio_reset_dev(self.handle, n, p_ids, p_mask, p_roots, _lib._s(stream)))

    def proprio_state(self) -> Optional[Dict[str, np.ndarray]]:
        """``filtered_lin_vel``, ``filtered_ang_vel`` ``f32[N,3]``, ``last_root_vel f32[N,6]``, ``last_actions``, ``last_dof_vel``
        ``f32[N,R]`` and ``noise_tick u32[N]``, or ``None`` when proprio is not set.  Synchronous."""
        if self._proprio is None:
            return None
        self._need_proprio("proprio_state")
        N, R = self.num_envs, self.nrobot_dof
        out = {"filtered_lin_vel": np.empty((N, 3), np.float32), "filtered_ang_vel": np.empty((N, 3), np.float32),
               "last_root_vel": np.empty((N, 6), np.float32), "last_actions": np.empty((N, R), np.float32),
               "last_dof_vel": np.empty((N, R), np.float32), "noise_tick": np.empty(N, np.uint32)}
        _lib.check(_lib.lib().gmr_motion_tracker_proprio_state(self.handle, *[_lib._ptr(out[k]) for k in PROPRIO_STATE]))
        return out

    # ---- terrain and feet ---------------------------------------------------------------------------
    @staticmethod
    def _terrain_setup(height_field, horizontal_scale, vertical_scale, border_pixels):
        """the checks of :meth:`set_terrain`, all of them before a device is touched -> ``(field i16[nx,ny] or None, hs, vs, border)``"""
        hs, vs = float(horizontal_scale), float(vertical_scale)
        with np.errstate(over="ignore"):
            if not (np.isfinite(hs) and hs > 0 and np.isfinite(np.float32(hs)) and np.float32(hs) > 0):
                raise ValueError(f"horizontal_scale = {horizontal_scale} must be positive and finite (in float32 too)")
        if not (np.isfinite(vs) and vs > 0):
            raise ValueError(f"vertical_scale = {vertical_scale} must be positive and finite")
        if int(border_pixels) != border_pixels or not 0 <= int(border_pixels) <= 2 ** 24:
            raise ValueError(f"border_pixels = {border_pixels}, a whole number of pixels from 0 to 2^24 is needed")
        field = None
        if height_field is not None:
            if not isinstance(height_field, np.ndarray) or height_field.dtype != np.int16:
                raise TypeError(f"height_field is an int16 array, got {getattr(height_field, 'dtype', type(height_field).__name__)}")
            if height_field.ndim != 2:
                raise ValueError(f"height_field has {height_field.ndim} dimensions, [nx, ny] needed")
            if min(height_field.shape) < 2 or max(height_field.shape) > 2 ** 24:
                raise ValueError(f"height_field has shape {height_field.shape}, 2 to 2^24 pixels per side are needed")
            field = np.ascontiguousarray(height_field)
        return field, hs, vs, int(border_pixels)

    def set_terrain(self, height_field=None, horizontal_scale: float = 1.0, vertical_scale: float = 1.0, border_pixels: int = 0) -> None:
        """The terrain the heights are taken from: ``height_field int16 [nx, ny]`` (the first index is x, the reference's
        ``height_field_raw``) with its ``horizontal_scale``, ``vertical_scale`` and ``border_pixels``, or ``None`` for the plane of height
        0 (the state of a new tracker).  Synchronous: launches in flight keep the field they were given."""
        field, hs, vs, b = self._terrain_setup(height_field, horizontal_scale, vertical_scale, border_pixels)
        nx, ny = (0, 0) if field is None else field.shape
        _lib.check(_lib.lib().gmr_motion_tracker_set_terrain(self.handle, _lib._ptr(field), nx, ny, hs, vs, b))

    def terrain_heights(self, points):
        """``Terrain.terrain_heights`` of the reference without its host round trip: ``points [M, k]``, k >= 2 (x and y lead) ->
        ``(heights f32[M], outside)``, the reference's bits inside the field.  A point whose cell leaves the field is clamped to it and
        counted in ``outside``; a coordinate that is not finite gives NaN and is counted too.  One launch."""
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] < 2:
            raise ValueError(f"points: shape {p.shape}, (M, k) with k >= 2 needed")
        h = np.empty(len(p), np.float32)
        outside = C.c_int32()
        _lib.check(_lib.lib().gmr_motion_tracker_terrain_heights(self.handle, len(p), _lib._ptr(p), p.shape[1], _lib._ptr(h), C.byref(outside)))
        return h, int(outside.value)

    def terrain_heights_dev(self, points, n: int, heights, outside=None, stride: int = 3, stream=None) -> None:
        """:meth:`terrain_heights` on device memory, asynchronous on ``stream``: ONE launch.  Point ``i`` is ``points[i * stride]`` and
        the float behind it (``stride`` >= 2 floats: 3 for packed positions, 13 for root states); ``heights f32[n]``; the points outside
        the field are ADDED to ``outside i32[1]``, which the caller has zeroed."""
        n, stride = int(n), int(stride)
        if n < 0:
            raise ValueError(f"terrain_heights_dev: n = {n}")
        if stride < 2:
            raise ValueError(f"terrain_heights_dev: stride = {stride} floats, a point has at least x and y")
        if points is None or heights is None:
            raise ValueError("terrain_heights_dev: points and heights are needed")
        ptrs = (_dev_ptr(points, "points", "float32", max((n - 1) * stride + 2, 0)), _dev_ptr(heights, "heights", "float32", n),
                _dev_ptr(outside, "outside", "int32", 1))
        _lib.check(_lib.lib().gmr_motion_tracker_terrain_heights_dev(self.handle, n, ptrs[0], stride, ptrs[1], ptrs[2], _lib._s(stream)))

    @staticmethod
    def _feet_setup(feet_bodies, edge_pos, num_bodies, termination_bodies, penalized_bodies, force_threshold, contact_clearance, feet_distance_ref,
                    swing_period, scales):
        """the checks of :meth:`set_feet`, all of them before a device is touched -> a dict of the checked values"""
        if int(num_bodies) != num_bodies or not 1 <= int(num_bodies) <= 2 ** 16:
            raise ValueError(f"num_bodies = {num_bodies} outside 1 to 2^16")
        nb = int(num_bodies)
        edges = np.ascontiguousarray(edge_pos, dtype=np.float32)
        if edges.ndim != 2 or edges.shape[1] != 3 or not 1 <= len(edges) <= FEET_MAX_EDGES:
            raise ValueError(f"edge_pos has shape {edges.shape}, (E, 3) with 1 <= E <= {FEET_MAX_EDGES} needed")
        if not np.isfinite(edges).all():
            raise ValueError("edge_pos is not finite")
        lists = {}
        for name, a, count in (("feet_bodies", feet_bodies, (2, 2)), ("termination_bodies", termination_bodies, (0, FEET_MAX_BODIES)),
                               ("penalized_bodies", penalized_bodies, (0, FEET_MAX_BODIES))):
            a = np.asarray([] if a is None else a)
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise TypeError(f"{name} holds body indices (integers), got {a.dtype}")
            a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
            if not count[0] <= len(a) <= count[1]:
                raise ValueError(f"{name} has {len(a)} entries, {count[0]} to {count[1]} needed" if count[0] != count[1] else
                                 f"{name} has {len(a)} entries, the left and the right foot are needed")
            if ((a < 0) | (a >= nb)).any():
                raise ValueError(f"{name} entries lie in [0, {nb}): {a.tolist()}")
            if name != "feet_bodies" and len(np.unique(a)) != len(a):
                raise ValueError(f"{name} names a body twice: {a.tolist()}")
            lists[name] = a.astype(np.int32)
        scalars = {}
        for k, v in (("force_threshold", force_threshold), ("contact_clearance", contact_clearance), ("feet_distance_ref", feet_distance_ref),
                     ("swing_period", swing_period)):
            v = float(v)
            with np.errstate(over="ignore"):
                if not (np.isfinite(v) and np.isfinite(np.float32(v))):
                    raise ValueError(f"{k} = {v} must be finite in float32")
            scalars[k] = v
        if scales is None:
            sc = np.zeros(len(FEET_TERMS), np.float32)
        else:
            if isinstance(scales, dict):
                unknown = sorted(set(scales) - set(FEET_TERMS))
                if unknown:
                    raise KeyError(f"scales: unknown terms {unknown} (known: {list(FEET_TERMS)})")
                scales = [scales.get(k, 0.0) for k in FEET_TERMS]
            sc = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
            if len(sc) != len(FEET_TERMS):
                raise ValueError(f"scales has {len(sc)} entries, there are {len(FEET_TERMS)} terms: {list(FEET_TERMS)}")
            if not np.isfinite(sc).all():
                raise ValueError("scales must be finite")
        return {"edge_pos": edges, "num_bodies": nb, **lists, **scalars, "scales": sc}

    def set_feet(self, feet_bodies, edge_pos, num_bodies: int, *, feet_distance_ref: float, swing_period: float, termination_bodies=(),
                 penalized_bodies=(), force_threshold: float = DEFAULT_FEET["force_threshold"],
                 contact_clearance: float = DEFAULT_FEET["contact_clearance"], scales=None) -> None:
        """Configures the feet: ``feet_bodies`` (left, right) among the ``num_bodies`` rigid bodies of the simulator's tensors,
        ``edge_pos [E,3]`` (1 to 8 points in the foot's frame, the reference's ``feet_edge_pos``), the bodies whose contact force ends an
        episode and those it is penalised on (0 to 64 each, distinct), the force threshold and the contact clearance (the reference's 1.0
        and 0.01), ``feet_distance_ref``, ``swing_period`` and ``scales``, eight numbers or a dict over :data:`FEET_TERMS` that weigh
        ``total`` (zero, the default: the term stays out).  Allocates ``last_feet_pos`` and ``gait_process`` (zeros).  Synchronous."""
        c = self._feet_setup(feet_bodies, edge_pos, num_bodies, termination_bodies, penalized_bodies, force_threshold, contact_clearance,
                             feet_distance_ref, swing_period, scales)
        cfg = _lib.FeetConfig()
        cfg.edge_pos, cfg.scales = c["edge_pos"].ctypes.data, c["scales"].ctypes.data
        cfg.termination_body = c["termination_bodies"].ctypes.data if len(c["termination_bodies"]) else None
        cfg.penalized_body = c["penalized_bodies"].ctypes.data if len(c["penalized_bodies"]) else None
        cfg.feet_body[0], cfg.feet_body[1] = int(c["feet_bodies"][0]), int(c["feet_bodies"][1])
        cfg.num_edges, cfg.nb = len(c["edge_pos"]), c["num_bodies"]
        cfg.num_termination, cfg.num_penalized = len(c["termination_bodies"]), len(c["penalized_bodies"])
        for k in ("force_threshold", "contact_clearance", "feet_distance_ref", "swing_period"):
            setattr(cfg, k, c[k])
        _lib.check(_lib.lib().gmr_motion_tracker_set_feet(self.handle, C.byref(cfg)))
        self._feet = (c["num_bodies"], len(c["edge_pos"]))

    def _need_feet(self, what: str):
        f = self._feet
        if f is None:
            raise ValueError(f"{what}: the feet are not set on this tracker, call set_feet() first")
        return f

    def _feet_counts(self):
        return _lib.widths(_lib.FEET_IN, nb=self._feet[0]), _lib.widths(_lib.FEET_OUT)

    @staticmethod
    def _feet_bodies(what: str, bodies):
        """``bodies`` of a feet call, checked: the packed tensor alone, or ``body_pos`` with ``body_rot``"""
        if not isinstance(bodies, dict):
            raise TypeError(f"{what}: bodies is {{'body_state': [N, nb, 13]}} or {{'body_pos': [N, nb, 3], 'body_rot': [N, nb, 4]}}")
        if set(bodies) not in ({"body_state"}, {"body_pos", "body_rot"}) or any(a is None for a in bodies.values()):
            raise TypeError(f"{what}: bodies is either {{'body_state': ..}} or {{'body_pos': .., 'body_rot': ..}}, got {sorted(bodies)}")
        return bodies

    def feet(self, bodies, root_states, contact_forces=None, episode_steps=None, gait_frequency=None) -> Dict[str, np.ndarray]:
        """The feet half of a step, host arrays in and out: from ``bodies`` -- the simulator's rigid bodies as ``{"body_state": [N, nb,
        13]}`` (pos, quat xyzw, vel, ang vel) or ``{"body_pos": [N, nb, 3], "body_rot": [N, nb, 4]}`` --, ``root_states [N,13]`` and, each
        optional, ``contact_forces [N, nb, 3]``, ``episode_steps i32[N]`` and ``gait_frequency [N]`` -- ``feet_pos [N,2,3]``,
        ``feet_roll``, ``feet_yaw`` ``[N,2]``, ``feet_contact i32[N,2]``, ``ground [N]`` (the terrain height under the root: the
        ``ground`` of :meth:`proprio`), ``gait [N,2]`` (the cos and sin columns of the observation row), ``term [N,8]`` in the order of
        :data:`FEET_TERMS`, ``total [N]`` and ``done i32[N]`` (:data:`FEET_DONE_CONTACT` where a termination body is in contact).
        Without ``contact_forces`` ``collision`` is 0 and stays out of ``total``, and ``done`` is 0.  Then ``last_feet_pos`` rolls over
        and the gait clock has moved.  One launch; clocks, clips and draw counters stay as they are."""
        nb, _ = self._need_feet("feet")
        ls, keep = self._bodies(self._feet_bodies("feet", bodies), ("body_pos", "body_rot"), nb, nb)
        given = {"root_states": root_states, "contact_forces": contact_forces, "gait_frequency": gait_frequency, "episode_steps": episode_steps}
        st, held = _lib.host_inputs(_lib.FeetIn, self._rows_of(_lib.FEET_IN, nb=nb), given, "feet", required=("root_states",))
        table, out = _lib.host_outputs(_lib.FeetOut, self._rows_of(_lib.FEET_OUT))
        _lib.check(_lib.lib().gmr_motion_tracker_feet(self.handle, C.byref(ls), C.byref(st), C.byref(table)))
        return out

    def feet_dev(self, bodies, root_states, contact_forces=None, episode_steps=None, gait_frequency=None, stream=None, **outputs) -> None:
        """:meth:`feet` on device memory, asynchronous on ``stream``: ONE launch.  ``bodies`` is ``{"body_state": array}`` for the packed
        ``[N, nb, 13]`` tensor or ``{"body_pos": array, "body_rot": array}``; ``outputs`` names whichever of the arrays of :meth:`feet`
        are wanted (``ground`` goes into :meth:`proprio_dev` as it lies, ``gait`` into its ``extra`` columns); every array is a
        ``_lib.DeviceBuffer``, a raw address or an object with ``data_ptr()``."""
        nb, _ = self._need_feet("feet_dev")
        bodies = self._feet_bodies("feet_dev", bodies)
        table = _lib.device_struct(_lib.FeetOut, self._rows_of(_lib.FEET_OUT), outputs, "feet_dev")
        ls, _ = self._bodies(bodies, ("body_pos", "body_rot"), nb, nb, device=True)
        given = {"root_states": root_states, "contact_forces": contact_forces, "episode_steps": episode_steps, "gait_frequency": gait_frequency}
        st = _lib.device_struct(_lib.FeetIn, self._rows_of(_lib.FEET_IN, nb=nb), given, "feet_dev", required=("root_states",))
        _lib.check(_lib.lib().gmr_motion_tracker_feet_dev(self.handle, C.byref(ls), C.byref(st), C.byref(table), _lib._s(stream)))

    def feet_state(self) -> Optional[Dict[str, np.ndarray]]:
        """``last_feet_pos f32[N,2,3]`` and ``gait_process f32[N]``, or ``None`` when the feet are not set.  Synchronous."""
        if self._feet is None:
            return None
        N = self.num_envs
        out = {"last_feet_pos": np.empty((N, 2, 3), np.float32), "gait_process": np.empty(N, np.float32)}
        _lib.check(_lib.lib().gmr_motion_tracker_feet_state(self.handle, *[_lib._ptr(out[k]) for k in FEET_STATE]))
        return out

    # ---- commands, curriculum, kicks and pushes ----------------------------------------------------------
    @staticmethod
    def _commands_setup(lin_vel_x, lin_vel_y, ang_vel_yaw, gait_frequency, resample_steps, still_proportion, tracking_sigma, scales, obs_scales,
                        curriculum):
        """the checks of :meth:`set_commands`, all of them before the library is loaded -> a dict of the checked values"""
        def fits(x):
            with np.errstate(over="ignore"):
                return bool(np.isfinite(x) and np.isfinite(np.float32(x)))
        c = {}
        for name, r in (("lin_vel_x", lin_vel_x), ("lin_vel_y", lin_vel_y), ("ang_vel_yaw", ang_vel_yaw), ("gait_frequency", gait_frequency)):
            if r is None or len(r) != 2:
                raise ValueError(f"{name}: a range is a pair (lower, upper), got {r!r}")
            lo, hi = float(r[0]), float(r[1])
            if not (fits(lo) and fits(hi) and fits(hi - lo)):
                raise ValueError(f"{name}: range {(lo, hi)} is not finite in float32")
            if hi < lo:
                raise ValueError(f"{name}: upper = {hi} < lower = {lo}")
            c[name] = (lo, hi)
        if resample_steps is None or len(resample_steps) != 2 or any(int(x) != x for x in resample_steps):
            raise ValueError(f"resample_steps: a pair of whole step counts, got {resample_steps!r}")
        lo, hi = (int(x) for x in resample_steps)
        if not 1 <= lo < hi < 2 ** 31:
            raise ValueError(f"resample_steps = {(lo, hi)}: hi > lo >= 1 needed (the caller's int(resampling_time_s / dt) pair)")
        c["resample_steps"] = (lo, hi)
        p = float(still_proportion)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"still_proportion = {still_proportion} outside [0, 1]")
        sg = float(tracking_sigma)
        if not (fits(sg) and np.float32(sg) > 0):
            raise ValueError(f"tracking_sigma = {tracking_sigma} must be positive and finite (in float32 too)")
        c["still_proportion"], c["tracking_sigma"] = p, sg
        if scales is None:
            sc = np.zeros(len(CMD_TERMS), np.float32)
        else:
            if isinstance(scales, dict):
                unknown = sorted(set(scales) - set(CMD_TERMS))
                if unknown:
                    raise KeyError(f"scales: unknown terms {unknown} (known: {list(CMD_TERMS)})")
                scales = [scales.get(k, 0.0) for k in CMD_TERMS]
            with np.errstate(over="ignore"):
                sc = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
            if len(sc) != len(CMD_TERMS):
                raise ValueError(f"scales has {len(sc)} entries, there are {len(CMD_TERMS)} terms: {list(CMD_TERMS)}")
            if not np.isfinite(sc).all():
                raise ValueError("scales must be finite")
        with np.errstate(over="ignore"):
            ob = np.ascontiguousarray((1.0, 1.0, 1.0) if obs_scales is None else obs_scales, dtype=np.float32).reshape(-1)
        if len(ob) != 3 or not np.isfinite(ob).all():
            raise ValueError(f"obs_scales: three finite numbers (lin_vel, lin_vel, ang_vel), got {obs_scales!r}")
        c["scales"], c["obs_scales"], c["curriculum"] = sc, ob, None
        if curriculum is not None:
            need = ("lin_vel_levels", "ang_vel_levels", "update_rate", "tolerances", "resolutions", "min_success_steps")
            unknown, missing = sorted(set(curriculum) - set(need) - {"index_order"}), [k for k in need if k not in curriculum]
            if unknown or missing:
                raise KeyError(f"curriculum: unknown keys {unknown}, missing keys {missing}")
            L, A = curriculum["lin_vel_levels"], curriculum["ang_vel_levels"]
            if int(L) != L or int(A) != A or not (0 <= L <= CMD_MAX_LEVELS and 0 <= A <= CMD_MAX_LEVELS):
                raise ValueError(f"curriculum: lin_vel_levels = {L}, ang_vel_levels = {A} are whole numbers in [0, {CMD_MAX_LEVELS}]")
            order = curriculum.get("index_order", "grid")
            if order not in CMD_INDEX_ORDERS:
                raise ValueError(f"curriculum: index_order is one of {sorted(CMD_INDEX_ORDERS)}, got {order!r}")
            if order == "reference" and int(L) != int(A):
                raise ValueError(f"curriculum: index_order 'reference' transposes the grid and needs lin_vel_levels == ang_vel_levels, got {(L, A)}")
            rate = float(curriculum["update_rate"])
            if not (fits(rate) and rate >= 0):
                raise ValueError(f"curriculum: update_rate = {rate} must be finite and not negative")
            tol, res = (tuple(float(x) for x in curriculum[k]) for k in ("tolerances", "resolutions"))
            if len(tol) != 3 or len(res) != 3 or not all(fits(x) for x in tol + res):
                raise ValueError(f"curriculum: tolerances {tol} and resolutions {res} are three numbers each, finite in float32")
            ms = curriculum["min_success_steps"]
            if int(ms) != ms or not 0 <= ms < 2 ** 31:
                raise ValueError(f"curriculum: min_success_steps = {ms}, a whole number of steps that is not negative is needed")
            c["curriculum"] = {"L": int(L), "A": int(A), "order": order, "rate": rate, "tol": tol, "res": res, "min_success_steps": int(ms)}
        return c

    @staticmethod
    def min_success_steps(episode_length_s: float, dt: float, episode_length_toler: float) -> int:
        """``floor(ceil(episode_length_s / dt) * (1 - toler))``: for a whole ``steps``, ``steps > that`` is the reference's comparison at
        t1.py:394-396"""
        return int(np.floor(np.ceil(episode_length_s / dt) * (1 - episode_length_toler)))

    def set_commands(self, lin_vel_x, lin_vel_y, ang_vel_yaw, gait_frequency, resample_steps, *, still_proportion: float = 0.0,
                     tracking_sigma: float = 0.25, scales=None, obs_scales=None, curriculum=None, keep_state: bool = False) -> None:
        """Configures the velocity commands: the three command ranges and the gait-frequency range ``(lower, upper)``, ``resample_steps
        (lo, hi)`` -- the caller's ``int(resampling_time_s / dt)`` pair --, ``still_proportion``, ``tracking_sigma``, ``scales`` -- four
        numbers or a dict over :data:`CMD_TERMS` that weigh ``total`` (zero, the default: the term stays out) --, ``obs_scales`` (``lin_vel,
        lin_vel, ang_vel`` of the normalisation) and, optionally, ``curriculum``: a dict of ``lin_vel_levels``, ``ang_vel_levels`` (0 to
        20), ``update_rate``, ``tolerances`` and ``resolutions`` (x, y, yaw), ``min_success_steps`` (:meth:`min_success_steps`) and
        ``index_order`` -- ``"grid"`` (default) or ``"reference"``, the reference's transposed split of a drawn cell, only for equal level
        counts.  Allocates the state (zeros; the centre cell of ``curriculum_prob`` is 1).  With ``keep_state`` only the configuration is
        replaced -- calls already enqueued keep theirs --, and the curriculum's presence and level counts must stay.  Synchronous."""
        c = self._commands_setup(lin_vel_x, lin_vel_y, ang_vel_yaw, gait_frequency, resample_steps, still_proportion, tracking_sigma, scales,
                                 obs_scales, curriculum)
        cur = c["curriculum"]
        shape = None if cur is None else (cur["L"], cur["A"])
        if keep_state:
            old = self._commands
            if old is None:
                raise ValueError("set_commands: keep_state needs commands that were set before")
            if old != (shape,):
                raise ValueError(f"set_commands: keep_state keeps the curriculum and its levels as they are, {old[0]} is set, {shape} given")
        cfg = _lib.CommandsConfig()
        for k in ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "gait_frequency"):
            getattr(cfg, k)[:] = c[k]
        cfg.resample_steps[:] = c["resample_steps"]
        cfg.still_proportion, cfg.tracking_sigma = c["still_proportion"], c["tracking_sigma"]
        cfg.scales[:] = c["scales"].tolist()
        cfg.obs_scale[:] = c["obs_scales"].tolist()
        if cur is not None:
            cfg.curriculum, cfg.lin_vel_levels, cfg.ang_vel_levels, cfg.update_rate = 1, cur["L"], cur["A"], cur["rate"]
            cfg.toler[:], cfg.resolution[:] = cur["tol"], cur["res"]
            cfg.min_success_steps, cfg.index_order = cur["min_success_steps"], _lib.CMD_INDEX_ORDERS[cur["order"]]
        _lib.check(_lib.lib().gmr_motion_tracker_set_commands(self.handle, C.byref(cfg), 1 if keep_state else 0))
        self._commands = (shape,)

    def _need_commands(self, what: str):
        c = self._commands
        if c is None:
            raise ValueError(f"{what}: commands are not set on this tracker, call set_commands() first")
        return c[0]

    def commands(self, episode_steps, done=None, lin_vel=None, ang_vel=None, cmd_obs=None) -> Dict[str, np.ndarray]:
        """The command half of a step, host arrays in and out: from ``episode_steps i32[N]`` (after the caller's increment, before any
        reset), the ``done`` mask (``None``: nobody resets) and the filtered velocities ``lin_vel``, ``ang_vel`` ``[N,3]`` of
        :meth:`proprio` (optional without a curriculum) -- ``term [N,4]`` in the order of :data:`CMD_TERMS` and ``total [N]`` for the
        commands of the episode that ends, then the curriculum's bookkeeping, the reset of the resample time of a done environment and the
        resample where the step count meets it; ``commands [N,3]``, ``gait_frequency [N]`` (what :meth:`feet` takes next step) and ``flags
        i32[N]`` (:data:`CMD_BOUNDARY`: OR it into the time-outs, :data:`CMD_RESAMPLED`, :data:`CMD_SUCCESS`).  ``cmd_obs`` is a host array
        ``[N,W]``, ``W >= 3``, or a pair ``(array, column)``: its three columns from ``column`` on get ``commands * obs_scales``, in place.
        One launch, three with a curriculum; clocks, clips and draw counters of the tracker stay as they are."""
        shape = self._need_commands("commands")
        N = self.num_envs
        if episode_steps is None:
            raise ValueError("commands: episode_steps is needed")
        ins = self._rows_of(_lib.CMD_IN)
        st, keep = _lib.host_inputs(_lib.CommandsIn, ins, {"episode_steps": episode_steps})
        m = _mask(done, "done", N)              # a mask may be bool: it goes in as 0 / 1
        if m is not None:
            st.done = m.ctypes.data
        if shape is not None and (lin_vel is None or ang_vel is None):
            raise ValueError("commands: the curriculum needs lin_vel and ang_vel (the filtered velocities)")
        st, held = _lib.host_inputs(st, ins, {"lin_vel": lin_vel, "ang_vel": ang_vel})
        table, out = _lib.host_outputs(_lib.CommandsOut, self._rows_of(_lib.CMD_OUT), skip=("cmd_obs",))
        if cmd_obs is not None:
            rows, col = cmd_obs if isinstance(cmd_obs, tuple) else (cmd_obs, 0)
            if not (isinstance(rows, np.ndarray) and rows.dtype == np.float32 and rows.flags.c_contiguous and rows.flags.writeable and rows.ndim == 2
                    and rows.shape[0] == N):
                raise ValueError(f"cmd_obs: a writeable C-contiguous float32 array [N = {N}, W] is needed")
            if int(col) != col or not 0 <= col <= rows.shape[1] - 3:
                raise ValueError(f"cmd_obs: column {col} leaves no three columns in rows of {rows.shape[1]}")
            table.cmd_obs, table.cmd_obs_stride = rows.ctypes.data + 4 * int(col), rows.shape[1]
        _lib.check(_lib.lib().gmr_motion_tracker_commands(self.handle, C.byref(st), C.byref(table)))
        return out

    def commands_dev(self, episode_steps, done=None, lin_vel=None, ang_vel=None, cmd_obs=None, cmd_obs_stride: int = 3, stream=None,
                     **outputs) -> None:
        """:meth:`commands` on device memory, asynchronous on ``stream``: ONE launch, THREE with a curriculum, no host synchronisation.
        ``outputs`` names whichever of ``term, total, commands, gait_frequency, flags`` are wanted; ``cmd_obs`` is the address of the
        first command column of environment 0 (``obs + 6`` floats of the row of :meth:`proprio_dev`) and ``cmd_obs_stride`` the row's
        width in floats.  Every array is a ``_lib.DeviceBuffer``, a raw address or an object with ``data_ptr()``."""
        shape = self._need_commands("commands_dev")
        N = self.num_envs
        table = _lib.device_struct(_lib.CommandsOut, self._rows_of(_lib.CMD_OUT), outputs, "commands_dev")
        if episode_steps is None:
            raise ValueError("commands_dev: episode_steps is needed")
        if shape is not None and (lin_vel is None or ang_vel is None):
            raise ValueError("commands_dev: the curriculum needs lin_vel and ang_vel (the filtered velocities)")
        given = {"episode_steps": episode_steps, "done": done, "lin_vel": lin_vel, "ang_vel": ang_vel}
        st = _lib.device_struct(_lib.CommandsIn, self._rows_of(_lib.CMD_IN), given)
        if cmd_obs is not None:
            if int(cmd_obs_stride) != cmd_obs_stride or cmd_obs_stride < 3:
                raise ValueError(f"commands_dev: cmd_obs_stride = {cmd_obs_stride}, at least 3 floats needed")
            table.cmd_obs = _dev_ptr(cmd_obs, "cmd_obs", "float32", (N - 1) * int(cmd_obs_stride) + 3).value
            table.cmd_obs_stride = int(cmd_obs_stride)
        _lib.check(_lib.lib().gmr_motion_tracker_commands_dev(self.handle, C.byref(st), C.byref(table), _lib._s(stream)))

    def command_state(self) -> Optional[Dict[str, object]]:
        """``commands f32[N,3]``, ``gait_frequency f32[N]``, ``cmd_resample_time i32[N]``, ``cmd_draws u32[N]`` and, with a curriculum,
        ``env_level i32[N,2]``, ``curriculum_prob f32[2L+1,2A+1]``, ``hits u32[G]``, ``cum f64[G+1]`` and -- formed here from ``env_level``
        -- ``mean_lin_vel_level``, ``mean_ang_vel_level``, ``max_lin_vel_level``, ``max_ang_vel_level`` (t1.py:421-424); ``None`` when the
        commands are not set.  Synchronous."""
        if self._commands is None:
            return None
        shape = self._need_commands("command_state")
        N = self.num_envs
        out = {"commands": np.empty((N, 3), np.float32), "gait_frequency": np.empty(N, np.float32), "cmd_resample_time": np.empty(N, np.int32),
               "cmd_draws": np.empty(N, np.uint32)}
        if shape is not None:
            nx, ny = 2 * shape[0] + 1, 2 * shape[1] + 1
            out.update({"env_level": np.empty((N, 2), np.int32), "curriculum_prob": np.empty((nx, ny), np.float32), "hits": np.empty(nx * ny, np.uint32),
                        "cum": np.empty(nx * ny + 1, np.float64)})
        ptrs = [_lib._ptr(out.get(k)) for k in COMMAND_STATE]
        _lib.check(_lib.lib().gmr_motion_tracker_command_state(self.handle, *ptrs))
        if shape is not None:
            mag = np.abs(out["env_level"])
            out["mean_lin_vel_level"], out["mean_ang_vel_level"] = (float(np.mean(mag[:, k].astype(np.float32))) for k in (0, 1))
            out["max_lin_vel_level"], out["max_ang_vel_level"] = int(mag[:, 0].max()), int(mag[:, 1].max())
        return out

    @staticmethod
    def disturb_actions(common_step: int, kick_every: int, push_every: int, push_duration: int) -> int:
        """What ``common_step`` does (t1.py:501, :508, :517): :data:`DISTURB_KICK` | :data:`DISTURB_PUSH_START` | :data:`DISTURB_PUSH_STOP`;
        a stop is the ``elif`` of a start.  The library decides by the same rule."""
        act = DISTURB_KICK if common_step % kick_every == 0 else 0
        if common_step % push_every == 0:
            act |= DISTURB_PUSH_START
        elif common_step % push_every == push_duration:
            act |= DISTURB_PUSH_STOP
        return act

    @staticmethod
    def _disturb_setup(kick_lin_vel, kick_ang_vel, push_force, push_torque, kick_every, push_every, push_duration, scale_push_force,
                       scale_push_torque):
        """the checks of :meth:`set_disturbances`, all of them before the library is loaded -> a dict of the checked values"""
        specs = [MotionTracker._noise_spec(k, s) for k, s in zip(DISTURB_SPECS, (kick_lin_vel, kick_ang_vel, push_force, push_torque))]
        for k, v, least in (("kick_every", kick_every, 1), ("push_every", push_every, 1), ("push_duration", push_duration, 0)):
            if int(v) != v or not least <= v < 2 ** 31:
                raise ValueError(f"{k} = {v}: a whole number of steps, at least {least}, is needed (the caller's ceil(seconds / dt))")
        with np.errstate(over="ignore"):
            sf, st = float(np.float32(scale_push_force)), float(np.float32(scale_push_torque))
        if not (np.isfinite(sf) and np.isfinite(st)):
            raise ValueError(f"scale_push_force = {scale_push_force} and scale_push_torque = {scale_push_torque} must be finite")
        return {"specs": specs, "periods": (int(kick_every), int(push_every), int(push_duration)), "scales": (sf, st)}

    def set_disturbances(self, kick_every: int, push_every: int, push_duration: int, *, kick_lin_vel=None, kick_ang_vel=None, push_force=None,
                         push_torque=None, scale_push_force: float = 1.0, scale_push_torque: float = 1.0) -> None:
        """Configures kicks and pushes: the three periods in steps (``ceil(seconds / dt)``), four specs in the form of the ``noise`` of
        :meth:`set_proprio` (``None``: the block is left alone) and the two privileged-observation scales.  Keeps no device state."""
        c = self._disturb_setup(kick_lin_vel, kick_ang_vel, push_force, push_torque, kick_every, push_every, push_duration, scale_push_force,
                                scale_push_torque)
        cfg = _lib.DisturbConfig()
        for k, (dist, op, a, b) in zip(DISTURB_SPECS, c["specs"]):
            s = getattr(cfg, k)
            s.distribution, s.operation, s.a, s.b = dist, op, a, b
        cfg.kick_every, cfg.push_every, cfg.push_duration = c["periods"]
        cfg.scale_push_force, cfg.scale_push_torque = c["scales"]
        _lib.check(_lib.lib().gmr_motion_tracker_set_disturbances(self.handle, C.byref(cfg)))
        self._disturb = c["periods"]

    def _need_disturb(self, what: str, common_step):
        if self._disturb is None:
            raise ValueError(f"{what}: disturbances are not set on this tracker, call set_disturbances() first")
        if int(common_step) != common_step or not 0 <= common_step < 2 ** 32:
            raise ValueError(f"{what}: common_step = {common_step}, a step count in [0, 2^32) is needed")
        return int(common_step)

    def disturb(self, common_step: int, root_states) -> Dict[str, object]:
        """Kicks and pushes at ``common_step``, host arrays: ``actions`` (the bits of :meth:`disturb_actions`), ``root_states [N,13]`` (a
        copy, columns 7 to 12 kicked on a kick step) and, on a step that starts or stops a push, ``push_force``, ``push_torque`` ``[N,3]``
        and ``push_obs [N,6]`` (zeros at a stop; ``None`` on other steps).  One launch, none on an idle step."""
        step = self._need_disturb("disturb", common_step)
        rows = self._rows_of(_lib.DISTURB_IO)
        rs = np.array(root_states, dtype=np.float32, order="C")
        if rs.shape != rows["root_states"][1]:
            raise ValueError(f"root_states: shape {rs.shape}, {rows['root_states'][1]} needed")
        out = {k: np.zeros(rows[k][1], np.float32) for k in ("push_force", "push_torque", "push_obs")}
        io = _lib.DisturbIo(root_states=rs.ctypes.data, push_force_stride=3, push_torque_stride=3, **{k: a.ctypes.data for k, a in out.items()})
        act = _lib.lib().gmr_motion_tracker_disturb(self.handle, step, C.byref(io))
        if act < 0:
            _lib.check(act)
        if not act & (DISTURB_PUSH_START | DISTURB_PUSH_STOP):
            out = dict.fromkeys(out)
        return {"actions": int(act), "root_states": rs, **out}

    def disturb_dev(self, common_step: int, root_states=None, push_force=None, push_torque=None, push_obs=None, push_force_stride: int = 3,
                    push_torque_stride: int = 3, stream=None) -> int:
        """:meth:`disturb` on device memory, asynchronous on ``stream``: ONE launch, none on an idle step.  ``root_states f32[N*13]`` is
        kicked in place; ``push_force`` / ``push_torque`` are the addresses of the base body's row of environment 0 (``forces + base_body *
        3`` floats) with the environment's row stride in floats (``num_bodies * 3``), so the push lands in the simulator's ``[N, nb, 3]``
        tensors; ``push_obs f32[N*6]``.  Returns the bits of :meth:`disturb_actions`: with :data:`DISTURB_KICK` hand ``root_states`` back
        to the simulator."""
        step = self._need_disturb("disturb_dev", common_step)
        N = self.num_envs
        io = _lib.device_struct(_lib.DisturbIo, self._rows_of(_lib.DISTURB_IO), {"root_states": root_states, "push_obs": push_obs})
        for k, x, stride in (("push_force", push_force, push_force_stride), ("push_torque", push_torque, push_torque_stride)):
            if x is None:
                continue
            if int(stride) != stride or stride < 3:
                raise ValueError(f"disturb_dev: {k}_stride = {stride}, at least 3 floats needed")
            setattr(io, k, _dev_ptr(x, k, "float32", (N - 1) * int(stride) + 3).value)
            setattr(io, k + "_stride", int(stride))
        if self.disturb_actions(step, *self._disturb) & DISTURB_KICK and root_states is None:
            raise ValueError("disturb_dev: a kick step needs root_states")
        act = _lib.lib().gmr_motion_tracker_disturb_dev(self.handle, step, C.byref(io), _lib._s(stream))
        if act < 0:
            _lib.check(act)
        return int(act)

    # ---- reset states, the reward total and the episode statistics ----------------------------------------
    @staticmethod
    def _noise_spec(name: str, spec):
        """one spec in the form of the ``noise`` of :meth:`set_proprio` -> ``(distribution, operation, a, b)``, checked"""
        if spec is None or spec.get("distribution", "none") == "none":
            return (0, 0, 0.0, 0.0)
        dist, op = spec.get("distribution"), spec.get("operation")
        if dist not in NOISE_DISTRIBUTIONS:
            raise ValueError(f"{name}: distribution is one of {sorted(NOISE_DISTRIBUTIONS)}, got {dist!r}")
        if op not in NOISE_OPERATIONS:
            raise ValueError(f"{name}: operation is one of {sorted(NOISE_OPERATIONS)}, got {op!r}")
        rng = spec.get("range")
        if rng is None or len(rng) != 2:
            raise ValueError(f"{name}: range is a pair, got {rng!r}")
        a, b = float(rng[0]), float(rng[1])
        with np.errstate(over="ignore", invalid="ignore"):
            fits = all(np.isfinite(np.float32(x)) for x in (a, b, b - a))
        if not fits:
            raise ValueError(f"{name}: range {(a, b)} is not finite in float32")
        if dist == "gaussian" and b < 0:
            raise ValueError(f"{name}: a gaussian's deviation {b} is negative")
        return (NOISE_DISTRIBUTIONS[dist], NOISE_OPERATIONS[op], a, b)

    def _reset_setup(self, base_init_state, default_dof_pos, env_origins, init_dof_pos, init_base_pos_xy, init_base_lin_vel_xy, yaw_range,
                     decimation, use_terrain):
        """the checks of :meth:`set_reset_states`, all of them before the library is loaded -> a dict of the checked values"""
        N, R = self.num_envs, self.nrobot_dof
        with np.errstate(over="ignore"):
            base = np.ascontiguousarray(base_init_state, dtype=np.float32).reshape(-1)
            q0 = np.ascontiguousarray(default_dof_pos, dtype=np.float32).reshape(-1)
        if len(base) != 13 or not np.isfinite(base).all():
            raise ValueError(f"base_init_state: 13 finite numbers (pos, quat xyzw, lin vel, ang vel), got {len(base)}")
        if len(q0) != R or not np.isfinite(q0).all():
            raise ValueError(f"default_dof_pos: {R} finite numbers needed, one per robot dof, got {len(q0)}")
        org = None
        if env_origins is not None:
            with np.errstate(over="ignore"):
                org = np.ascontiguousarray(env_origins, dtype=np.float32)
            if org.ndim == 2 and org.shape == (N, 3):
                org = np.ascontiguousarray(org[:, :2])
            if org.shape != (N, 2) or not np.isfinite(org).all():
                raise ValueError(f"env_origins: finite numbers of shape {(N, 2)} (or {(N, 3)}) needed, got {org.shape}")
        specs = [self._noise_spec(k, s) for k, s in zip(RESET_SPECS, (init_dof_pos, init_base_pos_xy, init_base_lin_vel_xy))]
        yaw = None
        if yaw_range is not None:
            if len(yaw_range) != 2:
                raise ValueError(f"yaw_range: a pair (lower, upper) or None, got {yaw_range!r}")
            lo, hi = float(yaw_range[0]), float(yaw_range[1])
            with np.errstate(over="ignore", invalid="ignore"):
                fits = all(np.isfinite(np.float32(x)) for x in (lo, hi, hi - lo))
            if not fits:
                raise ValueError(f"yaw_range {(lo, hi)} is not finite in float32")
            if hi < lo:
                raise ValueError(f"yaw_range: upper = {hi} < lower = {lo}")
            yaw = (lo, hi)
        if int(decimation) != decimation or not 0 <= decimation <= CONTROL_MAX_DECIMATION:
            raise ValueError(f"decimation = {decimation}: a whole number in [0, {CONTROL_MAX_DECIMATION}] is needed (0: no delay draw)")
        return {"base": base, "default_dof_pos": q0, "env_origins": org, "specs": specs, "yaw": yaw, "decimation": int(decimation),
                "use_terrain": bool(use_terrain)}

    def set_reset_states(self, base_init_state, default_dof_pos, *, env_origins=None, init_dof_pos=None, init_base_pos_xy=None,
                         init_base_lin_vel_xy=None, yaw_range=(0.0, 2.0 * np.pi), decimation: int = 0, use_terrain: bool = True) -> None:
        """Configures the reset states (t1.py:316-340): ``base_init_state [13]`` (pos, quat xyzw, lin vel, ang vel), ``default_dof_pos
        [R]``, optionally ``env_origins [N,2]`` (copied to the device), three specs in the form of the ``noise`` of :meth:`set_proprio`
        (``None``: no draw for that block), ``yaw_range (lower, upper)`` (``None``: no yaw draw, the row's quaternion stays), ``decimation``
        -- ``delay_steps`` is drawn below it, 0: no draw -- and ``use_terrain`` (the height of :meth:`set_terrain` under the drawn point is
        added to ``z``).  Allocates ``reset_draws`` (zeros).  Synchronous."""
        c = self._reset_setup(base_init_state, default_dof_pos, env_origins, init_dof_pos, init_base_pos_xy, init_base_lin_vel_xy, yaw_range,
                              decimation, use_terrain)
        cfg = _lib.ResetConfig()
        cfg.base_init_state[:] = c["base"].tolist()
        cfg.default_dof_pos = c["default_dof_pos"].ctypes.data
        if c["env_origins"] is not None:
            cfg.env_origins = c["env_origins"].ctypes.data
        for k, (dist, op, a, b) in zip(RESET_SPECS, c["specs"]):
            s = getattr(cfg, k)
            s.distribution, s.operation, s.a, s.b = dist, op, a, b
        if c["yaw"] is not None:
            cfg.yaw, cfg.yaw_range[0], cfg.yaw_range[1] = 1, c["yaw"][0], c["yaw"][1]
        cfg.decimation, cfg.use_terrain = c["decimation"], int(c["use_terrain"])
        _lib.check(_lib.lib().gmr_motion_tracker_set_reset_states(self.handle, C.byref(cfg)))
        self._resets = (self.nrobot_dof, c["decimation"])

    def _need_resets(self, what: str):
        r = self._resets
        if r is None:
            raise ValueError(f"{what}: reset states are not set on this tracker, call set_reset_states() first")
        if r[0] != self.nrobot_dof:
            raise ValueError(f"{what}: reset states were set for {r[0]} robot dofs, the dof map now has {self.nrobot_dof}: call "
                             "set_reset_states() again")
        return r

    def reset_states(self, root_states, dof_pos, dof_vel, mask=None, env_ids=None, delay_steps=None, episode_steps=None, init_root_states=None,
                     init_dof_pos=None, init_dof_vel=None, chain: bool = False) -> Dict[str, object]:
        """``_reset_dofs``, ``_reset_root_states`` and the ``delay_steps`` draw (t1.py:316-340) for every entry whose ``mask`` is set
        (``None``: all), host arrays: copies of ``root_states [N,13]``, ``dof_pos``, ``dof_vel`` ``[N,R]`` and, when given, ``delay_steps``
        and ``episode_steps`` ``i32[N]`` with the rows of the served environments rewritten, and ``ignored``: how many ids of served
        entries lay outside ``[0, num_envs)``.  Without ``env_ids`` the mask and the ``init_*`` rows cover every environment; with it
        (every environment at most once) they are indexed by list position, as the masks of :meth:`reset_done` are.  ``init_root_states
        [n,13]``, ``init_dof_pos``, ``init_dof_vel`` ``[n,R]`` take the place of ``base_init_state``, ``default_dof_pos`` and the zero
        velocity of that entry -- the rows of ``step_links(advance=False)`` can be fed in.  With ``chain`` the same launch also does what
        :meth:`hold` and :meth:`proprio_reset` would do afterwards, for the halves that are configured.  One launch."""
        self._need_resets("reset_states")
        n, ids, m = self._subset("reset_states", env_ids, mask)
        rows = _lib.resolve(_lib.RESET_IO, N=self.num_envs, n=n, R=self.nrobot_dof)
        rs = np.array(root_states, dtype=np.float32, order="C")
        if rs.shape != rows["root_states"][1]:
            raise ValueError(f"root_states: shape {rs.shape}, {rows['root_states'][1]} needed")
        out = {"root_states": rs, "dof_pos": self._rows(dof_pos, "dof_pos").copy(), "dof_vel": self._rows(dof_vel, "dof_vel").copy()}
        for k, a in (("delay_steps", delay_steps), ("episode_steps", episode_steps)):
            if a is not None:
                out[k] = self._per_env_ints(a, k).copy()
        io = _lib.ResetIo(**{k: a.ctypes.data for k, a in out.items()})               # copies: the caller's arrays stay as they are
        io, keep = _lib.host_inputs(io, rows, {"init_root_states": init_root_states, "init_dof_pos": init_dof_pos, "init_dof_vel": init_dof_vel})
        ignored = C.c_int()
        if n > 0:
            _lib.check(_lib.lib().gmr_motion_tracker_reset_states(self.handle, n, _lib._ptr(ids), _lib._ptr(m), C.byref(io), 1 if chain else 0,
                                                                  C.byref(ignored)))
        out["ignored"] = int(ignored.value)
        return out

    def reset_states_dev(self, root_states, dof_pos, dof_vel, mask=None, env_ids=None, n: Optional[int] = None, delay_steps=None,
                         episode_steps=None, init_root_states=None, init_dof_pos=None, init_dof_vel=None, chain: bool = False, stream=None) -> None:
        """:meth:`reset_states` on device memory, asynchronous on ``stream``: ONE launch, no ``nonzero``, no compaction, no read-back.
        ``root_states f32[N*13]``, ``dof_pos`` / ``dof_vel f32[N*R]``, ``delay_steps`` / ``episode_steps i32[N]`` are the simulator's own
        arrays, written in place in the rows of served entries; ``mask i32[n]`` as a step leaves it (``reset`` of :meth:`rewards_dev`); the
        ``init_*`` rows by list position; with ``env_ids`` (``i32[n]``) ``n`` is mandatory."""
        self._need_resets("reset_states_dev")
        n, p_ids, p_mask = self._subset("reset_states_dev", env_ids, mask, n, device=True)
        if root_states is None or dof_pos is None or dof_vel is None:
            raise ValueError("reset_states_dev: root_states, dof_pos and dof_vel are needed")
        given = {"root_states": root_states, "dof_pos": dof_pos, "dof_vel": dof_vel, "delay_steps": delay_steps, "episode_steps": episode_steps,
                 "init_root_states": init_root_states, "init_dof_pos": init_dof_pos, "init_dof_vel": init_dof_vel}
        io = _lib.device_struct(_lib.ResetIo, _lib.resolve(_lib.RESET_IO, N=self.num_envs, n=n, R=self.nrobot_dof), given)
        _lib.check(_lib.lib().gmr_motion_tracker_reset_states_dev(self.handle, n, p_ids, p_mask, C.byref(io), 1 if chain else 0, _lib._s(stream)))

    def reset_state(self) -> Optional[Dict[str, np.ndarray]]:
        """``reset_draws u32[N]``: the resets drawn for every environment so far; ``None`` when the reset states are not set.  Synchronous."""
        if self._resets is None:
            return None
        out = {"reset_draws": np.empty(self.num_envs, np.uint32)}
        _lib.check(_lib.lib().gmr_motion_tracker_reset_state(self.handle, _lib._ptr(out["reset_draws"])))
        return out

    def _reward_blocks(self):
        """the blocks configured on this tracker, in column order -> [(block, names)]"""
        blocks = [("terms", TERMS)]
        if self._links is not None:
            blocks.append(("links", LINK_TERMS))
        if self._proprio is not None:
            blocks.append(("proprio", PROPRIO_TERMS))
        if self._feet is not None:
            blocks.append(("feet", FEET_TERMS))
        if self._commands is not None:
            blocks.append(("commands", CMD_TERMS))
        return blocks

    def _rewards_setup(self, extra_names, extra_weights, groups, group_weight, only_positive, stats):
        """the checks of :meth:`set_rewards`, all of them before the library is loaded -> a dict of the checked values"""
        blocks = self._reward_blocks()
        names = [k for _, ks in blocks for k in ks]
        default = [REWARD_IMITATION if b in ("terms", "links") else REWARD_LOCOMOTION for b, ks in blocks for _ in ks]
        extra_names = [] if extra_names is None else [str(k) for k in extra_names]
        E = len(extra_names)
        if E > REWARD_MAX_EXTRA:
            raise ValueError(f"extra_names: {E} caller columns, at most {REWARD_MAX_EXTRA}")
        if len(set(extra_names)) != E or set(extra_names) & set(names) or set(extra_names) & {"reward", "steps", "episodes"}:
            raise ValueError(f"extra_names {extra_names} must differ from one another, from the blocks' terms and from reward / steps / episodes")
        with np.errstate(over="ignore"):
            ew = np.ascontiguousarray([] if extra_weights is None else extra_weights, dtype=np.float32).reshape(-1)
        if extra_weights is None:
            ew = np.ones(E, np.float32)
        if len(ew) != E or not np.isfinite(ew).all():
            raise ValueError(f"extra_weights: {E} finite numbers needed, one per caller column, got {len(ew)}")
        names += extra_names
        default += [REWARD_LOCOMOTION] * E
        if groups is None:
            g = default
        elif isinstance(groups, dict):
            unknown = sorted(set(groups) - set(names))
            if unknown:
                raise KeyError(f"groups: unknown columns {unknown} (known: {names})")
            g = [groups.get(k, d) for k, d in zip(names, default)]
        else:
            g = list(groups)
            if len(g) != len(names):
                raise ValueError(f"groups has {len(g)} entries, there are {len(names)} columns: {names}")
        if any(int(x) != x or not 0 <= x <= (REWARD_LOCOMOTION | REWARD_IMITATION) for x in g):
            raise ValueError(f"groups: each entry is a mask of REWARD_LOCOMOTION = 1 and REWARD_IMITATION = 2, got {g}")
        with np.errstate(over="ignore"):
            gw = np.ascontiguousarray(group_weight, dtype=np.float32).reshape(-1)
        if len(gw) != 2 or not np.isfinite(gw).all():
            raise ValueError(f"group_weight: two finite numbers (locomotion, imitation), got {group_weight!r}")
        if only_positive is None or len(only_positive) != 2:
            raise ValueError(f"only_positive: a pair of flags (locomotion, imitation), got {only_positive!r}")
        return {"blocks": blocks, "names": names, "E": E, "extra_weights": ew, "groups": [int(x) for x in g], "group_weight": gw,
                "only_positive": (bool(only_positive[0]), bool(only_positive[1])), "stats": bool(stats)}

    def set_rewards(self, *, extra_names=None, extra_weights=None, groups=None, group_weight=(1.0, 1.0), only_positive=(False, False),
                    stats: bool = False) -> Dict[str, object]:
        """Configures the reward (t1.py:560-572, t1_imitation.py:323-352).  The columns are the term rows of the blocks configured on the
        tracker NOW, in fixed order -- :data:`TERMS`, :data:`LINK_TERMS`, :data:`PROPRIO_TERMS`, :data:`FEET_TERMS`, :data:`CMD_TERMS` --,
        then one caller column per name of ``extra_names`` (at most 16) weighed by ``extra_weights`` (default 1); call it again after a
        block is configured.  The weight of a block's column is the one the block is configured with, read when a call is enqueued.
        ``groups``: per column (a list, or a dict by name over the defaults) a mask of :data:`REWARD_LOCOMOTION` and
        :data:`REWARD_IMITATION`; by default the tracking terms feed the imitation group and everything else locomotion; 3 counts a column
        in both, which is the reference's double count.  ``group_weight (locomotion, imitation)``, ``only_positive`` a pair of flags.
        ``stats``: keep the Recorder's episode statistics (allocates and zeroes their state).  Returns :meth:`reward_layout`.  Synchronous."""
        c = self._rewards_setup(extra_names, extra_weights, groups, group_weight, only_positive, stats)
        cfg = _lib.RewardConfig()
        cfg.group_weight[:] = c["group_weight"].tolist()
        for k, w in enumerate(c["extra_weights"].tolist()):
            cfg.extra_weights[k] = w
        cfg.only_positive[:] = [int(x) for x in c["only_positive"]]
        cfg.blocks = sum(REWARD_BLOCKS[b] for b, _ in c["blocks"])
        cfg.extra_cols, cfg.stats = c["E"], int(c["stats"])
        for k, g in enumerate(c["groups"]):
            cfg.groups[k] = g
        _lib.check(_lib.lib().gmr_motion_tracker_set_rewards(self.handle, C.byref(cfg)))
        self._rewards = c
        return self.reward_layout()

    def _need_rewards(self, what: str, stats: bool = False):
        c = self._rewards
        if c is None:
            raise ValueError(f"{what}: rewards are not set on this tracker, call set_rewards() first")
        if [b for b, _ in c["blocks"]] != [b for b, _ in self._reward_blocks()]:
            raise ValueError(f"{what}: the blocks configured on the tracker changed since set_rewards(): call it again")
        if stats and not c["stats"]:
            raise ValueError(f"{what}: the episode statistics are off, call set_rewards(stats=True)")
        return c

    def reward_layout(self) -> Optional[Dict[str, object]]:
        """``names``: the columns in order; ``blocks``: ``{block: (first column, count)}`` (``extra`` among them); ``groups``; ``num_cols``;
        ``None`` when the rewards are not set"""
        c = self._rewards
        if c is None:
            return None
        blocks, at = {}, 0
        for b, ks in c["blocks"]:
            blocks[b] = (at, len(ks))
            at += len(ks)
        blocks["extra"] = (at, c["E"])
        return {"names": tuple(c["names"]), "blocks": blocks, "groups": tuple(c["groups"]), "num_cols": len(c["names"])}

    _REWARD_INPUTS = {"term": "terms", "link_term": "links", "proprio_term": "proprio", "feet_term": "feet", "cmd_term": "commands"}    # input: its block

    def _reward_io(self, what: str, given):
        """the checks of a reward call that need no device -> the rows of its two tables"""
        c = self._need_rewards(what)
        have = {b for b, _ in c["blocks"]}
        for k, b in self._REWARD_INPUTS.items():
            if given[k] is not None and b not in have:
                raise ValueError(f"{what}: {k} given, but the block {b!r} is not configured on this tracker")
        return self._rows_of(_lib.REWARD_IN, E=c["E"]), self._rows_of(_lib.REWARD_OUT, C=len(c["names"]))

    def rewards(self, term=None, link_term=None, proprio_term=None, feet_term=None, cmd_term=None, extra=None, done=None,
                flags=None) -> Dict[str, np.ndarray]:
        """The reward of a step, host arrays in and out: from the ``term`` arrays as the blocks' calls left them (``None`` keeps that
        block's columns out), the caller's ``extra [N,E]``, the ``done`` word (the OR of the done words of :meth:`proprio` and
        :meth:`feet`) and the ``flags`` of :meth:`commands` -- ``reward [N]``, ``scaled [N,C]`` (weight times term, what the reference puts
        into ``extras["rew_terms"]``), ``group_total [N,2]``, ``reset i32[N] = done != 0`` and ``time_outs i32[N] = ((done & 4) | (flags &
        CMD_BOUNDARY)) != 0``.  With ``stats`` the episode sums move on.  One launch, two with the statistics."""
        given = dict(term=term, link_term=link_term, proprio_term=proprio_term, feet_term=feet_term, cmd_term=cmd_term, extra=extra, done=done, flags=flags)
        ins, outs = self._reward_io("rewards", given)
        st, keep = _lib.host_inputs(_lib.RewardIn, ins, given)
        table, out = _lib.host_outputs(_lib.RewardOut, outs)
        _lib.check(_lib.lib().gmr_motion_tracker_rewards(self.handle, C.byref(st), C.byref(table)))
        return out

    def rewards_dev(self, term=None, link_term=None, proprio_term=None, feet_term=None, cmd_term=None, extra=None, done=None, flags=None,
                    stream=None, **outputs) -> None:
        """:meth:`rewards` on device memory, asynchronous on ``stream``: ONE launch, TWO with the statistics, no host synchronisation.
        ``outputs`` names whichever of ``reward, scaled, group_total, reset, time_outs`` are wanted.  Every array is a
        ``_lib.DeviceBuffer``, a raw address or an object with ``data_ptr()``."""
        given = dict(term=term, link_term=link_term, proprio_term=proprio_term, feet_term=feet_term, cmd_term=cmd_term, extra=extra, done=done, flags=flags)
        ins, outs = self._reward_io("rewards_dev", given)
        table = _lib.device_struct(_lib.RewardOut, outs, outputs, "rewards_dev")
        st = _lib.device_struct(_lib.RewardIn, ins, given)
        _lib.check(_lib.lib().gmr_motion_tracker_rewards_dev(self.handle, C.byref(st), C.byref(table), _lib._s(stream)))

    def reward_stats_dev(self, out=None, clear: bool = True, stream=None) -> None:
        """Copies the three accumulators of the episode statistics into ``out`` -- ``u64[C + 3]`` on the device: episodes, steps, then the
        ``C + 1`` sums as float64, the reward first -- and, with ``clear``, zeroes them, in one launch; asynchronous on ``stream``."""
        c = self._need_rewards("reward_stats_dev", stats=True)
        p = _dev_ptr(out, "out", "uint64", len(c["names"]) + 3)
        _lib.check(_lib.lib().gmr_motion_tracker_reward_stats_dev(self.handle, p, 1 if clear else 0, _lib._s(stream)))

    def reward_stats(self, clear: bool = True, raw: bool = False) -> Dict[str, object]:
        """What the reference's ``Recorder`` writes (recorder.py:55-62): ``episodes`` finished since the last clear, ``steps`` their mean
        length, ``reward`` and every column by name the mean of the episode sums; 0.0 when no episode finished, as ``_mean`` gives.  The
        division is made here, on the host.  With ``raw`` the accumulators themselves: ``episodes``, ``steps`` (their sum) and ``sums
        f64[C + 1]``.  With ``clear`` the accumulators are zeroed in the same launch.  Synchronous."""
        c = self._need_rewards("reward_stats", stats=True)
        K = len(c["names"]) + 1
        buf = np.zeros(K + 2, np.uint64)
        _lib.check(_lib.lib().gmr_motion_tracker_reward_stats(self.handle, _lib._ptr(buf), 1 if clear else 0))
        episodes, steps, sums = int(buf[0]), int(buf[1]), buf[2:].view(np.float64).copy()
        if raw:
            return {"episodes": episodes, "steps": steps, "sums": sums}
        out = {"episodes": episodes, "steps": steps / episodes if episodes else 0.0}
        for k, name in enumerate(["reward"] + list(c["names"])):
            out[name] = float(sums[k]) / episodes if episodes else 0.0
        return out

    def reward_state(self) -> Optional[Dict[str, np.ndarray]]:
        """``ep_steps i32[N]`` and ``ep_sum f32[N,C+1]`` (column 0 is the reward) of the open episodes; ``None`` without statistics.
        Synchronous."""
        c = self._rewards
        if c is None or not c["stats"]:
            return None
        N, K = self.num_envs, len(c["names"]) + 1
        out = {"ep_steps": np.empty(N, np.int32), "ep_sum": np.empty((N, K), np.float32)}
        _lib.check(_lib.lib().gmr_motion_tracker_reward_state(self.handle, _lib._ptr(out["ep_steps"]), _lib._ptr(out["ep_sum"])))
        return out

    # ---- rollout storage, GAE, returns and advantages ---------------------------------------------------------
    @staticmethod
    def _rollout_setup(horizon, obs_cols, priv_cols, act_cols, gamma, lam):
        """the checks of :meth:`set_rollout`, all of them before the library is loaded -> a dict of the checked values"""
        for k, v, least in (("horizon", horizon, 1), ("obs_cols", obs_cols, 1), ("priv_cols", priv_cols, 0), ("act_cols", act_cols, 1)):
            if isinstance(v, bool) or int(v) != v or v < least or v >= 2 ** 31:
                raise ValueError(f"set_rollout: {k} = {v!r}: a whole number of at least {least} is needed")
        for k, v in (("gamma", gamma), ("lam", lam)):
            v = float(v)
            if not np.isfinite(v) or not 0.0 <= v <= 1.0:
                raise ValueError(f"set_rollout: {k} = {v}: a finite number in [0, 1] is needed")
        return {"horizon": int(horizon), "obs_cols": int(obs_cols), "priv_cols": int(priv_cols), "act_cols": int(act_cols), "gamma": float(gamma),
                "lam": float(lam)}

    def set_rollout(self, horizon: int, obs_cols: int, priv_cols: int, act_cols: int, gamma: float, lam: float) -> Dict[str, object]:
        """Configures the rollout (runner.py:36-42, :141-142): ``horizon`` slots of ``num_envs`` rows with ``obs_cols``, ``priv_cols`` (0:
        no privileged observations) and ``act_cols`` columns, and the two discounts of the advantages, each in ``[0, 1]``.  The arrays stay
        the caller's; the tracker allocates the scratch of the partial sums.  Returns :meth:`rollout_state`.  Synchronous."""
        c = self._rollout_setup(horizon, obs_cols, priv_cols, act_cols, gamma, lam)
        _lib.check(_lib.lib().gmr_motion_tracker_set_rollout(self.handle, c["horizon"], c["obs_cols"], c["priv_cols"], c["act_cols"], c["gamma"],
                                                             c["lam"]))
        self._rollout = c
        return self.rollout_state()

    def rollout_state(self) -> Optional[Dict[str, object]]:
        """The rollout configuration -- ``horizon, obs_cols, priv_cols, act_cols, gamma, lam``, ``num_envs`` and ``shapes``, the shape of
        each of the caller's six arrays (``priv``: ``None`` without privileged observations) --; ``None`` when the rollout was never set"""
        c = self._rollout
        if c is None:
            return None
        H, N = c["horizon"], self.num_envs
        shapes = {"obs": (H, N, c["obs_cols"]), "priv": (H, N, c["priv_cols"]) if c["priv_cols"] else None, "actions": (H, N, c["act_cols"]),
                  "rewards": (H, N), "dones": (H, N), "time_outs": (H, N)}
        return dict(c, num_envs=N, shapes=shapes)

    def _need_rollout(self, what: str):
        c = self._rollout
        if c is None:
            raise ValueError(f"{what}: the rollout is not set on this tracker, call set_rollout() first")
        return c

    def _rollout_io(self, what: str, io, need, device: bool):
        """the caller's rollout arrays ``io`` (a dict) as a ``gmr_rollout_io_t``: the arrays named in ``need`` must be there -> (table, keep)"""
        c = self._need_rollout(what)
        rows = self._rows_of(_lib.ROLLOUT_IO, H=c["horizon"], O=c["obs_cols"], P=c["priv_cols"], A=c["act_cols"])
        unknown = sorted(set(io) - set(rows))
        if unknown:
            raise ValueError(f"{what}: unknown rollout arrays {unknown} (known: {sorted(rows)})")
        given = {k: io.get(k) for k in rows}
        for k, a in given.items():
            if a is None and k in need:
                raise ValueError(f"{what}: the rollout array {k!r} is needed")
            if a is not None and k == "priv" and c["priv_cols"] == 0:
                raise ValueError(f"{what}: {k} given, but the rollout was set with priv_cols = 0")
        if device:
            return c, _lib.device_struct(_lib.RolloutIo, rows, given), []
        table, keep = _lib.RolloutIo(), []
        for k, a in given.items():          # written in place: nothing is converted, so no host_inputs here
            if a is None:
                continue
            dt, shape, _ = rows[k]
            if not isinstance(a, np.ndarray) or a.dtype not in ((np.dtype(dt),) if dt == "float32" else (np.dtype(np.uint8), np.dtype(np.bool_))) \
                    or not a.flags.c_contiguous or not a.flags.writeable:
                raise TypeError(f"{what}: {k} is written in place: a writeable C-contiguous {dt} array is needed")
            if a.shape != shape:
                raise ValueError(f"{what}: {k}: shape {a.shape}, {shape} needed")
            keep.append(a)
            setattr(table, k, a.ctypes.data)
        return c, table, keep

    def _record_inputs(self, what: str, c, obs, priv, actions, reward, done, time_outs):
        if priv is not None and c["priv_cols"] == 0:
            raise ValueError(f"{what}: priv given, but the rollout was set with priv_cols = 0")
        return (("obs", obs, "float32", c["obs_cols"], "obs"), ("priv", priv, "float32", c["priv_cols"], "priv"),
                ("actions", actions, "float32", c["act_cols"], "actions"), ("reward", reward, "float32", 0, "rewards"),
                ("done", done, "int32", 0, "dones"), ("time_outs", time_outs, "int32", 0, "time_outs"))

    def _check_slot(self, what: str, c, n):
        if isinstance(n, bool) or int(n) != n or not 0 <= n < c["horizon"]:
            raise ValueError(f"{what}: slot n = {n!r} outside [0, {c['horizon']})")
        return int(n)

    def record(self, n: int, io, obs=None, priv=None, actions=None, reward=None, done=None, time_outs=None) -> None:
        """What the runner's six ``update_data`` calls of a step do (runner.py:107-108, :115-118), host arrays: slot ``n`` of the arrays of
        ``io`` -- a dict of NumPy arrays in the shapes of :meth:`rollout_state`, written in place -- receives ``obs [N,O]``, ``priv [N,P]``,
        ``actions [N,A]``, ``reward [N]`` and the ``done`` and ``time_outs`` words (integers or booleans, stored as 0 / 1 bytes).  An input that
        is ``None`` leaves its slot as it is.  One launch."""
        c = self._need_rollout("record")
        n = self._check_slot("record", c, n)
        inputs = self._record_inputs("record", c, obs, priv, actions, reward, done, time_outs)
        _, table, keep = self._rollout_io("record", io, {slot for _, a, _, _, slot in inputs if a is not None}, device=False)
        N, args = self.num_envs, []
        for k, a, dt, w, _ in inputs:
            if a is None:
                args.append(None)
                continue
            if dt == "int32":
                a = np.asarray(a)
                a = self._per_env_ints(a.astype(np.int32) if a.dtype == np.bool_ else a, k)
            else:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if a.shape != ((N, w) if w else (N,)):
                    raise ValueError(f"record: {k}: shape {a.shape}, {(N, w) if w else (N,)} needed")
            keep.append(a)
            args.append(_lib._ptr(a))
        _lib.check(_lib.lib().gmr_motion_tracker_record(self.handle, n, C.byref(table), *args))

    def record_dev(self, n: int, io, obs=None, priv=None, actions=None, reward=None, done=None, time_outs=None, stream=None) -> None:
        """:meth:`record` on device memory, asynchronous on ``stream``: ONE launch.  ``io`` is a dict of device arrays (``obs f32[H*N*O]``,
        ``priv``, ``actions``, ``rewards f32[H*N]``, ``dones`` / ``time_outs u8[H*N]``); ``done`` and ``time_outs`` are the ``i32[N]`` words
        :meth:`rewards_dev` writes (``reset``, ``time_outs``).  Every array is a ``_lib.DeviceBuffer``, a raw address or an object with
        ``data_ptr()``."""
        c = self._need_rollout("record_dev")
        n = self._check_slot("record_dev", c, n)
        inputs = self._record_inputs("record_dev", c, obs, priv, actions, reward, done, time_outs)
        _, table, _ = self._rollout_io("record_dev", io, {slot for _, a, _, _, slot in inputs if a is not None}, device=True)
        args = [_dev_ptr(a, k, dt, self.num_envs * max(w, 1)) for k, a, dt, w, _ in inputs]
        _lib.check(_lib.lib().gmr_motion_tracker_record_dev(self.handle, n, C.byref(table), *args, _lib._s(stream)))

    def advantages(self, io, values, last_values, normalize: bool = True) -> Dict[str, object]:
        """What a mini-epoch does before the loss (runner.py:135-145, utils.py:33-44), host arrays: the rewards of timed-out steps become
        the critic's ``values [H,N]`` -- written into ``io["rewards"]`` in place, as the reference mutates its buffer --, then
        ``advantages`` (``discount_values`` with ``last_values [N]``), ``returns = values + advantages`` and, with ``normalize``,
        ``normalized`` and ``stats`` -- ``S1, S2, mean, std`` as float64 -- of all ``H N`` advantages (the unbiased deviation: ``H N >= 2``).
        ``io`` needs ``rewards``, ``dones`` and ``time_outs``."""
        c = self._need_rollout("advantages")
        H, N = c["horizon"], self.num_envs
        if normalize and H * N < 2:
            raise ValueError(f"advantages: normalize with H * N = {H * N}: the unbiased deviation needs two advantages")
        _, table, keep = self._rollout_io("advantages", {k: io.get(k) for k in ("rewards", "dones", "time_outs")}, {"rewards", "dones", "time_outs"},
                                          device=False)
        v, lv = np.ascontiguousarray(values, dtype=np.float32), np.ascontiguousarray(last_values, dtype=np.float32)
        if v.shape != (H, N) or lv.shape != (N,):
            raise ValueError(f"advantages: values {v.shape} and last_values {lv.shape}, {(H, N)} and {(N,)} needed")
        res, out = _lib.host_outputs(_lib.RolloutOut, self._rows_of(_lib.ROLLOUT_OUT, H=H), skip=() if normalize else ("normalized", "stats"))
        _lib.check(_lib.lib().gmr_motion_tracker_advantages(self.handle, C.byref(table), _lib._ptr(v), _lib._ptr(lv), C.byref(res),
                                                            1 if normalize else 0))
        return out

    def advantages_dev(self, io, values, last_values, out, normalize: bool = True, stream=None) -> None:
        """:meth:`advantages` on device memory, asynchronous on ``stream``: the scan, then with ``normalize`` the normalisation (beyond
        ``64 * 64`` environments a chain of one workgroup between them); no host synchronisation.  ``io`` names ``rewards``, ``dones``,
        ``time_outs``; ``out`` names whichever of ``advantages``, ``returns``, ``normalized`` (``f32[H*N]``) and ``stats`` (``f64[4]``) are
        wanted; no output may overlap another one, ``values``, ``last_values`` or an array of ``io`` (nothing checks it).  A torch loop
        hands ``values.detach()`` and its buffers as they are: anything with ``data_ptr()`` is taken."""
        c = self._need_rollout("advantages_dev")
        H, N = c["horizon"], self.num_envs
        if normalize and H * N < 2:
            raise ValueError(f"advantages_dev: normalize with H * N = {H * N}: the unbiased deviation needs two advantages")
        res = _lib.device_struct(_lib.RolloutOut, self._rows_of(_lib.ROLLOUT_OUT, H=H), out, "advantages_dev")
        _, table, _ = self._rollout_io("advantages_dev", {k: io.get(k) for k in ("rewards", "dones", "time_outs")},
                                       {"rewards", "dones", "time_outs"}, device=True)
        if values is None or last_values is None:
            raise ValueError("advantages_dev: values and last_values are needed")
        _lib.check(_lib.lib().gmr_motion_tracker_advantages_dev(self.handle, C.byref(table), _dev_ptr(values, "values", "float32", H * N),
                                                                _dev_ptr(last_values, "last_values", "float32", N), C.byref(res),
                                                                1 if normalize else 0, _lib._s(stream)))

    # ---- the PPO loss head, its gradients and the KL step -------------------------------------------------------
    def _loss_setup(self, bound_coef, entropy_coef, desired_kl, learning_rate, e_clip, lr_min, lr_max, lr_factor):
        """the checks of :meth:`set_loss`, all of them before the library is loaded -> a dict of the checked values, rows and columns"""
        r = self._need_rollout("set_loss")
        if r["act_cols"] > _lib.LOSS_MAX_ACT:
            raise ValueError(f"set_loss: act_cols = {r['act_cols']}, at most {_lib.LOSS_MAX_ACT}")
        c = {k: float(v) for k, v in (("bound_coef", bound_coef), ("entropy_coef", entropy_coef), ("desired_kl", desired_kl),
                                      ("learning_rate", learning_rate), ("e_clip", e_clip), ("lr_min", lr_min), ("lr_max", lr_max),
                                      ("lr_factor", lr_factor))}
        for k, v in c.items():
            if not np.isfinite(v):
                raise ValueError(f"set_loss: {k} = {v}: a finite number is needed")
        for k in ("desired_kl", "learning_rate", "lr_min"):
            if c[k] <= 0.0:
                raise ValueError(f"set_loss: {k} = {c[k]}: a number above 0 is needed")
        if not 0.0 < c["e_clip"] < 1.0:
            raise ValueError(f"set_loss: e_clip = {c['e_clip']}: a number in (0, 1) is needed")
        if c["lr_min"] > c["lr_max"]:
            raise ValueError(f"set_loss: lr_min = {c['lr_min']} above lr_max = {c['lr_max']}")
        if c["lr_factor"] < 1.0:
            raise ValueError(f"set_loss: lr_factor = {c['lr_factor']}: at least 1 is needed")
        return dict(c, rows=r["horizon"] * self.num_envs, cols=r["act_cols"])

    def set_loss(self, bound_coef: float, entropy_coef: float, desired_kl: float, learning_rate: float, e_clip: float = 0.2, lr_min: float = 1e-5,
                 lr_max: float = 1e-2, lr_factor: float = 1.5) -> Dict[str, object]:
        """Configures the loss head (runner.py:156-161, :175-178, utils.py:47): the two coefficients, the clip of the surrogate, the rule of
        the learning rate and the rate it starts from, which the tracker keeps as one double on the device.  Needs :meth:`set_rollout`
        first -- the rows ``M = horizon * num_envs`` and the columns ``A = act_cols`` are its --, and again after a new ``set_rollout``.
        Returns :meth:`loss_state`.  Synchronous."""
        c = self._loss_setup(bound_coef, entropy_coef, desired_kl, learning_rate, e_clip, lr_min, lr_max, lr_factor)
        _lib.check(_lib.lib().gmr_motion_tracker_set_loss(self.handle, *(c[k] for k in _lib.LOSS_STATE)))
        self._loss = c
        return self.loss_state()

    def _need_loss(self, what: str):
        c = self._loss
        if self._need_rollout(what) is None or c is None:
            raise ValueError(f"{what}: the loss is not set on this tracker, call set_loss() first")
        r = self._rollout
        if (c["rows"], c["cols"]) != (r["horizon"] * self.num_envs, r["act_cols"]):
            raise ValueError(f"{what}: the rollout was set again after the loss, call set_loss() again")
        return c

    def loss_state(self) -> Optional[Dict[str, object]]:
        """The loss configuration as given, ``rows`` and ``cols``, and ``learning_rate`` as the last ``update_lr`` call left it on the
        device; ``None`` when the loss was never set.  Synchronises."""
        c = self._loss
        if c is None:
            return None
        out = np.empty(len(_lib.LOSS_STATE), np.float64)
        _lib.check(_lib.lib().gmr_motion_tracker_loss_state(self.handle, _lib._ptr(out)))
        return dict(c, **{k: float(v) for k, v in zip(_lib.LOSS_STATE, out)})

    def _loss_rows(self, c):
        return self._rows_of(_lib.LOSS_IN, M=c["rows"], A=c["cols"]), self._rows_of(_lib.LOSS_OUT, M=c["rows"], A=c["cols"])

    def _loss_array(self, what: str, rows, k: str, a):
        """a host input of the loss as float32: ``[M, ...]`` or, as the rollout lays it out, ``[H, N, ...]``"""
        a = np.ascontiguousarray(a, dtype=np.float32)
        _, shape, count = rows[k]
        H, N = self._rollout["horizon"], self.num_envs
        if a.size != count or a.shape not in (shape, (H, N) + shape[1:] if shape[0] == H * N else shape):
            raise ValueError(f"{what}: {k}: shape {a.shape}, {shape} needed")
        return a

    def _loss_in(self, what: str, c, inputs, update_lr, device: bool):
        """the inputs of a loss call (a dict) as a ``gmr_loss_in_t`` -> (table, keep)"""
        rows, _ = self._loss_rows(c)
        unknown = sorted(set(inputs) - set(rows))
        if unknown:
            raise TypeError(f"{what}: unknown inputs {unknown} (known: {list(rows)})")
        old = [inputs.get(k) is not None for k in ("old_loc", "old_logstd")]
        if old[0] != old[1]:
            raise ValueError(f"{what}: old_loc and old_logstd are given together, or neither")
        if update_lr and not old[0]:
            raise ValueError(f"{what}: update_lr without old_loc and old_logstd: there is no KL to drive the learning rate")
        table, keep = _lib.LossIn(), []
        for k in rows:
            a = inputs.get(k)
            if a is None:
                if k not in ("old_loc", "old_logstd"):
                    raise ValueError(f"{what}: the input {k!r} is needed")
                continue
            if device:
                setattr(table, k, _dev_ptr(a, k, "float32", rows[k][2]).value)
                continue
            keep.append(self._loss_array(what, rows, k, a))
            setattr(table, k, keep[-1].ctypes.data)
        return table, keep

    def log_prob(self, loc, logstd, actions) -> np.ndarray:
        """``old_actions_log_prob`` (runner.py:123-125), host arrays: ``loc`` and ``actions`` ``[M, A]`` (or ``[H, N, A]``), ``logstd [A]``
        -> ``f32[M]``, the log-probability of every row's action under ``Normal(loc, exp(logstd))``, summed over the columns."""
        c = self._need_loss("log_prob")
        rows, _ = self._loss_rows(c)
        args = [self._loss_array("log_prob", rows, k, a) for k, a in (("loc", loc), ("logstd", logstd), ("actions", actions))]
        out = np.empty(c["rows"], np.float32)
        _lib.check(_lib.lib().gmr_motion_tracker_log_prob(self.handle, *(_lib._ptr(a) for a in args), _lib._ptr(out)))
        return out

    def log_prob_dev(self, loc, logstd, actions, out, stream=None) -> None:
        """:meth:`log_prob` on device memory, asynchronous on ``stream``: ONE launch.  ``loc`` and ``actions`` ``f32[M*A]``, ``logstd
        f32[A]``, ``out f32[M]``; each a ``_lib.DeviceBuffer``, a raw address or an object with ``data_ptr()``."""
        c = self._need_loss("log_prob_dev")
        M, A = c["rows"], c["cols"]
        args = [_dev_ptr(a, k, "float32", n) for k, a, n in (("loc", loc, M * A), ("logstd", logstd, A), ("actions", actions, M * A), ("out", out, M))]
        if any(a is None for a in args):
            raise ValueError("log_prob_dev: loc, logstd, actions and out are needed")
        _lib.check(_lib.lib().gmr_motion_tracker_log_prob_dev(self.handle, *args, _lib._s(stream)))

    def loss(self, inputs, update_lr: bool = False) -> Dict[str, object]:
        """The loss head of a mini-epoch (runner.py:146-180 without the networks and the optimiser), host arrays.  ``inputs`` is a dict of
        ``loc [M, A]``, ``logstd [A]``, ``actions [M, A]``, ``old_log_prob``, ``values``, ``returns``, ``advantages`` (the normalised ones)
        ``[M]`` and, for the KL, ``old_loc [M, A]`` with ``old_logstd [A]``.  Returns ``grad_loc [M, A]``, ``grad_logstd [A]``, ``grad_values
        [M]`` -- the gradient of the loss with respect to the networks' outputs --, ``log_prob [M]`` and ``terms`` ``f64[8]``: value_loss,
        actor_loss, bound_loss, entropy, loss, kl_mean, the learning rate after this call, clip_fraction.  With ``update_lr`` the KL steps
        the learning rate the tracker keeps."""
        c = self._need_loss("loss")
        table, keep = self._loss_in("loss", c, inputs, update_lr, device=False)
        res, out = _lib.host_outputs(_lib.LossOut, self._loss_rows(c)[1])
        _lib.check(_lib.lib().gmr_motion_tracker_loss(self.handle, C.byref(table), C.byref(res), 1 if update_lr else 0))
        return out

    def loss_dev(self, inputs, out, update_lr: bool = False, stream=None) -> None:
        """:meth:`loss` on device memory, asynchronous on ``stream``: the pass over the rows and, when ``terms``, ``grad_logstd`` or
        ``update_lr`` are wanted, the fold -- at most TWO launches, no host synchronisation.  ``out`` names whichever of ``grad_loc``
        (``f32[M*A]``), ``grad_logstd`` (``f32[A]``), ``grad_values``, ``log_prob`` (``f32[M]``) and ``terms`` (``f64[8]``) are wanted; no
        output may overlap another one or an input (nothing checks it).  A torch loop hands ``loc.detach()``, ``model.logstd.detach()``
        and ``values.detach()`` as they are: anything with ``data_ptr()`` is taken."""
        c = self._need_loss("loss_dev")
        res = _lib.device_struct(_lib.LossOut, self._loss_rows(c)[1], out, "loss_dev")
        table, _ = self._loss_in("loss_dev", c, inputs, update_lr, device=True)
        _lib.check(_lib.lib().gmr_motion_tracker_loss_dev(self.handle, C.byref(table), C.byref(res), 1 if update_lr else 0, _lib._s(stream)))

    # ---- the clip of the gradient norm and the Adam step --------------------------------------------------------
    def _optimizer_setup(self, sizes, learning_rate, betas, eps, max_norm):
        """the checks of :meth:`set_optimizer`, all of them before the library is loaded -> a dict of the checked values"""
        what = "set_optimizer"
        try:
            sizes = tuple(int(n) for n in sizes)
        except TypeError:
            raise ValueError(f"{what}: sizes is a list of element counts, one per tensor") from None
        if not 1 <= len(sizes) <= _lib.OPT_MAX_TENSORS:
            raise ValueError(f"{what}: K = {len(sizes)} tensors, 1 .. {_lib.OPT_MAX_TENSORS} are taken")
        for k, n in enumerate(sizes):
            if not 1 <= n <= 1 << 40:
                raise ValueError(f"{what}: sizes[{k}] = {n}: at least 1 element is needed")
        if len(tuple(betas)) != 2:
            raise ValueError(f"{what}: betas = {betas}: two numbers are needed")
        b1, b2 = (float(b) for b in betas)
        for k, b in (("beta1", b1), ("beta2", b2)):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"{what}: {k} = {b}: a number in [0, 1) is needed")
        eps, max_norm = float(eps), float(max_norm)
        for k, v in (("eps", eps), ("max_norm", max_norm)):
            if not np.isfinite(v) or v <= 0.0:
                raise ValueError(f"{what}: {k} = {v}: a finite number above 0 is needed")
        if learning_rate is None:
            self._need_loss(f"{what}: learning_rate=None follows the loss block's rate")
        else:
            learning_rate = float(learning_rate)
            if not np.isfinite(learning_rate) or learning_rate <= 0.0:
                raise ValueError(f"{what}: learning_rate = {learning_rate}: a finite number above 0, or None, is needed")
        return {"sizes": sizes, "learning_rate": learning_rate, "betas": (b1, b2), "eps": eps, "max_norm": max_norm}

    def set_optimizer(self, sizes, *, learning_rate: Optional[float] = None, betas=(0.9, 0.999), eps: float = 1e-8, max_norm: float = 1.0) -> None:
        """Configures the optimiser of runner.py:33 with the clip of :164: ``torch.optim.Adam`` at torch's defaults over ``K = len(sizes)``
        tensors of ``sizes[k]`` float32 elements (at most 32 tensors), the total norm of the gradients clipped to ``max_norm``.  ``exp_avg``
        and ``exp_avg_sq`` live in the tracker, zero, at step 0.  ``learning_rate=None`` FOLLOWS the loss block (needs :meth:`set_loss`
        first): the optimiser keeps a rate of its own, which starts as the loss block's; a step uses it and then takes the loss block's
        current rate for the next step.  With ``loss_dev(update_lr=True)`` enqueued before the step in every mini-epoch this is the
        reference's order: the step of mini-epoch n runs at the rate the rule left at the end of mini-epoch n - 1 (runner.py:165 before
        :175-180).  A number fixes the rate; :meth:`set_loss` is not needed then.  Synchronous."""
        c = self._optimizer_setup(sizes, learning_rate, betas, eps, max_norm)
        n = np.array(c["sizes"], np.int64)
        lr = float("nan") if c["learning_rate"] is None else c["learning_rate"]
        _lib.check(_lib.lib().gmr_motion_tracker_set_optimizer(self.handle, len(n), _lib._ptr(n), lr, *c["betas"], c["eps"], c["max_norm"]))
        self._optim = c

    def _need_optimizer(self, what: str):
        c = self._optim
        if c is None:
            raise ValueError(f"{what}: the optimiser is not set on this tracker, call set_optimizer() first")
        if c["learning_rate"] is None:
            self._need_loss(f"{what}: the optimiser follows the loss block's rate")
        return c

    @staticmethod
    def _optimizer_lists(what: str, c, **lists):
        K = len(c["sizes"])
        out = []
        for name, x in lists.items():
            x = list(x)
            if len(x) != K:
                raise ValueError(f"{what}: {name} names {len(x)} tensors, the optimiser was set for K = {K}")
            out.append(x)
        return out

    def optimizer_step_dev(self, params, grads, info=None, stream=None) -> None:
        """``clip_grad_norm_`` and ``optimizer.step()`` (runner.py:164-165) on device memory, asynchronous on ``stream``: the norm pass, the
        fold and the update pass -- at most THREE launches, no host synchronisation, no copy.  ``params`` and ``grads`` are lists of ``K``
        tensors in the order of :meth:`set_optimizer` (``f32[sizes[k]]``; each a ``_lib.DeviceBuffer``, a raw address or an object with
        ``data_ptr()``: a torch loop hands ``[p.data for p in model.parameters()]`` and ``[p.grad for ...]``); ``None`` in ``grads`` skips
        the tensor, as ``p.grad is None`` does.  The gradients are only read: the clipped gradient is never stored.  ``info`` (``f64[4]`` on
        the device, optional) gets total_norm, coef, the rate used and the step count."""
        c = self._need_optimizer("optimizer_step_dev")
        params, grads = self._optimizer_lists("optimizer_step_dev", c, params=params, grads=grads)
        K = len(params)
        tp, tg = (C.c_void_p * K)(), (C.c_void_p * K)()
        for k, n in enumerate(c["sizes"]):
            p = _dev_ptr(params[k], f"params[{k}]", "float32", n)
            if p is None or not p.value:
                raise ValueError(f"optimizer_step_dev: params[{k}] is needed (a tensor is skipped through grads[{k}] = None)")
            g = _dev_ptr(grads[k], f"grads[{k}]", "float32", n)
            tp[k], tg[k] = p.value, None if g is None else g.value
        d_info = _dev_ptr(info, "info", "float64", len(_lib.OPT_INFO))
        _lib.check(_lib.lib().gmr_motion_tracker_optimizer_step_dev(self.handle, tp, tg, d_info, _lib._s(stream)))

    def optimizer_step(self, params, grads):
        """:meth:`optimizer_step_dev` on host arrays -> ``(the new parameters, a list of K arrays in the shapes given; info f64[4])``.  The
        arrays handed in are not written."""
        c = self._need_optimizer("optimizer_step")
        params, grads = self._optimizer_lists("optimizer_step", c, params=params, grads=grads)
        K = len(params)
        new, keep = [], []
        tp, tg = (C.c_void_p * K)(), (C.c_void_p * K)()
        for k, n in enumerate(c["sizes"]):
            if params[k] is None:
                raise ValueError(f"optimizer_step: params[{k}] is needed (a tensor is skipped through grads[{k}] = None)")
            p = np.array(params[k], dtype=np.float32, order="C")                  # (a copy: the step writes it)
            g = None if grads[k] is None else np.ascontiguousarray(grads[k], dtype=np.float32)
            for name, a in (("params", p), ("grads", g)):
                if a is not None and a.size != n:
                    raise ValueError(f"optimizer_step: {name}[{k}]: {a.size} elements, {n} needed")
            new.append(p)
            keep.append(g)
            tp[k], tg[k] = p.ctypes.data, None if g is None else g.ctypes.data
        info = np.empty(len(_lib.OPT_INFO), np.float64)
        _lib.check(_lib.lib().gmr_motion_tracker_optimizer_step(self.handle, tp, tg, _lib._ptr(info)))
        return new, info

    def optimizer_state(self) -> Optional[Dict[str, object]]:
        """``{"step": int, "exp_avg": [K arrays], "exp_avg_sq": [K arrays]}``, flat ``f32[sizes[k]]`` each: what the ``state`` of
        ``torch.optim.Adam.state_dict()`` holds per parameter (INTEGRATION.md has the mapping); ``None`` when the optimiser was never set.
        Synchronises."""
        c = self._optim
        if c is None:
            return None
        total = sum(c["sizes"])
        step, m, v = C.c_int64(0), np.empty(total, np.float32), np.empty(total, np.float32)
        _lib.check(_lib.lib().gmr_motion_tracker_optimizer_state(self.handle, C.byref(step), _lib._ptr(m), _lib._ptr(v)))
        cut = np.cumsum(c["sizes"])[:-1]
        return {"step": int(step.value), "exp_avg": np.split(m, cut), "exp_avg_sq": np.split(v, cut)}

    def load_optimizer_state(self, state) -> None:
        """Continues from a state :meth:`optimizer_state` returned (or one mapped from a reference checkpoint, runner.py:95): ``step >= 0``
        and ``K`` arrays each of ``exp_avg`` and ``exp_avg_sq``, of any shape with ``sizes[k]`` elements.  In follow mode the next step
        runs at the loss block's current rate.  Synchronous."""
        c = self._need_optimizer("load_optimizer_state")
        unknown = sorted(set(state) - {"step", "exp_avg", "exp_avg_sq"})
        if unknown or len(state) != 3:
            raise ValueError(f"load_optimizer_state: the state holds step, exp_avg and exp_avg_sq (got {sorted(state)})")
        step = int(state["step"])
        if step != state["step"] or not 0 <= step <= 1 << 40:
            raise ValueError(f"load_optimizer_state: step = {state['step']}: a whole number, at least 0, is needed")
        flat = []
        for name, x in zip(("exp_avg", "exp_avg_sq"), self._optimizer_lists("load_optimizer_state", c, exp_avg=state["exp_avg"], exp_avg_sq=state["exp_avg_sq"])):
            x = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in x]
            for k, (a, n) in enumerate(zip(x, c["sizes"])):
                if a.size != n:
                    raise ValueError(f"load_optimizer_state: {name}[{k}]: {a.size} elements, {n} needed")
            flat.append(np.concatenate(x))
        _lib.check(_lib.lib().gmr_motion_tracker_optimizer_load_state(self.handle, step, _lib._ptr(flat[0]), _lib._ptr(flat[1])))

    # ---- the forward pass of the actor and the critic -----------------------------------------------------------
    @staticmethod
    def _policy_hidden_widths(what: str, net: str, hidden):
        try:
            hidden = tuple(int(h) for h in hidden)
        except TypeError:
            raise ValueError(f"{what}: {net}_hidden is a list of widths") from None
        if not 1 <= len(hidden) <= _lib.POLICY_MAX_HIDDEN:
            raise ValueError(f"{what}: {net}_hidden names {len(hidden)} hidden layers, 1 .. {_lib.POLICY_MAX_HIDDEN} are taken")
        for l, h in enumerate(hidden):
            if not _lib.POLICY_WIDTH_STEP <= h <= _lib.POLICY_MAX_WIDTH or h % _lib.POLICY_WIDTH_STEP:
                raise ValueError(f"{what}: {net}_hidden[{l}] = {h}: a multiple of {_lib.POLICY_WIDTH_STEP} in {_lib.POLICY_WIDTH_STEP} .. "
                                 f"{_lib.POLICY_MAX_WIDTH} is needed")
        return hidden

    def _policy_setup(self, obs_cols, priv_cols, act_cols, actor_hidden, critic_hidden):
        """the checks of :meth:`set_policy`, all of them before the library is loaded -> a dict of the checked shapes, with ``sizes``, the
        element counts of the parameter list, and ``first``, where each network's ``(W, b)`` pairs start in it"""
        what = "set_policy"
        O, P, A = int(obs_cols), int(priv_cols), int(act_cols)
        if O < 1 or P < 0 or O + P > _lib.POLICY_MAX_IN:
            raise ValueError(f"{what}: obs_cols = {O} and priv_cols = {P}: an input width of 1 .. {_lib.POLICY_MAX_IN} is needed (obs_cols at least 1)")
        if not 1 <= A <= _lib.LOSS_MAX_ACT:
            raise ValueError(f"{what}: act_cols = {A}, 1 .. {_lib.LOSS_MAX_ACT} are taken")
        ah, ch = self._policy_hidden_widths(what, "actor", actor_hidden), self._policy_hidden_widths(what, "critic", critic_hidden)
        widths = {"critic": (O + P,) + ch + (1,), "actor": (O,) + ah + (A,)}
        sizes, first = [A], {}
        for net in ("critic", "actor"):
            first[net] = len(sizes)
            w = widths[net]
            for l in range(len(w) - 1):
                sizes += [w[l + 1] * w[l], w[l + 1]]
        return {"obs_cols": O, "priv_cols": P, "act_cols": A, "actor_hidden": ah, "critic_hidden": ch, "widths": widths, "sizes": tuple(sizes), "first": first}

    def set_policy(self, obs_cols: int, priv_cols: int, act_cols: int, actor_hidden=(256, 128, 128), critic_hidden=(256, 256, 128)) -> None:
        """Configures the two networks of the reference's ``ActorCritic(act_cols, obs_cols, priv_cols)`` (booster_gym/utils/model.py:9-27,
        the defaults are its widths): ELU MLPs of 1 .. 4 hidden layers, every width a multiple of 32 up to 256, the critic on ``obs`` and
        ``priv`` side by side (at most 512 columns together), at most 32 actions.  The parameters stay the caller's: every call takes the
        list ``[logstd, critic W, b, .., actor W, b, ..]`` -- ``list(model.parameters())``, the list :meth:`optimizer_step_dev` takes.  The
        tracker keeps one count of sampled actions per environment, zero after this call.  Synchronous."""
        c = self._policy_setup(obs_cols, priv_cols, act_cols, actor_hidden, critic_hidden)
        ah, ch = np.array(c["actor_hidden"], np.int32), np.array(c["critic_hidden"], np.int32)
        _lib.check(_lib.lib().gmr_motion_tracker_set_policy(self.handle, c["obs_cols"], c["priv_cols"], c["act_cols"], len(ah), _lib._ptr(ah), len(ch), _lib._ptr(ch)))
        self._policy = c

    def _need_policy(self, what: str):
        c = self._policy
        if c is None:
            raise ValueError(f"{what}: the policy is not set on this tracker, call set_policy() first")
        return c

    def _policy_rows(self, what: str, rows, sample: bool) -> int:
        M = self.num_envs if rows is None else int(rows)
        if M < 1:
            raise ValueError(f"{what}: rows = {rows}: at least 1 is needed")
        if sample and M != self.num_envs:
            raise ValueError(f"{what}: sample=True draws for the environments, row e is environment e: rows = {M}, num_envs = {self.num_envs}")
        return M

    @staticmethod
    def _policy_params(what: str, c, params, device: bool):
        """the parameter list as a table of K addresses -> (table, arrays to keep alive)"""
        try:
            params = list(params)
        except TypeError:
            raise ValueError(f"{what}: params is the list of the model's parameters") from None
        K = len(c["sizes"])
        if len(params) != K:
            raise ValueError(f"{what}: params names {len(params)} tensors, the policy was set for K = {K}")
        table, keep = (C.c_void_p * K)(), []
        for k, n in enumerate(c["sizes"]):
            if params[k] is None:
                raise ValueError(f"{what}: params[{k}] is needed")
            if device:
                table[k] = _dev_ptr(params[k], f"params[{k}]", "float32", n).value
                continue
            a = np.ascontiguousarray(params[k], dtype=np.float32)
            if a.size != n:
                raise ValueError(f"{what}: params[{k}]: {a.size} elements, {n} needed")
            keep.append(a)
            table[k] = a.ctypes.data
        return table, keep

    @staticmethod
    def _policy_hidden(what: str, c, net: str, hidden, M: int, device: bool):
        """the optional hidden activations of a network -> (table of L addresses or None, {layer: host array})"""
        widths = c["widths"][net][1:-1]
        if hidden is None:
            return None, {}
        if device:
            hidden = list(hidden)
            if len(hidden) != len(widths):
                raise ValueError(f"{what}: hidden names {len(hidden)} layers, the {net} has {len(widths)} hidden layers (None leaves one out)")
            table = (C.c_void_p * len(widths))()
            for l, h in enumerate(widths):
                p = _dev_ptr(hidden[l], f"hidden[{l}]", "float32", M * h)
                table[l] = None if p is None else p.value
            return table, {}
        out = {l: np.empty((M, h), np.float32) for l, h in enumerate(widths)}
        return (C.c_void_p * len(widths))(*(a.ctypes.data for a in out.values())), out

    def act_dev(self, params, obs, loc, actions=None, hidden=None, sample: bool = True, rows: Optional[int] = None, stream=None) -> None:
        """``model.act(obs)`` (model.py:29-32) on device memory, asynchronous on ``stream``: ONE launch, no host synchronisation.  ``obs
        f32[rows*obs_cols]`` -> ``loc f32[rows*act_cols]`` and, with ``sample``, ``actions = loc + exp(logstd) * r`` with the tracker's own
        Gaussian draw -- ``model.act(obs).sample()`` of runner.py:109-111; sampling needs ``rows == num_envs`` (the default) and advances every
        environment's count.  ``sample=False`` is ``model.act(obs).loc`` for any ``rows``: the old-policy pass over the whole buffer, and
        ``Runner.play``.  ``hidden`` is a list with one array ``f32[rows*h_l]`` or ``None`` per hidden layer, for the activations after each
        ELU.  ``params`` is the list of :meth:`set_policy`, read in place: an :meth:`optimizer_step_dev` before this call is seen by it.
        Every array is a ``_lib.DeviceBuffer``, a raw address or an object with ``data_ptr()``."""
        c = self._need_policy("act_dev")
        M = self._policy_rows("act_dev", rows, sample)
        A = c["act_cols"]
        table, _ = self._policy_params("act_dev", c, params, device=True)
        hid, _ = self._policy_hidden("act_dev", c, "actor", hidden, M, device=True)
        d_obs, d_loc = _dev_ptr(obs, "obs", "float32", M * c["obs_cols"]), _dev_ptr(loc, "loc", "float32", M * A)
        d_act = _dev_ptr(actions, "actions", "float32", M * A)
        if d_obs is None or d_loc is None or (sample and d_act is None):
            raise ValueError("act_dev: obs and loc are needed" + (", and actions with sample=True" if sample else ""))
        _lib.check(_lib.lib().gmr_motion_tracker_act_dev(self.handle, table, M, d_obs, d_loc, d_act if sample else None, hid, 1 if sample else 0, _lib._s(stream)))

    def act(self, params, obs, sample: bool = True, hidden: bool = False) -> Dict[str, object]:
        """:meth:`act_dev` on host arrays: ``obs [rows, obs_cols]`` -> ``{"loc": [rows, act_cols]}``, with ``sample`` also ``"actions"``, with
        ``hidden`` also ``"hidden"``, the list of every hidden layer's activations."""
        c = self._need_policy("act")
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        if obs.ndim != 2 or obs.shape[1] != c["obs_cols"]:
            raise ValueError(f"act: obs: shape {obs.shape}, (rows, {c['obs_cols']}) needed")
        M = self._policy_rows("act", obs.shape[0], sample)
        table, keep = self._policy_params("act", c, params, device=False)
        hid, hout = self._policy_hidden("act", c, "actor", True if hidden else None, M, device=False)
        out = {"loc": np.empty((M, c["act_cols"]), np.float32)}
        if sample:
            out["actions"] = np.empty((M, c["act_cols"]), np.float32)
        _lib.check(_lib.lib().gmr_motion_tracker_act(self.handle, table, M, _lib._ptr(obs), _lib._ptr(out["loc"]), _lib._ptr(out.get("actions")), hid,
                                                     1 if sample else 0))
        if hidden:
            out["hidden"] = list(hout.values())
        return out

    def values_dev(self, params, obs, priv, values, hidden=None, rows: Optional[int] = None, stream=None) -> None:
        """``model.est_value(obs, privileged_obs)`` (model.py:34-36) on device memory, asynchronous on ``stream``: ONE launch, the two
        inputs concatenated inside it.  ``obs f32[rows*obs_cols]``, ``priv f32[rows*priv_cols]`` (``None`` when ``priv_cols`` is 0) ->
        ``values f32[rows]``; ``rows`` defaults to ``num_envs``, the ``last_values`` pass of runner.py:133.  ``hidden`` and ``params`` as in
        :meth:`act_dev`."""
        c = self._need_policy("values_dev")
        M = self._policy_rows("values_dev", rows, False)
        table, _ = self._policy_params("values_dev", c, params, device=True)
        hid, _ = self._policy_hidden("values_dev", c, "critic", hidden, M, device=True)
        d_obs, d_val = _dev_ptr(obs, "obs", "float32", M * c["obs_cols"]), _dev_ptr(values, "values", "float32", M)
        d_priv = _dev_ptr(priv, "priv", "float32", M * c["priv_cols"])
        if d_obs is None or d_val is None or (c["priv_cols"] and d_priv is None):
            raise ValueError("values_dev: obs and values are needed" + (", and priv" if c["priv_cols"] else ""))
        _lib.check(_lib.lib().gmr_motion_tracker_values_dev(self.handle, table, M, d_obs, d_priv if c["priv_cols"] else None, d_val, hid, _lib._s(stream)))

    def values(self, params, obs, priv=None, hidden: bool = False) -> Dict[str, object]:
        """:meth:`values_dev` on host arrays: ``obs [rows, obs_cols]``, ``priv [rows, priv_cols]`` -> ``{"values": [rows]}``, with ``hidden``
        also ``"hidden"``."""
        c = self._need_policy("values")
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        if obs.ndim != 2 or obs.shape[1] != c["obs_cols"]:
            raise ValueError(f"values: obs: shape {obs.shape}, (rows, {c['obs_cols']}) needed")
        M = self._policy_rows("values", obs.shape[0], False)
        P = c["priv_cols"]
        if P:
            priv = np.ascontiguousarray(priv, dtype=np.float32) if priv is not None else None
            if priv is None or priv.shape != (M, P):
                raise ValueError(f"values: priv: shape {None if priv is None else priv.shape}, {(M, P)} needed")
        else:
            priv = None
        table, keep = self._policy_params("values", c, params, device=False)
        hid, hout = self._policy_hidden("values", c, "critic", True if hidden else None, M, device=False)
        out = {"values": np.empty(M, np.float32)}
        _lib.check(_lib.lib().gmr_motion_tracker_values(self.handle, table, M, _lib._ptr(obs), _lib._ptr(priv), _lib._ptr(out["values"]), hid))
        if hidden:
            out["hidden"] = list(hout.values())
        return out

    def policy_state(self) -> Optional[Dict[str, object]]:
        """The shapes :meth:`set_policy` was given, as the library holds them, ``tile``, the rows a workgroup owns, and ``counts u32[N]``,
        the actions sampled for every environment so far; ``None`` when the policy was never set.  Synchronises."""
        if self._policy is None:
            return None
        shape, counts = np.zeros(_lib.POLICY_SHAPE, np.int32), np.empty(self.num_envs, np.uint32)
        _lib.check(_lib.lib().gmr_motion_tracker_policy_state(self.handle, _lib._ptr(shape), _lib._ptr(counts)))
        s = [int(x) for x in shape]
        return {"obs_cols": s[0], "priv_cols": s[1], "act_cols": s[2], "actor_hidden": tuple(s[4:4 + s[3]]), "critic_hidden": tuple(s[9:9 + s[8]]),
                "tile": s[13], "counts": counts}

    # ---- the backward pass through the actor and the critic ----------------------------------------------------
    def _backward_setup(self, max_rows):
        """the checks of :meth:`set_backward`, all of them before the library is loaded"""
        c = self._need_policy("set_backward")
        M = int(max_rows)
        if M != max_rows or not 1 <= M <= _lib.POLICY_BWD_MAX_ROWS:
            raise ValueError(f"set_backward: max_rows = {max_rows}: a whole number in 1 .. {_lib.POLICY_BWD_MAX_ROWS} is needed")
        return {"max_rows": M, "policy": c}

    def set_backward(self, max_rows: int) -> Dict[str, int]:
        """Prepares ``loss.backward()`` through the two networks of :meth:`set_policy` for any ``rows`` in ``1 .. max_rows`` (at most
        131 072): one workspace for the partial sums of every weight and bias gradient of the larger network per chunk of 256 rows, and
        the tile tables of the weight-gradient launch.  Needs :meth:`set_policy` first, and again after a new ``set_policy``.  Returns
        :meth:`backward_state`.  Synchronous."""
        c = self._backward_setup(max_rows)
        _lib.check(_lib.lib().gmr_motion_tracker_set_backward(self.handle, c["max_rows"]))
        self._backward = c
        return self.backward_state()

    def _need_backward(self, what: str):
        p = self._need_policy(what)
        c = self._backward
        if c is None:
            raise ValueError(f"{what}: the backward pass is not set on this tracker, call set_backward() first")
        if c["policy"] is not p:
            raise ValueError(f"{what}: the policy was set again after the backward pass, call set_backward() again")
        return c, p

    def _backward_rows(self, what: str, c, rows) -> int:
        M = self.num_envs if rows is None else int(rows)
        if not 1 <= M <= c["max_rows"]:
            raise ValueError(f"{what}: rows = {M}: 1 .. max_rows = {c['max_rows']} are taken")
        return M

    @staticmethod
    def _backward_grads(what: str, p, net: str, grads):
        """the gradient list as a table of K addresses: the network's own entries are needed, the others are not looked at"""
        try:
            grads = list(grads)
        except TypeError:
            raise ValueError(f"{what}: grads is the list of the gradients, in the order of params") from None
        K = len(p["sizes"])
        if len(grads) != K:
            raise ValueError(f"{what}: grads names {len(grads)} tensors, the policy was set for K = {K}")
        table = (C.c_void_p * K)()
        first = p["first"][net]
        for k in range(first, first + 2 * (len(p["widths"][net]) - 1)):
            g = _dev_ptr(grads[k], f"grads[{k}]", "float32", p["sizes"][k])
            if g is None or not g.value:
                raise ValueError(f"{what}: grads[{k}] is needed: the {net}'s gradients are written in full")
            table[k] = g.value
        return table

    @staticmethod
    def _backward_layers(what: str, p, net: str, name: str, arrays, M: int):
        """``hidden`` or ``delta``: one device array per hidden layer, all of them needed"""
        widths = p["widths"][net][1:-1]
        try:
            arrays = list(arrays)
        except TypeError:
            raise ValueError(f"{what}: {name} is a list with one array per hidden layer") from None
        if len(arrays) != len(widths):
            raise ValueError(f"{what}: {name} names {len(arrays)} layers, the {net} has {len(widths)} hidden layers")
        table = (C.c_void_p * len(widths))()
        for l, h in enumerate(widths):
            a = _dev_ptr(arrays[l], f"{name}[{l}]", "float32", M * h)
            if a is None or not a.value:
                raise ValueError(f"{what}: {name}[{l}] is needed: the backward pass takes every layer")
            table[l] = a.value
        return table

    def act_backward_dev(self, params, grads, obs, hidden, grad_loc, delta, rows: Optional[int] = None, stream=None) -> None:
        """The actor's share of ``loss.backward()`` (runner.py:163) on device memory, asynchronous on ``stream``: THREE launches, no host
        synchronisation.  From ``grad_loc f32[rows*act_cols]`` (:meth:`loss_dev`), the ``hidden`` list :meth:`act_dev` wrote and ``obs``,
        ``grads[k]`` of every weight and bias of the actor is OVERWRITTEN (no ``zero_grad``); ``grads[0]`` and the critic's entries are
        not looked at.  ``params`` and ``grads`` are lists in the order of :meth:`set_policy`; ``delta`` is a list of caller-owned arrays
        ``f32[rows*h_l]``, one per hidden layer, which receive the gradient at each layer's pre-activation.  Any ``rows`` in
        ``1 .. max_rows`` (default ``num_envs``)."""
        what = "act_backward_dev"
        c, p = self._need_backward(what)
        M = self._backward_rows(what, c, rows)
        table, _ = self._policy_params(what, p, params, device=True)
        tg = self._backward_grads(what, p, "actor", grads)
        th, td = self._backward_layers(what, p, "actor", "hidden", hidden, M), self._backward_layers(what, p, "actor", "delta", delta, M)
        d_obs, d_g = _dev_ptr(obs, "obs", "float32", M * p["obs_cols"]), _dev_ptr(grad_loc, "grad_loc", "float32", M * p["act_cols"])
        if d_obs is None or d_g is None:
            raise ValueError(f"{what}: obs and grad_loc are needed")
        _lib.check(_lib.lib().gmr_motion_tracker_act_backward_dev(self.handle, table, tg, M, d_obs, th, d_g, td, _lib._s(stream)))

    def values_backward_dev(self, params, grads, obs, priv, hidden, grad_values, delta, rows: Optional[int] = None, stream=None) -> None:
        """The critic's share, as :meth:`act_backward_dev`: from ``grad_values f32[rows]``, the ``hidden`` list of :meth:`values_dev`,
        ``obs`` and ``priv`` (side by side, ``None`` when ``priv_cols`` is 0) to ``grads[k]`` of the critic's weights and biases."""
        what = "values_backward_dev"
        c, p = self._need_backward(what)
        M = self._backward_rows(what, c, rows)
        table, _ = self._policy_params(what, p, params, device=True)
        tg = self._backward_grads(what, p, "critic", grads)
        th, td = self._backward_layers(what, p, "critic", "hidden", hidden, M), self._backward_layers(what, p, "critic", "delta", delta, M)
        d_obs, d_g = _dev_ptr(obs, "obs", "float32", M * p["obs_cols"]), _dev_ptr(grad_values, "grad_values", "float32", M)
        d_priv = _dev_ptr(priv, "priv", "float32", M * p["priv_cols"])
        if d_obs is None or d_g is None or (p["priv_cols"] and d_priv is None):
            raise ValueError(f"{what}: obs and grad_values are needed" + (", and priv" if p["priv_cols"] else ""))
        _lib.check(_lib.lib().gmr_motion_tracker_values_backward_dev(self.handle, table, tg, M, d_obs, d_priv if p["priv_cols"] else None, th, d_g, td,
                                                                   _lib._s(stream)))

    def _backward_host(self, what: str, net: str, params, obs, priv, hidden, g_out):
        """the NumPy twin of either call -> ``{"grads": {k: array in the tensor's shape}, "delta": [one array per hidden layer]}``"""
        c, p = self._need_backward(what)
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        if obs.ndim != 2 or obs.shape[1] != p["obs_cols"]:
            raise ValueError(f"{what}: obs: shape {obs.shape}, (rows, {p['obs_cols']}) needed")
        M = self._backward_rows(what, c, obs.shape[0])
        P = p["priv_cols"] if net == "critic" else 0
        if P:
            priv = np.ascontiguousarray(priv, dtype=np.float32) if priv is not None else None
            if priv is None or priv.shape != (M, P):
                raise ValueError(f"{what}: priv: shape {None if priv is None else priv.shape}, {(M, P)} needed")
        else:
            priv = None
        w = p["widths"][net]
        g_out = np.ascontiguousarray(g_out, dtype=np.float32)
        if g_out.size != M * w[-1]:
            raise ValueError(f"{what}: the output gradient: {g_out.size} elements, {M * w[-1]} needed")
        try:
            hidden = [np.ascontiguousarray(h, dtype=np.float32) for h in hidden]
        except TypeError:
            raise ValueError(f"{what}: hidden is the list of the forward pass") from None
        if len(hidden) != len(w) - 2:
            raise ValueError(f"{what}: hidden names {len(hidden)} layers, the {net} has {len(w) - 2} hidden layers")
        for l, h in enumerate(hidden):
            if h.shape != (M, w[l + 1]):
                raise ValueError(f"{what}: hidden[{l}]: shape {h.shape}, {(M, w[l + 1])} needed")
        table, keep = self._policy_params(what, p, params, device=False)
        K, first = len(p["sizes"]), p["first"][net]
        grads, tg = {}, (C.c_void_p * K)()
        for l in range(len(w) - 1):
            grads[first + 2 * l] = np.empty((w[l + 1], w[l]), np.float32)
            grads[first + 2 * l + 1] = np.empty(w[l + 1], np.float32)
        for k, a in grads.items():
            tg[k] = a.ctypes.data
        delta = [np.empty((M, h), np.float32) for h in w[1:-1]]
        th, td = (C.c_void_p * len(delta))(*(h.ctypes.data for h in hidden)), (C.c_void_p * len(delta))(*(d.ctypes.data for d in delta))
        if net == "actor":
            _lib.check(_lib.lib().gmr_motion_tracker_act_backward(self.handle, table, tg, M, _lib._ptr(obs), th, _lib._ptr(g_out), td))
        else:
            _lib.check(_lib.lib().gmr_motion_tracker_values_backward(self.handle, table, tg, M, _lib._ptr(obs), _lib._ptr(priv), th, _lib._ptr(g_out), td))
        return {"grads": grads, "delta": delta}

    def act_backward(self, params, obs, hidden, grad_loc) -> Dict[str, object]:
        """:meth:`act_backward_dev` on host arrays -> ``{"grads": {k: the gradient of params[k]} for the actor's tensors, "delta": [..]}``"""
        return self._backward_host("act_backward", "actor", params, obs, None, hidden, grad_loc)

    def values_backward(self, params, obs, priv, hidden, grad_values) -> Dict[str, object]:
        """:meth:`values_backward_dev` on host arrays, as :meth:`act_backward`, for the critic's tensors"""
        return self._backward_host("values_backward", "critic", params, obs, priv, hidden, grad_values)

    def backward_state(self) -> Optional[Dict[str, int]]:
        """``chunk``, the rows of one partial sum, ``chunks`` for ``max_rows``, ``workspace_bytes``, ``max_rows`` and the entries of the
        two tile tables, as the library holds them; ``None`` when :meth:`set_backward` never ran."""
        if self._backward is None:
            return None
        state = np.zeros(len(_lib.POLICY_BWD_STATE), np.int64)
        _lib.check(_lib.lib().gmr_motion_tracker_backward_state(self.handle, _lib._ptr(state)))
        return {k: int(v) for k, v in zip(_lib.POLICY_BWD_STATE, state)}

    # ---- the step ---------------------------------------------------------------------------------------------------------
    def _counts(self):
        return _lib.widths(_lib.TRACKER_OUT, R=self.nrobot_dof), _lib.widths(_lib.TRACKER_SIM, R=self.nrobot_dof)

    def _step_rows(self):
        return self._rows_of(_lib.TRACKER_OUT, R=self.nrobot_dof), self._rows_of(_lib.TRACKER_SIM, R=self.nrobot_dof)

    def step(self, sim: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
        """One environment step, host arrays in and out.  Returns ``ref_root_pos [N,3]``, ``ref_root_rot [N,4]`` xyzw, ``ref_root_vel``,
        ``ref_root_ang_vel``, ``ref_dof_pos [N,R]``, ``ref_dof_vel`` (robot dof order), ``status`` and ``finished`` (``i32[N]``); with
        ``sim`` -- any of ``base_pos, base_quat, base_lin_vel, base_ang_vel, dof_pos, dof_vel`` (quaternions xyzw) -- also ``err [N,6]``,
        ``term [N,6]`` and ``total [N]`` in the order of :data:`TERMS`."""
        outs, sims = self._step_rows()
        table, out = _lib.host_outputs(_lib.TrackerOut, outs, skip=("err", "term", "total") if sim is None else ())
        st, keep = (None, None) if sim is None else _lib.host_inputs(_lib.TrackerSim, sims, sim, "step", unknown="simulator arrays")
        _lib.check(_lib.lib().gmr_motion_tracker_step(self.handle, None if st is None else C.byref(st), C.byref(table)))
        return out

    def step_dev(self, sim: Optional[Dict[str, object]] = None, stream=None, **outputs) -> None:
        """The same on device memory, asynchronous on ``stream``: ``sim`` maps names to device arrays, ``outputs`` names whichever of the
        arrays of :meth:`step` are wanted; each is a ``_lib.DeviceBuffer``, a raw address or an object with ``data_ptr()``, checked as
        ``MotionLibrary.sample_dev`` checks them."""
        outs, sims = self._step_rows()
        table = _lib.device_struct(_lib.TrackerOut, outs, outputs, "step_dev")
        st = None if sim is None else _lib.device_struct(_lib.TrackerSim, sims, sim, "step_dev", unknown="simulator arrays")
        _lib.check(_lib.lib().gmr_motion_tracker_step_dev(self.handle, None if st is None else C.byref(st), C.byref(table), _lib._s(stream)))

    # ---- links ---------------------------------------------------------------------------------------
    def _link_setup(self, kinematics, bodies, sim_bodies, link_weight, frame):
        """the checks of :meth:`set_links`, all of them before a device is touched: ``(kinematics, has names, sel i32[nsel], sim_body
        i32[nsel], weight f32[nsel] or None, frame)``"""
        if frame not in FRAMES:
            raise ValueError(f"frame is one of {sorted(FRAMES)}, got {frame!r}")
        km, names = self.library._resolve_kinematics(kinematics)
        nbody = len(names) if names is not None else km.nbody
        sel, nsel = self.library._body_selection(bodies, names, nbody)
        if sel is None:
            if not 1 <= nbody <= 64:
                raise ValueError(f"a selection holds 1 to 64 bodies, the robot has {nbody}")
            sel = np.arange(nbody, dtype=np.int32)
        sb = np.arange(nsel, dtype=np.int32) if sim_bodies is None else np.ascontiguousarray(sim_bodies, dtype=np.int32).reshape(-1)
        if len(sb) != nsel:
            raise ValueError(f"sim_bodies has {len(sb)} entries, the selection {nsel}")
        if ((sb < 0) | (sb >= 1 << 16)).any():
            raise ValueError(f"sim_bodies entries lie in [0, 65536): {sb.tolist()}")
        w = None
        if link_weight is not None:
            w = np.ascontiguousarray(link_weight, dtype=np.float32).reshape(-1)
            if len(w) != nsel:
                raise ValueError(f"link_weight has {len(w)} entries, the selection {nsel}")
            if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
                raise ValueError("link_weight must be finite, not negative and not all zero")
        return km, names is not None, sel, sb, w, frame

    def set_links(self, kinematics=None, bodies=None, sim_bodies=None, link_weight=None, frame: str = "world") -> None:
        """Attaches link targets: the robot (``kinematics``, or the library's attached one) and ``bodies`` by name or index, in any
        order (``None``: all).  ``sim_bodies[s]`` is the simulator's body index of selection row ``s`` (identity by default),
        ``link_weight`` weighs the links inside the four link terms, ``frame`` is ``"world"`` or ``"heading"`` (each side relative to
        its own root with the root's yaw removed).  ``bodies=[]`` detaches.  Link targets follow the motion in the library's dof
        order: the ``dof_map`` does not enter."""
        if bodies is not None and len(bodies) == 0:
            _lib.check(_lib.lib().gmr_motion_tracker_set_links(self.handle, None, None, 0, None, None, 0))
            self._links = None
            return
        km, named, sel, sb, w, frame = self._link_setup(kinematics, bodies, sim_bodies, link_weight, frame)
        fk = km.hip_handle if named else km          # (a KinematicsModel makes its device handle here, after every check)
        _lib.check(_lib.lib().gmr_motion_tracker_set_links(self.handle, fk.handle, _lib._ptr(sel), len(sel), _lib._ptr(sb), _lib._ptr(w), FRAMES[frame]))
        self._links = (fk, len(sel), sb, frame)

    def set_link_terms(self, scales=None, weights=None, fail_dist: float = float("inf")) -> None:
        """``link_term = exp(-link_err / scale)`` over :data:`LINK_TERMS` (defaults :data:`DEFAULT_LINK_SCALES`, weights one; ``None``
        keeps what is set); ``fail = not (max_dist <= fail_dist)`` and ``fail_dist`` is set by every call."""
        sc, wt = _terms(scales, weights, LINK_TERMS, DEFAULT_LINK_SCALES)
        fail_dist = float(fail_dist)
        if not fail_dist > 0:
            raise ValueError(f"fail_dist = {fail_dist}, must be positive (or inf)")
        _lib.check(_lib.lib().gmr_motion_tracker_set_link_terms(self.handle, _lib._ptr(sc), _lib._ptr(wt), fail_dist))

    def _link_counts(self):
        return _lib.widths(_lib.TRACKER_LINKS_OUT, nsel=self._links[1] if self._links else 0)

    def _check_links(self, sim, links, device: bool):
        """the checks of a link step that need no device -> ``("packed", array) | ("separate", {name: array}) | None``"""
        if links is None:
            return None
        if self._links is None:
            raise ValueError("the tracker has no links attached: call set_links() first")
        _, nsel, sb, frame = self._links
        unknown = sorted(set(links) - set(LINK_SIM) - {"body_state"})
        if unknown:
            raise TypeError(f"step_links: unknown link arrays {unknown}")
        if frame == "heading" and (sim is None or sim.get("base_pos") is None or sim.get("base_quat") is None):
            raise ValueError('frame="heading" needs base_pos and base_quat of the simulator\'s root in sim')
        if "body_state" in links:
            if len(links) != 1:
                raise TypeError("links is either {'body_state': [N, nb, 13]} or the four separate arrays")
            return "packed", links["body_state"]
        given = {k: v for k, v in links.items() if v is not None}
        if not given:
            raise ValueError(f"links names none of {sorted(LINK_SIM)}: pass links=None for a step without the simulator's links")
        return "separate", given

    def step_links(self, sim: Optional[Dict[str, np.ndarray]] = None, links: Optional[Dict[str, np.ndarray]] = None,
                   advance: bool = True) -> Dict[str, np.ndarray]:
        """:meth:`step` plus, in the same launch, ``ref_body_pos [N,nsel,3]``, ``ref_body_rot [N,nsel,4]``, ``ref_body_vel``,
        ``ref_body_ang_vel`` of the attached links at the environments' own clocks and -- with ``links``, the simulator's rigid-body
        state as ``{"body_state": [N, nb, 13]}`` (pos, quat xyzw, vel, ang vel) or as ``body_pos / body_rot / body_vel / body_ang_vel
        [N, nsel, k]`` -- ``link_err [N,4]``, ``link_term [N,4]``, ``max_dist [N]`` and ``fail i32[N]``; ``total`` then includes the link
        terms.  ``advance=False`` leaves clocks and clips as they are (reference-state initialisation after :meth:`reset`)."""
        kind = self._check_links(sim, links, False)
        outs, sims = self._step_rows()
        skip = ("err", "term") if sim is None else ()
        table, out = _lib.host_outputs(_lib.TrackerOut, outs, skip=skip + ("total",) if sim is None and kind is None else skip)
        ltable, lout = _lib.TrackerLinksOut(), {}
        if self._links is not None:
            louts = self._rows_of(_lib.TRACKER_LINKS_OUT, nsel=self._links[1])
            ltable, lout = _lib.host_outputs(_lib.TrackerLinksOut, louts, skip=() if kind is not None else ("link_err", "link_term", "max_dist", "fail"))
        st, keep = (None, None) if sim is None else _lib.host_inputs(_lib.TrackerSim, sims, sim, "step_links", unknown="simulator arrays")
        ls, held = (None, None) if kind is None else self._links_sim(kind, None, False)
        _lib.check(_lib.lib().gmr_motion_tracker_step_links(self.handle, None if st is None else C.byref(st), None if ls is None else C.byref(ls),
                                                            C.byref(table), C.byref(ltable), 0 if advance else _lib.TRACKER_NO_ADVANCE))
        out.update(lout)
        return out

    def _links_sim(self, kind, nb, device: bool):
        """the simulator's links of a link step, as :meth:`_check_links` sorted them, through :meth:`_bodies`"""
        nsel, sb = self._links[1], self._links[2]
        if kind[0] == "packed":
            return self._bodies({"body_state": kind[1]}, LINK_SIM, nsel, nb, int(sb.max()), device)
        if not np.array_equal(sb, np.arange(nsel)):
            raise ValueError("separate link arrays are [N, nsel, k] in selection order: they need the identity sim_bodies")
        return self._bodies(kind[1], LINK_SIM, nsel, device=device)

    def step_links_dev(self, sim: Optional[Dict[str, object]] = None, links: Optional[Dict[str, object]] = None, advance: bool = True,
                       stream=None, **outputs) -> None:
        """:meth:`step_links` on device memory, asynchronous on ``stream``.  ``links`` is ``{"body_state": array, "num_bodies": nb}``
        for a packed ``[N, nb, 13]`` tensor or the four separate ``[N, nsel, k]`` arrays; ``outputs`` names whichever arrays of
        :meth:`step_links` are wanted."""
        links = None if links is None else dict(links)
        nb = None if links is None else links.pop("num_bodies", None)
        kind = self._check_links(sim, links, True)
        outs, sims = self._step_rows()
        louts = self._rows_of(_lib.TRACKER_LINKS_OUT, nsel=self._links[1] if self._links else 0)
        unknown = sorted(set(outputs) - set(outs) - set(louts))
        if unknown:
            raise TypeError(f"step_links_dev: unknown outputs {unknown}")
        table = _lib.device_struct(_lib.TrackerOut, outs, {k: x for k, x in outputs.items() if k in outs})
        ltable = _lib.device_struct(_lib.TrackerLinksOut, louts, {k: x for k, x in outputs.items() if k in louts})
        st = None if sim is None else _lib.device_struct(_lib.TrackerSim, sims, sim, "step_links_dev", unknown="simulator arrays")
        ls = None
        if kind is not None:
            if kind[0] == "packed" and nb is None:
                shape = getattr(kind[1], "shape", None)
                if shape is None or len(shape) != 3:
                    raise ValueError("a packed body_state on the device needs num_bodies (or a [N, nb, 13] shape)")
                nb = shape[1]
            ls, _ = self._links_sim(kind, None if nb is None else int(nb), True)
        _lib.check(_lib.lib().gmr_motion_tracker_step_links_dev(self.handle, None if st is None else C.byref(st), None if ls is None else C.byref(ls),
                                                                C.byref(table), C.byref(ltable), 0 if advance else _lib.TRACKER_NO_ADVANCE,
                                                                _lib._s(stream)))

    # ---- preview ------------------------------------------------------------------------------------
    def _preview_setup(self, offsets, blocks, frame, bodies):
        """the checks of :meth:`set_preview`, all of them before a device is touched: ``(offsets f32[K], blocks in row order, block
        bits, sel i32[nsel] or None)``"""
        off = np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1)
        if not 1 <= len(off) <= PREVIEW_MAX_OFFSETS:
            raise ValueError(f"a preview holds 1 to {PREVIEW_MAX_OFFSETS} offsets, got {len(off)}")
        if not np.isfinite(off).all():
            raise ValueError(f"offsets must be finite: {off.tolist()}")
        if isinstance(blocks, str):
            blocks = (blocks,)
        unknown = sorted(set(blocks) - set(PREVIEW_BLOCKS))
        if unknown:
            raise ValueError(f"unknown preview blocks {unknown} (known: {list(PREVIEW_BLOCKS)})")
        names = tuple(b for b in PREVIEW_BLOCKS if b in blocks)
        if not names:
            raise ValueError("a preview needs at least one block")
        if frame not in PREVIEW_FRAMES:
            raise ValueError(f"frame is one of {sorted(PREVIEW_FRAMES)}, got {frame!r}")
        lib = self.library
        if frame != "raw" and "root_ang_vel" in names and lib.ang_vel != "world":
            raise ValueError(f'root_ang_vel in frame "{frame}" needs a library built with ang_vel="world": the root_ang_vel of '
                             f'ang_vel="{lib.ang_vel}" is not a physical angular velocity and cannot be rotated')
        sel = None
        if "body_pos" in names:
            if not lib.has_local_body_pos:
                raise ValueError("the body_pos block needs a library that holds local_body_pos")
            if bodies is None or len(bodies) == 0:
                raise ValueError("the body_pos block needs bodies=: rows of the library's local_body_pos, by index or by name")
            ids = []
            for b in bodies:
                if isinstance(b, str):
                    lists = lib.link_body_lists
                    if not lists or not lists[0] or any(list(x) != list(lists[0]) for x in lists):
                        raise ValueError("bodies by name need every clip of the library to carry the same non-empty link_body_list")
                    if b not in lists[0]:
                        raise KeyError(f"unknown body {b!r}")
                    ids.append(list(lists[0]).index(b))
                else:
                    ids.append(int(b))
            if not 1 <= len(ids) <= PREVIEW_MAX_BODIES:
                raise ValueError(f"the body_pos block holds 1 to {PREVIEW_MAX_BODIES} bodies, got {len(ids)}")
            for b in ids:
                if not 0 <= b < lib.nbody:
                    raise ValueError(f"body {b} outside [0, {lib.nbody})")
            if len(set(ids)) != len(ids):
                raise ValueError("a selection names every body once")
            sel = np.array(ids, dtype=np.int32)
        elif bodies is not None and len(bodies):
            raise ValueError("bodies= is given but body_pos is not among the blocks")
        return off, names, sum(_lib.PREVIEW_BLOCKS[b] for b in names), sel

    @property
    def preview_layout(self) -> Optional[Dict[str, object]]:
        """``{block: slice into the last axis of obs, ..., "row_width": D}`` of the configured preview under the current dof tables,
        or ``None``"""
        if self._preview is None:
            return None
        _, names, _, nsel = self._preview
        width = {"root_pos": 3, "root_quat": 4, "root_rot6": 6, "root_vel": 3, "root_ang_vel": 3, "dof_pos": self.nrobot_dof,
                 "dof_vel": self.nrobot_dof, "body_pos": 3 * nsel}
        out, at = {}, 0
        for b in names:
            out[b] = slice(at, at + width[b])
            at += width[b]
        out["row_width"] = at
        return out

    def set_preview(self, offsets, blocks=PREVIEW_SAMPLER_BLOCKS, frame: str = "raw", bodies=None) -> Optional[Dict[str, object]]:
        """Configures the preview: ``offsets`` (1 to 16, seconds, any sign and order) added to every environment's clock, ``blocks`` out
        of :data:`PREVIEW_BLOCKS` (packed in that order whatever order they are named in), ``frame`` -- ``"raw"`` as sampled,
        ``"reference"`` relative to the reference root at the environment's current clock with its yaw removed, ``"sim"`` relative to the
        simulator's ``base_pos / base_quat`` -- and, for ``body_pos``, ``bodies``: rows of the library's ``local_body_pos`` by index, or
        by name when every clip carries the same ``link_body_list``.  Returns :attr:`preview_layout`.  ``offsets=[]`` removes the
        configuration.  Previews already enqueued keep the configuration they were launched with."""
        if offsets is None or np.size(offsets) == 0:
            _lib.check(_lib.lib().gmr_motion_tracker_set_preview(self.handle, 0, None, 0, 0, None, 0, None))
            self._preview = None
            return None
        off, names, bits, sel = self._preview_setup(offsets, blocks, frame, bodies)
        D = C.c_int()
        _lib.check(_lib.lib().gmr_motion_tracker_set_preview(self.handle, len(off), _lib._ptr(off), bits, PREVIEW_FRAMES[frame], _lib._ptr(sel),
                                                             0 if sel is None else len(sel), C.byref(D)))
        self._preview = (len(off), names, frame, 0 if sel is None else len(sel))
        assert self.preview_layout["row_width"] == D.value, (self.preview_layout, D.value)
        return self.preview_layout

    def _check_preview(self, sim, what):
        """the checks of a preview that need no device -> ``(K, D, frame)``"""
        if self._preview is None:
            raise ValueError("the tracker has no preview configured: call set_preview() first")
        K, _, frame, _ = self._preview
        if sim is not None:
            unknown = sorted(set(sim) - set(self._counts()[1]))
            if unknown:
                raise TypeError(f"{what}: unknown simulator arrays {unknown}")
        if frame == "sim" and (sim is None or sim.get("base_pos") is None or sim.get("base_quat") is None):
            raise ValueError('frame="sim" needs base_pos and base_quat of the simulator\'s root in sim')
        return K, self.preview_layout["row_width"], frame

    def preview(self, sim: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
        """The reference at every environment's clock plus each offset, host arrays out: ``obs [N,K,D]`` (see :attr:`preview_layout`),
        ``valid i32[N,K]`` -- 1 where the query lies inside the clip, neither wrapped nor clamped -- and ``status i32[N]``, 1 for a bad
        assignment (its rows are NaN).  One launch; clocks, clips and draw counters stay as they are.  ``sim`` is read in
        ``frame="sim"`` only: ``base_pos [N,3]``, ``base_quat [N,4]`` xyzw."""
        N = self.num_envs
        K, D, frame = self._check_preview(sim, "preview")
        st, keep = None, None
        if frame == "sim":
            st, keep = _lib.host_inputs(_lib.TrackerSim, self._step_rows()[1], {k: sim[k] for k in ("base_pos", "base_quat")})
        out = {"obs": np.empty((N, K, D), np.float32), "valid": np.empty((N, K), np.int32), "status": np.empty(N, np.int32)}
        _lib.check(_lib.lib().gmr_motion_tracker_preview(self.handle, None if st is None else C.byref(st), _lib._ptr(out["obs"]),
                                                         _lib._ptr(out["valid"]), _lib._ptr(out["status"])))
        return out

    def preview_dev(self, sim: Optional[Dict[str, object]] = None, stream=None, obs=None, valid=None, status=None) -> None:
        """:meth:`preview` on device memory, asynchronous on ``stream`` (the tracker's stream, or one the caller orders behind it):
        whichever of ``obs f32[N*K*D]``, ``valid i32[N*K]``, ``status i32[N]`` are wanted, each a ``_lib.DeviceBuffer``, a raw address or
        an object with ``data_ptr()``."""
        N = self.num_envs
        K, D, frame = self._check_preview(sim, "preview_dev")
        st = None
        if frame == "sim":
            st = _lib.device_struct(_lib.TrackerSim, self._step_rows()[1], {k: sim[k] for k in ("base_pos", "base_quat")})
        _lib.check(_lib.lib().gmr_motion_tracker_preview_dev(self.handle, None if st is None else C.byref(st),
                                                             _dev_ptr(obs, "obs", "float32", N * K * D), _dev_ptr(valid, "valid", "int32", N * K),
                                                             _dev_ptr(status, "status", "int32", N), _lib._s(stream)))

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h:
            _lib.lib().gmr_motion_tracker_destroy(h)
            self.handle = None
            self._proprio = None          # the state arrays went with the handle
            self._optim = None            # and so did exp_avg and exp_avg_sq
            self._policy = None           # and the counts of the sampled actions
            self._backward = None         # and the workspace of the backward pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
