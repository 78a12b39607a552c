"""ctypes binding of libgmrhip.so (include/gmr_hip.h).  No torch, no fallback: if the library is
missing or no GPU is visible the product path raises -- there is deliberately no CPU path here."""
from __future__ import annotations

import ctypes as C
import importlib.util
import math
import os
import sys
from typing import NamedTuple

import numpy as np

from .ik_config import MODEL_DTYPE, TASKSET_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GMR_HIP_LIBRARY") or os.path.join(_HERE, "libgmrhip.so")   # override: A/B builds of the library
_lib = None

FLAG_OFFSET_TO_GROUND = 1
FLAG_EVAL_ONLY = 2
FLAG_FRAME_LIMIT_FIRST = 4    # q0 is the pose of the frame before frame 0: the frame velocity limit bounds frame 0 too
POST_HEIGHT_ADJUST, POST_ROOT_ORIGIN_OFFSET = 1, 2
STATUS_OK, STATUS_QP_FAILED, STATUS_QP_MAXITER = 0, -1, -2


class GmrHipError(RuntimeError):
    pass


_SIGS = {
    "gmr_last_error": (C.c_char_p, []),
    "gmr_backend_info": (C.c_char_p, []),
    "gmr_device_count": (C.c_int, []),
    "gmr_set_device": (C.c_int, [C.c_int]),
    "gmr_sizeof_model": (C.c_size_t, []),
    "gmr_sizeof_taskset": (C.c_size_t, []),
    "gmr_malloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "gmr_free": (C.c_int, [C.c_void_p]),
    "gmr_memset": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "gmr_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gmr_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gmr_stream_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "gmr_stream_destroy": (C.c_int, [C.c_void_p]),
    "gmr_stream_sync": (C.c_int, [C.c_void_p]),
    "gmr_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "gmr_event_destroy": (C.c_int, [C.c_void_p]),
    "gmr_event_record": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmr_event_elapsed_ms": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "gmr_solver_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "gmr_solver_destroy": (C.c_int, [C.c_void_p]),
    "gmr_solver_dims": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gmr_solver_set_waves": (C.c_int, [C.c_void_p, C.c_int]),
    "gmr_solver_set_dispatch": (C.c_int, [C.c_void_p, C.c_int]),
    "gmr_solver_set_velocity_limits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_solver_velocity_limits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_solver_set_frame_velocity_limits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double]),
    "gmr_solver_frame_velocity_limits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "gmr_retarget_lds_bytes": (C.c_int, [C.c_void_p]),
    "gmr_retarget_streams_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_retarget_streams": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_retarget_streams_scaled_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]),
    "gmr_retarget_streams_scaled": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_retarget_group_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "gmr_retarget_group": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "gmr_retarget_group_window_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gmr_retarget_streams_weighted_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p]),
    "gmr_retarget_streams_weighted": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_retarget_group_weighted_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_retarget_group_weighted_window_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "gmr_retarget_group_weighted": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "gmr_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "gmr_host_free": (C.c_int, [C.c_void_p]),
    "gmr_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "gmr_host_unregister": (C.c_int, [C.c_void_p]),
    "gmr_fk_create": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                C.POINTER(C.c_void_p)]),
    "gmr_fk_destroy": (C.c_int, [C.c_void_p]),
    "gmr_fk_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "gmr_fk_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "gmr_fk_segment_min_z_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gmr_fk_batch_segments": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "gmr_postprocess_clips_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_smplx_create": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "gmr_smplx_destroy": (C.c_int, [C.c_void_p]),
    "gmr_smplx_rows": (C.c_int, [C.c_void_p]),
    "gmr_smplx_joints_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_smplx_joints": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_smplx_align_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "gmr_smplx_align": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_void_p]),
    "gmr_smplx_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gmr_smplx_compact_layout": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_int)]),
    "gmr_smplx_align_compact_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "gmr_smplx_batch_takes": (C.c_int, [C.c_void_p]),
    "gmr_smplx_target_times": (C.c_int, [C.c_int, C.c_int, C.c_void_p]),
    "gmr_smplx_batch_frames_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_smplx_batch_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_bvh_create": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "gmr_bvh_destroy": (C.c_int, [C.c_void_p]),
    "gmr_bvh_columns": (C.c_int, [C.c_void_p]),
    "gmr_bvh_frames_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gmr_bvh_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_chunk_plan": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gmr_chunk_gather_dev": (C.c_int, [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8),
    "gmr_chunk_stitch_dev": (C.c_int, [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10),
    "gmr_chunk_seams_dev": (C.c_int, [C.c_int] * 5 + [C.c_void_p] * 5 + [C.c_double] + [C.c_void_p] * 5),
    "gmr_motion_lib_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "gmr_motion_lib_destroy": (C.c_int, [C.c_void_p]),
    "gmr_motion_lib_fill_dev": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_void_p]),
    "gmr_motion_lib_fill": (C.c_int, [C.c_void_p] * 5 + [C.c_int]),
    "gmr_motion_lib_array": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "gmr_motion_sample_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9),
    "gmr_motion_sample": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8),
    "gmr_motion_body_state_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p]),
    "gmr_motion_body_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_motion_tracker_create": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint64, C.POINTER(C.c_void_p)]),
    "gmr_motion_tracker_destroy": (C.c_int, [C.c_void_p]),
    "gmr_motion_tracker_set_dof_map": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_terms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_assign_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_assign": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "gmr_motion_tracker_reset_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "gmr_motion_tracker_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int)]),
    "gmr_motion_tracker_step_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "gmr_motion_tracker_set_links": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_motion_tracker_set_link_terms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]),
    "gmr_motion_tracker_step_links_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_motion_tracker_step_links": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_motion_tracker_set_preview": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "gmr_motion_tracker_preview_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_preview": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_adaptive": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double]),
    "gmr_motion_tracker_adapt_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_adapt": (C.c_int, [C.c_void_p]),
    "gmr_motion_tracker_reset_done_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                                    C.c_void_p]),
    "gmr_motion_tracker_reset_done": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                                C.POINTER(C.c_int)]),
    "gmr_motion_tracker_adaptive_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_enable_anchors": (C.c_int, [C.c_void_p, C.c_int]),
    "gmr_motion_tracker_set_anchor_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_anchor": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "gmr_motion_tracker_anchor_to_root_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_motion_tracker_anchor_to_root": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "gmr_motion_tracker_anchor_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_control": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int]),
    "gmr_motion_tracker_targets_dev": (C.c_int, [C.c_void_p] * 7),
    "gmr_motion_tracker_targets": (C.c_int, [C.c_void_p] * 6),
    "gmr_motion_tracker_hold_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_hold": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "gmr_motion_tracker_torques_dev": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 8),
    "gmr_motion_tracker_torques": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 7),
    "gmr_motion_tracker_control_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_proprio": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_proprio_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_proprio": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_motion_tracker_proprio_reset_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_proprio_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "gmr_motion_tracker_proprio_state": (C.c_int, [C.c_void_p] * 7),
    "gmr_motion_tracker_set_terrain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]),
    "gmr_motion_tracker_terrain_heights_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_terrain_heights": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_feet": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_feet_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_feet": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_feet_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_commands": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_motion_tracker_commands_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_commands": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_command_state": (C.c_int, [C.c_void_p] * 9),
    "gmr_motion_tracker_set_disturbances": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_disturb_dev": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_disturb": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "gmr_motion_tracker_set_reset_states": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_reset_states_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_motion_tracker_reset_states": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "gmr_motion_tracker_reset_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_rewards": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_rewards_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_rewards": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_reward_stats_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_motion_tracker_reward_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_motion_tracker_reward_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_rollout": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]),
    "gmr_motion_tracker_record_dev": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 8),
    "gmr_motion_tracker_record": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 7),
    "gmr_motion_tracker_advantages_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_motion_tracker_advantages": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_motion_tracker_set_loss": (C.c_int, [C.c_void_p] + [C.c_double] * 8),
    "gmr_motion_tracker_loss_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_log_prob_dev": (C.c_int, [C.c_void_p] * 6),
    "gmr_motion_tracker_log_prob": (C.c_int, [C.c_void_p] * 5),
    "gmr_motion_tracker_loss_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_motion_tracker_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_motion_tracker_set_optimizer": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p] + [C.c_double] * 5),
    "gmr_motion_tracker_optimizer_step_dev": (C.c_int, [C.c_void_p] * 5),
    "gmr_motion_tracker_optimizer_step": (C.c_int, [C.c_void_p] * 4),
    "gmr_motion_tracker_optimizer_state": (C.c_int, [C.c_void_p] * 4),
    "gmr_motion_tracker_optimizer_load_state": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "gmr_motion_tracker_set_policy": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "gmr_motion_tracker_act_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]),
    "gmr_motion_tracker_act": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int]),
    "gmr_motion_tracker_values_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    "gmr_motion_tracker_values": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4),
    "gmr_motion_tracker_policy_state": (C.c_int, [C.c_void_p] * 3),
    "gmr_motion_tracker_set_backward": (C.c_int, [C.c_void_p, C.c_int64]),
    "gmr_motion_tracker_act_backward_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    "gmr_motion_tracker_act_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4),
    "gmr_motion_tracker_values_backward_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6),
    "gmr_motion_tracker_values_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    "gmr_motion_tracker_backward_state": (C.c_int, [C.c_void_p] * 2),
    "gmr_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "gmr_comm_destroy": (C.c_int, [C.c_void_p]),
    "gmr_comm_rank": (C.c_int, [C.c_void_p]),
    "gmr_comm_world": (C.c_int, [C.c_void_p]),
    "gmr_comm_backend": (C.c_char_p, [C.c_void_p]),
    "gmr_comm_broadcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "gmr_comm_broadcast_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "gmr_comm_barrier": (C.c_int, [C.c_void_p]),
    "gmr_comm_allreduce_max": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_comm_allreduce_sum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_comm_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "gmr_bootstrap_exchange": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t, C.c_double]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)


HIP_RUNTIME = None   # path of the HIP runtime preloaded by _share_hip_runtime(), if any


def _share_hip_runtime():
    """One HIP runtime per process.  A PyTorch-ROCm wheel bundles its own ``libamdhip64.so`` +
    ``libhsa-runtime64.so`` and asks the loader for them by their unversioned names, so when libgmrhip.so has
    already pulled in the system runtime (``/opt/rocm``, by SONAME ``libamdhip64.so.7``) a later ``import
    torch`` loads a SECOND runtime and finds "No HIP GPUs" (the first one owns the device).  The other order
    works (our SONAME request matches torch's copy).  So: if torch is installed but not yet imported, load ITS
    runtime first -- without importing torch -- and let libgmrhip.so bind to it.
    ``GMR_HIP_RUNTIME=system`` keeps the system runtime, ``GMR_HIP_RUNTIME=/path/libamdhip64.so`` picks one."""
    global HIP_RUNTIME
    mode = os.environ.get("GMR_HIP_RUNTIME", "auto")
    if mode == "system" or "torch" in sys.modules:
        return
    path = mode if mode not in ("auto", "torch") else None
    if path is None:
        try:
            spec = importlib.util.find_spec("torch")
        except (ImportError, ValueError):
            spec = None
        for d in (spec.submodule_search_locations or []) if spec else []:
            cand = os.path.join(d, "lib", "libamdhip64.so")
            if os.path.exists(cand):
                path = cand
                break
    if path:
        C.CDLL(path, mode=C.RTLD_GLOBAL)
        HIP_RUNTIME = path


def lib():
    """Load libgmrhip.so (raises GmrHipError when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GmrHipError(
                f"{LIB_PATH} not found: build it with `python -m general_motion_retargeting_amd.build` "
                "(there is no CPU fallback in the product path)")
        _share_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.gmr_sizeof_model() != MODEL_DTYPE.itemsize or L.gmr_sizeof_taskset() != TASKSET_DTYPE.itemsize:
            raise GmrHipError("ABI mismatch between libgmrhip.so and the Python struct layouts")
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise GmrHipError(f"libgmrhip error {rc}: {lib().gmr_last_error().decode()}")


def require_gpu() -> None:
    if lib().gmr_device_count() <= 0:
        raise GmrHipError("no HIP device visible: the product path needs an MI355X (no CPU fallback)")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _s(stream):
    """hipStream_t of a :class:`Stream`, a raw ``c_void_p`` or ``None`` (the default stream)."""
    return stream.ptr if isinstance(stream, Stream) else stream


def _d(x):
    """device pointer of a :class:`DeviceBuffer`, a raw ``c_void_p`` or ``None``."""
    return x.ptr if isinstance(x, DeviceBuffer) else x


class DeviceBuffer:
    """Owned device allocation (hipMalloc through the C-ABI)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().gmr_malloc(C.byref(p), self.nbytes))
        self.ptr = p

    @classmethod
    def from_host(cls, a: np.ndarray, stream=None) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        s = _s(stream)
        check(lib().gmr_memcpy_h2d(b.ptr, _ptr(a), a.nbytes, s))
        check(lib().gmr_stream_sync(s))
        return b

    def to_host(self, shape, dtype, stream=None) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        s = _s(stream)
        check(lib().gmr_memcpy_d2h(_ptr(out), self.ptr, out.nbytes, s))
        check(lib().gmr_stream_sync(s))
        return out

    def zero(self, stream=None):
        check(lib().gmr_memset(self.ptr, 0, self.nbytes, _s(stream)))
        check(lib().gmr_stream_sync(_s(stream)))

    def free(self):
        if self.ptr:
            lib().gmr_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _PinnedOwner:
    """Keeps one gmr_host_alloc block alive for the NumPy arrays that view it."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(lib().gmr_host_alloc(C.byref(p), max(int(nbytes), 8)))
        self.ptr, self.nbytes = p, int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                lib().gmr_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64) -> np.ndarray:
    """``np.empty`` in page-locked host memory (gmr_host_alloc): H2D / D2H copies of such arrays are asynchronous and run
    at PCIe speed, which is what lets :func:`retarget_group` overlap them with the kernels.  The block is freed when the
    last view of the array dies."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    owner = _PinnedOwner(n * dtype.itemsize)
    buf = (C.c_char * max(owner.nbytes, 1)).from_address(owner.ptr.value)
    buf._gmr_owner = owner                               # the ctypes buffer is the ndarray's base: it carries the owner
    return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)


def pinned_copy(a: np.ndarray) -> np.ndarray:
    out = pinned_empty(a.shape, a.dtype)
    np.copyto(out, a)
    return out


def align256(nbytes) -> int:
    """``nbytes`` rounded up to the 256-byte boundary every field of a packed device block starts on"""
    return (int(nbytes) + 255) // 256 * 256


class NamedBuffers:
    """The grow-only buffers, by name, of an object that runs batch after batch: device blocks and page-locked host blocks.
    A block that is too small is replaced, so the owner calls for one only when nothing enqueued still uses it (its batches
    end with a stream synchronisation)."""

    def __init__(self):
        self._dev = {}
        self._pin = {}

    def device(self, name: str, nbytes: int) -> DeviceBuffer:
        b = self._dev.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self._dev[name] = DeviceBuffer(nbytes + nbytes // 4 + 256)
        return b

    def pinned(self, name: str, shape, dtype) -> np.ndarray:
        """a [shape] view of the page-locked block ``name`` (grown by half when too small)"""
        need = int(np.prod(shape)) * np.dtype(dtype).itemsize
        blk = self._pin.get(name)
        if blk is None or blk.nbytes < need:
            self._pin.pop(name, None)
            blk = self._pin[name] = pinned_empty((need + need // 2 + 8,), np.uint8)
        return blk[:need].view(dtype).reshape(shape)


class Job(C.Structure):
    """``gmr_job_t``: one (solver, batch) of a group launch."""
    _fields_ = [("solver", C.c_void_p), ("S", C.c_int32), ("T", C.c_int32), ("q0", C.c_void_p), ("human", C.c_void_p),
                ("len", C.c_void_p), ("q_out", C.c_void_p), ("nsolve", C.c_void_p), ("status", C.c_void_p),
                ("tgt_out", C.c_void_p), ("err_out", C.c_void_p), ("scale", C.c_void_p)]


def check_scales(scales, S: int, nhuman: int, what: str = "scales"):
    """``scales`` as the contiguous ``f64[S, nhuman]`` table of per-stream human scale rows (None stays None); checked the way
    ``lens`` is, before any device call."""
    if scales is None:
        return None
    a = np.asarray(scales)
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise TypeError(f"{what}: numbers needed, got {a.dtype}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (S, nhuman):
        raise ValueError(f"{what} must be [{S},{nhuman}], got {a.shape}")
    return a


def check_weights(weights, S: int, T: int, nhuman: int, what: str = "weights", lens=None):
    """``weights`` as the contiguous ``f64[S, T, nhuman]`` array of per-frame body weights (None stays None): shape and values
    -- finite, not negative -- are checked here, before any device call.  ``lens`` (``i32[S]`` or None): only the frames a stream
    has are looked at; rows at or beyond ``lens[s]`` are padding that is never read, like the ``human`` rows there."""
    if weights is None:
        return None
    a = np.asarray(weights)
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer) or a.dtype == np.bool_):
        raise TypeError(f"{what}: numbers needed, got {a.dtype}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (S, T, nhuman):
        raise ValueError(f"{what} must be [{S},{T},{nhuman}], got {a.shape}")
    bad = ~(np.isfinite(a) & (a >= 0.0))
    if lens is not None:
        bad &= (np.arange(T)[None, :] < np.asarray(lens).reshape(S, 1))[..., None]
    if bad.any():
        s, t, b = (int(x) for x in np.argwhere(bad)[0])
        raise ValueError(f"{what}: stream {s}, frame {t}, body {b} is {a[s, t, b]}: must be finite and not negative")
    return a


def _weight_list(ws):
    """the parallel ``const double* const* weight`` of a job list: None when no job has weights"""
    if all(w is None for w in ws):
        return None, None
    arr = (C.c_void_p * len(ws))(*[_addr(w) for w in ws])
    return arr, C.cast(arr, C.c_void_p)


class PostSrc(C.Structure):
    """``gmr_post_src_t``: one IK job's output as a source of :meth:`FkHandle.postprocess_clips_dev`."""
    _fields_ = [("S", C.c_int32), ("T", C.c_int32), ("q_out", C.c_void_p), ("len", C.c_void_p)]


def _addr(x):
    """address of a host ndarray / DeviceBuffer / raw pointer / None"""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if isinstance(x, DeviceBuffer):
        return x.ptr.value
    return x.value if isinstance(x, C.c_void_p) else int(x)


def group_outputs(jobs, pinned: bool = True):
    """Output arrays ``(q_out, nsolve, status)`` per job for :func:`retarget_group` (``outs=``): page-locking memory costs
    far more than retargeting a batch does, so a caller that runs many batches allocates them once."""
    empty = pinned_empty if pinned else (lambda shape, dtype: np.empty(shape, dtype))
    outs = []
    for j in jobs:
        sol, (S, T) = j["solver"], j["human"].shape[:2]
        outs.append((empty((S, T, sol.nq), np.float64), empty((S, T, 2), np.int32), empty((S,), np.int32)))
    return outs


def retarget_group(jobs, flags: int = 0, slices: int = 0, out_pinned: bool = False, outs=None):
    """Several (solver, batch) jobs as ONE scheduling domain through host buffers (``gmr_retarget_group``): the mixed-robot
    batch of BASELINE.json configs[3].  ``jobs`` = list of dicts ``{"solver": Solver, "human": f64[S,T,nhuman,7], optional
    "q0": f64[S,nq] (default the solver's qpos0), "lens": i32[S], "scales": f64[S,nhuman] (a human scale table per stream in
    place of the solver's: :meth:`Solver.retarget_streams`), "weights": f64[S,T,nhuman] (per-frame body weights, 0 = the body is
    missing in that frame; ``gmr_retarget_group_weighted``)}``.  Returns one ``(q_out, nsolve, status)`` per job.
    Inputs in pinned memory (:func:`pinned_empty`) and pinned outputs (``outs=`` from :func:`group_outputs`, reused across
    calls; or ``out_pinned=True``: allocated per call, which is slow) make the copies asynchronous, so that they overlap the
    kernels slice by slice."""
    arr = (Job * max(len(jobs), 1))()
    keep, given, outs, wts = [], outs, [], []
    empty = pinned_empty if out_pinned else (lambda shape, dtype: np.empty(shape, dtype))
    for i, j in enumerate(jobs):
        sol = j["solver"]
        human = j["human"]
        if not (isinstance(human, np.ndarray) and human.dtype == np.float64 and human.flags.c_contiguous):
            human = np.ascontiguousarray(human, dtype=np.float64)
        if human.ndim != 4 or human.shape[2] != sol.nhuman or human.shape[3] != 7:
            raise ValueError(f"job {i}: human must be [S,T,{sol.nhuman},7], got {human.shape}")
        S, T = human.shape[:2]
        q0 = j.get("q0")
        if q0 is None:
            q0 = np.broadcast_to(sol.model_blob["qpos0"][0][: sol.nq], (S, sol.nq))
        q0 = np.ascontiguousarray(q0, dtype=np.float64)
        if q0.shape != (S, sol.nq):
            raise ValueError(f"job {i}: q0 must be [{S},{sol.nq}]")
        lens = j.get("lens")
        if lens is not None:
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            if lens.shape != (S,):
                raise ValueError(f"job {i}: lens must be [S]")
        scales = check_scales(j.get("scales"), S, sol.nhuman, f"job {i}: scales")
        wts.append(check_weights(j.get("weights"), S, T, sol.nhuman, f"job {i}: weights", lens))
        if given is not None:
            q_out, nsolve, status = given[i]
            if q_out.shape != (S, T, sol.nq) or nsolve.shape != (S, T, 2) or status.shape != (S,) or q_out.dtype != np.float64 \
                    or nsolve.dtype != np.int32 or status.dtype != np.int32 or not (q_out.flags.c_contiguous and nsolve.flags.c_contiguous):
                raise ValueError(f"job {i}: outs do not match the batch")
        else:
            q_out = empty((S, T, sol.nq), np.float64)
            nsolve = empty((S, T, 2), np.int32)
            status = np.zeros(S, dtype=np.int32)
        keep.append((human, q0, lens, scales))
        outs.append((q_out, nsolve, status))
        arr[i] = Job(sol.handle.value, S, T, _addr(q0), _addr(human), _addr(lens), _addr(q_out), _addr(nsolve), _addr(status),
                     None, None, _addr(scales))
    wkeep, wlist = _weight_list(wts)
    if wlist is None:
        check(lib().gmr_retarget_group(C.cast(arr, C.c_void_p), len(jobs), int(flags), int(slices)))
    else:
        check(lib().gmr_retarget_group_weighted(C.cast(arr, C.c_void_p), len(jobs), wlist, int(flags), int(slices)))
    return outs


class DevJob(NamedTuple):
    """One job of :func:`retarget_group_dev`: the fields of ``gmr_job_t`` a device caller fills, device pointers
    (DeviceBuffer or raw).  ``scale``: f64 [S][nhuman] per-stream human scale tables, or None for the solver's own."""
    solver: object
    S: int
    T: int
    q0: object
    human: object
    len: object
    q_out: object
    nsolve: object
    status: object
    scale: object = None


def dev_job(job, i: int = 0) -> DevJob:
    """``job`` (a :class:`DevJob` or any sequence of its first 9 or all 10 fields) as a :class:`DevJob`"""
    if len(job) not in (9, 10):
        raise ValueError(f"job {i}: 9 or 10 elements needed, got {len(job)}")
    return job if isinstance(job, DevJob) else DevJob(*job)


def retarget_group_dev(jobs, flags: int = 0, stream=None, window=None, weights=None):
    """``gmr_retarget_group_dev``: ``jobs`` = list of :class:`DevJob` (or plain sequences of its first 9 or all 10 fields; the
    scale tables are unchecked: the values are the caller's responsibility); asynchronous on ``stream``.  ``window=(t_begin, t_end)``: only those frames of
    every stream (``gmr_retarget_group_window_dev``; consecutive windows on one stream, starting at 0).  ``weights``: one entry
    per job, None or the job's per-frame body weights f64 [S][T][nhuman] on the device (unchecked, like the scale tables;
    ``gmr_retarget_group_weighted_dev`` / ``_window_dev``)."""
    if weights is not None and len(weights) != len(jobs):
        raise ValueError(f"weights: one entry per job needed, got {len(weights)} for {len(jobs)} jobs")
    wkeep, wlist = _weight_list(weights) if weights is not None else (None, None)
    arr = (Job * max(len(jobs), 1))()
    for i, job in enumerate(jobs):
        j = dev_job(job, i)
        arr[i] = Job(j.solver.handle.value, int(j.S), int(j.T), _addr(j.q0), _addr(j.human), _addr(j.len), _addr(j.q_out),
                     _addr(j.nsolve), _addr(j.status), None, None, _addr(j.scale))
    if wlist is not None and window is None:
        check(lib().gmr_retarget_group_weighted_dev(C.cast(arr, C.c_void_p), len(jobs), wlist, int(flags), _s(stream)))
    elif wlist is not None:
        check(lib().gmr_retarget_group_weighted_window_dev(C.cast(arr, C.c_void_p), len(jobs), wlist, int(flags), int(window[0]),
                                                           int(window[1]), _s(stream)))
    elif window is None:
        check(lib().gmr_retarget_group_dev(C.cast(arr, C.c_void_p), len(jobs), int(flags), _s(stream)))
    else:
        check(lib().gmr_retarget_group_window_dev(C.cast(arr, C.c_void_p), len(jobs), int(flags), int(window[0]), int(window[1]),
                                                  _s(stream)))


class Stream:
    """Non-blocking HIP stream (gmr_stream_create)."""

    def __init__(self):
        p = C.c_void_p()
        check(lib().gmr_stream_create(C.byref(p)))
        self.ptr = p

    def sync(self):
        check(lib().gmr_stream_sync(self.ptr))

    def __del__(self):
        try:
            if self.ptr:
                lib().gmr_stream_destroy(self.ptr)
        except Exception:
            pass


class Event:
    def __init__(self):
        p = C.c_void_p()
        check(lib().gmr_event_create(C.byref(p)))
        self.ptr = p

    def record(self, stream=None):
        check(lib().gmr_event_record(self.ptr, _s(stream)))

    def elapsed_ms(self, stop: "Event") -> float:
        ms = C.c_float()
        check(lib().gmr_event_elapsed_ms(self.ptr, stop.ptr, C.byref(ms)))
        return float(ms.value)

    def __del__(self):
        try:
            if self.ptr:
                lib().gmr_event_destroy(self.ptr)
        except Exception:
            pass


class Solver:
    """Device-resident (robot model, task set): handle behind gmr_solver_create."""

    def __init__(self, model_blob: np.ndarray, taskset_blob: np.ndarray):
        require_gpu()
        assert model_blob.dtype == MODEL_DTYPE and taskset_blob.dtype == TASKSET_DTYPE
        self.model_blob = np.ascontiguousarray(model_blob)
        self.taskset_blob = np.ascontiguousarray(taskset_blob)
        h = C.c_void_p()
        check(lib().gmr_solver_create(_ptr(self.model_blob), _ptr(self.taskset_blob), C.byref(h)))
        self.handle = h
        self.nq = int(model_blob["nq"][0])
        self.nv = int(model_blob["nv"][0])
        self.nhuman = int(taskset_blob["nhuman"][0])

    def set_waves(self, waves_per_stream: int) -> None:
        """0 = automatic, 1 = one wavefront per stream, 4 = main + 3 helper wavefronts per stream."""
        check(lib().gmr_solver_set_waves(self.handle, int(waves_per_stream)))

    def set_dispatch(self, frames_per_item: int) -> None:
        """Many-stream launches: > 0 = device-side FIFO of (stream, frames_per_item frames) items, 0 = one workgroup per stream."""
        check(lib().gmr_solver_set_dispatch(self.handle, int(frames_per_item)))

    def set_velocity_limit(self, vmax) -> None:
        """Per-hinge velocity limits ``vmax`` f64[nhinge] in rad/s (``inf`` = none for that hinge; ``None`` = none at all) for
        every launch from this solver issued afterwards: each solve keeps ``|dq_h| <= vmax_h * timestep`` (mink's
        ``VelocityLimit``).  A bound per SOLVE -- a frame runs up to 22 of them -- not on the velocity between frames."""
        if vmax is None:
            check(lib().gmr_solver_set_velocity_limits(self.handle, None, 0))
            return
        vmax = np.ascontiguousarray(vmax, dtype=np.float64)
        if vmax.ndim != 1:
            raise ValueError(f"velocity limits must be [{self.nv - 6}], got {vmax.shape}")
        check(lib().gmr_solver_set_velocity_limits(self.handle, _ptr(vmax), int(vmax.shape[0])))

    @property
    def velocity_limit(self) -> np.ndarray:
        """f64[nhinge], rad/s; ``inf`` where a hinge has none."""
        out = np.empty(self.nv - 6, dtype=np.float64)
        check(lib().gmr_solver_velocity_limits(self.handle, _ptr(out), int(out.shape[0])))
        return out

    def set_frame_velocity_limit(self, vmax, frame_dt: float = 0.0) -> None:
        """Per-hinge FRAME velocity limits ``vmax`` f64[nhinge] in rad/s (``inf`` = none for that hinge; ``None`` = none at
        all) at ``frame_dt`` seconds between frames, for every launch from this solver issued afterwards: the result keeps
        ``|theta_h(t) - theta_h(t - 1)| <= vmax_h * frame_dt`` (gmr_solver_set_frame_velocity_limits).  Frame 0 of a stream is
        free unless the launch carries ``FLAG_FRAME_LIMIT_FIRST``."""
        if vmax is None:
            check(lib().gmr_solver_set_frame_velocity_limits(self.handle, None, 0, C.c_double(0.0)))
            return
        vmax = np.ascontiguousarray(vmax, dtype=np.float64)
        if vmax.ndim != 1:
            raise ValueError(f"frame velocity limits must be [{self.nv - 6}], got {vmax.shape}")
        check(lib().gmr_solver_set_frame_velocity_limits(self.handle, _ptr(vmax), int(vmax.shape[0]), C.c_double(float(frame_dt))))

    def frame_velocity_limit(self):
        """``(vmax f64[nhinge] rad/s, frame_dt)``: ``inf`` where a hinge has none, ``frame_dt`` 0 while none has."""
        out = np.empty(self.nv - 6, dtype=np.float64)
        dt = C.c_double(0.0)
        check(lib().gmr_solver_frame_velocity_limits(self.handle, _ptr(out), int(out.shape[0]), C.byref(dt)))
        return out, float(dt.value)

    @property
    def lds_bytes(self) -> int:
        return int(lib().gmr_retarget_lds_bytes(self.handle))

    def retarget_streams(self, q0, human, lens=None, flags: int = 0, want_targets: bool = False,
                         want_errors: bool = False, scales=None, weights=None):
        """Host arrays in/out: q0[S,nq], human[S,T,nhuman,7] -> q_out[S,T,nq], nsolve[S,T,2], status[S]
        (+ targets[S,T,nhuman,7] = the kernel's preprocessed frames and/or errors[S,T,2] = error1/error2 at the
        configuration every frame ends with, when asked for).  ``scales`` f64[S,nhuman]: a human scale table per stream
        (``ik_config.scale_rows``) in place of the solver's own, so that subjects of different heights share one launch.
        ``weights`` f64[S,T,nhuman]: a multiplier per (stream, frame, human body) on the cost of every task bound to that body;
        0 = the body is missing in that frame and its ``human`` row may hold anything (``gmr_retarget_streams_weighted``)."""
        human = np.ascontiguousarray(human, dtype=np.float64)
        if human.ndim != 4 or human.shape[2] != self.nhuman or human.shape[3] != 7:
            raise ValueError(f"human must be [S,T,{self.nhuman},7], got {human.shape}")
        S, T = human.shape[:2]
        q0 = np.ascontiguousarray(q0, dtype=np.float64)
        if q0.shape != (S, self.nq):
            raise ValueError(f"q0 must be [{S},{self.nq}], got {q0.shape}")
        if lens is not None:
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            if lens.shape != (S,):
                raise ValueError("lens must be [S]")
        scales = check_scales(scales, S, self.nhuman)
        weights = check_weights(weights, S, T, self.nhuman, lens=lens)
        q_out = np.zeros((S, T, self.nq), dtype=np.float64)
        nsolve = np.zeros((S, T, 2), dtype=np.int32)
        status = np.zeros(S, dtype=np.int32)
        targets = np.zeros((S, T, self.nhuman, 7), dtype=np.float64) if want_targets else None
        errors = np.zeros((S, T, 2), dtype=np.float64) if want_errors else None
        if weights is None:
            check(lib().gmr_retarget_streams_scaled(self.handle, S, T, _ptr(q0), _ptr(human), _ptr(lens), _ptr(scales), int(flags),
                                                    _ptr(q_out), _ptr(nsolve), _ptr(status), _ptr(targets), _ptr(errors)))
        else:
            check(lib().gmr_retarget_streams_weighted(self.handle, S, T, _ptr(q0), _ptr(human), _ptr(lens), _ptr(scales), _ptr(weights),
                                                      int(flags), _ptr(q_out), _ptr(nsolve), _ptr(status), _ptr(targets), _ptr(errors)))
        if want_targets or want_errors:
            return q_out, nsolve, status, targets, errors
        return q_out, nsolve, status

    def retarget_streams_dev(self, S, T, d_q0, d_human, d_len, flags, d_q_out, d_nsolve, d_status, stream=None,
                             d_tgt_out=None, d_err_out=None, d_scale=None, d_weight=None):
        """Device pointers (DeviceBuffer or raw c_void_p); asynchronous on `stream`.  ``d_scale``: f64 [S][nhuman] per-stream
        human scale tables, ``d_weight``: f64 [S][T][nhuman] per-frame body weights (both unchecked: the values are the caller's
        responsibility)."""
        if d_weight is not None:
            check(lib().gmr_retarget_streams_weighted_dev(self.handle, int(S), int(T), _d(d_q0), _d(d_human), _d(d_len), _d(d_scale),
                                                          _d(d_weight), int(flags), _d(d_q_out), _d(d_nsolve), _d(d_status),
                                                          _d(d_tgt_out), _d(d_err_out), _s(stream)))
            return
        if d_scale is None:
            check(lib().gmr_retarget_streams_dev(self.handle, int(S), int(T), _d(d_q0), _d(d_human), _d(d_len), int(flags),
                                                 _d(d_q_out), _d(d_nsolve), _d(d_status), _d(d_tgt_out), _d(d_err_out),
                                                 _s(stream)))
            return
        check(lib().gmr_retarget_streams_scaled_dev(self.handle, int(S), int(T), _d(d_q0), _d(d_human), _d(d_len), _d(d_scale),
                                                    int(flags), _d(d_q_out), _d(d_nsolve), _d(d_status), _d(d_tgt_out),
                                                    _d(d_err_out), _s(stream)))

    def close(self):
        if self.handle:
            lib().gmr_solver_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- array tables --------------------------------------------------------------------------------------------------------------------
# Every struct of array addresses has ONE table beside it.  A row ``(name, dtype, shape)`` is an array: its full shape, each axis a number
# or the name of a dimension the caller resolves -- "N" environments (or queries), "n" listed entries, "R" robot dofs, "extra_cols" and
# "obs_cols" of the proprioception, "nb" simulator bodies, "nsel" selected bodies, "C" reward columns, "E" caller columns, "H" / "O" / "P" /
# "A" of the rollout, "M" = H N rows of the loss.  A row ``(name, ctype)`` is a plain value among the addresses.  The struct's ``_fields_``
# and the ``*_FIELDS`` tuple are derived; :func:`resolve` / :func:`resolved` turn a table into shapes and :func:`host_inputs`, :func:`host_outputs` and
# :func:`device_struct` fill the struct from them.  A new block adds its tables here and nothing else.
def _fields(table):
    return [(row[0], C.c_void_p if len(row) == 3 else row[1]) for row in table]


def _arrays(table):
    return tuple(row[0] for row in table if len(row) == 3)


def resolve(table, **dims):
    """``{name: (dtype, shape, element count)}`` of the arrays of ``table`` under ``dims``"""
    out = {}
    for row in table:
        if len(row) == 3:
            shape = tuple(dims[s] if isinstance(s, str) else s for s in row[2])
            out[row[0]] = (row[1], shape, math.prod(shape))
    return out


_RESOLVED = {}


def resolved(table, **dims):
    """:func:`resolve`, done once per table and set of dimensions (always named in the same order): what a call in a training loop pays is
    a dictionary look-up"""
    key = (id(table), *dims.values())
    rows = _RESOLVED.get(key)
    if rows is None:
        rows = _RESOLVED[key] = resolve(table, **dims)
    return rows


def widths(table, **dims):
    """``{name: elements per environment}`` of the arrays of ``table``"""
    return {k: count for k, (_, _, count) in resolve(table, N=1, n=1, **dims).items()}


def _unknown(what, noun, given, rows):
    unknown = sorted(set(given) - set(rows))
    if unknown:
        raise TypeError(f"{what}: unknown {noun} {unknown}")


def host_inputs(struct, rows, arrays, what="", required=(), unknown=None, prefix=""):
    """The caller's host ``arrays`` (``{name: array or None}``) as a ``struct`` of addresses -> ``(struct, arrays to keep alive)``.  Each
    array is made contiguous in the dtype of its row of ``rows`` (:func:`resolve`) and its shape is checked; an ``int32`` row takes
    integers only; the absence of a name in ``required`` is refused, and with ``unknown`` (a noun) so is a name outside ``rows``."""
    if unknown:
        _unknown(what, unknown, arrays, rows)
    st, keep = struct() if isinstance(struct, type) else struct, []          # (an instance: go on filling it)
    for k, a in arrays.items():
        if a is None:
            if k in required:
                raise ValueError(f"{what}: {k} is needed")
            continue
        dtype, shape, _ = rows[k]
        if dtype == "int32":
            a = np.asarray(a)
            if not np.issubdtype(a.dtype, np.integer):
                raise TypeError(f"{prefix}{k}: integers needed, got {a.dtype}")
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != shape:
            raise ValueError(f"{prefix}{k}: shape {a.shape}, {shape} needed")
        keep.append(a)
        setattr(st, k, a.ctypes.data)
    return st, keep


def host_outputs(struct, rows, skip=()):
    """Freshly allocated arrays for the rows of ``rows`` that are not in ``skip`` -> ``(struct of their addresses, {name: array})``"""
    out = {k: np.empty(shape, dtype) for k, (dtype, shape, _) in rows.items() if k not in skip}
    return struct(**{k: a.ctypes.data for k, a in out.items()}), out


def device_struct(struct, rows, arrays, what="", required=(), unknown="outputs"):
    """:func:`host_inputs` for device memory: every value of ``arrays`` a :class:`DeviceBuffer`, a raw address or an object with
    ``data_ptr()``, taken through :func:`_dev_ptr` with the element count of its row.  A name outside ``rows`` is refused."""
    if not rows.keys() >= arrays.keys():
        _unknown(what, unknown, arrays, rows)
    st = struct()
    for k, x in arrays.items():
        if x is None:
            if k in required:
                raise ValueError(f"{what}: {k} is needed")
            continue
        dtype, _, count = rows[k]
        setattr(st, k, _dev_ptr(x, k, dtype, count).value)
    return st


def _dev_ptr(x, what: str, dtype: str, count: int):
    """Device address of an array of a ``*_dev`` call: None, a :class:`DeviceBuffer`, a raw address (``int`` / ``c_void_p``) or an
    object with ``data_ptr()``, whose dtype, contiguity and size are checked when it tells them."""
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        need = count * np.dtype(dtype).itemsize
        if x.nbytes < need:
            raise ValueError(f"{what}: buffer of {x.nbytes} bytes, {need} needed")
        return x.ptr
    if isinstance(x, C.c_void_p):
        return x
    if isinstance(x, (int, np.integer)):
        return C.c_void_p(int(x))
    if hasattr(x, "data_ptr"):
        if isinstance(x, np.ndarray) or getattr(getattr(x, "device", None), "type", "cuda") == "cpu":
            raise ValueError(f"{what}: host memory handed to a device entry point")
        if hasattr(x, "dtype") and str(x.dtype).split(".")[-1] != dtype:
            raise ValueError(f"{what}: dtype {x.dtype}, {dtype} needed")
        if hasattr(x, "is_contiguous") and not x.is_contiguous():
            raise ValueError(f"{what}: not contiguous")
        if hasattr(x, "numel") and x.numel() < count:
            raise ValueError(f"{what}: {x.numel()} elements, {count} needed")
        return C.c_void_p(int(x.data_ptr()))
    raise TypeError(f"{what}: cannot take a device address from {type(x).__name__}")


_F, _I = "float32", "int32"
FK_MAX_BODIES = 64
BODY_STATE = (("root_pos", _F, ("N", 3)), ("root_rot", _F, ("N", 4)), ("root_vel", _F, ("N", 3)), ("root_ang_vel", _F, ("N", 3)),
              ("dof_pos", _F, ("N", "R")), ("dof_vel", _F, ("N", "R")), ("body_pos", _F, ("N", "nsel", 3)), ("body_rot", _F, ("N", "nsel", 4)),
              ("body_vel", _F, ("N", "nsel", 3)), ("body_ang_vel", _F, ("N", "nsel", 3)), ("status", _I, ("N",)))
BODY_STATE_FIELDS = _arrays(BODY_STATE)


class BodyStateOut(C.Structure):
    """``gmr_body_state_out_t``: the outputs of ``gmr_motion_body_state[_dev]``, each an address or NULL"""
    _fields_ = _fields(BODY_STATE)


TRACKER_MAX_DOF = 64
TRACKER_TERMS = 6
TRACKER_OUT = (("ref_root_pos", _F, ("N", 3)), ("ref_root_rot", _F, ("N", 4)), ("ref_root_vel", _F, ("N", 3)), ("ref_root_ang_vel", _F, ("N", 3)),
               ("ref_dof_pos", _F, ("N", "R")), ("ref_dof_vel", _F, ("N", "R")), ("err", _F, ("N", 6)), ("term", _F, ("N", 6)), ("total", _F, ("N",)),
               ("status", _I, ("N",)), ("finished", _I, ("N",)))
TRACKER_SIM = (("base_pos", _F, ("N", 3)), ("base_quat", _F, ("N", 4)), ("base_lin_vel", _F, ("N", 3)), ("base_ang_vel", _F, ("N", 3)),
               ("dof_pos", _F, ("N", "R")), ("dof_vel", _F, ("N", "R")))
TRACKER_OUT_FIELDS, TRACKER_SIM_FIELDS = _arrays(TRACKER_OUT), _arrays(TRACKER_SIM)


class TrackerOut(C.Structure):
    """``gmr_tracker_out_t``: the outputs of ``gmr_motion_tracker_step[_dev]``, each an address or NULL"""
    _fields_ = _fields(TRACKER_OUT)


class TrackerSim(C.Structure):
    """``gmr_tracker_sim_t``: the simulator state of ``gmr_motion_tracker_step[_dev]``, each an address or NULL"""
    _fields_ = _fields(TRACKER_SIM)


TRACKER_LINK_TERMS = 4
TRACKER_FRAME_WORLD, TRACKER_FRAME_HEADING = 0, 1
TRACKER_NO_ADVANCE = 1
ANCHOR_YAW, ANCHOR_Z = 1, 2          # gmr_motion_tracker_anchor_to_root[_dev] flags (include/gmr_hip.h, "tracker anchors")
TRACKER_LINKS_OUT = (("ref_body_pos", _F, ("N", "nsel", 3)), ("ref_body_rot", _F, ("N", "nsel", 4)), ("ref_body_vel", _F, ("N", "nsel", 3)),
                     ("ref_body_ang_vel", _F, ("N", "nsel", 3)), ("link_err", _F, ("N", 4)), ("link_term", _F, ("N", 4)), ("max_dist", _F, ("N",)),
                     ("fail", _I, ("N",)))
# the separate arrays hold the selected bodies ("nsel"; for the feet: every body of the simulator); a packed tensor goes in by offsets and strides
TRACKER_LINKS_SIM = (("body_pos", _F, ("N", "nsel", 3)), ("body_rot", _F, ("N", "nsel", 4)), ("body_vel", _F, ("N", "nsel", 3)),
                     ("body_ang_vel", _F, ("N", "nsel", 3)), ("env_stride", C.c_int64), ("body_stride", C.c_int64))
TRACKER_LINKS_OUT_FIELDS, TRACKER_LINKS_SIM_FIELDS = _arrays(TRACKER_LINKS_OUT), _arrays(TRACKER_LINKS_SIM)


class TrackerLinksOut(C.Structure):
    """``gmr_tracker_links_out_t``: the link outputs of ``gmr_motion_tracker_step_links[_dev]``, each an address or NULL"""
    _fields_ = _fields(TRACKER_LINKS_OUT)


class TrackerLinksSim(C.Structure):
    """``gmr_tracker_links_sim_t``: the simulator's rigid-body state, four addresses (or NULL) and the two strides in floats"""
    _fields_ = _fields(TRACKER_LINKS_SIM)


CONTROL_MAX_DECIMATION = 64           # gmr_motion_tracker_set_control (include/gmr_hip.h, "tracker control")
TRACKER_ACTUATOR_FIELDS = ("stiffness", "damping", "friction", "torque_limit")


class TrackerActuator(C.Structure):
    """``gmr_tracker_actuator_t``: the actuators of ``gmr_motion_tracker_torques[_dev]``, four addresses (``friction`` and ``torque_limit``
    may be NULL) and whether the first three are ``[N][R]`` (1) or ``[R]`` (0)"""
    _fields_ = [(k, C.c_void_p) for k in TRACKER_ACTUATOR_FIELDS] + [("per_env", C.c_int32)]


# gmr_motion_tracker_set_proprio / _proprio[_dev] (include/gmr_hip.h, "tracker proprioception"): the penalties in column order (t1.py:622-625,
# :631-694) and the blocks that take sensor noise
PROPRIO_TERMS = ("lin_vel_z", "ang_vel_xy", "orientation", "torques", "dof_vel", "dof_acc", "root_acc", "action_rate", "dof_pos_limits",
                 "dof_vel_limits", "torque_limits", "torque_tiredness", "power", "base_height")
PROPRIO_MAX_EXTRA = 16
PROPRIO_NOISE_BLOCKS = ("gravity", "ang_vel", "dof_pos", "dof_vel", "lin_vel", "height")
NOISE_DISTRIBUTIONS = {"none": 0, "gaussian": 1, "uniform": 2}
NOISE_OPERATIONS = {"additive": 0, "scaling": 1}
PROPRIO_CONFIG_TABLES = ("default_dof_pos", "dof_pos_limits", "dof_vel_limits", "torque_limits", "scales")
PROPRIO_IN = (("root_states", _F, ("N", 13)), ("dof_pos", _F, ("N", "R")), ("dof_vel", _F, ("N", "R")), ("actions", _F, ("N", "R")),
              ("mean_torques", _F, ("N", "R")), ("extra", _F, ("N", "extra_cols")), ("ground", _F, ("N",)), ("episode_steps", _I, ("N",)))
PROPRIO_OUT = (("base_lin_vel", _F, ("N", 3)), ("base_ang_vel", _F, ("N", 3)), ("projected_gravity", _F, ("N", 3)), ("filtered_lin_vel", _F, ("N", 3)),
               ("filtered_ang_vel", _F, ("N", 3)), ("obs", _F, ("N", "obs_cols")), ("priv", _F, ("N", 4)), ("term", _F, ("N", len(PROPRIO_TERMS))),
               ("total", _F, ("N",)), ("done", _I, ("N",)))
PROPRIO_IN_FIELDS, PROPRIO_OUT_FIELDS = _arrays(PROPRIO_IN), _arrays(PROPRIO_OUT)


class ProprioNoise(C.Structure):
    """``gmr_proprio_noise_t``: one spec of ``apply_randomization``"""
    _fields_ = [("distribution", C.c_int32), ("operation", C.c_int32), ("a", C.c_double), ("b", C.c_double)]


class ProprioConfig(C.Structure):
    """``gmr_proprio_config_t``: the configuration of ``gmr_motion_tracker_set_proprio``, host addresses and values"""
    _fields_ = ([(k, C.c_void_p) for k in PROPRIO_CONFIG_TABLES] + [("extra_cols", C.c_int32), ("max_episode_steps", C.c_int32)]
                + [(k, C.c_double) for k in ("filter_weight", "soft_dof_pos_limit", "soft_dof_vel_limit", "soft_torque_limit")]
                + [(k, C.c_float) for k in ("scale_gravity", "scale_lin_vel", "scale_ang_vel", "scale_dof_pos", "scale_dof_vel",
                                            "base_height_target", "terminate_vel", "terminate_height")]
                + [("noise", ProprioNoise * len(PROPRIO_NOISE_BLOCKS))])


class ProprioIn(C.Structure):
    """``gmr_proprio_in_t``: the inputs of ``gmr_motion_tracker_proprio[_dev]``, each an address or NULL"""
    _fields_ = _fields(PROPRIO_IN)


class ProprioOut(C.Structure):
    """``gmr_proprio_out_t``: the outputs of ``gmr_motion_tracker_proprio[_dev]``, each an address or NULL"""
    _fields_ = _fields(PROPRIO_OUT)


# gmr_motion_tracker_set_terrain / _terrain_heights[_dev] / _set_feet / _feet[_dev] (include/gmr_hip.h, "tracker feet"): the terms in column
# order (t1.py:627-629, :696-730); FEET_DONE_CONTACT is the bit of ``done``, OR-able with the bits 0 to 2 of the proprioception's
FEET_TERMS = ("collision", "feet_slip", "feet_vel_z", "feet_roll", "feet_yaw_diff", "feet_yaw_mean", "feet_distance", "feet_swing")
FEET_MAX_EDGES, FEET_MAX_BODIES = 8, 64
FEET_DONE_CONTACT = 8
FEET_CONFIG_TABLES = ("edge_pos", "termination_body", "penalized_body", "scales")
FEET_IN = (("contact_forces", _F, ("N", "nb", 3)), ("root_states", _F, ("N", 13)), ("episode_steps", _I, ("N",)), ("gait_frequency", _F, ("N",)))
FEET_OUT = (("feet_pos", _F, ("N", 2, 3)), ("feet_roll", _F, ("N", 2)), ("feet_yaw", _F, ("N", 2)), ("feet_contact", _I, ("N", 2)), ("ground", _F, ("N",)),
            ("gait", _F, ("N", 2)), ("term", _F, ("N", len(FEET_TERMS))), ("total", _F, ("N",)), ("done", _I, ("N",)))
FEET_IN_FIELDS, FEET_OUT_FIELDS = _arrays(FEET_IN), _arrays(FEET_OUT)


class FeetConfig(C.Structure):
    """``gmr_feet_config_t``: the configuration of ``gmr_motion_tracker_set_feet``, host addresses and values"""
    _fields_ = ([(k, C.c_void_p) for k in FEET_CONFIG_TABLES] + [("feet_body", C.c_int32 * 2)]
                + [(k, C.c_int32) for k in ("num_edges", "nb", "num_termination", "num_penalized")]
                + [(k, C.c_double) for k in ("force_threshold", "contact_clearance", "feet_distance_ref", "swing_period")])


class FeetIn(C.Structure):
    """``gmr_feet_in_t``: the inputs of ``gmr_motion_tracker_feet[_dev]`` beside the bodies, each an address or NULL"""
    _fields_ = _fields(FEET_IN)


class FeetOut(C.Structure):
    """``gmr_feet_out_t``: the outputs of ``gmr_motion_tracker_feet[_dev]``, each an address or NULL"""
    _fields_ = _fields(FEET_OUT)


# gmr_motion_tracker_set_commands / _commands[_dev] / _set_disturbances / _disturb[_dev] (include/gmr_hip.h, "tracker commands"): the terms in
# column order (t1.py:606-620), the bits of ``flags`` and of the disturbances
CMD_TERMS = ("survival", "tracking_lin_vel_x", "tracking_lin_vel_y", "tracking_ang_vel")
CMD_MAX_LEVELS, CMD_CHUNK = 20, 8
CMD_BOUNDARY, CMD_RESAMPLED, CMD_SUCCESS = 1, 2, 4
CMD_INDEX_ORDERS = {"grid": 0, "reference": 1}
DISTURB_KICK, DISTURB_PUSH_START, DISTURB_PUSH_STOP = 1, 2, 4
DISTURB_SPECS = ("kick_lin_vel", "kick_ang_vel", "push_force", "push_torque")
CMD_IN = (("episode_steps", _I, ("N",)), ("done", _I, ("N",)), ("lin_vel", _F, ("N", 3)), ("ang_vel", _F, ("N", 3)))
# cmd_obs is three columns inside the caller's rows of cmd_obs_stride floats; the two pushes of the disturbances lie in rows of their strides
CMD_OUT = (("term", _F, ("N", len(CMD_TERMS))), ("total", _F, ("N",)), ("commands", _F, ("N", 3)), ("gait_frequency", _F, ("N",)), ("flags", _I, ("N",)),
           ("cmd_obs", _F, ("N", 3)), ("cmd_obs_stride", C.c_int64))
DISTURB_IO = (("root_states", _F, ("N", 13)), ("push_force", _F, ("N", 3)), ("push_torque", _F, ("N", 3)), ("push_force_stride", C.c_int64),
              ("push_torque_stride", C.c_int64), ("push_obs", _F, ("N", 6)))
CMD_IN_FIELDS, CMD_OUT_FIELDS, DISTURB_IO_FIELDS = _arrays(CMD_IN), _arrays(CMD_OUT), _arrays(DISTURB_IO)


class CommandsConfig(C.Structure):
    """``gmr_commands_config_t``: the configuration of ``gmr_motion_tracker_set_commands``, values only"""
    _fields_ = ([(k, C.c_double * 2) for k in ("lin_vel_x", "lin_vel_y", "ang_vel_yaw", "gait_frequency")]
                + [(k, C.c_double) for k in ("still_proportion", "tracking_sigma", "update_rate")]
                + [("toler", C.c_double * 3), ("resolution", C.c_double * 3), ("scales", C.c_float * len(CMD_TERMS)), ("obs_scale", C.c_float * 3),
                   ("resample_steps", C.c_int32 * 2)]
                + [(k, C.c_int32) for k in ("curriculum", "lin_vel_levels", "ang_vel_levels", "min_success_steps", "index_order")])


class CommandsIn(C.Structure):
    """``gmr_commands_in_t``: the inputs of ``gmr_motion_tracker_commands[_dev]``, each an address or NULL"""
    _fields_ = _fields(CMD_IN)


class CommandsOut(C.Structure):
    """``gmr_commands_out_t``: the outputs of ``gmr_motion_tracker_commands[_dev]``, each an address or NULL, and the row stride of ``cmd_obs``"""
    _fields_ = _fields(CMD_OUT)


class DisturbConfig(C.Structure):
    """``gmr_disturb_config_t``: the configuration of ``gmr_motion_tracker_set_disturbances``"""
    _fields_ = ([(k, ProprioNoise) for k in DISTURB_SPECS] + [(k, C.c_int32) for k in ("kick_every", "push_every", "push_duration")]
                + [("scale_push_force", C.c_float), ("scale_push_torque", C.c_float)])


class DisturbIo(C.Structure):
    """``gmr_disturb_io_t``: what ``gmr_motion_tracker_disturb[_dev]`` writes, each an address or NULL, and the two row strides"""
    _fields_ = _fields(DISTURB_IO)


# gmr_motion_tracker_set_reset_states / _reset_states[_dev] / _set_rewards / _rewards[_dev] / _reward_stats[_dev] (include/gmr_hip.h,
# "tracker episode")
RESET_SPECS = ("init_dof_pos", "init_base_pos_xy", "init_base_lin_vel_xy")
REWARD_MAX_EXTRA, REWARD_MAX_COLS = 16, 52
REWARD_BLOCKS = {"terms": 1, "links": 2, "proprio": 4, "feet": 8, "commands": 16}      # the bits of gmr_reward_config_t.blocks, in column order
REWARD_LOCOMOTION, REWARD_IMITATION = 1, 2                                             # the bits of a column's ``groups`` entry
REWARD_DONE_TIME_OUT = 4
RESET_IO = (("root_states", _F, ("N", 13)), ("dof_pos", _F, ("N", "R")), ("dof_vel", _F, ("N", "R")), ("delay_steps", _I, ("N",)),
            ("episode_steps", _I, ("N",)), ("init_root_states", _F, ("n", 13)), ("init_dof_pos", _F, ("n", "R")), ("init_dof_vel", _F, ("n", "R")))
REWARD_IN = (("term", _F, ("N", TRACKER_TERMS)), ("link_term", _F, ("N", TRACKER_LINK_TERMS)), ("proprio_term", _F, ("N", len(PROPRIO_TERMS))),
             ("feet_term", _F, ("N", len(FEET_TERMS))), ("cmd_term", _F, ("N", len(CMD_TERMS))), ("extra", _F, ("N", "E")), ("done", _I, ("N",)),
             ("flags", _I, ("N",)))
REWARD_OUT = (("reward", _F, ("N",)), ("scaled", _F, ("N", "C")), ("group_total", _F, ("N", 2)), ("reset", _I, ("N",)), ("time_outs", _I, ("N",)))
RESET_IO_FIELDS, REWARD_IN_FIELDS, REWARD_OUT_FIELDS = _arrays(RESET_IO), _arrays(REWARD_IN), _arrays(REWARD_OUT)


class ResetConfig(C.Structure):
    """``gmr_reset_config_t``: the configuration of ``gmr_motion_tracker_set_reset_states``, values and two host addresses"""
    _fields_ = ([("base_init_state", C.c_float * 13), ("default_dof_pos", C.c_void_p), ("env_origins", C.c_void_p)]
                + [(k, ProprioNoise) for k in RESET_SPECS] + [("yaw_range", C.c_double * 2)]
                + [(k, C.c_int32) for k in ("yaw", "decimation", "use_terrain")])


class ResetIo(C.Structure):
    """``gmr_reset_io_t``: the arrays of ``gmr_motion_tracker_reset_states[_dev]``, each an address or NULL"""
    _fields_ = _fields(RESET_IO)


class RewardConfig(C.Structure):
    """``gmr_reward_config_t``: the configuration of ``gmr_motion_tracker_set_rewards``, values only"""
    _fields_ = ([("group_weight", C.c_float * 2), ("extra_weights", C.c_float * REWARD_MAX_EXTRA), ("only_positive", C.c_int32 * 2)]
                + [(k, C.c_int32) for k in ("blocks", "extra_cols", "stats")] + [("groups", C.c_uint8 * REWARD_MAX_COLS)])


class RewardIn(C.Structure):
    """``gmr_reward_in_t``: the inputs of ``gmr_motion_tracker_rewards[_dev]``, each an address or NULL"""
    _fields_ = _fields(REWARD_IN)


class RewardOut(C.Structure):
    """``gmr_reward_out_t``: the outputs of ``gmr_motion_tracker_rewards[_dev]``, each an address or NULL"""
    _fields_ = _fields(REWARD_OUT)


# gmr_motion_tracker_set_rollout / _record[_dev] / _advantages[_dev] (include/gmr_hip.h, "tracker rollout")
ROLLOUT_ENVS, ROLLOUT_FOLD = 64, 64
ROLLOUT_IO = (("obs", _F, ("H", "N", "O")), ("priv", _F, ("H", "N", "P")), ("actions", _F, ("H", "N", "A")), ("rewards", _F, ("H", "N")),
              ("dones", "uint8", ("H", "N")), ("time_outs", "uint8", ("H", "N")))
ROLLOUT_OUT = (("advantages", _F, ("H", "N")), ("returns", _F, ("H", "N")), ("normalized", _F, ("H", "N")), ("stats", "float64", (4,)))
ROLLOUT_IO_FIELDS, ROLLOUT_OUT_FIELDS = _arrays(ROLLOUT_IO), _arrays(ROLLOUT_OUT)


class RolloutIo(C.Structure):
    """``gmr_rollout_io_t``: the caller's rollout arrays, each an address or NULL"""
    _fields_ = _fields(ROLLOUT_IO)


class RolloutOut(C.Structure):
    """``gmr_rollout_out_t``: the outputs of ``gmr_motion_tracker_advantages[_dev]``, each an address or NULL"""
    _fields_ = _fields(ROLLOUT_OUT)


# gmr_motion_tracker_set_loss / _loss_state / _log_prob[_dev] / _loss[_dev] (include/gmr_hip.h, "tracker loss")
LOSS_ROWS, LOSS_FOLD, LOSS_MAX_ACT = 64, 64, 32
LOSS_TERMS = ("value_loss", "actor_loss", "bound_loss", "entropy", "loss", "kl_mean", "learning_rate", "clip_fraction")
LOSS_STATE = ("bound_coef", "entropy_coef", "desired_kl", "learning_rate", "e_clip", "lr_min", "lr_max", "lr_factor")
LOSS_IN = (("loc", _F, ("M", "A")), ("logstd", _F, ("A",)), ("actions", _F, ("M", "A")), ("old_log_prob", _F, ("M",)), ("values", _F, ("M",)),
           ("returns", _F, ("M",)), ("advantages", _F, ("M",)), ("old_loc", _F, ("M", "A")), ("old_logstd", _F, ("A",)))
LOSS_OUT = (("grad_loc", _F, ("M", "A")), ("grad_logstd", _F, ("A",)), ("grad_values", _F, ("M",)), ("log_prob", _F, ("M",)),
            ("terms", "float64", (len(LOSS_TERMS),)))
LOSS_IN_FIELDS, LOSS_OUT_FIELDS = _arrays(LOSS_IN), _arrays(LOSS_OUT)


# gmr_motion_tracker_set_optimizer / _optimizer_step[_dev] / _optimizer_state / _optimizer_load_state (include/gmr_hip.h, "tracker optimiser")
OPT_CHUNK, OPT_MAX_TENSORS = 1024, 32
OPT_INFO = ("total_norm", "coef", "learning_rate", "step")

# gmr_motion_tracker_set_policy / _act[_dev] / _values[_dev] / _policy_state (include/gmr_hip.h, "tracker policy"): the arrays of a call
# per network, the parameters and the hidden activations aside (lists, their shapes follow from set_policy)
POLICY_TILE, POLICY_MAX_HIDDEN, POLICY_WIDTH_STEP, POLICY_MAX_WIDTH, POLICY_MAX_IN, POLICY_MAX_TENSORS = 32, 4, 32, 256, 512, 21
POLICY_ACT = (("obs", _F, ("M", "O")), ("loc", _F, ("M", "A")), ("actions", _F, ("M", "A")))
POLICY_VALUES = (("obs", _F, ("M", "O")), ("priv", _F, ("M", "P")), ("values", _F, ("M",)))
POLICY_SHAPE = 16                        # the i32 words of gmr_motion_tracker_policy_state

# gmr_motion_tracker_set_backward / _act_backward[_dev] / _values_backward[_dev] / _backward_state (include/gmr_hip.h, "tracker policy backward")
POLICY_BWD_CHUNK, POLICY_BWD_MAX_ROWS = 256, 131072
POLICY_BWD_STATE = ("chunk", "chunks", "workspace_bytes", "max_rows", "actor_tiles", "critic_tiles")      # the i64 words of _backward_state


class LossIn(C.Structure):
    """``gmr_loss_in_t``: the inputs of ``gmr_motion_tracker_loss[_dev]``, each an address (``old_loc``, ``old_logstd``: or NULL)"""
    _fields_ = _fields(LOSS_IN)


class LossOut(C.Structure):
    """``gmr_loss_out_t``: the outputs of ``gmr_motion_tracker_loss[_dev]``, each an address or NULL"""
    _fields_ = _fields(LOSS_OUT)


# gmr_motion_tracker_set_preview: the block bits in row order, the frames and the limits (include/gmr_hip.h, "tracker preview")
PREVIEW_BLOCKS = {"root_pos": 1, "root_quat": 2, "root_rot6": 4, "root_vel": 8, "root_ang_vel": 16, "dof_pos": 32, "dof_vel": 64, "body_pos": 128}
PREVIEW_FRAME_RAW, PREVIEW_FRAME_REFERENCE, PREVIEW_FRAME_SIM = 0, 1, 2
PREVIEW_MAX_OFFSETS, PREVIEW_MAX_BODIES = 16, 32


class FkHandle:
    """Device-resident KinematicsModel tree: handle behind gmr_fk_create."""

    def __init__(self, tree: dict):
        require_gpu()
        self.nbody = int(len(tree["parent"]))
        self.ndof = int((np.asarray(tree["dof_dim"]) > 0).sum())
        self._keep = [np.ascontiguousarray(tree["parent"], dtype=np.int32),
                      np.ascontiguousarray(tree["local_translation"], dtype=np.float32),
                      np.ascontiguousarray(tree["local_rotation"], dtype=np.float32),
                      np.ascontiguousarray(tree["dof_idx"], dtype=np.int32),
                      np.ascontiguousarray(tree["axis"], dtype=np.float64)]
        h = C.c_void_p()
        check(lib().gmr_fk_create(self.nbody, *[_ptr(a) for a in self._keep], self.ndof, C.byref(h)))
        self.handle = h

    def fk(self, root_pos, root_rot, dof, want_rot=True, want_min_z=False):
        root_pos = np.ascontiguousarray(root_pos, dtype=np.float32)
        root_rot = np.ascontiguousarray(root_rot, dtype=np.float32)
        dof = np.ascontiguousarray(dof, dtype=np.float32)
        B = root_pos.shape[0]
        if root_pos.shape != (B, 3) or root_rot.shape != (B, 4) or dof.shape != (B, self.ndof):
            raise ValueError("shape mismatch in fk inputs")
        bp = np.zeros((B, self.nbody, 3), dtype=np.float32)
        br = np.zeros((B, self.nbody, 4), dtype=np.float32) if want_rot else None
        mz = np.zeros(1, dtype=np.float32) if want_min_z else None
        check(lib().gmr_fk_batch(self.handle, B, _ptr(root_pos), _ptr(root_rot), _ptr(dof), _ptr(bp), _ptr(br), _ptr(mz)))
        return bp, br, (float(mz[0]) if want_min_z else None)

    def fk_segments(self, root_pos, root_rot, dof, seg_start, want_pos=True):
        """Many clips in one launch: rows [seg_start[g], seg_start[g + 1]) are clip g.  Returns (body_pos [B, nb, 3] or None,
        seg_min_z [nseg]): the per-clip minimum of body_pos z (gmr_fk_batch_segments)."""
        root_pos = np.ascontiguousarray(root_pos, dtype=np.float32)
        root_rot = np.ascontiguousarray(root_rot, dtype=np.float32)
        dof = np.ascontiguousarray(dof, dtype=np.float32)
        seg_start = np.ascontiguousarray(seg_start, dtype=np.int32)
        B, nseg = root_pos.shape[0], len(seg_start) - 1
        if root_pos.shape != (B, 3) or root_rot.shape != (B, 4) or dof.shape != (B, self.ndof) or nseg < 0:
            raise ValueError("shape mismatch in fk inputs")
        bp = np.zeros((B, self.nbody, 3), dtype=np.float32) if want_pos else None
        mz = np.zeros(max(nseg, 0), dtype=np.float32)
        check(lib().gmr_fk_batch_segments(self.handle, B, _ptr(root_pos), _ptr(root_rot), _ptr(dof), nseg, _ptr(seg_start),
                                          _ptr(bp), _ptr(mz)))
        return bp, mz

    def fk_dev(self, B, d_root_pos, d_root_rot, d_dof, d_body_pos, d_body_rot=None, d_min_z=None, stream=None):
        check(lib().gmr_fk_batch_dev(self.handle, int(B), _d(d_root_pos), _d(d_root_rot), _d(d_dof), _d(d_body_pos),
                                     _d(d_body_rot), _d(d_min_z), _s(stream)))

    def postprocess_clips_dev(self, sources, d_seg_start, C_clips, B, d_root_pos, d_root_rot, d_dof_pos, d_local_body_pos,
                              d_lowest=None, height_adjust=True, root_origin_offset=True, ground_offset=0.0, stream=None):
        """``gmr_postprocess_clips_dev``: the five pkl arrays of ``B`` frames in ``C_clips`` clips straight from IK outputs on the
        device.  ``sources`` = list of ``(S, T, d_q_out, d_len or None)``, one per IK job, clips numbered in this order;
        ``d_seg_start`` i32[C + 1] = exclusive prefix sum of the clip lengths.  Device pointers (DeviceBuffer or raw);
        asynchronous on ``stream``."""
        arr = (PostSrc * max(len(sources), 1))()
        for i, (S, T, d_q, d_len) in enumerate(sources):
            arr[i] = PostSrc(int(S), int(T), _addr(d_q), _addr(d_len))
        flags = (POST_HEIGHT_ADJUST if height_adjust else 0) | (POST_ROOT_ORIGIN_OFFSET if root_origin_offset else 0)
        check(lib().gmr_postprocess_clips_dev(self.handle, C.cast(arr, C.c_void_p), len(sources), self.ndof + 7, _d(d_seg_start),
                                              int(C_clips), int(B), flags, float(ground_offset), _d(d_root_pos), _d(d_root_rot),
                                              _d(d_dof_pos), _d(d_local_body_pos), _d(d_lowest), _s(stream)))

    def close(self):
        if self.handle:
            lib().gmr_fk_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def smplx_target_times(N: int, nout: int) -> np.ndarray:
    """``np.linspace(0, N - 1, nout)`` as the batch kernels compute it (``gmr_smplx_target_times``; host code, no GPU needed)"""
    out = np.empty(int(nout), dtype=np.float64)
    check(lib().gmr_smplx_target_times(int(N), int(nout), _ptr(out)))
    return out


class SmplxHandle:
    """Kinematic tree + joint selection behind gmr_smplx_create (N1: SMPL-X frame extraction)."""

    def __init__(self, parents, sel=None):
        require_gpu()
        self.parents = np.ascontiguousarray(parents, dtype=np.int32)
        self.J = int(len(self.parents))
        self.sel = None if sel is None else np.ascontiguousarray(sel, dtype=np.int32)
        h = C.c_void_p()
        check(lib().gmr_smplx_create(self.J, _ptr(self.parents), 0 if self.sel is None else len(self.sel),
                                     _ptr(self.sel), C.byref(h)))
        self.handle = h
        self.rows = int(lib().gmr_smplx_rows(h))

    def joints(self, j_rest, full_pose, transl):
        j_rest = np.ascontiguousarray(j_rest, dtype=np.float64)
        full_pose = np.ascontiguousarray(full_pose, dtype=np.float32).reshape(-1, self.J, 3)
        transl = np.ascontiguousarray(transl, dtype=np.float32).reshape(-1, 3)
        N = full_pose.shape[0]
        if j_rest.shape != (self.J, 3) or transl.shape[0] != N:
            raise ValueError("shape mismatch in smplx joints inputs")
        out = np.zeros((N, self.J, 3), dtype=np.float32)
        check(lib().gmr_smplx_joints(self.handle, N, _ptr(j_rest), _ptr(full_pose), _ptr(transl), _ptr(out)))
        return out

    def align(self, full_pose, joints, target_time=None):
        full_pose = np.ascontiguousarray(full_pose, dtype=np.float32).reshape(-1, self.J, 3)
        joints = np.ascontiguousarray(joints, dtype=np.float32)
        N = full_pose.shape[0]
        if joints.ndim != 3 or joints.shape[0] != N or joints.shape[1] < self.J or joints.shape[2] != 3:
            raise ValueError("joints must be [N, >=J, 3]")
        tt = None if target_time is None else np.ascontiguousarray(target_time, dtype=np.float64)
        nout = N if tt is None else int(len(tt))
        out = np.zeros((nout, self.rows, 7), dtype=np.float64)
        check(lib().gmr_smplx_align(self.handle, N, int(joints.shape[1]), _ptr(full_pose), _ptr(joints), nout, _ptr(tt),
                                    _ptr(out)))
        return out

    def frames(self, j_rest, full_pose, transl, target_time=None):
        """Joints-only body model + alignment of the selected rows in one call (``gmr_smplx_frames``): the packed frames
        ``f64[Nout, rows, 7]`` only; bit-identical to :meth:`joints` followed by :meth:`align`."""
        full_pose = np.ascontiguousarray(full_pose, dtype=np.float32).reshape(-1, self.J, 3)
        N = full_pose.shape[0]
        j_rest = np.ascontiguousarray(j_rest, dtype=np.float64)
        transl = np.ascontiguousarray(transl, dtype=np.float32).reshape(N, 3)
        if j_rest.shape != (self.J, 3):
            raise ValueError(f"j_rest must be [{self.J}, 3]")
        tt = None if target_time is None else np.ascontiguousarray(target_time, dtype=np.float64)
        nout = N if tt is None else len(tt)
        out = np.empty((nout, self.rows, 7), dtype=np.float64)
        check(lib().gmr_smplx_frames(self.handle, N, _ptr(j_rest), _ptr(full_pose), _ptr(transl), nout, _ptr(tt), _ptr(out)))
        return out

    def compact_layout(self):
        """(pose_joints, row_joints): the joints whose poses / positions the alignment reads, in the order of the compact
        inputs of :meth:`align_compact_dev`."""
        pj = np.zeros(self.J, dtype=np.int32)
        rj = np.zeros(self.J, dtype=np.int32)
        npose, nrow = C.c_int(), C.c_int()
        check(lib().gmr_smplx_compact_layout(self.handle, _ptr(pj), C.byref(npose), _ptr(rj), C.byref(nrow)))
        return pj[: npose.value].copy(), rj[: nrow.value].copy()

    def align_compact_dev(self, N, d_pose_c, d_joints_c, nout, d_target_time, d_out, stream=None):
        check(lib().gmr_smplx_align_compact_dev(self.handle, int(N), _d(d_pose_c), _d(d_joints_c), int(nout), _d(d_target_time),
                                                _d(d_out), _s(stream)))

    def align_dev(self, N, jstride, d_full_pose, d_joints, nout, d_target_time, d_out, stream=None):
        check(lib().gmr_smplx_align_dev(self.handle, int(N), int(jstride), _d(d_full_pose), _d(d_joints), int(nout),
                                        _d(d_target_time), _d(d_out), _s(stream)))

    def joints_dev(self, N, d_j_rest, d_full_pose, d_transl, d_joints, stream=None):
        check(lib().gmr_smplx_joints_dev(self.handle, int(N), _d(d_j_rest), _d(d_full_pose), _d(d_transl), _d(d_joints),
                                         _s(stream)))

    @property
    def batch_takes(self) -> bool:
        """whether :meth:`batch_frames_dev` / :meth:`batch_frames` take this selection (its ancestor closure inside joints 0..21)"""
        return bool(lib().gmr_smplx_batch_takes(self.handle))

    def batch_frames_dev(self, nclip, B, d_root_orient, d_pose_body, d_trans, d_src_start, d_nout, d_align, d_j_rest, d_clip_out,
                         stream=None):
        """``gmr_smplx_batch_frames_dev``: the packed frames of ``nclip`` clips (``B`` source frames, concatenated) written at the
        device addresses of the table ``d_clip_out`` -- asynchronous, nothing comes back to the host."""
        check(lib().gmr_smplx_batch_frames_dev(self.handle, int(nclip), int(B), _d(d_root_orient), _d(d_pose_body), _d(d_trans),
                                               _d(d_src_start), _d(d_nout), _d(d_align), _d(d_j_rest), _d(d_clip_out), _s(stream)))

    def batch_frames(self, root_orient, pose_body, trans, src_start, nout, align, j_rest, T=None):
        """``gmr_smplx_batch_frames``: ``root_orient f32[B,3]``, ``pose_body f32[B,63]``, ``trans f32[B,3]`` of the clips
        ``src_start i32[nclip + 1]`` with ``nout i32[nclip]`` output frames each, ``align`` (per clip: fps alignment or frame by
        frame) and ``j_rest f64[nclip,J,3]`` -> ``human f64[nclip, T, rows, 7]`` (``T`` defaults to the largest ``nout``;
        frames at or beyond ``nout[c]`` are zeros).  The bits of one :meth:`frames` call per clip."""
        seg = np.ascontiguousarray(src_start, dtype=np.int32)
        nclip = len(seg) - 1
        root_orient = np.ascontiguousarray(root_orient, dtype=np.float32).reshape(-1, 3)
        B = root_orient.shape[0]
        pose_body = np.ascontiguousarray(pose_body, dtype=np.float32).reshape(B, 63)
        trans = np.ascontiguousarray(trans, dtype=np.float32).reshape(B, 3)
        nout = np.ascontiguousarray(nout, dtype=np.int32)
        align = np.ascontiguousarray(align, dtype=np.uint8)
        j_rest = np.ascontiguousarray(j_rest, dtype=np.float64)
        if nclip < 0 or nout.shape != (nclip,) or align.shape != (nclip,) or j_rest.shape != (nclip, self.J, 3):
            raise ValueError(f"nout, align must be [{nclip}], j_rest [{nclip}, {self.J}, 3]")
        if T is None:
            T = max(int(nout.max()) if nclip else 0, 1)
        out = np.zeros((nclip, int(T), self.rows, 7), dtype=np.float64)
        check(lib().gmr_smplx_batch_frames(self.handle, nclip, B, _ptr(root_orient), _ptr(pose_body), _ptr(trans), _ptr(seg), _ptr(nout),
                                           _ptr(align), _ptr(j_rest), int(T), _ptr(out)))
        return out

    def close(self):
        if self.handle:
            lib().gmr_smplx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BvhHandle:
    """BVH topology + row selection behind gmr_bvh_create (N2: raw channel rows -> packed human frames)."""

    def __init__(self, parents, channels: int, order: str, sel_pos, sel_rot):
        require_gpu()
        self.parents = np.ascontiguousarray(parents, dtype=np.int32)
        self.J = int(len(self.parents))
        self.sel_pos = np.ascontiguousarray(sel_pos, dtype=np.int32)
        self.sel_rot = np.ascontiguousarray(sel_rot, dtype=np.int32)
        if self.sel_pos.shape != self.sel_rot.shape or self.sel_pos.ndim != 1:
            raise ValueError("sel_pos and sel_rot are two lists of the same length")
        self.rows = int(len(self.sel_pos))
        h = C.c_void_p()
        check(lib().gmr_bvh_create(self.J, _ptr(self.parents), int(channels), str(order).encode(), self.rows, _ptr(self.sel_pos),
                                   _ptr(self.sel_rot), C.byref(h)))
        self.handle = h
        self.ncol = int(lib().gmr_bvh_columns(h))

    def frames(self, rows, seg_start, offsets, T=None):
        """``gmr_bvh_frames``: ``rows f64[B, ncol]`` of the clips ``seg_start i32[nclip + 1]`` with ``offsets f64[nclip, J, 3]``
        -> ``human f64[nclip, T, rows, 7]`` (``T`` defaults to the longest clip; frames beyond a clip's length are zeros)."""
        rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, self.ncol)
        seg = np.ascontiguousarray(seg_start, dtype=np.int32)
        nclip = len(seg) - 1
        offsets = np.ascontiguousarray(offsets, dtype=np.float64)
        if nclip < 0 or offsets.shape != (nclip, self.J, 3):
            raise ValueError(f"offsets must be [{nclip}, {self.J}, 3]")
        if T is None:
            T = max(int(np.diff(seg).max()) if nclip else 0, 1)
        out = np.zeros((nclip, int(T), self.rows, 7), dtype=np.float64)
        check(lib().gmr_bvh_frames(self.handle, nclip, rows.shape[0], _ptr(rows), _ptr(seg), _ptr(offsets), int(T), _ptr(out)))
        return out

    def frames_dev(self, nclip, B, d_rows, d_seg_start, d_offsets, T, d_human, stream=None):
        check(lib().gmr_bvh_frames_dev(self.handle, int(nclip), int(B), _d(d_rows), _d(d_seg_start), _d(d_offsets), int(T),
                                       _d(d_human), _s(stream)))

    def close(self):
        if self.handle:
            lib().gmr_bvh_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
