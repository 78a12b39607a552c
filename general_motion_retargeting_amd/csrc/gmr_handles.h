// gmr_handles.h -- the handles of the C-ABI that more than one translation unit of libgmrhip.so looks into (not part of the
// C-ABI): the FK tree (created in gmr_abi.hip) and the motion library (gmr_motion.hip), both read by gmr_body_state.hip.
#pragma once
#include <stdint.h>

#include "../../include/gmr_hip.h"
#include "gmr_fk_tree.h"
#include "gmr_workspace.h"

struct gmr_fk {
  gmr::FkTree tree;
  gmr::DeviceBlock d_tree;       // the tree as the kernels read it
  const gmr::FkTree* dev() const { return (const gmr::FkTree*)d_tree.data(); }
  gmr::DeviceBlock min_part;     // gmr_fk_batch_dev: one float per block of the min_z reduction
  gmr::StreamWorkspace post_ws;  // gmr_postprocess_clips_dev
};

namespace gmr {
// the arrays of a motion library as its kernels see them (device pointers into the library's one block)
struct MotionArrays {
  int C, B, ndof, nbody;
  const int32_t* seg_start;   // [C + 1], validated on the host when the library was created
  const double* fps;          // [C]
  float *root_pos, *root_rot, *dof_pos, *local_body_pos, *root_vel, *root_ang_vel, *dof_vel, *stats;
};
}  // namespace gmr

struct gmr_motion_lib {
  gmr::MotionArrays A;
  gmr::DeviceBlock block;        // every array of the library: one allocation
  size_t off[GMR_MOTION_FPS + 1], bytes[GMR_MOTION_FPS + 1];
  int filled = 0;                // 1 once a fill has been enqueued
  int has_body = 0;              // the fill was given local_body_pos
  int reference_angvel = 0;      // the fill was asked for GMR_MOTION_ANGVEL_REFERENCE: root_ang_vel is not a physical angular velocity
};
