// gmr_fk_handle.h -- the FK handle of the C-ABI (not part of the C-ABI): created in gmr_fk.hip, read by gmr_post.hip and, through
// gmr_handles.h, by gmr_body_state.hip and the motion tracker.  A header of its own, so that the FK and post-processing
// sources do not see the tracker's headers.
#pragma once
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
