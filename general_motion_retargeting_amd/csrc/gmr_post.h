// gmr_post.h -- the table of IK outputs a post-processing call reads (gmr_post.hip), shared with its entry point at the end of that file.
#pragma once
#include <stdint.h>

namespace gmr {

constexpr int POST_MAX_SRC = 8;   // like the jobs of gmr_retarget_group_window_dev

// gmr_post_src_t[nsrc] as a kernel argument: clips clip0[k] .. clip0[k + 1] - 1 are the streams of source k
struct PostSources {
  int32_t nsrc;
  int32_t clip0[POST_MAX_SRC + 1];
  int32_t T[POST_MAX_SRC];
  const double* q_out[POST_MAX_SRC];
  const int32_t* len[POST_MAX_SRC];
};

}  // namespace gmr
