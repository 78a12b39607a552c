// gmr_ik_weight_stage.h -- the per-frame body weights of an IK job (gmr_retarget_streams_weighted, gmr_retarget_group_weighted),
// stated ONCE next to gmr_ik_stage.h: gmr_job_t is closed (88 bytes, scale last), so the array travels beside the job list and
// is no row of kIkFields.  It is one more per-frame INPUT: f64 [S][T][nhuman], a row of 8 nhuman bytes per frame, carved on a
// 256-byte boundary like every array of a job, with slice and window copies of the form of `human`'s.  Plain C++ without HIP:
// gmr_ik_host.hip issues what this header describes, tests/cpp/ik_weight_stage_check.cpp runs the same code with memcpy.
#pragma once
#include "gmr_ik_stage.h"

namespace gmr {

constexpr int IK_WEIGHT = IK_NFIELD;      // what IkCopy::field says in a copy of the weight array (no row of kIkFields)

// S streams of a job's weights in a workspace; a job without the array takes no bytes (row = 0)
struct IkWeightOff {
  size_t S, T, at, row;
  size_t stride() const { return T * row; }      // from one stream to the next
};
// Carve it BEFORE the job's own arrays: [0, out_begin) of a workspace then holds every input, and the one staged H2D copy of a
// small call covers it.
inline IkWeightOff ik_carve_weight(Carve& c, const double* weight, size_t nhuman, size_t S, size_t T) {
  IkWeightOff o;
  o.S = S; o.T = T;
  o.row = weight ? 8 * nhuman : 0;
  o.at = c.take(S * o.stride());
  return o;
}
// the device pointer a kernel gets: null for a job without weights
inline const double* ik_weight_at(char* d, const IkWeightOff& o) { return o.row ? reinterpret_cast<const double*>(d + o.at) : nullptr; }

// the streams [s0, s0 + o.S): one plain piece; returns the number of copies (0 without the array or without streams)
inline int ik_weight_slice_copy(const IkWeightOff& o, size_t s0, IkCopy* c) {
  if (!o.row || !o.S) return 0;
  *c = IkCopy{IK_WEIGHT, s0 * o.stride(), o.at, 0, o.S * o.stride(), 1};
  return 1;
}
// the frames [tb, min(te, T)) of every stream: o.S pieces, a stream's row apart (none when tb >= T)
inline int ik_weight_window_copy(const IkWeightOff& o, size_t tb, size_t te, IkCopy* c) {
  if (te > o.T) te = o.T;
  if (!o.row || !o.S || tb >= te) return 0;
  *c = IkCopy{IK_WEIGHT, tb * o.row, o.at + tb * o.row, o.T * o.row, (te - tb) * o.row, o.S};
  return 1;
}

}  // namespace gmr
