// gmr_ik_stage.h -- the arrays of an IK job (gmr_job_t), stated ONCE: what each holds, where it lies in a device workspace, which
// copies move a slice or a window of it, and the integer rules that decide how a batch is cut.  Plain C++ without HIP:
// gmr_ik_host.hip issues what this header describes, tests/cpp/ik_stage_check.cpp runs the same code with memcpy under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gmr_hip.h"
#include "gmr_workspace.h"

namespace gmr {

// the workspace order; [IK_Q_OUT, end) is what the kernel writes and what a zero-fill covers
enum { IK_Q0, IK_HUMAN, IK_LEN, IK_SCALE, IK_Q_OUT, IK_NSOLVE, IK_STATUS, IK_TGT_OUT, IK_ERR_OUT, IK_NFIELD };
struct IkField {
  size_t member;                      // offsetof(gmr_job_t, the pointer)
  bool out, per_frame, optional;      // the kernel writes it; [S][T][..], not [S][..]; the caller may pass null
  size_t per_nq, per_nhuman, fixed;   // bytes of one stream (per_frame: of one frame of a stream) = per_nq nq + per_nhuman nhuman + fixed
};
constexpr IkField kIkFields[IK_NFIELD] = {
    {offsetof(gmr_job_t, q0), false, false, false, 8, 0, 0},          // f64 [S][nq]
    {offsetof(gmr_job_t, human), false, true, false, 0, 56, 0},       // f64 [S][T][nhuman][7]
    {offsetof(gmr_job_t, len), false, false, true, 0, 0, 4},          // i32 [S]
    {offsetof(gmr_job_t, scale), false, false, true, 0, 8, 0},        // f64 [S][nhuman]
    {offsetof(gmr_job_t, q_out), true, true, false, 8, 0, 0},         // f64 [S][T][nq]
    {offsetof(gmr_job_t, nsolve), true, true, false, 0, 0, 8},        // i32 [S][T][2]
    {offsetof(gmr_job_t, status), true, false, false, 0, 0, 4},       // i32 [S]
    {offsetof(gmr_job_t, tgt_out), true, true, true, 0, 56, 0},       // f64 [S][T][nhuman][7]
    {offsetof(gmr_job_t, err_out), true, true, true, 0, 0, 16},       // f64 [S][T][2]
};
// the pointer of field f as the job holds it (every object pointer is stored alike)
inline char* ik_ptr(const gmr_job_t& J, int f) { char* p; memcpy(&p, (const char*)&J + kIkFields[f].member, sizeof p); return p; }
inline void ik_set_ptr(gmr_job_t& J, int f, const void* p) { memcpy((char*)&J + kIkFields[f].member, &p, sizeof p); }

// S streams of a job in a workspace: every array it carries on a 256-byte boundary, an absent optional one takes no bytes
struct IkJobOff {
  size_t S, T, end;
  size_t at[IK_NFIELD];
  size_t row[IK_NFIELD];              // bytes of one stream, or of one frame of a stream; 0: the job does not carry the array
  size_t stride(int f) const { return (kIkFields[f].per_frame ? T : 1) * row[f]; }      // from one stream to the next
  size_t out_begin() const { return at[IK_Q_OUT]; }
};
inline IkJobOff ik_carve_job(Carve& c, const gmr_job_t& J, size_t nq, size_t nhuman, size_t S) {
  IkJobOff o;
  o.S = S; o.T = (size_t)J.T;
  for (int f = 0; f < IK_NFIELD; f++) {
    const IkField& d = kIkFields[f];
    o.row[f] = (d.optional && !ik_ptr(J, f)) ? 0 : d.per_nq * nq + d.per_nhuman * nhuman + d.fixed;
    o.at[f] = c.take(S * o.stride(f));
  }
  o.end = c.total();
  return o;
}
// job J with its buffers at those offsets of the device block d (an array the job does not carry stays null)
inline gmr_job_t ik_job_at(const gmr_job_t& J, char* d, const IkJobOff& o) {
  gmr_job_t D = J;
  for (int f = 0; f < IK_NFIELD; f++) ik_set_ptr(D, f, o.row[f] ? d + o.at[f] : nullptr);
  return D;
}

// One copy between the host array of `field` and the device block, in bytes: `rows` pieces of `width`, `pitch` apart on both
// sides (rows == 1: one plain piece).  The table says which way it goes.
struct IkCopy { int field; size_t host, dev, pitch, width, rows; };
enum { IK_PER_STREAM = 1, IK_PER_FRAME = 2, IK_WHOLE = 3 };
// the streams [s0, s0 + o.S) of the inputs (out = false) or outputs the job carries, of the given kinds; returns their number
inline int ik_slice_copies(const IkJobOff& o, bool out, size_t s0, IkCopy* c, int kinds = IK_WHOLE) {
  int n = 0;
  for (int f = 0; f < IK_NFIELD; f++)
    if (kIkFields[f].out == out && o.row[f] && (kinds & (kIkFields[f].per_frame ? IK_PER_FRAME : IK_PER_STREAM)))
      c[n++] = IkCopy{f, s0 * o.stride(f), o.at[f], 0, o.S * o.stride(f), 1};
  return n;
}
// the frames [tb, min(te, T)) of every stream, for the per-frame inputs or outputs the job carries (none when tb >= T)
inline int ik_window_copies(const IkJobOff& o, bool out, size_t tb, size_t te, IkCopy* c) {
  int n = 0;
  if (te > o.T) te = o.T;
  for (int f = 0; f < IK_NFIELD && tb < te; f++)
    if (kIkFields[f].out == out && o.row[f] && kIkFields[f].per_frame)
      c[n++] = IkCopy{f, tb * o.row[f], o.at[f] + tb * o.row[f], o.T * o.row[f], (te - tb) * o.row[f], o.S};
  return n;
}

// ---- how a batch is cut ---------------------------------------------------------------------------------------------------
// slice k of n holds the streams [S k / n, S (k + 1) / n) of every job
inline void ik_slice_range(long long S, int k, int n, int* s0, int* count) {
  *s0 = (int)(S * k / n);
  *count = (int)(S * (k + 1) / n) - *s0;
}
// slices > 0: the caller's choice, at most one per stream; < 0: windows, one slice; 0: about 64 MB of input per slice, at most
// 16, and never fewer than 4096 streams each -- twice the resident width of an MI355X (8 wavefronts x 256 CUs)
inline int ik_slice_count(int slices, long long total, size_t in_bytes) {
  if (slices > 0) return (int)(slices < total ? slices : total);
  if (slices < 0) return 1;
  long long n = (long long)(in_bytes >> 26) < 16 ? (long long)(in_bytes >> 26) : 16;
  if (total / 4096 < n) n = total / 4096;
  return (int)(n > 1 ? n : 1);
}
// frames per window when maxT frames are cut into about W windows: whole queue items (4 frames)
inline int ik_window_frames(int maxT, int W) {
  W = W < maxT / 2 ? W : maxT / 2;
  if (W < 2) W = 2;
  return ((maxT + W - 1) / W + 3) / 4 * 4;
}
// a batch too narrow to be cut by streams but long enough to be cut in time (slices < 0: the caller's choice)
inline bool ik_cut_in_time(int slices, int n, int maxT, size_t in_bytes) {
  return (slices < 0 || (slices == 0 && n == 1 && maxT >= 32 && in_bytes >= ((size_t)64 << 20))) && maxT >= 4;
}
// Up to this many streams a launch uses the 4-wave (main + 3 helpers) shape; measured crossover on MI355X
// (tools/shape_sweep.py, G1): S=256 1.04M vs 0.93M frames/s, S=384 1.24M vs 1.40M (NW=4 vs NW=1): the switch
// sits just above one workgroup per CU (256 CUs)
constexpr long long IK_HELPER_MAX_STREAMS = 300;
// few streams: 4 waves per stream (helpers share the wide assembly phases, shorter per-frame latency); many streams: 1 wave per
// stream (more streams resident, more frames per second), in the throughput kernel when the robot fits it.  `force`: 0, or 1 / 4.
inline bool ik_helpers_shape(bool tree_ok, int force, long long streams) { return tree_ok && (force ? force == 4 : streams <= IK_HELPER_MAX_STREAMS); }
inline bool ik_throughput_shape(bool tree_ok, int force, long long streams, bool wide_ok) { return !ik_helpers_shape(tree_ok, force, streams) && wide_ok; }

}  // namespace gmr
