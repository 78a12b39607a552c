// gmr_tracker_anchor.hip -- the anchors of the motion tracker: per environment a rigid move about the vertical,
// yaw then translation, that every world-frame quantity of the tracker goes through, so that N environments spread over a grid of
// origins, each facing wherever its robot faces, track one library.  The step kernels apply it (gmr_tracker.hip,
// gmr_tracker_links.hip, gmr_tracker_preview.hip through the helpers of gmr_tracker_dev.h); this file owns the two arrays and sets them.
//
//   tracker_anchor_set_kernel    one lane per listed environment: the translation and / or the yaw, given as an angle or as (z, w)
//   tracker_anchor_root_kernel   ONE launch, one lane per environment (or per list entry): a lane whose mask is not set leaves; the
//                                others sample the reference root at their own (clip, clock) with the sampler's lines and choose the
//                                anchor that carries it onto the root they are given -- yaw and x / y, optionally z
//
// The kernels write the tracker's anchors (and its count of ignored ids) and nothing else; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_motion_sample.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/anchor_mirror.py states every line in float32 NumPy, and the host states anchor_half_angle
#pragma clang fp contract(off)

namespace gmr {

// (sin, cos) of psi / 2 in float32, the same bits on the host and on the device: only +, -, * and floor, so neither side's libm
// enters.  h = psi / 2 is reduced in float64 by k = floor(h 2/pi + 1/2) quarter turns to r in [-pi/4, pi/4]; the two polynomials in
// r r are the classic single-precision ones (Cephes sinf / cosf), about one ulp; the quadrant k mod 4 picks and signs them.
__host__ __device__ inline void anchor_half_angle(float psi, float* z, float* w) {
  const float h = psi * 0.5f;
  const double kd = floor((double)h * 0.63661977236758134308 + 0.5);
  const float r = (float)((double)h - kd * 1.57079632679489661923);
  const int quad = (int)(kd - 4.0 * floor(kd * 0.25));      // 0 .. 3 while kd is an integer that float64 holds
  const float r2 = r * r;
  const float sn = ((-1.9515295891e-4f * r2 + 8.3321608736e-3f) * r2 - 1.6666654611e-1f) * r2 * r + r;
  const float cs = ((2.443315711809948e-5f * r2 - 1.388731625493765e-3f) * r2 + 4.166664568298827e-2f) * r2 * r2 - 0.5f * r2 + 1.0f;
  switch (quad) {
    case 0: *z = sn; *w = cs; break;
    case 1: *z = cs; *w = -sn; break;
    case 2: *z = -sn; *w = -cs; break;
    default: *z = -cs; *w = sn; break;
  }
}

// Entry i of the list (environment i without one): pos[i][3] and / or yaw.  yaw_is_zw: yaw[i][2] is (z, w) as it stands (the
// synchronous twin converts on the host); else yaw[i] is an angle in radians.
__global__ __launch_bounds__(256) void tracker_anchor_set_kernel(const TrackerState S, int N, int n, const int32_t* __restrict__ ids,
                                                                 const float* __restrict__ pos, const float* __restrict__ yaw, int yaw_is_zw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int e = tracker_env(S, ids, i, N);
  if (e < 0) return;
  if (pos) {
    S.anchor_pos[(size_t)e * 3] = pos[(size_t)i * 3];
    S.anchor_pos[(size_t)e * 3 + 1] = pos[(size_t)i * 3 + 1];
    S.anchor_pos[(size_t)e * 3 + 2] = pos[(size_t)i * 3 + 2];
  }
  if (yaw) {
    float z, w;
    if (yaw_is_zw) { z = yaw[(size_t)i * 2]; w = yaw[(size_t)i * 2 + 1]; }
    else anchor_half_angle(yaw[i], &z, &w);
    S.anchor_yaw[(size_t)e * 2] = z;
    S.anchor_yaw[(size_t)e * 2 + 1] = w;
  }
}

// Entry i: mask[i], root_pos[i][3], root_quat[i][4] xyzw.  The reference root is the sampler's at (clip, (double)time); a bad
// assignment or a root that is not finite leaves the anchor as it was.
__global__ __launch_bounds__(256) void tracker_anchor_root_kernel(const MotionArrays A, const TrackerState S, int N, int n,
                                                                  const int32_t* __restrict__ ids, const int32_t* __restrict__ mask,
                                                                  const float* __restrict__ root_pos, const float* __restrict__ root_quat,
                                                                  int loop, int flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (mask && mask[i] == 0) return;
  const int e = tracker_env(S, ids, i, N);
  if (e < 0) return;
  const int c = S.clip[e];
  const MotionQuery Q = motion_query(A, c, (double)S.time[e], loop);
  if (!Q.ok) return;
  const float sx = root_pos[(size_t)i * 3], sy = root_pos[(size_t)i * 3 + 1], sz = root_pos[(size_t)i * 3 + 2];
  const float* sq = root_quat + (size_t)i * 4;
  if (!(isfinite(sx) && isfinite(sy) && isfinite(sz) && isfinite(sq[0]) && isfinite(sq[1]) && isfinite(sq[2]) && isfinite(sq[3]))) return;
  const float rx = lerp1(A.root_pos, Q.rl * 3, Q.rh * 3, Q.same, Q.w0, Q.w1);
  const float ry = lerp1(A.root_pos, Q.rl * 3 + 1, Q.rh * 3 + 1, Q.same, Q.w0, Q.w1);
  const float rz = lerp1(A.root_pos, Q.rl * 3 + 2, Q.rh * 3 + 2, Q.same, Q.w0, Q.w1);
  Anchor a;
  a.z = S.anchor_yaw[(size_t)e * 2]; a.w = S.anchor_yaw[(size_t)e * 2 + 1];
  if (flags & GMR_ANCHOR_YAW) {
    float zr, wr, zs, ws;
    yaw_of_exact(slerp1(A.root_rot, Q.rl, Q.rh, 2, Q.same, Q.w0, Q.w1), slerp1(A.root_rot, Q.rl, Q.rh, 3, Q.same, Q.w0, Q.w1), zr, wr);
    yaw_of_exact(sq[2], sq[3], zs, ws);
    yaw_of_exact(zs * wr - ws * zr, ws * wr + zs * zr, a.z, a.w);      // yaw(sim) * conj(yaw(reference)), a unit quaternion again
    S.anchor_yaw[(size_t)e * 2] = a.z;
    S.anchor_yaw[(size_t)e * 2 + 1] = a.w;
  }
  a.c = a.w * a.w - a.z * a.z; a.s = 2.0f * a.z * a.w;
  S.anchor_pos[(size_t)e * 3] = sx - (a.c * rx - a.s * ry);
  S.anchor_pos[(size_t)e * 3 + 1] = sy - (a.s * rx + a.c * ry);
  if (flags & GMR_ANCHOR_Z) S.anchor_pos[(size_t)e * 3 + 2] = sz - rz;
}

// the two arrays, filled with the identity (the caller holds the mutex); nothing happens when they are there already
static int anchors_on(gmr_motion_tracker* t) {
  if (t->S.anchor_pos) return GMR_OK;
  const size_t n = (size_t)t->N;
  Carve cv;
  const size_t o_pos = cv.take(n * 12), o_yaw = cv.take(n * 8);
  GMR_HIP_TRY(hipDeviceSynchronize());
  GMR_HIP_TRY(t->anchor_block.reserve(cv.total() + 256));
  char* d = t->anchor_block.data();
  std::vector<float> yaw(n * 2);
  for (size_t e = 0; e < n; e++) { yaw[e * 2] = 0.0f; yaw[e * 2 + 1] = 1.0f; }
  GMR_HIP_TRY(hipMemset(d + o_pos, 0, n * 12));
  GMR_HIP_TRY(hipMemcpy(d + o_yaw, yaw.data(), n * 8, hipMemcpyHostToDevice));
  GMR_HIP_TRY(hipDeviceSynchronize());
  t->S.anchor_pos = (float*)(d + o_pos);
  t->S.anchor_yaw = (float*)(d + o_yaw);
  return GMR_OK;
}

static int anchor_yaw_allowed(const gmr_motion_tracker* t) {
  if (t->lib->reference_angvel)
    return gmr_fail(GMR_ERR_ARG, "a yaw anchor needs a library filled with GMR_MOTION_ANGVEL_WORLD: the root_ang_vel of "
                                 "GMR_MOTION_ANGVEL_REFERENCE is not a physical angular velocity and cannot be rotated");
  return GMR_OK;
}

// every check of a set_anchor that its two entry points share, and the launch
static int anchor_set_launch(gmr_motion_tracker* t, const TrackerState& S, int n, const int32_t* d_ids, const float* d_pos, const float* d_yaw,
                             int yaw_is_zw, hipStream_t stream) {
  if (!S.anchor_pos) return gmr_fail(GMR_ERR_ARG, "anchors are not enabled on this tracker (gmr_motion_tracker_enable_anchors)");
  int rc = subset_check(t->N, n, d_ids, "every environment is set");
  if (rc == GMR_OK && d_yaw) rc = anchor_yaw_allowed(t);
  if (rc != GMR_OK) return rc;
  if (n == 0 || (!d_pos && !d_yaw)) return GMR_OK;
  hipLaunchKernelGGL(tracker_anchor_set_kernel, dim3(lane_blocks(n)), dim3(256), 0, stream, S, t->N, n, d_ids, d_pos, d_yaw, yaw_is_zw);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

static int anchor_root_launch(gmr_motion_tracker* t, const TrackerState& S, int n, const int32_t* d_ids, const int32_t* d_mask,
                              const float* d_root_pos, const float* d_root_quat, int flags, hipStream_t stream) {
  if (!S.anchor_pos) return gmr_fail(GMR_ERR_ARG, "anchors are not enabled on this tracker (gmr_motion_tracker_enable_anchors)");
  if (flags & ~(GMR_ANCHOR_YAW | GMR_ANCHOR_Z)) return gmr_fail(GMR_ERR_ARG, "unknown anchor flag bits 0x%x", flags);
  int rc = subset_check(t->N, n, d_ids, "the mask and the roots cover every environment");
  if (rc == GMR_OK && (flags & GMR_ANCHOR_YAW)) rc = anchor_yaw_allowed(t);
  if (rc != GMR_OK) return rc;
  if (n == 0) return GMR_OK;
  if (!d_root_pos || !d_root_quat) return gmr_fail(GMR_ERR_ARG, "null root_pos / root_quat");
  hipLaunchKernelGGL(tracker_anchor_root_kernel, dim3(lane_blocks(n)), dim3(256), 0, stream, t->lib->A, S, t->N, n, d_ids, d_mask, d_root_pos, d_root_quat,
                     t->loop, flags);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker anchors") ---------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_enable_anchors(gmr_motion_tracker_t* t, int on) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  if (on) return gmr::anchors_on(t);
  if (!t->S.anchor_pos) return GMR_OK;
  GMR_HIP_TRY(hipDeviceSynchronize());
  t->S.anchor_pos = nullptr;
  t->S.anchor_yaw = nullptr;
  GMR_HIP_TRY(t->anchor_block.release());
  return GMR_OK;
}

int gmr_motion_tracker_set_anchor_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const float* d_pos, const float* d_yaw,
                                      void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::TrackerState S;
  {
    std::lock_guard<std::mutex> g(t->mu);
    S = t->S;
  }
  return gmr::anchor_set_launch(t, S, n, d_env_ids, d_pos, d_yaw, 0, (hipStream_t)stream);
}

int gmr_motion_tracker_set_anchor(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const float* pos, const float* yaw, int* ignored) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (ignored) *ignored = 0;
  int rc = gmr::subset_check(t->N, n, env_ids, "every environment is set");
  if (rc != GMR_OK) return rc;
  for (size_t i = 0; i < (size_t)n; i++) {
    if (pos && !(std::isfinite(pos[i * 3]) && std::isfinite(pos[i * 3 + 1]) && std::isfinite(pos[i * 3 + 2])))
      return gmr_fail(GMR_ERR_ARG, "pos[%zu] is not finite", i);
    if (yaw && !std::isfinite(yaw[i])) return gmr_fail(GMR_ERR_ARG, "yaw[%zu] is not finite", i);
  }
  if (yaw && (rc = gmr::anchor_yaw_allowed(t)) != GMR_OK) return rc;
  std::lock_guard<std::mutex> g(t->mu);
  if ((rc = gmr::anchors_on(t)) != GMR_OK) return rc;
  if (n == 0 || (!pos && !yaw)) return GMR_OK;
  std::vector<float> zw;
  if (yaw) {
    zw.resize((size_t)n * 2);
    for (size_t i = 0; i < (size_t)n; i++) gmr::anchor_half_angle(yaw[i], &zw[i * 2], &zw[i * 2 + 1]);
  }
  const size_t nn = (size_t)n;
  gmr::HostStage st;
  const int32_t* d_ids;
  const float *d_pos, *d_yaw;
  st.in(d_ids, env_ids, nn * 4); st.in(d_pos, pos, nn * 12); st.in(d_yaw, yaw ? zw.data() : nullptr, nn * 8);
  GMR_STAGE_TRY(st, upload);
  gmr::IgnoredDelta ig(t->S.ignored, ignored);
  if ((rc = ig.begin()) != GMR_OK) return rc;
  rc = gmr::anchor_set_launch(t, t->S, n, d_ids, d_pos, d_yaw, 1, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return ig.end();
}

int gmr_motion_tracker_anchor_to_root_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_mask,
                                          const float* d_root_pos, const float* d_root_quat, int flags, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::TrackerState S;
  {
    std::lock_guard<std::mutex> g(t->mu);
    S = t->S;
  }
  return gmr::anchor_root_launch(t, S, n, d_env_ids, d_mask, d_root_pos, d_root_quat, flags, (hipStream_t)stream);
}

int gmr_motion_tracker_anchor_to_root(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* mask, const float* root_pos,
                                      const float* root_quat, int flags, int* ignored) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (ignored) *ignored = 0;
  if (flags & ~(GMR_ANCHOR_YAW | GMR_ANCHOR_Z)) return gmr_fail(GMR_ERR_ARG, "unknown anchor flag bits 0x%x", flags);
  int rc = gmr::subset_check(t->N, n, env_ids, "the mask and the roots cover every environment");
  if (rc != GMR_OK) return rc;
  if (n > 0 && (!root_pos || !root_quat)) return gmr_fail(GMR_ERR_ARG, "null root_pos / root_quat");
  if ((flags & GMR_ANCHOR_YAW) && (rc = gmr::anchor_yaw_allowed(t)) != GMR_OK) return rc;
  std::lock_guard<std::mutex> g(t->mu);
  if ((rc = gmr::anchors_on(t)) != GMR_OK) return rc;
  if (n == 0) return GMR_OK;
  const size_t nn = (size_t)n;
  gmr::HostStage st;
  const int32_t *d_ids, *d_mask;
  const float *d_pos, *d_quat;
  st.in(d_ids, env_ids, nn * 4); st.in(d_mask, mask, nn * 4); st.in(d_pos, root_pos, nn * 12); st.in(d_quat, root_quat, nn * 16);
  GMR_STAGE_TRY(st, upload);
  gmr::IgnoredDelta ig(t->S.ignored, ignored);
  if ((rc = ig.begin()) != GMR_OK) return rc;
  rc = gmr::anchor_root_launch(t, t->S, n, d_ids, d_mask, d_pos, d_quat, flags, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return ig.end();
}

int gmr_motion_tracker_anchor_state(gmr_motion_tracker_t* t, float* pos, float* yaw_zw) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  if (!t->S.anchor_pos) return gmr_fail(GMR_ERR_ARG, "anchors are not enabled on this tracker (gmr_motion_tracker_enable_anchors)");
  const size_t n = (size_t)t->N;
  return gmr::read_back({{pos, t->S.anchor_pos, n * 12}, {yaw_zw, t->S.anchor_yaw, n * 8}});
}

}  // extern "C"
