// gmr_tracker_dev.h -- what the kernels of the motion tracker share on the device: tracker_step_kernel (gmr_tracker.hip),
// tracker_links_kernel (gmr_tracker_links.hip) and the masked reset (gmr_tracker_adaptive.hip).  One definition of the pointer tables,
// the clip length, the Philox draws (by clip weight, and from the bins of adaptive sampling), the redraw of a finished clip and the
// 16-lane sum, so that a link step leaves the same clocks, draws and term bits as a plain step.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gmr_handles.h"
#include "gmr_motion_sample.h"
#include "gmr_philox.h"

// one rounding per operation (the including files say so too; the pragma holds to the end of the translation unit)
#pragma clang fp contract(off)

namespace gmr {

struct TrackerSim {
  const float *base_pos, *base_quat, *base_lin_vel, *base_ang_vel, *dof_pos, *dof_vel;
};
struct TrackerOut {
  float *ref_root_pos, *ref_root_rot, *ref_root_vel, *ref_root_ang_vel, *ref_dof_pos, *ref_dof_vel, *err, *term, *total;
  int32_t *status, *finished;
};

// (float)(T / fps) of clip c; 0 for a clip id outside [0, C)
__device__ __forceinline__ float clip_length(const MotionArrays& A, int c) {
  if (c < 0 || c >= A.C) return 0.0f;
  return (float)((double)(A.seg_start[c + 1] - A.seg_start[c]) / A.fps[c]);
}

// One draw for environment e: counter (e, draws[e], 0, 0), after which draws[e] is one more.  With want_clip, *clip is set
// from word 0; the return value is u of word 1.
__device__ __forceinline__ float tracker_draw(const MotionArrays& A, const TrackerState& S, uint32_t key0, uint32_t key1, int e,
                                              bool want_clip, int* clip) {
  const uint32_t ctr[4] = {(uint32_t)e, S.draws[e], 0u, 0u}, key[2] = {key0, key1};
  uint32_t w[4];
  philox4x32(ctr, key, w);
  S.draws[e] = ctr[1] + 1u;
  if (want_clip) {
    if (S.cdf) {
      // the largest k with cdf[k] <= x (cdf[0] = 0 <= x always)
      const double x = (double)w[0] * 2.3283064365386963e-10;
      int lo = 0, hi = A.C - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (S.cdf[mid] <= x) lo = mid; else hi = mid - 1;
      }
      *clip = lo;
    } else {
      *clip = philox_below(w[0], A.C);
    }
  }
  return philox_unit(w[1]);
}

// One draw for environment e from the bins of adaptive sampling: the counter and key of tracker_draw,
// word 0 picks the bin -- the largest b with cdf[b] <= word0 2^-32 --, word 1 the start inside it.  Returns the start time.
__device__ __forceinline__ float tracker_draw_bin(const MotionArrays& A, const TrackerState& S, uint32_t key0, uint32_t key1, int e, int* clip) {
  const uint32_t ctr[4] = {(uint32_t)e, S.draws[e], 0u, 0u}, key[2] = {key0, key1};
  uint32_t w[4];
  philox4x32(ctr, key, w);
  S.draws[e] = ctr[1] + 1u;
  const AdaptiveBins Bn = *S.bins;
  const double x = (double)w[0] * 2.3283064365386963e-10;
  int lo = 0, hi = Bn.nbins - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (Bn.cdf[mid] <= x) lo = mid; else hi = mid - 1;
  }
  const int c = Bn.clip[lo];
  const long long F = Bn.frames[c], T = A.seg_start[c + 1] - A.seg_start[c];
  const long long f0 = (long long)(lo - Bn.start[c]) * F;
  const long long f1 = f0 + F < T ? f0 + F : T;                     // bin k covers frames [k F, min((k + 1) F, T))
  const double u = (double)philox_unit(w[1]);
  *clip = c;
  return (float)(((double)f0 + u * (double)(f1 - f0)) / A.fps[c]);
}

// What a step does with a finished clip (loop off), for both step kernels: the new clip of environment e and its start time.  A
// plain tracker draws the clip and starts at 0 (:201-213); an adaptive one takes clip and start from the bins, and records nothing.
__device__ __forceinline__ float tracker_redraw(const MotionArrays& A, const TrackerState& S, uint32_t key0, uint32_t key1, int e, int* clip) {
  if (S.bins) return tracker_draw_bin(A, S, key0, key1, e, clip);
  (void)tracker_draw(A, S, key0, key1, e, true, clip);
  return 0.0f;
}

// the environment of lane i of a reset / assign: ids[i], or i itself without a list; -1 (and counted) outside [0, N)
__device__ __forceinline__ int tracker_env(const TrackerState& S, const int32_t* __restrict__ ids, int i, int N) {
  const int e = ids ? ids[i] : i;
  if (e >= 0 && e < N) return e;
  atomicAdd(S.ignored, 1u);
  return -1;
}

// the sum over the 16 lanes of an environment, in every one of them
__device__ __forceinline__ float group_sum(float x) {
#pragma unroll
  for (int m = 1; m < MOTION_GROUP; m <<= 1) x = x + __shfl_xor(x, m, MOTION_GROUP);
  return x;
}

// ---- tracker anchors (include/gmr_hip.h N8; the statement of record is tests/anchor_mirror.py) ----------------

// the yaw of a rotation as the unit quaternion (0, 0, z, w): normalize(0, 0, q.z, q.w), the identity when both are zero
__device__ __forceinline__ void yaw_of(float qz, float qw, float& z, float& w) {
  const float n2 = qz * qz + qw * qw;
  z = 0.0f; w = 1.0f;
  if (n2 != 0.0f) {                // (a NaN goes through the division and stays one)
    const float n = __fsqrt_rn(n2);
    z = __fdiv_rn(qz, n); w = __fdiv_rn(qw, n);
  }
}

// yaw_of with a correctly rounded square root (sqrtf; __fsqrt_rn above is the hardware's, good to one ulp): what anchor_to_root
// uses, so that tests/anchor_mirror.py reproduces the anchor's bits in NumPy.  The heading frame keeps yaw_of and with it its bits.
__device__ __forceinline__ void yaw_of_exact(float qz, float qw, float& z, float& w) {
  const float n2 = qz * qz + qw * qw;
  z = 0.0f; w = 1.0f;
  if (n2 != 0.0f) {
    const float n = sqrtf(n2);
    z = qz / n; w = qw / n;
  }
}

// The anchor of one environment: yaw (z, w) with c = w w - z z, s = 2 z w, then the translation.  tx, ty, tz are filled by
// anchor_load (lane = environment); a lane that holds ONE component of a row keeps its own translation component beside it.
struct Anchor {
  float z, w, c, s, tx, ty, tz;
};
__device__ __forceinline__ void anchor_turn(const TrackerState& S, size_t e, Anchor& a) {
  a.z = S.anchor_yaw[e * 2]; a.w = S.anchor_yaw[e * 2 + 1];
  a.c = a.w * a.w - a.z * a.z; a.s = 2.0f * a.z * a.w;
}
__device__ __forceinline__ Anchor anchor_load(const TrackerState& S, size_t e) {
  Anchor a;
  anchor_turn(S, e, a);
  a.tx = S.anchor_pos[e * 3]; a.ty = S.anchor_pos[e * 3 + 1]; a.tz = S.anchor_pos[e * 3 + 2];
  return a;
}
// lane = environment: a vector (x and y turn, z stays), a position (the vector, then the translation), a quaternion xyzw
__device__ __forceinline__ void anchor_vector(const Anchor& a, float& x, float& y) {
  const float nx = a.c * x - a.s * y, ny = a.s * x + a.c * y;
  x = nx; y = ny;
}
__device__ __forceinline__ void anchor_point(const Anchor& a, float& x, float& y, float& z) {
  anchor_vector(a, x, y);
  x = x + a.tx; y = y + a.ty; z = z + a.tz;
}
__device__ __forceinline__ void anchor_quat(const Anchor& a, float& qx, float& qy, float& qz, float& qw) {
  const float nx = a.w * qx - a.z * qy, ny = a.w * qy + a.z * qx, nz = a.w * qz + a.z * qw, nw = a.w * qw - a.z * qz;
  qx = nx; qy = ny; qz = nz; qw = nw;
}
// lane = component: lane l of a 16-lane row holds component l (x, y, z; w of a quaternion in lane 3).  Lanes 0 and 1 (2 and 3) swap
// inside the row; the lanes of a row are all here or all gone.  Lanes that hold no component return something nobody reads.
__device__ __forceinline__ float anchor_vector_lane(const Anchor& a, int l, float v) {
  const float o = __shfl(v, l ^ 1, MOTION_GROUP);
  return l == 0 ? a.c * v - a.s * o : (l == 1 ? a.s * o + a.c * v : v);
}
__device__ __forceinline__ float anchor_point_lane(const Anchor& a, int l, float v, float t) { return anchor_vector_lane(a, l, v) + t; }
__device__ __forceinline__ float anchor_quat_lane(const Anchor& a, int l, float q) {
  const float o = __shfl(q, l ^ 1, MOTION_GROUP);
  return (l == 0 || l == 3) ? a.w * q - a.z * o : a.w * q + a.z * o;
}

}  // namespace gmr
