// gmr_tracker_dev.h -- what the kernels of the motion tracker (gmr_tracker*.hip) share on the device.  One definition each of
//   * the pointer tables of a step, the clip length, the Philox draws (by clip weight, and from the bins of adaptive sampling) and the
//     redraw of a finished clip, so that a link step leaves the same clocks, draws and term bits as a plain step;
//   * the counter domains of the tracker's draws, and the noise of a spec (tracker_words, tracker_noise): sensor noise, kicks and
//     pushes, reset states;
//   * the environment of a lane (tracker_env) and the test of a 16-lane row (tracker_row_skip) of a list of environments;
//   * the reductions over the 16 lanes of an environment (group_sum, group_or, group_count);
//   * the heading frame (yaw_of, unyaw, unyaw_zw, unyaw_q) and the anchors;
//   * three floats, their selection by lane and the reference's two quaternion rotations (V3, pick, rotate_inverse, rotate_forward).
// Device code only; the host's counterpart is gmr_tracker_host.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gmr_fk_walk.h"      // f4
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

// Word 3 of a Philox counter keeps the draws of the blocks apart: the clip and start draws of resets and finished clips, the sensor noise
// (DESIGN.md section 6q), the command resample (6s), the kicks and pushes (6s), the reset states (6t), the sampled actions (6z).
constexpr uint32_t DRAW_RESET = 0u, DRAW_SENSOR = 1u, DRAW_COMMAND = 2u, DRAW_DISTURB = 3u, DRAW_RESET_STATE = 4u, DRAW_ACTION = 5u;

// (float)(T / fps) of clip c; 0 for a clip id outside [0, C)
__device__ __forceinline__ float clip_length(const MotionArrays& A, int c) {
  if (c < 0 || c >= A.C) return 0.0f;
  return (float)((double)(A.seg_start[c + 1] - A.seg_start[c]) / A.fps[c]);
}

// One draw for environment e: counter (e, draws[e], 0, 0), after which draws[e] is one more.  With want_clip, *clip is set
// from word 0; the return value is u of word 1.
__device__ __forceinline__ float tracker_draw(const MotionArrays& A, const TrackerState& S, uint32_t key0, uint32_t key1, int e,
                                              bool want_clip, int* clip) {
  const uint32_t ctr[4] = {(uint32_t)e, S.draws[e], 0u, DRAW_RESET}, key[2] = {key0, key1};
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
  const uint32_t ctr[4] = {(uint32_t)e, S.draws[e], 0u, DRAW_RESET}, key[2] = {key0, key1};
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

// The same test for a kernel that gives entry i of a list a row of 16 lanes (l: the lane inside the row, e = ids ? ids[i] : i): true when
// the row has nothing to do, because the mask leaves the entry out or e lies outside [0, N) -- counted once, by lane 0.  (The id stays
// with the kernel and the result is a flag: the shapes that hand e back through the helper cost the three kernels registers.)
__device__ __forceinline__ bool tracker_row_skip(const TrackerState& S, const int32_t* mask, int i, int l, int e, int N) {
  if (mask && mask[i] == 0) return true;
  if (e >= 0 && e < N) return false;
  if (l == 0) atomicAdd(S.ignored, 1u);
  return true;
}

// the sum over the 16 lanes of an environment, in every one of them; any and the counts go through the same butterfly as integers
__device__ __forceinline__ float group_sum(float x) {
#pragma unroll
  for (int m = 1; m < MOTION_GROUP; m <<= 1) x = x + __shfl_xor(x, m, MOTION_GROUP);
  return x;
}
__device__ __forceinline__ int group_or(int x) {
#pragma unroll
  for (int m = 1; m < MOTION_GROUP; m <<= 1) x |= __shfl_xor(x, m, MOTION_GROUP);
  return x;
}
__device__ __forceinline__ int group_count(int x) {
#pragma unroll
  for (int m = 1; m < MOTION_GROUP; m <<= 1) x += __shfl_xor(x, m, MOTION_GROUP);
  return x;
}

// ---- the noise of a spec (apply_randomization, utils/utils.py:9-25; the statements of record are the mirrors of the three blocks) --------

// the two words of element i of environment e at its count n: philox4x32((e, n, i >> 1, domain), key), words (0, 1) for an even i,
// (2, 3) for an odd one.  Returns the first, *wb is the second.
__device__ __forceinline__ uint32_t tracker_words(uint32_t e, uint32_t n, uint32_t i, uint32_t domain, uint32_t key0, uint32_t key1, uint32_t* wb) {
  const uint32_t ctr[4] = {e, n, i >> 1, domain}, key[2] = {key0, key1};
  uint32_t w[4];
  philox4x32(ctr, key, w);
  *wb = (i & 1u) ? w[3] : w[1];
  return (i & 1u) ? w[2] : w[0];
}

// x with the noise of element i; called for a block with a spec only (S.dist != GMR_NOISE_NONE)
__device__ __forceinline__ float tracker_noise(float x, const ProprioNoise& S, uint32_t e, uint32_t n, uint32_t i, uint32_t domain, uint32_t key0,
                                               uint32_t key1) {
  uint32_t wb;
  const uint32_t wa = tracker_words(e, n, i, domain, key0, key1, &wb);
  float r;
  if (S.dist == GMR_NOISE_GAUSSIAN) {
    const float u1 = philox_unit_open(wa), u2 = philox_unit(wb);
    r = __fsqrt_rn(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
  } else {
    r = philox_unit(wa);
  }
  const float nz = S.a + S.m * r;
  return S.op == GMR_NOISE_SCALING ? x * nz : x + nz;
}

// ---- three floats -----------------------------------------------------------------------------------------------------------------------
struct V3 {
  float x, y, z;
};
__device__ __forceinline__ float pick(const V3& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// quat_rotate_inverse of the reference (torch_utils.py:78-87) in its own grouping; the quaternion as given
__device__ __forceinline__ V3 rotate_inverse(float qx, float qy, float qz, float qw, const V3& v) {
  const float s = 2.0f * (qw * qw) - 1.0f;
  const float d = (qx * v.x + qy * v.y) + qz * v.z;
  V3 r;
  r.x = v.x * s - (qy * v.z - qz * v.y) * qw * 2.0f + qx * d * 2.0f;
  r.y = v.y * s - (qz * v.x - qx * v.z) * qw * 2.0f + qy * d * 2.0f;
  r.z = v.z * s - (qx * v.y - qy * v.x) * qw * 2.0f + qz * d * 2.0f;
  return r;
}
// quat_rotate of the reference (torch_utils.py:66-75) in its own grouping, a + b + c; the quaternion as given
__device__ __forceinline__ V3 rotate_forward(float qx, float qy, float qz, float qw, const V3& v) {
  const float s = 2.0f * (qw * qw) - 1.0f;
  const float d = (qx * v.x + qy * v.y) + qz * v.z;
  V3 r;
  r.x = (v.x * s + (qy * v.z - qz * v.y) * qw * 2.0f) + qx * d * 2.0f;
  r.y = (v.y * s + (qz * v.x - qx * v.z) * qw * 2.0f) + qy * d * 2.0f;
  r.z = (v.z * s + (qx * v.y - qy * v.x) * qw * 2.0f) + qz * d * 2.0f;
  return r;
}

// ---- the heading frame of the links and the preview (DESIGN.md sections 6l, 6m) -----------------------------------------------------------

// the yaw of a rotation as the unit quaternion (0, 0, z, w): normalize(0, 0, q.z, q.w), the identity when both are zero
__device__ __forceinline__ void yaw_of(float qz, float qw, float& z, float& w) {
  const float n2 = qz * qz + qw * qw;
  z = 0.0f; w = 1.0f;
  if (n2 != 0.0f) {                // (a NaN goes through the division and stays one)
    const float n = __fsqrt_rn(n2);
    z = __fdiv_rn(qz, n); w = __fdiv_rn(qw, n);
  }
}

// Rz(-psi) (x, y) with c = cos psi, s = sin psi; for the yaw (z, w): c = w w - z z, s = 2 z w
__device__ __forceinline__ void unyaw(float c, float s, float& x, float& y) {
  const float nx = c * x + s * y, ny = c * y - s * x;
  x = nx; y = ny;
}
__device__ __forceinline__ void unyaw_zw(float z, float w, float& x, float& y) { unyaw(w * w - z * z, 2.0f * z * w, x, y); }
// conj(0, 0, z, w) * q
__device__ __forceinline__ f4 unyaw_q(float z, float w, f4 q) {
  return f4{w * q.x + z * q.y, w * q.y - z * q.x, w * q.z - z * q.w, w * q.w + z * q.z};
}

// ---- tracker anchors (include/gmr_hip.h N8; the statement of record is tests/anchor_mirror.py) ----------------

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
