// gmr_motion_sample.h -- what one (clip, time) query of the motion library computes, shared by the kernels that answer
// queries: motion_sample_kernel (gmr_motion.hip) and body_state_kernel (gmr_body_state.hip).  One definition of the frame
// pair, the blend weights, the lerp and the float32 slerp, so that both kernels give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gmr_handles.h"      // MotionArrays

// float32 arithmetic here mirrors NumPy's / torch's (one rounding per operation: a multiply and an add stay two; the including
// files say so too, and the pragma holds to the end of the translation unit)
#pragma clang fp contract(off)

namespace gmr {

constexpr int MOTION_GROUP = 16;     // lanes per query that stride over the columns of the two source rows

// The scalars of a query: whether it is answered at all, the two source rows and the blend weights.
struct MotionQuery {
  bool ok, same;        // !ok: a clip id outside [0, C), an empty clip or a non-finite time -- nothing of the library is read
  size_t rl, rh;        // rows of the library: frame lo and frame hi = min(lo + 1, T - 1); same = (lo == hi)
  float w0, w1;         // (float)(1 - blend), (float)blend
};

__device__ __forceinline__ MotionQuery motion_query(const MotionArrays& A, int c, double tm, int loop) {
  MotionQuery Q;
  int T = 0, first = 0;
  const bool clip_ok = c >= 0 && c < A.C;
  if (clip_ok) { first = A.seg_start[c]; T = A.seg_start[c + 1] - first; }
  Q.ok = clip_ok && T >= 1 && isfinite(tm);
  Q.same = true; Q.rl = Q.rh = 0; Q.w0 = 1.0f; Q.w1 = 0.0f;
  if (!Q.ok) return Q;
  // :165-175 in float64
  const double fps = A.fps[c];
  const double dt = 1.0 / fps, duration = (double)T / fps;
  double t;
  if (loop) {
    t = fmod(tm, duration);             // Python's %: the sign of the divisor
    if (t < 0.0) t += duration;
  } else {
    t = fmin(tm, duration - dt);
  }
  const double x = t * fps, fl = floor(x);
  int lo;
  double blend;
  // where the reference would index out of range (a negative time without loop; t * fps rounding up to T): the nearest frame
  if (!(fl >= 0.0)) { lo = 0; blend = 0.0; }
  else if (fl > (double)(T - 1)) { lo = T - 1; blend = 0.0; }
  else { lo = (int)fl; blend = x - fl; }
  const int hi = min(lo + 1, T - 1);
  Q.same = lo == hi;
  Q.rl = (size_t)(first + lo); Q.rh = (size_t)(first + hi);
  Q.w0 = (float)(1.0 - blend); Q.w1 = (float)blend;
  return Q;
}

// a[lo] (same) or (float)(1 - blend) a[lo] + (float)blend a[hi] as a separate multiply and add (:196-200)
__device__ __forceinline__ float lerp1(const float* __restrict__ a, size_t lo, size_t hi, bool same, float w0, float w1) {
  const float x = a[lo];
  return same ? x : w0 * x + w1 * a[hi];
}

// component l (xyzw) of the root quaternion between rows rl and rh of root_rot
__device__ __forceinline__ float slerp1(const float* __restrict__ root_rot, size_t rl, size_t rh, int l, bool same, float w0, float w1) {
  const float* q1 = root_rot + rl * 4;      // xyzw
  float r;
  if (same) {
    r = q1[l];
  } else {
    // :205-233 in float32; the component order of the dot is wxyz, as the reference sums it
    const float* q2 = root_rot + rh * 4;
    float dot = q1[3] * q2[3];
    dot = dot + q1[0] * q2[0];
    dot = dot + q1[1] * q2[1];
    dot = dot + q1[2] * q2[2];
    const float sgn = dot < 0.0f ? -1.0f : 1.0f;
    dot = fminf(fmaxf(sgn * dot, -1.0f), 1.0f);
    const float a = q1[l], b = sgn * q2[l];
    if (dot > 0.9995f) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = w0 * q1[k] + w1 * (sgn * q2[k]);
      float n2 = v[3] * v[3];
      n2 = n2 + v[0] * v[0];
      n2 = n2 + v[1] * v[1];
      n2 = n2 + v[2] * v[2];
      r = __fdiv_rn(w0 * a + w1 * b, __fsqrt_rn(n2));
    } else {
      const float th0 = acosf(dot), sn0 = sinf(th0);
      const float th = th0 * w1, sn = sinf(th);
      const float s0 = cosf(th) - __fdiv_rn(dot * sn, sn0), s1 = __fdiv_rn(sn, sn0);
      r = s0 * a + s1 * b;
    }
  }
  return r;
}

}  // namespace gmr
