// gmr_fk_walk.h -- the per-body step of the float32 forward kinematics (reference kinematics_model.py:213-246), shared by the
// kernels that walk the tree lane = frame: fk_batch_kernel / fk_split_kernel (gmr_fk.hip) and body_state_kernel
// (gmr_body_state.hip).  One definition, so that every walk rounds alike: tools/fk_bitcheck.py and the bit-equality tests of
// tests/test_motion_body_state.py compare their outputs bit for bit.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gmr_fk_tree.h"

// float32 arithmetic here mirrors torch eager ops (one rounding per operation): no FMA contraction (the including files
// say so too; the pragma holds to the end of the translation unit)
#pragma clang fp contract(off)

namespace gmr {

struct f4 { float x, y, z, w; };

__device__ __forceinline__ f4 qmul_xyzw(f4 a, f4 b) {
  f4 r;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
  r.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  return r;
}

// torch_utils.quat_rotate (reference torch_utils.py:65-75), same operation order
__device__ __forceinline__ void qrot_xyzw(f4 q, float vx, float vy, float vz, float& ox, float& oy, float& oz) {
  float s = 2.0f * q.w * q.w - 1.0f;
  float cx = q.y * vz - q.z * vy, cy = q.z * vx - q.x * vz, cz = q.x * vy - q.y * vx;
  float d = q.x * vx + q.y * vy + q.z * vz;
  ox = vx * s + cx * q.w * 2.0f + q.x * d * 2.0f;
  oy = vy * s + cy * q.w * 2.0f + q.y * d * 2.0f;
  oz = vz * s + cz * q.w * 2.0f + q.z * d * 2.0f;
}

// sin and cos of a joint half angle (|x| of a few radians): Cody-Waite reduction by pi/2 in three pieces, the Cephes
// single-precision kernels on [-pi/4, pi/4] (~1 ulp).  28 instructions instead of the 125 of the library call (which
// carries a large-argument path); explicit fmaf, so `fp contract(off)` does not change it.  The three-piece reduction is
// exact only while k * 1.5703125 is (|k| < 2^13): beyond |x| = 1000 rad -- forward_kinematics accepts any user angle,
// torch.sin / torch.cos are accurate for all of them -- and for NaN / Inf (where `(int)k` would be undefined) the
// library call is taken: a wave-rare branch.
__device__ __forceinline__ void sincosf_small(float x, float* sn, float* cs) {
  if (!(fabsf(x) <= 1000.0f)) { sincosf(x, sn, cs); return; }
  const float k = rintf(x * 0.636619772367581343f);
  float r = fmaf(-k, 1.5703125f, x);
  r = fmaf(-k, 4.837512969970703125e-4f, r);
  r = fmaf(-k, 7.54978995489188216e-8f, r);
  const float z = r * r;
  const float ps = fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f);
  const float pc = fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f);
  const float s = fmaf(r * z, ps, r);
  const float c = fmaf(z * z, pc, fmaf(-0.5f, z, 1.0f));
  const int q = (int)k;
  const float ss = (q & 1) ? c : s, cc = (q & 1) ? s : c;
  *sn = (q & 2) ? -ss : ss;
  *cs = ((q + 1) & 2) ? -cc : cc;
}

// quat_rotate for a vector with known exact zeros (ZM bit k: component k is exactly 0): the terms of qrot_xyzw that survive,
// in its order -- a local translation is wave-uniform and most have one or two zero components (G1: 31 of 38 bodies)
template <bool ZA, bool ZB> __device__ __forceinline__ float diff_z(float a, float b) {
  if (ZA && ZB) return 0.0f;
  if (ZA) return -b;
  if (ZB) return a;
  return a - b;
}
template <bool ZA, bool ZB, bool ZC> __device__ __forceinline__ float sum3_z(float a, float b, float c) {
  if (ZA && ZB) return c;          // (callers never pass three zeros)
  if (ZA && ZC) return b;
  if (ZB && ZC) return a;
  if (ZA) return b + c;
  if (ZB) return a + c;
  if (ZC) return a + b;
  return a + b + c;
}
template <int ZM>
__device__ __forceinline__ void qrot_sparse(f4 q, float vx, float vy, float vz, float& ox, float& oy, float& oz) {
  constexpr bool zx = ZM & 1, zy = (ZM >> 1) & 1, zz = (ZM >> 2) & 1;
  if (zx && zy && zz) { ox = 0.0f; oy = 0.0f; oz = 0.0f; return; }
  const float s = 2.0f * q.w * q.w - 1.0f;
  const float cx = diff_z<zz, zy>(q.y * vz, q.z * vy), cy = diff_z<zx, zz>(q.z * vx, q.x * vz), cz = diff_z<zy, zx>(q.x * vy, q.y * vx);
  const float d = sum3_z<zx, zy, zz>(q.x * vx, q.y * vy, q.z * vz);
  ox = sum3_z<zx, zy && zz, false>(vx * s, cx * q.w * 2.0f, q.x * d * 2.0f);
  oy = sum3_z<zy, zz && zx, false>(vy * s, cy * q.w * 2.0f, q.y * d * 2.0f);
  oz = sum3_z<zz, zx && zy, false>(vz * s, cz * q.w * 2.0f, q.z * d * 2.0f);
}

// a * b for b = (.., b_k, .., b_w) with the two other components exactly zero (K = 0, 1, 2: x, y, z): the terms of
// qmul_xyzw that survive, in its order -- the dropped ones are products with an exact zero, added to or subtracted from the
// running sum without changing it (only the sign of a zero RESULT can differ, and non-finite operands: 0 * inf)
template <int K>
__device__ __forceinline__ f4 qmul_axis(f4 a, float bk, float bw) {
  f4 r;
  if (K == 0) {
    r.x = a.w * bk + a.x * bw; r.y = a.y * bw + a.z * bk; r.z = a.z * bw - a.y * bk; r.w = a.w * bw - a.x * bk;
  } else if (K == 1) {
    r.x = a.x * bw - a.z * bk; r.y = a.w * bk + a.y * bw; r.z = a.x * bk + a.z * bw; r.w = a.w * bw - a.y * bk;
  } else {
    r.x = a.x * bw + a.y * bk; r.y = a.y * bw - a.x * bk; r.z = a.w * bk + a.z * bw; r.w = a.w * bw - a.z * bk;
  }
  return r;
}

// The same for a whole wavefront: when every lane's argument lies in [-0.785, 0.785] -- joint half angles of a humanoid in
// motion almost always do: |angle| <= 90 degrees -- the reduction (k = 0, r = x exactly) and the quadrant selects fall away:
// the same two polynomials on the same r, bit-identical, 14 instead of 30 instructions per hinge body.  One ballot decides.
__device__ __forceinline__ void sincosf_wave(float x, float* sn, float* cs) {
  if (__builtin_amdgcn_ballot_w64(!(fabsf(x) <= 0.785f)) != 0ull) { sincosf_small(x, sn, cs); return; }
  const float z = x * x;
  const float ps = fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f);
  const float pc = fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f);
  *sn = fmaf(x * z, ps, x);
  *cs = fmaf(z * z, pc, fmaf(-0.5f, z, 1.0f));
}

// One body of the walk: world rotation `rot` = prot * (r_j * joint(ang)) and the world offset of its origin
// R(prot) t_j (reference kinematics_model.py:213-246).  Everything in `cur` is wave-uniform (SGPRs), so the record's flags
// select code, not lanes: a local rotation that is exactly (0, 0, 0, 1) (meta bit 1: r_j * x = x) and a hinge axis that is
// exactly +-e_k (meta bits [3:2] = k + 1: the joint quaternion has two exact zeros) skip the products whose factor is an
// exact 0 or 1.  Every shipped robot's hinges are axis-aligned and three quarters of the bodies carry no local rotation:
// 186 -> ~115 vector instructions for such a body, in a walk that is bound by instruction issue.
__device__ __forceinline__ void fk_body(const FkBodyRec& cur, float ang, f4 prot, float& wx, float& wy, float& wz, f4& rot) {
  const f4 lr = {cur.r[0], cur.r[1], cur.r[2], cur.r[3]};
  const bool unit_lr = cur.meta & 2u;
  const unsigned kind = (cur.meta >> 2) & 3u;
  switch ((cur.next_park >> 16) & 7u) {     // which components of t_j are exactly zero (record flags, wave-uniform)
    case 1: qrot_sparse<1>(prot, cur.t[0], cur.t[1], cur.t[2], wx, wy, wz); break;
    case 2: qrot_sparse<2>(prot, cur.t[0], cur.t[1], cur.t[2], wx, wy, wz); break;
    case 3: qrot_sparse<3>(prot, cur.t[0], cur.t[1], cur.t[2], wx, wy, wz); break;
    case 4: qrot_sparse<4>(prot, cur.t[0], cur.t[1], cur.t[2], wx, wy, wz); break;
    case 5: qrot_sparse<5>(prot, cur.t[0], cur.t[1], cur.t[2], wx, wy, wz); break;
    case 6: qrot_sparse<6>(prot, cur.t[0], cur.t[1], cur.t[2], wx, wy, wz); break;
    case 7: qrot_sparse<7>(prot, cur.t[0], cur.t[1], cur.t[2], wx, wy, wz); break;
    default: qrot_xyzw(prot, cur.t[0], cur.t[1], cur.t[2], wx, wy, wz); break;
  }
  if (cur.meta & 1u) {
    // dof_to_rot: sin/cos of the float32 half angle; products and the normalisation in float64;
    // rounded to float32 on assignment (kinematics_model.py:21-36, torch_utils.py:353-359).
    // the record's axis is normalize(axis) (float64, computed once on the host).
    float th = ang / 2.0f;
    float sf, cf;
#ifdef GMR_FK_LIBM_SINCOS
    sincosf(th, &sf, &cf);
#else
    sincosf_wave(th, &sf, &cf);
#endif
    double s = (double)sf, c = (double)cf;
    if (kind) {
      const double qk = cur.axis[0] * s, qw = c;      // (the record of such a hinge carries its +-1.0 in axis[0])
      const double e = fma(qk, qk, fma(qw, qw, -1.0));
      const double rn = fma(e, fma(e, 0.375, -0.5), 1.0);
      const float jk = (float)(qk * rn), jw = (float)(qw * rn);
      if (unit_lr) {
        rot = kind == 1 ? qmul_axis<0>(prot, jk, jw) : (kind == 2 ? qmul_axis<1>(prot, jk, jw) : qmul_axis<2>(prot, jk, jw));
      } else {
        const f4 cr = kind == 1 ? qmul_axis<0>(lr, jk, jw) : (kind == 2 ? qmul_axis<1>(lr, jk, jw) : qmul_axis<2>(lr, jk, jw));
        rot = qmul_xyzw(prot, cr);
      }
      return;
    }
    double qx = cur.axis[0] * s, qy = cur.axis[1] * s, qz = cur.axis[2] * s, qw = c;
    // quat_unit in float64: x / |q|.  |q|^2 = 1 + e with |e| ~ 1e-7 (float32 sin / cos of one angle, a unit axis), so
    // 1 / |q| = 1 - e/2 + 3 e^2 / 8 to 1e-21: the quotient differs from x / sqrt(|q|^2) by < 1 ulp of float64 and
    // rounds to the same float32 (measured bit-equal with the rsqrt form on 2^20 random frames, tools/fk_bitcheck.py)
#ifdef GMR_FK_RSQRT_NORM
    double rn = rsqrt(fmax(qx * qx + qy * qy + qz * qz + qw * qw, 1e-18));
#else
    const double e = fma(qx, qx, fma(qy, qy, fma(qz, qz, fma(qw, qw, -1.0))));
    const double rn = fma(e, fma(e, 0.375, -0.5), 1.0);
#endif
    f4 jr = {(float)(qx * rn), (float)(qy * rn), (float)(qz * rn), (float)(qw * rn)};
    rot = qmul_xyzw(prot, unit_lr ? jr : qmul_xyzw(lr, jr));
    return;
  }  // no joint: r_j * (0,0,0,1) == r_j exactly
  rot = unit_lr ? prot : qmul_xyzw(prot, lr);
}

}  // namespace gmr
