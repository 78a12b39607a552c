// gmr_smplx.hip -- SMPL-X frame extraction on the device: the step in
// front of the retargeting loop.  Replaces, for a whole clip in one launch each,
//   * the joints-only part of the body-model forward pass called at utils/smpl.py:12-34
//     (smplx_joints_kernel; the mesh, 10 475 vertices, is never needed by GMR), and
//   * get_smplx_data_offline_fast / get_smplx_data (utils/smpl.py:44-197): SLERP fps alignment of every
//     local joint rotation, linear interpolation of the joint positions, chain of global orientations
//     (smplx_align_kernel), writing the packed human[T'][nhuman][7] frames the IK kernel consumes.
//
// Mapping: lane = output frame.  The tree is walked in DFS order (host-built program); the transform of the
// ancestor at depth d sits in a lane-private LDS column stack[d][.][lane] (conflict-free), so LDS holds
// max_depth, not J, transforms.  Both kernels are streaming (read 2 pose rows + 2 joint rows, write nsel x 56 B
// per frame); the transcendental chain per joint makes them FP64-VALU bound well below the HBM roof, three
// orders of magnitude above the IK kernel's frame rate, so they are written for exactness, not tuned.
//
// Arithmetic follows the SciPy formulas the reference goes through (from_rotvec / as_rotvec small-angle
// series at 1e-3, from_quat normalisation, interp1d's float32 difference).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_internal.h"
#include "gmr_workspace.h"

#include "gmr_smplx_prog.h"        // SmplxProg, make_prog, the LDS sizes (host-only, checked by tests/cpp/ingest_prog_check.cpp)

namespace gmr {

struct q4 { double x, y, z, w; };   // xyzw like SciPy

__device__ __forceinline__ q4 sx_from_rotvec(double vx, double vy, double vz) {
  const double a = sqrt(vx * vx + vy * vy + vz * vz);
  double scale;
  if (a <= 1e-3) {
    const double a2 = a * a;
    scale = 0.5 - a2 / 48.0 + a2 * a2 / 3840.0;
  } else {
    scale = sin(a / 2.0) / a;
  }
  return q4{scale * vx, scale * vy, scale * vz, cos(a / 2.0)};
}

__device__ __forceinline__ q4 sx_normalize(q4 q) {
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return q4{q.x / n, q.y / n, q.z / n, q.w / n};
}

__device__ __forceinline__ q4 sx_compose(q4 p, q4 q) {
  const double cx = p.y * q.z - p.z * q.y, cy = p.z * q.x - p.x * q.z, cz = p.x * q.y - p.y * q.x;
  q4 r;
  r.x = p.w * q.x + q.w * p.x + cx;
  r.y = p.w * q.y + q.w * p.y + cy;
  r.z = p.w * q.z + q.w * p.z + cz;
  r.w = p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z;
  return sx_normalize(r);
}

// slerp() of utils/smpl.py:76-107 followed by .as_rotvec() and from_rotvec() again (:140, :181-186)
__device__ __forceinline__ q4 sx_slerp_local(q4 q1, q4 q2, double t) {
  q1 = sx_normalize(q1);
  q2 = sx_normalize(q2);
  double dot = q1.x * q2.x + q1.y * q2.y + q1.z * q2.z + q1.w * q2.w;
  if (dot < 0.0) { q2 = q4{-q2.x, -q2.y, -q2.z, -q2.w}; dot = -dot; }
  q4 q;
  if (dot > 0.9995) {
    q = q4{q1.x + t * (q2.x - q1.x), q1.y + t * (q2.y - q1.y), q1.z + t * (q2.z - q1.z), q1.w + t * (q2.w - q1.w)};
  } else {
    const double th0 = acos(dot), th = th0 * t;
    const double st = sin(th), st0 = sin(th0);
    const double s0 = cos(th) - dot * st / st0, s1 = st / st0;
    q = q4{s0 * q1.x + s1 * q2.x, s0 * q1.y + s1 * q2.y, s0 * q1.z + s1 * q2.z, s0 * q1.w + s1 * q2.w};
  }
  q = sx_normalize(q);
  // as_rotvec
  if (q.w < 0) q = q4{-q.x, -q.y, -q.z, -q.w};
  const double a = 2.0 * atan2(sqrt(q.x * q.x + q.y * q.y + q.z * q.z), q.w);
  double scale;
  if (a <= 1e-3) {
    const double a2 = a * a;
    scale = 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0;
  } else {
    scale = a / sin(a / 2.0);
  }
  return sx_from_rotvec(scale * q.x, scale * q.y, scale * q.z);
}

#pragma clang fp contract(off)

// out[Nout][nrow][7]: pos xyz, quat wxyz.  ALIGN: target_time[Nout] (np.linspace(0, N-1, Nout)); else Nout == N.
// COMPACT: the inputs hold only what the kernel reads, FRAME-MINOR -- full_pose[P.n][3][N] in the order of the program's
// steps (the ancestor closure of the selection), joints[P.nrow][3][N] in output-row order.  A load instruction of the walk
// (one component of one joint, 64 consecutive output frames) then reads one short contiguous run of source frames, and
// the two frames of an interpolation pair sit next to each other in it: every fetched line is consumed by the loads that
// brought it in.  (Frame-major rows -- a lane's 240 B of poses touched joint by joint over the 200 us its libm chains
// take, 14 000 lanes per XCD -- kept 14 MB of lines open against 4 MB of L2 and fetched them two to three times:
// 6.3 x the algorithmic traffic in round 2, unchanged by compact frame-major rows in round 3.)
template <bool ALIGN, bool COMPACT>
__global__ __launch_bounds__(SX_BLOCK) void smplx_align_kernel(SmplxProg P, int N, int jstride,
                                                               const float* __restrict__ full_pose,
                                                               const float* __restrict__ joints, int Nout,
                                                               const double* __restrict__ target_time,
                                                               double* __restrict__ out) {
  extern __shared__ __align__(16) double stack[];   // [max_depth][4][SX_BLOCK]
  const int lane = threadIdx.x;
  const int o = blockIdx.x * SX_BLOCK + lane;
  if (o >= Nout) return;                             // no barriers in this kernel: columns are lane-private
  double t = 0.0, alpha = 0.0;
  int idx1 = o, idx2 = o, lo = o, hi = o;
  if (ALIGN) {
    t = target_time[o];
    idx1 = (int)floor(t);
    idx1 = min(max(idx1, 0), N - 1);
    idx2 = min(idx1 + 1, N - 1);
    alpha = t - (double)idx1;
    int ss = (int)ceil(t);
    ss = min(max(ss, 1), N - 1);
    lo = ss - 1; hi = ss;
  }
  // COMPACT with jstride < 0: the planes are those of ALL joints, indexed by joint (what the joints kernel reads and writes:
  // gmr_smplx_frames runs both steps without a gather in between)
  const bool byjoint = COMPACT && jstride < 0;
  // element (joint j, component c) of source frame f: frame-major rows, or frame-minor planes (COMPACT)
  const size_t pstep = COMPACT ? (size_t)N : 1, pj3 = COMPACT ? 3 * (size_t)N : 3;
  const float* p1 = full_pose + (COMPACT ? (size_t)idx1 : (size_t)idx1 * P.J * 3);
  const float* p2 = full_pose + (COMPACT ? (size_t)idx2 : (size_t)idx2 * P.J * 3);
  const float* jl = joints + (COMPACT ? (size_t)lo : (size_t)lo * jstride * 3);
  const float* jh = joints + (COMPACT ? (size_t)hi : (size_t)hi * jstride * 3);
  double* orow = out + (size_t)o * P.nrow * 7;
  for (int k = 0; k < P.n; k++) {
    const int j = (COMPACT && !byjoint) ? k : P.joint[k], d = P.depth[k];
    q4 ql;
    const float* a1 = p1 + (size_t)j * pj3;
    if (ALIGN) {
      const float* a2 = p2 + (size_t)j * pj3;
      q4 qa = sx_from_rotvec((double)a1[0], (double)a1[pstep], (double)a1[2 * pstep]);
      q4 qb = sx_from_rotvec((double)a2[0], (double)a2[pstep], (double)a2[2 * pstep]);
      ql = sx_slerp_local(qa, qb, alpha);
    } else {
      ql = sx_from_rotvec((double)a1[0], (double)a1[pstep], (double)a1[2 * pstep]);
    }
    q4 qg = ql;
    if (d > 0) {
      const double* s = stack + (size_t)(d - 1) * 4 * SX_BLOCK + lane;
      qg = sx_compose(q4{s[0], s[SX_BLOCK], s[2 * SX_BLOCK], s[3 * SX_BLOCK]}, ql);
    }
    {
      double* s = stack + (size_t)d * 4 * SX_BLOCK + lane;
      s[0] = qg.x; s[SX_BLOCK] = qg.y; s[2 * SX_BLOCK] = qg.z; s[3 * SX_BLOCK] = qg.w;
    }
    const int r = P.row[k];
    if (r >= 0) {
      double* w = orow + r * 7;
      const int jj = (COMPACT && !byjoint) ? r : j;                   // (compact joints: one row per output row)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if (ALIGN) {
          const float ylo = jl[(size_t)jj * pj3 + c * pstep], yhi = jh[(size_t)jj * pj3 + c * pstep];
          const float df = yhi - ylo;                                  // float32 difference (interp1d on a float32 y)
          const double slope = (double)df / (double)(hi - lo);
          w[c] = slope * (t - (double)lo) + (double)ylo;
        } else {
          w[c] = (double)jl[(size_t)jj * pj3 + c * pstep];
        }
      }
      w[3] = qg.w; w[4] = qg.x; w[5] = qg.y; w[6] = qg.z;
    }
  }
}

// Frame-major rows f32[N][C] <-> frame-minor planes f32[C][N] (C = J * 3 <= 256), 64 frames per block through one LDS tile.
// The joints kernel reads its poses and writes its joints as planes -- lane = frame, so every load / store instruction is
// one contiguous run; with frame-major rows a lane's 660-byte row stays open for the 200 us of its walk, and at eight or
// more blocks per CU the rows in flight (100 MB) no longer fit the L2: 2.2 GB fetched and 3.0 GB written for 0.69 + 0.69 GB
// (measured, profiles/r03_v6_*).  A block's 64 rows are ONE contiguous range of the row array (read / written flat, 16 bytes
// per lane), its piece of a plane 256 bytes.  (First version: generic 64 x 64 tiles, whose row side moved 256-byte pieces of
// 660-byte rows: 0.42 ms per 2^20 x 165 floats, 3.3 TB/s.)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

template <bool TO_PLANES>
__global__ __launch_bounds__(256) void rows_planes_kernel(const float* __restrict__ src, int N, int C, float* __restrict__ dst) {
  extern __shared__ float tile[];                      // [64][C + 1]
  const int r0 = blockIdx.x * 64, nr = min(64, N - r0), ld = C + 1, n = nr * C;
  const unsigned magic = (1u << 24) / (unsigned)C + 1u; // e / C for e < 2^14, C <= 256
  const int q = (threadIdx.x & 15) * 4, g = threadIdx.x >> 4;
  const float* rows_in = src + (size_t)r0 * C;          // TO_PLANES: flat rows in
  float* rows_out = dst + (size_t)r0 * C;               // else: flat rows out
  if (TO_PLANES) {
    for (int i = threadIdx.x * 4; i < n; i += 1024) {
      float v[4];
      if (i + 3 < n) { const f4u t = *reinterpret_cast<const f4u*>(rows_in + i); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
      else for (int k = 0; k < 4; k++) v[k] = i + k < n ? rows_in[i + k] : 0.0f;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const unsigned e = (unsigned)(i + k), r = (e * magic) >> 24;
        if ((int)e < n) tile[r * ld + (e - r * C)] = v[k];
      }
    }
  } else {
    for (int c = g; c < C; c += 16) {
      const float* p = src + (size_t)c * N + r0 + q;
      if (q + 3 < nr) { const f4u t = *reinterpret_cast<const f4u*>(p); tile[q * ld + c] = t.x; tile[(q + 1) * ld + c] = t.y; tile[(q + 2) * ld + c] = t.z; tile[(q + 3) * ld + c] = t.w; }
      else for (int k = 0; k < 4 && q + k < nr; k++) tile[(q + k) * ld + c] = p[k];
    }
  }
  __syncthreads();
  if (TO_PLANES) {
    for (int c = g; c < C; c += 16) {
      float* p = dst + (size_t)c * N + r0 + q;
      if (q + 3 < nr) { f4u t; t.x = tile[q * ld + c]; t.y = tile[(q + 1) * ld + c]; t.z = tile[(q + 2) * ld + c]; t.w = tile[(q + 3) * ld + c]; *reinterpret_cast<f4u*>(p) = t; }
      else for (int k = 0; k < 4 && q + k < nr; k++) p[k] = tile[(q + k) * ld + c];
    }
  } else {
    for (int i = threadIdx.x * 4; i < n; i += 1024) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const unsigned e = (unsigned)(i + k), r = (e * magic) >> 24;
        v[k] = (int)e < n ? tile[r * ld + (e - r * C)] : 0.0f;
      }
      if (i + 3 < n) { f4u t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3]; *reinterpret_cast<f4u*>(rows_out + i) = t; }
      else for (int k = 0; k < 4 && i + k < n; k++) rows_out[i + k] = v[k];
    }
  }
}

// joints from rest joints f64[J][3], poses, translations f32[N][3].  PLANES: poses and joints are frame-minor planes
// f32[J * 3][N] (the entry point transposes on either side); else frame-major rows f32[N][J][3]
template <bool PLANES>
__global__ __launch_bounds__(SX_BLOCK) void smplx_joints_kernel(SmplxProg P, int N, const double* __restrict__ j_rest,
                                                                const float* __restrict__ full_pose,
                                                                const float* __restrict__ transl,
                                                                float* __restrict__ joints) {
  // Parked transforms [nslot][12][SX_BLOCK] (R row-major, p), one column per lane.  A depth-indexed stack needs 11 levels for
  // SMPL-X -- 66 KB, two single-wavefront blocks per CU for a kernel whose time is the latency of its libm chains --; in DFS
  // order a joint's first child follows it immediately, so only joints with several children are parked: 3 slots, 18 KB.
  extern __shared__ __align__(16) double stack[];
  const int lane = threadIdx.x;
  const int n = blockIdx.x * SX_BLOCK + lane;
  if (n >= N) return;
  // element c of joint j of this lane's frame
  const float* pr = full_pose + (PLANES ? (size_t)n : (size_t)n * P.J * 3);
  float* jo = joints + (PLANES ? (size_t)n : (size_t)n * P.J * 3);
  const size_t es = PLANES ? (size_t)N : 1;
  const double tx = transl[(size_t)n * 3], ty = transl[(size_t)n * 3 + 1], tz = transl[(size_t)n * 3 + 2];
  double Rc[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pc[3] = {0, 0, 0};        // the transform of the previous step
  // the innermost parking slot (SMPL-X: a wrist while its fingers are walked, the head for jaw and eyes) is 24 registers
  // instead of 6 KB of LDS: 2 slots = 12 KB, twelve blocks per CU
  const int rslot = P.nslot - 1;
  double Rs[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, ps[3] = {0, 0, 0};
  // the pose of step k + 1 and its rest offset are requested while step k computes (a lane's pose row shares no line with its
  // neighbours': every read is a trip to L2 that nothing else would hide at two wavefronts per SIMD)
  float nvx = pr[(3 * P.joint[0]) * es], nvy = pr[(3 * P.joint[0] + 1) * es], nvz = pr[(3 * P.joint[0] + 2) * es];
  double nrel[3] = {j_rest[3 * P.joint[0]], j_rest[3 * P.joint[0] + 1], j_rest[3 * P.joint[0] + 2]};
  for (int k = 0; k < P.n; k++) {
    const int j = P.joint[k], d = P.depth[k];
    const double vx = nvx, vy = nvy, vz = nvz;
    const double rel[3] = {nrel[0], nrel[1], nrel[2]};      // step 0: the root's rest position
    if (k + 1 < P.n) {
      const int jn = P.joint[k + 1], pn = P.parent[k + 1];
      nvx = pr[(3 * jn) * es]; nvy = pr[(3 * jn + 1) * es]; nvz = pr[(3 * jn + 2) * es];
      nrel[0] = j_rest[3 * jn] - j_rest[3 * pn]; nrel[1] = j_rest[3 * jn + 1] - j_rest[3 * pn + 1]; nrel[2] = j_rest[3 * jn + 2] - j_rest[3 * pn + 2];
    }
    const double ax = vx + 1e-8, ay = vy + 1e-8, az = vz + 1e-8;
    const double ang = sqrt(ax * ax + ay * ay + az * az);
    const double x = vx / ang, y = vy / ang, z = vz / ang, s = sin(ang), c1 = 1.0 - cos(ang);
    const double K[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    double Rl[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) {
        double acc = 0;
#pragma unroll
        for (int m = 0; m < 3; m++) acc += K[a * 3 + m] * K[m * 3 + b];
        Rl[a * 3 + b] = (a == b ? 1.0 : 0.0) + s * K[a * 3 + b] + c1 * acc;
      }
    double Rg[9], pg[3];
    if (d == 0) {
#pragma unroll
      for (int i = 0; i < 9; i++) Rg[i] = Rl[i];
      pg[0] = rel[0]; pg[1] = rel[1]; pg[2] = rel[2];
    } else {
      double Rp[9], pp[3];
      const int ld = P.load[k];                       // (uniform)
      if (ld == rslot) {
#pragma unroll
        for (int i = 0; i < 9; i++) Rp[i] = Rs[i];
#pragma unroll
        for (int i = 0; i < 3; i++) pp[i] = ps[i];
      } else if (ld >= 0) {
        const double* sp = stack + (size_t)ld * 12 * SX_BLOCK + lane;
#pragma unroll
        for (int i = 0; i < 9; i++) Rp[i] = sp[i * SX_BLOCK];
#pragma unroll
        for (int i = 0; i < 3; i++) pp[i] = sp[(9 + i) * SX_BLOCK];
      } else {
#pragma unroll
        for (int i = 0; i < 9; i++) Rp[i] = Rc[i];
#pragma unroll
        for (int i = 0; i < 3; i++) pp[i] = pc[i];
      }
#pragma unroll
      for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int b = 0; b < 3; b++) {
          double acc = 0;
#pragma unroll
          for (int m = 0; m < 3; m++) acc += Rp[a * 3 + m] * Rl[m * 3 + b];
          Rg[a * 3 + b] = acc;
        }
        pg[a] = pp[a] + Rp[a * 3] * rel[0] + Rp[a * 3 + 1] * rel[1] + Rp[a * 3 + 2] * rel[2];
      }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) Rc[i] = Rg[i];
#pragma unroll
    for (int i = 0; i < 3; i++) pc[i] = pg[i];
    const int sv = P.save[k];                         // (uniform)
    if (sv == rslot) {
#pragma unroll
      for (int i = 0; i < 9; i++) Rs[i] = Rg[i];
#pragma unroll
      for (int i = 0; i < 3; i++) ps[i] = pg[i];
    } else if (sv >= 0) {
      double* so = stack + (size_t)sv * 12 * SX_BLOCK + lane;
#pragma unroll
      for (int i = 0; i < 9; i++) so[i * SX_BLOCK] = Rg[i];
#pragma unroll
      for (int i = 0; i < 3; i++) so[(9 + i) * SX_BLOCK] = pg[i];
    }
    jo[(3 * j) * es] = (float)(pg[0] + tx);
    jo[(3 * j + 1) * es] = (float)(pg[1] + ty);
    jo[(3 * j + 2) * es] = (float)(pg[2] + tz);
  }
}

// ---- a ragged batch of clips straight from the AMASS arrays (gmr_smplx_batch_frames_dev) ----------------------------------
// Two launches over the B concatenated source frames, lane = frame, 64 frames per block:
//   smplx_batch_joints_kernel  lane = SOURCE frame.  The block's 64 pose_body rows are ONE contiguous range (64 x 252 B), copied
//       flat into an LDS tile (16-byte loads, every fetched line consumed at once) and read back by row (stride 63 words: no bank
//       conflict); root_orient and trans are 12-byte rows, read directly.  The walk is smplx_joints_kernel's over the ancestor
//       closure of the selection only (a joint's transform depends on its ancestors alone, so the closure's joints get the bits
//       of the all-joints walk).  It leaves what the second kernel reads as FRAME-MINOR planes in the call's scratch: the poses
//       of the closure pose_t f32[P.n][3][Bp] in walk order and the joints of the output rows joints_t f32[P.nrow][3][Bp] --
//       the compact layout of smplx_align_kernel, whose measured history (above) is why frame-major rows are not read there:
//       an output frame's two source frames are 1 .. 8 rows apart, so a wavefront's rows span up to 130 KB.
//   smplx_batch_align_kernel   lane = OUTPUT frame o of its clip, indexed in the SOURCE frames' index space (nout <= N for every
//       clip, so lane b of clip c is output frame o = b - src_start[c], idle when o >= nout[c]: no second prefix array, and at
//       120 -> 30 fps whole wavefronts leave at once).  smplx_align_kernel's arithmetic, `align` a per-clip run-time flag, the
//       target time computed here (sx_target_time), the frame stored at clip_out[c] + o * nrow * 7.
// Frame -> clip: binary search of src_start (the prefix array the caller has anyway; a clip may be shorter than a wavefront or
// longer than thousands of blocks, so whole blocks per clip would idle most lanes of short clips).  The tables are not trusted:
// the search ends after log2(nclip) steps whatever they hold, the clip's range is clamped into [0, B], and a lane outside its
// clip's clamped range returns, so every load stays inside the B-frame inputs and the scratch.  A store goes to frame o <
// min(nout[c], N_c) of clip_out[c].
// np.linspace(0, N - 1, Nout)[o] (utils/smpl.py:127): arange(Nout) * ((N - 1) / (Nout - 1)), the last one set to N - 1
__host__ __device__ inline double sx_target_time(int o, int N, int Nout) {
  if (Nout <= 1) return 0.0;
  if (o == Nout - 1) return (double)(N - 1);
  return (double)o * ((double)(N - 1) / (double)(Nout - 1));
}

// the last clip whose start is <= b (empty clips in front of it are skipped); always in [0, nclip - 1]
__device__ __forceinline__ int sx_clip_of(const int32_t* __restrict__ src_start, int nclip, int b) {
  int lo = 0, hi = nclip - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (src_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(SX_BLOCK) void smplx_batch_joints_kernel(SmplxProg P, int nclip, int B, size_t Bp, int nslot_lds,
                                                                      const float* __restrict__ root_orient,
                                                                      const float* __restrict__ pose_body,
                                                                      const float* __restrict__ trans,
                                                                      const int32_t* __restrict__ src_start,
                                                                      const double* __restrict__ j_rest,
                                                                      float* __restrict__ pose_t, float* __restrict__ joints_t) {
  extern __shared__ __align__(16) double stack[];     // parked transforms [nslot_lds][12][SX_BLOCK], then the tile f32[64][63]
  float* tile = reinterpret_cast<float*>(stack + (size_t)nslot_lds * 12 * SX_BLOCK);
  const int lane = threadIdx.x;
  const int b0 = blockIdx.x * SX_BLOCK, b = b0 + lane;
  {
    const int n = min(SX_BLOCK, B - b0) * SX_BODY_POSE;
    const float* rows_in = pose_body + (size_t)b0 * SX_BODY_POSE;
    for (int i = lane * 4; i < n; i += SX_BLOCK * 4) {
      if (i + 3 < n) {
        const f4u t = *reinterpret_cast<const f4u*>(rows_in + i);
        tile[i] = t.x; tile[i + 1] = t.y; tile[i + 2] = t.z; tile[i + 3] = t.w;
      } else {
        for (int k = 0; i + k < n; k++) tile[i + k] = rows_in[i + k];
      }
    }
  }
  __syncthreads();                                     // the only barrier: every lane of the block reaches it
  if (b >= B) return;
  const int c = sx_clip_of(src_start, nclip, b);
  const double* jr = j_rest + (size_t)c * P.J * 3;
  const float* pr = tile + lane * SX_BODY_POSE;        // joint j >= 1: pr[3 (j - 1) + c]
  const float* ro = root_orient + (size_t)b * 3;
  const double tx = trans[(size_t)b * 3], ty = trans[(size_t)b * 3 + 1], tz = trans[(size_t)b * 3 + 2];
  double Rc[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pc[3] = {0, 0, 0};        // the transform of the previous step
  const int rslot = P.nslot - 1;                                         // the innermost parking slot lives in registers
  double Rs[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, ps[3] = {0, 0, 0};
  for (int k = 0; k < P.n; k++) {
    const int j = P.joint[k], d = P.depth[k], pj = P.parent[k];
    // full_pose of the host path: concatenate, then `+ pose_mean` (zero on the body joints; -0.0f + 0.0f = +0.0f)
    float fx, fy, fz;
    if (j == 0) { fx = ro[0] + 0.0f; fy = ro[1] + 0.0f; fz = ro[2] + 0.0f; }                // (uniform)
    else { const float* q = pr + 3 * (j - 1); fx = q[0] + 0.0f; fy = q[1] + 0.0f; fz = q[2] + 0.0f; }
    pose_t[(size_t)(3 * k) * Bp + b] = fx;
    pose_t[(size_t)(3 * k + 1) * Bp + b] = fy;
    pose_t[(size_t)(3 * k + 2) * Bp + b] = fz;
    const double vx = fx, vy = fy, vz = fz;
    double rel[3];
    if (k == 0) { rel[0] = jr[3 * j]; rel[1] = jr[3 * j + 1]; rel[2] = jr[3 * j + 2]; }     // the root's rest position
    else { rel[0] = jr[3 * j] - jr[3 * pj]; rel[1] = jr[3 * j + 1] - jr[3 * pj + 1]; rel[2] = jr[3 * j + 2] - jr[3 * pj + 2]; }
    const double ax = vx + 1e-8, ay = vy + 1e-8, az = vz + 1e-8;
    const double ang = sqrt(ax * ax + ay * ay + az * az);
    const double x = vx / ang, y = vy / ang, z = vz / ang, s = sin(ang), c1 = 1.0 - cos(ang);
    const double K[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    double Rl[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int e = 0; e < 3; e++) {
        double acc = 0;
#pragma unroll
        for (int m = 0; m < 3; m++) acc += K[a * 3 + m] * K[m * 3 + e];
        Rl[a * 3 + e] = (a == e ? 1.0 : 0.0) + s * K[a * 3 + e] + c1 * acc;
      }
    double Rg[9], pg[3];
    if (d == 0) {
#pragma unroll
      for (int i = 0; i < 9; i++) Rg[i] = Rl[i];
      pg[0] = rel[0]; pg[1] = rel[1]; pg[2] = rel[2];
    } else {
      double Rp[9], pp[3];
      const int ld = P.load[k];                       // (uniform)
      if (ld == rslot) {
#pragma unroll
        for (int i = 0; i < 9; i++) Rp[i] = Rs[i];
#pragma unroll
        for (int i = 0; i < 3; i++) pp[i] = ps[i];
      } else if (ld >= 0) {
        const double* sp = stack + (size_t)ld * 12 * SX_BLOCK + lane;
#pragma unroll
        for (int i = 0; i < 9; i++) Rp[i] = sp[i * SX_BLOCK];
#pragma unroll
        for (int i = 0; i < 3; i++) pp[i] = sp[(9 + i) * SX_BLOCK];
      } else {
#pragma unroll
        for (int i = 0; i < 9; i++) Rp[i] = Rc[i];
#pragma unroll
        for (int i = 0; i < 3; i++) pp[i] = pc[i];
      }
#pragma unroll
      for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int e = 0; e < 3; e++) {
          double acc = 0;
#pragma unroll
          for (int m = 0; m < 3; m++) acc += Rp[a * 3 + m] * Rl[m * 3 + e];
          Rg[a * 3 + e] = acc;
        }
        pg[a] = pp[a] + Rp[a * 3] * rel[0] + Rp[a * 3 + 1] * rel[1] + Rp[a * 3 + 2] * rel[2];
      }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) Rc[i] = Rg[i];
#pragma unroll
    for (int i = 0; i < 3; i++) pc[i] = pg[i];
    const int sv = P.save[k];                         // (uniform)
    if (sv == rslot) {
#pragma unroll
      for (int i = 0; i < 9; i++) Rs[i] = Rg[i];
#pragma unroll
      for (int i = 0; i < 3; i++) ps[i] = pg[i];
    } else if (sv >= 0) {
      double* so = stack + (size_t)sv * 12 * SX_BLOCK + lane;
#pragma unroll
      for (int i = 0; i < 9; i++) so[i * SX_BLOCK] = Rg[i];
#pragma unroll
      for (int i = 0; i < 3; i++) so[(9 + i) * SX_BLOCK] = pg[i];
    }
    const int r = P.row[k];
    if (r >= 0) {
      joints_t[(size_t)(3 * r) * Bp + b] = (float)(pg[0] + tx);
      joints_t[(size_t)(3 * r + 1) * Bp + b] = (float)(pg[1] + ty);
      joints_t[(size_t)(3 * r + 2) * Bp + b] = (float)(pg[2] + tz);
    }
  }
}

__global__ __launch_bounds__(SX_BLOCK) void smplx_batch_align_kernel(SmplxProg P, int nclip, int B, size_t Bp,
                                                                     const int32_t* __restrict__ src_start,
                                                                     const int32_t* __restrict__ nout,
                                                                     const uint8_t* __restrict__ align,
                                                                     const float* __restrict__ pose_t,
                                                                     const float* __restrict__ joints_t,
                                                                     double* const* __restrict__ clip_out) {
  extern __shared__ __align__(16) double stack[];   // [max_depth][4][SX_BLOCK]
  const int lane = threadIdx.x;
  const int b = blockIdx.x * SX_BLOCK + lane;
  if (b >= B) return;                                // no barriers in this kernel: columns are lane-private
  const int c = sx_clip_of(src_start, nclip, b);
  const int s0 = min(max(src_start[c], 0), B), s1 = min(max(src_start[c + 1], s0), B);
  const int N = s1 - s0, o = b - s0, Nout = nout[c];
  if (o < 0 || o >= N || o >= Nout) return;
  const bool al = align[c] != 0;
  if (al && N < 2) return;                           // (the host entry point refuses such a clip)
  double* dst = clip_out[c];
  if (!dst) return;
  double t = 0.0, alpha = 0.0;
  int idx1 = o, idx2 = o, lo = o, hi = o;
  if (al) {
    t = sx_target_time(o, N, Nout);
    idx1 = (int)floor(t);
    idx1 = min(max(idx1, 0), N - 1);
    idx2 = min(idx1 + 1, N - 1);
    alpha = t - (double)idx1;
    int ss = (int)ceil(t);
    ss = min(max(ss, 1), N - 1);
    lo = ss - 1; hi = ss;
  }
  const size_t pstep = Bp, pj3 = 3 * Bp;
  const float* p1 = pose_t + s0 + idx1;
  const float* p2 = pose_t + s0 + idx2;
  const float* jl = joints_t + s0 + lo;
  const float* jh = joints_t + s0 + hi;
  double* orow = dst + (size_t)o * P.nrow * 7;
  for (int k = 0; k < P.n; k++) {
    const int d = P.depth[k];
    q4 ql;
    const float* a1 = p1 + (size_t)k * pj3;
    if (al) {
      const float* a2 = p2 + (size_t)k * pj3;
      q4 qa = sx_from_rotvec((double)a1[0], (double)a1[pstep], (double)a1[2 * pstep]);
      q4 qb = sx_from_rotvec((double)a2[0], (double)a2[pstep], (double)a2[2 * pstep]);
      ql = sx_slerp_local(qa, qb, alpha);
    } else {
      ql = sx_from_rotvec((double)a1[0], (double)a1[pstep], (double)a1[2 * pstep]);
    }
    q4 qg = ql;
    if (d > 0) {
      const double* s = stack + (size_t)(d - 1) * 4 * SX_BLOCK + lane;
      qg = sx_compose(q4{s[0], s[SX_BLOCK], s[2 * SX_BLOCK], s[3 * SX_BLOCK]}, ql);
    }
    {
      double* s = stack + (size_t)d * 4 * SX_BLOCK + lane;
      s[0] = qg.x; s[SX_BLOCK] = qg.y; s[2 * SX_BLOCK] = qg.z; s[3 * SX_BLOCK] = qg.w;
    }
    const int r = P.row[k];
    if (r >= 0) {
      double* w = orow + r * 7;
#pragma unroll
      for (int e = 0; e < 3; e++) {
        if (al) {
          const float ylo = jl[(size_t)r * pj3 + e * pstep], yhi = jh[(size_t)r * pj3 + e * pstep];
          const float df = yhi - ylo;                                  // float32 difference (interp1d on a float32 y)
          const double slope = (double)df / (double)(hi - lo);
          w[e] = slope * (t - (double)lo) + (double)ylo;
        } else {
          w[e] = (double)jl[(size_t)r * pj3 + e * pstep];
        }
      }
      w[3] = qg.w; w[4] = qg.x; w[5] = qg.y; w[6] = qg.z;
    }
  }
}

}  // namespace gmr

struct gmr_smplx {
  int J = 0, nsel = 0;
  gmr::SmplxProg all, sel;       // every joint (rows = joint index) / ancestor closure of the selection
  gmr::DeviceBlock jrest;        // staging of the host entry points: j_rest f64[J][3]
  gmr::DeviceBlock ws;           // their device workspace, grown on demand and kept (a hipMalloc / hipFree pair per clip costs
                                 //  more than the kernels of a short clip)
  std::mutex mu;                 // the host entry points of one handle run one at a time (they share jrest and ws)
  gmr::StreamWorkspace planes;   // gmr_smplx_joints_dev: the transposed poses and joints of a launch
  // gmr_smplx_batch_frames_dev takes the handle only when the selection's ancestor closure lies inside the body joints
  bool batch_ok = false;
  int batch_lds_joints = 0, batch_lds_align = 0, batch_nslot_lds = 1;
  gmr::StreamWorkspace batch_ws;
  std::mutex batch_host_mu;      // gmr_smplx_batch_frames: device staging of the host buffers, grown on demand and kept
  gmr::DeviceBlock batch_host_ws;
};

extern "C" {

int gmr_smplx_create(int J, const int32_t* parents, int nsel, const int32_t* sel, gmr_smplx_t** out) {
  if (!parents || !out || J < 1 || J > SX_MAX_JOINTS) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_create: 1 <= J <= %d", SX_MAX_JOINTS);
  if (nsel < 0 || nsel > J || (nsel > 0 && !sel)) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_create: bad selection");
  for (int j = 0; j < J; j++)
    if (parents[j] >= j || (j > 0 && parents[j] < 0) || (j == 0 && parents[j] >= 0))
      return gmr_fail(GMR_ERR_ARG, "gmr_smplx_create: parents must precede children, joint 0 is the only root (joint %d)", j);
  gmr_smplx* h = new (std::nothrow) gmr_smplx;
  if (!h) return gmr_fail(GMR_ERR_ARG, "out of memory");
  h->J = J;
  h->nsel = nsel;
  const bool ok = gmr::smplx_make_progs(J, parents, nsel, sel, &h->all, &h->sel);
  if (!ok) { delete h; return gmr_fail(GMR_ERR_ARG, "gmr_smplx_create: bad tree or duplicate / out-of-range selection"); }
  const gmr::SmplxLds lds = gmr::smplx_lds(h->all, h->sel, nsel);
  const int lds_align = lds.align, lds_joints = lds.joints;
  if (lds_joints > gmr::SX_LDS_LIMIT) { delete h; return gmr_fail(GMR_ERR_ARG, "gmr_smplx_create: tree too deep (%d levels)", h->all.max_depth); }
  hipError_t e = hipSuccess;
  if (lds_align > gmr::SX_LDS_DEFAULT) {
    e = hipFuncSetAttribute((const void*)gmr::smplx_align_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_align);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)gmr::smplx_align_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_align);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)gmr::smplx_align_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_align);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)gmr::smplx_align_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_align);
  }
  if (e == hipSuccess && lds_joints > gmr::SX_LDS_DEFAULT)
    {
    e = hipFuncSetAttribute((const void*)gmr::smplx_joints_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_joints);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)gmr::smplx_joints_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_joints);
  }
  h->batch_ok = lds.batch_ok;
  h->batch_nslot_lds = lds.batch_nslot;
  h->batch_lds_joints = lds.batch_joints;
  h->batch_lds_align = lds.batch_align;
  if (e == hipSuccess && h->batch_ok && h->batch_lds_joints > gmr::SX_LDS_DEFAULT)
    e = hipFuncSetAttribute((const void*)gmr::smplx_batch_joints_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, h->batch_lds_joints);
  if (e == hipSuccess && h->batch_ok && h->batch_lds_align > gmr::SX_LDS_DEFAULT)
    e = hipFuncSetAttribute((const void*)gmr::smplx_batch_align_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, h->batch_lds_align);
  if (e == hipSuccess) e = h->jrest.reserve((size_t)J * 3 * sizeof(double));
  if (e != hipSuccess) { delete h; return gmr_fail(GMR_ERR_HIP, "gmr_smplx_create: %s", hipGetErrorString(e)); }
  *out = h;
  return GMR_OK;
}

int gmr_smplx_destroy(gmr_smplx_t* h) {
  delete h;                                // (freeing its blocks waits for the device: nothing of the handle is in flight afterwards)
  return GMR_OK;
}

int gmr_smplx_rows(const gmr_smplx_t* h) { return h ? h->sel.nrow : 0; }

int gmr_smplx_joints_dev(gmr_smplx_t* h, int N, const double* d_j_rest, const float* d_full_pose, const float* d_transl,
                         float* d_joints, void* stream) {
  if (!h || N < 0 || !d_j_rest || !d_full_pose || !d_transl || !d_joints) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_joints_dev: bad argument");
  if (N == 0) return GMR_OK;
  const int lds = std::max(h->all.nslot - 1, 1) * 12 * SX_BLOCK * 8;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((N + SX_BLOCK - 1) / SX_BLOCK), block(SX_BLOCK);
  static const bool rows = getenv("GMR_SMPLX_ROWS") != nullptr;       // A/B: the walk on frame-major rows
  if (rows) {
    hipLaunchKernelGGL(gmr::smplx_joints_kernel<false>, grid, block, lds, st, h->all, N, d_j_rest, d_full_pose, d_transl, d_joints);
  } else {
    const int C = h->J * 3;
    gmr::Carve c;
    const size_t o_pose = c.take((size_t)N * C * sizeof(float)), o_joints = c.take((size_t)N * C * sizeof(float));
    const auto ws = h->planes.acquire(st, c.total());                 // (held until the last launch below is enqueued)
    GMR_NAMED_HIP_TRY("gmr_smplx_joints_dev", ws.error());
    float* pose_t = reinterpret_cast<float*>(ws.base() + o_pose);
    float* joints_t = reinterpret_cast<float*>(ws.base() + o_joints);
    hipLaunchKernelGGL(gmr::rows_planes_kernel<true>, dim3((N + 63) / 64), dim3(256), 64 * (C + 1) * sizeof(float), st, d_full_pose, N, C, pose_t);
    hipLaunchKernelGGL(gmr::smplx_joints_kernel<true>, grid, block, lds, st, h->all, N, d_j_rest, pose_t, d_transl, joints_t);
    hipLaunchKernelGGL(gmr::rows_planes_kernel<false>, dim3((N + 63) / 64), dim3(256), 64 * (C + 1) * sizeof(float), st, joints_t, N, C, d_joints);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return gmr_fail(GMR_ERR_HIP, "smplx_joints_kernel: %s", hipGetErrorString(e));
  return GMR_OK;
}

static int smplx_align_launch(gmr_smplx_t* h, bool compact, int N, int jstride, const float* d_full_pose, const float* d_joints,
                              int Nout, const double* d_target_time, double* d_out, void* stream) {
  if (!h || N < 1 || Nout < 0 || (!compact && jstride < h->J) || !d_full_pose || !d_joints || !d_out)
    return gmr_fail(GMR_ERR_ARG, "gmr_smplx_align_dev: bad argument");
  if (!d_target_time && Nout != N) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_align_dev: without target times Nout must equal N");
  if (d_target_time && N < 2) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_align_dev: fps alignment needs at least two source frames");
  if (Nout == 0) return GMR_OK;
  const gmr::SmplxProg& P = h->sel;
  const int lds = P.max_depth * 4 * SX_BLOCK * 8;
  dim3 grid((Nout + SX_BLOCK - 1) / SX_BLOCK), block(SX_BLOCK);
#define GMR_SX_LAUNCH(A, C)                                                                                              \
  hipLaunchKernelGGL((gmr::smplx_align_kernel<A, C>), grid, block, lds, (hipStream_t)stream, P, N, jstride, d_full_pose, \
                     d_joints, Nout, d_target_time, d_out)
  if (d_target_time) { if (compact) GMR_SX_LAUNCH(true, true); else GMR_SX_LAUNCH(true, false); }
  else { if (compact) GMR_SX_LAUNCH(false, true); else GMR_SX_LAUNCH(false, false); }
#undef GMR_SX_LAUNCH
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return gmr_fail(GMR_ERR_HIP, "smplx_align_kernel: %s", hipGetErrorString(e));
  return GMR_OK;
}

int gmr_smplx_align_dev(gmr_smplx_t* h, int N, int jstride, const float* d_full_pose, const float* d_joints, int Nout,
                        const double* d_target_time, double* d_out, void* stream) {
  return smplx_align_launch(h, false, N, jstride, d_full_pose, d_joints, Nout, d_target_time, d_out, stream);
}

// the joints the alignment reads, in the order the compact layout stores them: pose_joints[npose] = the ancestor closure of
// the selection in walk order, row_joints[nrow] = the joint of every output row
int gmr_smplx_compact_layout(const gmr_smplx_t* h, int32_t* pose_joints, int* npose, int32_t* row_joints, int* nrow) {
  if (!h) return gmr_fail(GMR_ERR_ARG, "null handle");
  const gmr::SmplxProg& P = h->sel;
  if (npose) *npose = P.n;
  if (nrow) *nrow = P.nrow;
  for (int k = 0; k < P.n; k++) {
    if (pose_joints) pose_joints[k] = P.joint[k];
    if (row_joints && P.row[k] >= 0) row_joints[P.row[k]] = P.joint[k];
  }
  return GMR_OK;
}

int gmr_smplx_align_compact_dev(gmr_smplx_t* h, int N, const float* d_pose_c, const float* d_joints_c, int Nout,
                                const double* d_target_time, double* d_out, void* stream) {
  return smplx_align_launch(h, true, N, 0, d_pose_c, d_joints_c, Nout, d_target_time, d_out, stream);
}

// host-buffer variants: copy, launch, synchronise
int gmr_smplx_joints(gmr_smplx_t* h, int N, const double* j_rest, const float* full_pose, const float* transl, float* joints) {
  if (!h || N < 0 || !j_rest || !full_pose || !transl || !joints) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_joints: bad argument");
  if (N == 0) return GMR_OK;
  const size_t nb_pose = (size_t)N * h->J * 3 * sizeof(float), nb_tr = (size_t)N * 3 * sizeof(float);
  std::lock_guard<std::mutex> guard(h->mu);
  GMR_NAMED_HIP_TRY("gmr_smplx_joints", h->ws.reserve(2 * nb_pose + nb_tr + 64, 4));
  char* ws = h->ws.data();
  hipError_t e = hipSuccess;
  float* d_pose = (float*)ws;
  float* d_j = (float*)(ws + nb_pose);
  float* d_tr = (float*)(ws + 2 * nb_pose);
  int rc = GMR_OK;
  if ((e = hipMemcpy(h->jrest.data(), j_rest, (size_t)h->J * 3 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d_pose, full_pose, nb_pose, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d_tr, transl, nb_tr, hipMemcpyHostToDevice)) != hipSuccess)
    rc = gmr_fail(GMR_ERR_HIP, "gmr_smplx_joints: %s", hipGetErrorString(e));
  if (rc == GMR_OK) rc = gmr_smplx_joints_dev(h, N, (const double*)h->jrest.data(), d_pose, d_tr, d_j, nullptr);
  if (rc == GMR_OK && (e = hipMemcpy(joints, d_j, nb_pose, hipMemcpyDeviceToHost)) != hipSuccess)
    rc = gmr_fail(GMR_ERR_HIP, "gmr_smplx_joints: %s", hipGetErrorString(e));
  return rc;
}

// Both steps for one clip, host buffers in and out, nothing but the packed frames coming back: poses up, transposed once,
// the body model's joints written as planes, the alignment reading pose and joint planes by joint index -- no joints on
// the host, no gather, no second upload (utils/smpl.py:12-41 + :109-197 in one call).  target_time == NULL: Nout == N.
int gmr_smplx_frames(gmr_smplx_t* h, int N, const double* j_rest, const float* full_pose, const float* transl, int Nout,
                     const double* target_time, double* out) {
  if (!h || N < 1 || Nout < 0 || !j_rest || !full_pose || !transl || !out) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_frames: bad argument");
  if (!target_time && Nout != N) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_frames: without target times Nout must equal N");
  if (target_time && N < 2) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_frames: fps alignment needs at least two source frames");
  if (Nout == 0) return GMR_OK;
  const int C = h->J * 3;
  const size_t nb_pose = (size_t)N * C * sizeof(float);
  gmr::Carve c;
  const size_t o_pose = c.take(nb_pose), o_pose_t = c.take(nb_pose), o_joints_t = c.take(nb_pose), o_tr = c.take((size_t)N * 3 * sizeof(float)),
               o_t = c.take((size_t)Nout * sizeof(double)), o_out = c.take((size_t)Nout * h->sel.nrow * 7 * sizeof(double));
  std::lock_guard<std::mutex> guard(h->mu);
  GMR_NAMED_HIP_TRY("gmr_smplx_frames", h->ws.reserve(c.total(), 4));
  char* ws = h->ws.data();
  hipError_t e = hipSuccess;
  float* d_pose = (float*)(ws + o_pose);
  float* pose_t = (float*)(ws + o_pose_t);
  float* joints_t = (float*)(ws + o_joints_t);
  float* d_tr = (float*)(ws + o_tr);
  double* d_t = (double*)(ws + o_t);
  double* d_o = (double*)(ws + o_out);
  if ((e = hipMemcpy(h->jrest.data(), j_rest, (size_t)h->J * 3 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d_pose, full_pose, (size_t)N * C * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d_tr, transl, (size_t)N * 3 * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess ||
      (target_time && (e = hipMemcpy(d_t, target_time, (size_t)Nout * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess))
    return gmr_fail(GMR_ERR_HIP, "gmr_smplx_frames: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(gmr::rows_planes_kernel<true>, dim3((N + 63) / 64), dim3(256), 64 * (C + 1) * sizeof(float), nullptr, d_pose, N, C, pose_t);
  hipLaunchKernelGGL(gmr::smplx_joints_kernel<true>, dim3((N + SX_BLOCK - 1) / SX_BLOCK), dim3(SX_BLOCK),
                     std::max(h->all.nslot - 1, 1) * 12 * SX_BLOCK * 8, nullptr, h->all, N, (const double*)h->jrest.data(), pose_t, d_tr, joints_t);
  if ((e = hipGetLastError()) != hipSuccess) return gmr_fail(GMR_ERR_HIP, "gmr_smplx_frames: %s", hipGetErrorString(e));
  int rc = smplx_align_launch(h, true, N, -1, pose_t, joints_t, Nout, target_time ? d_t : nullptr, d_o, nullptr);
  if (rc == GMR_OK && (e = hipMemcpy(out, d_o, (size_t)Nout * h->sel.nrow * 7 * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess)
    rc = gmr_fail(GMR_ERR_HIP, "gmr_smplx_frames: %s", hipGetErrorString(e));
  return rc;
}

int gmr_smplx_align(gmr_smplx_t* h, int N, int jstride, const float* full_pose, const float* joints, int Nout,
                    const double* target_time, double* out) {
  if (!h || N < 1 || Nout < 0 || jstride < (h ? h->J : 0) || !full_pose || !joints || !out)
    return gmr_fail(GMR_ERR_ARG, "gmr_smplx_align: bad argument");
  if (Nout == 0) return GMR_OK;
  // only what the walk reads crosses the bus and lies in device memory: the poses of the selection's ancestor closure, in walk
  // order, and the joints of the output rows (for the G1's 14 bodies: 20 + 14 of 55 + 55 joints)
  const gmr::SmplxProg& P = h->sel;
  const size_t np = (size_t)P.n, nr = (size_t)P.nrow;
  std::vector<float> pc((size_t)N * np * 3), jc((size_t)N * nr * 3);
  int rowj[SX_MAX_JOINTS];
  for (int k = 0; k < P.n; k++) if (P.row[k] >= 0) rowj[P.row[k]] = P.joint[k];
  for (int n = 0; n < N; n++) {                       // frame-minor planes [joint][component][frame]
    const float* ps = full_pose + (size_t)n * h->J * 3;
    const float* js = joints + (size_t)n * jstride * 3;
    for (size_t k = 0; k < np; k++) {
      const int j = P.joint[k];
      for (int c = 0; c < 3; c++) pc[(3 * k + c) * (size_t)N + n] = ps[3 * j + c];
    }
    for (size_t r = 0; r < nr; r++) {
      const int j = rowj[r];
      for (int c = 0; c < 3; c++) jc[(3 * r + c) * (size_t)N + n] = js[3 * j + c];
    }
  }
  const size_t nb_pose = pc.size() * sizeof(float), nb_j = jc.size() * sizeof(float);
  const size_t nb_t = (size_t)Nout * sizeof(double), nb_out = (size_t)Nout * h->sel.nrow * 7 * sizeof(double);
  gmr::Carve c;
  const size_t o_pose = c.take(nb_pose), o_j = c.take(nb_j), o_t = c.take(nb_t), o_out = c.take(nb_out);
  std::lock_guard<std::mutex> guard(h->mu);
  GMR_NAMED_HIP_TRY("gmr_smplx_align", h->ws.reserve(c.total(), 4));
  char* ws = h->ws.data();
  hipError_t e = hipSuccess;
  float* d_pose = (float*)(ws + o_pose);
  float* d_j = (float*)(ws + o_j);
  double* d_t = (double*)(ws + o_t);
  double* d_o = (double*)(ws + o_out);
  int rc = GMR_OK;
  if ((e = hipMemcpy(d_pose, pc.data(), nb_pose, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d_j, jc.data(), nb_j, hipMemcpyHostToDevice)) != hipSuccess ||
      (target_time && (e = hipMemcpy(d_t, target_time, nb_t, hipMemcpyHostToDevice)) != hipSuccess))
    rc = gmr_fail(GMR_ERR_HIP, "gmr_smplx_align: %s", hipGetErrorString(e));
  if (rc == GMR_OK) rc = gmr_smplx_align_compact_dev(h, N, d_pose, d_j, Nout, target_time ? d_t : nullptr, d_o, nullptr);
  if (rc == GMR_OK && (e = hipMemcpy(out, d_o, nb_out, hipMemcpyDeviceToHost)) != hipSuccess)
    rc = gmr_fail(GMR_ERR_HIP, "gmr_smplx_align: %s", hipGetErrorString(e));
  return rc;
}

// ---- ragged batches --------------------------------------------------------------------------------------------------------
int gmr_smplx_batch_takes(const gmr_smplx_t* h) { return h && h->batch_ok ? 1 : 0; }

int gmr_smplx_target_times(int N, int Nout, double* out) {
  if (N < 1 || Nout < 0 || (Nout > 0 && !out)) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_target_times: N >= 1, Nout >= 0");
  for (int o = 0; o < Nout; o++) out[o] = gmr::sx_target_time(o, N, Nout);
  return GMR_OK;
}

int gmr_smplx_batch_frames_dev(gmr_smplx_t* h, int nclip, int B, const float* d_root_orient, const float* d_pose_body,
                               const float* d_trans, const int32_t* d_src_start, const int32_t* d_nout, const uint8_t* d_align,
                               const double* d_j_rest, double* const* d_clip_out, void* stream) {
  if (!h) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames_dev: null handle");
  if (!h->batch_ok)
    return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames_dev: the selection reaches beyond the body joints 0 .. %d (root_orient + pose_body)",
                    SX_BODY_JOINTS - 1);
  if (nclip < 0 || B < 0) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames_dev: negative nclip / B");
  if (nclip == 0 || B == 0) return GMR_OK;
  if (!d_root_orient || !d_pose_body || !d_trans || !d_src_start || !d_nout || !d_align || !d_j_rest || !d_clip_out)
    return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames_dev: null buffer");
  const gmr::SmplxProg& P = h->sel;
  // scratch: pose_t f32[P.n][3][Bp], joints_t f32[P.nrow][3][Bp]
  const size_t Bp = ((size_t)B + 63) / 64 * 64;
  const size_t o_pose = 0, o_joints = o_pose + (size_t)P.n * 3 * Bp * sizeof(float), total = o_joints + (size_t)P.nrow * 3 * Bp * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  const auto ws = h->batch_ws.acquire(st, total);              // (held until the last launch below is enqueued)
  GMR_NAMED_HIP_TRY("gmr_smplx_batch_frames_dev", ws.error());
  float* pose_t = (float*)(ws.base() + o_pose);
  float* joints_t = (float*)(ws.base() + o_joints);
  const dim3 grid((unsigned)(Bp / SX_BLOCK)), block(SX_BLOCK);
  hipLaunchKernelGGL(gmr::smplx_batch_joints_kernel, grid, block, h->batch_lds_joints, st, P, nclip, B, Bp, h->batch_nslot_lds,
                     d_root_orient, d_pose_body, d_trans, d_src_start, d_j_rest, pose_t, joints_t);
  hipLaunchKernelGGL(gmr::smplx_batch_align_kernel, grid, block, h->batch_lds_align, st, P, nclip, B, Bp, d_src_start, d_nout, d_align,
                     pose_t, joints_t, d_clip_out);
  GMR_NAMED_HIP_TRY("gmr_smplx_batch_frames_dev", hipGetLastError());
  return GMR_OK;
}

int gmr_smplx_batch_frames(gmr_smplx_t* h, int nclip, int B, const float* root_orient, const float* pose_body, const float* trans,
                           const int32_t* src_start, const int32_t* nout, const uint8_t* align, const double* j_rest, int T,
                           double* human) {
  if (!h) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: null handle");
  if (!h->batch_ok)
    return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: the selection reaches beyond the body joints 0 .. %d (root_orient + pose_body)",
                    SX_BODY_JOINTS - 1);
  if (nclip < 0 || B < 0 || T < 0) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: negative nclip / B / T");
  if (nclip == 0) return B == 0 ? GMR_OK : gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: B = %d frames but no clip", B);
  if (!src_start || !nout || !align || !j_rest || !human || (B > 0 && (!root_orient || !pose_body || !trans)))
    return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: null buffer");
  if (src_start[0] != 0 || src_start[nclip] != B) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: src_start runs from 0 to B = %d", B);
  for (int c = 0; c < nclip; c++) {
    const long long n = (long long)src_start[c + 1] - src_start[c];
    if (n < 0) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: src_start descends at clip %d", c);
    if (align[c] && n < 2) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: clip %d: fps alignment needs at least two source frames", c);
    if (nout[c] < 0 || nout[c] > n || nout[c] > T)
      return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: clip %d: nout = %d of %lld source frames, T = %d", c, nout[c], n, T);
    if (!align[c] && nout[c] != n) return gmr_fail(GMR_ERR_ARG, "gmr_smplx_batch_frames: clip %d: without alignment nout must equal N", c);
  }
  const int nrow = h->sel.nrow, J = h->J;
  const size_t nb_ro = (size_t)B * 3 * 4, nb_pb = (size_t)B * SX_BODY_POSE * 4, nb_seg = (size_t)(nclip + 1) * 4, nb_no = (size_t)nclip * 4,
               nb_al = (size_t)nclip, nb_jr = (size_t)nclip * J * 3 * 8, nb_tab = (size_t)nclip * sizeof(double*),
               nb_out = (size_t)nclip * T * nrow * 7 * 8;
  if (nb_out == 0 || B == 0) { if (nb_out) memset(human, 0, nb_out); return GMR_OK; }
  gmr::Carve c;
  const size_t o_ro = c.take(nb_ro), o_pb = c.take(nb_pb), o_tr = c.take(nb_ro), o_seg = c.take(nb_seg), o_no = c.take(nb_no),
               o_al = c.take(nb_al), o_jr = c.take(nb_jr), o_tab = c.take(nb_tab), o_out = c.take(nb_out);
  std::lock_guard<std::mutex> guard(h->batch_host_mu);
  GMR_NAMED_HIP_TRY("gmr_smplx_batch_frames", h->batch_host_ws.reserve(c.total(), 4));
  char* d = h->batch_host_ws.data();
  hipError_t e = hipSuccess;
  std::vector<double*> tab(nclip);
  for (int c = 0; c < nclip; c++) tab[c] = (double*)(d + o_out) + (size_t)c * T * nrow * 7;
  // frames at or beyond nout[c] come back as zeros (the kernels do not write them)
  if ((e = hipMemset(d + o_out, 0, nb_out)) != hipSuccess ||
      (e = hipMemcpy(d + o_ro, root_orient, nb_ro, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d + o_pb, pose_body, nb_pb, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d + o_tr, trans, nb_ro, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d + o_seg, src_start, nb_seg, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d + o_no, nout, nb_no, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d + o_al, align, nb_al, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d + o_jr, j_rest, nb_jr, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d + o_tab, tab.data(), nb_tab, hipMemcpyHostToDevice)) != hipSuccess)
    return gmr_fail(GMR_ERR_HIP, "gmr_smplx_batch_frames: %s", hipGetErrorString(e));
  int rc = gmr_smplx_batch_frames_dev(h, nclip, B, (const float*)(d + o_ro), (const float*)(d + o_pb), (const float*)(d + o_tr),
                                      (const int32_t*)(d + o_seg), (const int32_t*)(d + o_no), (const uint8_t*)(d + o_al),
                                      (const double*)(d + o_jr), (double* const*)(d + o_tab), nullptr);
  if (rc == GMR_OK && (e = hipMemcpy(human, d + o_out, nb_out, hipMemcpyDeviceToHost)) != hipSuccess)
    rc = gmr_fail(GMR_ERR_HIP, "gmr_smplx_batch_frames: %s", hipGetErrorString(e));
  return rc;
}

}  // extern "C"
