// gmr_motion.hip -- the motion library: what the training-side loader (reference booster_gym/utils/motion_loader.py) does
// with the pkl arrays the dataset drivers write, for many clips at once and on the device.
//
//   motion_fill_kernel    the float32 library arrays from the float64 arrays gmr_postprocess_clips_dev leaves (:72-98: .float()),
//                         root_vel / dof_vel by backward differences (:122-124, :147-149) and root_ang_vel = rotvec(r_i r_{i-1}^-1) / dt
//                         in float64 (:127-143), all inside a clip, frame 0 copying frame 1
//   motion_stats_kernel   per clip and column of root_pos / dof_pos: mean, unbiased std, min, max (:101-113), FP64 two-pass
//   motion_sample_kernel  N (clip, time) queries: loop / clamp, the lerp of five fields and the slerp of the root quaternion
//                         (get_motion_state, :151-247), one group of 16 lanes per query
//
// Semantics that differ from the reference are deliberate and listed in DESIGN.md section 6h: the angular velocity has two modes
// (the reference hands a wxyz-reordered quaternion to a scalar-last constructor, :131-135), a clip of one frame has zero
// velocities (the reference raises), a frame index that leaves the clip is clamped (the reference wraps or raises), and a query
// with a bad clip id or a non-finite time gives NaN and status 1 instead of reading anything.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <new>

#include "../../include/gmr_hip.h"
#include "gmr_device_math.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_motion_sample.h"
#include "gmr_workspace.h"

// float32 arithmetic here mirrors NumPy's / torch's (one rounding per operation: a multiply and an add stay two)
#pragma clang fp contract(off)

namespace gmr {

constexpr int MOTION_ROWS = 64;      // rows per block of the fill kernel
constexpr int MOTION_STAT_ROWS = 4;  // mean, std, min, max

// the clip of row b: the LAST c with seg_start[c] <= b (an empty clip shares its start with the clip after it)
__device__ __forceinline__ int clip_of_row(const int32_t* __restrict__ seg_start, int C, int b) {
  int lo = 0, hi = C - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One column range of the fill: n = nrow * ncol contiguous float64 elements of `src` starting at row b0 -> their float32
// rounding in `dst` and, in `vel`, (x[h] - x[h - 1]) / (float)dt with h = the row itself, or row 1 of the clip for its row 0.
// Row h - 1 is ncol elements back in the same contiguous range: the neighbouring lanes of this or the previous block loaded
// it, so it comes from the cache.  s_hi[r] = h - b0 for row r (so that h and h - 1 never leave the clip), or -1 for a clip
// of one frame (velocity 0).
__device__ __forceinline__ void fill_columns(const double* __restrict__ src, float* __restrict__ dst, float* __restrict__ vel,
                                             int b0, int nrow, int ncol, const int* s_hi, const float* s_dtf) {
  const size_t base = (size_t)b0 * ncol;
  for (int e = threadIdx.x; e < nrow * ncol; e += 256) {
    const int r = e / ncol, c = e - r * ncol;
    const float x = (float)src[base + e];
    dst[base + e] = x;
    if (!vel) continue;
    float v = 0.0f;
    const int h = s_hi[r];
    if (h >= 0) {
      const size_t eh = base + (size_t)((long long)h * ncol + c);
      const float a = (h == r) ? x : (float)src[eh];
      v = __fdiv_rn(a - (float)src[eh - ncol], s_dtf[r]);
    }
    vel[base + e] = v;
  }
}

// Block i owns rows [64 i, 64 i + 64) of the concatenation of all clips.  No load leaves rows [0, B) of the inputs.
__global__ __launch_bounds__(256) void motion_fill_kernel(const MotionArrays A, const double* __restrict__ root_pos,
                                                          const double* __restrict__ root_rot, const double* __restrict__ dof_pos,
                                                          const float* __restrict__ local_body_pos, int reference_angvel) {
  __shared__ int s_hi[MOTION_ROWS];
  __shared__ float s_dtf[MOTION_ROWS];
  __shared__ double s_dt[MOTION_ROWS];
  const int b0 = blockIdx.x * MOTION_ROWS;
  const int nrow = min(A.B - b0, MOTION_ROWS);
  if (threadIdx.x < nrow) {
    const int b = b0 + threadIdx.x;
    const int c = clip_of_row(A.seg_start, A.C, b);
    const int first = A.seg_start[c], T = A.seg_start[c + 1] - first;
    const double dt = 1.0 / A.fps[c];
    s_hi[threadIdx.x] = T < 2 ? -1 : (b == first ? b + 1 : b) - b0;
    s_dt[threadIdx.x] = dt;
    s_dtf[threadIdx.x] = (float)dt;
  }
  __syncthreads();
  fill_columns(root_pos, A.root_pos, A.root_vel, b0, nrow, 3, s_hi, s_dtf);
  fill_columns(root_rot, A.root_rot, nullptr, b0, nrow, 4, s_hi, s_dtf);
  if (A.ndof > 0) fill_columns(dof_pos, A.dof_pos, A.dof_vel, b0, nrow, A.ndof, s_hi, s_dtf);
  // root_ang_vel: one lane per row, float64 from the float32 quaternions (what scipy is handed, :131-143).  scipy normalises
  // what from_quat is given and the product; so3_log then is its as_rotvec (shortest arc: w < 0 flips).
  if (threadIdx.x < nrow) {
    const int r = threadIdx.x, h = s_hi[r];
    float w[3] = {0.0f, 0.0f, 0.0f};
    if (h >= 0) {
      const double* p2 = root_rot + (size_t)(b0 + h) * 4;
      const double* p1 = p2 - 4;
      double a[4], b[4];
#pragma unroll
      for (int k = 0; k < 4; k++) { a[k] = (double)(float)p1[k]; b[k] = (double)(float)p2[k]; }
      // stored xyzw.  World mode reads it as such; reference mode applies the index map [3, 0, 1, 2] and then reads the
      // result as xyzw all the same (:131-135), i.e. (x, y, z, w) <- (w, x, y, z).
      d4 q1, q2;
      if (reference_angvel) { q1 = {a[2], a[3], a[0], a[1]}; q2 = {b[2], b[3], b[0], b[1]}; }
      else { q1 = {a[3], a[0], a[1], a[2]}; q2 = {b[3], b[0], b[1], b[2]}; }
      const double n1 = sqrt(q1.w * q1.w + q1.x * q1.x + q1.y * q1.y + q1.z * q1.z);
      const double n2 = sqrt(q2.w * q2.w + q2.x * q2.x + q2.y * q2.y + q2.z * q2.z);
      q1 = {q1.w / n1, q1.x / n1, q1.y / n1, q1.z / n1};
      q2 = {q2.w / n2, q2.x / n2, q2.y / n2, q2.z / n2};
      d4 d = qmul(q2, qconj(q1));
      const double nd = sqrt(d.w * d.w + d.x * d.x + d.y * d.y + d.z * d.z);
      d = {d.w / nd, d.x / nd, d.y / nd, d.z / nd};
      const d3 rv = so3_log(d);
      const double dt = s_dt[r];
      w[0] = (float)(rv.x / dt); w[1] = (float)(rv.y / dt); w[2] = (float)(rv.z / dt);
    }
    float* o = A.root_ang_vel + (size_t)(b0 + r) * 3;
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
  }
  // local_body_pos: a copy.  64 rows of nbody * 12 B from a 16-byte aligned base start 16-byte aligned.
  if (local_body_pos && A.nbody > 0) {
    const size_t base = (size_t)b0 * A.nbody * 3;
    const int n = nrow * A.nbody * 3, n4 = n >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(local_body_pos + base);
    float4* d4p = reinterpret_cast<float4*>(A.local_body_pos + base);
    for (int e = threadIdx.x; e < n4; e += 256) d4p[e] = s4[e];
    for (int e = (n4 << 2) + threadIdx.x; e < n; e += 256) A.local_body_pos[base + e] = local_body_pos[base + e];
  }
}

// One workgroup per clip, two passes over its float32 rows (the second comes from the L2: the longest LAFAN1 clip is 9 855
// frames x 128 B = 1.3 MB).  A group of G lanes (G = the power of two >= the column count, at most 64) takes one row at a
// time, lane = column, so a wavefront reads 64 / G consecutive rows in one instruction; columns beyond 64 take another sweep.
// Sums are FP64: partial sums per lane, then over the groups of a wavefront by __shfl_xor, then over the four wavefronts in
// LDS.  stats f32 [C][4][3 + ndof]: mean, std (unbiased; NaN for one frame as torch.std gives), min, max; all four rows NaN
// for an empty clip.
__global__ __launch_bounds__(256) void motion_stats_kernel(const MotionArrays A) {
  __shared__ double s_a[4][64], s_mn[4][64], s_mx[4][64];
  const int c = blockIdx.x;
  const int first = A.seg_start[c], T = A.seg_start[c + 1] - first;
  const int ncol = 3 + A.ndof;
  int G = 4;
  while (G < ncol && G < 64) G <<= 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / G, l = lane - g * G;            // group inside the wavefront, column inside the sweep
  const int ngroup = 4 * (64 / G), mygroup = wave * (64 / G) + g;
  float* out = A.stats + (size_t)c * MOTION_STAT_ROWS * ncol;
  if (T == 0) {
    // an empty clip has no statistics: NaN in all four rows (the sums below would leave mean 0 / 0, std sqrt(0 / -1) = -0.0,
    // min +inf, max -inf -- a std that reads as a constant clip).  T is the block's own: the branch is uniform.
    for (int e = threadIdx.x; e < MOTION_STAT_ROWS * ncol; e += 256) out[e] = NAN;
    return;
  }
  for (int col0 = 0; col0 < ncol; col0 += 64) {
    const int col = col0 + l;
    const bool on = col < ncol;
    const float* src = col < 3 ? A.root_pos + (size_t)first * 3 + col : A.dof_pos + (size_t)first * A.ndof + (col - 3);
    const int stride = col < 3 ? 3 : A.ndof;
    double mean = 0.0, var = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int pass = 0; pass < 2; pass++) {
      double acc = 0.0;
      bool nan = false;
      if (on)
        for (int t = mygroup; t < T; t += ngroup) {
          const double x = (double)src[(size_t)t * stride];
          if (pass == 0) {
            acc += x;
            mn = fmin(mn, x); mx = fmax(mx, x);     // (fmin / fmax drop a NaN: it is carried separately, as torch.min does)
            nan |= (x != x);
          } else {
            acc += (x - mean) * (x - mean);
          }
        }
      if (nan) mn = mx = NAN;
      for (int off = G; off < 64; off <<= 1) {
        acc += __shfl_xor(acc, off, 64);
        if (pass == 0) {
          const double omn = __shfl_xor(mn, off, 64), omx = __shfl_xor(mx, off, 64);
          mn = (omn != omn || mn != mn) ? NAN : fmin(mn, omn);
          mx = (omx != omx || mx != mx) ? NAN : fmax(mx, omx);
        }
      }
      __syncthreads();                                // (the previous round's readers are done with s_*)
      if (lane < G) { s_a[wave][l] = acc; s_mn[wave][l] = mn; s_mx[wave][l] = mx; }
      __syncthreads();
      acc = ((s_a[0][l] + s_a[1][l]) + s_a[2][l]) + s_a[3][l];
      if (pass == 0) {
        mean = acc / (double)T;
        for (int w = 0; w < 4; w++) {
          const double omn = s_mn[w][l], omx = s_mx[w][l];
          mn = (omn != omn || mn != mn) ? NAN : fmin(mn, omn);
          mx = (omx != omx || mx != mx) ? NAN : fmax(mx, omx);
        }
      } else {
        var = acc / (double)(T - 1);                  // T == 1: 0 / 0 = NaN
      }
    }
    if (on && threadIdx.x < G) {
      out[0 * ncol + col] = (float)mean;
      out[1 * ncol + col] = (float)sqrt(var);
      out[2 * ncol + col] = (float)mn;
      out[3 * ncol + col] = (float)mx;
    }
  }
}

struct MotionSampleOut {
  float *root_pos, *root_rot, *root_vel, *root_ang_vel, *dof_pos, *dof_vel, *local_body_pos;
  int32_t* status;
};

// 16 lanes per query: they stride over the columns of the two source rows, so the row reads and the output writes of a
// query are contiguous.  The scalars of a query (frame pair, blend, slerp weights) are computed by all 16 lanes alike -- in
// a SIMD that is the same instruction stream as computing them once and sharing them.
__global__ __launch_bounds__(256) void motion_sample_kernel(const MotionArrays A, int N, const int32_t* __restrict__ clip,
                                                            const double* __restrict__ time, int loop, const MotionSampleOut O) {
  const int q = (blockIdx.x * 256 + threadIdx.x) / MOTION_GROUP;
  const int l = threadIdx.x & (MOTION_GROUP - 1);
  if (q >= N) return;
  const int c = clip[q];
  const double tm = time[q];
  const int ndof = A.ndof, nb3 = A.nbody * 3;
  const MotionQuery Q = motion_query(A, c, tm, loop);      // (gmr_motion_sample.h)
  const bool ok = Q.ok;
  if (O.status && l == 0) O.status[q] = ok ? 0 : 1;
  if (!ok) {
    // neutralised: NaN rows, nothing of the library is read
    const float nan = NAN;
    if (l < 3) {
      if (O.root_pos) O.root_pos[(size_t)q * 3 + l] = nan;
      if (O.root_vel) O.root_vel[(size_t)q * 3 + l] = nan;
      if (O.root_ang_vel) O.root_ang_vel[(size_t)q * 3 + l] = nan;
    }
    if (l < 4 && O.root_rot) O.root_rot[(size_t)q * 4 + l] = nan;
    for (int k = l; k < ndof; k += MOTION_GROUP) {
      if (O.dof_pos) O.dof_pos[(size_t)q * ndof + k] = nan;
      if (O.dof_vel) O.dof_vel[(size_t)q * ndof + k] = nan;
    }
    if (O.local_body_pos)
      for (int k = l; k < nb3; k += MOTION_GROUP) O.local_body_pos[(size_t)q * nb3 + k] = nan;
    return;
  }
  const bool same = Q.same;
  const size_t rl = Q.rl, rh = Q.rh;
  const float w0 = Q.w0, w1 = Q.w1;
  if (l < 3) {
    if (O.root_pos) O.root_pos[(size_t)q * 3 + l] = lerp1(A.root_pos, rl * 3 + l, rh * 3 + l, same, w0, w1);
    if (O.root_vel) O.root_vel[(size_t)q * 3 + l] = lerp1(A.root_vel, rl * 3 + l, rh * 3 + l, same, w0, w1);
    if (O.root_ang_vel) O.root_ang_vel[(size_t)q * 3 + l] = lerp1(A.root_ang_vel, rl * 3 + l, rh * 3 + l, same, w0, w1);
  }
  for (int k = l; k < ndof; k += MOTION_GROUP) {
    if (O.dof_pos) O.dof_pos[(size_t)q * ndof + k] = lerp1(A.dof_pos, rl * ndof + k, rh * ndof + k, same, w0, w1);
    if (O.dof_vel) O.dof_vel[(size_t)q * ndof + k] = lerp1(A.dof_vel, rl * ndof + k, rh * ndof + k, same, w0, w1);
  }
  if (O.local_body_pos)
    for (int k = l; k < nb3; k += MOTION_GROUP)
      O.local_body_pos[(size_t)q * nb3 + k] = lerp1(A.local_body_pos, rl * nb3 + k, rh * nb3 + k, same, w0, w1);
  if (O.root_rot && l < 4) O.root_rot[(size_t)q * 4 + l] = slerp1(A.root_rot, rl, rh, l, same, w0, w1);
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "motion library") ---------------------------------------------------------------------------

extern "C" {

int gmr_motion_lib_create(int C, int B, int ndof, int nbody, const int32_t* seg_start, const double* fps, gmr_motion_lib_t** out) {
  if (!out) return gmr_fail(GMR_ERR_ARG, "gmr_motion_lib_create: null out pointer");
  *out = nullptr;
  if (C < 1 || B < 1) return gmr_fail(GMR_ERR_ARG, "a motion library needs at least one clip and one frame (C = %d, B = %d)", C, B);
  if (ndof < 0 || nbody < 0 || ndof > 4096 || nbody > 4096) return gmr_fail(GMR_ERR_ARG, "ndof = %d, nbody = %d out of range", ndof, nbody);
  if (!seg_start || !fps) return gmr_fail(GMR_ERR_ARG, "null seg_start / fps");
  if (seg_start[0] != 0) return gmr_fail(GMR_ERR_ARG, "seg_start[0] = %d, must be 0", seg_start[0]);
  for (int c = 0; c < C; c++) {
    if (seg_start[c + 1] < seg_start[c]) return gmr_fail(GMR_ERR_ARG, "seg_start descends at clip %d (%d -> %d)", c, seg_start[c], seg_start[c + 1]);
    if (!(fps[c] > 0.0) || !std::isfinite(fps[c])) return gmr_fail(GMR_ERR_ARG, "fps[%d] = %g, must be positive and finite", c, fps[c]);
  }
  if (seg_start[C] != B) return gmr_fail(GMR_ERR_ARG, "seg_start[C] = %d, but B = %d", seg_start[C], B);
  if ((long long)B * (ndof > nbody * 3 ? ndof : nbody * 3) > (1LL << 40)) return gmr_fail(GMR_ERR_ARG, "library too large");
  gmr_motion_lib* lib = new (std::nothrow) gmr_motion_lib;
  if (!lib) return gmr_fail(GMR_ERR_ARG, "out of host memory");
  const size_t b = (size_t)B, ncol = 3 + (size_t)ndof;
  const size_t want[GMR_MOTION_FPS + 1] = {b * 12, b * 16, b * ndof * 4, b * nbody * 12, b * 12, b * 12, b * ndof * 4,
                                           (size_t)C * gmr::MOTION_STAT_ROWS * ncol * 4, ((size_t)C + 1) * 4, (size_t)C * 8};
  gmr::Carve c;
  for (int k = 0; k <= GMR_MOTION_FPS; k++) {
    lib->off[k] = c.take(want[k]);
    lib->bytes[k] = want[k];
  }
  hipError_t e = lib->block.reserve(c.total());
  char* d_block = lib->block.data();
  if (e == hipSuccess) e = hipMemcpy(d_block + lib->off[GMR_MOTION_SEG_START], seg_start, want[GMR_MOTION_SEG_START], hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_block + lib->off[GMR_MOTION_FPS], fps, want[GMR_MOTION_FPS], hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    delete lib;
    return gmr_fail(GMR_ERR_HIP, "gmr_motion_lib_create: %s", hipGetErrorString(e));
  }
  auto at = [&](int k) { return (float*)(d_block + lib->off[k]); };
  lib->A = gmr::MotionArrays{C, B, ndof, nbody, (const int32_t*)at(GMR_MOTION_SEG_START), (const double*)at(GMR_MOTION_FPS),
                             at(GMR_MOTION_ROOT_POS), at(GMR_MOTION_ROOT_ROT), at(GMR_MOTION_DOF_POS), at(GMR_MOTION_LOCAL_BODY_POS),
                             at(GMR_MOTION_ROOT_VEL), at(GMR_MOTION_ROOT_ANG_VEL), at(GMR_MOTION_DOF_VEL), at(GMR_MOTION_STATS)};
  *out = lib;
  return GMR_OK;
}

int gmr_motion_lib_destroy(gmr_motion_lib_t* lib) {
  delete lib;
  return GMR_OK;
}

int gmr_motion_lib_fill_dev(gmr_motion_lib_t* lib, const double* d_root_pos, const double* d_root_rot_xyzw, const double* d_dof_pos,
                            const float* d_local_body_pos, int flags, void* stream) {
  if (!lib) return gmr_fail(GMR_ERR_ARG, "null motion library");
  if (flags & ~GMR_MOTION_ANGVEL_REFERENCE) return gmr_fail(GMR_ERR_ARG, "unknown fill flag bits 0x%x", flags);
  if (!d_root_pos || !d_root_rot_xyzw || (lib->A.ndof > 0 && !d_dof_pos)) return gmr_fail(GMR_ERR_ARG, "null input array");
  if (d_local_body_pos && ((uintptr_t)d_local_body_pos & 15)) return gmr_fail(GMR_ERR_ARG, "local_body_pos must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int B = lib->A.B;
  lib->has_body = d_local_body_pos && lib->A.nbody > 0;
  lib->reference_angvel = (flags & GMR_MOTION_ANGVEL_REFERENCE) ? 1 : 0;
  hipLaunchKernelGGL(gmr::motion_fill_kernel, dim3((B + gmr::MOTION_ROWS - 1) / gmr::MOTION_ROWS), dim3(256), 0, st, lib->A, d_root_pos,
                     d_root_rot_xyzw, d_dof_pos, d_local_body_pos, (flags & GMR_MOTION_ANGVEL_REFERENCE) ? 1 : 0);
  GMR_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(gmr::motion_stats_kernel, dim3(lib->A.C), dim3(256), 0, st, lib->A);
  GMR_HIP_TRY(hipGetLastError());
  lib->filled = 1;
  return GMR_OK;
}

int gmr_motion_lib_fill(gmr_motion_lib_t* lib, const double* root_pos, const double* root_rot_xyzw, const double* dof_pos,
                        const float* local_body_pos, int flags) {
  if (!lib) return gmr_fail(GMR_ERR_ARG, "null motion library");
  if (!root_pos || !root_rot_xyzw || (lib->A.ndof > 0 && !dof_pos)) return gmr_fail(GMR_ERR_ARG, "null input array");
  const size_t B = (size_t)lib->A.B;
  gmr::HostStage st;
  const double *d_root_pos, *d_root_rot, *d_dof_pos;
  const float* d_body;
  st.in(d_root_pos, root_pos, B * 24); st.in(d_root_rot, root_rot_xyzw, B * 32);
  st.in(d_dof_pos, dof_pos, B * lib->A.ndof * 8);      // (of no dofs: an address that is never read)
  st.in(d_body, local_body_pos, B * lib->A.nbody * 12);
  GMR_STAGE_TRY(st, upload);
  const int rc = gmr_motion_lib_fill_dev(lib, d_root_pos, d_root_rot, d_dof_pos, d_body, flags, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_lib_array(const gmr_motion_lib_t* lib, int which, void** d_ptr, size_t* bytes) {
  if (!lib) return gmr_fail(GMR_ERR_ARG, "null motion library");
  if (which < 0 || which > GMR_MOTION_FPS) return gmr_fail(GMR_ERR_ARG, "unknown array id %d", which);
  if (which == GMR_MOTION_LOCAL_BODY_POS && lib->filled && !lib->has_body) {
    if (d_ptr) *d_ptr = nullptr;
    if (bytes) *bytes = 0;
    return GMR_OK;
  }
  if (d_ptr) *d_ptr = lib->block.data() + lib->off[which];
  if (bytes) *bytes = lib->bytes[which];
  return GMR_OK;
}

int gmr_motion_sample_dev(const gmr_motion_lib_t* lib, int N, const int32_t* d_clip, const double* d_time, int flags, float* d_root_pos,
                          float* d_root_rot, float* d_root_vel, float* d_root_ang_vel, float* d_dof_pos, float* d_dof_vel,
                          float* d_local_body_pos, int32_t* d_status, void* stream) {
  if (!lib) return gmr_fail(GMR_ERR_ARG, "null motion library");
  if (!lib->filled) return gmr_fail(GMR_ERR_ARG, "the motion library has not been filled");
  if (flags & ~GMR_MOTION_LOOP) return gmr_fail(GMR_ERR_ARG, "unknown sample flag bits 0x%x", flags);
  if (N < 0 || N > (1 << 26)) return gmr_fail(GMR_ERR_ARG, "N = %d out of range", N);
  if (N == 0) return GMR_OK;
  if (!d_clip || !d_time) return gmr_fail(GMR_ERR_ARG, "null clip / time");
  if (d_local_body_pos && !lib->has_body) return gmr_fail(GMR_ERR_ARG, "this library was filled without local_body_pos");
  const gmr::MotionSampleOut O{d_root_pos, d_root_rot, d_root_vel, d_root_ang_vel, d_dof_pos, d_dof_vel, d_local_body_pos, d_status};
  const int per_block = 256 / gmr::MOTION_GROUP;
  hipLaunchKernelGGL(gmr::motion_sample_kernel, dim3((N + per_block - 1) / per_block), dim3(256), 0, (hipStream_t)stream, lib->A, N, d_clip,
                     d_time, (flags & GMR_MOTION_LOOP) ? 1 : 0, O);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

int gmr_motion_sample(const gmr_motion_lib_t* lib, int N, const int32_t* clip, const double* time, int flags, float* root_pos,
                      float* root_rot, float* root_vel, float* root_ang_vel, float* dof_pos, float* dof_vel, float* local_body_pos,
                      int32_t* status) {
  if (!lib) return gmr_fail(GMR_ERR_ARG, "null motion library");
  if (N < 0 || N > (1 << 26)) return gmr_fail(GMR_ERR_ARG, "N = %d out of range", N);
  if (N == 0) return GMR_OK;
  if (!clip || !time) return gmr_fail(GMR_ERR_ARG, "null clip / time");
  const size_t n = (size_t)N, ndof = (size_t)lib->A.ndof, nb3 = (size_t)lib->A.nbody * 3;
  gmr::HostStage st;
  const int32_t* d_clip;
  const double* d_time;
  float *d_root_pos, *d_root_rot, *d_root_vel, *d_root_ang_vel, *d_dof_pos, *d_dof_vel, *d_body;
  int32_t* d_status;
  st.in(d_clip, clip, n * 4); st.in(d_time, time, n * 8);
  st.out(d_root_pos, root_pos, n * 12); st.out(d_root_rot, root_rot, n * 16); st.out(d_root_vel, root_vel, n * 12);
  st.out(d_root_ang_vel, root_ang_vel, n * 12); st.out(d_dof_pos, dof_pos, n * ndof * 4); st.out(d_dof_vel, dof_vel, n * ndof * 4);
  st.out(d_body, local_body_pos, n * nb3 * 4); st.out(d_status, status, n * 4);
  GMR_STAGE_TRY(st, upload);
  const int rc = gmr_motion_sample_dev(lib, N, d_clip, d_time, flags, d_root_pos, d_root_rot, d_root_vel, d_root_ang_vel, d_dof_pos, d_dof_vel,
                                       d_body, d_status, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

}  // extern "C"
