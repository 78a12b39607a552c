// gmr_tracker.hip -- the motion tracker: what an imitation environment does with the motion library every step (reference
// booster_gym/envs/t1_imitation.py:103-235, 249-309), for N environments and on the device.
//
//   tracker_step_kernel     ONE launch per environment step, the sampler's shape (16 lanes per environment, 16 environments per
//                           workgroup): the query of gmr_motion_sample.h at the environment's own (clip, clock), the reference
//                           rows with the dofs in robot order, the six tracking errors and terms against the simulator's
//                           state, the float32 clock advance and, without loop, the redraw of a finished clip; with anchors
//                           enabled (gmr_tracker_anchor.hip) the four root rows are moved by the environment's anchor first
//   tracker_reset_kernel    _reset_idx (:215-235): one lane per listed environment, one Philox draw each
//   tracker_assign_kernel   (clip, time) set explicitly, one lane per listed environment
//
// The kernels write the tracker's own state and nothing else of either handle: a tracker is single-stream (include/gmr_hip.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <new>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_motion_sample.h"
#include "gmr_philox.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation, as in the sampler whose bits the reference rows reproduce
#pragma clang fp contract(off)

namespace gmr {

// Lanes l < 3 (l < 4) of an environment hold component l of the root rows, as in the sampler; all 16 stride over the robot
// dofs.  Each lane squares what it holds, the six sums of an environment are butterflies over its 16-lane row, and lane 0
// writes the terms, the flags and the new clock.  The dof tables are the same for every environment: they come in as a kernel
// argument and are staged in LDS once per workgroup.
__global__ __launch_bounds__(256) void tracker_step_kernel(const MotionArrays A, const TrackerState S, const TrackerTables Tb, int N, int loop,
                                                           float dtf, uint32_t key0, uint32_t key1, const TrackerSim X, const TrackerOut O) {
  __shared__ int s_map[TRACKER_MAX_DOF];
  __shared__ float s_def[TRACKER_MAX_DOF], s_w[TRACKER_MAX_DOF];
  if (threadIdx.x < TRACKER_MAX_DOF) {
    s_map[threadIdx.x] = Tb.map[threadIdx.x];
    s_def[threadIdx.x] = Tb.dof_default[threadIdx.x];
    s_w[threadIdx.x] = Tb.dof_weight[threadIdx.x];
  }
  __syncthreads();
  const int e = (blockIdx.x * 256 + threadIdx.x) / MOTION_GROUP;
  const int l = threadIdx.x & (MOTION_GROUP - 1);
  if (e >= N) return;
  const int R = Tb.R, ndof = A.ndof;
  const int c = S.clip[e];
  const float tf = S.time[e];
  const MotionQuery Q = motion_query(A, c, (double)tf, loop);      // (gmr_motion_sample.h)
  const bool terms = O.err || O.term || O.total;
  if (!Q.ok) {
    // neutralised: NaN rows, nothing of the library is read, the clock stays
    const float nan = NAN;
    if (l < 3) {
      if (O.ref_root_pos) O.ref_root_pos[(size_t)e * 3 + l] = nan;
      if (O.ref_root_vel) O.ref_root_vel[(size_t)e * 3 + l] = nan;
      if (O.ref_root_ang_vel) O.ref_root_ang_vel[(size_t)e * 3 + l] = nan;
    }
    if (l < 4 && O.ref_root_rot) O.ref_root_rot[(size_t)e * 4 + l] = nan;
    for (int j = l; j < R; j += MOTION_GROUP) {
      if (O.ref_dof_pos) O.ref_dof_pos[(size_t)e * R + j] = nan;
      if (O.ref_dof_vel) O.ref_dof_vel[(size_t)e * R + j] = nan;
    }
    if (l < TRACKER_TERMS) {
      if (O.err) O.err[(size_t)e * TRACKER_TERMS + l] = nan;
      if (O.term) O.term[(size_t)e * TRACKER_TERMS + l] = nan;
    }
    if (l == 0) {
      if (O.total) O.total[e] = nan;
      if (O.status) O.status[e] = 1;
      if (O.finished) O.finished[e] = 0;
    }
    return;
  }
  const bool same = Q.same;
  const size_t rl = Q.rl, rh = Q.rh;
  const float w0 = Q.w0, w1 = Q.w1;
  float acc[TRACKER_TERMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};      // this lane's share of the six sums
  // the anchor of the environment: one branch, the same in every lane of the launch
  const bool anchored = S.anchor_pos != nullptr;
  Anchor An;
  float at = 0.0f;                                                     // component l of its translation
  if (anchored) {
    anchor_turn(S, (size_t)e, An);
    if (l < 3) at = S.anchor_pos[(size_t)e * 3 + l];
  }
  if (l < 3) {
    float p = lerp1(A.root_pos, rl * 3 + l, rh * 3 + l, same, w0, w1);
    float v = lerp1(A.root_vel, rl * 3 + l, rh * 3 + l, same, w0, w1);
    float w = lerp1(A.root_ang_vel, rl * 3 + l, rh * 3 + l, same, w0, w1);
    if (anchored) {      // lanes 0 and 1 swap x and y; the root terms below compare against the anchored rows
      p = anchor_point_lane(An, l, p, at);
      v = anchor_vector_lane(An, l, v);
      w = anchor_vector_lane(An, l, w);
    }
    if (O.ref_root_pos) O.ref_root_pos[(size_t)e * 3 + l] = p;
    if (O.ref_root_vel) O.ref_root_vel[(size_t)e * 3 + l] = v;
    if (O.ref_root_ang_vel) O.ref_root_ang_vel[(size_t)e * 3 + l] = w;
    if (terms) {
      if (X.base_pos) { const float d = X.base_pos[(size_t)e * 3 + l] - p; acc[0] = d * d; }
      if (X.base_lin_vel) { const float d = X.base_lin_vel[(size_t)e * 3 + l] - v; acc[2] = d * d; }
      if (X.base_ang_vel) { const float d = X.base_ang_vel[(size_t)e * 3 + l] - w; acc[3] = d * d; }
    }
  }
  if (l < 4 && (O.ref_root_rot || (terms && X.base_quat))) {
    float q = slerp1(A.root_rot, rl, rh, l, same, w0, w1);
    if (anchored) q = anchor_quat_lane(An, l, q);
    if (O.ref_root_rot) O.ref_root_rot[(size_t)e * 4 + l] = q;
    if (terms && X.base_quat) acc[1] = X.base_quat[(size_t)e * 4 + l] * q;      // <q, q_ref> = the w of conj(q) * q_ref
  }
  for (int j = l; j < R; j += MOTION_GROUP) {
    const int m = s_map[j];
    float p = s_def[j], v = 0.0f;
    if (m >= 0) {
      p = lerp1(A.dof_pos, rl * ndof + m, rh * ndof + m, same, w0, w1);
      v = lerp1(A.dof_vel, rl * ndof + m, rh * ndof + m, same, w0, w1);
    }
    if (O.ref_dof_pos) O.ref_dof_pos[(size_t)e * R + j] = p;
    if (O.ref_dof_vel) O.ref_dof_vel[(size_t)e * R + j] = v;
    if (terms) {
      if (X.dof_pos) { const float d = s_w[j] * (X.dof_pos[(size_t)e * R + j] - p); acc[4] = acc[4] + d * d; }
      if (X.dof_vel) { const float d = s_w[j] * (X.dof_vel[(size_t)e * R + j] - v); acc[5] = acc[5] + d * d; }
    }
  }
  if (terms) {
#pragma unroll
    for (int k = 0; k < TRACKER_TERMS; k++) acc[k] = group_sum(acc[k]);
    if (l == 0) {
      const bool given[TRACKER_TERMS] = {X.base_pos != nullptr, X.base_quat != nullptr, X.base_lin_vel != nullptr,
                                         X.base_ang_vel != nullptr, X.dof_pos != nullptr, X.dof_vel != nullptr};
      float total = 0.0f;
#pragma unroll
      for (int k = 0; k < TRACKER_TERMS; k++) {
        float err = 0.0f, term = 0.0f;
        if (given[k]) {
          if (k == 1) {
            float a = fabsf(acc[1]);
            a = a > 1.0f ? 1.0f : a;                 // (a NaN stays one, as torch.clamp leaves it)
            err = 2.0f * acosf(a);
          } else {
            err = __fsqrt_rn(acc[k]);
          }
          term = expf(-__fdiv_rn(err, Tb.scale[k]));
          if (Tb.weight[k] != 0.0f) total = total + Tb.weight[k] * term;
        }
        if (O.err) O.err[(size_t)e * TRACKER_TERMS + k] = err;
        if (O.term) O.term[(size_t)e * TRACKER_TERMS + k] = term;
      }
      if (O.total) O.total[e] = total;
    }
  }
  if (l == 0) {
    float tn = tf + dtf;                                             // :198, a float32 tensor += dt
    int finished = 0;
    if (!loop && tn >= S.length[e]) {                                // :201-213
      int nc = c;
      tn = tracker_redraw(A, S, key0, key1, e, &nc);
      S.clip[e] = nc;
      S.length[e] = clip_length(A, nc);
      finished = 1;
    }
    S.time[e] = tn;
    if (O.status) O.status[e] = 0;
    if (O.finished) O.finished[e] = finished;
  }
}

__global__ __launch_bounds__(256) void tracker_reset_kernel(const MotionArrays A, const TrackerState S, int N, int n,
                                                            const int32_t* __restrict__ ids, int resample, float lo, float hi, uint32_t key0,
                                                            uint32_t key1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int e = tracker_env(S, ids, i, N);
  if (e < 0) return;
  int c = 0;
  const float u = tracker_draw(A, S, key0, key1, e, resample != 0, &c);
  if (resample) {
    S.clip[e] = c;
    S.length[e] = clip_length(A, c);
  }
  S.time[e] = lo + (hi - lo) * u;          // :232-234
}

// clip == null: clip 0 at time 0 (how a tracker starts)
__global__ __launch_bounds__(256) void tracker_assign_kernel(const MotionArrays A, const TrackerState S, int N, int n,
                                                             const int32_t* __restrict__ ids, const int32_t* __restrict__ clip,
                                                             const float* __restrict__ time) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int e = tracker_env(S, ids, i, N);
  if (e < 0) return;
  const int c = clip ? clip[i] : 0;
  S.clip[e] = c;
  S.time[e] = clip ? time[i] : 0.0f;
  S.length[e] = clip_length(A, c);
}

// the dof tables of a tracker from the caller's host arrays, validated; the terms of T are left as they are
static int tracker_tables(const gmr_motion_lib* lib, int R, const int32_t* dof_map, const float* dof_default, const float* dof_weight,
                          TrackerTables* T) {
  const int ndof = lib->A.ndof;
  if (R < 1 || R > TRACKER_MAX_DOF) return gmr_fail(GMR_ERR_ARG, "R = %d robot dofs outside [1, %d]", R, TRACKER_MAX_DOF);
  if (!dof_map && R != ndof) return gmr_fail(GMR_ERR_ARG, "the identity map needs R = ndof (R = %d, ndof = %d)", R, ndof);
  for (int j = 0; j < R; j++) {
    const int m = dof_map ? dof_map[j] : j;
    if (m < -1 || m >= ndof || m > INT8_MAX) return gmr_fail(GMR_ERR_ARG, "dof_map[%d] = %d outside [-1, %d)", j, m, ndof <= INT8_MAX ? ndof : INT8_MAX + 1);
    if (dof_default && !std::isfinite(dof_default[j])) return gmr_fail(GMR_ERR_ARG, "dof_default[%d] is not finite", j);
    if (dof_weight && !std::isfinite(dof_weight[j])) return gmr_fail(GMR_ERR_ARG, "dof_weight[%d] is not finite", j);
  }
  for (int j = 0; j < TRACKER_MAX_DOF; j++) {
    const bool on = j < R;
    T->map[j] = (int8_t)(on ? (dof_map ? dof_map[j] : j) : -1);
    T->dof_default[j] = on && dof_default ? dof_default[j] : 0.0f;
    T->dof_weight[j] = on ? (dof_weight ? dof_weight[j] : 1.0f) : 0.0f;
  }
  T->R = R;
  return GMR_OK;
}

// what the two step entry points share once the tables are in hand
static int tracker_step_launch(gmr_motion_tracker* t, const TrackerState& S, const TrackerTables& T, const gmr_tracker_sim_t* sim,
                               const gmr_tracker_out_t* out, hipStream_t stream) {
  if (!sim && (out->err || out->term || out->total)) return gmr_fail(GMR_ERR_ARG, "err / term / total need the simulator's state");
  const TrackerSim X = sim ? TrackerSim{sim->base_pos, sim->base_quat, sim->base_lin_vel, sim->base_ang_vel, sim->dof_pos, sim->dof_vel}
                           : TrackerSim{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const TrackerOut O{out->ref_root_pos, out->ref_root_rot, out->ref_root_vel, out->ref_root_ang_vel, out->ref_dof_pos, out->ref_dof_vel,
                     out->err, out->term, out->total, out->status, out->finished};
  hipLaunchKernelGGL(tracker_step_kernel, dim3(row_blocks(t->N, MOTION_GROUP)), dim3(256), 0, stream, t->lib->A, S, T, t->N, t->loop, t->dtf,
                     t->key[0], t->key[1], X, O);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "motion tracker") ----------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_create(const gmr_motion_lib_t* lib, int N, double dt, int flags, int R, const int32_t* dof_map,
                              const float* dof_default, const float* dof_weight, const double* clip_weights, uint64_t seed,
                              gmr_motion_tracker_t** out) {
  if (!out) return gmr_fail(GMR_ERR_ARG, "gmr_motion_tracker_create: null out pointer");
  *out = nullptr;
  if (!lib) return gmr_fail(GMR_ERR_ARG, "null motion library");
  if (!lib->filled) return gmr_fail(GMR_ERR_ARG, "the motion library has not been filled");
  if (flags & ~GMR_MOTION_LOOP) return gmr_fail(GMR_ERR_ARG, "unknown tracker flag bits 0x%x", flags);
  if (N < 1 || N > (1 << 26)) return gmr_fail(GMR_ERR_ARG, "N = %d environments out of range", N);
  if (!std::isfinite(dt) || !std::isfinite((float)dt)) return gmr_fail(GMR_ERR_ARG, "dt = %g is not finite", dt);
  const int C = lib->A.C;
  double sum = 0.0;
  if (clip_weights) {
    for (int c = 0; c < C; c++) {
      if (!(clip_weights[c] >= 0.0) || !std::isfinite(clip_weights[c]))
        return gmr_fail(GMR_ERR_ARG, "clip_weights[%d] = %g, must be finite and not negative", c, clip_weights[c]);
      sum += clip_weights[c];
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) return gmr_fail(GMR_ERR_ARG, "the clip weights sum to %g", sum);
  }
  gmr_motion_tracker* t = new (std::nothrow) gmr_motion_tracker;
  if (!t) return gmr_fail(GMR_ERR_ARG, "out of host memory");
  const int rc = gmr::tracker_tables(lib, R, dof_map, dof_default, dof_weight, &t->tab);
  if (rc != GMR_OK) {
    delete t;
    return rc;
  }
  const float scale[gmr::TRACKER_TERMS] = {0.5f, 0.5f, 2.0f, 1.0f, 1.0f, 0.1f};      // T1Imitation.yaml:327-332
  for (int k = 0; k < gmr::TRACKER_TERMS; k++) { t->tab.scale[k] = scale[k]; t->tab.weight[k] = 1.0f; }
  t->lib = lib; t->N = N; t->loop = (flags & GMR_MOTION_LOOP) ? 1 : 0;
  if (clip_weights) t->clip_w.assign(clip_weights, clip_weights + C);
  t->dtf = (float)dt;
  t->key[0] = (uint32_t)seed; t->key[1] = (uint32_t)(seed >> 32);
  const size_t n = (size_t)N;
  gmr::Carve cv;
  const size_t o_clip = cv.take(n * 4), o_time = cv.take(n * 4), o_len = cv.take(n * 4), o_draws = cv.take(n * 4), o_ign = cv.take(4),
               o_cdf = cv.take(clip_weights ? (size_t)C * 8 : 0);
  hipError_t e = t->block.reserve(cv.total() + 256);
  char* d = t->block.data();
  if (e == hipSuccess) e = hipMemset(d, 0, cv.total());
  if (e == hipSuccess && clip_weights) {
    double* cdf = new (std::nothrow) double[C];
    if (!cdf) {
      delete t;
      return gmr_fail(GMR_ERR_ARG, "out of host memory");
    }
    double before = 0.0;
    for (int c = 0; c < C; c++) { cdf[c] = before / sum; before += clip_weights[c]; }
    e = hipMemcpy(d + o_cdf, cdf, (size_t)C * 8, hipMemcpyHostToDevice);
    delete[] cdf;
  }
  if (e == hipSuccess) {
    t->S = gmr::TrackerState{(int32_t*)(d + o_clip), (float*)(d + o_time), (float*)(d + o_len), (uint32_t*)(d + o_draws), (uint32_t*)(d + o_ign),
                             clip_weights ? (const double*)(d + o_cdf) : nullptr};
    // every environment on clip 0 at time 0; the length of clip 0 is the library's to say
    hipLaunchKernelGGL(gmr::tracker_assign_kernel, dim3(gmr::lane_blocks(N)), dim3(256), 0, nullptr, lib->A, t->S, N, N, nullptr, nullptr, nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    delete t;
    return gmr_fail(GMR_ERR_HIP, "gmr_motion_tracker_create: %s", hipGetErrorString(e));
  }
  *out = t;
  return GMR_OK;
}

int gmr_motion_tracker_destroy(gmr_motion_tracker_t* t) {
  delete t;
  return GMR_OK;
}

int gmr_motion_tracker_set_dof_map(gmr_motion_tracker_t* t, int R, const int32_t* dof_map, const float* dof_default, const float* dof_weight) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  gmr::TrackerTables T = t->tab;
  const int rc = gmr::tracker_tables(t->lib, R, dof_map, dof_default, dof_weight, &T);
  if (rc == GMR_OK) t->tab = T;
  return rc;
}

int gmr_motion_tracker_set_terms(gmr_motion_tracker_t* t, const float* scale, const float* weight) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  for (int k = 0; k < gmr::TRACKER_TERMS; k++) {
    if (scale && (!(scale[k] > 0.0f) || !std::isfinite(scale[k])))
      return gmr_fail(GMR_ERR_ARG, "scale[%d] = %g, must be positive and finite", k, (double)scale[k]);
    if (weight && !std::isfinite(weight[k])) return gmr_fail(GMR_ERR_ARG, "weight[%d] is not finite", k);
  }
  std::lock_guard<std::mutex> g(t->mu);
  for (int k = 0; k < gmr::TRACKER_TERMS; k++) {
    if (scale) t->tab.scale[k] = scale[k];
    if (weight) t->tab.weight[k] = weight[k];
  }
  return GMR_OK;
}

int gmr_motion_tracker_assign_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_clip, const float* d_time,
                                  void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  const int rc = gmr::subset_check(t->N, n, d_env_ids, "every environment is assigned");
  if (rc != GMR_OK || n == 0) return rc;
  if (!d_clip || !d_time) return gmr_fail(GMR_ERR_ARG, "null clip / time");
  hipLaunchKernelGGL(gmr::tracker_assign_kernel, dim3(gmr::lane_blocks(n)), dim3(256), 0, (hipStream_t)stream, t->lib->A, t->S, t->N, n, d_env_ids,
                     d_clip, d_time);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

int gmr_motion_tracker_reset_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, int resample, float lo, float hi, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!d_env_ids) n = t->N;
  const int rc = gmr::subset_check(t->N, n, d_env_ids, nullptr);      // (without a list every environment is reset, whatever n says)
  if (rc != GMR_OK) return rc;
  if (!std::isfinite(lo) || !std::isfinite(hi)) return gmr_fail(GMR_ERR_ARG, "time_offset_range (%g, %g) is not finite", (double)lo, (double)hi);
  if (n == 0) return GMR_OK;
  hipLaunchKernelGGL(gmr::tracker_reset_kernel, dim3(gmr::lane_blocks(n)), dim3(256), 0, (hipStream_t)stream, t->lib->A, t->S, t->N, n, d_env_ids,
                     resample ? 1 : 0, lo, hi, t->key[0], t->key[1]);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

int gmr_motion_tracker_step_dev(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, const gmr_tracker_out_t* out, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!out) return gmr_fail(GMR_ERR_ARG, "null output table");
  gmr::TrackerTables T;
  gmr::TrackerState S;
  {
    std::lock_guard<std::mutex> g(t->mu);
    T = t->tab; S = t->S;
  }
  return gmr::tracker_step_launch(t, S, T, sim, out, (hipStream_t)stream);
}

int gmr_motion_tracker_assign(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* clip, const float* time, int* ignored) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (ignored) *ignored = 0;
  int rc = gmr::subset_check(t->N, n, env_ids, "every environment is assigned");
  if (rc != GMR_OK || n == 0) return rc;
  if (!clip || !time) return gmr_fail(GMR_ERR_ARG, "null clip / time");
  std::lock_guard<std::mutex> g(t->mu);
  const size_t nb = (size_t)n * 4;
  gmr::HostStage st;
  const int32_t *d_ids, *d_clip;
  const float* d_time;
  st.in(d_ids, env_ids, nb); st.in(d_clip, clip, nb); st.in(d_time, time, nb);
  GMR_STAGE_TRY(st, upload);
  gmr::IgnoredDelta ig(t->S.ignored, ignored);
  if ((rc = ig.begin()) == GMR_OK) rc = gmr_motion_tracker_assign_dev(t, n, d_ids, d_clip, d_time, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return ig.end();
}

int gmr_motion_tracker_reset(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, int resample, float lo, float hi, int* ignored) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (ignored) *ignored = 0;
  int rc = gmr::subset_check(t->N, n, env_ids, nullptr);      // (the rule of reset_dev)
  if (rc != GMR_OK || (env_ids && n == 0)) return rc;
  std::lock_guard<std::mutex> g(t->mu);
  gmr::HostStage st;
  const int32_t* d_ids;
  st.in(d_ids, env_ids, (size_t)n * 4);
  GMR_STAGE_TRY(st, upload);
  gmr::IgnoredDelta ig(t->S.ignored, ignored);
  if ((rc = ig.begin()) == GMR_OK) rc = gmr_motion_tracker_reset_dev(t, n, d_ids, resample, lo, hi, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return ig.end();
}

int gmr_motion_tracker_step(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, const gmr_tracker_out_t* out) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!out) return gmr_fail(GMR_ERR_ARG, "null output table");
  std::lock_guard<std::mutex> g(t->mu);
  const size_t n = (size_t)t->N, r = (size_t)t->tab.R;
  gmr::HostStage st;
  gmr_tracker_sim_t dsim = {};
  gmr_tracker_out_t dout = {};
  if (sim) gmr::stage_tracker_sim(st, dsim, *sim, n, r);
  gmr::stage_tracker_out(st, dout, *out, n, r);
  GMR_STAGE_TRY(st, upload);
  const int rc = gmr::tracker_step_launch(t, t->S, t->tab, sim ? &dsim : nullptr, &dout, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_tracker_state(gmr_motion_tracker_t* t, int32_t* clip, float* time, float* length, uint32_t* draws, uint32_t* ignored) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const size_t nb = (size_t)t->N * 4;
  return gmr::read_back({{clip, t->S.clip, nb}, {time, t->S.time, nb}, {length, t->S.length, nb}, {draws, t->S.draws, nb}, {ignored, t->S.ignored, 4}});
}

}  // extern "C"
