// gmr_tracker_control.hip -- the control half of an imitation step on the motion tracker: the joint targets of
// booster_gym/envs/t1_imitation.py:386-415 and the actuator model that the reference runs `decimation` times per step between physics
// substeps (:449-462, t1.py:443-456).  The statement of record is tests/control_mirror.py.
//
//   tracker_targets_kernel   ONE launch per environment step, the sampler's shape (16 lanes per environment, 16 environments per
//                            workgroup): the query of gmr_motion_sample.h at the environment's own (clip, clock), the reference's joint
//                            row in robot order with the lines of tracker_step_kernel, the cosine easing from the default pose over the
//                            first seconds of an episode, the clipped action as a residual.  Reads the tracker's state, writes none of it.
//   tracker_hold_kernel      last_dof_targets[env_ids] = dof_pos[env_ids] after a reset (t1.py:309): 16 lanes per list entry
//   tracker_torques_kernel   ONE launch per physics substep, flat over the N * R elements of the contiguous [N][R] blocks, four elements
//                            per lane through 16-byte accesses and one lane for the tail: actuator delay, PD law, Coulomb friction,
//                            torque clip, running sum and mean.  The environment of an element is needed for delay_steps and the
//                            per-dof tables only: one division per four elements.
//
// The two arrays (held, torque_acc) belong to the tracker and are written by the last two kernels only; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_motion_sample.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/control_mirror.py states every line in float32 NumPy
#pragma clang fp contract(off)

namespace gmr {

// min(max(x, -c), c) as torch.clip does it: a NaN stays one
__device__ __forceinline__ float clip_sym(float x, float c) {
  const float lo = -c;
  x = x < lo ? lo : x;
  return x > c ? c : x;
}

__global__ __launch_bounds__(256) void tracker_targets_kernel(const MotionArrays A, const TrackerState S, const TrackerTables Tb,
                                                              const ControlTables Ct, int N, int loop, float dtf,
                                                              const float* __restrict__ actions, const int32_t* __restrict__ steps,
                                                              float* __restrict__ targets, float* __restrict__ clipped,
                                                              int32_t* __restrict__ status) {
  __shared__ int s_map[TRACKER_MAX_DOF];
  __shared__ float s_def[TRACKER_MAX_DOF], s_pose[TRACKER_MAX_DOF];
  if (threadIdx.x < TRACKER_MAX_DOF) {
    s_map[threadIdx.x] = Tb.map[threadIdx.x];
    s_def[threadIdx.x] = Tb.dof_default[threadIdx.x];
    s_pose[threadIdx.x] = Ct.default_pos[threadIdx.x];
  }
  __syncthreads();
  const int e = (blockIdx.x * 256 + threadIdx.x) / MOTION_GROUP;
  const int l = threadIdx.x & (MOTION_GROUP - 1);
  if (e >= N) return;
  const int R = Tb.R, ndof = A.ndof;
  const MotionQuery Q = motion_query(A, S.clip[e], (double)S.time[e], loop);      // (gmr_motion_sample.h)
  // the phase of the episode (:387-403); s is used in start-up only, where p < 1
  bool startup = false;
  float s = 0.0f;
  if (steps) {
    const float te = (float)steps[e] * dtf;
    startup = te < Ct.startup;
    if (startup) {
      const float p = fminf(fmaxf(__fdiv_rn(te, Ct.startup), 0.0f), 1.0f);
      s = 0.5f * (1.0f - cosf(p * 3.14159f));
    }
  }
  const float gain = startup ? Ct.gain_startup : Ct.gain_run;
  const float nan = NAN;
  for (int j = l; j < R; j += MOTION_GROUP) {
    const size_t at = (size_t)e * R + j;
    float a = 0.0f;
    if (actions) {
      a = clip_sym(actions[at], Ct.clip);                                          // (t1.py:439)
      if (clipped) clipped[at] = a;
    }
    if (!targets) continue;
    float tg = nan;                                                                // a bad assignment: nothing of the library is read
    if (Q.ok) {
      const int m = s_map[j];
      float r = s_def[j];
      if (m >= 0) r = lerp1(A.dof_pos, Q.rl * ndof + m, Q.rh * ndof + m, Q.same, Q.w0, Q.w1);      // the line of tracker_step_kernel
      tg = startup ? s_pose[j] * (1.0f - s) + r * s : r;                           // :406-410
      if (actions) tg = tg + (Ct.action_scale * a) * gain;                        // :414-415, the reference's product order
    }
    targets[at] = tg;
  }
  if (l == 0 && status) status[e] = Q.ok ? 0 : 1;
}

// Entry i of the list (environment i without one): a lane row of 16 copies dof_pos[i][:] into held[e][:] and clears torque_acc[e][:]
__global__ __launch_bounds__(256) void tracker_hold_kernel(const TrackerState S, int N, int R, int n, const int32_t* __restrict__ ids,
                                                           const int32_t* __restrict__ mask, const float* __restrict__ dof_pos,
                                                           float* __restrict__ held, float* __restrict__ acc) {
  const int i = (blockIdx.x * 256 + threadIdx.x) / MOTION_GROUP;
  const int l = threadIdx.x & (MOTION_GROUP - 1);
  if (i >= n) return;
  const int e = ids ? ids[i] : i;
  if (tracker_row_skip(S, mask, i, l, e, N)) return;
  for (int j = l; j < R; j += MOTION_GROUP) {
    held[(size_t)e * R + j] = dof_pos[(size_t)i * R + j];
    acc[(size_t)e * R + j] = 0.0f;
  }
}

struct TorqueArgs {
  const float *targets, *q, *qd;       // [N][R]
  const float *kp, *kd, *fr, *lim;     // kp, kd, fr: [N][R] (per_env) or [R]; fr, lim may be null
  const int32_t* delay;                // [N] or null
  float *held, *acc;                   // [N][R], the tracker's
  float *tau, *mean;                   // [N][R]; mean may be null
  int32_t per_env, substep, M, R, N;
};

// K consecutive elements of a flat [N][R] block from element `at`: one 16-byte access for K = 4 (`at` is a multiple of 4 and the block
// starts on a 16-byte boundary: tracker_torques_launch checks it), one float for K = 1
template <int K>
struct Pack {
  float v[K];
};
template <int K>
__device__ __forceinline__ Pack<K> pack_load(const float* p, size_t at) {
  Pack<K> r;
  if constexpr (K == 4) {
    const float4 x = *reinterpret_cast<const float4*>(p + at);
    r.v[0] = x.x; r.v[1] = x.y; r.v[2] = x.z; r.v[3] = x.w;
  } else {
    r.v[0] = p[at];
  }
  return r;
}
template <int K>
__device__ __forceinline__ void pack_store(float* p, size_t at, const Pack<K>& r) {
  if constexpr (K == 4) *reinterpret_cast<float4*>(p + at) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else p[at] = r.v[0];
}

// the actuator model for the K elements from `at` (all of them inside the block); s_* are the [R] tables in LDS
template <int K>
__device__ __forceinline__ void torque_items(const TorqueArgs& T, size_t at, const float* s_kp, const float* s_kd, const float* s_fr,
                                             const float* s_lim) {
  const uint32_t R = (uint32_t)T.R;
  uint32_t e = (uint32_t)at / R;                     // at < N R <= 2^32 and the last element's index fits 32 bits
  uint32_t j = (uint32_t)at - e * R;
  int col[K];
  bool hit[K], any = false;
  int ds = T.delay ? T.delay[e] : 0;
#pragma unroll
  for (int k = 0; k < K; k++) {
    col[k] = (int)j;
    hit[k] = ds == T.substep;
    any = any || hit[k];
    if (k + 1 < K && ++j == R) {
      j = 0; e++;
      ds = (T.delay && e < (uint32_t)T.N) ? T.delay[e] : 0;
    }
  }
  const Pack<K> q = pack_load<K>(T.q, at), qd = pack_load<K>(T.qd, at);
  Pack<K> h = pack_load<K>(T.held, at), kp, kd, fr, acc, tg;
  if (any) tg = pack_load<K>(T.targets, at);
  if (T.per_env) {
    kp = pack_load<K>(T.kp, at); kd = pack_load<K>(T.kd, at);
    if (T.fr) fr = pack_load<K>(T.fr, at);
  }
  if (T.substep != 0) acc = pack_load<K>(T.acc, at);
  const bool last = T.mean && T.substep == T.M - 1;
  const float Mf = (float)T.M;
  Pack<K> tau, mean;
#pragma unroll
  for (int k = 0; k < K; k++) {
    if (!T.per_env) {
      kp.v[k] = s_kp[col[k]]; kd.v[k] = s_kd[col[k]];
      if (T.fr) fr.v[k] = s_fr[col[k]];
    }
    if (hit[k]) h.v[k] = tg.v[k];                                                // the delay (:451)
    float t = kp.v[k] * (h.v[k] - q.v[k]) - kd.v[k] * qd.v[k];                    // :452
    if (T.fr) {                                                                  // :453, torch.min propagates a NaN, sign(NaN) = 0
      const float a = fabsf(t), f0 = fr.v[k];
      float f = f0 < a ? f0 : a;
      if (f0 != f0) f = f0;
      const float sg = t > 0.0f ? 1.0f : (t < 0.0f ? -1.0f : 0.0f);
      t = t - f * sg;
    }
    if (T.lim) t = clip_sym(t, s_lim[col[k]]);                                   // :454
    tau.v[k] = t;
    acc.v[k] = (T.substep == 0 ? 0.0f : acc.v[k]) + t;                           // :449, :455
    if (last) mean.v[k] = __fdiv_rn(acc.v[k], Mf);                                       // :462
  }
  if (any) pack_store<K>(T.held, at, h);
  pack_store<K>(T.tau, at, tau);
  pack_store<K>(T.acc, at, acc);
  if (last) pack_store<K>(T.mean, at, mean);
}

// VEC: lane g < nvec serves elements [4 g, 4 g + 4), lane nvec the total - 4 nvec < 4 elements of the tail.  Without VEC (a block that
// does not start on a 16-byte boundary) lane g serves element g.  The same arithmetic either way.
template <bool VEC>
__global__ __launch_bounds__(256) void tracker_torques_kernel(const TorqueArgs T, size_t total) {
  __shared__ float s_kp[TRACKER_MAX_DOF], s_kd[TRACKER_MAX_DOF], s_fr[TRACKER_MAX_DOF], s_lim[TRACKER_MAX_DOF];
  if ((int)threadIdx.x < T.R) {
    if (!T.per_env) {
      s_kp[threadIdx.x] = T.kp[threadIdx.x];
      s_kd[threadIdx.x] = T.kd[threadIdx.x];
      if (T.fr) s_fr[threadIdx.x] = T.fr[threadIdx.x];
    }
    if (T.lim) s_lim[threadIdx.x] = T.lim[threadIdx.x];
  }
  __syncthreads();
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if constexpr (VEC) {
    const size_t nvec = total / 4;
    if (g < nvec) {
      torque_items<4>(T, g * 4, s_kp, s_kd, s_fr, s_lim);
    } else if (g == nvec) {
      for (size_t at = nvec * 4; at < total; at++) torque_items<1>(T, at, s_kp, s_kd, s_fr, s_lim);
    }
  } else {
    if (g < total) torque_items<1>(T, g, s_kp, s_kd, s_fr, s_lim);
  }
}

static int control_set(const gmr_motion_tracker* t, const ControlTables& Ct) {
  if (Ct.R == 0) return gmr_fail(GMR_ERR_ARG, "control is not set on this tracker (gmr_motion_tracker_set_control)");
  if (Ct.R != t->tab.R)
    return gmr_fail(GMR_ERR_ARG, "control was set for R = %d robot dofs, the dof map now has %d: call gmr_motion_tracker_set_control again", Ct.R,
                    t->tab.R);
  return GMR_OK;
}

// what the entry points copy under the mutex: everything a launch carries
struct ControlView {
  TrackerTables tab;
  TrackerState S;
  ControlTables ctl;
  float *held, *acc;
};
static ControlView control_view(gmr_motion_tracker* t) { return ControlView{t->tab, t->S, t->control, t->held, t->torque_acc}; }

static int targets_launch(gmr_motion_tracker* t, const ControlView& V, const float* d_actions, const int32_t* d_steps, float* d_targets,
                          float* d_clipped, int32_t* d_status, hipStream_t stream) {
  const int rc = control_set(t, V.ctl);
  if (rc != GMR_OK) return rc;
  if (d_clipped && !d_actions) return gmr_fail(GMR_ERR_ARG, "actions_clipped needs actions");
  if (!d_targets && !d_clipped && !d_status) return GMR_OK;
  hipLaunchKernelGGL(tracker_targets_kernel, dim3(row_blocks(t->N, MOTION_GROUP)), dim3(256), 0, stream, t->lib->A, V.S, V.tab, V.ctl, t->N, t->loop,
                     t->dtf, d_actions, d_steps, d_targets, d_clipped, d_status);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// the checks of a hold call that need no device
static int hold_check(const gmr_motion_tracker* t, const ControlTables& Ct, int n, const void* ids, const void* dof_pos) {
  int rc = control_set(t, Ct);
  if (rc != GMR_OK) return rc;
  if ((rc = subset_check(t->N, n, ids, "the mask and dof_pos cover every environment")) != GMR_OK) return rc;
  if (n > 0 && !dof_pos) return gmr_fail(GMR_ERR_ARG, "null dof_pos");
  return GMR_OK;
}

static int hold_launch(gmr_motion_tracker* t, const ControlView& V, int n, const int32_t* d_ids, const int32_t* d_mask, const float* d_dof_pos,
                       hipStream_t stream) {
  const int rc = hold_check(t, V.ctl, n, d_ids, d_dof_pos);
  if (rc != GMR_OK || n == 0) return rc;
  hipLaunchKernelGGL(tracker_hold_kernel, dim3(row_blocks(n, MOTION_GROUP)), dim3(256), 0, stream, V.S, t->N, V.ctl.R, n, d_ids, d_mask, d_dof_pos,
                     V.held, V.acc);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// the checks of a torques call that need no device
static int torques_check(const gmr_motion_tracker* t, const ControlTables& Ct, int substep, const void* targets, const void* q, const void* qd,
                         const gmr_tracker_actuator_t* act, const void* tau) {
  const int rc = control_set(t, Ct);
  if (rc != GMR_OK) return rc;
  if (substep < 0 || substep >= Ct.M) return gmr_fail(GMR_ERR_ARG, "substep = %d outside [0, %d)", substep, Ct.M);
  if (!targets || !q || !qd || !tau) return gmr_fail(GMR_ERR_ARG, "null dof_targets / dof_pos / dof_vel / dof_torques");
  if (!act || !act->stiffness || !act->damping) return gmr_fail(GMR_ERR_ARG, "null actuator table / stiffness / damping");
  if (act->per_env != 0 && act->per_env != 1) return gmr_fail(GMR_ERR_ARG, "per_env = %d, must be 0 or 1", act->per_env);
  return GMR_OK;
}

static int torques_launch(gmr_motion_tracker* t, const ControlView& V, int substep, const float* d_targets, const float* d_q, const float* d_qd,
                          const gmr_tracker_actuator_t* act, const int32_t* d_delay, float* d_tau, float* d_mean, hipStream_t stream) {
  const int rc = torques_check(t, V.ctl, substep, d_targets, d_q, d_qd, act, d_tau);
  if (rc != GMR_OK) return rc;
  const TorqueArgs T{d_targets, d_q, d_qd, act->stiffness, act->damping, act->friction, act->torque_limit, d_delay, V.held, V.acc,
                     d_tau, d_mean, act->per_env, substep, V.ctl.M, V.ctl.R, t->N};
  const size_t total = (size_t)t->N * (size_t)V.ctl.R;
  bool vec = aligned16(d_targets) && aligned16(d_q) && aligned16(d_qd) && aligned16(d_tau) && aligned16(d_mean) && aligned16(V.held) &&
             aligned16(V.acc);
  if (act->per_env) vec = vec && aligned16(act->stiffness) && aligned16(act->damping) && aligned16(act->friction);
  if (vec) {
    hipLaunchKernelGGL(tracker_torques_kernel<true>, dim3(lane_blocks(total / 4 + 1)), dim3(256), 0, stream, T, total);
  } else {
    hipLaunchKernelGGL(tracker_torques_kernel<false>, dim3(lane_blocks(total)), dim3(256), 0, stream, T, total);
  }
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker control") ---------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_control(gmr_motion_tracker_t* t, const float* default_dof_pos, float action_scale, float clip_actions,
                                   float startup_seconds, float gain_startup, float gain_run, int decimation) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!default_dof_pos) return gmr_fail(GMR_ERR_ARG, "null default_dof_pos");
  if (!std::isfinite(action_scale) || !std::isfinite(gain_startup) || !std::isfinite(gain_run))
    return gmr_fail(GMR_ERR_ARG, "action_scale = %g, gain_startup = %g, gain_run = %g must be finite", (double)action_scale, (double)gain_startup,
                    (double)gain_run);
  if (!(clip_actions > 0.0f)) return gmr_fail(GMR_ERR_ARG, "clip_actions = %g, must be positive (inf: no clipping)", (double)clip_actions);
  if (!(startup_seconds >= 0.0f) || !std::isfinite(startup_seconds))
    return gmr_fail(GMR_ERR_ARG, "startup_seconds = %g, must be finite and not negative", (double)startup_seconds);
  if (decimation < 1 || decimation > gmr::CONTROL_MAX_DECIMATION)
    return gmr_fail(GMR_ERR_ARG, "decimation = %d outside [1, %d]", decimation, gmr::CONTROL_MAX_DECIMATION);
  std::lock_guard<std::mutex> g(t->mu);
  const int R = t->tab.R;
  for (int j = 0; j < R; j++)
    if (!std::isfinite(default_dof_pos[j])) return gmr_fail(GMR_ERR_ARG, "default_dof_pos[%d] is not finite", j);
  const size_t nr = (size_t)t->N * (size_t)R * 4;
  gmr::Carve cv;
  const size_t o_held = cv.take(nr), o_acc = cv.take(nr);
  const int rc = gmr::fresh_block(t->control_block, cv);
  if (rc != GMR_OK) return rc;
  char* d = t->control_block.data();
  gmr::ControlTables Ct;
  Ct.R = R; Ct.M = decimation;
  Ct.action_scale = action_scale; Ct.clip = clip_actions;
  Ct.startup = startup_seconds; Ct.gain_startup = gain_startup; Ct.gain_run = gain_run;
  for (int j = 0; j < R; j++) Ct.default_pos[j] = default_dof_pos[j];
  t->control = Ct;
  t->held = (float*)(d + o_held);
  t->torque_acc = (float*)(d + o_acc);
  return GMR_OK;
}

int gmr_motion_tracker_targets_dev(gmr_motion_tracker_t* t, const float* d_actions, const int32_t* d_episode_steps, float* d_dof_targets,
                                   float* d_actions_clipped, int32_t* d_status, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::ControlView V;
  {
    std::lock_guard<std::mutex> g(t->mu);
    V = gmr::control_view(t);
  }
  return gmr::targets_launch(t, V, d_actions, d_episode_steps, d_dof_targets, d_actions_clipped, d_status, (hipStream_t)stream);
}

int gmr_motion_tracker_targets(gmr_motion_tracker_t* t, const float* actions, const int32_t* episode_steps, float* dof_targets,
                               float* actions_clipped, int32_t* status) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::ControlView V = gmr::control_view(t);
  int rc = gmr::control_set(t, V.ctl);
  if (rc != GMR_OK) return rc;
  if (actions_clipped && !actions) return gmr_fail(GMR_ERR_ARG, "actions_clipped needs actions");
  const size_t n = (size_t)t->N, nr = n * (size_t)V.ctl.R * 4;
  gmr::HostStage st;
  const float* d_actions;
  const int32_t* d_steps;
  float *d_targets, *d_clipped;
  int32_t* d_status;
  st.in(d_actions, actions, nr); st.in(d_steps, episode_steps, n * 4);
  st.out(d_targets, dof_targets, nr); st.out(d_clipped, actions_clipped, nr); st.out(d_status, status, n * 4);
  GMR_STAGE_TRY(st, upload);
  rc = gmr::targets_launch(t, V, d_actions, d_steps, d_targets, d_clipped, d_status, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_tracker_hold_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_mask, const float* d_dof_pos,
                                void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::ControlView V;
  {
    std::lock_guard<std::mutex> g(t->mu);
    V = gmr::control_view(t);
  }
  return gmr::hold_launch(t, V, n, d_env_ids, d_mask, d_dof_pos, (hipStream_t)stream);
}

int gmr_motion_tracker_hold(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* mask, const float* dof_pos, int* ignored) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (ignored) *ignored = 0;
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::ControlView V = gmr::control_view(t);
  int rc = gmr::hold_check(t, V.ctl, n, env_ids, dof_pos);
  if (rc != GMR_OK || n == 0) return rc;
  const size_t nn = (size_t)n, nr = nn * (size_t)V.ctl.R * 4;
  gmr::HostStage st;
  const int32_t *d_ids, *d_mask;
  const float* d_pos;
  st.in(d_ids, env_ids, nn * 4); st.in(d_mask, mask, nn * 4); st.in(d_pos, dof_pos, nr);
  GMR_STAGE_TRY(st, upload);
  gmr::IgnoredDelta ig(V.S.ignored, ignored);
  if ((rc = ig.begin()) != GMR_OK) return rc;
  rc = gmr::hold_launch(t, V, n, d_ids, d_mask, d_pos, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return ig.end();
}

int gmr_motion_tracker_torques_dev(gmr_motion_tracker_t* t, int substep, const float* d_dof_targets, const float* d_dof_pos,
                                   const float* d_dof_vel, const gmr_tracker_actuator_t* act, const int32_t* d_delay_steps,
                                   float* d_dof_torques, float* d_mean_torques, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::ControlView V;
  {
    std::lock_guard<std::mutex> g(t->mu);
    V = gmr::control_view(t);
  }
  return gmr::torques_launch(t, V, substep, d_dof_targets, d_dof_pos, d_dof_vel, act, d_delay_steps, d_dof_torques, d_mean_torques,
                             (hipStream_t)stream);
}

int gmr_motion_tracker_torques(gmr_motion_tracker_t* t, int substep, const float* dof_targets, const float* dof_pos, const float* dof_vel,
                               const gmr_tracker_actuator_t* act, const int32_t* delay_steps, float* dof_torques, float* mean_torques) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::ControlView V = gmr::control_view(t);
  int rc = gmr::torques_check(t, V.ctl, substep, dof_targets, dof_pos, dof_vel, act, dof_torques);
  if (rc != GMR_OK) return rc;
  const size_t n = (size_t)t->N, r = (size_t)V.ctl.R, nr = n * r * 4;
  const size_t gain = act->per_env ? nr : r * 4;
  gmr::HostStage st;
  const float *d_targets, *d_pos, *d_vel;
  gmr_tracker_actuator_t dact = *act;
  const int32_t* d_delay;
  float *d_tau, *d_mean;
  st.in(d_targets, dof_targets, nr); st.in(d_pos, dof_pos, nr); st.in(d_vel, dof_vel, nr); st.in(dact.stiffness, act->stiffness, gain);
  st.in(dact.damping, act->damping, gain); st.in(dact.friction, act->friction, gain); st.in(dact.torque_limit, act->torque_limit, r * 4);
  st.in(d_delay, delay_steps, n * 4);
  st.out(d_tau, dof_torques, nr);
  st.out(d_mean, mean_torques, nr, substep == V.ctl.M - 1);      // (the mean of an environment step: there after its last substep)
  GMR_STAGE_TRY(st, upload);
  rc = gmr::torques_launch(t, V, substep, d_targets, d_pos, d_vel, &dact, d_delay, d_tau, d_mean, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_tracker_control_state(gmr_motion_tracker_t* t, float* held, float* torque_acc) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const int rc = gmr::control_set(t, t->control);
  if (rc != GMR_OK) return rc;
  const size_t nr = (size_t)t->N * (size_t)t->control.R * 4;
  return gmr::read_back({{held, t->held, nr}, {torque_acc, t->torque_acc, nr}});
}

}  // extern "C"
