// gmr_tracker_proprio.hip -- the proprioception half of an imitation step on the motion tracker: what
// booster_gym/envs/t1.py::step does between "physics is done" and "the policy gets its next input" -- the body-frame base state and the
// filtered velocities (:463-473), the observation row and the privileged block with sensor noise (:574-603, utils/utils.py:5-30), the
// fourteen regularisation penalties (:622-625, :631-694), the state-based termination (:554-557) and the roll-over of the three last_*
// arrays (:492-494).  The statement of record is tests/proprio_mirror.py.
//
//   tracker_proprio_kernel         ONE launch per environment step, the shape of tracker_targets_kernel (16 lanes per environment, 16
//                                  environments per workgroup).  The root quantities are computed in every lane of the group from one
//                                  broadcast load; the lanes stride over the dofs for the sums and the roll-over (lane l adds the columns
//                                  l, l + 16, .., then group_sum: the order of tracker_step_kernel), then over the W columns of the
//                                  observation row, one Philox call per noisy column.
//   tracker_proprio_reset_kernel   filtered velocities = 0, last_root_vel = root_states[i][7:13] after a reset (:310-313): 16 lanes per
//                                  list entry
//
// The six arrays of ProprioState belong to the tracker and are written by these two kernels only; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <mutex>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_motion_sample.h"
#include "gmr_philox.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/proprio_mirror.py states every line in float32 NumPy
#pragma clang fp contract(off)

namespace gmr {

struct ProprioIn {
  const float *root, *q, *qd, *act, *tau, *extra, *ground;
  const int32_t* steps;
};
struct ProprioOut {
  float *blv, *bav, *pg, *flv, *fav, *obs, *priv, *term, *total;
  int32_t* done;
};

// (V3, pick, rotate_inverse and the sensor noise, tracker_noise at the environment's noise tick: gmr_tracker_dev.h)

__global__ __launch_bounds__(256) void tracker_proprio_kernel(const ProprioTables Pt, const ProprioState St, const ProprioIn X, const ProprioOut O,
                                                              int N, float dtf, uint32_t key0, uint32_t key1, int noise) {
  __shared__ float s_def[TRACKER_MAX_DOF], s_lo[TRACKER_MAX_DOF], s_hi[TRACKER_MAX_DOF], s_vs[TRACKER_MAX_DOF], s_tl[TRACKER_MAX_DOF],
      s_ts[TRACKER_MAX_DOF];
  if (threadIdx.x < TRACKER_MAX_DOF) {
    s_def[threadIdx.x] = Pt.default_pos[threadIdx.x];
    s_lo[threadIdx.x] = Pt.lower[threadIdx.x];
    s_hi[threadIdx.x] = Pt.upper[threadIdx.x];
    s_vs[threadIdx.x] = Pt.vel_soft[threadIdx.x];
    s_tl[threadIdx.x] = Pt.tq_lim[threadIdx.x];
    s_ts[threadIdx.x] = Pt.tq_soft[threadIdx.x];
  }
  __syncthreads();
  const int e = (blockIdx.x * 256 + threadIdx.x) / MOTION_GROUP;
  const int l = threadIdx.x & (MOTION_GROUP - 1);
  if (e >= N) return;
  const int R = Pt.R, C = Pt.C, W = 6 + C + 3 * R;
  const bool draw = noise != 0 && Pt.any_noise != 0;
  const uint32_t tick = St.noise_tick[e];

  // ---- the root, in every lane of the group from one broadcast load (:463-473) ----
  const float* rs = X.root + (size_t)e * 13;
  const float pz = rs[2], qx = rs[3], qy = rs[4], qz = rs[5], qw = rs[6];
  float rv[6];
#pragma unroll
  for (int k = 0; k < 6; k++) rv[k] = rs[7 + k];
  const float h = pz - (X.ground ? X.ground[e] : 0.0f);
  const V3 blv = rotate_inverse(qx, qy, qz, qw, V3{rv[0], rv[1], rv[2]});
  const V3 bav = rotate_inverse(qx, qy, qz, qw, V3{rv[3], rv[4], rv[5]});
  const V3 pg = rotate_inverse(qx, qy, qz, qw, V3{0.0f, 0.0f, -1.0f});
  const float* fl = St.filtered_lin_vel + (size_t)e * 3;
  const float* fa = St.filtered_ang_vel + (size_t)e * 3;
  const V3 flv{blv.x * Pt.fw + fl[0] * Pt.fw1, blv.y * Pt.fw + fl[1] * Pt.fw1, blv.z * Pt.fw + fl[2] * Pt.fw1};
  const V3 fav{bav.x * Pt.fw + fa[0] * Pt.fw1, bav.y * Pt.fw + fa[1] * Pt.fw1, bav.z * Pt.fw + fa[2] * Pt.fw1};
  float root_acc = 0.0f, speed2 = 0.0f;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const float d = __fdiv_rn(St.last_root_vel[(size_t)e * 6 + k] - rv[k], dtf);          // :657
    root_acc = root_acc + d * d;
    speed2 = speed2 + rv[k] * rv[k];                                                     // :554
  }

  // ---- the sums over the dofs and their roll-over: lane l owns the columns l, l + 16, .. (:643-694, :492-493) ----
  float a_tau = 0.0f, a_qd = 0.0f, a_acc = 0.0f, a_rate = 0.0f, a_plim = 0.0f, a_vlim = 0.0f, a_tlim = 0.0f, a_tired = 0.0f, a_pow = 0.0f;
  for (int j = l; j < R; j += MOTION_GROUP) {
    const size_t at = (size_t)e * R + j;
    const float q = X.q[at], qd = X.qd[at];
    a_qd = a_qd + qd * qd;
    const float dd = __fdiv_rn(St.last_dof_vel[at] - qd, dtf);
    a_acc = a_acc + dd * dd;
    a_plim = a_plim + ((q < s_lo[j] || q > s_hi[j]) ? 1.0f : 0.0f);
    float ex = fabsf(qd) - s_vs[j];
    ex = ex < 0.0f ? 0.0f : ex;
    ex = ex > 1.0f ? 1.0f : ex;                                  // (a NaN stays one, as torch.clip leaves it)
    a_vlim = a_vlim + ex;
    if (X.act) {
      const float a = X.act[at], da = St.last_actions[at] - a;
      a_rate = a_rate + da * da;
      St.last_actions[at] = a;
    }
    if (X.tau) {
      const float t = X.tau[at];
      a_tau = a_tau + t * t;
      float over = fabsf(t) - s_ts[j];
      over = over < 0.0f ? 0.0f : over;
      a_tlim = a_tlim + over;
      const float rel = __fdiv_rn(t, s_tl[j]);
      float tired = rel * rel;
      tired = tired > 1.0f ? 1.0f : tired;
      a_tired = a_tired + tired;
      float pw = t * qd;
      pw = pw < 0.0f ? 0.0f : pw;
      a_pow = a_pow + pw;
    }
    St.last_dof_vel[at] = qd;
  }
  const bool terms = O.term || O.total;
  if (terms) {
    a_qd = group_sum(a_qd); a_acc = group_sum(a_acc); a_plim = group_sum(a_plim); a_vlim = group_sum(a_vlim);
    if (X.act) a_rate = group_sum(a_rate);
    if (X.tau) { a_tau = group_sum(a_tau); a_tlim = group_sum(a_tlim); a_tired = group_sum(a_tired); a_pow = group_sum(a_pow); }
    const float dh = h - Pt.height_target;
    const float t[PROPRIO_TERMS] = {flv.z * flv.z, bav.x * bav.x + bav.y * bav.y, pg.x * pg.x + pg.y * pg.y, a_tau, a_qd, a_acc, root_acc,
                                    a_rate, a_plim, a_vlim, a_tlim, a_tired, a_pow, dh * dh};
    float mine = 0.0f, total = 0.0f;
#pragma unroll
    for (int k = 0; k < PROPRIO_TERMS; k++) {
      const bool given = (k == 7) ? X.act != nullptr : ((k == 3 || (k >= 10 && k <= 12)) ? X.tau != nullptr : true);
      if (given && Pt.scale[k] != 0.0f) total = total + Pt.scale[k] * t[k];
      mine = l == k ? t[k] : mine;
    }
    if (O.term && l < PROPRIO_TERMS) O.term[(size_t)e * PROPRIO_TERMS + l] = mine;
    if (O.total && l == 0) O.total[e] = total;
  }

  // ---- the observation row: the lanes stride over its W columns (:580-590) ----
  if (O.obs) {
    float* row = O.obs + (size_t)e * W;
    const int c_q = 6 + C, c_qd = c_q + R, c_a = c_qd + R;
    for (int i = l; i < W; i += MOTION_GROUP) {
      float x;
      int blk = -1;                      // the noise block of the column
      float sc = 1.0f;
      if (i < 3) { x = pick(pg, i); blk = 0; sc = Pt.s_g; }
      else if (i < 6) { x = pick(bav, i - 3); blk = 1; sc = Pt.s_w; }
      else if (i < c_q) { x = X.extra[(size_t)e * C + (i - 6)]; }
      else if (i < c_qd) { x = X.q[(size_t)e * R + (i - c_q)] - s_def[i - c_q]; blk = 2; sc = Pt.s_q; }
      else if (i < c_a) { x = X.qd[(size_t)e * R + (i - c_qd)]; blk = 3; sc = Pt.s_qd; }
      else { x = X.act ? X.act[(size_t)e * R + (i - c_a)] : 0.0f; }
      if (blk >= 0) {
        if (draw && Pt.noise[blk].dist != GMR_NOISE_NONE) x = tracker_noise(x, Pt.noise[blk], (uint32_t)e, tick, (uint32_t)i, DRAW_SENSOR, key0, key1);
        x = x * sc;
      }
      row[i] = x;
    }
  }
  // ---- the privileged block (:596-597): lane k < 4 serves column k, element W + k of the environment ----
  if (O.priv && l < 4) {
    const int blk = l < 3 ? 4 : 5;
    float x = l < 3 ? pick(blv, l) : h;
    if (draw && Pt.noise[blk].dist != GMR_NOISE_NONE) x = tracker_noise(x, Pt.noise[blk], (uint32_t)e, tick, (uint32_t)(W + l), DRAW_SENSOR, key0, key1);
    if (l < 3) x = x * Pt.s_v;
    O.priv[(size_t)e * 4 + l] = x;
  }
  if (l < 3) {
    if (O.blv) O.blv[(size_t)e * 3 + l] = pick(blv, l);
    if (O.bav) O.bav[(size_t)e * 3 + l] = pick(bav, l);
    if (O.pg) O.pg[(size_t)e * 3 + l] = pick(pg, l);
    if (O.flv) O.flv[(size_t)e * 3 + l] = pick(flv, l);
    if (O.fav) O.fav[(size_t)e * 3 + l] = pick(fav, l);
  }
  if (O.done && l == 0) {
    int d = speed2 > Pt.term_vel ? 1 : 0;                                 // :554; a NaN compares false
    if (h < Pt.term_height) d |= 2;                                       // :555
    if (X.steps && X.steps[e] > Pt.max_steps) d |= 4;                     // :556
    O.done[e] = d;
  }
  // ---- the root's share of the roll-over (:468-473, :494).  Every lane of the group has read the old values of these three arrays and
  // the group is part of ONE wavefront, so the stores below follow the loads in program order; the wait makes sure the loads have
  // also returned before a store to the same address is issued (vmcnt(0), the other counters left alone). ----
  __builtin_amdgcn_s_waitcnt(0x0F70);
  if (l < 3) {
    St.filtered_lin_vel[(size_t)e * 3 + l] = pick(flv, l);
    St.filtered_ang_vel[(size_t)e * 3 + l] = pick(fav, l);
  }
  if (l < 6) {
    float v = rv[0];
#pragma unroll
    for (int k = 1; k < 6; k++) v = l == k ? rv[k] : v;
    St.last_root_vel[(size_t)e * 6 + l] = v;
  }
  if (l == 0 && draw) St.noise_tick[e] = tick + 1u;
}

// Entry i of the list (environment i without one): filtered velocities to zero, last_root_vel from the entry's root state
__global__ __launch_bounds__(256) void tracker_proprio_reset_kernel(const TrackerState S, const ProprioState St, int N, int n,
                                                                    const int32_t* __restrict__ ids, const int32_t* __restrict__ mask,
                                                                    const float* __restrict__ root) {
  const int i = (blockIdx.x * 256 + threadIdx.x) / MOTION_GROUP;
  const int l = threadIdx.x & (MOTION_GROUP - 1);
  if (i >= n) return;
  const int e = ids ? ids[i] : i;
  if (tracker_row_skip(S, mask, i, l, e, N)) return;
  if (l < 3) {
    St.filtered_lin_vel[(size_t)e * 3 + l] = 0.0f;
    St.filtered_ang_vel[(size_t)e * 3 + l] = 0.0f;
  }
  if (l < 6) St.last_root_vel[(size_t)e * 6 + l] = root[(size_t)i * 13 + 7 + l];
}

static int proprio_set(const gmr_motion_tracker* t, const ProprioTables& Pt) {
  if (Pt.R == 0) return gmr_fail(GMR_ERR_ARG, "proprio is not set on this tracker (gmr_motion_tracker_set_proprio)");
  if (Pt.R != t->tab.R)
    return gmr_fail(GMR_ERR_ARG, "proprio was set for R = %d robot dofs, the dof map now has %d: call gmr_motion_tracker_set_proprio again", Pt.R,
                    t->tab.R);
  return GMR_OK;
}

// what the entry points copy under the mutex: everything a launch carries
struct ProprioView {
  TrackerState S;
  ProprioTables tab;
  ProprioState st;
};
static ProprioView proprio_view(gmr_motion_tracker* t) { return ProprioView{t->S, t->proprio, t->proprio_state}; }

// the checks of a proprio call that need no device
static int proprio_check(const gmr_motion_tracker* t, const ProprioTables& Pt, const gmr_proprio_in_t* in, int noise, const gmr_proprio_out_t* out) {
  const int rc = proprio_set(t, Pt);
  if (rc != GMR_OK) return rc;
  if (!in || !out) return gmr_fail(GMR_ERR_ARG, "null input / output table");
  if (!in->root_states || !in->dof_pos || !in->dof_vel) return gmr_fail(GMR_ERR_ARG, "null root_states / dof_pos / dof_vel");
  if ((in->extra != nullptr) != (Pt.C > 0))
    return gmr_fail(GMR_ERR_ARG, "extra is needed exactly when extra_cols > 0 (extra_cols = %d, extra %s)", Pt.C, in->extra ? "given" : "null");
  if (noise != 0 && noise != 1) return gmr_fail(GMR_ERR_ARG, "noise = %d, must be 0 or 1", noise);
  return GMR_OK;
}

static int proprio_launch(gmr_motion_tracker* t, const ProprioView& V, const gmr_proprio_in_t* in, int noise, const gmr_proprio_out_t* out,
                          hipStream_t stream) {
  const int rc = proprio_check(t, V.tab, in, noise, out);
  if (rc != GMR_OK) return rc;
  const ProprioIn X{in->root_states, in->dof_pos, in->dof_vel, in->actions, in->mean_torques, in->extra, in->ground, in->episode_steps};
  const ProprioOut O{out->base_lin_vel, out->base_ang_vel, out->projected_gravity, out->filtered_lin_vel, out->filtered_ang_vel,
                     out->obs, out->priv, out->term, out->total, out->done};
  hipLaunchKernelGGL(tracker_proprio_kernel, dim3(row_blocks(t->N, MOTION_GROUP)), dim3(256), 0, stream, V.tab, V.st, X, O, t->N, t->dtf, t->key[0],
                     t->key[1], noise);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

static int proprio_reset_check(const gmr_motion_tracker* t, const ProprioTables& Pt, int n, const void* ids, const void* root) {
  int rc = proprio_set(t, Pt);
  if (rc != GMR_OK) return rc;
  if ((rc = subset_check(t->N, n, ids, "the mask and root_states cover every environment")) != GMR_OK) return rc;
  if (n > 0 && !root) return gmr_fail(GMR_ERR_ARG, "null root_states");
  return GMR_OK;
}

static int proprio_reset_launch(gmr_motion_tracker* t, const ProprioView& V, int n, const int32_t* d_ids, const int32_t* d_mask,
                                const float* d_root, hipStream_t stream) {
  const int rc = proprio_reset_check(t, V.tab, n, d_ids, d_root);
  if (rc != GMR_OK) return rc;
  if (n == 0) return GMR_OK;
  hipLaunchKernelGGL(tracker_proprio_reset_kernel, dim3(row_blocks(n, MOTION_GROUP)), dim3(256), 0, stream, V.S, V.st, t->N, n, d_ids, d_mask, d_root);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker proprioception") ----------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_proprio(gmr_motion_tracker_t* t, const gmr_proprio_config_t* cfg) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!cfg) return gmr_fail(GMR_ERR_ARG, "null configuration");
  if (!cfg->default_dof_pos || !cfg->dof_pos_limits || !cfg->dof_vel_limits || !cfg->torque_limits || !cfg->scales)
    return gmr_fail(GMR_ERR_ARG, "null default_dof_pos / dof_pos_limits / dof_vel_limits / torque_limits / scales");
  if (cfg->extra_cols < 0 || cfg->extra_cols > GMR_PROPRIO_MAX_EXTRA)
    return gmr_fail(GMR_ERR_ARG, "extra_cols = %d outside [0, %d]", cfg->extra_cols, GMR_PROPRIO_MAX_EXTRA);
  if (cfg->max_episode_steps < 0) return gmr_fail(GMR_ERR_ARG, "max_episode_steps = %d is negative", cfg->max_episode_steps);
  if (!std::isfinite(cfg->filter_weight) || !std::isfinite(cfg->soft_dof_pos_limit) || !std::isfinite(cfg->soft_dof_vel_limit) ||
      !std::isfinite(cfg->soft_torque_limit))
    return gmr_fail(GMR_ERR_ARG, "filter_weight and the three soft factors must be finite");
  const float sc[8] = {cfg->scale_gravity, cfg->scale_lin_vel, cfg->scale_ang_vel, cfg->scale_dof_pos, cfg->scale_dof_vel, cfg->base_height_target,
                       cfg->terminate_vel, cfg->terminate_height};
  for (int k = 0; k < 8; k++)
    if (!std::isfinite(sc[k])) return gmr_fail(GMR_ERR_ARG, "the normalisation scales, base_height_target and the termination thresholds must be finite");
  gmr::ProprioTables Pt;
  for (int k = 0; k < GMR_PROPRIO_NOISE_BLOCKS; k++) {
    char name[16];
    snprintf(name, sizeof name, "noise[%d]", k);
    const int rc = gmr::noise_spec(cfg->noise[k], name, &Pt.noise[k]);
    if (rc != GMR_OK) return rc;
    if (Pt.noise[k].dist != GMR_NOISE_NONE) Pt.any_noise = 1;
  }
  for (int k = 0; k < GMR_PROPRIO_TERMS; k++) {
    if (!std::isfinite(cfg->scales[k])) return gmr_fail(GMR_ERR_ARG, "scales[%d] is not finite", k);
    Pt.scale[k] = cfg->scales[k];
  }
  std::lock_guard<std::mutex> g(t->mu);
  const int R = t->tab.R;
  const float half = (float)(0.5 * (1.0 - cfg->soft_dof_pos_limit));          // t1.py:665: a Python number times a float32 tensor
  const float sv = (float)cfg->soft_dof_vel_limit, stq = (float)cfg->soft_torque_limit;
  {
    for (int j = 0; j < R; j++) {
      const float lo = cfg->dof_pos_limits[2 * j], hi = cfg->dof_pos_limits[2 * j + 1];
      if (!std::isfinite(cfg->default_dof_pos[j]) || !std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(cfg->dof_vel_limits[j]) ||
          !std::isfinite(cfg->torque_limits[j]))
        return gmr_fail(GMR_ERR_ARG, "default_dof_pos / dof_pos_limits / dof_vel_limits / torque_limits of dof %d are not finite", j);
      const float span = hi - lo;
      Pt.lower[j] = lo + half * span;                                          // :665-667
      Pt.upper[j] = hi - half * span;                                          // :668-670
      Pt.vel_soft[j] = cfg->dof_vel_limits[j] * sv;                            // :677
      Pt.tq_lim[j] = cfg->torque_limits[j];
      Pt.tq_soft[j] = cfg->torque_limits[j] * stq;                             // :684
      Pt.default_pos[j] = cfg->default_dof_pos[j];
      if (!std::isfinite(Pt.lower[j]) || !std::isfinite(Pt.upper[j]) || !std::isfinite(Pt.vel_soft[j]) || !std::isfinite(Pt.tq_soft[j]))
        return gmr_fail(GMR_ERR_ARG, "the soft limits of dof %d are not finite", j);
      if (Pt.upper[j] < Pt.lower[j]) return gmr_fail(GMR_ERR_ARG, "dof %d: upper = %g < lower = %g", j, (double)Pt.upper[j], (double)Pt.lower[j]);
    }
  }
  Pt.R = R; Pt.C = cfg->extra_cols; Pt.max_steps = cfg->max_episode_steps;
  Pt.fw = (float)cfg->filter_weight; Pt.fw1 = (float)(1.0 - cfg->filter_weight);
  Pt.s_g = cfg->scale_gravity; Pt.s_v = cfg->scale_lin_vel; Pt.s_w = cfg->scale_ang_vel; Pt.s_q = cfg->scale_dof_pos; Pt.s_qd = cfg->scale_dof_vel;
  Pt.height_target = cfg->base_height_target; Pt.term_vel = cfg->terminate_vel; Pt.term_height = cfg->terminate_height;
  const size_t n = (size_t)t->N, nr = n * (size_t)R * 4;
  gmr::Carve cv;
  const size_t o_flv = cv.take(n * 12), o_fav = cv.take(n * 12), o_lrv = cv.take(n * 24), o_la = cv.take(nr), o_ldv = cv.take(nr), o_tick = cv.take(n * 4);
  const int rc = gmr::fresh_block(t->proprio_block, cv);
  if (rc != GMR_OK) return rc;
  char* d = t->proprio_block.data();
  t->proprio = Pt;
  t->proprio_state = gmr::ProprioState{(float*)(d + o_flv), (float*)(d + o_fav), (float*)(d + o_lrv), (float*)(d + o_la), (float*)(d + o_ldv),
                                       (uint32_t*)(d + o_tick)};
  return GMR_OK;
}

int gmr_motion_tracker_proprio_dev(gmr_motion_tracker_t* t, const gmr_proprio_in_t* in, int noise, const gmr_proprio_out_t* out, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::ProprioView V;
  {
    std::lock_guard<std::mutex> g(t->mu);
    V = gmr::proprio_view(t);
  }
  return gmr::proprio_launch(t, V, in, noise, out, (hipStream_t)stream);
}

int gmr_motion_tracker_proprio(gmr_motion_tracker_t* t, const gmr_proprio_in_t* in, int noise, const gmr_proprio_out_t* out) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::ProprioView V = gmr::proprio_view(t);
  int rc = gmr::proprio_check(t, V.tab, in, noise, out);
  if (rc != GMR_OK) return rc;
  const size_t n = (size_t)t->N, r = (size_t)V.tab.R, nr = n * r * 4, w = 6 + (size_t)V.tab.C + 3 * r;
  gmr::HostStage st;
  gmr_proprio_in_t din = {};
  gmr_proprio_out_t dout = {};
  st.in(din.root_states, in->root_states, n * 52); st.in(din.dof_pos, in->dof_pos, nr); st.in(din.dof_vel, in->dof_vel, nr);
  st.in(din.actions, in->actions, nr); st.in(din.mean_torques, in->mean_torques, nr); st.in(din.extra, in->extra, n * (size_t)V.tab.C * 4);
  st.in(din.ground, in->ground, n * 4); st.in(din.episode_steps, in->episode_steps, n * 4);
  st.out(dout.base_lin_vel, out->base_lin_vel, n * 12); st.out(dout.base_ang_vel, out->base_ang_vel, n * 12);
  st.out(dout.projected_gravity, out->projected_gravity, n * 12); st.out(dout.filtered_lin_vel, out->filtered_lin_vel, n * 12);
  st.out(dout.filtered_ang_vel, out->filtered_ang_vel, n * 12); st.out(dout.obs, out->obs, n * w * 4); st.out(dout.priv, out->priv, n * 16);
  st.out(dout.term, out->term, n * GMR_PROPRIO_TERMS * 4); st.out(dout.total, out->total, n * 4); st.out(dout.done, out->done, n * 4);
  GMR_STAGE_TRY(st, upload);
  rc = gmr::proprio_launch(t, V, &din, noise, &dout, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_tracker_proprio_reset_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_mask,
                                         const float* d_root_states, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::ProprioView V;
  {
    std::lock_guard<std::mutex> g(t->mu);
    V = gmr::proprio_view(t);
  }
  return gmr::proprio_reset_launch(t, V, n, d_env_ids, d_mask, d_root_states, (hipStream_t)stream);
}

int gmr_motion_tracker_proprio_reset(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* mask, const float* root_states,
                                     int* ignored) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (ignored) *ignored = 0;
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::ProprioView V = gmr::proprio_view(t);
  int rc = gmr::proprio_reset_check(t, V.tab, n, env_ids, root_states);
  if (rc != GMR_OK) return rc;
  if (n == 0) return GMR_OK;
  const size_t nn = (size_t)n;
  gmr::HostStage st;
  const int32_t *d_ids, *d_mask;
  const float* d_root;
  st.in(d_ids, env_ids, nn * 4); st.in(d_mask, mask, nn * 4); st.in(d_root, root_states, nn * 52);
  GMR_STAGE_TRY(st, upload);
  gmr::IgnoredDelta ig(V.S.ignored, ignored);
  if ((rc = ig.begin()) != GMR_OK) return rc;
  rc = gmr::proprio_reset_launch(t, V, n, d_ids, d_mask, d_root, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return ig.end();
}

int gmr_motion_tracker_proprio_state(gmr_motion_tracker_t* t, float* filtered_lin_vel, float* filtered_ang_vel, float* last_root_vel,
                                     float* last_actions, float* last_dof_vel, uint32_t* noise_tick) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const int rc = gmr::proprio_set(t, t->proprio);
  if (rc != GMR_OK) return rc;
  const gmr::ProprioState& st = t->proprio_state;
  const size_t n = (size_t)t->N, nr = n * (size_t)t->proprio.R * 4;
  return gmr::read_back({{filtered_lin_vel, st.filtered_lin_vel, n * 12}, {filtered_ang_vel, st.filtered_ang_vel, n * 12},
                         {last_root_vel, st.last_root_vel, n * 24}, {last_actions, st.last_actions, nr}, {last_dof_vel, st.last_dof_vel, nr},
                         {noise_tick, st.noise_tick, n * 4}});
}

}  // extern "C"
