// gmr_tracker_commands.hip -- the velocity commands, their curriculum, and the kicks and pushes of an environment step on the motion tracker
// (DESIGN.md section 6s): what booster_gym/envs/t1.py::step still left to the caller after sections 6k-6r -- _resample_commands and
// _resample_curriculum_commands (:362-389, :415-435), _update_curriculum (:391-413), the three command-tracking rewards and survival
// (:606-620), the command columns of the observation row (:584), _kick_robots and _push_robots (:499-527) with the push columns of the
// privileged block (:598-599).  The statement of record is tests/commands_mirror.py.
//
//   tracker_commands_kernel<3>     without a curriculum: ONE launch, one lane per environment -- terms, boundary flag, reset of the resample
//                                  time, resample, outputs
//   tracker_commands_kernel<1>     with a curriculum, first of three: terms, boundary flag, the success stencil into hits (unsigned integer
//                                  atomics), reset of the resample time; the flag bits go to CommandState::carry
//   tracker_commands_grid_kernel   second: ONE workgroup; prob += rate * hits clamped at 1, hits = 0, then cum by chunks of CMD_CHUNK cells
//                                  chained in rising order (the argument of section 6n: non-decreasing, an empty interval for prob = 0)
//   tracker_commands_kernel<2>     third: the draw from cum, resample, outputs
//   tracker_disturb_kernel         ONE launch on a step that kicks, starts or stops a push: 16 lanes per environment, 12 of them an element
//
// The arrays of CommandState belong to the tracker and are written by these kernels only; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_philox.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/commands_mirror.py states every line in float32 NumPy
#pragma clang fp contract(off)

namespace gmr {

struct CmdIn {
  const int32_t *steps, *done;
  const float *lin, *ang;
};
struct CmdOut {
  float *term, *total, *commands, *gait;
  int32_t* flags;
  float* obs;
  int64_t obs_stride;
};
struct DisturbIo {
  float *root, *force, *torque, *obs;
  int64_t force_stride, torque_stride;
};

// one tracking term (:612): expf(-((c - f) * (c - f)) / sigma)
__device__ __forceinline__ float tracking(float c, float f, float sigma) {
  const float d = c - f;
  return expf(__fdiv_rn(-(d * d), sigma));
}

// PHASE bit 0: steps 1 to 4 of the call, bit 1: steps 6 and 7 (include/gmr_hip.h N12)
template <int PHASE>
__global__ __launch_bounds__(256) void tracker_commands_kernel(const CommandTables Ct, const CommandState St, const CmdIn X, const CmdOut O, int N,
                                                               uint32_t key0, uint32_t key1) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  const bool d = X.done != nullptr && X.done[e] != 0;
  const int32_t steps = X.steps[e];
  int32_t rt = St.resample_time[e];
  float c0 = St.commands[(size_t)e * 3], c1 = St.commands[(size_t)e * 3 + 1], c2 = St.commands[(size_t)e * 3 + 2];
  float gf = St.gait_frequency[e];
  int flags = 0;
  if (PHASE & 1) {
    float f0 = 0.0f, f1 = 0.0f, g2 = 0.0f;
    if (X.lin) { f0 = X.lin[(size_t)e * 3]; f1 = X.lin[(size_t)e * 3 + 1]; }
    if (X.ang) g2 = X.ang[(size_t)e * 3 + 2];
    // ---- 1: the terms of the episode's commands (:606-620) ----
    if (O.term || O.total) {
      const float t[CMD_TERMS] = {1.0f, X.lin ? tracking(c0, f0, Ct.sigma) : 0.0f, X.lin ? tracking(c1, f1, Ct.sigma) : 0.0f,
                                  X.ang ? tracking(c2, g2, Ct.sigma) : 0.0f};
      float total = 0.0f;
#pragma unroll
      for (int k = 0; k < CMD_TERMS; k++) {
        const bool given = k == 0 ? true : (k == 3 ? X.ang != nullptr : X.lin != nullptr);
        if (given && Ct.scale[k] != 0.0f) total = total + Ct.scale[k] * t[k];
        if (O.term) O.term[(size_t)e * CMD_TERMS + k] = t[k];
      }
      if (O.total) O.total[e] = total;
    }
    // ---- 2: the boundary, before any reset (:558) ----
    if (steps == rt) flags |= GMR_CMD_BOUNDARY;
    // ---- 3: the curriculum's bookkeeping of an environment that resets (:391-413) ----
    if (Ct.curriculum && d) {
      const bool success = steps > Ct.min_success && fabsf(f0 - c0) < Ct.tol[0] && fabsf(f1 - c1) < Ct.tol[1] && fabsf(g2 - c2) < Ct.tol[2];
      if (success) {
        flags |= GMR_CMD_SUCCESS;
        const int nx = 2 * Ct.L + 1, ny = 2 * Ct.A + 1;
        const int x = St.level[(size_t)e * 2] + Ct.L, y = St.level[(size_t)e * 2 + 1] + Ct.A;
        if (x >= 0 && x < nx && y >= 0 && y < ny) {      // (levels are written by these kernels alone: always true)
          atomicAdd(St.hits + (x * ny + y), 1u);
          if (x > 0) atomicAdd(St.hits + ((x - 1) * ny + y), 1u);
          if (x < nx - 1) atomicAdd(St.hits + ((x + 1) * ny + y), 1u);
          if (y > 0) atomicAdd(St.hits + (x * ny + y - 1), 1u);
          if (y < ny - 1) atomicAdd(St.hits + (x * ny + y + 1), 1u);
        }
      }
    }
    // ---- 4: the reset (:314) ----
    if (d) rt = 0;
    if (!(PHASE & 2)) {
      if (d) St.resample_time[e] = 0;
      St.carry[e] = flags;
    }
  }
  if (PHASE & 2) {
    if (!(PHASE & 1)) flags = St.carry[e];
    const int32_t now = d ? 0 : steps;
    // ---- 6: the resample (:362-389, :415-435) ----
    if (now == rt) {
      const uint32_t n = St.draws[e], key[2] = {key0, key1};
      const uint32_t ca[4] = {(uint32_t)e, n, 0u, DRAW_COMMAND}, cb[4] = {(uint32_t)e, n, 1u, DRAW_COMMAND};
      uint32_t w[4], v[4];
      philox4x32(ca, key, w);
      philox4x32(cb, key, v);
      const float u0 = philox_unit(w[0]), u1 = philox_unit(w[1]), u2 = philox_unit(w[2]), u3 = philox_unit(w[3]), u4 = philox_unit(v[0]);
      if (Ct.curriculum) {
        const int G = Ct.G, ny = 2 * Ct.A + 1;
        const double target = (double)v[2] * 2.3283064365386963e-10 * St.cum[G];
        int lo = 0, hi = G;                        // cum[lo] <= target < cum[hi] throughout
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (St.cum[mid] <= target) lo = mid; else hi = mid;
        }
        const int lin = Ct.order == GMR_CMD_ORDER_REFERENCE ? lo % ny - Ct.L : lo / ny - Ct.L;
        const int ang = Ct.order == GMR_CMD_ORDER_REFERENCE ? lo / ny - Ct.A : lo % ny - Ct.A;
        St.level[(size_t)e * 2] = lin;
        St.level[(size_t)e * 2 + 1] = ang;
        c0 = ((float)lin + (u0 + -0.5f)) * Ct.res[0];
        c1 = ((float)(lin < 0 ? -lin : lin) * (2.0f * u1 + -1.0f)) * Ct.res[1];
        c2 = ((float)ang + (u2 + -0.5f)) * Ct.res[2];
      } else {
        c0 = Ct.span[0] * u0 + Ct.lo[0];
        c1 = Ct.span[1] * u1 + Ct.lo[1];
        c2 = Ct.span[2] * u2 + Ct.lo[2];
      }
      gf = Ct.span[3] * u3 + Ct.lo[3];
      if (u4 < Ct.still) { c0 = 0.0f; c1 = 0.0f; c2 = 0.0f; gf = 0.0f; }
      rt = rt + (Ct.rs_lo + philox_below(v[1], Ct.rs_span));
      flags |= GMR_CMD_RESAMPLED;
      St.draws[e] = n + 1u;
      St.commands[(size_t)e * 3] = c0; St.commands[(size_t)e * 3 + 1] = c1; St.commands[(size_t)e * 3 + 2] = c2;
      St.gait_frequency[e] = gf;
    }
    if ((PHASE & 1) ? (d || (flags & GMR_CMD_RESAMPLED)) : (flags & GMR_CMD_RESAMPLED)) St.resample_time[e] = rt;
    // ---- 7: the outputs ----
    if (O.commands) { O.commands[(size_t)e * 3] = c0; O.commands[(size_t)e * 3 + 1] = c1; O.commands[(size_t)e * 3 + 2] = c2; }
    if (O.gait) O.gait[e] = gf;
    if (O.flags) O.flags[e] = flags;
    if (O.obs) {
      float* row = O.obs + (int64_t)e * O.obs_stride;
      row[0] = c0 * Ct.obs_scale[0]; row[1] = c1 * Ct.obs_scale[1]; row[2] = c2 * Ct.obs_scale[2];
    }
  }
}

// step 5: ONE workgroup.  Lane k owns the cells CMD_CHUNK k .. CMD_CHUNK k + 7 of the flattened grid.
__global__ __launch_bounds__(256) void tracker_commands_grid_kernel(const CommandTables Ct, const CommandState St) {
  __shared__ double s_sum[256], s_base[256];
  const int k = threadIdx.x, G = Ct.G, nch = (G + CMD_CHUNK - 1) / CMD_CHUNK;      // nch <= 211
  double s[CMD_CHUNK];            // s[i]: the sum of the chunk's cells before cell i
  double run = 0.0;
#pragma unroll
  for (int i = 0; i < CMD_CHUNK; i++) {
    const int g = k * CMD_CHUNK + i;
    s[i] = run;
    if (g < G) {
      float p = St.prob[g] + Ct.rate * (float)St.hits[g];
      p = p > 1.0f ? 1.0f : p;                                                     // :413
      St.prob[g] = p;
      St.hits[g] = 0u;
      run = run + (double)p;
    }
  }
  s_sum[k] = run;
  __syncthreads();
  if (k == 0) {
    double b = 0.0;
    for (int c = 0; c < nch; c++) {
      s_base[c] = b;
      b = b + s_sum[c];
    }
  }
  __syncthreads();
  if (k >= nch) return;
  const double b = s_base[k];
#pragma unroll
  for (int i = 0; i < CMD_CHUNK; i++) {
    const int g = k * CMD_CHUNK + i;
    if (g < G) St.cum[g] = b + s[i];
  }
  if (k == nch - 1) St.cum[G] = b + run;
}

// (the noise of element i of environment e at common_step: tracker_noise of gmr_tracker_dev.h in the domain of the kicks and pushes)
__global__ __launch_bounds__(256) void tracker_disturb_kernel(const DisturbTables Dt, const DisturbIo io, int N, uint32_t step, int act,
                                                              uint32_t key0, uint32_t key1) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t e = idx >> 4;
  const int i = (int)(idx & 15);
  if (e >= N || i >= 12) return;
  if (i < 6) {                                       // the kick (:502-503)
    if (!(act & GMR_DISTURB_KICK)) return;
    const ProprioNoise& S = Dt.spec[i < 3 ? 0 : 1];
    if (S.dist == GMR_NOISE_NONE) return;
    float* p = io.root + e * 13 + 7 + i;
    *p = tracker_noise(*p, S, (uint32_t)e, step, (uint32_t)i, DRAW_DISTURB, key0, key1);
    return;
  }
  if (!(act & (GMR_DISTURB_PUSH_START | GMR_DISTURB_PUSH_STOP))) return;
  const bool torque = i >= 9;
  const int k = i - (torque ? 9 : 6);
  const ProprioNoise& S = Dt.spec[torque ? 3 : 2];
  float v = 0.0f;                                    // the push (:509-521): the randomisation of zero, or zero
  if ((act & GMR_DISTURB_PUSH_START) && S.dist != GMR_NOISE_NONE) v = tracker_noise(0.0f, S, (uint32_t)e, step, (uint32_t)i, DRAW_DISTURB, key0, key1);
  float* dst = torque ? io.torque : io.force;
  if (dst) dst[e * (torque ? io.torque_stride : io.force_stride) + k] = v;
  if (io.obs) io.obs[e * 6 + (i - 6)] = v * (torque ? Dt.s_torque : Dt.s_force);      // :598-599
}

// what the entry points copy under the mutex: everything a launch carries
struct CommandView {
  CommandTables tab;
  CommandState st;
};

static int commands_check(const CommandTables& Ct, const gmr_commands_in_t* in, const gmr_commands_out_t* out) {
  if (!Ct.on) return gmr_fail(GMR_ERR_ARG, "commands are not set on this tracker (gmr_motion_tracker_set_commands)");
  if (!in || !out) return gmr_fail(GMR_ERR_ARG, "null input / output table");
  if (!in->episode_steps) return gmr_fail(GMR_ERR_ARG, "null episode_steps");
  if (Ct.curriculum && (!in->lin_vel || !in->ang_vel)) return gmr_fail(GMR_ERR_ARG, "the curriculum needs lin_vel and ang_vel (the filtered velocities)");
  if (out->cmd_obs && out->cmd_obs_stride < 3) return gmr_fail(GMR_ERR_ARG, "cmd_obs_stride = %lld, at least 3 floats needed", (long long)out->cmd_obs_stride);
  return GMR_OK;
}

static int commands_launch(gmr_motion_tracker* t, const CommandView& V, const gmr_commands_in_t* in, const gmr_commands_out_t* out, hipStream_t stream) {
  const int rc = commands_check(V.tab, in, out);
  if (rc != GMR_OK) return rc;
  const CmdIn X{in->episode_steps, in->done, in->lin_vel, in->ang_vel};
  const CmdOut O{out->term, out->total, out->commands, out->gait_frequency, out->flags, out->cmd_obs, out->cmd_obs_stride};
  const dim3 grid(lane_blocks(t->N)), block(256);
  if (!V.tab.curriculum) {
    hipLaunchKernelGGL(tracker_commands_kernel<3>, grid, block, 0, stream, V.tab, V.st, X, O, t->N, t->key[0], t->key[1]);
  } else {
    hipLaunchKernelGGL(tracker_commands_kernel<1>, grid, block, 0, stream, V.tab, V.st, X, O, t->N, t->key[0], t->key[1]);
    hipLaunchKernelGGL(tracker_commands_grid_kernel, dim3(1), block, 0, stream, V.tab, V.st);
    hipLaunchKernelGGL(tracker_commands_kernel<2>, grid, block, 0, stream, V.tab, V.st, X, O, t->N, t->key[0], t->key[1]);
  }
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// what common_step does: the modulo rule of t1.py:501, :508, :517
static int disturb_actions(const DisturbTables& Dt, uint32_t step) {
  int act = 0;
  if (step % (uint32_t)Dt.kick_every == 0u) act |= GMR_DISTURB_KICK;
  if (step % (uint32_t)Dt.push_every == 0u) act |= GMR_DISTURB_PUSH_START;
  else if (step % (uint32_t)Dt.push_every == (uint32_t)Dt.push_duration) act |= GMR_DISTURB_PUSH_STOP;
  return act;
}

static int disturb_check(const DisturbTables& Dt, const gmr_disturb_io_t* io, int act) {
  if (!Dt.on) return gmr_fail(GMR_ERR_ARG, "disturbances are not set on this tracker (gmr_motion_tracker_set_disturbances)");
  if (!io) return gmr_fail(GMR_ERR_ARG, "null io table");
  if ((act & GMR_DISTURB_KICK) && !io->root_states) return gmr_fail(GMR_ERR_ARG, "a kick step needs root_states");
  if ((io->push_force && io->push_force_stride < 3) || (io->push_torque && io->push_torque_stride < 3))
    return gmr_fail(GMR_ERR_ARG, "push strides (%lld, %lld): at least 3 floats needed", (long long)io->push_force_stride, (long long)io->push_torque_stride);
  return GMR_OK;
}

// the launch of a step that acts (act != 0, checked)
static int disturb_launch(gmr_motion_tracker* t, const DisturbTables& Dt, uint32_t step, int act, const gmr_disturb_io_t* io, hipStream_t stream) {
  const DisturbIo D{io->root_states, io->push_force, io->push_torque, io->push_obs, io->push_force_stride, io->push_torque_stride};
  hipLaunchKernelGGL(tracker_disturb_kernel, dim3(lane_blocks((int64_t)t->N * 16)), dim3(256), 0, stream, Dt, D, t->N, step, act, t->key[0], t->key[1]);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker commands") -----------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_commands(gmr_motion_tracker_t* t, const gmr_commands_config_t* cfg, int keep_state) {
  using gmr::fits;
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!cfg) return gmr_fail(GMR_ERR_ARG, "null configuration");
  if (keep_state != 0 && keep_state != 1) return gmr_fail(GMR_ERR_ARG, "keep_state = %d, must be 0 or 1", keep_state);
  gmr::CommandTables Ct;
  const double* rng[4] = {cfg->lin_vel_x, cfg->lin_vel_y, cfg->ang_vel_yaw, cfg->gait_frequency};
  static const char* const names[4] = {"lin_vel_x", "lin_vel_y", "ang_vel_yaw", "gait_frequency"};
  for (int k = 0; k < 4; k++) {
    const double lo = rng[k][0], hi = rng[k][1];
    if (!fits(lo) || !fits(hi) || !fits(hi - lo)) return gmr_fail(GMR_ERR_ARG, "%s: range (%g, %g) is not finite in float32", names[k], lo, hi);
    if (hi < lo) return gmr_fail(GMR_ERR_ARG, "%s: upper = %g < lower = %g", names[k], hi, lo);
    Ct.lo[k] = (float)lo;
    Ct.span[k] = (float)(hi - lo);
  }
  if (!(cfg->still_proportion >= 0.0 && cfg->still_proportion <= 1.0)) return gmr_fail(GMR_ERR_ARG, "still_proportion = %g outside [0, 1]", cfg->still_proportion);
  if (!fits(cfg->tracking_sigma) || !((float)cfg->tracking_sigma > 0.0f)) return gmr_fail(GMR_ERR_ARG, "tracking_sigma = %g must be positive and finite", cfg->tracking_sigma);
  if (cfg->resample_steps[0] < 1 || cfg->resample_steps[1] <= cfg->resample_steps[0])
    return gmr_fail(GMR_ERR_ARG, "resample_steps = (%d, %d): hi > lo >= 1 needed", cfg->resample_steps[0], cfg->resample_steps[1]);
  for (int k = 0; k < GMR_CMD_TERMS; k++) {
    if (!std::isfinite(cfg->scales[k])) return gmr_fail(GMR_ERR_ARG, "scales[%d] is not finite", k);
    Ct.scale[k] = cfg->scales[k];
  }
  for (int k = 0; k < 3; k++) {
    if (!std::isfinite(cfg->obs_scale[k])) return gmr_fail(GMR_ERR_ARG, "obs_scale[%d] is not finite", k);
    Ct.obs_scale[k] = cfg->obs_scale[k];
  }
  Ct.still = (float)cfg->still_proportion;
  Ct.sigma = (float)cfg->tracking_sigma;
  Ct.rs_lo = cfg->resample_steps[0];
  Ct.rs_span = cfg->resample_steps[1] - cfg->resample_steps[0];
  if (cfg->curriculum != 0 && cfg->curriculum != 1) return gmr_fail(GMR_ERR_ARG, "curriculum = %d, must be 0 or 1", cfg->curriculum);
  if (cfg->curriculum) {
    const int L = cfg->lin_vel_levels, A = cfg->ang_vel_levels;
    if (L < 0 || L > GMR_CMD_MAX_LEVELS || A < 0 || A > GMR_CMD_MAX_LEVELS)
      return gmr_fail(GMR_ERR_ARG, "lin_vel_levels = %d, ang_vel_levels = %d outside [0, %d]", L, A, GMR_CMD_MAX_LEVELS);
    if (cfg->index_order != GMR_CMD_ORDER_GRID && cfg->index_order != GMR_CMD_ORDER_REFERENCE) return gmr_fail(GMR_ERR_ARG, "index_order = %d", cfg->index_order);
    if (cfg->index_order == GMR_CMD_ORDER_REFERENCE && L != A)
      return gmr_fail(GMR_ERR_ARG, "index_order \"reference\" transposes the grid and needs lin_vel_levels == ang_vel_levels (%d, %d)", L, A);
    if (!fits(cfg->update_rate) || cfg->update_rate < 0.0) return gmr_fail(GMR_ERR_ARG, "update_rate = %g must be finite and not negative", cfg->update_rate);
    if (cfg->min_success_steps < 0) return gmr_fail(GMR_ERR_ARG, "min_success_steps = %d is negative", cfg->min_success_steps);
    for (int k = 0; k < 3; k++) {
      if (!fits(cfg->toler[k]) || !fits(cfg->resolution[k])) return gmr_fail(GMR_ERR_ARG, "toler[%d] / resolution[%d] is not finite in float32", k, k);
      Ct.tol[k] = (float)cfg->toler[k];
      Ct.res[k] = (float)cfg->resolution[k];
    }
    Ct.curriculum = 1; Ct.L = L; Ct.A = A; Ct.G = (2 * L + 1) * (2 * A + 1);
    Ct.order = cfg->index_order; Ct.min_success = cfg->min_success_steps; Ct.rate = (float)cfg->update_rate;
  }
  Ct.on = 1;
  std::lock_guard<std::mutex> g(t->mu);
  if (keep_state) {
    const gmr::CommandTables& old = t->commands;
    if (!old.on) return gmr_fail(GMR_ERR_ARG, "keep_state: commands were never set on this tracker");
    if (old.curriculum != Ct.curriculum || old.L != Ct.L || old.A != Ct.A)
      return gmr_fail(GMR_ERR_ARG, "keep_state: the curriculum and its levels must stay as they are (curriculum %d, L %d, A %d)", old.curriculum, old.L, old.A);
    t->commands = Ct;
    return GMR_OK;
  }
  const size_t n = (size_t)t->N, G = (size_t)Ct.G;
  gmr::Carve cv;
  const size_t o_cmd = cv.take(n * 12), o_gait = cv.take(n * 4), o_rt = cv.take(n * 4), o_draws = cv.take(n * 4), o_carry = cv.take(n * 4);
  const size_t o_level = cv.take(Ct.curriculum ? n * 8 : 0), o_prob = cv.take(G * 4), o_hits = cv.take(G * 4), o_cum = cv.take(Ct.curriculum ? (G + 1) * 8 : 0);
  const int rc = gmr::fresh_block(t->command_block, cv);
  if (rc != GMR_OK) return rc;
  char* d = t->command_block.data();
  gmr::CommandState st;
  st.commands = (float*)(d + o_cmd); st.gait_frequency = (float*)(d + o_gait); st.resample_time = (int32_t*)(d + o_rt);
  st.draws = (uint32_t*)(d + o_draws); st.carry = (int32_t*)(d + o_carry);
  if (Ct.curriculum) {
    st.level = (int32_t*)(d + o_level); st.prob = (float*)(d + o_prob); st.hits = (uint32_t*)(d + o_hits); st.cum = (double*)(d + o_cum);
    const float one = 1.0f;                          // :245-251: the centre cell
    GMR_HIP_TRY(hipMemcpy(st.prob + ((size_t)Ct.L * (2 * Ct.A + 1) + Ct.A), &one, 4, hipMemcpyHostToDevice));
    GMR_HIP_TRY(hipDeviceSynchronize());
  }
  t->commands = Ct;
  t->command_state = st;
  return GMR_OK;
}

int gmr_motion_tracker_commands_dev(gmr_motion_tracker_t* t, const gmr_commands_in_t* in, const gmr_commands_out_t* out, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::CommandView V;
  {
    std::lock_guard<std::mutex> g(t->mu);
    V = gmr::CommandView{t->commands, t->command_state};
  }
  return gmr::commands_launch(t, V, in, out, (hipStream_t)stream);
}

int gmr_motion_tracker_commands(gmr_motion_tracker_t* t, const gmr_commands_in_t* in, const gmr_commands_out_t* out) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::CommandView V{t->commands, t->command_state};
  int rc = gmr::commands_check(V.tab, in, out);
  if (rc != GMR_OK) return rc;
  const size_t n = (size_t)t->N;
  const size_t obs_bytes = out->cmd_obs ? ((n - 1) * (size_t)out->cmd_obs_stride + 3) * 4 : 0;
  gmr::HostStage st;
  gmr_commands_in_t din = {};
  gmr_commands_out_t dout = {};
  st.in(din.episode_steps, in->episode_steps, n * 4); st.in(din.done, in->done, n * 4);
  st.in(din.lin_vel, in->lin_vel, n * 12); st.in(din.ang_vel, in->ang_vel, n * 12);
  st.out(dout.term, out->term, n * GMR_CMD_TERMS * 4); st.out(dout.total, out->total, n * 4); st.out(dout.commands, out->commands, n * 12);
  st.out(dout.gait_frequency, out->gait_frequency, n * 4); st.out(dout.flags, out->flags, n * 4);
  st.in(dout.cmd_obs, out->cmd_obs, obs_bytes);      // rows of the caller's: in, and copied back below
  dout.cmd_obs_stride = out->cmd_obs_stride;
  GMR_STAGE_TRY(st, upload);
  rc = gmr::commands_launch(t, V, &din, &dout, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  if (out->cmd_obs) GMR_HIP_TRY(hipMemcpy(out->cmd_obs, dout.cmd_obs, obs_bytes, hipMemcpyDeviceToHost));
  return GMR_OK;
}

int gmr_motion_tracker_command_state(gmr_motion_tracker_t* t, float* commands, float* gait_frequency, int32_t* cmd_resample_time,
                                     uint32_t* cmd_draws, int32_t* env_level, float* curriculum_prob, uint32_t* hits, double* cum) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::CommandTables& Ct = t->commands;
  if (!Ct.on) return gmr_fail(GMR_ERR_ARG, "commands are not set on this tracker (gmr_motion_tracker_set_commands)");
  if (!Ct.curriculum && (env_level || curriculum_prob || hits || cum))
    return gmr_fail(GMR_ERR_ARG, "env_level / curriculum_prob / hits / cum exist with a curriculum only");
  const gmr::CommandState& st = t->command_state;
  const size_t n = (size_t)t->N, G = (size_t)Ct.G;
  return gmr::read_back({{commands, st.commands, n * 12}, {gait_frequency, st.gait_frequency, n * 4}, {cmd_resample_time, st.resample_time, n * 4},
                         {cmd_draws, st.draws, n * 4}, {env_level, st.level, n * 8}, {curriculum_prob, st.prob, G * 4}, {hits, st.hits, G * 4},
                         {cum, st.cum, (G + 1) * 8}});
}

int gmr_motion_tracker_set_disturbances(gmr_motion_tracker_t* t, const gmr_disturb_config_t* cfg) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!cfg) return gmr_fail(GMR_ERR_ARG, "null configuration");
  gmr::DisturbTables Dt;
  const gmr_proprio_noise_t* specs[4] = {&cfg->kick_lin_vel, &cfg->kick_ang_vel, &cfg->push_force, &cfg->push_torque};
  static const char* const names[4] = {"kick_lin_vel", "kick_ang_vel", "push_force", "push_torque"};
  for (int k = 0; k < 4; k++) {
    const int rc = gmr::noise_spec(*specs[k], names[k], &Dt.spec[k]);
    if (rc != GMR_OK) return rc;
  }
  if (cfg->kick_every < 1 || cfg->push_every < 1 || cfg->push_duration < 0)
    return gmr_fail(GMR_ERR_ARG, "kick_every = %d, push_every = %d must be at least 1 and push_duration = %d not negative", cfg->kick_every,
                    cfg->push_every, cfg->push_duration);
  if (!std::isfinite(cfg->scale_push_force) || !std::isfinite(cfg->scale_push_torque)) return gmr_fail(GMR_ERR_ARG, "the push scales must be finite");
  Dt.kick_every = cfg->kick_every; Dt.push_every = cfg->push_every; Dt.push_duration = cfg->push_duration;
  Dt.s_force = cfg->scale_push_force; Dt.s_torque = cfg->scale_push_torque;
  Dt.on = 1;
  std::lock_guard<std::mutex> g(t->mu);
  t->disturb = Dt;
  return GMR_OK;
}

int gmr_motion_tracker_disturb_dev(gmr_motion_tracker_t* t, uint32_t common_step, const gmr_disturb_io_t* io, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::DisturbTables Dt;
  {
    std::lock_guard<std::mutex> g(t->mu);
    Dt = t->disturb;
  }
  const int act = Dt.on ? gmr::disturb_actions(Dt, common_step) : 0;
  int rc = gmr::disturb_check(Dt, io, act);
  if (rc != GMR_OK) return rc;
  if (act == 0) return 0;
  rc = gmr::disturb_launch(t, Dt, common_step, act, io, (hipStream_t)stream);
  return rc != GMR_OK ? rc : act;
}

int gmr_motion_tracker_disturb(gmr_motion_tracker_t* t, uint32_t common_step, const gmr_disturb_io_t* io) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::DisturbTables Dt = t->disturb;
  const int act = Dt.on ? gmr::disturb_actions(Dt, common_step) : 0;
  int rc = gmr::disturb_check(Dt, io, act);
  if (rc != GMR_OK) return rc;
  if (act == 0) return 0;
  const size_t n = (size_t)t->N;
  const size_t fb = io->push_force ? ((n - 1) * (size_t)io->push_force_stride + 3) * 4 : 0;
  const size_t tb = io->push_torque ? ((n - 1) * (size_t)io->push_torque_stride + 3) * 4 : 0;
  gmr::HostStage st;
  gmr_disturb_io_t d = {};
  st.in(d.root_states, io->root_states, n * 52); st.in(d.push_force, io->push_force, fb); st.in(d.push_torque, io->push_torque, tb);
  st.out(d.push_obs, io->push_obs, n * 24);
  d.push_force_stride = io->push_force_stride; d.push_torque_stride = io->push_torque_stride;
  GMR_STAGE_TRY(st, upload);
  rc = gmr::disturb_launch(t, Dt, common_step, act, &d, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  // the three arrays that are the caller's rows: copied in above, copied back whole here
  if (io->root_states) GMR_HIP_TRY(hipMemcpy(io->root_states, d.root_states, n * 52, hipMemcpyDeviceToHost));
  if (io->push_force) GMR_HIP_TRY(hipMemcpy(io->push_force, d.push_force, fb, hipMemcpyDeviceToHost));
  if (io->push_torque) GMR_HIP_TRY(hipMemcpy(io->push_torque, d.push_torque, tb, hipMemcpyDeviceToHost));
  return act;
}

}  // extern "C"
