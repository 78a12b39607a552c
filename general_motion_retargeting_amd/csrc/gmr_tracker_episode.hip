// gmr_tracker_episode.hip -- the start and the end of an episode on the motion tracker: the reset states of the
// simulator's own arrays, the one reward the learner reads and the episode statistics the reference's Recorder keeps.  What _reset_dofs,
// _reset_root_states and the delay_steps draw (booster_gym/envs/t1.py:316-340), booster_gym/envs/t1.py::_compute_reward (:560-572),
// t1_imitation.py::_compute_reward (:323-352), the reset and time-out words of t1.py:556-558 and utils/recorder.py::record_episode_statistics
// (:36-53, a Python loop with one device read per finished environment and reward term) still left to the caller after sections 6k-6s.
// The statement of record is tests/episode_mirror.py.
//
//   tracker_reset_states_kernel    ONE launch, 16 lanes per list entry: the lanes stride over the dofs, lane 0 does the root, the delay, the
//                                  step count and the reset counter; chained, also what hold and proprio_reset do afterwards
//   tracker_rewards_kernel         ONE launch, 16 lanes per environment and 16 environments per workgroup: the weighted columns, the two
//                                  group sums in rising column order, the clip, the reward, reset and time_outs; with statistics also the
//                                  running episode sums, the counters (integer atomics) and ONE partial sum per workgroup and column
//   tracker_rewards_chain_kernel   with statistics, second: ONE workgroup chains the partials of the workgroups that finished an episode
//                                  in rising workgroup order (no floating-point atomics: arrival order cannot matter)
//   tracker_reward_stats_kernel    the read-out: the three accumulators copied out and, if asked, zeroed, in one launch
//
// reset_draws and the arrays of RewardState belong to the tracker and are written by these kernels only; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_philox.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/episode_mirror.py states every line in float32 NumPy
#pragma clang fp contract(off)

#include "gmr_terrain.h"

namespace gmr {

// ---- A. reset states ------------------------------------------------------------------------------------------------------------
struct ResetIo {
  float *root, *dof_pos, *dof_vel;                         // [N][13], [N][R], [N][R]: the simulator's, rows of masked entries written
  int32_t *delay, *steps;                                  // [N] or null
  const float *init_root, *init_dof_pos, *init_dof_vel;    // [n][13], [n][R], [n][R] by list position, or null
};
// what a chained reset also writes: the state of control and proprio; null: that half is not configured or the reset is not chained
struct ResetChain {
  float *held, *acc;
  float *filtered_lin_vel, *filtered_ang_vel, *last_root_vel;
};

constexpr int RESET_GROUP = 16;             // lanes per list entry

// (the draws of element i of environment e at its reset count: tracker_words and tracker_noise of gmr_tracker_dev.h in the domain of the
// reset states)

// Entry i of the list (environment i without one), t1.py:319-340, :311, :316 in the reference's order
__global__ __launch_bounds__(256) void tracker_reset_states_kernel(const ResetTables Rt, const TerrainTables T, const TrackerState S, uint32_t* draws,
                                                                   const ResetIo io, const ResetChain ch, int N, int n,
                                                                   const int32_t* __restrict__ ids, const int32_t* __restrict__ mask, uint32_t key0,
                                                                   uint32_t key1) {
  const int i = (blockIdx.x * 256 + threadIdx.x) / RESET_GROUP;
  const int l = threadIdx.x & (RESET_GROUP - 1);
  if (i >= n) return;
  // (the test of tracker_row_skip, gmr_tracker_dev.h, written out: through the helper this kernel measured 1 % slower at N = 2^20)
  if (mask && mask[i] == 0) return;
  const int e = ids ? ids[i] : i;
  if (e < 0 || e >= N) {
    if (l == 0) atomicAdd(S.ignored, 1u);
    return;
  }
  const int R = Rt.R;
  const uint32_t ue = (uint32_t)e, nd = draws[e];
  // ---- 1: the dofs (:319-320) ----
  for (int j = l; j < R; j += RESET_GROUP) {
    float q = io.init_dof_pos ? io.init_dof_pos[(size_t)i * R + j] : Rt.default_pos[j];
    if (Rt.spec[0].dist != GMR_NOISE_NONE) q = tracker_noise(q, Rt.spec[0], ue, nd, (uint32_t)j, DRAW_RESET_STATE, key0, key1);
    io.dof_pos[(size_t)e * R + j] = q;
    io.dof_vel[(size_t)e * R + j] = io.init_dof_vel ? io.init_dof_vel[(size_t)i * R + j] : 0.0f;
    if (ch.held) {                                               // what hold does (:309)
      ch.held[(size_t)e * R + j] = q;
      ch.acc[(size_t)e * R + j] = 0.0f;
    }
  }
  if (l != 0) return;
  // ---- 2: the root row, its origin and the randomised xy (:328-330) ----
  float r[13];
#pragma unroll
  for (int k = 0; k < 13; k++) r[k] = io.init_root ? io.init_root[(size_t)i * 13 + k] : Rt.base[k];
  if (Rt.origins) {
    r[0] = r[0] + Rt.origins[(size_t)e * 2];
    r[1] = r[1] + Rt.origins[(size_t)e * 2 + 1];
  }
  if (Rt.spec[1].dist != GMR_NOISE_NONE) {
    r[0] = tracker_noise(r[0], Rt.spec[1], ue, nd, (uint32_t)R, DRAW_RESET_STATE, key0, key1);
    r[1] = tracker_noise(r[1], Rt.spec[1], ue, nd, (uint32_t)R + 1u, DRAW_RESET_STATE, key0, key1);
  }
  // ---- 3: the terrain under the drawn point (:331) ----
  if (Rt.use_terrain) {
    bool outside;
    r[2] = r[2] + terrain_height(T, r[0], r[1], &outside);
  }
  // ---- 4: the yaw (:332-336) ----
  if (Rt.yaw) {
    uint32_t wb;
    const float u = philox_unit(tracker_words(ue, nd, (uint32_t)R + 2u, DRAW_RESET_STATE, key0, key1, &wb));
    const float half = 0.5f * (Rt.yaw_lo + Rt.yaw_span * u);
    r[3] = 0.0f; r[4] = 0.0f; r[5] = sinf(half); r[6] = cosf(half);
  }
  // ---- 5: the planar velocity: the randomisation of zero (:337-340), of the given row's where one is given ----
  if (!io.init_root) { r[7] = 0.0f; r[8] = 0.0f; }
  if (Rt.spec[2].dist != GMR_NOISE_NONE) {
    r[7] = tracker_noise(r[7], Rt.spec[2], ue, nd, (uint32_t)R + 3u, DRAW_RESET_STATE, key0, key1);
    r[8] = tracker_noise(r[8], Rt.spec[2], ue, nd, (uint32_t)R + 4u, DRAW_RESET_STATE, key0, key1);
  }
#pragma unroll
  for (int k = 0; k < 13; k++) io.root[(size_t)e * 13 + k] = r[k];
  // ---- 6, 7, 8: the delay (:316), the step count (:311), the reset counter ----
  if (Rt.decimation > 0 && io.delay) {
    uint32_t wb;
    io.delay[e] = philox_below(tracker_words(ue, nd, (uint32_t)R + 5u, DRAW_RESET_STATE, key0, key1, &wb), Rt.decimation);
  }
  if (io.steps) io.steps[e] = 0;
  draws[e] = nd + 1u;
  if (ch.last_root_vel) {                                        // what proprio_reset does (:310, :312-313)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      ch.filtered_lin_vel[(size_t)e * 3 + k] = 0.0f;
      ch.filtered_ang_vel[(size_t)e * 3 + k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) ch.last_root_vel[(size_t)e * 6 + k] = r[7 + k];
  }
}

// what the entry points copy under the mutex: everything a launch carries
struct ResetView {
  ResetTables tab;
  TerrainTables terrain;
  TrackerState S;
  uint32_t* draws;
  ResetChain chain;     // of the halves that are configured for the tracker's dofs
  int R;                // the robot dofs now
};
static ResetView reset_view(gmr_motion_tracker* t) {
  ResetView V{t->resets, t->terrain, t->S, t->reset_draws, ResetChain{nullptr, nullptr, nullptr, nullptr, nullptr}, t->tab.R};
  if (t->control.R > 0 && t->control.R == t->tab.R) { V.chain.held = t->held; V.chain.acc = t->torque_acc; }
  if (t->proprio.R > 0 && t->proprio.R == t->tab.R) {
    V.chain.filtered_lin_vel = t->proprio_state.filtered_lin_vel; V.chain.filtered_ang_vel = t->proprio_state.filtered_ang_vel;
    V.chain.last_root_vel = t->proprio_state.last_root_vel;
  }
  return V;
}

static int reset_states_check(const gmr_motion_tracker* t, const ResetView& V, int n, const void* ids, const gmr_reset_io_t* io, int chain) {
  if (V.tab.R == 0) return gmr_fail(GMR_ERR_ARG, "reset states are not set on this tracker (gmr_motion_tracker_set_reset_states)");
  if (V.tab.R != V.R)
    return gmr_fail(GMR_ERR_ARG, "reset states were set for R = %d robot dofs, the dof map now has %d: call gmr_motion_tracker_set_reset_states again",
                    V.tab.R, V.R);
  const int rc = subset_check(t->N, n, ids, "the mask and the init rows cover every environment");
  if (rc != GMR_OK) return rc;
  if (chain != 0 && chain != 1) return gmr_fail(GMR_ERR_ARG, "chain = %d, must be 0 or 1", chain);
  if (!io) return gmr_fail(GMR_ERR_ARG, "null io table");
  if (!io->root_states || !io->dof_pos || !io->dof_vel) return gmr_fail(GMR_ERR_ARG, "null root_states / dof_pos / dof_vel");
  return GMR_OK;
}

static int reset_states_launch(gmr_motion_tracker* t, const ResetView& V, int n, const int32_t* d_ids, const int32_t* d_mask, const gmr_reset_io_t* io,
                               int chain, hipStream_t stream) {
  const int rc = reset_states_check(t, V, n, d_ids, io, chain);
  if (rc != GMR_OK) return rc;
  if (n == 0) return GMR_OK;
  const ResetIo X{io->root_states, io->dof_pos, io->dof_vel, io->delay_steps, io->episode_steps, io->init_root_states, io->init_dof_pos, io->init_dof_vel};
  const ResetChain none{nullptr, nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(tracker_reset_states_kernel, dim3(row_blocks(n, RESET_GROUP)), dim3(256), 0, stream, V.tab, V.terrain, V.S, V.draws, X,
                     chain ? V.chain : none, t->N, n, d_ids, d_mask, t->key[0], t->key[1]);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// ---- B, C. the reward and the episode statistics ------------------------------------------------------------------------------------

struct RewardIn {
  const float* src[REWARD_BLOCKS + 1];      // term, link_term, proprio_term, feet_term, cmd_term, extra
  const int32_t *done, *flags;
};
struct RewardOut {
  float *reward, *scaled, *group_total;
  int32_t *reset, *time_outs;
};

constexpr int REWARD_ENVS = 16;             // environments per workgroup: 16 lanes each
constexpr int REWARD_SLOTS = (REWARD_MAX_COLS + 15) / 16;      // columns per lane

// in0 / in1: bit c set when column c is in (its weight not zero, its array given) and feeds group 0 / 1: formed on the host, so that the
// gather loop reads no table
__global__ __launch_bounds__(256) void tracker_rewards_kernel(const RewardTables Rt, const RewardState St, const RewardIn X, const RewardOut O, int N,
                                                              unsigned long long in0, unsigned long long in1) {
  __shared__ float s_ep[REWARD_ENVS][REWARD_MAX_COLS + 1];
  __shared__ int s_reset[REWARD_ENVS];
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int64_t e = (int64_t)blockIdx.x * REWARD_ENVS + g;
  const bool live = e < N;
  const int C = Rt.C, K = C + 1;
  // ---- 1: scaled_c = w_c * term_c; a column whose weight is zero or whose array is absent is +0 and stays out of the sums ----
  float sc[REWARD_SLOTS];
#pragma unroll
  for (int j = 0; j < REWARD_SLOTS; j++) {
    const int c = l + 16 * j;
    float v = 0.0f;
    if (live && c < C) {
      const int b = Rt.block[c];
      const float* p = X.src[b];
      if (p != nullptr && Rt.w[c] != 0.0f) v = Rt.w[c] * p[e * Rt.width[b] + Rt.off[c]];
      if (O.scaled) O.scaled[e * C + c] = v;
    }
    sc[j] = v;
  }
  // ---- 2: the group sums from +0 in rising c: every lane of the environment gathers the row through the group's permutes and holds the sums ----
  float S0 = 0.0f, S1 = 0.0f;
#pragma unroll
  for (int j = 0; j < REWARD_SLOTS; j++) {
    for (int i = 0; i < 16; i++) {
      const int c = 16 * j + i;
      if (c >= C) break;                                         // (uniform)
      const float v = __shfl(sc[j], i, 16);
      if ((in0 >> c) & 1ull) S0 = S0 + v;
      if ((in1 >> c) & 1ull) S1 = S1 + v;
    }
  }
  // ---- 3, 4: the clip (a NaN stays, as torch.clip keeps it) and the reward ----
  if (Rt.pos[0] && S0 < 0.0f) S0 = 0.0f;
  if (Rt.pos[1] && S1 < 0.0f) S1 = 0.0f;
  const float r0 = Rt.gw[0] * S0, r1 = Rt.gw[1] * S1;
  const float reward = r0 + r1;
  const int32_t dn = (live && X.done) ? X.done[e] : 0, fl = (live && X.flags) ? X.flags[e] : 0;
  const bool reset = dn != 0;
  if (live && l == 0) {
    if (O.reward) O.reward[e] = reward;
    if (O.group_total) { O.group_total[e * 2] = S0; O.group_total[e * 2 + 1] = S1; }
    if (O.reset) O.reset[e] = reset ? 1 : 0;
    if (O.time_outs) O.time_outs[e] = ((dn & GMR_REWARD_DONE_TIME_OUT) | (fl & GMR_CMD_BOUNDARY)) != 0 ? 1 : 0;       // t1.py:556-558
  }
  if (!Rt.stats) return;                                         // (uniform)
  // ---- the Recorder's half (recorder.py:36-53) ----
  if (live) {
    if (l == 0) {
      int32_t n = St.ep_steps[e] + (*St.started ? 1 : 0);        // the very first call starts from zeros (:37-40)
      if (reset) {
        atomicAdd(St.fin_count, 1u);
        atomicAdd(St.fin_steps, (unsigned long long)(uint32_t)n);
        n = 0;
      }
      St.ep_steps[e] = n;
      const float s = St.ep_sum[e * K] + reward;                 // column 0 is the reward
      s_ep[g][0] = s;
      St.ep_sum[e * K] = reset ? 0.0f : s;
    }
#pragma unroll
    for (int j = 0; j < REWARD_SLOTS; j++) {
      const int c = l + 16 * j;
      if (c < C) {
        const float s = St.ep_sum[e * K + 1 + c] + sc[j];
        s_ep[g][1 + c] = s;
        St.ep_sum[e * K + 1 + c] = reset ? 0.0f : s;
      }
    }
  }
  if (l == 0) s_reset[g] = live && reset;
  __syncthreads();
  // the workgroup's partial of column k: from +0, its finished environments in rising order, in double
  const int k = threadIdx.x;
  bool any = false;
  double p = 0.0;
  for (int q = 0; q < REWARD_ENVS; q++) {
    if (!s_reset[q]) continue;
    any = true;
    if (k < K) p = p + (double)s_ep[q][k];
  }
  if (any && k < K) St.part[(int64_t)blockIdx.x * K + k] = p;
  if (k == 0) St.wg_any[blockIdx.x] = any ? 1u : 0u;
}

// fin_sum[k] = (..((fin_sum[k] + part[w0][k]) + part[w1][k]) ..) over the workgroups w0 < w1 < .. that finished an episode in this call.
// A tile is 1024 workgroups: their flags become sixteen ballots, the flagged ones are ranked in rising order, the whole workgroup loads
// their rows into LDS side by side (one memory latency per tile, not one per row) and the first K lanes add them in rank order; a tile
// with more than CHAIN_ROWS flagged workgroups is added straight from memory, in the same order.
constexpr int CHAIN_ROWS = 120;
__global__ __launch_bounds__(1024) void tracker_rewards_chain_kernel(const RewardState St, int nwg, int K) {
  __shared__ unsigned long long s_mask[16];
  __shared__ int s_list[CHAIN_ROWS];
  __shared__ double s_rows[CHAIN_ROWS * (REWARD_MAX_COLS + 1)];
  const int tid = threadIdx.x;
  double acc = tid < K ? St.fin_sum[tid] : 0.0;
  for (int base = 0; base < nwg; base += 1024) {
    const int w = base + tid;
    const bool flagged = w < nwg && St.wg_any[w] != 0u;
    const unsigned long long m = __ballot(flagged);
    if ((tid & 63) == 0) s_mask[tid >> 6] = m;
    __syncthreads();
    int total = 0, rank = 0;
    for (int q = 0; q < 16; q++) {
      const int cnt = __popcll(s_mask[q]);
      if (q < (tid >> 6)) rank += cnt;
      total += cnt;
    }
    if (total == 0) {                                            // (uniform)
      __syncthreads();
      continue;
    }
    if (total <= CHAIN_ROWS) {                                   // (uniform)
      rank += __popcll(m & ((1ull << (tid & 63)) - 1ull));
      if (flagged) s_list[rank] = tid;
      __syncthreads();
      for (int idx = tid; idx < total * K; idx += 1024) {
        const int r = idx / K, k = idx - r * K;
        s_rows[idx] = St.part[(int64_t)(base + s_list[r]) * K + k];
      }
      __syncthreads();
      if (tid < K)
        for (int r = 0; r < total; r++) acc = acc + s_rows[r * K + tid];
    } else if (tid < K) {
      for (int q = 0; q < 16; q++) {
        unsigned long long bits = s_mask[q];
        while (bits) {
          const int b = __ffsll((long long)bits) - 1;
          bits &= bits - 1;
          acc = acc + St.part[(int64_t)(base + q * 64 + b) * K + tid];
        }
      }
    }
    __syncthreads();
  }
  if (tid < K) St.fin_sum[tid] = acc;
  if (tid == 0) *St.started = 1u;
}

// out: u64 episodes, u64 steps, f64 sums[K]
__global__ __launch_bounds__(64) void tracker_reward_stats_kernel(const RewardState St, int K, uint64_t* out, int clear) {
  const int k = threadIdx.x;
  if (k < K) {
    if (out) ((double*)(out + 2))[k] = St.fin_sum[k];
    if (clear) St.fin_sum[k] = 0.0;
  }
  if (k == 0) {
    if (out) { out[0] = (uint64_t)*St.fin_count; out[1] = (uint64_t)*St.fin_steps; }
    if (clear) { *St.fin_count = 0u; *St.fin_steps = 0ull; }
  }
}

// what the entry points copy under the mutex: everything a launch carries, the weights of the blocks as they are configured now
struct RewardView {
  RewardTables tab;
  RewardState st;
  int mask;             // the blocks configured on the tracker now
};

static int configured_blocks(const gmr_motion_tracker* t) {
  return GMR_REWARD_BLOCK_TERMS | (t->links.nsel > 0 ? GMR_REWARD_BLOCK_LINKS : 0) | (t->proprio.R > 0 ? GMR_REWARD_BLOCK_PROPRIO : 0) |
         (t->feet.E > 0 ? GMR_REWARD_BLOCK_FEET : 0) | (t->commands.on ? GMR_REWARD_BLOCK_COMMANDS : 0);
}

// (under the mutex)
static RewardView reward_view(const gmr_motion_tracker* t) {
  RewardView V{t->rewards, t->reward_state, configured_blocks(t)};
  const float* weights[REWARD_BLOCKS] = {t->tab.weight, t->links.term_weight, t->proprio.scale, t->feet.scale, t->commands.scale};
  for (int c = 0; c < V.tab.C - V.tab.E; c++) V.tab.w[c] = weights[V.tab.block[c]][V.tab.off[c]];
  return V;
}

static int rewards_check(const RewardView& V, const gmr_reward_in_t* in, const gmr_reward_out_t* out) {
  if (!V.tab.on) return gmr_fail(GMR_ERR_ARG, "rewards are not set on this tracker (gmr_motion_tracker_set_rewards)");
  if (V.mask != V.tab.mask)
    return gmr_fail(GMR_ERR_ARG, "the blocks configured on the tracker (%d) are not those the reward columns were laid out for (%d): set the rewards again",
                    V.mask, V.tab.mask);
  if (!in || !out) return gmr_fail(GMR_ERR_ARG, "null input / output table");
  return GMR_OK;
}

static int rewards_launch(gmr_motion_tracker* t, const RewardView& V, const gmr_reward_in_t* in, const gmr_reward_out_t* out, hipStream_t stream) {
  const int rc = rewards_check(V, in, out);
  if (rc != GMR_OK) return rc;
  const RewardIn X{{in->term, in->link_term, in->proprio_term, in->feet_term, in->cmd_term, in->extra}, in->done, in->flags};
  const RewardOut O{out->reward, out->scaled, out->group_total, out->reset, out->time_outs};
  const int nwg = (t->N + REWARD_ENVS - 1) / REWARD_ENVS;
  unsigned long long in0 = 0, in1 = 0;
  for (int c = 0; c < V.tab.C; c++) {
    if (V.tab.w[c] == 0.0f || X.src[V.tab.block[c]] == nullptr) continue;
    if (V.tab.group[c] & GMR_REWARD_LOCOMOTION) in0 |= 1ull << c;
    if (V.tab.group[c] & GMR_REWARD_IMITATION) in1 |= 1ull << c;
  }
  hipLaunchKernelGGL(tracker_rewards_kernel, dim3((unsigned)nwg), dim3(256), 0, stream, V.tab, V.st, X, O, t->N, in0, in1);
  if (V.tab.stats) hipLaunchKernelGGL(tracker_rewards_chain_kernel, dim3(1), dim3(1024), 0, stream, V.st, nwg, V.tab.C + 1);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

static int stats_check(const RewardTables& Rt) {
  if (!Rt.on) return gmr_fail(GMR_ERR_ARG, "rewards are not set on this tracker (gmr_motion_tracker_set_rewards)");
  if (!Rt.stats) return gmr_fail(GMR_ERR_ARG, "the episode statistics are off (gmr_reward_config_t.stats)");
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker episode") --------------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_reset_states(gmr_motion_tracker_t* t, const gmr_reset_config_t* cfg) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!cfg) return gmr_fail(GMR_ERR_ARG, "null configuration");
  if (!cfg->default_dof_pos) return gmr_fail(GMR_ERR_ARG, "null default_dof_pos");
  gmr::ResetTables Rt;
  for (int k = 0; k < 13; k++) {
    if (!std::isfinite(cfg->base_init_state[k])) return gmr_fail(GMR_ERR_ARG, "base_init_state[%d] is not finite", k);
    Rt.base[k] = cfg->base_init_state[k];
  }
  const gmr_proprio_noise_t* specs[gmr::RESET_SPECS] = {&cfg->init_dof_pos, &cfg->init_base_pos_xy, &cfg->init_base_lin_vel_xy};
  static const char* const names[gmr::RESET_SPECS] = {"init_dof_pos", "init_base_pos_xy", "init_base_lin_vel_xy"};
  for (int k = 0; k < gmr::RESET_SPECS; k++) {
    const int rc = gmr::noise_spec(*specs[k], names[k], &Rt.spec[k]);
    if (rc != GMR_OK) return rc;
  }
  if (cfg->yaw != 0 && cfg->yaw != 1) return gmr_fail(GMR_ERR_ARG, "yaw = %d, must be 0 or 1", cfg->yaw);
  if (cfg->use_terrain != 0 && cfg->use_terrain != 1) return gmr_fail(GMR_ERR_ARG, "use_terrain = %d, must be 0 or 1", cfg->use_terrain);
  if (cfg->yaw) {
    const double lo = cfg->yaw_range[0], hi = cfg->yaw_range[1];
    if (!gmr::fits(lo) || !gmr::fits(hi) || !gmr::fits(hi - lo)) return gmr_fail(GMR_ERR_ARG, "yaw_range (%g, %g) is not finite in float32", lo, hi);
    if (hi < lo) return gmr_fail(GMR_ERR_ARG, "yaw_range: upper = %g < lower = %g", hi, lo);
    Rt.yaw = 1; Rt.yaw_lo = (float)lo; Rt.yaw_span = (float)(hi - lo);
  }
  if (cfg->decimation < 0 || cfg->decimation > gmr::CONTROL_MAX_DECIMATION)
    return gmr_fail(GMR_ERR_ARG, "decimation = %d outside [0, %d]", cfg->decimation, gmr::CONTROL_MAX_DECIMATION);
  Rt.decimation = cfg->decimation;
  Rt.use_terrain = cfg->use_terrain;
  std::lock_guard<std::mutex> g(t->mu);
  const int R = t->tab.R;
  for (int j = 0; j < R; j++) {
    if (!std::isfinite(cfg->default_dof_pos[j])) return gmr_fail(GMR_ERR_ARG, "default_dof_pos[%d] is not finite", j);
    Rt.default_pos[j] = cfg->default_dof_pos[j];
  }
  const size_t n = (size_t)t->N;
  if (cfg->env_origins)
    for (size_t k = 0; k < n * 2; k++)
      if (!std::isfinite(cfg->env_origins[k])) return gmr_fail(GMR_ERR_ARG, "env_origins[%zu][%zu] is not finite", k / 2, k % 2);
  Rt.R = R;
  gmr::Carve cv;
  const size_t o_draws = cv.take(n * 4), o_org = cv.take(cfg->env_origins ? n * 8 : 0);
  GMR_HIP_TRY(hipDeviceSynchronize());               // nothing in flight reads the origins this call replaces
  GMR_HIP_TRY(t->reset_block.reserve(cv.total() + 256));
  char* d = t->reset_block.data();
  GMR_HIP_TRY(hipMemset(d + o_draws, 0, n * 4));
  if (cfg->env_origins) {
    GMR_HIP_TRY(hipMemcpy(d + o_org, cfg->env_origins, n * 8, hipMemcpyHostToDevice));
    Rt.origins = (const float*)(d + o_org);
  }
  GMR_HIP_TRY(hipDeviceSynchronize());
  t->resets = Rt;
  t->reset_draws = (uint32_t*)(d + o_draws);
  return GMR_OK;
}

int gmr_motion_tracker_reset_states_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_mask, const gmr_reset_io_t* io,
                                        int chain, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::ResetView V;
  {
    std::lock_guard<std::mutex> g(t->mu);
    V = gmr::reset_view(t);
  }
  return gmr::reset_states_launch(t, V, n, d_env_ids, d_mask, io, chain, (hipStream_t)stream);
}

int gmr_motion_tracker_reset_states(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* mask, const gmr_reset_io_t* io, int chain,
                                    int* ignored) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (ignored) *ignored = 0;
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::ResetView V = gmr::reset_view(t);
  int rc = gmr::reset_states_check(t, V, n, env_ids, io, chain);
  if (rc != GMR_OK) return rc;
  if (n == 0) return GMR_OK;
  if (env_ids) {                                     // an environment twice in a list would be written by two lane rows
    std::vector<char> seen((size_t)t->N, 0);
    for (int i = 0; i < n; i++) {
      const int e = env_ids[i];
      if ((mask && mask[i] == 0) || e < 0 || e >= t->N) continue;
      if (seen[(size_t)e]) return gmr_fail(GMR_ERR_ARG, "env_ids names environment %d twice", e);
      seen[(size_t)e] = 1;
    }
  }
  const size_t nn = (size_t)n, N = (size_t)t->N, R = (size_t)V.R;
  gmr::HostStage st;
  const int32_t *d_ids, *d_mask;
  gmr_reset_io_t d = {};
  st.in(d_ids, env_ids, nn * 4); st.in(d_mask, mask, nn * 4);
  // the five arrays that are the caller's rows: copied in here, copied back whole below
  st.in(d.root_states, io->root_states, N * 52); st.in(d.dof_pos, io->dof_pos, N * R * 4); st.in(d.dof_vel, io->dof_vel, N * R * 4);
  st.in(d.delay_steps, io->delay_steps, N * 4); st.in(d.episode_steps, io->episode_steps, N * 4);
  st.in(d.init_root_states, io->init_root_states, nn * 52); st.in(d.init_dof_pos, io->init_dof_pos, nn * R * 4);
  st.in(d.init_dof_vel, io->init_dof_vel, nn * R * 4);
  GMR_STAGE_TRY(st, upload);
  gmr::IgnoredDelta ig(V.S.ignored, ignored);
  if ((rc = ig.begin()) != GMR_OK) return rc;
  rc = gmr::reset_states_launch(t, V, n, d_ids, d_mask, &d, chain, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  GMR_HIP_TRY(hipMemcpy(io->root_states, d.root_states, N * 52, hipMemcpyDeviceToHost));
  GMR_HIP_TRY(hipMemcpy(io->dof_pos, d.dof_pos, N * R * 4, hipMemcpyDeviceToHost));
  GMR_HIP_TRY(hipMemcpy(io->dof_vel, d.dof_vel, N * R * 4, hipMemcpyDeviceToHost));
  if (io->delay_steps) GMR_HIP_TRY(hipMemcpy(io->delay_steps, d.delay_steps, N * 4, hipMemcpyDeviceToHost));
  if (io->episode_steps) GMR_HIP_TRY(hipMemcpy(io->episode_steps, d.episode_steps, N * 4, hipMemcpyDeviceToHost));
  return ig.end();
}

int gmr_motion_tracker_reset_state(gmr_motion_tracker_t* t, uint32_t* reset_draws) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  if (t->resets.R == 0) return gmr_fail(GMR_ERR_ARG, "reset states are not set on this tracker (gmr_motion_tracker_set_reset_states)");
  return gmr::read_back({{reset_draws, t->reset_draws, (size_t)t->N * 4}});
}

int gmr_motion_tracker_set_rewards(gmr_motion_tracker_t* t, const gmr_reward_config_t* cfg) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!cfg) return gmr_fail(GMR_ERR_ARG, "null configuration");
  gmr::RewardTables Rt;
  const int E = cfg->extra_cols;
  if (E < 0 || E > GMR_REWARD_MAX_EXTRA) return gmr_fail(GMR_ERR_ARG, "extra_cols = %d outside [0, %d]", E, GMR_REWARD_MAX_EXTRA);
  if ((cfg->stats != 0 && cfg->stats != 1) || (cfg->only_positive[0] != 0 && cfg->only_positive[0] != 1) ||
      (cfg->only_positive[1] != 0 && cfg->only_positive[1] != 1))
    return gmr_fail(GMR_ERR_ARG, "stats = %d, only_positive = (%d, %d): each must be 0 or 1", cfg->stats, cfg->only_positive[0], cfg->only_positive[1]);
  if (!std::isfinite(cfg->group_weight[0]) || !std::isfinite(cfg->group_weight[1])) return gmr_fail(GMR_ERR_ARG, "group_weight must be finite");
  for (int k = 0; k < E; k++)
    if (!std::isfinite(cfg->extra_weights[k])) return gmr_fail(GMR_ERR_ARG, "extra_weights[%d] is not finite", k);
  std::lock_guard<std::mutex> g(t->mu);
  const int mask = gmr::configured_blocks(t);
  if (cfg->blocks != mask)
    return gmr_fail(GMR_ERR_ARG, "blocks = %d, but the blocks configured on this tracker are %d (GMR_REWARD_BLOCK_*)", cfg->blocks, mask);
  static const int widths[gmr::REWARD_BLOCKS + 1] = {gmr::TRACKER_TERMS, gmr::LINK_TERMS, gmr::PROPRIO_TERMS, gmr::FEET_TERMS, gmr::CMD_TERMS, 0};
  int C = 0;
  for (int b = 0; b <= gmr::REWARD_BLOCKS; b++) {
    const int wd = b < gmr::REWARD_BLOCKS ? widths[b] : E;
    Rt.width[b] = wd;
    if (b < gmr::REWARD_BLOCKS && !(mask & (1 << b))) continue;
    for (int j = 0; j < wd; j++, C++) {
      Rt.block[C] = (uint8_t)b;
      Rt.off[C] = (uint8_t)j;
      if (b == gmr::REWARD_BLOCKS) Rt.w[C] = cfg->extra_weights[j];
    }
  }
  for (int c = 0; c < C; c++) {
    if (cfg->groups[c] > (GMR_REWARD_LOCOMOTION | GMR_REWARD_IMITATION)) return gmr_fail(GMR_ERR_ARG, "groups[%d] = %d has bits beyond the two groups", c, cfg->groups[c]);
    Rt.group[c] = cfg->groups[c];
  }
  Rt.on = 1; Rt.mask = mask; Rt.C = C; Rt.E = E; Rt.stats = cfg->stats;
  Rt.pos[0] = cfg->only_positive[0]; Rt.pos[1] = cfg->only_positive[1];
  Rt.gw[0] = cfg->group_weight[0]; Rt.gw[1] = cfg->group_weight[1];
  gmr::RewardState st;
  if (!Rt.stats) GMR_HIP_TRY(hipDeviceSynchronize());      // nothing in flight reads the arrays this call drops (fresh_block waits too)
  if (Rt.stats) {
    const size_t n = (size_t)t->N, K = (size_t)C + 1, nwg = (n + gmr::REWARD_ENVS - 1) / gmr::REWARD_ENVS;
    gmr::Carve cv;
    const size_t o_steps = cv.take(n * 4), o_sum = cv.take(n * K * 4), o_fsum = cv.take(K * 8), o_fsteps = cv.take(8), o_count = cv.take(4);
    const size_t o_started = cv.take(4), o_part = cv.take(nwg * K * 8), o_any = cv.take(nwg * 4);
    const int rc = gmr::fresh_block(t->reward_block, cv);
    if (rc != GMR_OK) return rc;
    char* d = t->reward_block.data();
    st.ep_steps = (int32_t*)(d + o_steps); st.ep_sum = (float*)(d + o_sum); st.fin_sum = (double*)(d + o_fsum);
    st.fin_steps = (unsigned long long*)(d + o_fsteps); st.fin_count = (uint32_t*)(d + o_count); st.started = (uint32_t*)(d + o_started);
    st.part = (double*)(d + o_part); st.wg_any = (uint32_t*)(d + o_any);
  }
  t->rewards = Rt;
  t->reward_state = st;
  return GMR_OK;
}

int gmr_motion_tracker_rewards_dev(gmr_motion_tracker_t* t, const gmr_reward_in_t* in, const gmr_reward_out_t* out, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::RewardView V;
  {
    std::lock_guard<std::mutex> g(t->mu);
    V = gmr::reward_view(t);
  }
  return gmr::rewards_launch(t, V, in, out, (hipStream_t)stream);
}

int gmr_motion_tracker_rewards(gmr_motion_tracker_t* t, const gmr_reward_in_t* in, const gmr_reward_out_t* out) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::RewardView V = gmr::reward_view(t);
  int rc = gmr::rewards_check(V, in, out);
  if (rc != GMR_OK) return rc;
  const size_t n = (size_t)t->N, C = (size_t)V.tab.C;
  gmr::HostStage st;
  gmr_reward_in_t din = {};
  gmr_reward_out_t dout = {};
  const bool has[gmr::REWARD_BLOCKS] = {true, (V.mask & GMR_REWARD_BLOCK_LINKS) != 0, (V.mask & GMR_REWARD_BLOCK_PROPRIO) != 0,
                                        (V.mask & GMR_REWARD_BLOCK_FEET) != 0, (V.mask & GMR_REWARD_BLOCK_COMMANDS) != 0};
  // (the array of a block that has no columns is never read: not staged)
  st.in(din.term, in->term, n * gmr::TRACKER_TERMS * 4);
  st.in(din.link_term, has[1] ? in->link_term : nullptr, n * gmr::LINK_TERMS * 4);
  st.in(din.proprio_term, has[2] ? in->proprio_term : nullptr, n * gmr::PROPRIO_TERMS * 4);
  st.in(din.feet_term, has[3] ? in->feet_term : nullptr, n * gmr::FEET_TERMS * 4);
  st.in(din.cmd_term, has[4] ? in->cmd_term : nullptr, n * gmr::CMD_TERMS * 4);
  st.in(din.extra, V.tab.E ? in->extra : nullptr, n * (size_t)V.tab.E * 4);
  st.in(din.done, in->done, n * 4); st.in(din.flags, in->flags, n * 4);
  st.out(dout.reward, out->reward, n * 4); st.out(dout.scaled, out->scaled, n * C * 4); st.out(dout.group_total, out->group_total, n * 8);
  st.out(dout.reset, out->reset, n * 4); st.out(dout.time_outs, out->time_outs, n * 4);
  GMR_STAGE_TRY(st, upload);
  rc = gmr::rewards_launch(t, V, &din, &dout, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_tracker_reward_stats_dev(gmr_motion_tracker_t* t, uint64_t* out, int clear, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (clear != 0 && clear != 1) return gmr_fail(GMR_ERR_ARG, "clear = %d, must be 0 or 1", clear);
  gmr::RewardTables Rt;
  gmr::RewardState St;
  {
    std::lock_guard<std::mutex> g(t->mu);
    Rt = t->rewards;
    St = t->reward_state;
  }
  const int rc = gmr::stats_check(Rt);
  if (rc != GMR_OK) return rc;
  hipLaunchKernelGGL(gmr::tracker_reward_stats_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, St, Rt.C + 1, out, clear);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

int gmr_motion_tracker_reward_stats(gmr_motion_tracker_t* t, uint64_t* out, int clear) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (clear != 0 && clear != 1) return gmr_fail(GMR_ERR_ARG, "clear = %d, must be 0 or 1", clear);
  std::lock_guard<std::mutex> g(t->mu);
  const int rc = gmr::stats_check(t->rewards);
  if (rc != GMR_OK) return rc;
  const int K = t->rewards.C + 1;
  gmr::HostStage st;
  uint64_t* d_out = nullptr;
  st.out(d_out, out, (size_t)(K + 2) * 8);
  GMR_STAGE_TRY(st, upload);
  hipLaunchKernelGGL(gmr::tracker_reward_stats_kernel, dim3(1), dim3(64), 0, nullptr, t->reward_state, K, d_out, clear);
  GMR_HIP_TRY(hipGetLastError());
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_tracker_reward_state(gmr_motion_tracker_t* t, int32_t* ep_steps, float* ep_sum) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const int rc = gmr::stats_check(t->rewards);
  if (rc != GMR_OK) return rc;
  const size_t n = (size_t)t->N, K = (size_t)t->rewards.C + 1;
  return gmr::read_back({{ep_steps, t->reward_state.ep_steps, n * 4}, {ep_sum, t->reward_state.ep_sum, n * K * 4}});
}

}  // extern "C"
