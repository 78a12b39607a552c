// gmr_tracker_rollout.hip -- the rollout of a training iteration on the motion tracker: what the reference's runner
// does with the outputs of a step before the loss reads them.  The six indexed assignments into its ExperienceBuffer per step
// (booster_gym/utils/runner.py:107-108, :115-118, utils/buffer.py:15-16) and, per mini-epoch, the bootstrap of the timed-out rewards
// (runner.py:135), discount_values (utils/utils.py:33-44: a Python loop over the horizon), the returns (:144), the mean, the unbiased
// deviation and the normalisation (:145).  The statement of record is tests/rollout_mirror.py.
//
//   tracker_rollout_record_kernel     ONE launch: the rows of a step into slot n of the caller's arrays, the two int32 words as bytes
//   tracker_rollout_scan_kernel       one lane per environment walks the horizon downward, loads and stores coalesced across the
//                                     environments, sixteen rows requested ahead of the sixteen it works on; with normalize ONE pair of
//                                     partial sums per workgroup
//   tracker_rollout_chain_kernel      beyond GMR_ROLLOUT_FOLD groups: ONE workgroup chains the partials in rising group order
//   tracker_rollout_normalize_kernel  the normalisation; up to GMR_ROLLOUT_FOLD groups every workgroup chains the partials itself, in
//                                     the same order (no floating-point atomics: arrival order cannot matter)
//
// The arrays are the caller's; the partial sums belong to the tracker and are written by these kernels only; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <type_traits>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/rollout_mirror.py states every line in float32 (the sums in float64) NumPy
#pragma clang fp contract(off)

namespace gmr {

// ---- A. record ------------------------------------------------------------------------------------------------------------------
constexpr int RECORD_COPIES = 3;            // obs, priv, actions
struct RecordArgs {
  const float* src[RECORD_COPIES];          // [N][cols] or null
  float* dst[RECORD_COPIES];                // slot n of the caller's array
  long long items[RECORD_COPIES];           // work items of the copy: float4s when vec, floats else; 0: not handed in
  long long count[RECORD_COPIES];           // floats
  int vec[RECORD_COPIES];                   // both addresses on 16 bytes
  const float* reward;                      // [N] or null
  const int32_t *done, *time_outs;          // [N] or null
  float* rewards;                           // slot n
  uint8_t *dones, *touts;                   // slot n
  int N;
};

// Work item i: the copies side by side, then one item per environment for the three scalars
__global__ __launch_bounds__(256) void tracker_rollout_record_kernel(const RecordArgs X) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
#pragma unroll
  for (int s = 0; s < RECORD_COPIES; s++) {
    if (i < X.items[s]) {
      if (X.vec[s]) {
        const long long at = i * 4;
        if (at + 4 <= X.count[s]) {
          *reinterpret_cast<float4*>(X.dst[s] + at) = *reinterpret_cast<const float4*>(X.src[s] + at);
        } else {
          for (long long k = at; k < X.count[s]; k++) X.dst[s][k] = X.src[s][k];
        }
      } else {
        X.dst[s][i] = X.src[s][i];
      }
      return;
    }
    i -= X.items[s];
  }
  if (i >= X.N) return;
  if (X.reward) X.rewards[i] = X.reward[i];
  if (X.done) X.dones[i] = X.done[i] != 0 ? 1 : 0;
  if (X.time_outs) X.touts[i] = X.time_outs[i] != 0 ? 1 : 0;
}

// the slots of a record call and what goes into them; a null input keeps its slot out
struct RecordSlots {
  float *obs, *priv, *actions, *rewards;
  uint8_t *dones, *time_outs;
};

static int record_check(const RolloutTables& R, int n, const gmr_rollout_io_t* io, const float* obs, const float* priv, const float* actions,
                        const float* reward, const int32_t* done, const int32_t* time_outs) {
  if (R.H == 0) return gmr_fail(GMR_ERR_ARG, "the rollout is not set on this tracker (gmr_motion_tracker_set_rollout)");
  if (n < 0 || n >= R.H) return gmr_fail(GMR_ERR_ARG, "slot n = %d outside [0, %d)", n, R.H);
  if (!io) return gmr_fail(GMR_ERR_ARG, "null io table");
  if (priv && R.P == 0) return gmr_fail(GMR_ERR_ARG, "priv given, but the rollout was set with priv_cols = 0");
  if ((obs && !io->obs) || (priv && !io->priv) || (actions && !io->actions) || (reward && !io->rewards) || (done && !io->dones) ||
      (time_outs && !io->time_outs))
    return gmr_fail(GMR_ERR_ARG, "an input was handed in whose rollout array is null in the io table");
  return GMR_OK;
}

static int record_launch(const RolloutTables& R, int N, const RecordSlots& S, const float* obs, const float* priv, const float* actions,
                         const float* reward, const int32_t* done, const int32_t* time_outs, hipStream_t stream) {
  RecordArgs X = {};
  const float* src[RECORD_COPIES] = {obs, priv, actions};
  float* dst[RECORD_COPIES] = {S.obs, S.priv, S.actions};
  const int cols[RECORD_COPIES] = {R.O, R.P, R.A};
  long long total = 0;
  for (int s = 0; s < RECORD_COPIES; s++) {
    if (!src[s]) continue;
    X.src[s] = src[s];
    X.dst[s] = dst[s];
    X.count[s] = (long long)N * cols[s];
    X.vec[s] = (((uintptr_t)src[s] | (uintptr_t)dst[s]) & 15u) == 0;
    X.items[s] = X.vec[s] ? (X.count[s] + 3) / 4 : X.count[s];
    total += X.items[s];
  }
  X.reward = reward; X.done = done; X.time_outs = time_outs;
  X.rewards = S.rewards; X.dones = S.dones; X.touts = S.time_outs;
  X.N = N;
  if (reward || done || time_outs) total += N;
  if (total == 0) return GMR_OK;
  hipLaunchKernelGGL(tracker_rollout_record_kernel, dim3(lane_blocks(total)), dim3(256), 0, stream, X);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// ---- B. advantages ----------------------------------------------------------------------------------------------------------------
constexpr int ENVS = GMR_ROLLOUT_ENVS;      // environments per workgroup of the scan: one wavefront, so that N = 4096 spreads over 64 CUs
constexpr int FOLD = GMR_ROLLOUT_FOLD;      // up to this many groups the normalisation chains the partials itself
constexpr int ROWS = 16;                    // rows of the horizon a lane requests at once
static_assert(ENVS == 64, "the tree of the scan is the wavefront's");

struct ScanArgs {
  float* rewards;                           // [H][N], the timed-out entries rewritten
  const uint8_t *dones, *time_outs;         // [H][N]
  const float *values, *last_values;        // [H][N], [N]
  float *adv, *ret;                         // [H][N] or null
  double* part;                             // [groups][2] or null: no sums wanted
  int H, N;
  float g, gl;
};

struct ScanRow {
  float r, v;
  uint8_t d, to;
};

// Inside the one divergent region of the live lanes everything is straight-line code with uniform branches only: a load or a store
// under a per-row condition leaves the compiler without a count of the requests in flight, and it then waits for all of them at every
// row.  So a row below 0 is requested as row 0 and not worked on, and the reward goes back to its place whether it was replaced or not.
// ALL: advantages and returns are both wanted (no test per row).
template <bool ALL>
__global__ __launch_bounds__(ENVS) void tracker_rollout_scan_kernel(const ScanArgs X) {
  const int64_t e = (int64_t)blockIdx.x * ENVS + threadIdx.x;
  const int64_t N = X.N;
  const int H = X.H;
  double s1 = 0.0, s2 = 0.0;
  if (e < N) {
    ScanRow a[ROWS], b[ROWS];
    float last = 0.0f, nv = X.last_values[e];
    // rows t0, t0 - 1, .. of the horizon
    auto request = [&](ScanRow(&w)[ROWS], int t0) {
#pragma unroll
      for (int k = 0; k < ROWS; k++) {
        const int t = t0 - k;
        const int64_t at = (int64_t)(t > 0 ? t : 0) * N + e;
        w[k].r = X.rewards[at]; w[k].v = X.values[at]; w[k].d = X.dones[at]; w[k].to = X.time_outs[at];
      }
    };
    auto work = [&](const ScanRow(&w)[ROWS], int t0, auto whole) {
#pragma unroll
      for (int k = 0; k < ROWS; k++) {
        const int t = t0 - k;
        if (decltype(whole)::value || t >= 0) {                        // (uniform)
          const int64_t at = (int64_t)t * N + e;
          const float v = w[k].v;
          const float r = w[k].to ? v : w[k].r;                        // runner.py:135
          X.rewards[at] = r;
          const float nn = (w[k].d | w[k].to) ? 0.0f : 1.0f;           // runner.py:138, utils.py:37
          const float delta = (r + (X.g * nn) * nv) - v;               // utils.py:42
          last = delta + (X.gl * nn) * last;                           // utils.py:43
          if (ALL || X.adv) X.adv[at] = last;
          if (ALL || X.ret) X.ret[at] = v + last;                      // runner.py:144
          const double dl = (double)last;
          s1 = s1 + dl;
          s2 = s2 + dl * dl;
          nv = v;
        }
      }
    };
    auto chunk = [&](const ScanRow(&w)[ROWS], int t0) {
      if (t0 >= ROWS - 1) work(w, t0, std::true_type{});
      else if (t0 >= 0) work(w, t0, std::false_type{});
    };
    request(a, H - 1);
    for (int t0 = H - 1; t0 >= 0; t0 -= 2 * ROWS) {
      request(b, t0 - ROWS);
      chunk(a, t0);
      request(a, t0 - 2 * ROWS);
      chunk(b, t0 - ROWS);
    }
  }
  if (!X.part) return;                                               // (uniform)
  // the group's pair: x[i] = x[i] + x[i + s], s = 1, 2, 4, ..; an absent environment holds +0
#pragma unroll
  for (int s = 1; s < ENVS; s <<= 1) {
    s1 = s1 + __shfl_down(s1, s, ENVS);
    s2 = s2 + __shfl_down(s2, s, ENVS);
  }
  if (threadIdx.x == 0) {
    X.part[(int64_t)blockIdx.x * 2] = s1;
    X.part[(int64_t)blockIdx.x * 2 + 1] = s2;
  }
}

// S1, S2 from +0 in rising group order, then the mean and torch's unbiased deviation in double
__device__ __forceinline__ void rollout_stats(double S1, double S2, double M, double* out) {
  const double mean = __ddiv_rn(S1, M);
  const double var = __ddiv_rn(S2 - __ddiv_rn(S1 * S1, M), M - 1.0);
  out[0] = S1; out[1] = S2; out[2] = mean; out[3] = __dsqrt_rn(var);
}

// beyond FOLD groups: ONE workgroup; a tile of 512 groups is loaded side by side (one memory latency per tile), then added in order
__global__ __launch_bounds__(1024) void tracker_rollout_chain_kernel(const double* __restrict__ part, int groups, double M, double* sums, double* stats) {
  __shared__ double s_part[1024];
  double S1 = 0.0, S2 = 0.0;
  for (int base = 0; base < groups; base += 512) {
    const int n = min(512, groups - base);
    if ((int)threadIdx.x < 2 * n) s_part[threadIdx.x] = part[(int64_t)base * 2 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int q = 0; q < n; q++) {
        S1 = S1 + s_part[2 * q];
        S2 = S2 + s_part[2 * q + 1];
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double st[4];
    rollout_stats(S1, S2, M, st);
    for (int k = 0; k < 4; k++) {
      sums[k] = st[k];
      if (stats) stats[k] = st[k];
    }
  }
}

// groups > 0: the partials are chained here, by every workgroup alike, and workgroup 0 writes stats; groups = 0: sums holds the four.
// out may be adv itself: element i is read, then written, by one lane.
__global__ __launch_bounds__(256) void tracker_rollout_normalize_kernel(const float* adv, float* out, int64_t M,
                                                                        const double* __restrict__ part, int groups,
                                                                        const double* __restrict__ sums, double* stats) {
  __shared__ double s_part[2 * FOLD];
  double st[4];
  if (groups > 0) {                                                  // (uniform)
    if ((int)threadIdx.x < 2 * groups) s_part[threadIdx.x] = part[threadIdx.x];
    __syncthreads();
    double S1 = 0.0, S2 = 0.0;
    for (int q = 0; q < groups; q++) {
      S1 = S1 + s_part[2 * q];
      S2 = S2 + s_part[2 * q + 1];
    }
    rollout_stats(S1, S2, (double)M, st);
    if (stats && blockIdx.x == 0 && threadIdx.x < 4) stats[threadIdx.x] = st[threadIdx.x];
  } else {
    st[2] = sums[2]; st[3] = sums[3];
  }
  if (!out) return;
  const float mean = (float)st[2], den = (float)st[3] + 1e-8f;       // runner.py:145
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) out[i] = __fdiv_rn(adv[i] - mean, den);
}

static int advantages_check(const RolloutTables& R, int N, const gmr_rollout_io_t* io, const float* values, const float* last_values,
                            const gmr_rollout_out_t* out, int normalize) {
  if (R.H == 0) return gmr_fail(GMR_ERR_ARG, "the rollout is not set on this tracker (gmr_motion_tracker_set_rollout)");
  if (normalize != 0 && normalize != 1) return gmr_fail(GMR_ERR_ARG, "normalize = %d, must be 0 or 1", normalize);
  if (!io || !out) return gmr_fail(GMR_ERR_ARG, "null io / output table");
  if (!io->rewards || !io->dones || !io->time_outs) return gmr_fail(GMR_ERR_ARG, "null rewards / dones / time_outs");
  if (!values || !last_values) return gmr_fail(GMR_ERR_ARG, "null values / last_values");
  if (normalize && (int64_t)R.H * N < 2)
    return gmr_fail(GMR_ERR_ARG, "normalize with H * N = %lld: the unbiased deviation needs two advantages", (long long)R.H * N);
  return GMR_OK;
}

static int advantages_launch(const RolloutTables& R, int N, const gmr_rollout_io_t* io, const float* values, const float* last_values,
                             const gmr_rollout_out_t* out, int normalize, hipStream_t stream) {
  const int rc = advantages_check(R, N, io, values, last_values, out, normalize);
  if (rc != GMR_OK) return rc;
  const int groups = (N + ENVS - 1) / ENVS;
  const int64_t M = (int64_t)R.H * N;
  const bool sums = normalize && (out->normalized || out->stats);
  // the outputs overlap neither one another nor an input (include/gmr_hip.h N14: the scan requests rows ahead of its stores);
  // without an advantages array the raw ones pass through the normalised one
  float* adv = out->advantages ? out->advantages : (sums ? out->normalized : nullptr);
  const ScanArgs X{io->rewards, io->dones, io->time_outs, values, last_values, adv, out->returns, sums ? R.part : nullptr, R.H, N, R.g, R.gl};
  if (X.adv && X.ret) hipLaunchKernelGGL(tracker_rollout_scan_kernel<true>, dim3((unsigned)groups), dim3(ENVS), 0, stream, X);
  else hipLaunchKernelGGL(tracker_rollout_scan_kernel<false>, dim3((unsigned)groups), dim3(ENVS), 0, stream, X);
  if (sums) {
    const bool fold = groups <= FOLD;
    if (!fold) hipLaunchKernelGGL(tracker_rollout_chain_kernel, dim3(1), dim3(1024), 0, stream, R.part, groups, (double)M, R.sums, out->stats);
    if (fold || out->normalized) {
      const int64_t blocks = out->normalized ? (M + 255) / 256 : 1;
      hipLaunchKernelGGL(tracker_rollout_normalize_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, adv, out->normalized, M,
                         R.part, fold ? groups : 0, R.sums, fold ? out->stats : nullptr);
    }
  }
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker rollout") --------------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_rollout(gmr_motion_tracker_t* t, int horizon, int obs_cols, int priv_cols, int act_cols, double gamma, double lam) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (horizon < 1) return gmr_fail(GMR_ERR_ARG, "horizon = %d, at least 1 needed", horizon);
  if (obs_cols < 1 || act_cols < 1 || priv_cols < 0)
    return gmr_fail(GMR_ERR_ARG, "obs_cols = %d and act_cols = %d must be at least 1, priv_cols = %d at least 0", obs_cols, act_cols, priv_cols);
  if (!std::isfinite(gamma) || !std::isfinite(lam) || gamma < 0.0 || gamma > 1.0 || lam < 0.0 || lam > 1.0)
    return gmr_fail(GMR_ERR_ARG, "gamma = %g and lam = %g must be finite and in [0, 1]", gamma, lam);
  gmr::RolloutTables R;
  R.H = horizon; R.O = obs_cols; R.P = priv_cols; R.A = act_cols;
  R.gamma = gamma; R.lam = lam;
  R.g = (float)gamma; R.gl = (float)(gamma * lam);
  std::lock_guard<std::mutex> g(t->mu);
  const size_t groups = ((size_t)t->N + gmr::ENVS - 1) / gmr::ENVS;
  gmr::Carve cv;
  const size_t o_part = cv.take(groups * 16), o_sums = cv.take(32);
  const int rc = gmr::fresh_block(t->rollout_block, cv);
  if (rc != GMR_OK) return rc;
  char* d = t->rollout_block.data();
  R.part = (double*)(d + o_part);
  R.sums = (double*)(d + o_sums);
  t->rollout = R;
  return GMR_OK;
}

int gmr_motion_tracker_record_dev(gmr_motion_tracker_t* t, int n, const gmr_rollout_io_t* io, const float* d_obs, const float* d_priv,
                                  const float* d_actions, const float* d_reward, const int32_t* d_done, const int32_t* d_time_outs, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::RolloutTables R;
  {
    std::lock_guard<std::mutex> g(t->mu);
    R = t->rollout;
  }
  const int rc = gmr::record_check(R, n, io, d_obs, d_priv, d_actions, d_reward, d_done, d_time_outs);
  if (rc != GMR_OK) return rc;
  const size_t row = (size_t)n * (size_t)t->N;
  const gmr::RecordSlots S{d_obs ? io->obs + row * R.O : nullptr, d_priv ? io->priv + row * R.P : nullptr, d_actions ? io->actions + row * R.A : nullptr,
                           d_reward ? io->rewards + row : nullptr, d_done ? io->dones + row : nullptr, d_time_outs ? io->time_outs + row : nullptr};
  return gmr::record_launch(R, t->N, S, d_obs, d_priv, d_actions, d_reward, d_done, d_time_outs, (hipStream_t)stream);
}

int gmr_motion_tracker_record(gmr_motion_tracker_t* t, int n, const gmr_rollout_io_t* io, const float* obs, const float* priv, const float* actions,
                              const float* reward, const int32_t* done, const int32_t* time_outs) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::RolloutTables R = t->rollout;
  int rc = gmr::record_check(R, n, io, obs, priv, actions, reward, done, time_outs);
  if (rc != GMR_OK) return rc;
  const size_t N = (size_t)t->N, row = (size_t)n * N;
  gmr::HostStage st;
  const float *d_obs, *d_priv, *d_actions, *d_reward;
  const int32_t *d_done, *d_touts;
  gmr::RecordSlots S = {};
  st.in(d_obs, obs, N * R.O * 4); st.in(d_priv, priv, N * R.P * 4); st.in(d_actions, actions, N * R.A * 4);
  st.in(d_reward, reward, N * 4); st.in(d_done, done, N * 4); st.in(d_touts, time_outs, N * 4);
  // slot n alone of every array that has an input: the kernel writes it whole
  st.out(S.obs, obs ? io->obs + row * R.O : nullptr, N * R.O * 4); st.out(S.priv, priv ? io->priv + row * R.P : nullptr, N * R.P * 4);
  st.out(S.actions, actions ? io->actions + row * R.A : nullptr, N * R.A * 4); st.out(S.rewards, reward ? io->rewards + row : nullptr, N * 4);
  st.out(S.dones, done ? io->dones + row : nullptr, N); st.out(S.time_outs, time_outs ? io->time_outs + row : nullptr, N);
  GMR_STAGE_TRY(st, upload);
  rc = gmr::record_launch(R, t->N, S, d_obs, d_priv, d_actions, d_reward, d_done, d_touts, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_tracker_advantages_dev(gmr_motion_tracker_t* t, const gmr_rollout_io_t* io, const float* d_values, const float* d_last_values,
                                      const gmr_rollout_out_t* out, int normalize, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::RolloutTables R;
  {
    std::lock_guard<std::mutex> g(t->mu);
    R = t->rollout;
  }
  return gmr::advantages_launch(R, t->N, io, d_values, d_last_values, out, normalize, (hipStream_t)stream);
}

int gmr_motion_tracker_advantages(gmr_motion_tracker_t* t, const gmr_rollout_io_t* io, const float* values, const float* last_values,
                                  const gmr_rollout_out_t* out, int normalize) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::RolloutTables R = t->rollout;
  int rc = gmr::advantages_check(R, t->N, io, values, last_values, out, normalize);
  if (rc != GMR_OK) return rc;
  const size_t N = (size_t)t->N, M = (size_t)R.H * N;
  gmr::HostStage st;
  gmr_rollout_io_t d = {};
  gmr_rollout_out_t dout = {};
  const float *d_values, *d_last;
  // rewards are the caller's rows: copied in here, copied back whole below
  st.in(d.rewards, io->rewards, M * 4); st.in(d.dones, io->dones, M); st.in(d.time_outs, io->time_outs, M);
  st.in(d_values, values, M * 4); st.in(d_last, last_values, N * 4);
  st.out(dout.advantages, out->advantages, M * 4); st.out(dout.returns, out->returns, M * 4);
  st.out(dout.normalized, normalize ? out->normalized : nullptr, M * 4); st.out(dout.stats, normalize ? out->stats : nullptr, 32);
  GMR_STAGE_TRY(st, upload);
  rc = gmr::advantages_launch(R, t->N, &d, d_values, d_last, &dout, normalize, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  GMR_HIP_TRY(hipMemcpy(io->rewards, d.rewards, M * 4, hipMemcpyDeviceToHost));
  return GMR_OK;
}

}  // extern "C"
