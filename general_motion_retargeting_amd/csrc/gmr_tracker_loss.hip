// gmr_tracker_loss.hip -- the PPO loss head of a training iteration on the motion tracker: what the reference's
// runner does between the outputs of its two networks and its optimiser.  old_actions_log_prob (booster_gym/utils/runner.py:123-125); the
// value, surrogate, bound and entropy terms and their sum (:146-161, utils/utils.py:47-52); the backward pass of that sum down to loc,
// logstd and values (what :163 delivers at the outputs of the networks); the KL between the old and the new policy (:168-174) and the
// learning-rate rule it drives (:175-178).  The statement of record is tests/ppo_mirror.py.
//
//   tracker_loss_kernel       ONE workgroup per group of GMR_LOSS_ROWS rows.  The group's tile of every [M][A] array is a run of
//                             ROWS * A consecutive floats that starts on 256 bytes of its array: it is read once, coalesced over the
//                             flat floats (16 bytes per lane where the arrays are 16-byte aligned, floats else).  A lane keeps d and loc
//                             of its elements in registers and puts the per-element log-probability, KL and bound squares into LDS
//                             (row stride A | 1: odd); one lane per row adds them over rising a and makes the row's ratio, weight and
//                             surrogate; every lane then writes the grad_loc of its own elements, coalesced again, and the per-element
//                             products behind grad_logstd go through the row tree in LDS.  Instances: log-probability alone; the loss
//                             with / without grad_loc, with / without the sums, with / without the KL -- no test per element.
//   tracker_loss_fold_kernel  ONE workgroup: the groups' partial sums by blocks of GMR_LOSS_FOLD (a wavefront's tree each), the blocks in
//                             rising order; writes terms and grad_logstd and steps the learning rate
//
// The arrays are the caller's; the partial sums and the learning rate belong to the tracker; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/ppo_mirror.py states every line in float32 (the sums in float64) NumPy
#pragma clang fp contract(off)

namespace gmr {

constexpr int LROWS = GMR_LOSS_ROWS;        // rows per group: one workgroup
constexpr int LFOLD = GMR_LOSS_FOLD;        // groups per block of the fold: one wavefront
constexpr int MAXA = GMR_LOSS_MAX_ACT;
constexpr int LTHREADS = 256;
constexpr int ROWK = 6;                     // the row-level sums: value, surrogate, bound above, bound below, kl, clipped rows
constexpr int KMAX = MAXA + ROWK;
constexpr int LSTRIDE = MAXA + 1;           // the largest row stride in LDS
static_assert(LROWS == 64 && LFOLD == 64, "the trees are written for 64 rows and for the wavefront");
static_assert((LROWS * 4) % 16 == 0, "a group of any A starts on 16 bytes");

enum : int { L_GRAD = 1, L_SUMS = 2, L_KL = 4, L_LOSS = 8 };   // L_LOSS absent: the log-probability alone

struct LossArgs {
  const float *loc, *logstd, *actions;      // [M][A], [A], [M][A]
  const float *old_lp, *values, *returns, *adv;      // [M]
  const float *old_loc, *old_logstd;        // [M][A], [A] or null
  float *grad_loc, *grad_values, *log_prob; // [M][A], [M], [M] or null
  double* part;                             // [A + ROWK][G]
  int64_t M, G;
  int A;
  float Mf, lo, hi, cb, C0;
};

// float32 exp and log with ONE rounding: formed in double, rounded once (a few lanes per workgroup pay for it, no element does)
__device__ __forceinline__ float exp_once(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float log_once(float x) { return (float)log((double)x); }

// the per-column quantities: the reference takes the log of the exp (torch.distributions.Normal: scale.log())
__device__ __forceinline__ void loss_column(float logstd, float& scale, float& var, float& log_scale) {
  scale = exp_once(logstd);
  var = scale * scale;
  log_scale = log_once(scale);
}

// Normal.log_prob of one element
__device__ __forceinline__ float log_prob_element(float d, float two_var, float log_scale, float C0) {
  return (__fdiv_rn(-(d * d), two_var) - log_scale) - C0;
}

template <bool VEC, int MODE>
__global__ __launch_bounds__(LTHREADS) void tracker_loss_kernel(const LossArgs X) {
  constexpr bool GRAD = (MODE & L_GRAD) != 0, SUMS = (MODE & L_SUMS) != 0, KL = (MODE & L_KL) != 0, LOSS = (MODE & L_LOSS) != 0;
  constexpr int W = VEC ? 4 : 1;
  constexpr int PASSES = LROWS * MAXA / (LTHREADS * W);
  constexpr int NF = 1 + (KL ? 1 : 0) + (SUMS ? 2 : 0);              // float arrays of the tile
  constexpr int PLANE = LROWS * LSTRIDE;
  static_assert(!SUMS || NF * PLANE * 4 >= LROWS * MAXA * 8, "the products behind grad_logstd reuse the tile's space");
  __shared__ __align__(16) float s_tile[NF * PLANE];
  __shared__ float s_var[MAXA], s_two_var[MAXA], s_log_scale[MAXA], s_log_ratio[KL ? MAXA : 1], s_old_var[KL ? MAXA : 1];
  __shared__ float s_glp[LOSS ? LROWS : 1];
  __shared__ double s_row[SUMS ? LROWS * ROWK : 1];
  float* const s_lp = s_tile;
  float* const s_kl = s_tile + (KL ? PLANE : 0);
  float* const s_bh = s_tile + (SUMS ? (NF - 2) * PLANE : 0);
  float* const s_bl = s_tile + (SUMS ? (NF - 1) * PLANE : 0);
  double* const s_prod = reinterpret_cast<double*>(s_tile);          // [LROWS][A] after the rows are done with the tile

  const int tid = threadIdx.x;
  const int A = X.A, AP = A | 1;
  const int64_t row0 = (int64_t)blockIdx.x * LROWS;
  const int rows = (int)(X.M - row0 < LROWS ? X.M - row0 : LROWS);
  const int cnt = rows * A;                                           // floats of the tile
  const int64_t base = row0 * A;

  // ---- 1. the elements, flat: the loads of the tile are issued first, the per-column quantities are made under them --------------------
  float d[PASSES][W], lc[PASSES][W], ol[PASSES][W];
#pragma unroll
  for (int p = 0; p < PASSES; p++) {
    const int f0 = (p * LTHREADS + tid) * W;
#pragma unroll
    for (int j = 0; j < W; j++) {
      lc[p][j] = d[p][j] = 0.0f;                                      // (d holds the action until the difference is taken)
      if (KL) ol[p][j] = 0.0f;
    }
    if (VEC && f0 + W <= cnt) {
      const float4 l4 = *reinterpret_cast<const float4*>(X.loc + base + f0), a4 = *reinterpret_cast<const float4*>(X.actions + base + f0);
      lc[p][0] = l4.x; lc[p][W > 1 ? 1 : 0] = l4.y; lc[p][W > 2 ? 2 : 0] = l4.z; lc[p][W > 3 ? 3 : 0] = l4.w;
      d[p][0] = a4.x; d[p][W > 1 ? 1 : 0] = a4.y; d[p][W > 2 ? 2 : 0] = a4.z; d[p][W > 3 ? 3 : 0] = a4.w;
      if (KL) {
        const float4 o4 = *reinterpret_cast<const float4*>(X.old_loc + base + f0);
        ol[p][0] = o4.x; ol[p][W > 1 ? 1 : 0] = o4.y; ol[p][W > 2 ? 2 : 0] = o4.z; ol[p][W > 3 ? 3 : 0] = o4.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < W; j++)
        if (f0 + j < cnt) {
          lc[p][j] = X.loc[base + f0 + j]; d[p][j] = X.actions[base + f0 + j];
          if (KL) ol[p][j] = X.old_loc[base + f0 + j];
        }
    }
  }

  if (tid < A) {                                                      // once per workgroup
    float scale, var, ls;
    loss_column(X.logstd[tid], scale, var, ls);
    s_var[tid] = var; s_two_var[tid] = 2.0f * var; s_log_scale[tid] = ls;
    if (KL) {
      float oscale, ovar, ols;
      loss_column(X.old_logstd[tid], oscale, ovar, ols);
      s_log_ratio[tid] = log_once(__fdiv_rn(scale, oscale));
      s_old_var[tid] = ovar;
    }
  }
  __syncthreads();

#pragma unroll
  for (int p = 0; p < PASSES; p++) {
    const int f0 = (p * LTHREADS + tid) * W;
    float l[W], o[W];
#pragma unroll
    for (int j = 0; j < W; j++) {
      l[j] = lc[p][j];
      o[j] = KL ? ol[p][j] : 0.0f;
    }
    int r = f0 / A, c = f0 - r * A;
#pragma unroll
    for (int j = 0; j < W; j++) {
      d[p][j] = d[p][j] - l[j];
      if (f0 + j < cnt) {
        const int at = r * AP + c;
        s_lp[at] = log_prob_element(d[p][j], s_two_var[c], s_log_scale[c], X.C0);
        if (KL) {                                                     // runner.py:169-171
          const float dl = l[j] - o[j];
          const float h = 0.5f * (s_old_var[c] + dl * dl);
          s_kl[at] = (s_log_ratio[c] + __fdiv_rn(h, s_var[c])) - 0.5f;
        }
        if (SUMS) {                                                   // runner.py:152
          const float m1 = fmaxf(l[j] - 1.0f, 0.0f), m2 = fminf(l[j] + 1.0f, 0.0f);
          s_bh[at] = m1 * m1; s_bl[at] = m2 * m2;
        }
      }
      if (++c == A) { c = 0; r++; }
    }
  }
  __syncthreads();

  // ---- 2. the rows ----------------------------------------------------------------------------------------------------------------
  if (tid < LROWS) {
    const int64_t R = row0 + tid;
    if (tid < rows) {
      const int at = tid * AP;
      float lp = s_lp[at];
      for (int a = 1; a < A; a++) lp = lp + s_lp[at + a];
      if (X.log_prob) X.log_prob[R] = lp;                             // (uniform)
      if (LOSS) {
        const float ratio = expf(lp - X.old_lp[R]);                   // utils.py:48-51
        const float na = -X.adv[R];
        const float s = na * ratio;
        const float sc = na * fminf(fmaxf(ratio, X.lo), X.hi);
        const float surr = fmaxf(s, sc);
        // what torch's backward of max and clamp leaves on the row: inside the closed interval sc is s bit for bit, a tie with both
        // halves alive; outside, the clamp passes nothing on
        const float w = (ratio >= X.lo && ratio <= X.hi) ? 1.0f : (s > sc ? 1.0f : (s == sc ? 0.5f : 0.0f));
        s_glp[tid] = __fdiv_rn(w * s, X.Mf);
        const float dv = X.values[R] - X.returns[R];
        if (X.grad_values) X.grad_values[R] = __fdiv_rn(2.0f * dv, X.Mf);      // (uniform)
        if (SUMS) {
          double bh = 0.0, bl = 0.0;
          for (int a = 0; a < A; a++) {
            bh = bh + (double)s_bh[at + a];
            bl = bl + (double)s_bl[at + a];
          }
          double kl = 0.0;
          if (KL) {
            float k = s_kl[at];
            for (int a = 1; a < A; a++) k = k + s_kl[at + a];
            kl = (double)k;
          }
          double* o = s_row + tid * ROWK;
          o[0] = (double)(dv * dv); o[1] = (double)surr; o[2] = bh; o[3] = bl; o[4] = kl; o[5] = w == 0.0f ? 1.0 : 0.0;
        }
      }
    } else if (LOSS) {                                                // an absent row holds +0
      s_glp[tid] = 0.0f;
      if (SUMS)
        for (int k = 0; k < ROWK; k++) s_row[tid * ROWK + k] = 0.0;
    }
  }
  if (!LOSS) return;
  __syncthreads();

  // ---- 3. the gradient of the elements, flat again --------------------------------------------------------------------------------
  if (GRAD || SUMS) {
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      const int f0 = (p * LTHREADS + tid) * W;
      int r = f0 / A, c = f0 - r * A;
      float g[W];
#pragma unroll
      for (int j = 0; j < W; j++) {
        g[j] = 0.0f;
        if (f0 + j < cnt) {
          const float glp = s_glp[r], var = s_var[c];
          if (GRAD) {
            const float m1 = fmaxf(lc[p][j] - 1.0f, 0.0f), m2 = fminf(lc[p][j] + 1.0f, 0.0f);
            g[j] = glp * __fdiv_rn(d[p][j], var) + X.cb * (2.0f * m1 + 2.0f * m2);
          }
          if (SUMS) s_prod[f0 + j] = (double)glp * (double)(__fdiv_rn(d[p][j] * d[p][j], var) - 1.0f);
        } else if (SUMS && f0 + j < LROWS * A) {
          s_prod[f0 + j] = 0.0;
        }
        if (++c == A) { c = 0; r++; }
      }
      if (GRAD) {
        if (VEC && f0 + W <= cnt) {
          *reinterpret_cast<float4*>(X.grad_loc + base + f0) = make_float4(g[0], g[W > 1 ? 1 : 0], g[W > 2 ? 2 : 0], g[W > 3 ? 3 : 0]);
        } else {
#pragma unroll
          for (int j = 0; j < W; j++)
            if (f0 + j < cnt) X.grad_loc[base + f0 + j] = g[j];
        }
      }
    }
  }
  if (!SUMS) return;

  // ---- 4. the rows of the group by the balanced tree x[i] = x[i] + x[i + s], every column alike -----------------------------------
  const int K = A + ROWK;
  for (int s = 1; s < LROWS; s <<= 1) {
    __syncthreads();
    const int items = (LROWS / (2 * s)) * K;
    for (int idx = tid; idx < items; idx += LTHREADS) {
      const int q = idx / K, k = idx - q * K, i = q * 2 * s;
      if (k < ROWK) s_row[i * ROWK + k] = s_row[i * ROWK + k] + s_row[(i + s) * ROWK + k];
      else s_prod[i * A + (k - ROWK)] = s_prod[i * A + (k - ROWK)] + s_prod[(i + s) * A + (k - ROWK)];
    }
  }
  __syncthreads();
  if (tid < K) X.part[(int64_t)tid * X.G + blockIdx.x] = tid < ROWK ? s_row[tid] : s_prod[tid - ROWK];
}

struct FoldArgs {
  const double* part;                       // [A + ROWK][G]
  const float* logstd;                      // [A]
  double* lr;                               // [1] the tracker's
  double* terms;                            // [8] or null
  float* grad_logstd;                       // [A] or null
  int64_t M, G;
  int A, update_lr, has_kl;
  float E0;
  double bound_coef, entropy_coef, desired_kl, lr_min, lr_max, lr_factor;
};

// Wavefront w of a round takes block b0 + w: lane i holds group b * LFOLD + i of every column (an absent group +0), six __shfl_down
// steps are the tree; then the blocks of the round are added in rising order, one lane per column.
__global__ __launch_bounds__(1024) void tracker_loss_fold_kernel(const FoldArgs X) {
  constexpr int WAVES = 16;
  __shared__ double s_blk[WAVES][KMAX];
  __shared__ double s_tot[KMAX];
  __shared__ float s_ls[MAXA];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = X.A, K = A + ROWK;
  const int64_t B = (X.G + LFOLD - 1) / LFOLD;
  double tot = 0.0;
  for (int64_t b0 = 0; b0 < B; b0 += WAVES) {
    const int64_t b = b0 + wave;
    if (b < B) {                                                      // (uniform in the wavefront)
      const int64_t g = b * LFOLD + lane;
      double v[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; k++) v[k] = (k < K && g < X.G) ? X.part[(int64_t)k * X.G + g] : 0.0;
#pragma unroll
      for (int k = 0; k < KMAX; k++) {
        if (k < K) {                                                  // (uniform)
          double x = v[k];
#pragma unroll
          for (int s = 1; s < LFOLD; s <<= 1) x = x + __shfl_down(x, s, LFOLD);
          if (lane == 0) s_blk[wave][k] = x;
        }
      }
    }
    __syncthreads();
    if (tid < K) {
      const int n = (int)(B - b0 < WAVES ? B - b0 : WAVES);
      for (int w = 0; w < n; w++) tot = tot + s_blk[w][tid];
    }
    __syncthreads();
  }
  if (tid < K) s_tot[tid] = tot;
  if (tid < A) {
    float scale, var, ls;
    loss_column(X.logstd[tid], scale, var, ls);
    s_ls[tid] = ls;
  }
  __syncthreads();
  if (X.grad_logstd && tid < A) X.grad_logstd[tid] = (float)(s_tot[ROWK + tid] + X.entropy_coef);
  if (tid != 0) return;
  const double Md = (double)X.M, MA = (double)X.M * (double)A;
  const double value_loss = __ddiv_rn(s_tot[0], Md), actor_loss = __ddiv_rn(s_tot[1], Md);
  const double bound_loss = __ddiv_rn(s_tot[2], MA) + __ddiv_rn(s_tot[3], MA);
  double entropy = 0.0;
  for (int a = 0; a < A; a++) entropy = entropy + (double)(X.E0 + s_ls[a]);      // runner.py:154
  const double loss = ((value_loss + actor_loss) + X.bound_coef * bound_loss) + X.entropy_coef * entropy;      // runner.py:156-161
  const double kl_mean = X.has_kl ? __ddiv_rn(s_tot[4], Md) : 0.0;
  double lr = *X.lr;
  if (X.update_lr) {                                                  // runner.py:175-178, the comparison in double
    if (kl_mean > X.desired_kl * 2.0) lr = fmax(X.lr_min, __ddiv_rn(lr, X.lr_factor));
    else if (kl_mean < X.desired_kl * 0.5) lr = fmin(X.lr_max, lr * X.lr_factor);
    *X.lr = lr;
  }
  if (X.terms) {
    X.terms[0] = value_loss; X.terms[1] = actor_loss; X.terms[2] = bound_loss; X.terms[3] = entropy; X.terms[4] = loss;
    X.terms[5] = kl_mean; X.terms[6] = lr; X.terms[7] = __ddiv_rn(s_tot[5], Md);
  }
}

template <int MODE>
static void loss_kernel_launch(bool vec, const LossArgs& X, hipStream_t stream) {
  if (vec) hipLaunchKernelGGL((tracker_loss_kernel<true, MODE>), dim3((unsigned)X.G), dim3(LTHREADS), 0, stream, X);
  else hipLaunchKernelGGL((tracker_loss_kernel<false, MODE>), dim3((unsigned)X.G), dim3(LTHREADS), 0, stream, X);
}

// the configuration still belongs to the rollout it was made for
static int loss_ready(const LossTables& L, const RolloutTables& R, int N) {
  if (!L.on) return gmr_fail(GMR_ERR_ARG, "the loss is not set on this tracker (gmr_motion_tracker_set_loss)");
  if (L.M != (int64_t)R.H * N || L.A != R.A)
    return gmr_fail(GMR_ERR_ARG, "the rollout was set again after the loss (%lld rows of %d, now %lld of %d): call gmr_motion_tracker_set_loss again",
                    (long long)L.M, L.A, (long long)R.H * N, R.A);
  return GMR_OK;
}

static LossArgs loss_args(const LossTables& L) {
  LossArgs X = {};
  X.M = L.M; X.A = L.A; X.G = (L.M + LROWS - 1) / LROWS;
  X.Mf = (float)L.M;
  X.lo = (float)(1.0 - L.e_clip); X.hi = (float)(1.0 + L.e_clip);
  X.cb = (float)(L.bound_coef / ((double)L.M * (double)L.A));
  X.C0 = (float)std::log(std::sqrt(2.0 * M_PI));
  X.part = L.part;
  return X;
}

static int log_prob_launch(const LossTables& L, const RolloutTables& R, int N, const float* loc, const float* logstd, const float* actions, float* out,
                           hipStream_t stream) {
  const int rc = loss_ready(L, R, N);
  if (rc != GMR_OK) return rc;
  if (!loc || !logstd || !actions || !out) return gmr_fail(GMR_ERR_ARG, "null loc / logstd / actions / out");
  LossArgs X = loss_args(L);
  X.loc = loc; X.logstd = logstd; X.actions = actions; X.log_prob = out;
  loss_kernel_launch<0>(aligned16(loc) && aligned16(actions), X, stream);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

static int loss_check(const LossTables& L, const RolloutTables& R, int N, const gmr_loss_in_t* in, const gmr_loss_out_t* out, int update_lr) {
  const int rc = loss_ready(L, R, N);
  if (rc != GMR_OK) return rc;
  if (update_lr != 0 && update_lr != 1) return gmr_fail(GMR_ERR_ARG, "update_lr = %d, must be 0 or 1", update_lr);
  if (!in || !out) return gmr_fail(GMR_ERR_ARG, "null input / output table");
  if (!in->loc || !in->logstd || !in->actions || !in->old_log_prob || !in->values || !in->returns || !in->advantages)
    return gmr_fail(GMR_ERR_ARG, "null loc / logstd / actions / old_log_prob / values / returns / advantages");
  if ((in->old_loc == nullptr) != (in->old_logstd == nullptr)) return gmr_fail(GMR_ERR_ARG, "old_loc and old_logstd are given together, or both NULL");
  if (update_lr && !in->old_loc) return gmr_fail(GMR_ERR_ARG, "update_lr without old_loc and old_logstd: there is no KL to drive the learning rate");
  return GMR_OK;
}

static int loss_launch(const LossTables& L, const RolloutTables& R, int N, const gmr_loss_in_t* in, const gmr_loss_out_t* out, int update_lr,
                       hipStream_t stream) {
  const int rc = loss_check(L, R, N, in, out, update_lr);
  if (rc != GMR_OK) return rc;
  const bool sums = out->terms || out->grad_logstd || update_lr;
  const bool kl = sums && in->old_loc;
  if (!sums && !out->grad_loc && !out->grad_values && !out->log_prob) return GMR_OK;
  LossArgs X = loss_args(L);
  X.loc = in->loc; X.logstd = in->logstd; X.actions = in->actions;
  X.old_lp = in->old_log_prob; X.values = in->values; X.returns = in->returns; X.adv = in->advantages;
  X.old_loc = kl ? in->old_loc : nullptr; X.old_logstd = kl ? in->old_logstd : nullptr;
  X.grad_loc = out->grad_loc; X.grad_values = out->grad_values; X.log_prob = out->log_prob;
  const bool vec = aligned16(X.loc) && aligned16(X.actions) && aligned16(X.old_loc) && aligned16(X.grad_loc);
  switch ((X.grad_loc ? L_GRAD : 0) | (sums ? L_SUMS : 0) | (kl ? L_KL : 0)) {
    case 0: loss_kernel_launch<L_LOSS>(vec, X, stream); break;
    case L_GRAD: loss_kernel_launch<L_LOSS | L_GRAD>(vec, X, stream); break;
    case L_SUMS: loss_kernel_launch<L_LOSS | L_SUMS>(vec, X, stream); break;
    case L_GRAD | L_SUMS: loss_kernel_launch<L_LOSS | L_GRAD | L_SUMS>(vec, X, stream); break;
    case L_SUMS | L_KL: loss_kernel_launch<L_LOSS | L_SUMS | L_KL>(vec, X, stream); break;
    default: loss_kernel_launch<L_LOSS | L_GRAD | L_SUMS | L_KL>(vec, X, stream); break;
  }
  if (sums) {
    FoldArgs Y = {};
    Y.part = L.part; Y.logstd = in->logstd; Y.lr = L.lr; Y.terms = out->terms; Y.grad_logstd = out->grad_logstd;
    Y.M = X.M; Y.G = X.G; Y.A = X.A; Y.update_lr = update_lr; Y.has_kl = kl ? 1 : 0;
    Y.E0 = (float)(0.5 + 0.5 * std::log(2.0 * M_PI));
    Y.bound_coef = L.bound_coef; Y.entropy_coef = L.entropy_coef; Y.desired_kl = L.desired_kl;
    Y.lr_min = L.lr_min; Y.lr_max = L.lr_max; Y.lr_factor = L.lr_factor;
    hipLaunchKernelGGL(tracker_loss_fold_kernel, dim3(1), dim3(1024), 0, stream, Y);
  }
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker loss") ----------------------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_loss(gmr_motion_tracker_t* t, double bound_coef, double entropy_coef, double desired_kl, double learning_rate, double e_clip,
                                double lr_min, double lr_max, double lr_factor) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!std::isfinite(bound_coef) || !std::isfinite(entropy_coef)) return gmr_fail(GMR_ERR_ARG, "bound_coef = %g and entropy_coef = %g must be finite", bound_coef, entropy_coef);
  if (!std::isfinite(desired_kl) || desired_kl <= 0.0) return gmr_fail(GMR_ERR_ARG, "desired_kl = %g must be finite and above 0", desired_kl);
  if (!(e_clip > 0.0 && e_clip < 1.0)) return gmr_fail(GMR_ERR_ARG, "e_clip = %g must lie in (0, 1)", e_clip);
  if (!std::isfinite(lr_min) || !std::isfinite(lr_max) || lr_min <= 0.0 || lr_min > lr_max)
    return gmr_fail(GMR_ERR_ARG, "lr_min = %g and lr_max = %g must be finite with 0 < lr_min <= lr_max", lr_min, lr_max);
  if (!std::isfinite(lr_factor) || lr_factor < 1.0) return gmr_fail(GMR_ERR_ARG, "lr_factor = %g must be finite and at least 1", lr_factor);
  if (!std::isfinite(learning_rate) || learning_rate <= 0.0) return gmr_fail(GMR_ERR_ARG, "learning_rate = %g must be finite and above 0", learning_rate);
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::RolloutTables R = t->rollout;
  if (R.H == 0) return gmr_fail(GMR_ERR_ARG, "the rollout is not set on this tracker (gmr_motion_tracker_set_rollout): the loss takes its rows and columns from it");
  if (R.A > GMR_LOSS_MAX_ACT) return gmr_fail(GMR_ERR_ARG, "act_cols = %d, at most GMR_LOSS_MAX_ACT = %d", R.A, GMR_LOSS_MAX_ACT);
  gmr::LossTables L;
  L.M = (int64_t)R.H * t->N; L.A = R.A;
  if ((L.M + gmr::LROWS - 1) / gmr::LROWS > 0x7fffffffLL) return gmr_fail(GMR_ERR_ARG, "H * N = %lld rows are more groups than a launch takes", (long long)L.M);
  L.bound_coef = bound_coef; L.entropy_coef = entropy_coef; L.desired_kl = desired_kl; L.e_clip = e_clip;
  L.lr_min = lr_min; L.lr_max = lr_max; L.lr_factor = lr_factor;
  const size_t groups = (size_t)((L.M + gmr::LROWS - 1) / gmr::LROWS);
  gmr::Carve cv;
  const size_t o_part = cv.take(groups * (size_t)(L.A + gmr::ROWK) * 8), o_lr = cv.take(8);
  const int rc = gmr::fresh_block(t->loss_block, cv);
  if (rc != GMR_OK) return rc;
  char* d = t->loss_block.data();
  GMR_HIP_TRY(hipMemcpy(d + o_lr, &learning_rate, 8, hipMemcpyHostToDevice));
  GMR_HIP_TRY(hipDeviceSynchronize());
  L.part = (double*)(d + o_part);
  L.lr = (double*)(d + o_lr);
  L.on = 1;
  t->loss = L;
  return GMR_OK;
}

int gmr_motion_tracker_loss_state(gmr_motion_tracker_t* t, double* out) {
  if (!t || !out) return gmr_fail(GMR_ERR_ARG, "null motion tracker / out");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::LossTables L = t->loss;
  if (!L.on) return gmr_fail(GMR_ERR_ARG, "the loss is not set on this tracker (gmr_motion_tracker_set_loss)");
  GMR_HIP_TRY(hipDeviceSynchronize());
  out[0] = L.bound_coef; out[1] = L.entropy_coef; out[2] = L.desired_kl;
  GMR_HIP_TRY(hipMemcpy(out + 3, L.lr, 8, hipMemcpyDeviceToHost));
  out[4] = L.e_clip; out[5] = L.lr_min; out[6] = L.lr_max; out[7] = L.lr_factor;
  return GMR_OK;
}

int gmr_motion_tracker_log_prob_dev(gmr_motion_tracker_t* t, const float* d_loc, const float* d_logstd, const float* d_actions, float* d_out, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::LossTables L;
  gmr::RolloutTables R;
  {
    std::lock_guard<std::mutex> g(t->mu);
    L = t->loss; R = t->rollout;
  }
  return gmr::log_prob_launch(L, R, t->N, d_loc, d_logstd, d_actions, d_out, (hipStream_t)stream);
}

int gmr_motion_tracker_log_prob(gmr_motion_tracker_t* t, const float* loc, const float* logstd, const float* actions, float* out) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::LossTables L = t->loss;
  const gmr::RolloutTables R = t->rollout;
  int rc = gmr::loss_ready(L, R, t->N);
  if (rc != GMR_OK) return rc;
  if (!loc || !logstd || !actions || !out) return gmr_fail(GMR_ERR_ARG, "null loc / logstd / actions / out");
  const size_t M = (size_t)L.M, A = (size_t)L.A;
  gmr::HostStage st;
  const float *d_loc, *d_logstd, *d_actions;
  float* d_out;
  st.in(d_loc, loc, M * A * 4); st.in(d_logstd, logstd, A * 4); st.in(d_actions, actions, M * A * 4);
  st.out(d_out, out, M * 4);
  GMR_STAGE_TRY(st, upload);
  rc = gmr::log_prob_launch(L, R, t->N, d_loc, d_logstd, d_actions, d_out, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_tracker_loss_dev(gmr_motion_tracker_t* t, const gmr_loss_in_t* in, const gmr_loss_out_t* out, int update_lr, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::LossTables L;
  gmr::RolloutTables R;
  {
    std::lock_guard<std::mutex> g(t->mu);
    L = t->loss; R = t->rollout;
  }
  return gmr::loss_launch(L, R, t->N, in, out, update_lr, (hipStream_t)stream);
}

int gmr_motion_tracker_loss(gmr_motion_tracker_t* t, const gmr_loss_in_t* in, const gmr_loss_out_t* out, int update_lr) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::LossTables L = t->loss;
  const gmr::RolloutTables R = t->rollout;
  int rc = gmr::loss_check(L, R, t->N, in, out, update_lr);
  if (rc != GMR_OK) return rc;
  const size_t M = (size_t)L.M, A = (size_t)L.A;
  gmr::HostStage st;
  gmr_loss_in_t d = {};
  gmr_loss_out_t dout = {};
  st.in(d.loc, in->loc, M * A * 4); st.in(d.logstd, in->logstd, A * 4); st.in(d.actions, in->actions, M * A * 4);
  st.in(d.old_log_prob, in->old_log_prob, M * 4); st.in(d.values, in->values, M * 4); st.in(d.returns, in->returns, M * 4);
  st.in(d.advantages, in->advantages, M * 4); st.in(d.old_loc, in->old_loc, M * A * 4); st.in(d.old_logstd, in->old_logstd, A * 4);
  st.out(dout.grad_loc, out->grad_loc, M * A * 4); st.out(dout.grad_logstd, out->grad_logstd, A * 4); st.out(dout.grad_values, out->grad_values, M * 4);
  st.out(dout.log_prob, out->log_prob, M * 4); st.out(dout.terms, out->terms, 64);
  GMR_STAGE_TRY(st, upload);
  rc = gmr::loss_launch(L, R, t->N, &d, &dout, update_lr, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

}  // extern "C"
