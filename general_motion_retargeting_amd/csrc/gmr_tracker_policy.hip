// gmr_tracker_policy.hip -- the forward pass of the two networks of a training iteration on the motion tracker:
// model.act(obs).loc and .sample() (booster_gym/utils/model.py:29-32, runner.py:109-111, :123-124, the whole of Runner.play) and
// model.est_value(obs, privileged_obs) (model.py:34-36).  The statement of record is tests/policy_mirror.py.
//
//   tracker_policy_kernel<SAMPLE>   ONE workgroup of four wavefronts per GMR_POLICY_TILE = 32 rows, one launch per network per call.  The
//                                   input row block is staged into LDS (the critic's from two arrays side by side, the width padded with
//                                   zeros to a multiple of eight), and the activations stay there from the first layer to the last in two
//                                   buffers a layer reads and the next one writes.  A hidden layer runs on v_mfma_f32_32x32x2_f32: a
//                                   wavefront owns output columns 32 c .. 32 c + 31 for c = wave, wave + 4, the activations are the A operand
//                                   from LDS, W^T the B operand straight from global memory (the weights stay in L2), four consecutive k per
//                                   lane and load; bias and ELU in the epilogue, out of the accumulator.  The last layer (at most 32
//                                   outputs, the critic's one) runs on the vector ALU, an output element per lane.  <true> adds the sampled
//                                   action and advances the counts.
//
// The parameters are the caller's and travel by address in the kernel arguments; the counts belong to the tracker; the tracker stays
// single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_tracker_dev.h"
#include "gmr_tracker_host.h"
#include "gmr_tracker_policy_plan.h"
#include "gmr_workspace.h"

// one rounding per operation on the elementwise lines: tests/policy_mirror.py states them in float32 NumPy (the sums are explicit fmaf
// chains and the matrix instruction's, which are the same thing)
#pragma clang fp contract(off)

namespace gmr {

constexpr int PT = GMR_POLICY_TILE;         // rows per workgroup: the M of one matrix instruction
constexpr int PMAXL = GMR_POLICY_MAX_HIDDEN;
constexpr int PTHREADS = 256;
constexpr int PWAVES = PTHREADS / 64;
constexpr int PKB = 8;                      // k per operand load: four consecutive ones in either half of the wavefront
static_assert(PT == 32 && GMR_POLICY_WIDTH_STEP == 32, "a column tile and the row tile are the 32 x 32 of v_mfma_f32_32x32x2_f32");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct PolicyArgs {
  const float* W[PMAXL + 1];                // [width[l + 1]][width[l]]
  const float* b[PMAXL + 1];                // [width[l + 1]]
  float* hidden[PMAXL];                     // [rows][width[l + 1]] or null
  int32_t width[PMAXL + 2];
  int32_t L;
  uint32_t vec;                             // bit l: W[l] is read 16 bytes at a time
  int32_t stride[2];                        // floats per row of the two LDS buffers
  const float *obs, *priv;                  // [rows][obs_cols], [rows][priv_cols] (null: the actor, or priv_cols = 0)
  int32_t obs_cols, priv_cols;
  int64_t rows;
  float* out;                               // [rows][width[L + 1]]: loc or values
  float* actions;                           // [rows][width[L + 1]]   (SAMPLE)
  const float* logstd;                      // [width[L + 1]]         (SAMPLE)
  uint32_t* counts;                         // [rows]                 (SAMPLE)
  uint32_t key0, key1;
};

// the four weights W[j][k .. k + 3] of one lane, zero beyond the row's end
template <bool VEC>
__device__ __forceinline__ void load_w(const float* wrow, int k, int K, float (&w)[4]) {
  if (VEC) {                                                          // (K is a multiple of four: a block lies inside the row or beyond it)
    const float4 q = k < K ? *reinterpret_cast<const float4*>(wrow + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = k + j < K ? wrow[k + j] : 0.0f;
  }
}

// One hidden layer of a tile: dst[row][j] = elu(b[j] + sum_k src[row][k] W[j][k]) for the 32 rows and the N outputs; K the width of W's
// rows, Kp that of the activations in src (K up to a multiple of eight, the rest zeros).
template <bool VEC>
__device__ __forceinline__ void hidden_layer(const float* __restrict__ W, const float* __restrict__ b, const float* src, int ss, float* dst, int ds,
                                             int K, int Kp, int N, float* __restrict__ hid, int64_t row0, int nrow) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const float* arow = src + r * ss + 4 * h;
  for (int c0 = wave * 32; c0 < N; c0 += PWAVES * 32) {               // (uniform over the wavefront)
    const float* wrow = W + (size_t)(c0 + r) * K;
    f32x16 acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float4 a = *reinterpret_cast<const float4*>(arow);
    float w[4];
    load_w<VEC>(wrow, 4 * h, K, w);
    for (int kb = 0; kb < Kp; kb += PKB) {
      float4 an = a;                                                  // the next block's operands are on their way during this block's four steps
      float wn[4] = {w[0], w[1], w[2], w[3]};
      if (kb + PKB < Kp) {
        an = *reinterpret_cast<const float4*>(arow + kb + PKB);
        load_w<VEC>(wrow, kb + PKB + 4 * h, K, wn);
      }
      // A[i = row r][k = h], B[k = h][j = column r]: step j sums k = kb + j, then k = kb + 4 + j
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w[3], acc, 0, 0, 0);
      a = an;
#pragma unroll
      for (int j = 0; j < 4; j++) w[j] = wn[j];
    }
    const float bj = b[c0 + r];
#pragma unroll
    for (int g = 0; g < 16; g++) {                                    // the accumulator: column r, row (g & 3) + 8 (g >> 2) + 4 h
      const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
      const float z = acc[g] + bj;
      const float y = z > 0.0f ? z : expm1f(z);
      dst[row * ds + c0 + r] = y;
      if (hid && row < nrow) hid[(row0 + row) * N + c0 + r] = y;
    }
  }
}

template <bool SAMPLE>
__global__ __launch_bounds__(PTHREADS) void tracker_policy_kernel(const PolicyArgs X) {
  extern __shared__ __align__(16) float s_act[];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * PT;
  const int nrow = (int)(X.rows - row0 < PT ? X.rows - row0 : PT);
  float* buf[2] = {s_act, s_act + PT * X.stride[0]};
  const int in = X.width[0], inp = (in + PKB - 1) & ~(PKB - 1);
  // the input rows side by side, zeros beyond the width and beyond the last row
  for (int i = tid; i < PT * inp; i += PTHREADS) {
    const int r = i / inp, c = i - r * inp;
    float v = 0.0f;
    if (r < nrow) {
      if (c < X.obs_cols) v = X.obs[(row0 + r) * X.obs_cols + c];
      else if (c < in) v = X.priv[(row0 + r) * X.priv_cols + (c - X.obs_cols)];
    }
    buf[0][r * X.stride[0] + c] = v;
  }
  __syncthreads();
  const int L = X.L;
  for (int l = 0; l < L; l++) {
    const int s = l & 1, K = X.width[l], Kp = l == 0 ? inp : K;
    if ((X.vec >> l) & 1u) hidden_layer<true>(X.W[l], X.b[l], buf[s], X.stride[s], buf[s ^ 1], X.stride[s ^ 1], K, Kp, X.width[l + 1], X.hidden[l], row0, nrow);
    else hidden_layer<false>(X.W[l], X.b[l], buf[s], X.stride[s], buf[s ^ 1], X.stride[s ^ 1], K, Kp, X.width[l + 1], X.hidden[l], row0, nrow);
    __syncthreads();
  }
  // the last layer on the vector ALU: an output element per lane, the k in rising order
  const float* src = buf[L & 1];
  const int ss = X.stride[L & 1], K = X.width[L], A = X.width[L + 1];
  const float* __restrict__ W = X.W[L];
  for (int o = tid; o < nrow * A; o += PTHREADS) {
    const int r = o / A, j = o - r * A;
    const float* arow = src + r * ss;
    const float* wrow = W + (size_t)j * K;
    float acc = 0.0f;
    for (int k = 0; k < K; k += 4) {
      const float4 a = *reinterpret_cast<const float4*>(arow + k);
      acc = fmaf(a.x, wrow[k], acc);
      acc = fmaf(a.y, wrow[k + 1], acc);
      acc = fmaf(a.z, wrow[k + 2], acc);
      acc = fmaf(a.w, wrow[k + 3], acc);
    }
    const float z = acc + X.b[L][j];
    const int64_t e = row0 + r;
    X.out[e * A + j] = z;
    if (SAMPLE) {
      // the gaussian branch of the tracker's noise: z + (0 + exp(logstd) * r)
      const ProprioNoise spec = {GMR_NOISE_GAUSSIAN, GMR_NOISE_ADDITIVE, 0.0f, expf(X.logstd[j])};
      X.actions[e * A + j] = tracker_noise(z, spec, (uint32_t)e, X.counts[e], (uint32_t)j, DRAW_ACTION, X.key0, X.key1);
    }
  }
  if (SAMPLE) {
    __syncthreads();                                                  // every lane of the tile has read its count
    if (tid < nrow) X.counts[row0 + tid] = X.counts[row0 + tid] + 1u;
  }
}

// the LDS of the widest network the capacities allow: what both instances are allowed to ask for
constexpr size_t PMAXLDS = (size_t)PT * (GMR_POLICY_MAX_IN + 4 + GMR_POLICY_MAX_WIDTH + 4) * sizeof(float);

// The checks of a call and its launch on the network S of P (critic: P.critic, else P.actor).
static int policy_launch(const gmr_motion_tracker* t, const PolicyTables& P, bool critic, const float* const* params, int64_t rows, const float* obs,
                         const float* priv, float* out, float* actions, float* const* hidden, bool sample, hipStream_t stream) {
  if (!P.on) return gmr_fail(GMR_ERR_ARG, "the policy is not set on this tracker (gmr_motion_tracker_set_policy)");
  const PolicyShape& S = critic ? P.critic : P.actor;
  if (!params || !obs || !out) return gmr_fail(GMR_ERR_ARG, "null params / obs / output");
  if (rows < 1 || rows > (int64_t)1 << 36) return gmr_fail(GMR_ERR_ARG, "rows = %lld, 1 .. 2^36 are taken", (long long)rows);
  if (sample && rows != t->N) return gmr_fail(GMR_ERR_ARG, "sampling needs a row per environment: rows = %lld, N = %d", (long long)rows, t->N);
  if (sample && !actions) return gmr_fail(GMR_ERR_ARG, "sampling needs actions");
  if (critic && P.priv_cols > 0 && !priv) return gmr_fail(GMR_ERR_ARG, "priv is needed: priv_cols = %d", P.priv_cols);
  for (int k = sample ? 0 : S.first; k < S.first + 2 * (S.L + 1); k = k == 0 ? S.first : k + 1) {      // logstd for a sample, the network's pairs
    if (!params[k]) return gmr_fail(GMR_ERR_ARG, "params[%d] is NULL", k);
    if ((uintptr_t)params[k] & 3u) return gmr_fail(GMR_ERR_ARG, "params[%d] is not on 4 bytes", k);
  }
  PolicyArgs X = {};
  X.L = S.L;
  for (int l = 0; l <= S.L + 1; l++) X.width[l] = S.width[l];
  for (int l = 0; l <= S.L; l++) {
    X.W[l] = params[S.first + 2 * l];
    X.b[l] = params[S.first + 2 * l + 1];
    if (l < S.L && aligned16(X.W[l]) && S.width[l] % 4 == 0) X.vec |= 1u << l;
    if (l < S.L) X.hidden[l] = hidden ? hidden[l] : nullptr;
  }
  X.stride[0] = S.stride[0]; X.stride[1] = S.stride[1];
  X.obs = obs; X.priv = critic ? priv : nullptr;
  X.obs_cols = P.obs_cols; X.priv_cols = critic ? P.priv_cols : 0;
  X.rows = rows; X.out = out;
  if (sample) {
    X.actions = actions; X.logstd = params[0]; X.counts = P.counts;
    X.key0 = t->key[0]; X.key1 = t->key[1];
  }
  const unsigned blocks = (unsigned)((rows + PT - 1) / PT);
  if (sample) hipLaunchKernelGGL(tracker_policy_kernel<true>, dim3(blocks), dim3(PTHREADS), S.lds, stream, X);
  else hipLaunchKernelGGL(tracker_policy_kernel<false>, dim3(blocks), dim3(PTHREADS), S.lds, stream, X);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// The synchronous twin of either call: the parameters the network reads, the inputs and the outputs through one staging block.
static int policy_host(gmr_motion_tracker* t, bool critic, const float* const* params, int64_t rows, const float* obs, const float* priv,
                       float* out, float* actions, float* const* hidden, bool sample) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const PolicyTables P = t->policy;
  const PolicyShape& S = critic ? P.critic : P.actor;
  if (!P.on) return gmr_fail(GMR_ERR_ARG, "the policy is not set on this tracker (gmr_motion_tracker_set_policy)");
  if (!params || !obs || !out) return gmr_fail(GMR_ERR_ARG, "null params / obs / output");
  if (rows < 1 || rows > (1 << 26)) return gmr_fail(GMR_ERR_ARG, "rows = %lld, 1 .. 2^26 are taken", (long long)rows);
  const size_t M = (size_t)rows;
  HostStage st;
  const float* dp[GMR_POLICY_MAX_TENSORS] = {};
  float* dh[PMAXL] = {};
  const float *d_obs, *d_priv = nullptr;
  float *d_out, *d_actions = nullptr;
  if (!critic) {
    if (!params[0]) return gmr_fail(GMR_ERR_ARG, "params[0] is NULL");
    st.in(dp[0], params[0], (size_t)P.act_cols * 4);
  }
  for (int l = 0; l <= S.L; l++) {
    const int kw = S.first + 2 * l;
    if (!params[kw] || !params[kw + 1]) return gmr_fail(GMR_ERR_ARG, "params[%d] is NULL", params[kw] ? kw + 1 : kw);
    st.in(dp[kw], params[kw], (size_t)S.width[l] * S.width[l + 1] * 4);
    st.in(dp[kw + 1], params[kw + 1], (size_t)S.width[l + 1] * 4);
    if (l < S.L && hidden) st.out(dh[l], hidden[l], M * S.width[l + 1] * 4);
  }
  st.in(d_obs, obs, M * P.obs_cols * 4);
  if (critic) st.in(d_priv, priv, M * P.priv_cols * 4);
  st.out(d_out, out, M * S.width[S.L + 1] * 4);
  if (sample) st.out(d_actions, actions, M * P.act_cols * 4);
  GMR_STAGE_TRY(st, upload);
  const int rc = policy_launch(t, P, critic, dp, rows, d_obs, d_priv, d_out, d_actions, hidden ? dh : nullptr, sample, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker policy") ---------------------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_policy(gmr_motion_tracker_t* t, int obs_cols, int priv_cols, int act_cols, int n_actor_hidden, const int* actor_hidden,
                                  int n_critic_hidden, const int* critic_hidden) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::PolicyTables P;
  int rc = gmr::policy_plan(obs_cols, priv_cols, act_cols, n_actor_hidden, actor_hidden, n_critic_hidden, critic_hidden, &P.actor, &P.critic);
  if (rc != GMR_OK) return rc;
  P.on = 1; P.obs_cols = obs_cols; P.priv_cols = priv_cols; P.act_cols = act_cols;
  // the widest networks ask for more LDS than a kernel gets unasked
  GMR_HIP_TRY(hipFuncSetAttribute((const void*)gmr::tracker_policy_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gmr::PMAXLDS));
  GMR_HIP_TRY(hipFuncSetAttribute((const void*)gmr::tracker_policy_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gmr::PMAXLDS));
  std::lock_guard<std::mutex> g(t->mu);
  gmr::Carve cv;
  const size_t o_counts = cv.take((size_t)t->N * 4);
  rc = gmr::fresh_block(t->policy_block, cv);
  if (rc != GMR_OK) return rc;
  P.counts = (uint32_t*)(t->policy_block.data() + o_counts);
  t->policy = P;
  return GMR_OK;
}

int gmr_motion_tracker_act_dev(gmr_motion_tracker_t* t, const float* const* d_params, int64_t rows, const float* d_obs, float* d_loc, float* d_actions,
                               float* const* d_hidden, int sample, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::PolicyTables P;
  {
    std::lock_guard<std::mutex> g(t->mu);
    P = t->policy;
  }
  return gmr::policy_launch(t, P, false, d_params, rows, d_obs, nullptr, d_loc, d_actions, d_hidden, sample != 0, (hipStream_t)stream);
}

int gmr_motion_tracker_act(gmr_motion_tracker_t* t, const float* const* params, int64_t rows, const float* obs, float* loc, float* actions,
                           float* const* hidden, int sample) {
  if (sample && !actions) return gmr_fail(GMR_ERR_ARG, "sampling needs actions");
  return gmr::policy_host(t, false, params, rows, obs, nullptr, loc, actions, hidden, sample != 0);
}

int gmr_motion_tracker_values_dev(gmr_motion_tracker_t* t, const float* const* d_params, int64_t rows, const float* d_obs, const float* d_priv,
                                  float* d_values, float* const* d_hidden, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::PolicyTables P;
  {
    std::lock_guard<std::mutex> g(t->mu);
    P = t->policy;
  }
  return gmr::policy_launch(t, P, true, d_params, rows, d_obs, d_priv, d_values, nullptr, d_hidden, false, (hipStream_t)stream);
}

int gmr_motion_tracker_values(gmr_motion_tracker_t* t, const float* const* params, int64_t rows, const float* obs, const float* priv, float* values,
                              float* const* hidden) {
  return gmr::policy_host(t, true, params, rows, obs, priv, values, nullptr, hidden, false);
}

int gmr_motion_tracker_policy_state(gmr_motion_tracker_t* t, int32_t* shape, uint32_t* counts) {
  if (!t || !shape) return gmr_fail(GMR_ERR_ARG, "null motion tracker / shape");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::PolicyTables P = t->policy;
  if (!P.on) return gmr_fail(GMR_ERR_ARG, "the policy is not set on this tracker (gmr_motion_tracker_set_policy)");
  for (int i = 0; i < 16; i++) shape[i] = 0;
  shape[0] = P.obs_cols; shape[1] = P.priv_cols; shape[2] = P.act_cols;
  shape[3] = P.actor.L; shape[8] = P.critic.L;
  for (int l = 0; l < P.actor.L; l++) shape[4 + l] = P.actor.width[l + 1];
  for (int l = 0; l < P.critic.L; l++) shape[9 + l] = P.critic.width[l + 1];
  shape[13] = GMR_POLICY_TILE;
  return gmr::read_back({{counts, P.counts, (size_t)t->N * 4}});
}

}  // extern "C"
