// gmr_tracker_optim.hip -- the optimiser of a training iteration on the motion tracker: what the reference's runner
// does with the gradients of a mini-epoch.  clip_grad_norm_(model.parameters(), 1.0) and optimizer.step() (booster_gym/utils/runner.py:
// 164-165) of the torch.optim.Adam of :33, at the learning rate the rule of :175-180 left behind.  The statement of record is
// tests/optim_mirror.py.
//
//   tracker_optim_norm_kernel    ONE workgroup per chunk of GMR_OPT_CHUNK elements of one tensor (the chunk table is built once, the sizes
//                                are fixed; the addresses come with every call, by value in the kernel arguments).  A lane takes four
//                                consecutive gradients -- 16 bytes where the tensor's addresses are 16-byte aligned, floats else and in the
//                                tail --, squares them in double and the chunk's balanced tree runs through the lane, the wavefront and
//                                the four wavefronts: one double per chunk.
//   tracker_optim_fold_kernel    ONE workgroup: the chunks' partial sums from +0 in rising order; the step count, coef and the Adam scalars
//                                in double; info; then, in follow mode, the loss block's rate becomes the rate of the NEXT step.
//   tracker_optim_update_kernel  ONE workgroup per chunk: p, g, m, v of four consecutive elements per lane and the scalars of the fold;
//                                writes p, m, v.  The gradients are read-only: the clipped gradient lives in a register.
//
// The parameters and gradients are the caller's; exp_avg, exp_avg_sq, the partial sums, the scalars and the rate belong to the tracker; the
// tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/optim_mirror.py states every line in float32 (the sum and the scalars in float64) NumPy
#pragma clang fp contract(off)

namespace gmr {

constexpr int OCHUNK = GMR_OPT_CHUNK;       // elements per chunk: one workgroup
constexpr int OMAXT = GMR_OPT_MAX_TENSORS;
constexpr int OTHREADS = 256;
constexpr int OW = 4;                       // elements per lane: 16 bytes
constexpr int OFOLD = 1024;                 // partial sums the fold stages at a time
static_assert(OCHUNK == OTHREADS * OW, "a lane holds four consecutive elements of the chunk");

struct OptimGrads { const float* g[OMAXT]; };
struct OptimParams { float* p[OMAXT]; };

template <bool VEC>
__device__ __forceinline__ void load4(const float* a, int f0, int cnt, float (&x)[OW]) {
  if (VEC && f0 + OW <= cnt) {
    const float4 q = *reinterpret_cast<const float4*>(a + f0);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < OW; j++) x[j] = f0 + j < cnt ? a[f0 + j] : 0.0f;
  }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* a, int f0, int cnt, const float (&x)[OW]) {
  if (VEC && f0 + OW <= cnt) {
    *reinterpret_cast<float4*>(a + f0) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int j = 0; j < OW; j++)
      if (f0 + j < cnt) a[f0 + j] = x[j];
  }
}

struct NormArgs {
  OptimGrads G;
  const OptimChunk* table;                  // [chunks]
  double* part;                             // [chunks]
  uint32_t vec;                             // bit k: the addresses of tensor k are 16-byte aligned
};

__global__ __launch_bounds__(OTHREADS) void tracker_optim_norm_kernel(const NormArgs X) {
  __shared__ double s_wave[OTHREADS / 64];
  const int tid = threadIdx.x, f0 = tid * OW;
  const OptimChunk row = X.table[blockIdx.x];
  const int k = __builtin_amdgcn_readfirstlane(row.tensor), cnt = __builtin_amdgcn_readfirstlane(row.count);
  const float* g = X.G.g[k];
  if (!g) {                                                           // p.grad is None: +0 (uniform)
    if (tid == 0) X.part[blockIdx.x] = 0.0;
    return;
  }
  g += row.first;
  float x[OW];
  if ((X.vec >> k) & 1u) load4<true>(g, f0, cnt, x);
  else load4<false>(g, f0, cnt, x);
  // the tree x[i] = x[i] + x[i + s]: s = 1, 2 inside the lane, 4 .. 128 across the wavefront, 256, 512 across the wavefronts
  double q[OW];
#pragma unroll
  for (int j = 0; j < OW; j++) q[j] = (double)x[j] * (double)x[j];
  double a = (q[0] + q[1]) + (q[2] + q[3]);
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) a = a + __shfl_down(a, s, 64);
  if ((tid & 63) == 0) s_wave[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) X.part[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

struct OptimFoldArgs {
  const double* part;                       // [chunks]
  int64_t chunks;
  double* state;                            // [4] the rate, the step count, beta1^t, beta2^t
  float* scal;                              // [4] coef, bc2s, ns
  double* info;                             // [4] or null
  const double* follow;                     // the loss block's rate, or null: the rate is fixed
  double beta1, beta2, max_norm;
};

__global__ __launch_bounds__(OTHREADS) void tracker_optim_fold_kernel(const OptimFoldArgs X) {
  __shared__ double s_part[OFOLD];
  const int tid = threadIdx.x;
  double total = 0.0;
  for (int64_t c0 = 0; c0 < X.chunks; c0 += OFOLD) {
    const int n = (int)(X.chunks - c0 < OFOLD ? X.chunks - c0 : OFOLD);
    for (int i = tid; i < n; i += OTHREADS) s_part[i] = X.part[c0 + i];
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < n; i++) total = total + s_part[i];          // from +0, in rising order
    __syncthreads();
  }
  if (tid != 0) return;
  const double norm = __dsqrt_rn(total);
  const double coef = fmin(1.0, __ddiv_rn(X.max_norm, norm + 1e-6));
  const double lr = X.state[0], t = X.state[1] + 1.0;
  const double b1t = X.state[2] * X.beta1, b2t = X.state[3] * X.beta2;
  X.state[1] = t; X.state[2] = b1t; X.state[3] = b2t;
  X.scal[0] = (float)coef;
  X.scal[1] = (float)__dsqrt_rn(1.0 - b2t);
  X.scal[2] = (float)(-__ddiv_rn(lr, 1.0 - b1t));
  if (X.info) {
    X.info[0] = norm; X.info[1] = (double)(float)coef; X.info[2] = lr; X.info[3] = t;
  }
  if (X.follow) X.state[0] = *X.follow;                               // the rate of the NEXT step: what the rule has left by now
}

struct UpdateArgs {
  OptimParams P;
  OptimGrads G;
  const OptimChunk* table;                  // [chunks]
  float *exp_avg, *exp_avg_sq;
  const float* scal;                        // [4] coef, bc2s, ns: the fold's
  uint32_t vec;
  float w1, b2, c2, e;
};

template <bool VEC>
__device__ __forceinline__ void update_chunk(float* p, const float* g, float* m, float* v, int f0, int cnt, const UpdateArgs& X) {
  float xp[OW], xg[OW], xm[OW], xv[OW];
  load4<VEC>(p, f0, cnt, xp);
  load4<VEC>(g, f0, cnt, xg);
  load4<true>(m, f0, cnt, xm);                                        // (the state starts on 256 bytes whatever the caller's addresses)
  load4<true>(v, f0, cnt, xv);
  const float coef = X.scal[0], bc2s = X.scal[1], ns = X.scal[2];
#pragma unroll
  for (int j = 0; j < OW; j++) {
    const float gc = xg[j] * coef;
    xm[j] = xm[j] + X.w1 * (gc - xm[j]);                              // lerp_
    xv[j] = xv[j] * X.b2;                                             // mul_
    xv[j] = xv[j] + (X.c2 * gc) * gc;                                 // addcmul_
    const float den = __fdiv_rn(sqrtf(xv[j]), bc2s) + X.e;            // (sqrtf is the correctly rounded one: __fsqrt_rn is the native one here)
    xp[j] = xp[j] + __fdiv_rn(ns * xm[j], den);                       // addcdiv_
  }
  store4<VEC>(p, f0, cnt, xp);
  store4<true>(m, f0, cnt, xm);
  store4<true>(v, f0, cnt, xv);
}

__global__ __launch_bounds__(OTHREADS) void tracker_optim_update_kernel(const UpdateArgs X) {
  const int f0 = threadIdx.x * OW;
  const OptimChunk row = X.table[blockIdx.x];
  const int k = __builtin_amdgcn_readfirstlane(row.tensor), cnt = __builtin_amdgcn_readfirstlane(row.count);
  const float* g = X.G.g[k];
  if (!g) return;                                                     // p.grad is None (uniform)
  float* p = X.P.p[k] + row.first;
  g += row.first;
  float *m = X.exp_avg + row.state, *v = X.exp_avg_sq + row.state;
  if ((X.vec >> k) & 1u) update_chunk<true>(p, g, m, v, f0, cnt, X);
  else update_chunk<false>(p, g, m, v, f0, cnt, X);
}

static int optim_check(const OptimTables& T, const LossTables& L, float* const* params, const float* const* grads) {
  if (T.K == 0) return gmr_fail(GMR_ERR_ARG, "the optimiser is not set on this tracker (gmr_motion_tracker_set_optimizer)");
  if (T.follow && !L.on) return gmr_fail(GMR_ERR_ARG, "the optimiser follows the loss block's learning rate and the loss is not set (gmr_motion_tracker_set_loss)");
  if (!params || !grads) return gmr_fail(GMR_ERR_ARG, "null params / grads table");
  for (int k = 0; k < T.K; k++)
    if (!params[k]) return gmr_fail(GMR_ERR_ARG, "params[%d] is NULL (a tensor is skipped through a NULL gradient)", k);
  return GMR_OK;
}

static int optim_launch(const OptimTables& T, const LossTables& L, float* const* params, const float* const* grads, double* info, hipStream_t stream) {
  const int rc = optim_check(T, L, params, grads);
  if (rc != GMR_OK) return rc;
  NormArgs N = {};
  UpdateArgs U = {};
  uint32_t vec = 0;
  for (int k = 0; k < T.K; k++) {
    N.G.g[k] = U.G.g[k] = grads[k];
    U.P.p[k] = params[k];
    if (aligned16(params[k]) && aligned16(grads[k])) vec |= 1u << k;
  }
  N.table = U.table = T.table; N.part = T.part; N.vec = U.vec = vec;
  hipLaunchKernelGGL(tracker_optim_norm_kernel, dim3((unsigned)T.chunks), dim3(OTHREADS), 0, stream, N);
  OptimFoldArgs F = {};
  F.part = T.part; F.chunks = T.chunks; F.state = T.state; F.scal = T.scal; F.info = info; F.follow = T.follow ? L.lr : nullptr;
  F.beta1 = T.beta1; F.beta2 = T.beta2; F.max_norm = T.max_norm;
  hipLaunchKernelGGL(tracker_optim_fold_kernel, dim3(1), dim3(OTHREADS), 0, stream, F);
  U.exp_avg = T.exp_avg; U.exp_avg_sq = T.exp_avg_sq; U.scal = T.scal;
  U.w1 = (float)(1.0 - T.beta1); U.b2 = (float)T.beta2; U.c2 = (float)(1.0 - T.beta2); U.e = (float)T.eps;
  hipLaunchKernelGGL(tracker_optim_update_kernel, dim3((unsigned)T.chunks), dim3(OTHREADS), 0, stream, U);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// beta^t as the fold forms it: the product of t factors from 1
static double optim_power(double beta, int64_t t) {
  double x = 1.0;
  for (int64_t i = 0; i < t && x != 0.0; i++) x = x * beta;
  return x;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker optimiser") ------------------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_optimizer(gmr_motion_tracker_t* t, int K, const int64_t* sizes, double learning_rate, double beta1, double beta2,
                                     double eps, double max_norm) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (K < 1 || K > GMR_OPT_MAX_TENSORS) return gmr_fail(GMR_ERR_ARG, "K = %d tensors, 1 .. GMR_OPT_MAX_TENSORS = %d are taken", K, GMR_OPT_MAX_TENSORS);
  if (!sizes) return gmr_fail(GMR_ERR_ARG, "null sizes");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return gmr_fail(GMR_ERR_ARG, "beta1 = %g and beta2 = %g must lie in [0, 1)", beta1, beta2);
  if (!std::isfinite(eps) || eps <= 0.0) return gmr_fail(GMR_ERR_ARG, "eps = %g must be finite and above 0", eps);
  if (!std::isfinite(max_norm) || max_norm <= 0.0) return gmr_fail(GMR_ERR_ARG, "max_norm = %g must be finite and above 0", max_norm);
  const bool follow = std::isnan(learning_rate);
  if (!follow && (!std::isfinite(learning_rate) || learning_rate <= 0.0))
    return gmr_fail(GMR_ERR_ARG, "learning_rate = %g must be finite and above 0, or NaN: follow the loss block", learning_rate);
  gmr::OptimTables T;
  T.K = K; T.follow = follow ? 1 : 0;
  T.beta1 = beta1; T.beta2 = beta2; T.eps = eps; T.max_norm = max_norm;
  for (int k = 0; k < K; k++) {
    if (sizes[k] < 1 || sizes[k] > (int64_t)1 << 40) return gmr_fail(GMR_ERR_ARG, "sizes[%d] = %lld, 1 .. 2^40 elements are taken", k, (long long)sizes[k]);
    T.size[k] = sizes[k];
    T.off[k] = T.state_floats;
    T.state_floats += (sizes[k] + 63) / 64 * 64;                     // every tensor's state on 256 bytes
    T.chunks += (sizes[k] + gmr::OCHUNK - 1) / gmr::OCHUNK;
    T.total += sizes[k];
  }
  if (T.chunks > 0x7fffffffLL) return gmr_fail(GMR_ERR_ARG, "%lld elements are more chunks than a launch takes", (long long)T.total);
  std::vector<gmr::OptimChunk> table((size_t)T.chunks);
  size_t c = 0;
  for (int k = 0; k < K; k++)
    for (int64_t first = 0; first < T.size[k]; first += gmr::OCHUNK) {
      const int64_t left = T.size[k] - first;
      table[c++] = gmr::OptimChunk{first, T.off[k] + first, k, (int32_t)(left < gmr::OCHUNK ? left : gmr::OCHUNK)};
    }
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::LossTables L = t->loss;
  if (follow && !L.on)
    return gmr_fail(GMR_ERR_ARG, "learning_rate NaN follows the loss block's rate and the loss is not set on this tracker (gmr_motion_tracker_set_loss)");
  gmr::Carve cv;
  const size_t o_table = cv.take(table.size() * sizeof(gmr::OptimChunk)), o_m = cv.take((size_t)T.state_floats * 4), o_v = cv.take((size_t)T.state_floats * 4);
  const size_t o_part = cv.take((size_t)T.chunks * 8), o_state = cv.take(32), o_scal = cv.take(16);
  const int rc = gmr::fresh_block(t->optim_block, cv);
  if (rc != GMR_OK) return rc;
  char* d = t->optim_block.data();
  GMR_HIP_TRY(hipMemcpy(d + o_table, table.data(), table.size() * sizeof(gmr::OptimChunk), hipMemcpyHostToDevice));
  const double state[4] = {follow ? 0.0 : learning_rate, 0.0, 1.0, 1.0};
  GMR_HIP_TRY(hipMemcpy(d + o_state, state, 32, hipMemcpyHostToDevice));
  if (follow) GMR_HIP_TRY(hipMemcpy(d + o_state, L.lr, 8, hipMemcpyDeviceToDevice));
  GMR_HIP_TRY(hipDeviceSynchronize());
  T.table = (const gmr::OptimChunk*)(d + o_table);
  T.exp_avg = (float*)(d + o_m); T.exp_avg_sq = (float*)(d + o_v);
  T.part = (double*)(d + o_part); T.state = (double*)(d + o_state); T.scal = (float*)(d + o_scal);
  t->optim = T;
  return GMR_OK;
}

int gmr_motion_tracker_optimizer_step_dev(gmr_motion_tracker_t* t, float* const* d_params, const float* const* d_grads, double* d_info, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::OptimTables T;
  gmr::LossTables L;
  {
    std::lock_guard<std::mutex> g(t->mu);
    T = t->optim; L = t->loss;
  }
  return gmr::optim_launch(T, L, d_params, d_grads, d_info, (hipStream_t)stream);
}

int gmr_motion_tracker_optimizer_step(gmr_motion_tracker_t* t, float* const* params, const float* const* grads, double* info) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::OptimTables T = t->optim;
  const gmr::LossTables L = t->loss;
  int rc = gmr::optim_check(T, L, params, grads);
  if (rc != GMR_OK) return rc;
  // the K tensors as two flat host arrays, every tensor on 256 bytes like the state: two copies in, one launch, the parameters back
  std::vector<float> hp((size_t)T.state_floats), hg((size_t)T.state_floats);
  for (int k = 0; k < T.K; k++) {
    memcpy(hp.data() + T.off[k], params[k], (size_t)T.size[k] * 4);
    if (grads[k]) memcpy(hg.data() + T.off[k], grads[k], (size_t)T.size[k] * 4);
  }
  gmr::HostStage st;
  float* d_p;
  const float* d_g;
  double* d_info;
  st.in(d_p, hp.data(), hp.size() * 4); st.in(d_g, hg.data(), hg.size() * 4);
  st.out(d_info, info, 32);
  GMR_STAGE_TRY(st, upload);
  float* dp[GMR_OPT_MAX_TENSORS];
  const float* dg[GMR_OPT_MAX_TENSORS];
  for (int k = 0; k < T.K; k++) {
    dp[k] = d_p + T.off[k];
    dg[k] = grads[k] ? d_g + T.off[k] : nullptr;
  }
  rc = gmr::optim_launch(T, L, dp, dg, d_info, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  GMR_HIP_TRY(hipMemcpy(hp.data(), d_p, hp.size() * 4, hipMemcpyDeviceToHost));      // (the parameters are read and written in place)
  for (int k = 0; k < T.K; k++) memcpy(params[k], hp.data() + T.off[k], (size_t)T.size[k] * 4);
  return GMR_OK;
}

int gmr_motion_tracker_optimizer_state(gmr_motion_tracker_t* t, int64_t* step, float* exp_avg, float* exp_avg_sq) {
  if (!t || !step || !exp_avg || !exp_avg_sq) return gmr_fail(GMR_ERR_ARG, "null motion tracker / step / exp_avg / exp_avg_sq");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::OptimTables T = t->optim;
  if (T.K == 0) return gmr_fail(GMR_ERR_ARG, "the optimiser is not set on this tracker (gmr_motion_tracker_set_optimizer)");
  GMR_HIP_TRY(hipDeviceSynchronize());
  double state[4];
  GMR_HIP_TRY(hipMemcpy(state, T.state, 32, hipMemcpyDeviceToHost));
  *step = (int64_t)state[1];
  int64_t at = 0;
  for (int k = 0; k < T.K; k++) {
    GMR_HIP_TRY(hipMemcpy(exp_avg + at, T.exp_avg + T.off[k], (size_t)T.size[k] * 4, hipMemcpyDeviceToHost));
    GMR_HIP_TRY(hipMemcpy(exp_avg_sq + at, T.exp_avg_sq + T.off[k], (size_t)T.size[k] * 4, hipMemcpyDeviceToHost));
    at += T.size[k];
  }
  return GMR_OK;
}

int gmr_motion_tracker_optimizer_load_state(gmr_motion_tracker_t* t, int64_t step, const float* exp_avg, const float* exp_avg_sq) {
  if (!t || !exp_avg || !exp_avg_sq) return gmr_fail(GMR_ERR_ARG, "null motion tracker / exp_avg / exp_avg_sq");
  if (step < 0 || step > (int64_t)1 << 40) return gmr_fail(GMR_ERR_ARG, "step = %lld, 0 .. 2^40 are taken", (long long)step);
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::OptimTables T = t->optim;
  const gmr::LossTables L = t->loss;
  if (T.K == 0) return gmr_fail(GMR_ERR_ARG, "the optimiser is not set on this tracker (gmr_motion_tracker_set_optimizer)");
  if (T.follow && !L.on) return gmr_fail(GMR_ERR_ARG, "the optimiser follows the loss block's learning rate and the loss is not set (gmr_motion_tracker_set_loss)");
  GMR_HIP_TRY(hipDeviceSynchronize());
  int64_t at = 0;
  for (int k = 0; k < T.K; k++) {
    GMR_HIP_TRY(hipMemcpy(T.exp_avg + T.off[k], exp_avg + at, (size_t)T.size[k] * 4, hipMemcpyHostToDevice));
    GMR_HIP_TRY(hipMemcpy(T.exp_avg_sq + T.off[k], exp_avg_sq + at, (size_t)T.size[k] * 4, hipMemcpyHostToDevice));
    at += T.size[k];
  }
  const double state[3] = {(double)step, gmr::optim_power(T.beta1, step), gmr::optim_power(T.beta2, step)};
  GMR_HIP_TRY(hipMemcpy(T.state + 1, state, 24, hipMemcpyHostToDevice));
  if (T.follow) GMR_HIP_TRY(hipMemcpy(T.state, L.lr, 8, hipMemcpyDeviceToDevice));
  GMR_HIP_TRY(hipDeviceSynchronize());
  return GMR_OK;
}

}  // extern "C"
