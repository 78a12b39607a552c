// gmr_tracker_adaptive.hip -- adaptive start sampling and masked resets of the motion tracker: every clip is
// cut into time bins, the device keeps a failure count and a discounted failure history per bin, and a reset takes its done / failed
// flags as masks on the device.
//
//   tracker_reset_done_kernel    ONE launch per reset, one lane per environment (or per list entry): a lane that is not done leaves
//                                after its flag; a failed one adds 1 to the bin of its clock (adaptive tracker); then the draw -- the
//                                plain tracker's (tracker_reset_kernel's lines), or the one from the bins (tracker_draw_bin)
//   tracker_adapt_ema_kernel     step 1 of an Adapt: ema and the reset of the counters, one lane per bin
//   tracker_adapt_score_kernel   step 2: the look-ahead sum s, parked in prob, and one partial sum of s per 4096 bins
//   tracker_adapt_cdf_kernel     steps 3 and 4 in ONE workgroup: S, prob, and a cdf summed in one fixed order
//
// The kernels write the tracker's own state and nothing else of either handle; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_motion_sample.h"
#include "gmr_philox.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/adaptive_mirror.py states every line of an Adapt in float64 NumPy
#pragma clang fp contract(off)

// 1: the lanes of a wavefront that hit one bin fold into one atomic; 0: one atomic per lane (an A/B build through build_variant).
// DESIGN.md 6n has the numbers: folding costs an eighth where the failures are spread and wins 55 x where they meet in one bin.
#ifndef GMR_ADAPTIVE_AGGREGATE
#define GMR_ADAPTIVE_AGGREGATE 1
#endif

namespace gmr {

// the bin of environment e's clock, or -1 for a bad assignment: integer arithmetic on the lower frame of the sampler's query
__device__ __forceinline__ int tracker_bin(const MotionArrays& A, const TrackerState& S, int e, int loop) {
  const int c = S.clip[e];
  const MotionQuery Q = motion_query(A, c, (double)S.time[e], loop);
  if (!Q.ok) return -1;
  const int lo = (int)(Q.rl - (size_t)A.seg_start[c]);
  const AdaptiveBins Bn = *S.bins;
  const int b0 = Bn.start[c], nb = Bn.start[c + 1] - b0;
  const int k = lo / Bn.frames[c];
  return b0 + (k < nb - 1 ? k : nb - 1);
}

// Lane i serves entry i of the list, or environment i without one; done / failed are indexed the same way.  An entry that is not
// done is not looked at any further (its id is not read).
__global__ __launch_bounds__(256) void tracker_reset_done_kernel(const MotionArrays A, const TrackerState S, uint32_t* __restrict__ fail_now, int N,
                                                                 int n, const int32_t* __restrict__ ids, const int32_t* __restrict__ done,
                                                                 const int32_t* __restrict__ failed, int loop, int resample, float lo, float hi,
                                                                 uint32_t key0, uint32_t key1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (done && done[i] == 0) return;
  const int e = tracker_env(S, ids, i, N);
  const bool adaptive = S.bins != nullptr;
  int b = -1;
  if (e >= 0 && adaptive && failed && failed[i] != 0) b = tracker_bin(A, S, e, loop);
#if GMR_ADAPTIVE_AGGREGATE
  // the lanes still here take turns: the lowest pending lane names its bin, every lane on that bin is counted, the leader adds
  unsigned long long pending = __ballot(b >= 0);
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const int lb = __shfl(b, leader);
    const unsigned long long same = __ballot(b == lb);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&fail_now[lb], (uint32_t)__popcll(same));
    pending &= ~same;
  }
#else
  if (b >= 0) atomicAdd(&fail_now[b], 1u);
#endif
  if (e < 0) return;
  if (adaptive) {
    int c = 0;
    S.time[e] = tracker_draw_bin(A, S, key0, key1, e, &c);
    S.clip[e] = c;
    S.length[e] = clip_length(A, c);
    return;
  }
  int c = 0;                                 // (the lines of tracker_reset_kernel)
  const float u = tracker_draw(A, S, key0, key1, e, resample != 0, &c);
  if (resample) {
    S.clip[e] = c;
    S.length[e] = clip_length(A, c);
  }
  S.time[e] = lo + (hi - lo) * u;
}

// v of lane i (the same i in every lane) in every lane
__device__ __forceinline__ double lane_value(double v, int i) {
  const long long x = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)x, i), hi = __builtin_amdgcn_readlane((int)(x >> 32), i);
  return __longlong_as_double(((long long)hi << 32) | (long long)(uint32_t)lo);
}

// step 1: ema = (1 - alpha) ema + alpha (double)fail_now, fail_now = 0
__global__ __launch_bounds__(256) void tracker_adapt_ema_kernel(const AdaptivePlan P, const AdaptiveArrays R) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= P.Bt) return;
  R.ema[b] = (1.0 - P.alpha) * R.ema[b] + P.alpha * (double)R.fail_now[b];
  R.fail_now[b] = 0u;
}

// step 2: s[b] = sum over u < K of g[u] ema[min(b + u, last bin of b's clip)] in ascending u, 0 for a clip of weight zero; s is
// parked in prob.  The partial sum of a workgroup's 4096 bins: lane t adds its 16 bins (t, t + 256, ..) in ascending order, then the
// 256 lane sums meet pairwise (t with t + 128, then + 64, .. + 1).
__global__ __launch_bounds__(256) void tracker_adapt_score_kernel(const AdaptivePlan P, const AdaptiveArrays R, const AdaptiveBins Bn) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double mine = 0.0;
  for (int i = 0; i < ADAPT_TILE / 256; i++) {
    const int b = blockIdx.x * ADAPT_TILE + i * 256 + t;
    if (b >= P.Bt) break;
    double s = 0.0;
    if (R.base[b] != 0.0) {
      const int last = Bn.start[Bn.clip[b] + 1] - 1;
      for (int u = 0; u < P.K; u++) s = s + P.g[u] * R.ema[b + u < last ? b + u : last];
    }
    R.prob[b] = s;
    mine = mine + s;
  }
  red[t] = mine;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) red[t] = red[t] + red[t + h];
    __syncthreads();
  }
  if (t == 0) R.part[blockIdx.x] = red[0];
}

// steps 3 and 4 in one workgroup of 1024 lanes.
//   S     lane t takes part[t] (at most 1024 of them), the lanes meet pairwise as above
//   prob  p = base, or ((1 - uniform) s) / S + uniform base
//   cdf   in ONE order, so that it cannot decrease and a bin of p = 0 gets an empty interval: a lane owns chunks of 64 consecutive
//         bins and adds their p in ascending order (run); wavefront 0 then adds the chunk totals in ascending order, one after the
//         other (off); cdf[b] = off[chunk of b] + run before b.  x -> fl(off + x) does not decrease, run does not decrease inside a
//         chunk, and off of the next chunk is fl(off + total) with total >= every run of this one.
__global__ __launch_bounds__(1024) void tracker_adapt_cdf_kernel(const AdaptivePlan P, const AdaptiveArrays R) {
  __shared__ double red[1024];
  const int t = threadIdx.x, Bt = P.Bt;
  const int nparts = (Bt + ADAPT_TILE - 1) / ADAPT_TILE, nchunks = (Bt + ADAPT_CHUNK - 1) / ADAPT_CHUNK;
  red[t] = t < nparts ? R.part[t] : 0.0;
  __syncthreads();
  for (int h = 512; h >= 1; h >>= 1) {
    if (t < h) red[t] = red[t] + red[t + h];
    __syncthreads();
  }
  const double total = red[0];
  for (int j = t; j < nchunks; j += 1024) {
    const int b1 = (j + 1) * ADAPT_CHUNK < Bt ? (j + 1) * ADAPT_CHUNK : Bt;
    double run = 0.0;
    for (int b = j * ADAPT_CHUNK; b < b1; b++) {
      const double base = R.base[b];
      const double p = total == 0.0 ? base : (1.0 - P.uniform) * R.prob[b] / total + P.uniform * base;
      R.prob[b] = p;
      run = run + p;
    }
    R.tot[j] = run;
  }
  __syncthreads();
  if (t < 64) {      // wavefront 0: every lane adds the same 64 totals in order, lane i keeps the sum in front of total i
    double off = 0.0;
    for (int j0 = 0; j0 < nchunks; j0 += 64) {
      const double v = j0 + t < nchunks ? R.tot[j0 + t] : 0.0;
      double at = 0.0;
      for (int i = 0; i < 64; i++) {
        if (i == t) at = off;
        off = off + lane_value(v, i);
      }
      if (j0 + t < nchunks) R.tot[j0 + t] = at;
    }
  }
  __syncthreads();
  for (int j = t; j < nchunks; j += 1024) {
    const int b1 = (j + 1) * ADAPT_CHUNK < Bt ? (j + 1) * ADAPT_CHUNK : Bt;
    const double off = R.tot[j];
    double run = 0.0;
    for (int b = j * ADAPT_CHUNK; b < b1; b++) {
      R.cdf[b] = off + run;
      run = run + R.prob[b];
    }
  }
}

static int adapt_launch(const AdaptivePlan& P, const AdaptiveArrays& R, const AdaptiveBins& Bn, hipStream_t stream) {
  hipLaunchKernelGGL(tracker_adapt_ema_kernel, dim3(lane_blocks(P.Bt)), dim3(256), 0, stream, P, R);
  hipLaunchKernelGGL(tracker_adapt_score_kernel, dim3((unsigned)((P.Bt + ADAPT_TILE - 1) / ADAPT_TILE)), dim3(256), 0, stream, P, R, Bn);
  hipLaunchKernelGGL(tracker_adapt_cdf_kernel, dim3(1), dim3(1024), 0, stream, P, R);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// every check of a masked reset, and its launch
static int reset_done_launch(gmr_motion_tracker* t, const TrackerState& S, uint32_t* fail_now, int n, const int32_t* d_env_ids, const int32_t* d_done,
                             const int32_t* d_failed, int resample, float lo, float hi, hipStream_t stream) {
  const int rc = subset_check(t->N, n, d_env_ids, "the masks cover every environment");
  if (rc != GMR_OK) return rc;
  if (!std::isfinite(lo) || !std::isfinite(hi)) return gmr_fail(GMR_ERR_ARG, "time_offset_range (%g, %g) is not finite", (double)lo, (double)hi);
  if (S.bins && (!resample || lo != 0.0f || hi != 0.0f))
    return gmr_fail(GMR_ERR_ARG, "an adaptive tracker draws clip and start from its bins: resample = 1 and time_offset_range (0, 0) "
                                 "(got %d, (%g, %g)); gmr_motion_tracker_reset_dev serves a range", resample, (double)lo, (double)hi);
  if (n == 0) return GMR_OK;
  hipLaunchKernelGGL(tracker_reset_done_kernel, dim3(lane_blocks(n)), dim3(256), 0, stream, t->lib->A, S, fail_now, t->N, n, d_env_ids,
                     d_done, d_failed, t->loop, resample ? 1 : 0, lo, hi, t->key[0], t->key[1]);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// alpha, uniform, K and gamma into a plan (Bt is left as it is)
static int adaptive_params(double alpha, double uniform, int K, double gamma, AdaptivePlan* P) {
  if (!(alpha >= 0.0 && alpha <= 1.0)) return gmr_fail(GMR_ERR_ARG, "alpha = %g outside [0, 1]", alpha);
  if (!(uniform >= 0.0 && uniform <= 1.0)) return gmr_fail(GMR_ERR_ARG, "uniform = %g outside [0, 1]", uniform);
  if (K < 1 || K > ADAPT_MAX_K) return gmr_fail(GMR_ERR_ARG, "K = %d outside [1, %d]", K, ADAPT_MAX_K);
  if (!(gamma > 0.0 && gamma <= 1.0)) return gmr_fail(GMR_ERR_ARG, "gamma = %g outside (0, 1]", gamma);
  P->alpha = alpha; P->uniform = uniform; P->K = K;
  double g = 1.0;
  for (int u = 0; u < ADAPT_MAX_K; u++) {
    P->g[u] = u < K ? g : 0.0;
    g = g * gamma;
  }
  return GMR_OK;
}

// adaptive sampling off: the draws of a plain tracker again (the caller holds the mutex and has synchronised the device)
static void adaptive_off(gmr_motion_tracker* t) {
  t->S.bins = nullptr;
  t->bin_tab = AdaptiveBins{};
  t->adaptive = AdaptivePlan{};
  t->bins = AdaptiveArrays{};
  t->bin_seconds = 0.0;
  (void)t->bin_block.release();
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker adaptive sampling") -----------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_adaptive(gmr_motion_tracker_t* t, double bin_seconds, double alpha, double uniform, int K, double gamma) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (std::isnan(bin_seconds) || std::isinf(bin_seconds)) return gmr_fail(GMR_ERR_ARG, "bin_seconds = %g is not finite", bin_seconds);
  std::lock_guard<std::mutex> g(t->mu);
  if (bin_seconds <= 0.0) {
    GMR_HIP_TRY(hipDeviceSynchronize());
    gmr::adaptive_off(t);
    return GMR_OK;
  }
  gmr::AdaptivePlan P = t->adaptive;
  const int rc = gmr::adaptive_params(alpha, uniform, K, gamma, &P);
  if (rc != GMR_OK) return rc;
  if (t->adaptive.Bt > 0 && bin_seconds == t->bin_seconds) {      // the same bins: new parameters for the Adapts to come, ema stays
    t->adaptive = P;
    return GMR_OK;
  }
  // the bin tables, from the library's own seg_start and fps
  const int C = t->lib->A.C;
  std::vector<int32_t> seg((size_t)C + 1), bin_start((size_t)C + 1), frames((size_t)C);
  std::vector<double> fps((size_t)C);
  GMR_HIP_TRY(hipDeviceSynchronize());
  GMR_HIP_TRY(hipMemcpy(seg.data(), t->lib->A.seg_start, ((size_t)C + 1) * 4, hipMemcpyDeviceToHost));
  GMR_HIP_TRY(hipMemcpy(fps.data(), t->lib->A.fps, (size_t)C * 8, hipMemcpyDeviceToHost));
  long long Bt = 0;
  double wsum = 0.0;      // over the clips that have bins, in clip order
  for (int c = 0; c < C; c++) {
    const long long T = seg[c + 1] - seg[c];
    const double f = bin_seconds * fps[c];
    long long F = f >= 2147483647.0 ? 2147483647LL : std::llround(f);
    if (F < 1) F = 1;
    if (F > T) F = T > 1 ? T : 1;      // (one bin either way; keeps k F inside 32 bits)
    frames[c] = (int32_t)F;
    bin_start[c] = (int32_t)Bt;
    Bt += (T + F - 1) / F;
    if (Bt > gmr::ADAPT_MAX_BINS) break;
    if (T > 0) wsum += t->clip_w.empty() ? 1.0 : t->clip_w[c];
  }
  if (Bt < 1 || Bt > gmr::ADAPT_MAX_BINS)
    return gmr_fail(GMR_ERR_ARG, "bin_seconds = %g gives %s bins: 1 to %d are served", bin_seconds, Bt < 1 ? "no" : "too many", gmr::ADAPT_MAX_BINS);
  if (!(wsum > 0.0)) return gmr_fail(GMR_ERR_ARG, "every clip that has frames has weight zero");
  bin_start[C] = (int32_t)Bt;
  std::vector<int32_t> bin_clip((size_t)Bt);
  std::vector<double> base((size_t)Bt);
  for (int c = 0; c < C; c++) {
    const long long T = seg[c + 1] - seg[c], F = frames[c];
    const double wn = (t->clip_w.empty() ? 1.0 : t->clip_w[c]) / wsum;
    for (int b = bin_start[c]; b < bin_start[c + 1]; b++) {
      const long long f0 = (long long)(b - bin_start[c]) * F, f1 = f0 + F < T ? f0 + F : T;
      bin_clip[b] = c;
      base[b] = wn * (double)(f1 - f0) / (double)T;
    }
  }
  gmr::adaptive_off(t);
  const size_t nb = (size_t)Bt;
  gmr::Carve cv;
  const size_t o_tab = cv.take(sizeof(gmr::AdaptiveBins)), o_start = cv.take(((size_t)C + 1) * 4), o_frames = cv.take((size_t)C * 4), o_clip = cv.take(nb * 4), o_base = cv.take(nb * 8),
               o_fail = cv.take(nb * 4), o_ema = cv.take(nb * 8), o_prob = cv.take(nb * 8), o_cdf = cv.take(nb * 8),
               o_part = cv.take((nb + gmr::ADAPT_TILE - 1) / gmr::ADAPT_TILE * 8), o_tot = cv.take((nb + gmr::ADAPT_CHUNK - 1) / gmr::ADAPT_CHUNK * 8);
  GMR_HIP_TRY(t->bin_block.reserve(cv.total() + 256));
  char* d = t->bin_block.data();
  hipError_t e = hipMemset(d, 0, cv.total());
  if (e == hipSuccess) e = hipMemcpy(d + o_start, bin_start.data(), ((size_t)C + 1) * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_frames, frames.data(), (size_t)C * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_clip, bin_clip.data(), nb * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_base, base.data(), nb * 8, hipMemcpyHostToDevice);
  const gmr::AdaptiveBins Bn{(int32_t)Bt, (const double*)(d + o_cdf), (const int32_t*)(d + o_start), (const int32_t*)(d + o_clip),
                             (const int32_t*)(d + o_frames)};
  if (e == hipSuccess) e = hipMemcpy(d + o_tab, &Bn, sizeof(Bn), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    gmr::adaptive_off(t);
    return gmr_fail(GMR_ERR_HIP, "gmr_motion_tracker_set_adaptive: %s", hipGetErrorString(e));
  }
  P.Bt = (int32_t)Bt;
  const gmr::AdaptiveArrays R{(const double*)(d + o_base), (uint32_t*)(d + o_fail), (double*)(d + o_ema), (double*)(d + o_prob), (double*)(d + o_cdf),
                              (double*)(d + o_part), (double*)(d + o_tot)};
  int rc2 = gmr::adapt_launch(P, R, Bn, nullptr);      // ema = 0: the cdf of base
  if (rc2 == GMR_OK && (e = hipDeviceSynchronize()) != hipSuccess) rc2 = gmr_fail(GMR_ERR_HIP, "gmr_motion_tracker_set_adaptive: %s", hipGetErrorString(e));
  if (rc2 != GMR_OK) {
    gmr::adaptive_off(t);
    return rc2;
  }
  t->S.bins = (const gmr::AdaptiveBins*)(d + o_tab);
  t->bin_tab = Bn; t->bins = R; t->adaptive = P; t->bin_seconds = bin_seconds;
  return GMR_OK;
}

int gmr_motion_tracker_adapt_dev(gmr_motion_tracker_t* t, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::AdaptivePlan P;
  gmr::AdaptiveArrays R;
  gmr::AdaptiveBins Bn;
  {
    std::lock_guard<std::mutex> g(t->mu);
    P = t->adaptive; R = t->bins; Bn = t->bin_tab;
  }
  if (P.Bt == 0) return gmr_fail(GMR_ERR_ARG, "adaptive sampling is not configured (gmr_motion_tracker_set_adaptive)");
  return gmr::adapt_launch(P, R, Bn, (hipStream_t)stream);
}

int gmr_motion_tracker_adapt(gmr_motion_tracker_t* t) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  if (t->adaptive.Bt == 0) return gmr_fail(GMR_ERR_ARG, "adaptive sampling is not configured (gmr_motion_tracker_set_adaptive)");
  const int rc = gmr::adapt_launch(t->adaptive, t->bins, t->bin_tab, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_HIP_TRY(hipDeviceSynchronize());
  return GMR_OK;
}

int gmr_motion_tracker_reset_done_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_done, const int32_t* d_failed,
                                      int resample, float lo, float hi, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::TrackerState S;
  uint32_t* fail_now;
  {
    std::lock_guard<std::mutex> g(t->mu);
    S = t->S; fail_now = t->bins.fail_now;
  }
  return gmr::reset_done_launch(t, S, fail_now, n, d_env_ids, d_done, d_failed, resample, lo, hi, (hipStream_t)stream);
}

int gmr_motion_tracker_reset_done(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* done, const int32_t* failed, int resample,
                                  float lo, float hi, int* ignored) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (ignored) *ignored = 0;
  int rc = gmr::subset_check(t->N, n, env_ids, nullptr);      // (the launch checks the rest)
  if (rc != GMR_OK) return rc;
  std::lock_guard<std::mutex> g(t->mu);
  const size_t nb = (size_t)n * 4;
  gmr::HostStage st;
  const int32_t *d_ids, *d_done, *d_failed;
  st.in(d_ids, env_ids, nb); st.in(d_done, done, nb); st.in(d_failed, failed, nb);
  GMR_STAGE_TRY(st, upload);
  gmr::IgnoredDelta ig(t->S.ignored, ignored);
  if ((rc = ig.begin()) == GMR_OK) rc = gmr::reset_done_launch(t, t->S, t->bins.fail_now, n, d_ids, d_done, d_failed, resample, lo, hi, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return ig.end();
}

int gmr_motion_tracker_adaptive_state(gmr_motion_tracker_t* t, int32_t* bin_start, uint32_t* fail_now, double* ema, double* prob, double* cdf) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  if (t->adaptive.Bt == 0) return gmr_fail(GMR_ERR_ARG, "adaptive sampling is not configured (gmr_motion_tracker_set_adaptive)");
  const size_t nb = (size_t)t->adaptive.Bt;
  return gmr::read_back({{bin_start, t->bin_tab.start, ((size_t)t->lib->A.C + 1) * 4}, {fail_now, t->bins.fail_now, nb * 4}, {ema, t->bins.ema, nb * 8},
                         {prob, t->bins.prob, nb * 8}, {cdf, t->bins.cdf, nb * 8}});
}

}  // extern "C"
