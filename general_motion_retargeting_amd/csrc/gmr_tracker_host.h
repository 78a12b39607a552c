// gmr_tracker_host.h -- what the entry points of the motion tracker (gmr_tracker*.hip) share on the host (not part of the C-ABI): the
// check of a noise spec, the check of a list of environments, the two grid sizes, and, where HIP compiles it, the ignored-id count of a
// synchronous call, the allocation of a block's state and the read-back of a *_state call.  The upper half asks nothing of the HIP
// runtime, so that tests/cpp/tracker_host_check.cpp drives it under plain g++ with a gmr_fail of its own, as gmr_workspace.h is driven.
#ifndef GMR_TRACKER_HOST_H
#define GMR_TRACKER_HOST_H
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <initializer_list>

#include "../../include/gmr_hip.h"
#include "gmr_internal.h"
#include "gmr_workspace.h"

namespace gmr {

// one noise spec as the kernels apply it (tracker_noise, gmr_tracker_dev.h): n = a + m * (z or u), then x + n or x * n
struct ProprioNoise {
  int32_t dist = 0, op = 0;                 // GMR_NOISE_NONE / _GAUSSIAN / _UNIFORM, GMR_NOISE_ADDITIVE / _SCALING
  float a = 0.0f, m = 0.0f;                 // gaussian: (float)mu, (float)sigma; uniform: (float)lower, (float)(upper - lower), the span formed in double
};

// finite, and finite as a float32 too
inline bool fits(double x) { return std::isfinite(x) && std::isfinite((float)x); }

// The spec `name` of a configuration into the form the kernels read; the messages start with the name.
inline int noise_spec(const gmr_proprio_noise_t& s, const char* name, ProprioNoise* out) {
  *out = ProprioNoise{};
  if (s.distribution < GMR_NOISE_NONE || s.distribution > GMR_NOISE_UNIFORM) return gmr_fail(GMR_ERR_ARG, "%s: distribution = %d", name, s.distribution);
  if (s.distribution == GMR_NOISE_NONE) return GMR_OK;
  if (s.operation != GMR_NOISE_ADDITIVE && s.operation != GMR_NOISE_SCALING) return gmr_fail(GMR_ERR_ARG, "%s: operation = %d", name, s.operation);
  if (!fits(s.a) || !fits(s.b)) return gmr_fail(GMR_ERR_ARG, "%s: range (%g, %g) is not finite", name, s.a, s.b);
  if (s.distribution == GMR_NOISE_GAUSSIAN && s.b < 0.0) return gmr_fail(GMR_ERR_ARG, "%s: a gaussian's deviation %g is negative", name, s.b);
  out->dist = s.distribution;
  out->op = s.operation;
  out->a = (float)s.a;
  out->m = s.distribution == GMR_NOISE_GAUSSIAN ? (float)s.b : (float)(s.b - s.a);
  if (!std::isfinite(out->m)) return gmr_fail(GMR_ERR_ARG, "%s: range (%g, %g) is too wide", name, s.a, s.b);
  return GMR_OK;
}

// A list of n entries over N environments: n in range, and without env_ids entry i is environment i, so n = N.  `phrase` says what
// then covers every environment; null: the caller has a rule of its own for a missing list, and only the range is checked.
inline int subset_check(int N, int n, const void* ids, const char* phrase) {
  if (n < 0 || n > (1 << 26)) return gmr_fail(GMR_ERR_ARG, "n = %d out of range", n);
  if (phrase && !ids && n != N) return gmr_fail(GMR_ERR_ARG, "without env_ids %s: n = %d, N = %d", phrase, n, N);
  return GMR_OK;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// workgroups of 256 lanes: one lane per item, and one row of `lanes` lanes per item
inline unsigned lane_blocks(long long n) { return (unsigned)((n + 255) / 256); }
inline unsigned row_blocks(int n, int lanes) {
  const int per_block = 256 / lanes;
  return (unsigned)((n + per_block - 1) / per_block);
}

#ifdef __HIPCC__
// the ids outside [0, N) counted so far at d_counter (TrackerState::ignored); synchronous
inline int read_ignored(const uint32_t* d_counter, uint32_t* value) {
  GMR_HIP_TRY(hipMemcpy(value, d_counter, 4, hipMemcpyDeviceToHost));
  return GMR_OK;
}
// What a synchronous entry point reports as *ignored: begin() before its launch, end() after its wait.
class IgnoredDelta {
 public:
  IgnoredDelta(const uint32_t* d_counter, int* ignored) : d_(d_counter), out_(ignored) {}
  int begin() { return read_ignored(d_, &before_); }
  int end() {
    uint32_t after = 0;
    const int rc = read_ignored(d_, &after);
    if (rc == GMR_OK && out_) *out_ = (int)(after - before_);
    return rc;
  }

 private:
  const uint32_t* d_;
  int* out_;
  uint32_t before_ = 0;
};

// The state of a set_* call: the device is idle (nothing in flight reads the arrays a larger block replaces), the block holds the
// carved fields and they are all zero.
inline int fresh_block(DeviceBlock& block, const Carve& cv) {
  GMR_HIP_TRY(hipDeviceSynchronize());
  GMR_HIP_TRY(block.reserve(cv.total() + 256));
  GMR_HIP_TRY(hipMemset(block.data(), 0, cv.total()));
  GMR_HIP_TRY(hipDeviceSynchronize());
  return GMR_OK;
}

// A *_state call: wait for the device, then one copy per destination that is not null.
struct ReadBack {
  void* host;
  const void* dev;
  size_t bytes;
};
inline int read_back(std::initializer_list<ReadBack> arrays) {
  GMR_HIP_TRY(hipDeviceSynchronize());
  for (const ReadBack& a : arrays)
    if (a.host) GMR_HIP_TRY(hipMemcpy(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost));
  return GMR_OK;
}
#endif

}  // namespace gmr
#endif
