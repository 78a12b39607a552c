// jlinv_apply_probe.hip -- TEST-ONLY: se3_jlinv_coef5 / se3_jlinv_apply5 of csrc/gmr_device_math.h (included unchanged)
// on the GPU for tests/test_jlinv_apply.py.  One plain C entry point, host pointers in and out; the return value is 0 or
// the hipError_t of the first failing runtime call (negative: a rejected argument).  Built twice by
// build.build_jlinv_probe(), like math_probe.hip.  Nothing of this file is linked into libgmrhip.so.
#include <hip/hip_runtime.h>

#include "../../general_motion_retargeting_amd/csrc/gmr_device_math.h"
using namespace gmr;

namespace {

constexpr int kMaxN = 1 << 20;
constexpr int kBlock = 256;

#define PROBE_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
#define PROBE_RC(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

struct Buf {
  double* d = nullptr;
  size_t n = 0;
  ~Buf() { if (d) (void)hipFree(d); }
  int in(const double* h, size_t count) {
    n = count;
    PROBE_TRY(hipMalloc(&d, n * sizeof(double)));
    PROBE_TRY(hipMemcpy(d, h, n * sizeof(double), hipMemcpyHostToDevice));
    return 0;
  }
  int out(size_t count) {
    n = count;
    PROBE_TRY(hipMalloc(&d, n * sizeof(double)));
    PROBE_TRY(hipMemset(d, 0xff, n * sizeof(double)));     // NaN pattern: an element the kernel skipped shows
    return 0;
  }
  int back(double* h) const { PROBE_TRY(hipMemcpy(h, d, n * sizeof(double), hipMemcpyDeviceToHost)); return 0; }
};

// e[6], aux5[5], jl[3], ja[3] per element -> coef[8], [top; bot][6]
__global__ void k_apply(int n, const double* e, const double* aux, const double* jl, const double* ja, double* coef, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double ee[6], ax[5], cf[8];
  for (int r = 0; r < 6; r++) ee[r] = e[6 * i + r];
  for (int r = 0; r < 5; r++) ax[r] = aux[5 * i + r];
  se3_jlinv_coef5(ee, ax, cf);
  for (int r = 0; r < 8; r++) coef[8 * i + r] = cf[r];
  d3 top, bot;
  se3_jlinv_apply5(ee, cf, d3{jl[3 * i], jl[3 * i + 1], jl[3 * i + 2]}, d3{ja[3 * i], ja[3 * i + 1], ja[3 * i + 2]}, top, bot);
  double* o = out + 6 * i;
  o[0] = top.x; o[1] = top.y; o[2] = top.z; o[3] = bot.x; o[4] = bot.y; o[5] = bot.z;
}

}  // namespace

extern "C" int gmr_probe_jlinv_apply(int n, const double* e, const double* aux5, const double* jl, const double* ja, double* coef,
                                     double* out) {
  if (n <= 0 || n > kMaxN) return -1;
  Buf E, A, Jl, Ja, Cf, O;
  PROBE_RC(E.in(e, 6 * (size_t)n)); PROBE_RC(A.in(aux5, 5 * (size_t)n)); PROBE_RC(Jl.in(jl, 3 * (size_t)n)); PROBE_RC(Ja.in(ja, 3 * (size_t)n));
  PROBE_RC(Cf.out(8 * (size_t)n)); PROBE_RC(O.out(6 * (size_t)n));
  k_apply<<<(n + kBlock - 1) / kBlock, kBlock>>>(n, E.d, A.d, Jl.d, Ja.d, Cf.d, O.d);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_RC(Cf.back(coef));
  return O.back(out);
}
