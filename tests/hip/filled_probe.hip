// filled_probe.hip -- TEST-ONLY: the hazard-complete solver statements of csrc/gmr_device_math.h (row_bcast_fnma_pivot,
// row_backsub_fill, row_dot_backsub; the header is included unchanged) on the GPU for tests/test_filled_waits.py.  Plain C
// entry points, host pointers in and out; the return value is 0 or the hipError_t of the first failing runtime call
// (negative: a rejected argument).  One wavefront and one launch per kernel.  Built by build.build_filled_probe() under
// the library's flags.  Nothing of this file is linked into libgmrhip.so.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../general_motion_retargeting_amd/csrc/gmr_device_math.h"
using namespace gmr;

namespace {

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

template <int I0, int I1, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I0 < I1) {
    f(std::integral_constant<int, I0>{});
    static_for<I0 + 1, I1>(f);
  }
}

constexpr int NL = 7, NT = 9, NV = NL + NT;

// ---- (a) every statement against the composition of primitives it replaces -------------------------------------------
// in[IN_ROWS][64]: rows 0..15 r / f, 16 l, 17 acc, 18 dinv, 19 fs, 20 v, 21..29 m[9], 30..38 y[9].
// out[OUT_ROWS][64]: the fourteen pivots the solver issues (limb pivots 0..5: K = p + 1, N = 16 - K; trunk pivots 0..7:
// K = 8 + q, N = 16 - K), 17 rows each (r[0..15] with the untouched ones as they came, then d); the trunk back substitution
// (f[16], acc); the limb's dot product and back substitution (acc).
constexpr int IN_ROWS = 39, OUT_ROWS = 14 * 17 + 17 + 1;

template <int K, bool NEW>
__device__ __forceinline__ void pivot_case(const double* rin, double l, int lane, double* out) {
  constexpr int N = NV - K;
  double r[NV];
#pragma unroll
  for (int i = 0; i < NV; i++) r[i] = rin[i];
  double d;
  if constexpr (NEW) {
    d = row_bcast_fnma_pivot<K, N>(r + K, l);
  } else {
    d = row_bcast_fnma_bcast<K>(r[K], l);
    if constexpr (N > 1) row_bcast_fnma_cols<K + 1, N - 1>(r + K + 1, l);
  }
#pragma unroll
  for (int i = 0; i < NV; i++) out[i * 64 + lane] = r[i];
  out[NV * 64 + lane] = d;
}

template <bool NEW>
__device__ __forceinline__ void statements(const double* in, double* out) {
  const int lane = threadIdx.x;
  double r[NV], m[NT], y[NT];
#pragma unroll
  for (int i = 0; i < NV; i++) r[i] = in[i * 64 + lane];
  const double l = in[16 * 64 + lane], acc = in[17 * 64 + lane], dinv = in[18 * 64 + lane], fs = in[19 * 64 + lane], v = in[20 * 64 + lane];
#pragma unroll
  for (int i = 0; i < NT; i++) { m[i] = in[(21 + i) * 64 + lane]; y[i] = in[(30 + i) * 64 + lane]; }
  static_for<0, 6>([&](auto P) __attribute__((always_inline)) {          // limb pivots
    constexpr int p = decltype(P)::value;
    pivot_case<p + 1, NEW>(r, l, lane, out + p * 17 * 64);
  });
  static_for<0, 8>([&](auto Q) __attribute__((always_inline)) {          // trunk pivots
    constexpr int q = decltype(Q)::value;
    pivot_case<NL + q + 1, NEW>(r, l, lane, out + (6 + q) * 17 * 64);
  });
  double* o = out + 14 * 17 * 64;
  {
    double f[NV], a = acc;
#pragma unroll
    for (int i = 0; i < NV; i++) f[i] = r[i];
    if constexpr (NEW) {
      a = row_backsub_fill<NL>(a, dinv, m, f, fs);
    } else {
#pragma unroll
      for (int i = 0; i < NV; i++) f[i] = f[i] * fs;
      static_for<0, NT>([&](auto I) __attribute__((always_inline)) {
        constexpr int q = NT - 1 - decltype(I)::value;
        a = row_bcast_fma<NL + q, true>(a, a * dinv, m[q]);
      });
    }
#pragma unroll
    for (int i = 0; i < NV; i++) o[i * 64 + lane] = f[i];
    o[NV * 64 + lane] = a;
  }
  {
    double a = acc;
    if constexpr (NEW) {
      a = row_dot_backsub<NL, 0>(a, v, y, dinv, m);
    } else {
      a = row_bcast_fma_dot<NL, 1, NT, true>(a, v, y);
      static_for<0, NL>([&](auto I) __attribute__((always_inline)) {
        constexpr int p = NL - 1 - decltype(I)::value;
        a = row_bcast_fma<p, true>(a, a * dinv, m[p]);
      });
    }
    o[17 * 64 + lane] = a;
  }
}

__global__ void k_stmt(const double* in, double* filled, double* composed) {
  statements<true>(in, filled);
  statements<false>(in, composed);
}

// ---- (b) one local elimination and solve of the <7, 9> shape, as csrc/gmr_ik_tree.h issues it, written both ways -------
// Lane i of each 16-lane row holds row i of the local matrix (7 limb rows, 9 trunk rows); the four rows of the wavefront
// work on four cases at a time.  FILLED = true uses the hazard-complete statements at every site where the solver does,
// FILLED = false the per-step folded forms they replace (local_solve<true> of rowfma_probe.hip).  1 / sqrt(d) is the
// correctly rounded quotient of the correctly rounded root here, as there.  Output layout as there: per case and lane
// cols[16], own[16], schur[9], y, yt, x.
constexpr int OUT_PER_LANE = 16 + 16 + 9 + 3;

template <bool FILLED>
__device__ __forceinline__ void local_solve(const double* A, const double* rhs, unsigned fixedmask, int lane, double* o) {
  const bool is_limb = lane < NL, is_trunk = lane >= NL;
  const int t = lane - NL;
  const bool self_fixed = (fixedmask >> lane) & 1u;
  double h[NV], r[NV];
#pragma unroll
  for (int m = 0; m < NV; m++) h[m] = A[lane * NV + m];
#pragma unroll
  for (int m = 0; m < NL; m++) {
    const bool cfixed = (fixedmask >> m) & 1u;
    double v = (!self_fixed && !cfixed) ? h[m] : 0.0;
    if (is_limb && m == lane && (self_fixed || cfixed)) v = 1.0;
    r[m] = v;
  }
#pragma unroll
  for (int u = 0; u < NT; u++) {
    const bool cfixed = (fixedmask >> (NL + u)) & 1u;
    r[NL + u] = (is_limb && !self_fixed && !cfixed) ? h[NL + u] : 0.0;
  }
  const double rhs0 = rhs[lane];
  double b = is_limb ? rhs0 : 0.0;
  // limb pivots
  double mydinv = 1.0;
  double dp = row_bcast_d(r[0], 0);
  double dinv = 1.0 / sqrt(dp);
  static_for<0, NL>([&](auto P) __attribute__((always_inline)) {
    constexpr int p = decltype(P)::value;
    const double rs = r[p] * dinv;
    const double l = lane > p ? rs : 0.0;
    o[p] = lane >= p ? rs : 0.0;
    if (lane == p) mydinv = dinv;
    double dinv_next = 1.0;
    if constexpr (p + 1 < NL) {
      if constexpr (FILLED) dp = row_bcast_fnma_pivot<p + 1, NV - p - 1>(r + p + 1, l);
      else dp = row_bcast_fnma_bcast<p + 1>(r[p + 1], l);
      dinv_next = 1.0 / sqrt(dp);
    }
    const double yp = row_bcast_d(b, p) * dinv;
    b = fma(-l, yp, b);
    constexpr int k0 = p + 1 < NL ? p + 2 : p + 1;
    if constexpr (!(FILLED && p + 1 < NL)) row_bcast_fnma_cols<k0, NV - k0>(r + k0, l);
    dinv = dinv_next;
  });
  if (is_limb) b *= mydinv;
  double ltl[NL], yl[NT];
  if constexpr (!FILLED) {
#pragma unroll
    for (int m = 0; m < NL; m++) ltl[m] = (is_limb && m > lane) ? r[m] * mydinv : 0.0;
#pragma unroll
    for (int u = 0; u < NT; u++) yl[u] = r[NL + u] * mydinv;
  }
#pragma unroll
  for (int u = 0; u < NT; u++) o[32 + u] = r[NL + u];
  o[41] = b;
  // trunk: H's trunk block plus this limb's Schur part
  double s[NT];
  const bool live = is_trunk && !self_fixed;
#pragma unroll
  for (int u = 0; u < NT; u++) {
    const bool cfixed = (fixedmask >> (NL + u)) & 1u;
    double v = (live && !cfixed) ? h[NL + u] + r[NL + u] : 0.0;
    if (is_trunk && u == t && !(live && !cfixed)) v = 1.0;
    s[u] = v;
  }
  double bt = is_trunk ? (live ? rhs0 + b : rhs0) : 0.0;
  double tdinv = 1.0;
  double dq = row_bcast_d(s[0], NL);
  dinv = 1.0 / sqrt(dq);
  static_for<0, NT>([&](auto Q) __attribute__((always_inline)) {
    constexpr int q = decltype(Q)::value;
    const double ss = s[q] * dinv;
    const double l = t > q ? ss : 0.0;
    o[NL + q] = t >= q ? ss : 0.0;
    if (t == q) tdinv = dinv;
    double dinv_next = 1.0;
    if constexpr (q + 1 < NT) {
      if constexpr (FILLED) dq = row_bcast_fnma_pivot<NL + q + 1, NT - q - 1>(s + q + 1, l);
      else dq = row_bcast_fnma_bcast<NL + q + 1>(s[q + 1], l);
      dinv_next = 1.0 / sqrt(dq);
    }
    const double yq = row_bcast_d(bt, NL + q) * dinv;
    bt = fma(-l, yq, bt);
    if constexpr (!FILLED && q + 2 < NT) row_bcast_fnma_cols<NL + q + 2, NT - q - 2>(s + q + 2, l);
    dinv = dinv_next;
  });
  double lt[NT];
#pragma unroll
  for (int q = 0; q < NT; q++) lt[q] = (is_trunk && q > t) ? s[q] * tdinv : 0.0;
  if (is_trunk) {
#pragma unroll
    for (int q = 0; q < NT; q++) o[16 + NL + q] = lt[q];
  }
  bt *= tdinv;
  o[42] = bt;
  if constexpr (FILLED) {
    double f[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) f[j] = r[(NL + j) % NV];
    bt = row_backsub_fill<NL>(bt, tdinv, lt, f, mydinv);
#pragma unroll
    for (int u = 0; u < NT; u++) yl[u] = f[u];
#pragma unroll
    for (int m = 0; m < NL; m++) ltl[m] = (is_limb && m > lane) ? f[NT + m] : 0.0;
  } else {
    static_for<0, NT>([&](auto I) __attribute__((always_inline)) {
      constexpr int q = NT - 1 - decltype(I)::value;
      bt = row_bcast_fma<NL + q, true>(bt, bt * tdinv, lt[q]);
    });
  }
  if (is_limb) {
#pragma unroll
    for (int m = 0; m < NL; m++) o[16 + m] = ltl[m];
#pragma unroll
    for (int u = 0; u < NT; u++) o[16 + NL + u] = yl[u];
  }
  bt *= tdinv;
  // limbs: y_l - Y_l^T x_T, back substitution
  double x = bt, bb = b;
  if constexpr (FILLED) {
    bb = row_dot_backsub<NL, 0>(bb, bt, yl, mydinv, ltl);
  } else {
    bb = row_bcast_fma_dot<NL, 1, NT, true>(bb, bt, yl);
    static_for<0, NL>([&](auto I) __attribute__((always_inline)) {
      constexpr int p = NL - 1 - decltype(I)::value;
      bb = row_bcast_fma<p, true>(bb, bb * mydinv, ltl[p]);
    });
  }
  if (is_limb) x = bb * mydinv;
  o[43] = x;
}

// ncase cases (padded by the caller to a multiple of 4): A[ncase][16][16], rhs[ncase][16], fixedmask[ncase] (as doubles)
__global__ void k_elim(int ncase, const double* A, const double* rhs, const double* fixedmask, double* filled, double* stepwise) {
  const int row = threadIdx.x >> 4, lane = threadIdx.x & 15;
  for (int c0 = 0; c0 < ncase; c0 += 4) {          // (uniform trip count: all 64 lanes stay enabled)
    const int c = c0 + row;
    const unsigned fm = (unsigned)fixedmask[c];
    double of[OUT_PER_LANE], op[OUT_PER_LANE];
#pragma unroll
    for (int i = 0; i < OUT_PER_LANE; i++) { of[i] = 0.0; op[i] = 0.0; }
    local_solve<true>(A + c * NV * NV, rhs + c * NV, fm, lane, of);
    local_solve<false>(A + c * NV * NV, rhs + c * NV, fm, lane, op);
#pragma unroll
    for (int i = 0; i < OUT_PER_LANE; i++) {
      filled[(c * NV + lane) * OUT_PER_LANE + i] = of[i];
      stepwise[(c * NV + lane) * OUT_PER_LANE + i] = op[i];
    }
  }
}

}  // namespace

extern "C" int gmr_probe_filled_in_rows() { return IN_ROWS; }
extern "C" int gmr_probe_filled_out_rows() { return OUT_ROWS; }

extern "C" int gmr_probe_filled_stmt(const double* in, double* filled, double* composed) {
  Buf I, F, Cc;
  PROBE_RC(I.in(in, (size_t)IN_ROWS * 64));
  PROBE_RC(F.out((size_t)OUT_ROWS * 64)); PROBE_RC(Cc.out((size_t)OUT_ROWS * 64));
  k_stmt<<<1, 64>>>(I.d, F.d, Cc.d);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_RC(F.back(filled));
  return Cc.back(composed);
}

extern "C" int gmr_probe_filled_out_per_lane() { return OUT_PER_LANE; }

extern "C" int gmr_probe_filled_elim(int ncase, const double* A, const double* rhs, const double* fixedmask, double* filled, double* stepwise) {
  if (ncase <= 0 || ncase > 64 || ncase % 4 != 0) return -1;
  Buf Ad, Rd, Fd, O1, O2;
  PROBE_RC(Ad.in(A, (size_t)ncase * NV * NV)); PROBE_RC(Rd.in(rhs, (size_t)ncase * NV)); PROBE_RC(Fd.in(fixedmask, (size_t)ncase));
  PROBE_RC(O1.out((size_t)ncase * NV * OUT_PER_LANE)); PROBE_RC(O2.out((size_t)ncase * NV * OUT_PER_LANE));
  k_elim<<<1, 64>>>(ncase, Ad.d, Rd.d, Fd.d, O1.d, O2.d);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_RC(O1.back(filled));
  return O2.back(stepwise);
}
