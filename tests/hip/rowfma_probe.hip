// rowfma_probe.hip -- TEST-ONLY: the folded row broadcasts (row_bcast_fma and its multi-update forms) and div_const of
// csrc/gmr_device_math.h (included unchanged) on the GPU for tests/test_row_bcast_fma.py.  Plain C entry points, host
// pointers in and out; the return value is 0 or the hipError_t of the first failing runtime call (negative: a rejected
// argument).  Every kernel is one launch; (a) and (b) run one wavefront.  Built by build.build_rowfma_probe() under the
// library's flags.  Nothing of this file is linked into libgmrhip.so.
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

// ---- (a) the primitive against fma(+-row_bcast_d(v, K), m, acc): out[(2 K + sign) * 64 + lane], sign 1 = minus ----------
__global__ void k_prim(const double* v, const double* m, const double* acc, double* prim, double* ref) {
  const int lane = threadIdx.x;
  const double vv = v[lane], mm = m[lane], aa = acc[lane];
  static_for<0, 16>([&](auto KK) __attribute__((always_inline)) {
    constexpr int K = decltype(KK)::value;
    prim[(2 * K) * 64 + lane] = row_bcast_fma<K, false>(aa, vv, mm);
    prim[(2 * K + 1) * 64 + lane] = row_bcast_fma<K, true>(aa, vv, mm);
    ref[(2 * K) * 64 + lane] = fma(row_bcast_d(vv, K), mm, aa);
    ref[(2 * K + 1) * 64 + lane] = fma(-row_bcast_d(vv, K), mm, aa);
  });
}

// ---- (b) one local elimination and solve of the <7, 9> shape, as csrc/gmr_ik_tree.h issues it, written both ways -------
// Lane i of each 16-lane row holds row i of the local matrix (7 limb rows, 9 trunk rows); the four rows of the wavefront
// work on four cases at a time.  FOLD = true uses the folded forms at every site where the solver does, FOLD = false
// row_bcast_d + fma.  1 / sqrt(d) is the correctly rounded quotient of the correctly rounded root here (any function of
// d_p that every lane is given alike serves the comparison; this one is what tests/tree_sym_mirror.py uses).
constexpr int NL = 7, NT = 9, NV = NL + NT;
// per case and lane: cols[16] (column p of the lower factor as this lane sees it at pivot p: limb pivots 0..6, trunk
// pivots 7..15), own[16] (the lane's own row times its own 1 / sqrt(d): ltl[7] then yl[9] for a limb lane, lt[9] at 7..15
// for a trunk lane), schur[9] (trunk columns after the limb pivots), y (substituted right-hand side: limb phase), yt
// (trunk phase), x (solution)
constexpr int OUT_PER_LANE = 16 + 16 + 9 + 3;

template <bool FOLD>
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
      if constexpr (FOLD) {
        dp = row_bcast_fnma_bcast<p + 1>(r[p + 1], l);
      } else {
        r[p + 1] = fma(-l, row_bcast_d(l, p + 1), r[p + 1]);
        dp = row_bcast_d(r[p + 1], p + 1);
      }
      dinv_next = 1.0 / sqrt(dp);
    }
    const double yp = row_bcast_d(b, p) * dinv;
    b = fma(-l, yp, b);
    constexpr int k0 = p + 1 < NL ? p + 2 : p + 1;
    if constexpr (FOLD) {
      row_bcast_fnma_cols<k0, NV - k0>(r + k0, l);
    } else {
#pragma unroll
      for (int k = k0; k < NV; k++) r[k] = fma(-l, row_bcast_d(l, k), r[k]);
    }
    dinv = dinv_next;
  });
  if (is_limb) b *= mydinv;
  double ltl[NL], yl[NT];
#pragma unroll
  for (int m = 0; m < NL; m++) ltl[m] = (is_limb && m > lane) ? r[m] * mydinv : 0.0;
#pragma unroll
  for (int u = 0; u < NT; u++) yl[u] = r[NL + u] * mydinv;
  if (is_limb) {
#pragma unroll
    for (int m = 0; m < NL; m++) o[16 + m] = ltl[m];
#pragma unroll
    for (int u = 0; u < NT; u++) o[16 + NL + u] = yl[u];
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
      if constexpr (FOLD) {
        dq = row_bcast_fnma_bcast<NL + q + 1>(s[q + 1], l);
      } else {
        s[q + 1] = fma(-l, row_bcast_d(l, NL + q + 1), s[q + 1]);
        dq = row_bcast_d(s[q + 1], NL + q + 1);
      }
      dinv_next = 1.0 / sqrt(dq);
    }
    const double yq = row_bcast_d(bt, NL + q) * dinv;
    bt = fma(-l, yq, bt);
    if constexpr (FOLD && q + 2 < NT) {
      row_bcast_fnma_cols<NL + q + 2, NT - q - 2>(s + q + 2, l);
    } else {
#pragma unroll
      for (int k = q + 2; k < NT; k++) s[k] = fma(-l, row_bcast_d(l, NL + k), s[k]);
    }
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
  if constexpr (FOLD) {
    static_for<0, NT>([&](auto I) __attribute__((always_inline)) {
      constexpr int q = NT - 1 - decltype(I)::value;
      bt = row_bcast_fma<NL + q, true>(bt, bt * tdinv, lt[q]);
    });
  } else {
#pragma unroll
    for (int q = NT - 1; q >= 0; q--) bt = fma(-lt[q], row_bcast_d(bt * tdinv, NL + q), bt);
  }
  bt *= tdinv;
  // limbs: y_l - Y_l^T x_T, back substitution
  double x = bt, bb = b;
  if constexpr (FOLD) {
    bb = row_bcast_fma_dot<NL, 1, NT, true>(bb, bt, yl);
    static_for<0, NL>([&](auto I) __attribute__((always_inline)) {
      constexpr int p = NL - 1 - decltype(I)::value;
      bb = row_bcast_fma<p, true>(bb, bb * mydinv, ltl[p]);
    });
  } else {
#pragma unroll
    for (int u = 0; u < NT; u++) {
      const double xt = row_bcast_d(bt, NL + u);
      if (is_limb) bb = fma(-yl[u], xt, bb);
    }
#pragma unroll
    for (int p = NL - 1; p >= 0; p--) bb = fma(-ltl[p], row_bcast_d(bb * mydinv, p), bb);
  }
  if (is_limb) x = bb * mydinv;
  o[43] = x;
}

// ncase cases (padded by the caller to a multiple of 4): A[ncase][16][16], rhs[ncase][16], fixedmask[ncase] (as doubles)
__global__ void k_elim(int ncase, const double* A, const double* rhs, const double* fixedmask, double* folded, double* plain) {
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
      folded[(c * NV + lane) * OUT_PER_LANE + i] = of[i];
      plain[(c * NV + lane) * OUT_PER_LANE + i] = op[i];
    }
  }
}

// ---- (c) div_const against the division, per literal: x[9][n] -> helper[9][n], quotient[9][n] ---------------------------
#define DIV_CASE(I, C) case I: hq = div_const(xv, C); dq = xv / C; break;
__global__ void k_div(int n, const double* x, double* helper, double* quotient) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int lit = blockIdx.y;
  const double xv = x[(size_t)lit * n + i];
  double hq = 0.0, dq = 0.0;
  switch (lit) {
    DIV_CASE(0, 6.0) DIV_CASE(1, 120.0) DIV_CASE(2, 720.0) DIV_CASE(3, 5040.0) DIV_CASE(4, 40320.0) DIV_CASE(5, 362880.0)
    DIV_CASE(6, 3628800.0) DIV_CASE(7, 39916800.0) DIV_CASE(8, 47900160.0)
  }
  helper[(size_t)lit * n + i] = hq;
  quotient[(size_t)lit * n + i] = dq;
}

}  // namespace

extern "C" int gmr_probe_rowfma_prim(const double* v, const double* m, const double* acc, double* prim, double* ref) {
  Buf V, M, A, P, R;
  PROBE_RC(V.in(v, 64)); PROBE_RC(M.in(m, 64)); PROBE_RC(A.in(acc, 64));
  PROBE_RC(P.out(32 * 64)); PROBE_RC(R.out(32 * 64));
  k_prim<<<1, 64>>>(V.d, M.d, A.d, P.d, R.d);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_RC(P.back(prim));
  return R.back(ref);
}

extern "C" int gmr_probe_rowfma_out_per_lane() { return OUT_PER_LANE; }

extern "C" int gmr_probe_rowfma_elim(int ncase, const double* A, const double* rhs, const double* fixedmask, double* folded, double* plain) {
  if (ncase <= 0 || ncase > 64 || ncase % 4 != 0) return -1;
  Buf Ad, Rd, Fd, O1, O2;
  PROBE_RC(Ad.in(A, (size_t)ncase * NV * NV)); PROBE_RC(Rd.in(rhs, (size_t)ncase * NV)); PROBE_RC(Fd.in(fixedmask, (size_t)ncase));
  PROBE_RC(O1.out((size_t)ncase * NV * OUT_PER_LANE)); PROBE_RC(O2.out((size_t)ncase * NV * OUT_PER_LANE));
  k_elim<<<1, 64>>>(ncase, Ad.d, Rd.d, Fd.d, O1.d, O2.d);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_RC(O1.back(folded));
  return O2.back(plain);
}

extern "C" int gmr_probe_div_const_literals() { return 9; }

extern "C" int gmr_probe_div_const(int n, const double* x, double* helper, double* quotient) {
  if (n <= 0 || n > (1 << 20)) return -1;
  Buf X, Hq, Dq;
  PROBE_RC(X.in(x, 9 * (size_t)n)); PROBE_RC(Hq.out(9 * (size_t)n)); PROBE_RC(Dq.out(9 * (size_t)n));
  k_div<<<dim3((n + 255) / 256, 9), 256>>>(n, X.d, Hq.d, Dq.d);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_RC(Hq.back(helper));
  return Dq.back(quotient);
}
