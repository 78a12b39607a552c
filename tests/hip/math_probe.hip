// math_probe.hip -- TEST-ONLY: calls every function of csrc/gmr_device_math.h (included unchanged) on the GPU so that
// tests/test_device_math.py can compare each primitive with the multiprecision fixture.  Plain C entry points, host
// pointers in and out; each call allocates, copies, launches one small grid and frees.  The return value is 0 or the
// hipError_t of the first failing runtime call (negative: a rejected argument).  Built twice by build.build_probe():
// with the product's FLAGS and with the PER_SOURCE_FLAGS of gmr_ik_wide.hip added, because the shipped library
// instantiates the header under both.  Nothing of this file is linked into libgmrhip.so.
#include <hip/hip_runtime.h>

#include "../../general_motion_retargeting_amd/csrc/gmr_device_math.h"
using namespace gmr;

namespace {

constexpr int kMaxN = 1 << 20;   // elements per call
constexpr int kBlock = 256;

#define PROBE_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// device copies of the inputs / room for the outputs of one call; freed when the call returns
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
#define PROBE_RC(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

int finish() {
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  return 0;
}
inline int grid(int n) { return (n + kBlock - 1) / kBlock; }
inline bool bad(int n) { return n <= 0 || n > kMaxN; }

__global__ void k_rcp_rsqrt(int n, const double* x, double* rc, double* rs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  rc[i] = fast_rcp(x[i]);
  rs[i] = fast_rsqrt(x[i]);
}
__global__ void k_sincos(int n, const double* x, double* s, double* c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sincos_small(x[i], &s[i], &c[i]);
}
__global__ void k_atan2(int n, const double* yx, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  o[i] = atan2_q1(yx[2 * i], yx[2 * i + 1]);
}
__global__ void k_so3_log(int n, const double* q, double* w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const d3 r = so3_log(d4{q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]});
  w[3 * i] = r.x; w[3 * i + 1] = r.y; w[3 * i + 2] = r.z;
}
__global__ void k_vinv(int n, const double* t2, double* a, double* asc, double* sn, double* cs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a[i] = vinv_coef(t2[i]);
  asc[i] = vinv_coef_sc(t2[i], sn[i], cs[i]);
}

struct Pose { d3 pb; d4 qb; d3 pt; d4 qt; };
__device__ Pose load_pose(const double* p) {
  return {d3{p[0], p[1], p[2]}, d4{p[3], p[4], p[5], p[6]}, d3{p[7], p[8], p[9]}, d4{p[10], p[11], p[12], p[13]}};
}
__global__ void k_se3_log(int n, const double* in, double* e, double* aux, double* e5, double* aux5) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Pose P = load_pose(in + 14 * i);
  double ee[6], ax[3], ee5[6], ax5[5];
  se3_log_rel(P.pb, P.qb, P.pt, P.qt, ee, ax);
  se3_log_rel5(P.pb, P.qb, P.pt, P.qt, ee5, ax5);
  for (int r = 0; r < 6; r++) { e[6 * i + r] = ee[r]; e5[6 * i + r] = ee5[r]; }
  for (int r = 0; r < 3; r++) aux[3 * i + r] = ax[r];
  for (int r = 0; r < 5; r++) aux5[5 * i + r] = ax5[r];
}
// A | B (row-major, 18 numbers) of the three Jl^-1 versions from what the two logs hand over
__device__ void jlinv_all(const double e[6], const double aux[3], const double e5[6], const double aux5[5], double* ab, double* ab5,
                          double* abc) {
  m3 A, B;
  se3_jlinv_aux(e, aux, A, B);
  for (int r = 0; r < 9; r++) { ab[r] = A.a[r]; ab[9 + r] = B.a[r]; }
  se3_jlinv_aux5(e5, aux5, A, B);
  for (int r = 0; r < 9; r++) { ab5[r] = A.a[r]; ab5[9 + r] = B.a[r]; }
  for (int j = 0; j < 3; j++) {
    double Ac[3], Bc[3];
    se3_jlinv_col5(e5, aux5, j, Ac, Bc);
    for (int r = 0; r < 3; r++) { abc[3 * r + j] = Ac[r]; abc[9 + 3 * r + j] = Bc[r]; }
  }
}
__global__ void k_se3_jlinv(int n, const double* in, double* ab, double* ab5, double* abc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Pose P = load_pose(in + 14 * i);
  double e[6], aux[3], e5[6], aux5[5];
  se3_log_rel(P.pb, P.qb, P.pt, P.qt, e, aux);
  se3_log_rel5(P.pb, P.qb, P.pt, P.qt, e5, aux5);
  jlinv_all(e, aux, e5, aux5, ab + 18 * i, ab5 + 18 * i, abc + 18 * i);
}
// Jl^-1 at a given tangent e with |w|^2 < 1e-2, where both logs hand over a = vinv_coef(|w|^2) and the sentinels
__global__ void k_se3_jlinv_e(int n, const double* ein, double* ab, double* ab5, double* abc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double e[6];
  for (int r = 0; r < 6; r++) e[r] = ein[6 * i + r];
  const double t2 = dot(d3{e[3], e[4], e[5]}, d3{e[3], e[4], e[5]});
  double aux[3], aux5[5] = {0.0, 0.0, 1.0, 0.0, 0.0};
  aux[0] = vinv_coef_sc(t2, aux[1], aux[2]);
  aux5[0] = aux[0];
  jlinv_all(e, aux, e, aux5, ab + 18 * i, ab5 + 18 * i, abc + 18 * i);
}
// in: qa[4] qb[4] v[3] axis[3] angle;  out: qnormalize(qa)[4], qrot(qn, v)[3], qrot_inv(qn, v)[3], qmul(qa, qb)[4], axis_angle[4]
__global__ void k_quat(int n, const double* in, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* p = in + 15 * i;
  double* r = o + 18 * i;
  const d4 qa = {p[0], p[1], p[2], p[3]}, qb = {p[4], p[5], p[6], p[7]};
  const d3 v = {p[8], p[9], p[10]};
  const d4 qn = qnormalize(qa);
  const d3 a = qrot(qn, v), b = qrot_inv(qn, v);
  const d4 m = qmul(qa, qb), aa = axis_angle(d3{p[11], p[12], p[13]}, p[14]);
  r[0] = qn.w; r[1] = qn.x; r[2] = qn.y; r[3] = qn.z;
  r[4] = a.x; r[5] = a.y; r[6] = a.z; r[7] = b.x; r[8] = b.y; r[9] = b.z;
  r[10] = m.w; r[11] = m.x; r[12] = m.y; r[13] = m.z;
  r[14] = aa.w; r[15] = aa.x; r[16] = aa.y; r[17] = aa.z;
}

// One wave64 block per input set, every lane active.  Output rows of 64, in this order (GMR_PROBE_LANE_ROWS of them):
// wave_sum, wave_min, wave_max, dpp_row_shr n = 1, 2, 4, 8 (with `fill`), dpp_swap_pairs, row_bcast_d k = 0..15,
// row0_sum (lanes 16..63 fed 0), row0_sum (all lanes fed), row0_min, rows3_max, fresh_lane.
constexpr int kLaneRows = 29;
__global__ void __launch_bounds__(64) k_lanes(const double* x, const double* fill, double* out) {
  const int lane = threadIdx.x;
  const double v = x[64 * blockIdx.x + lane], f = fill[blockIdx.x];
  double* o = out + (size_t)blockIdx.x * kLaneRows * 64 + lane;
  int r = 0;
  o[64 * r++] = wave_sum(v);
  o[64 * r++] = wave_min(v);
  o[64 * r++] = wave_max(v);
  o[64 * r++] = dpp_row_shr(v, f, 1);
  o[64 * r++] = dpp_row_shr(v, f, 2);
  o[64 * r++] = dpp_row_shr(v, f, 4);
  o[64 * r++] = dpp_row_shr(v, f, 8);
  o[64 * r++] = dpp_swap_pairs(v);
#pragma unroll
  for (int k = 0; k < 16; k++) o[64 * r++] = row_bcast_d(v, k);
  o[64 * r++] = row0_sum(lane < 16 ? v : 0.0);
  o[64 * r++] = row0_sum(v);
  o[64 * r++] = row0_min(v);
  o[64 * r++] = rows3_max(v);
  o[64 * r++] = (double)fresh_lane(lane);
}

}  // namespace

extern "C" {

int gmr_probe_lane_rows() { return kLaneRows; }

int gmr_probe_rcp_rsqrt(int n, const double* x, double* rcp, double* rsqrt) {
  if (bad(n)) return -1;
  Buf X, A, B;
  PROBE_RC(X.in(x, n)); PROBE_RC(A.out(n)); PROBE_RC(B.out(n));
  k_rcp_rsqrt<<<grid(n), kBlock>>>(n, X.d, A.d, B.d);
  PROBE_RC(finish());
  PROBE_RC(A.back(rcp));
  return B.back(rsqrt);
}
int gmr_probe_sincos_small(int n, const double* x, double* sn, double* cs) {
  if (bad(n)) return -1;
  Buf X, A, B;
  PROBE_RC(X.in(x, n)); PROBE_RC(A.out(n)); PROBE_RC(B.out(n));
  k_sincos<<<grid(n), kBlock>>>(n, X.d, A.d, B.d);
  PROBE_RC(finish());
  PROBE_RC(A.back(sn));
  return B.back(cs);
}
int gmr_probe_atan2_q1(int n, const double* yx, double* out) {
  if (bad(n)) return -1;
  Buf X, A;
  PROBE_RC(X.in(yx, 2 * (size_t)n)); PROBE_RC(A.out(n));
  k_atan2<<<grid(n), kBlock>>>(n, X.d, A.d);
  PROBE_RC(finish());
  return A.back(out);
}
int gmr_probe_so3_log(int n, const double* q, double* w) {
  if (bad(n)) return -1;
  Buf X, A;
  PROBE_RC(X.in(q, 4 * (size_t)n)); PROBE_RC(A.out(3 * (size_t)n));
  k_so3_log<<<grid(n), kBlock>>>(n, X.d, A.d);
  PROBE_RC(finish());
  return A.back(w);
}
int gmr_probe_vinv_coef(int n, const double* t2, double* a, double* a_sc, double* sin_t, double* cos_t) {
  if (bad(n)) return -1;
  Buf X, A, B, S, Cc;
  PROBE_RC(X.in(t2, n)); PROBE_RC(A.out(n)); PROBE_RC(B.out(n)); PROBE_RC(S.out(n)); PROBE_RC(Cc.out(n));
  k_vinv<<<grid(n), kBlock>>>(n, X.d, A.d, B.d, S.d, Cc.d);
  PROBE_RC(finish());
  PROBE_RC(A.back(a)); PROBE_RC(B.back(a_sc)); PROBE_RC(S.back(sin_t));
  return Cc.back(cos_t);
}
// poses: pb[3] qb[4] pt[3] qt[4] per element
int gmr_probe_se3_log(int n, const double* poses, double* e, double* aux, double* e5, double* aux5) {
  if (bad(n)) return -1;
  Buf X, E, A, E5, A5;
  PROBE_RC(X.in(poses, 14 * (size_t)n)); PROBE_RC(E.out(6 * (size_t)n)); PROBE_RC(A.out(3 * (size_t)n));
  PROBE_RC(E5.out(6 * (size_t)n)); PROBE_RC(A5.out(5 * (size_t)n));
  k_se3_log<<<grid(n), kBlock>>>(n, X.d, E.d, A.d, E5.d, A5.d);
  PROBE_RC(finish());
  PROBE_RC(E.back(e)); PROBE_RC(A.back(aux)); PROBE_RC(E5.back(e5));
  return A5.back(aux5);
}
// from_e == 0: poses as above;  from_e != 0: tangents e[6] with |w|^2 < 1e-2.  Outputs A | B, 18 numbers per element.
int gmr_probe_se3_jlinv(int n, int from_e, const double* in, double* ab_aux, double* ab_aux5, double* ab_col5) {
  if (bad(n)) return -1;
  Buf X, A, B, Cc;
  PROBE_RC(X.in(in, (from_e ? 6 : 14) * (size_t)n));
  PROBE_RC(A.out(18 * (size_t)n)); PROBE_RC(B.out(18 * (size_t)n)); PROBE_RC(Cc.out(18 * (size_t)n));
  if (from_e) k_se3_jlinv_e<<<grid(n), kBlock>>>(n, X.d, A.d, B.d, Cc.d);
  else k_se3_jlinv<<<grid(n), kBlock>>>(n, X.d, A.d, B.d, Cc.d);
  PROBE_RC(finish());
  PROBE_RC(A.back(ab_aux)); PROBE_RC(B.back(ab_aux5));
  return Cc.back(ab_col5);
}
int gmr_probe_quat(int n, const double* in, double* out) {
  if (bad(n)) return -1;
  Buf X, A;
  PROBE_RC(X.in(in, 15 * (size_t)n)); PROBE_RC(A.out(18 * (size_t)n));
  k_quat<<<grid(n), kBlock>>>(n, X.d, A.d);
  PROBE_RC(finish());
  return A.back(out);
}
// x[64 nset], fill[nset] -> out[nset][gmr_probe_lane_rows()][64]
int gmr_probe_lanes(int nset, const double* x, const double* fill, double* out) {
  if (nset <= 0 || nset > 4096) return -1;
  Buf X, F, A;
  PROBE_RC(X.in(x, 64 * (size_t)nset)); PROBE_RC(F.in(fill, nset)); PROBE_RC(A.out((size_t)nset * kLaneRows * 64));
  k_lanes<<<nset, 64>>>(X.d, F.d, A.d);
  PROBE_RC(finish());
  return A.back(out);
}

}  // extern "C"
