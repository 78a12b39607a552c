// split_eval_probe.hip -- TEST-ONLY, for tests/test_split_eval.py: (1) the two halves of se3_log_rel5 of
// csrc/gmr_device_math.h and the original, each in a kernel of its own, (2) the latency kernel's two walks of the kinematic tree (fk_wave<4, false>
// and qwalk_wave of csrc/gmr_ik.hip, included unchanged up to its walks) on one configuration.  Plain C entry points, host
// pointers in and out; the return value is 0 or the hipError_t of the first failing runtime call (negative: a rejected
// argument).  Built by build.build_split_probe().  Nothing of this file is linked into libgmrhip.so.
#define GMR_IK_WALKS_ONLY
#include "../../general_motion_retargeting_amd/csrc/gmr_ik.hip"
using namespace gmr;

namespace {

constexpr int kMaxN = 1 << 20;
constexpr int kBlock = 256;

#define PROBE_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
#define PROBE_RC(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

template <class T>
struct Buf {
  T* d = nullptr;
  size_t n = 0;
  ~Buf() { if (d) (void)hipFree(d); }
  int in(const T* h, size_t count) {
    n = count;
    PROBE_TRY(hipMalloc(&d, n * sizeof(T)));
    PROBE_TRY(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
  int out(size_t count) {
    n = count;
    PROBE_TRY(hipMalloc(&d, n * sizeof(T)));
    PROBE_TRY(hipMemset(d, 0xff, n * sizeof(T)));     // NaN pattern: an element the kernel skipped shows
    return 0;
  }
  int back(T* h) const { PROBE_TRY(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost)); return 0; }
};

// pose[14] = pb, qb, pt, qt per element -> out[11] = e[6], aux[5].  SPLIT: the two halves instead of se3_log_rel5 (a kernel
// each, so that neither form's compilation sees the other's expressions)
template <bool SPLIT>
__global__ void k_log(int n, const double* pose, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* x = pose + 14 * i;
  const d3 pb = {x[0], x[1], x[2]}, pt = {x[7], x[8], x[9]};
  const d4 qb = {x[3], x[4], x[5], x[6]}, qt = {x[10], x[11], x[12], x[13]};
  double e[6], aux[5];
  if (SPLIT) {
    se3_log_rel5_rot(qb, qt, e + 3, aux);
    se3_log_rel5_pos(pb, qb, pt, e + 3, aux[0], e);
  } else {
    se3_log_rel5(pb, qb, pt, qt, e, aux);
  }
  double* o = out + 11 * i;
  for (int r = 0; r < 6; r++) o[r] = e[r];
  for (int r = 0; r < 5; r++) o[6 + r] = aux[r];
}

// what the walks read of the kernel's layout
struct WalkLay {
  int nb, nhop;
  struct { int q, hsc, xa, xaxis; } o;
};
constexpr int kMaxBodies = 64, kMaxHinges = 64;

// one wavefront, lane = body.  q[7 + nh] with a unit base quaternion; tree[(2 + IK_MAX_HOPS) * nb] = depth, hinge, hop rounds
// (source lanes); local[10 * nb] = parent-relative quaternion, position, hinge axis.  xa[7 * nb]: the full walk; rot[4 * nb]:
// the rotation walk.
__global__ void k_walks(int nb, int nh, int nhop, const double* q, const int* tree, const double* local, double* xa, double* rot) {
  __shared__ double sm[7 + kMaxHinges + 2 * kMaxHinges + 7 * kMaxBodies + 3 * kMaxBodies];
  WalkLay L;
  L.nb = nb; L.nhop = nhop;
  L.o.q = 0; L.o.hsc = 7 + kMaxHinges; L.o.xa = L.o.hsc + 2 * kMaxHinges; L.o.xaxis = L.o.xa + 7 * kMaxBodies;
  const int lane = threadIdx.x;
  for (int i = lane; i < 7 + nh; i += 64) sm[L.o.q + i] = q[i];
  __syncthreads();
  if (lane < nh) {            // hinge_sincos of the kernel
    double s, c;
    sincos_small(0.5 * sm[L.o.q + 7 + lane], &s, &c);
    sm[L.o.hsc + 2 * lane] = s; sm[L.o.hsc + 2 * lane + 1] = c;
  }
  __syncthreads();
  FkLane F;
  const int b = lane < nb ? lane : 0;
  F.dep = lane < nb ? tree[b] : 0;
  F.hinge = lane < nb ? tree[nb + b] : -1;
  if (F.hinge >= nh) F.hinge = -1;
  for (int r = 0; r < IK_MAX_HOPS; r++) F.src[r] = r < nhop ? 4 * min(max(tree[(2 + r) * nb + b], 0), nb - 1) : 0;
  const double* lo = local + 10 * b;
  F.bq = d4{lo[0], lo[1], lo[2], lo[3]};
  F.bp = d3{lo[4], lo[5], lo[6]};
  F.ax = d3{lo[7], lo[8], lo[9]};
  Prof pr;
  fk_wave<4, false>(L, sm, F, lane, pr);
  const d4 qr = qwalk_wave(L, sm, F, fresh_lane(lane));
  __syncthreads();
  if (lane < nb) {
    for (int r = 0; r < 7; r++) xa[7 * lane + r] = sm[L.o.xa + 7 * lane + r];
    rot[4 * lane] = qr.w; rot[4 * lane + 1] = qr.x; rot[4 * lane + 2] = qr.y; rot[4 * lane + 3] = qr.z;
  }
}

}  // namespace

extern "C" int gmr_probe_split_eval(int n, const double* pose, double* ref, double* split) {
  if (n <= 0 || n > kMaxN) return -1;
  Buf<double> P, R, S;
  PROBE_RC(P.in(pose, 14 * (size_t)n)); PROBE_RC(R.out(11 * (size_t)n)); PROBE_RC(S.out(11 * (size_t)n));
  k_log<false><<<(n + kBlock - 1) / kBlock, kBlock>>>(n, P.d, R.d);
  PROBE_TRY(hipGetLastError());
  k_log<true><<<(n + kBlock - 1) / kBlock, kBlock>>>(n, P.d, S.d);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_RC(R.back(ref));
  return S.back(split);
}

extern "C" int gmr_probe_max_hops(void) { return IK_MAX_HOPS; }

extern "C" int gmr_probe_walks(int nb, int nh, int nhop, const double* q, const int* tree, const double* local, double* xa, double* rot) {
  if (nb <= 0 || nb > kMaxBodies || nh < 0 || nh > kMaxHinges || nhop < 0 || nhop > IK_MAX_HOPS) return -1;
  Buf<double> Q, Lc, X, R;
  Buf<int> Tr;
  PROBE_RC(Q.in(q, 7 + (size_t)nh)); PROBE_RC(Tr.in(tree, (2 + (size_t)IK_MAX_HOPS) * nb)); PROBE_RC(Lc.in(local, 10 * (size_t)nb));
  PROBE_RC(X.out(7 * (size_t)nb)); PROBE_RC(R.out(4 * (size_t)nb));
  k_walks<<<1, 64>>>(nb, nh, nhop, Q.d, Tr.d, Lc.d, X.d, R.d);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_RC(X.back(xa));
  return R.back(rot);
}
