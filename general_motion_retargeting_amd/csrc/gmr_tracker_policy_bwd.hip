// gmr_tracker_policy_bwd.hip -- the backward pass through the two networks of a training iteration on the motion tracker (DESIGN.md
// section 6za): what loss.backward() (runner.py:163) computes behind the gradients at the networks' outputs, for the ELU MLPs of
// booster_gym/utils/model.py:9-27.  The statement of record is tests/policy_bwd_mirror.py.  Three launches per network per call:
//
//   tracker_policy_sweep_kernel     ONE workgroup of four wavefronts per GMR_POLICY_TILE = 32 rows: the forward kernel run backwards.  g_l
//                                   stays in LDS in two buffers that alternate.  The first step, from g_L (at most 32 columns, the
//                                   critic's one), runs on the vector ALU, an output element per lane.  A hidden step dA = g_l W_l runs on
//                                   v_mfma_f32_32x32x2_f32: g_l is the A operand from LDS, W_l the B operand straight from global memory --
//                                   B[k = j][n = i] = W[j][i], so consecutive lanes read consecutive addresses.  The epilogue multiplies by
//                                   ELU's derivative taken from hidden[l - 1] and writes g_{l-1} to LDS and to delta[l - 1].
//   tracker_policy_dw_kernel        ONE wavefront per (layer, 64 x 64 block of dW, row chunk) through the tile table: a 2 x 2 block of
//                                   accumulator tiles, both operands read down the rows of row-major arrays (the lanes of either half of
//                                   the wavefront take 32 consecutive columns of one row), so each operand register feeds two matrix
//                                   instructions and the chain over a chunk's rows runs in rising row order.  db comes from the same
//                                   pass in the blocks at i0 = 0: the same A operand against a column of ones.  Edges (5, 47, 80 inputs,
//                                   1 or A outputs) are zeros in registers.  The partial sums of every chunk go to the workspace.
//   tracker_policy_fold_kernel      per output element the chunks' partial sums in double, in rising chunk order, rounded once into grads.
//
// The parameters and the gradients are the caller's and travel by address in the kernel arguments; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_tracker_host.h"
#include "gmr_tracker_policy_bwd_plan.h"
#include "gmr_workspace.h"

// one rounding per operation on the elementwise lines, as in gmr_tracker_policy.hip
#pragma clang fp contract(off)

namespace gmr {

constexpr int BT = GMR_POLICY_TILE;
constexpr int BMAXL = GMR_POLICY_MAX_HIDDEN;
constexpr int BTHREADS = 256;
constexpr int BWAVES = BTHREADS / 64;
constexpr int BKB = 8;                      // k per operand load of the sweep: four consecutive ones in either half of the wavefront
constexpr int BCH = GMR_POLICY_BWD_CHUNK;
constexpr int BTENSORS = 2 * (BMAXL + 1);
static_assert(BT == 32 && PBW_TILE == 64, "the tiles are those of v_mfma_f32_32x32x2_f32");

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define GMR_F32X16_ZERO {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}

// ---- the sweep --------------------------------------------------------------------------------------------------------------------------
struct SweepArgs {
  const float* W[BMAXL + 1];                // [width[l + 1]][width[l]]; W[0] is not read
  const float* hid[BMAXL];                  // [rows][width[l + 1]]
  float* delta[BMAXL];                      // [rows][width[l + 1]]
  const float* gL;                          // [rows][width[L + 1]]
  int32_t width[BMAXL + 2];
  int32_t L;
  int32_t stride[2];                        // floats per row of the two LDS buffers: g_l lives in buffer l & 1
  int64_t rows;
};

// ELU's derivative from its output
__device__ __forceinline__ float elu_slope(float y) { return y > 0.0f ? 1.0f : y + 1.0f; }

// One hidden step of a tile: g_{l-1}[row][i] = (sum_j src[row][j] W[j][i]) * d(hid[row][i]) for the 32 rows and the K columns of layer l's
// input; N the width of g_l.  keep: g_{l-1} is read again by the next step.
__device__ __forceinline__ void sweep_layer(const float* __restrict__ W, const float* src, int ss, float* dst, int ds, int N, int K, const float* __restrict__ hid,
                                            float* __restrict__ delta, int64_t row0, int nrow, bool keep) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const float* arow = src + r * ss + 4 * h;
  for (int c0 = wave * 32; c0 < K; c0 += BWAVES * 32) {               // (uniform over the wavefront)
    const float* wcol = W + (size_t)(4 * h) * K + c0 + r;
    f32x16 acc = GMR_F32X16_ZERO;
    float4 a = *reinterpret_cast<const float4*>(arow);
    float w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = wcol[(size_t)j * K];
    for (int kb = 0; kb < N; kb += BKB) {
      float4 an = a;
      float wn[4] = {w[0], w[1], w[2], w[3]};
      if (kb + BKB < N) {
        an = *reinterpret_cast<const float4*>(arow + kb + BKB);
#pragma unroll
        for (int j = 0; j < 4; j++) wn[j] = wcol[(size_t)(kb + BKB + j) * K];
      }
      // A[row r][k = h], B[k = h][column r]: step j sums k = kb + j, then k = kb + 4 + j
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w[3], acc, 0, 0, 0);
      a = an;
#pragma unroll
      for (int j = 0; j < 4; j++) w[j] = wn[j];
    }
#pragma unroll
    for (int g = 0; g < 16; g++) {                                    // the accumulator: column r, row (g & 3) + 8 (g >> 2) + 4 h
      const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
      const bool live = row < nrow;
      const float y = live ? hid[(row0 + row) * K + c0 + r] : 0.0f;
      const float v = acc[g] * elu_slope(y);
      if (keep) dst[row * ds + c0 + r] = v;
      if (live) delta[(row0 + row) * K + c0 + r] = v;
    }
  }
}

__global__ __launch_bounds__(BTHREADS) void tracker_policy_sweep_kernel(const SweepArgs X) {
  extern __shared__ __align__(16) float s_g[];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * BT;
  const int nrow = (int)(X.rows - row0 < BT ? X.rows - row0 : BT);
  float* buf[2] = {s_g, s_g + BT * X.stride[0]};
  const int L = X.L, A = X.width[L + 1];
  // g_L of the tile, zeros beyond the last row
  {
    float* dst = buf[L & 1];
    const int ds = X.stride[L & 1];
    for (int o = tid; o < BT * A; o += BTHREADS) {
      const int m = o / A, j = o - m * A;
      dst[m * ds + j] = m < nrow ? X.gL[(row0 + m) * A + j] : 0.0f;
    }
  }
  __syncthreads();
  // the first step on the vector ALU: an output element per lane, the j in rising order
  {
    const int K = X.width[L];
    const float* __restrict__ W = X.W[L];
    const float* src = buf[L & 1];
    const int ss = X.stride[L & 1];
    float* dst = buf[(L - 1) & 1];
    const int ds = X.stride[(L - 1) & 1];
    const float* __restrict__ hid = X.hid[L - 1];
    float* __restrict__ delta = X.delta[L - 1];
    const bool keep = L > 1;
    for (int o = tid; o < BT * K; o += BTHREADS) {
      const int m = o / K, i = o - m * K;
      float acc = 0.0f;
      for (int j = 0; j < A; j++) acc = fmaf(src[m * ss + j], W[(size_t)j * K + i], acc);
      const bool live = m < nrow;
      const float y = live ? hid[(row0 + m) * K + i] : 0.0f;
      const float v = acc * elu_slope(y);
      if (keep) dst[m * ds + i] = v;
      if (live) delta[(row0 + m) * K + i] = v;
    }
  }
  __syncthreads();
  for (int l = L - 1; l >= 1; l--) {
    const int s = l & 1;
    sweep_layer(X.W[l], buf[s], X.stride[s], buf[s ^ 1], X.stride[s ^ 1], X.width[l + 1], X.width[l], X.hid[l - 1], X.delta[l - 1], row0, nrow, l > 1);
    __syncthreads();
  }
}

// ---- the weight gradients ---------------------------------------------------------------------------------------------------------------
struct DwLayer {
  const float* g;                           // g_l [rows][N]
  const float *a0, *a1;                     // a_l [rows][c0] and, side by side, [rows][c1] (the critic's first layer; else c1 = 0)
  int32_t N, K, c0, c1;
  int64_t offW, offb;                       // in a chunk's record, floats
};
struct DwArgs {
  DwLayer lay[BMAXL + 1];
  const PolicyBwdTile* tab;
  int32_t tiles;
  int64_t items;                            // tiles * the chunks of rows
  int64_t rows, elems;
  float* part;                              // [chunks][elems]
};

// One step of the chain: rows m and m + 1 of the chunk in the two halves of the wavefront.  CLAMP: the last step of an odd chunk, whose
// upper half has no row -- it reads the row below and contributes zeros.
template <bool CLAMP>
__device__ __forceinline__ void dw_step(int64_t m, int64_t m_end, const float* g0, const float* g1, int N, bool okj0, bool okj1, const float* b0, int sb0,
                                        const float* b1, int sb1, bool oki0, bool oki1, float (&v)[4]) {
  bool live = true;
  if (CLAMP) {
    live = m < m_end;
    m = live ? m : m_end - 1;
  }
  const float ga0 = g0[m * N], ga1 = g1[m * N], ba0 = b0[m * sb0], ba1 = b1[m * sb1];
  v[0] = okj0 && live ? ga0 : 0.0f;
  v[1] = okj1 && live ? ga1 : 0.0f;
  v[2] = oki0 && live ? ba0 : 0.0f;
  v[3] = oki1 && live ? ba1 : 0.0f;
}

__global__ __launch_bounds__(BTHREADS) void tracker_policy_dw_kernel(const DwArgs X) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (the item and its tile stay in scalar registers)
  const int r = lane & 31, h = lane >> 5;
  const int64_t item = (int64_t)blockIdx.x * BWAVES + wave;
  if (item >= X.items) return;                                        // (uniform over the wavefront; the kernel has no barrier)
  const int64_t chunk = item / X.tiles;
  const PolicyBwdTile T = X.tab[item - chunk * X.tiles];
  const DwLayer Y = X.lay[T.layer];
  const int N = Y.N, K = Y.K;
  const int64_t m_begin = chunk * BCH, m_end = X.rows < m_begin + BCH ? X.rows : m_begin + BCH;
  // the lane's two columns of g and of a; a column beyond the width reads column 0 of a live row and counts as zero
  const int j0 = T.j0 + r, j1 = j0 + 32, i0 = T.i0 + r, i1 = i0 + 32;
  const bool okj0 = j0 < N, okj1 = j1 < N, oki0 = i0 < K, oki1 = i1 < K;
  const float* g0 = Y.g + (okj0 ? j0 : 0);
  const float* g1 = Y.g + (okj1 ? j1 : 0);
  const int ci0 = oki0 ? i0 : 0, ci1 = oki1 ? i1 : 0;
  const float* b0 = ci0 < Y.c0 ? Y.a0 + ci0 : Y.a1 + (ci0 - Y.c0);
  const float* b1 = ci1 < Y.c0 ? Y.a0 + ci1 : Y.a1 + (ci1 - Y.c0);
  const int sb0 = ci0 < Y.c0 ? Y.c0 : Y.c1, sb1 = ci1 < Y.c0 ? Y.c0 : Y.c1;
  const bool tj1 = T.j0 + 32 < N, ti1 = T.i0 + 32 < K, bias = T.bias != 0;      // (uniform)
  f32x16 acc00 = GMR_F32X16_ZERO, acc01 = GMR_F32X16_ZERO, acc10 = GMR_F32X16_ZERO, acc11 = GMR_F32X16_ZERO, accb0 = GMR_F32X16_ZERO, accb1 = GMR_F32X16_ZERO;
  const int64_t n = m_end - m_begin, full = n / 2;
  // A[row j][k = h] = g[m + h][j], B[k = h][column i] = a[m + h][i]: an instruction sums row m, then row m + 1
#define GMR_DW_MFMA(v)                                                                          \
  acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(v[0], v[2], acc00, 0, 0, 0);                     \
  if (ti1) acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(v[0], v[3], acc01, 0, 0, 0);            \
  if (tj1) acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(v[1], v[2], acc10, 0, 0, 0);            \
  if (tj1 && ti1) acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(v[1], v[3], acc11, 0, 0, 0);     \
  if (bias) {                                                                                   \
    accb0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v[0], 1.0f, accb0, 0, 0, 0);                   \
    if (tj1) accb1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v[1], 1.0f, accb1, 0, 0, 0);          \
  }
  int64_t s = 0;
  for (; s + 2 <= full; s += 2) {                                     // two steps' operands on their way before the first one's instructions
    float va[4], vb[4];
    dw_step<false>(m_begin + 2 * s + h, m_end, g0, g1, N, okj0, okj1, b0, sb0, b1, sb1, oki0, oki1, va);
    dw_step<false>(m_begin + 2 * s + 2 + h, m_end, g0, g1, N, okj0, okj1, b0, sb0, b1, sb1, oki0, oki1, vb);
    GMR_DW_MFMA(va)
    GMR_DW_MFMA(vb)
  }
  for (; s < full; s++) {
    float v[4];
    dw_step<false>(m_begin + 2 * s + h, m_end, g0, g1, N, okj0, okj1, b0, sb0, b1, sb1, oki0, oki1, v);
    GMR_DW_MFMA(v)
  }
  if (n & 1) {
    float v[4];
    dw_step<true>(m_begin + 2 * full + h, m_end, g0, g1, N, okj0, okj1, b0, sb0, b1, sb1, oki0, oki1, v);
    GMR_DW_MFMA(v)
  }
#undef GMR_DW_MFMA
  float* rec = X.part + chunk * X.elems;
#pragma unroll
  for (int g = 0; g < 16; g++) {                                      // an accumulator: column r, row (g & 3) + 8 (g >> 2) + 4 h
    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
    const int ja = T.j0 + row, jb = ja + 32;
    if (ja < N) {
      if (oki0) rec[Y.offW + (int64_t)ja * K + i0] = acc00[g];
      if (oki1) rec[Y.offW + (int64_t)ja * K + i1] = acc01[g];
      if (bias && r == 0) rec[Y.offb + ja] = accb0[g];
    }
    if (jb < N) {
      if (oki0) rec[Y.offW + (int64_t)jb * K + i0] = acc10[g];
      if (oki1) rec[Y.offW + (int64_t)jb * K + i1] = acc11[g];
      if (bias && r == 0) rec[Y.offb + jb] = accb1[g];
    }
  }
}

// ---- the fold ---------------------------------------------------------------------------------------------------------------------------
struct FoldArgs {
  float* grad[BTENSORS];                    // W_0, b_0, W_1, b_1, ..
  int64_t off[BTENSORS];                    // where each starts in a chunk's record
  int32_t tensors, chunks;
  int64_t elems;
  const float* part;
};

__global__ __launch_bounds__(BTHREADS) void tracker_policy_fold_kernel(const FoldArgs X) {
  const int64_t e = (int64_t)blockIdx.x * BTHREADS + threadIdx.x;
  if (e >= X.elems) return;
  const float* p = X.part + e;
  double s = 0.0;
#pragma unroll 4
  for (int c = 0; c < X.chunks; c++) s = s + (double)p[(int64_t)c * X.elems];
  float* gp = X.grad[0];
  int64_t base = 0;
#pragma unroll
  for (int k = 1; k < BTENSORS; k++)
    if (k < X.tensors && e >= X.off[k]) {
      gp = X.grad[k];
      base = X.off[k];
    }
  gp[e - base] = (float)s;
}

// the LDS of the sweep of the widest network
constexpr size_t BMAXLDS = (size_t)BT * 2 * (GMR_POLICY_MAX_WIDTH + 4) * sizeof(float);

static bool same_shape(const PolicyShape& a, const PolicyShape& b) {
  if (a.L != b.L || a.first != b.first) return false;
  for (int l = 0; l <= a.L + 1; l++)
    if (a.width[l] != b.width[l]) return false;
  return true;
}

// The checks of a call and its three launches on the network S of P (critic: P.critic, else P.actor).
static int backward_launch(const PolicyTables& P, const PolicyBwdTables& B, bool critic, const float* const* params, float* const* grads, int64_t rows,
                           const float* obs, const float* priv, const float* const* hidden, const float* gL, float* const* delta, hipStream_t stream) {
  if (!P.on) return gmr_fail(GMR_ERR_ARG, "the policy is not set on this tracker (gmr_motion_tracker_set_policy)");
  if (!B.on) return gmr_fail(GMR_ERR_ARG, "the backward pass is not set on this tracker (gmr_motion_tracker_set_backward)");
  if (!same_shape(P.actor, B.actor) || !same_shape(P.critic, B.critic) || P.obs_cols != B.obs_cols || P.priv_cols != B.priv_cols)
    return gmr_fail(GMR_ERR_ARG, "the policy was set again after the backward pass (gmr_motion_tracker_set_backward again)");
  const PolicyShape& S = critic ? P.critic : P.actor;
  const PolicyBwdNet& Nn = critic ? B.plan.critic : B.plan.actor;
  if (!params || !grads || !obs || !hidden || !gL || !delta) return gmr_fail(GMR_ERR_ARG, "null params / grads / obs / hidden / output gradient / delta");
  if (rows < 1 || rows > B.plan.max_rows) return gmr_fail(GMR_ERR_ARG, "rows = %lld, 1 .. max_rows = %lld are taken", (long long)rows, (long long)B.plan.max_rows);
  if (critic && P.priv_cols > 0 && !priv) return gmr_fail(GMR_ERR_ARG, "priv is needed: priv_cols = %d", P.priv_cols);
  for (int k = S.first; k < S.first + 2 * (S.L + 1); k++) {
    if (!params[k] || !grads[k]) return gmr_fail(GMR_ERR_ARG, "%s[%d] is NULL", params[k] ? "grads" : "params", k);
    if (((uintptr_t)params[k] | (uintptr_t)grads[k]) & 3u) return gmr_fail(GMR_ERR_ARG, "%s[%d] is not on 4 bytes", ((uintptr_t)params[k] & 3u) ? "params" : "grads", k);
  }
  for (int l = 0; l < S.L; l++) {
    if (!hidden[l] || !delta[l]) return gmr_fail(GMR_ERR_ARG, "%s[%d] is NULL: the backward pass needs every layer", hidden[l] ? "delta" : "hidden", l);
    if (((uintptr_t)hidden[l] | (uintptr_t)delta[l]) & 3u) return gmr_fail(GMR_ERR_ARG, "%s[%d] is not on 4 bytes", ((uintptr_t)hidden[l] & 3u) ? "hidden" : "delta", l);
  }
  const int L = S.L;
  SweepArgs X = {};
  X.L = L;
  for (int l = 0; l <= L + 1; l++) X.width[l] = S.width[l];
  for (int l = 0; l <= L; l++) X.W[l] = params[S.first + 2 * l];
  for (int l = 0; l < L; l++) {
    X.hid[l] = hidden[l];
    X.delta[l] = delta[l];
  }
  X.gL = gL;
  X.stride[0] = Nn.stride[0]; X.stride[1] = Nn.stride[1];
  X.rows = rows;
  hipLaunchKernelGGL(tracker_policy_sweep_kernel, dim3((unsigned)((rows + BT - 1) / BT)), dim3(BTHREADS), Nn.lds, stream, X);
  GMR_HIP_TRY(hipGetLastError());
  const int64_t chunks = policy_bwd_chunks(rows);
  DwArgs Y = {};
  for (int l = 0; l <= L; l++) {
    DwLayer& y = Y.lay[l];
    y.g = l == L ? gL : delta[l];
    y.N = S.width[l + 1]; y.K = S.width[l];
    if (l == 0) {
      y.a0 = obs; y.c0 = P.obs_cols;
      y.a1 = critic ? priv : nullptr; y.c1 = critic ? P.priv_cols : 0;
    } else {
      y.a0 = hidden[l - 1]; y.c0 = S.width[l];
    }
    y.offW = Nn.off[2 * l]; y.offb = Nn.off[2 * l + 1];
  }
  Y.tab = critic ? B.tab_critic : B.tab_actor;
  Y.tiles = Nn.tiles;
  Y.items = chunks * Nn.tiles;
  Y.rows = rows; Y.elems = Nn.elems;
  Y.part = B.part;
  hipLaunchKernelGGL(tracker_policy_dw_kernel, dim3((unsigned)((Y.items + BWAVES - 1) / BWAVES)), dim3(BTHREADS), 0, stream, Y);
  GMR_HIP_TRY(hipGetLastError());
  FoldArgs Z = {};
  Z.tensors = 2 * (L + 1);
  for (int k = 0; k < Z.tensors; k++) {
    Z.grad[k] = grads[S.first + k];
    Z.off[k] = Nn.off[k];
  }
  Z.chunks = (int32_t)chunks;
  Z.elems = Nn.elems;
  Z.part = B.part;
  hipLaunchKernelGGL(tracker_policy_fold_kernel, dim3(lane_blocks(Nn.elems)), dim3(BTHREADS), 0, stream, Z);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

// The synchronous twin of either call: the network's parameters, the inputs and the outputs through one staging block.
static int backward_host(gmr_motion_tracker* t, bool critic, const float* const* params, float* const* grads, int64_t rows, const float* obs, const float* priv,
                         const float* const* hidden, const float* gL, float* const* delta) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const PolicyTables P = t->policy;
  const PolicyBwdTables B = t->bwd;
  if (!P.on) return gmr_fail(GMR_ERR_ARG, "the policy is not set on this tracker (gmr_motion_tracker_set_policy)");
  if (!B.on) return gmr_fail(GMR_ERR_ARG, "the backward pass is not set on this tracker (gmr_motion_tracker_set_backward)");
  const PolicyShape& S = critic ? P.critic : P.actor;
  if (!params || !grads || !obs || !hidden || !gL || !delta) return gmr_fail(GMR_ERR_ARG, "null params / grads / obs / hidden / output gradient / delta");
  if (rows < 1 || rows > B.plan.max_rows) return gmr_fail(GMR_ERR_ARG, "rows = %lld, 1 .. max_rows = %lld are taken", (long long)rows, (long long)B.plan.max_rows);
  if (critic && P.priv_cols > 0 && !priv) return gmr_fail(GMR_ERR_ARG, "priv is needed: priv_cols = %d", P.priv_cols);
  const size_t M = (size_t)rows;
  HostStage st;
  const float* dp[GMR_POLICY_MAX_TENSORS] = {};
  float* dg[GMR_POLICY_MAX_TENSORS] = {};
  const float* dh[BMAXL] = {};
  float* dd[BMAXL] = {};
  const float *d_obs, *d_priv = nullptr, *d_g;
  for (int l = 0; l <= S.L; l++) {
    const int kw = S.first + 2 * l;
    for (int k = kw; k < kw + 2; k++)
      if (!params[k] || !grads[k]) return gmr_fail(GMR_ERR_ARG, "%s[%d] is NULL", params[k] ? "grads" : "params", k);
    const size_t nw = (size_t)S.width[l] * S.width[l + 1] * 4, nb = (size_t)S.width[l + 1] * 4;
    st.in(dp[kw], params[kw], nw);
    st.in(dp[kw + 1], params[kw + 1], nb);
    st.out(dg[kw], grads[kw], nw);
    st.out(dg[kw + 1], grads[kw + 1], nb);
    if (l < S.L) {
      if (!hidden[l] || !delta[l]) return gmr_fail(GMR_ERR_ARG, "%s[%d] is NULL: the backward pass needs every layer", hidden[l] ? "delta" : "hidden", l);
      st.in(dh[l], hidden[l], M * S.width[l + 1] * 4);
      st.out(dd[l], delta[l], M * S.width[l + 1] * 4);
    }
  }
  st.in(d_obs, obs, M * P.obs_cols * 4);
  if (critic) st.in(d_priv, priv, M * P.priv_cols * 4);
  st.in(d_g, gL, M * S.width[S.L + 1] * 4);
  GMR_STAGE_TRY(st, upload);
  const int rc = backward_launch(P, B, critic, dp, dg, rows, d_obs, d_priv, dh, d_g, dd, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

static int backward_dev(gmr_motion_tracker* t, bool critic, const float* const* params, float* const* grads, int64_t rows, const float* obs, const float* priv,
                        const float* const* hidden, const float* gL, float* const* delta, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  PolicyTables P;
  PolicyBwdTables B;
  {
    std::lock_guard<std::mutex> g(t->mu);
    P = t->policy;
    B = t->bwd;
  }
  return backward_launch(P, B, critic, params, grads, rows, obs, priv, hidden, gL, delta, (hipStream_t)stream);
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker policy backward") -------------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_backward(gmr_motion_tracker_t* t, int64_t max_rows) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::PolicyTables P = t->policy;
  if (!P.on) return gmr_fail(GMR_ERR_ARG, "the policy is not set on this tracker (gmr_motion_tracker_set_policy)");
  gmr::PolicyBwdTables B;
  int rc = gmr::policy_bwd_plan(P.actor, P.critic, max_rows, &B.plan);
  if (rc != GMR_OK) return rc;
  // the widest networks ask for more LDS than a kernel gets unasked
  GMR_HIP_TRY(hipFuncSetAttribute((const void*)gmr::tracker_policy_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gmr::BMAXLDS));
  gmr::Carve cv;
  const size_t o_part = cv.take(B.plan.o_tab_actor - B.plan.o_part);
  const size_t o_ta = cv.take(B.plan.o_tab_critic - B.plan.o_tab_actor);
  const size_t o_tc = cv.take(B.plan.bytes - B.plan.o_tab_critic);
  if (o_part != B.plan.o_part || o_ta != B.plan.o_tab_actor || o_tc != B.plan.o_tab_critic || cv.total() != B.plan.bytes)
    return gmr_fail(GMR_ERR_ARG, "the plan of the backward block and its carving disagree");
  rc = gmr::fresh_block(t->bwd_block, cv);
  if (rc != GMR_OK) return rc;
  std::vector<gmr::PolicyBwdTile> ta(gmr::PBW_MAX_TILES), tc(gmr::PBW_MAX_TILES);
  gmr::PolicyBwdNet na, nc;
  gmr::policy_bwd_net(P.actor, &na, ta.data());
  gmr::policy_bwd_net(P.critic, &nc, tc.data());
  char* base = t->bwd_block.data();
  GMR_HIP_TRY(hipMemcpy(base + o_ta, ta.data(), (size_t)na.tiles * sizeof(gmr::PolicyBwdTile), hipMemcpyHostToDevice));
  GMR_HIP_TRY(hipMemcpy(base + o_tc, tc.data(), (size_t)nc.tiles * sizeof(gmr::PolicyBwdTile), hipMemcpyHostToDevice));
  GMR_HIP_TRY(hipDeviceSynchronize());
  B.on = 1;
  B.actor = P.actor; B.critic = P.critic;
  B.obs_cols = P.obs_cols; B.priv_cols = P.priv_cols;
  B.part = (float*)(base + o_part);
  B.tab_actor = (const gmr::PolicyBwdTile*)(base + o_ta);
  B.tab_critic = (const gmr::PolicyBwdTile*)(base + o_tc);
  t->bwd = B;
  return GMR_OK;
}

int gmr_motion_tracker_act_backward_dev(gmr_motion_tracker_t* t, const float* const* d_params, float* const* d_grads, int64_t rows, const float* d_obs,
                                        const float* const* d_hidden, const float* d_grad_loc, float* const* d_delta, void* stream) {
  return gmr::backward_dev(t, false, d_params, d_grads, rows, d_obs, nullptr, d_hidden, d_grad_loc, d_delta, stream);
}

int gmr_motion_tracker_act_backward(gmr_motion_tracker_t* t, const float* const* params, float* const* grads, int64_t rows, const float* obs,
                                    const float* const* hidden, const float* grad_loc, float* const* delta) {
  return gmr::backward_host(t, false, params, grads, rows, obs, nullptr, hidden, grad_loc, delta);
}

int gmr_motion_tracker_values_backward_dev(gmr_motion_tracker_t* t, const float* const* d_params, float* const* d_grads, int64_t rows, const float* d_obs,
                                           const float* d_priv, const float* const* d_hidden, const float* d_grad_values, float* const* d_delta, void* stream) {
  return gmr::backward_dev(t, true, d_params, d_grads, rows, d_obs, d_priv, d_hidden, d_grad_values, d_delta, stream);
}

int gmr_motion_tracker_values_backward(gmr_motion_tracker_t* t, const float* const* params, float* const* grads, int64_t rows, const float* obs,
                                       const float* priv, const float* const* hidden, const float* grad_values, float* const* delta) {
  return gmr::backward_host(t, true, params, grads, rows, obs, priv, hidden, grad_values, delta);
}

int gmr_motion_tracker_backward_state(gmr_motion_tracker_t* t, int64_t* state) {
  if (!t || !state) return gmr_fail(GMR_ERR_ARG, "null motion tracker / state");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::PolicyBwdTables B = t->bwd;
  if (!B.on) return gmr_fail(GMR_ERR_ARG, "the backward pass is not set on this tracker (gmr_motion_tracker_set_backward)");
  state[0] = GMR_POLICY_BWD_CHUNK;
  state[1] = B.plan.chunks;
  state[2] = (int64_t)B.plan.bytes;
  state[3] = B.plan.max_rows;
  state[4] = B.plan.actor.tiles;
  state[5] = B.plan.critic.tiles;
  return GMR_OK;
}

}  // extern "C"
