// gmr_bvh.hip -- BVH clips on the device (row N2 of SURVEY.md section 8f): raw channel rows -> the packed human frames of
// gmr_job_t.human, written where the IK kernels read them.  Per frame exactly what utils/lafan1.py does on the host
// (read_bvh's numeric half, euler_to_quat, remove_quat_discontinuities, quat_fk, _global_poses; the reference's
// utils/lafan1.py:8-41 on top of lafan_vendor/extract.py:43-166 and lafan_vendor/utils.py:42-162, 251-268), in the host's
// operation order and without FP contraction: everything but sin / cos is the NumPy path's bits.
//
//   bvh_flip_scan_kernel  row b -> its clip (binary search of seg_start), the local quaternions of frame b and -- by a
//                         shuffle from the lane below -- of frame b - 1, one bit per joint: sign(<q[b-1], q[b]>) < 0.
//                         The de-flip state of a frame is the XOR of those bits from its clip's first frame on: a
//                         segmented inclusive XOR scan, in the wavefront by shuffles, over the block's four wavefronts
//                         through LDS.  Every wavefront owns 63 rows; its lane 0 recomputes the row below them.
//   bvh_carry_kernel      one thread per clip: the scan carried over the blocks the clip spans (block totals)
//   bvh_frames_kernel     64 rows per block, lane = frame: local quaternions again (cheaper than 576 B per frame through
//                         memory), de-flip, FK over the ancestor closure of the selected joints (parents first; a joint with
//                         a child that is not the next step parks its transform in an LDS slot), Y-up cm -> Z-up m, the
//                         frame's nsel x 7 doubles staged in LDS and flushed as contiguous runs at [clip][t] of the padded
//                         batch.  Rows at or beyond a clip's length are not written (the IK kernels never read them).
//
// Rows are dense (block i owns rows [64 i, 64 i + 64) of the concatenation, whatever clips they belong to), like gmr_post.hip;
// seg_start is clamped to [0, B] and a frame index to [0, min(len, T)), so no access leaves the buffers for any seg_start.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_internal.h"
#include "gmr_workspace.h"

// float64 arithmetic here mirrors NumPy's (one rounding per operation)
#pragma clang fp contract(off)

#include "gmr_bvh_prog.h"          // BvhProg, bvh_make_prog, the LDS size (host-only, checked by tests/cpp/ingest_prog_check.cpp)

#define BVH_SCAN_BLOCK 256
#define BVH_SCAN_ROWS 252       // four wavefronts x 63 rows (lane 0 of each is the row below its 63)

namespace gmr {

struct bq { double w, x, y, z; };
struct bv { double x, y, z; };

// _quat_mul(x, y) of utils/lafan1.py, term by term
__device__ __forceinline__ bq bvh_qmul(bq x, bq y) {
  bq r;
  r.w = y.w * x.w - y.x * x.x - y.y * x.y - y.z * x.z;
  r.x = y.w * x.x + y.x * x.w - y.y * x.z + y.z * x.y;
  r.y = y.w * x.y + y.x * x.z + y.y * x.w - y.z * x.x;
  r.z = y.w * x.z - y.x * x.y + y.y * x.x + y.z * x.w;
  return r;
}

__device__ __forceinline__ bv bvh_cross(bv a, bv b) {
  return bv{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// _quat_mul_vec(q, x): t = 2 (qv x x); x + q0 t + qv x t
__device__ __forceinline__ bv bvh_qrot(bq q, bv x) {
  const bv qv{q.x, q.y, q.z};
  const bv c = bvh_cross(qv, x);
  const bv t{2.0 * c.x, 2.0 * c.y, 2.0 * c.z};
  const bv u = bvh_cross(qv, t);
  return bv{(x.x + q.w * t.x) + u.x, (x.y + q.w * t.y) + u.y, (x.z + q.w * t.z) + u.z};
}

// _angle_axis_to_quat(np.radians(deg), axis): (cos(a / 2), sin(a / 2) * axis) with the unit vector's zeros multiplied in
__device__ __forceinline__ bq bvh_axis_quat(double deg, int ax) {
  const double a = deg * (M_PI / 180.0);
  double s, c;
  sincos(a / 2.0, &s, &c);
  const double z = s * 0.0;
  return bq{c, ax == 0 ? s : z, ax == 1 ? s : z, ax == 2 ? s : z};
}

// euler_to_quat: q0 (x) (q1 (x) q2)
__device__ __forceinline__ bq bvh_local_quat(const BvhProg& P, const double* __restrict__ row, int k) {
  const double* e = row + P.rcol[k];
  const bq q0 = bvh_axis_quat(e[0], P.ax[0]), q1 = bvh_axis_quat(e[1], P.ax[1]), q2 = bvh_axis_quat(e[2], P.ax[2]);
  return bvh_qmul(q0, bvh_qmul(q1, q2));
}

__device__ __forceinline__ int bvh_seg(const int32_t* __restrict__ seg_start, int i, int B) { return min(max(seg_start[i], 0), B); }

// the clip of row b: the LAST s with seg_start[s] <= b (an empty clip shares its start with the clip after it)
__device__ __forceinline__ int bvh_find_clip(const int32_t* __restrict__ seg_start, int nclip, int B, int b) {
  int lo = 0, hi = nclip - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bvh_seg(seg_start, mid, B) <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Flip bits and their segmented prefix XOR inside a block.  row_pref[b] = XOR of the flip masks of the rows from the later of
// (the clip's first row, the block's first row) to b; blk_tail[i] = that of the block's last row (the part of block i a clip
// carries into block i + 1).  The first nclip + 1 threads of the grid also leave seg_start clamped to [0, B].
__global__ __launch_bounds__(BVH_SCAN_BLOCK) void bvh_flip_scan_kernel(const BvhProg P, const double* __restrict__ rows,
                                                                       const int32_t* __restrict__ seg_start, int nclip, int B,
                                                                       int nblk, unsigned long long* __restrict__ row_pref,
                                                                       int32_t* __restrict__ row_clip,
                                                                       unsigned long long* __restrict__ blk_tail,
                                                                       int32_t* __restrict__ seg_clamped) {
  __shared__ unsigned long long w_v[BVH_SCAN_BLOCK / 64];
  __shared__ int w_f[BVH_SCAN_BLOCK / 64];
  const int gid = blockIdx.x * BVH_SCAN_BLOCK + threadIdx.x;
  if (gid <= nclip) seg_clamped[gid] = bvh_seg(seg_start, gid, B);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * BVH_SCAN_ROWS + w * 63 + lane - 1;      // lane 0: the row below this wavefront's 63
  const bool owns = lane >= 1 && b < B;
  const int br = min(max(b, 0), B - 1);
  const int s = bvh_find_clip(seg_start, nclip, B, br);
  const bool head = bvh_seg(seg_start, s, B) == br;
  const double* row = rows + (size_t)br * P.ncol;
  unsigned long long m = 0;
  for (int k = 0; k < P.n; k++) {
    const bq q = bvh_local_quat(P, row, k);
    const double pw = __shfl_up(q.w, 1), px = __shfl_up(q.x, 1), py = __shfl_up(q.y, 1), pz = __shfl_up(q.z, 1);
    const double d = ((pw * q.w + px * q.x) + py * q.y) + pz * q.z;   // np.sum over the four products, in order
    if (d < -d) m |= 1ull << k;                                       // strict: a tie keeps the sign
  }
  if (!owns || head) m = 0;                                           // a clip's first frame has no frame before it
  int f = owns && head;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long pv = __shfl_up(m, d);
    const int pf = __shfl_up(f, d);
    if (lane >= d) {
      if (!f) m ^= pv;
      f |= pf;
    }
  }
  if (lane == 63) { w_v[w] = m; w_f[w] = f; }
  __syncthreads();
  unsigned long long cv = 0;
  for (int i = 0; i < w; i++) cv = w_f[i] ? w_v[i] : (cv ^ w_v[i]);
  if (!f) m ^= cv;
  if (owns) { row_pref[b] = m; row_clip[b] = s; }
  if (threadIdx.x == BVH_SCAN_BLOCK - 1 && (int)blockIdx.x < nblk) blk_tail[blockIdx.x] = m;
}

// carry[i] = the de-flip state a clip brings into block i (used by the rows of block i that precede the block's first clip
// start).  A clip that spans blocks first .. last: the tail of `first`, then whole blocks.
__global__ __launch_bounds__(256) void bvh_carry_kernel(const int32_t* __restrict__ seg_clamped, int nclip, int nblk,
                                                        const unsigned long long* __restrict__ blk_tail,
                                                        unsigned long long* __restrict__ carry) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nclip) return;
  const int a = seg_clamped[c], e = seg_clamped[c + 1];
  if (e <= a) return;
  const int first = a / BVH_SCAN_ROWS, last = min((e - 1) / BVH_SCAN_ROWS, nblk - 1);
  unsigned long long acc = blk_tail[first];
  for (int i = first + 1; i <= last; i++) {
    carry[i] = acc;
    acc ^= blk_tail[i];
  }
}

__global__ __launch_bounds__(BVH_BLOCK) void bvh_frames_kernel(const BvhProg P, const double* __restrict__ rows,
                                                               const int32_t* __restrict__ seg_clamped,
                                                               const double* __restrict__ offsets, int nclip, int B, int T,
                                                               const unsigned long long* __restrict__ row_pref,
                                                               const int32_t* __restrict__ row_clip,
                                                               const unsigned long long* __restrict__ carry,
                                                               double* __restrict__ human) {
  extern __shared__ __align__(16) double bsm[];       // stage [64][nrow * 7], slots [nslot][7][64]
  const int W = P.nrow * 7;
  double* stage = bsm + (size_t)threadIdx.x * W;
  double* slots = bsm + (size_t)BVH_BLOCK * W + threadIdx.x;
  const int lane = threadIdx.x;
  const int b0 = blockIdx.x * BVH_BLOCK, b = b0 + lane;
  const int br = min(b, B - 1);
  const int s = min(max(row_clip[br], 0), nclip - 1);
  const int a = seg_clamped[s], len = min(seg_clamped[s + 1] - a, T);
  const int t = b - a;
  const bool ok = b < B && t >= 0 && t < len;
  unsigned long long m = row_pref[br];
  const int blk = br / BVH_SCAN_ROWS;
  if (a < blk * BVH_SCAN_ROWS) m ^= carry[blk];        // the clip began in an earlier block of the scan
  const double* row = rows + (size_t)br * P.ncol;
  const double* off = offsets + (size_t)s * P.J * 3;
  bq gr{1.0, 0.0, 0.0, 0.0};
  bv gp{0.0, 0.0, 0.0};
  for (int k = 0; k < P.n; k++) {
    bq q = bvh_local_quat(P, row, k);
    if ((m >> k) & 1) q = bq{-q.w, -q.x, -q.y, -q.z};  // rotations * sign
    const double* lp = P.pcol[k] >= 0 ? row + P.pcol[k] : off + 3 * P.joint[k];
    const bv lpos{lp[0], lp[1], lp[2]};
    const int ld = P.load[k];
    if (ld == -2) {
      gr = q;
      gp = lpos;
    } else {
      bq pr = gr;
      bv pp = gp;
      if (ld >= 0) {
        const double* sl = slots + (size_t)ld * 7 * BVH_BLOCK;
        pr = bq{sl[0], sl[BVH_BLOCK], sl[2 * BVH_BLOCK], sl[3 * BVH_BLOCK]};
        pp = bv{sl[4 * BVH_BLOCK], sl[5 * BVH_BLOCK], sl[6 * BVH_BLOCK]};
      }
      const bv r = bvh_qrot(pr, lpos);
      gp = bv{r.x + pp.x, r.y + pp.y, r.z + pp.z};
      gr = bvh_qmul(pr, q);
    }
    if (P.save[k] >= 0) {
      double* sl = slots + (size_t)P.save[k] * 7 * BVH_BLOCK;
      sl[0] = gr.w; sl[BVH_BLOCK] = gr.x; sl[2 * BVH_BLOCK] = gr.y; sl[3 * BVH_BLOCK] = gr.z;
      sl[4 * BVH_BLOCK] = gp.x; sl[5 * BVH_BLOCK] = gp.y; sl[6 * BVH_BLOCK] = gp.z;
    }
    const int e0 = P.ent0[k], e1 = P.ent0[k + 1];
    if (e0 < e1) {
      // Y-up centimetres -> Z-up metres: _ROT_QUAT (x) gr, and gp @ _ROT.T / 100 with the matrix's zeros multiplied in
      const bq o = bvh_qmul(bq{M_SQRT1_2, M_SQRT1_2, 0.0, 0.0}, gr);
      const double x = ((gp.x * 1.0 + gp.y * 0.0) + gp.z * 0.0) / 100.0;
      const double y = ((gp.x * 0.0 + gp.y * 0.0) + gp.z * -1.0) / 100.0;
      const double z = ((gp.x * 0.0 + gp.y * 1.0) + gp.z * 0.0) / 100.0;
      for (int e = e0; e < e1; e++) {
        double* dst = stage + (P.ent[e] >> 1) * 7;
        if (P.ent[e] & 1) { dst[3] = o.w; dst[4] = o.x; dst[5] = o.y; dst[6] = o.z; }
        else { dst[0] = x; dst[1] = y; dst[2] = z; }
      }
    }
  }
  __syncthreads();
  // flush: frame by frame, a frame's W doubles contiguous; consecutive frames of one clip continue the same run
  const long long mine = ok ? ((long long)s * T + t) * W : -1;
  const int nrow = min(B - b0, BVH_BLOCK);
  for (int f = 0; f < nrow; f++) {
    const long long d = __shfl(mine, f);
    if (d < 0) continue;
    const double* src = bsm + (size_t)f * W;
    for (int c = lane; c < W; c += BVH_BLOCK) human[d + c] = src[c];
  }
}

}  // namespace gmr

// ---- the handle and the C-ABI --------------------------------------------------------------------------------------------
struct gmr_bvh {
  gmr::BvhProg prog;
  size_t lds_bytes = 0;
  gmr::StreamWorkspace ws;       // gmr_bvh_frames_dev
  // gmr_bvh_frames: device staging of the host buffers, grown on demand and kept
  std::mutex host_mu;
  gmr::DeviceBlock host_ws;
};

extern "C" {

int gmr_bvh_create(int J, const int32_t* parents, int channels, const char* order, int nsel, const int32_t* sel_pos,
                   const int32_t* sel_rot, gmr_bvh_t** out) {
  if (!out || !parents || J < 1 || J > BVH_MAX_JOINTS) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: 1 <= J <= %d", BVH_MAX_JOINTS);
  if (channels != 3 && channels != 6) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: channels = %d (3 or 6)", channels);
  int ax[3];
  bool seen[3] = {false, false, false};
  if (!order || strlen(order) != 3) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: the Euler order is three letters, a permutation of xyz");
  for (int i = 0; i < 3; i++) {
    const char c = order[i];
    if (c < 'x' || c > 'z' || seen[c - 'x']) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: Euler order \"%s\" is not a permutation of xyz", order);
    seen[c - 'x'] = true;
    ax[i] = c - 'x';
  }
  if (parents[0] >= 0) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: joint 0 is the root (parent -1)");
  for (int j = 1; j < J; j++)
    if (parents[j] < 0 || parents[j] >= j) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: parents must precede children, joint 0 is the only root (joint %d)", j);
  if (nsel < 1 || nsel > BVH_MAX_ROWS || !sel_pos || !sel_rot) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: 1 <= nsel <= %d", BVH_MAX_ROWS);
  for (int r = 0; r < nsel; r++)
    if (sel_pos[r] < 0 || sel_pos[r] >= J || sel_rot[r] < 0 || sel_rot[r] >= J)
      return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: row %d selects joint %d / %d of %d", r, sel_pos[r], sel_rot[r], J);
  gmr_bvh* h = new (std::nothrow) gmr_bvh;
  if (!h) return gmr_fail(GMR_ERR_ARG, "out of memory");
  gmr::BvhProg& P = h->prog;
  const gmr::BvhProgStatus ps = gmr::bvh_make_prog(J, parents, channels, ax, nsel, sel_pos, sel_rot, &P, &h->lds_bytes);
  if (ps == gmr::BVH_PROG_STEPS) { delete h; return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: the selection needs more than %d joints", BVH_MAX_STEPS); }
  if (ps == gmr::BVH_PROG_LDS) {
    const int nslot = P.nslot;
    delete h;
    return gmr_fail(GMR_ERR_ARG, "gmr_bvh_create: %d rows and %d parked joints do not fit the LDS", nsel, nslot);
  }
  if (h->lds_bytes > gmr::BVH_LDS_DEFAULT) {
    hipError_t e = hipFuncSetAttribute((const void*)gmr::bvh_frames_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes);
    if (e != hipSuccess) { delete h; return gmr_fail(GMR_ERR_HIP, "gmr_bvh_create: %s", hipGetErrorString(e)); }
  }
  *out = h;
  return GMR_OK;
}

int gmr_bvh_destroy(gmr_bvh_t* h) {
  delete h;                                // (freeing its blocks waits for the device: nothing of the handle is in flight afterwards)
  return GMR_OK;
}

int gmr_bvh_columns(const gmr_bvh_t* h) { return h ? h->prog.ncol : 0; }

int gmr_bvh_frames_dev(gmr_bvh_t* h, int nclip, int B, const double* d_rows, const int32_t* d_seg_start, const double* d_offsets,
                       int T, double* d_human, void* stream) {
  if (!h) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames_dev: null handle");
  if (nclip < 0 || B < 0 || T < 0) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames_dev: negative nclip / B / T");
  if (nclip == 0 || B == 0) return GMR_OK;
  if (T < 1) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames_dev: B = %d rows need T >= 1", B);
  if (!d_rows || !d_seg_start || !d_offsets || !d_human) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames_dev: null buffer");
  const int nblk = (B + BVH_SCAN_ROWS - 1) / BVH_SCAN_ROWS;
  // scratch: row_pref [B] u64, blk_tail [nblk] u64, carry [nblk] u64, row_clip [B] i32, seg_clamped [nclip + 1] i32
  gmr::Carve c;
  const size_t o_rp = c.take((size_t)B * 8), o_bt = c.take((size_t)nblk * 8), o_ca = c.take((size_t)nblk * 8), o_rc = c.take((size_t)B * 4),
               o_sc = c.take((size_t)(nclip + 1) * 4);
  hipStream_t st = (hipStream_t)stream;
  const auto ws = h->ws.acquire(st, c.total());                // (held until the last launch below is enqueued)
  GMR_NAMED_HIP_TRY("gmr_bvh_frames_dev", ws.error());
  char* d = ws.base();
  unsigned long long* row_pref = (unsigned long long*)(d + o_rp);
  unsigned long long* blk_tail = (unsigned long long*)(d + o_bt);
  unsigned long long* carry = (unsigned long long*)(d + o_ca);
  int32_t* row_clip = (int32_t*)(d + o_rc);
  int32_t* seg_clamped = (int32_t*)(d + o_sc);
  const int scan_grid = std::max(nblk, (nclip + 1 + BVH_SCAN_BLOCK - 1) / BVH_SCAN_BLOCK);
  hipLaunchKernelGGL(gmr::bvh_flip_scan_kernel, dim3(scan_grid), dim3(BVH_SCAN_BLOCK), 0, st, h->prog, d_rows, d_seg_start, nclip, B,
                     nblk, row_pref, row_clip, blk_tail, seg_clamped);
  if (nblk > 1)
    hipLaunchKernelGGL(gmr::bvh_carry_kernel, dim3((nclip + 255) / 256), dim3(256), 0, st, seg_clamped, nclip, nblk, blk_tail, carry);
  hipLaunchKernelGGL(gmr::bvh_frames_kernel, dim3((B + BVH_BLOCK - 1) / BVH_BLOCK), dim3(BVH_BLOCK), h->lds_bytes, st, h->prog, d_rows,
                     seg_clamped, d_offsets, nclip, B, T, row_pref, row_clip, carry, d_human);
  GMR_NAMED_HIP_TRY("gmr_bvh_frames_dev", hipGetLastError());
  return GMR_OK;
}

int gmr_bvh_frames(gmr_bvh_t* h, int nclip, int B, const double* rows, const int32_t* seg_start, const double* offsets, int T,
                   double* human) {
  if (!h) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames: null handle");
  if (nclip < 0 || B < 0 || T < 0) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames: negative nclip / B / T");
  if (nclip == 0) return B == 0 ? GMR_OK : gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames: B = %d rows but no clip", B);
  if (!seg_start || !offsets || !human || (B > 0 && !rows)) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames: null buffer");
  if (seg_start[0] != 0 || seg_start[nclip] != B) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames: seg_start runs from 0 to B = %d", B);
  for (int c = 0; c < nclip; c++) {
    const long long n = (long long)seg_start[c + 1] - seg_start[c];
    if (n < 0 || n > T) return gmr_fail(GMR_ERR_ARG, "gmr_bvh_frames: clip %d has %lld frames (0 .. T = %d)", c, n, T);
  }
  const gmr::BvhProg& P = h->prog;
  const size_t nb_rows = (size_t)B * P.ncol * 8, nb_seg = (size_t)(nclip + 1) * 4, nb_off = (size_t)nclip * P.J * 3 * 8,
               nb_out = (size_t)nclip * T * P.nrow * 7 * 8;
  gmr::Carve c;
  const size_t o_rows = c.take(nb_rows), o_seg = c.take(nb_seg), o_off = c.take(nb_off), o_out = c.take(nb_out);
  if (nb_out == 0) return GMR_OK;
  std::lock_guard<std::mutex> guard(h->host_mu);
  GMR_NAMED_HIP_TRY("gmr_bvh_frames", h->host_ws.reserve(c.total(), 4));
  char* d = h->host_ws.data();
  hipError_t e = hipSuccess;
  // rows at or beyond a clip's length come back as zeros (the kernels do not write them)
  if ((e = hipMemset(d + o_out, 0, nb_out)) != hipSuccess ||
      (nb_rows && (e = hipMemcpy(d + o_rows, rows, nb_rows, hipMemcpyHostToDevice)) != hipSuccess) ||
      (e = hipMemcpy(d + o_seg, seg_start, nb_seg, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d + o_off, offsets, nb_off, hipMemcpyHostToDevice)) != hipSuccess)
    return gmr_fail(GMR_ERR_HIP, "gmr_bvh_frames: %s", hipGetErrorString(e));
  int rc = gmr_bvh_frames_dev(h, nclip, B, (const double*)(d + o_rows), (const int32_t*)(d + o_seg), (const double*)(d + o_off), T,
                              (double*)(d + o_out), nullptr);
  if (rc == GMR_OK && (e = hipMemcpy(human, d + o_out, nb_out, hipMemcpyDeviceToHost)) != hipSuccess)
    rc = gmr_fail(GMR_ERR_HIP, "gmr_bvh_frames: %s", hipGetErrorString(e));
  return rc;
}

}  // extern "C"
