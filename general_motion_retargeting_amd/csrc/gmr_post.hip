// gmr_post.hip -- post-processing of the dataset drivers on the device (row H10 of SURVEY.md section 8a): what
// `process_file` does between the retargeting loop and pickle.dump (reference scripts/smplx_to_robot_dataset.py:97-131),
// for every clip of a batch, reading the IK launch's padded float64 output where it lies.
//
//   post_row_map_kernel   output row b -> (clip, frame) -> address of its qpos row (binary search of seg_start, once per
//                         row; the two FK passes and the gather all find their row through this map)
//   fk_*_kernel<FkSrcQpos>  (gmr_fk.hip) the tree walk of the FK entry points, fed from those rows: identity root ->
//                         local_body_pos; the frame's own root -> workspace -> fk_segment_min_kernel -> lowest[clip]
//   post_gather_kernel    root_pos / root_rot (wxyz -> xyzw) / dof_pos, clip-contiguous float64, with the two root
//                         adjustments applied on the way (the per-clip minimum is known by then)
//
// Output rows are dense: block i of every kernel owns rows [64 i, 64 i + 64) of the concatenation of all clips, whatever
// clip they belong to.  The FK flush relies on a block's output range starting 16-byte aligned, which 64 * nbody * 12 B
// blocks from an aligned base do and clip-aligned blocks (seg_start[s] * nbody * 12 B) would not.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gmr_hip.h"
#include "gmr_fk_handle.h"    // struct gmr_fk: the tree and the scratch of a call
#include "gmr_internal.h"
#include "gmr_launch.h"       // the prototypes of the launchers below and of the FK launchers
#include "gmr_post.h"

// float64 arithmetic here mirrors NumPy's (one rounding per operation)
#pragma clang fp contract(off)

namespace gmr {

// One thread per output row.  seg_start comes from the caller and is not trusted beyond what the host could check: the
// search runs over [0, C), a frame index is clamped into the rows its clip's IK stream owns, so every address written to
// row_q lies inside a source's q_out even for an inconsistent prefix sum.  The first C + 1 threads also leave a copy of
// seg_start clamped to [0, B] for the kernels that use it as loop bounds (fk_segment_min_kernel) or as a row index.
__global__ __launch_bounds__(256) void post_row_map_kernel(const PostSources src, const int32_t* __restrict__ seg_start, int C,
                                                           int B, int nq, const double** __restrict__ row_q,
                                                           int32_t* __restrict__ row_clip, int32_t* __restrict__ seg_clamped) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b <= C) seg_clamped[b] = min(max(seg_start[b], 0), B);
  if (b >= B) return;
  // the clip of row b: the LAST s with seg_start[s] <= b (an empty clip shares its start with the clip after it)
  int lo = 0, hi = C - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const int s = lo;
  // its source: a scan of a few wave-uniform counts (clip0 ascends: the last source that starts at or before s)
  int c0 = src.clip0[0], T = src.T[0];
  const int32_t* len = src.len[0];
  const double* q = src.q_out[0];
#pragma unroll
  for (int k = 1; k < POST_MAX_SRC; k++)
    if (k < src.nsrc && s >= src.clip0[k]) { c0 = src.clip0[k]; T = src.T[k]; len = src.len[k]; q = src.q_out[k]; }
  const int ls = s - c0;
  const int rows = len ? min(max(len[ls], 1), T) : T;
  const int t = min(max(b - seg_start[s], 0), rows - 1);
  row_q[b] = q + ((size_t)ls * T + t) * nq;
  row_clip[b] = s;
}

// Flat over the 8-byte elements of the valid rows: element e = (row b, column c).  The rows of a clip are one contiguous
// range of q_out, so a wavefront's loads are contiguous except across a clip boundary, and its stores are contiguous runs
// of the three outputs.  Block i handles rows [64 i, 64 i + 64).
constexpr int POST_ROWS = 64;
__global__ __launch_bounds__(256) void post_gather_kernel(const double* const* __restrict__ row_q, const int32_t* __restrict__ row_clip,
                                                          const int32_t* __restrict__ seg_clamped, const float* __restrict__ lowest,
                                                          int B, int nq, int flags, double ground_offset,
                                                          double* __restrict__ root_pos, double* __restrict__ root_rot,
                                                          double* __restrict__ dof_pos) {
  const int b0 = blockIdx.x * POST_ROWS;
  const int nrow = min(B - b0, POST_ROWS), ndof = nq - 7;
  for (int e = threadIdx.x; e < nrow * nq; e += 256) {
    const int r = e / nq, c = e - r * nq, b = b0 + r;
    double v = row_q[b][c];
    if (c >= 7) {
      dof_pos[(size_t)b * ndof + (c - 7)] = v;
    } else if (c >= 3) {
      root_rot[(size_t)b * 4 + ((c - 4) & 3)] = v;                    // wxyz -> xyzw (:98)
    } else {
      if (c == 2) {
        // root_pos[:, 2] = root_pos[:, 2] - lowest + ground_offset: two float64 operations in this order (:126)
        if (flags & GMR_POST_HEIGHT_ADJUST) v = v - (double)lowest[row_clip[b]] + ground_offset;
      } else if (flags & GMR_POST_ROOT_ORIGIN_OFFSET) {
        // root_pos[:, :2] -= root_pos[0, :2] (:130): the clip's first frame as the IK left it
        v = v - row_q[min(seg_clamped[row_clip[b]], B - 1)][c];
      }
      root_pos[(size_t)b * 3 + c] = v;
    }
  }
}

}  // namespace gmr

extern "C" hipError_t gmr_launch_post_row_map(const gmr::PostSources* src, const int32_t* d_seg_start, int C, int B, int nq,
                                              const double** d_row_q, int32_t* d_row_clip, int32_t* d_seg_clamped,
                                              hipStream_t stream) {
  const int n = (B > C + 1 ? B : C + 1);
  hipLaunchKernelGGL(gmr::post_row_map_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *src, d_seg_start, C, B, nq, d_row_q,
                     d_row_clip, d_seg_clamped);
  return hipGetLastError();
}

extern "C" hipError_t gmr_launch_post_gather(const double* const* d_row_q, const int32_t* d_row_clip, const int32_t* d_seg_clamped,
                                             const float* d_lowest, int B, int nq, int flags, double ground_offset,
                                             double* d_root_pos, double* d_root_rot, double* d_dof_pos, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(gmr::post_gather_kernel, dim3((B + gmr::POST_ROWS - 1) / gmr::POST_ROWS), dim3(256), 0, stream, d_row_q,
                     d_row_clip, d_seg_clamped, d_lowest, B, nq, flags, ground_offset, d_root_pos, d_root_rot, d_dof_pos);
  return hipGetLastError();
}

// ---- the C-ABI: the dataset drivers' post-processing on the device ---------------------------------------------------------
#define fail gmr_fail
extern "C" {

int gmr_postprocess_clips_dev(gmr_fk_t* k, const gmr_post_src_t* src, int nsrc, int nq, const int32_t* d_seg_start, int C, int B,
                              int flags, double ground_offset, double* d_root_pos, double* d_root_rot, double* d_dof_pos,
                              float* d_local_body_pos, float* d_lowest, void* stream) {
  if (!k) return fail(GMR_ERR_ARG, "null fk handle");
  if (nsrc < 0 || nsrc > gmr::POST_MAX_SRC || (nsrc > 0 && !src)) return fail(GMR_ERR_ARG, "bad source list (at most %d sources)", gmr::POST_MAX_SRC);
  if (nq != 7 + k->tree.ndof) return fail(GMR_ERR_ARG, "nq = %d, but this tree has %d dofs (nq = %d)", nq, k->tree.ndof, 7 + k->tree.ndof);
  if (C < 0 || B < 0) return fail(GMR_ERR_ARG, "negative C / B");
  if (flags & ~(GMR_POST_HEIGHT_ADJUST | GMR_POST_ROOT_ORIGIN_OFFSET)) return fail(GMR_ERR_ARG, "unknown flag bits 0x%x", flags);
  gmr::PostSources ps;
  memset(&ps, 0, sizeof ps);
  ps.nsrc = nsrc;
  long long clips = 0, rows = 0;
  for (int i = 0; i < nsrc; i++) {
    if (src[i].S < 0 || src[i].T < 0) return fail(GMR_ERR_ARG, "source %d: negative S/T", i);
    if (src[i].S > 0 && (src[i].T < 1 || !src[i].q_out)) return fail(GMR_ERR_ARG, "source %d: S = %d streams need T >= 1 and q_out", i, src[i].S);
    ps.clip0[i] = (int32_t)clips;
    ps.T[i] = src[i].T;
    ps.q_out[i] = src[i].q_out;
    ps.len[i] = src[i].len;
    clips += src[i].S;
    rows += (long long)src[i].S * src[i].T;
    if (clips > INT32_MAX) return fail(GMR_ERR_ARG, "too many clips");
  }
  for (int i = nsrc; i <= gmr::POST_MAX_SRC; i++) ps.clip0[i] = (int32_t)clips;
  if (clips != C) return fail(GMR_ERR_ARG, "C = %d, but the sources hold %lld clips", C, clips);
  if (B > rows) return fail(GMR_ERR_ARG, "B = %d rows, but the sources hold only %lld", B, rows);
  if (C == 0) return GMR_OK;
  if (!d_seg_start) return fail(GMR_ERR_ARG, "null seg_start");
  if (B > 0 && (!d_root_pos || !d_root_rot || !d_local_body_pos || (k->tree.ndof > 0 && !d_dof_pos))) return fail(GMR_ERR_ARG, "null output buffer");
  const bool height = flags & GMR_POST_HEIGHT_ADJUST;
  if (B == 0 && !(height && d_lowest)) return GMR_OK;
  // scratch: row_q [B] pointers, row_clip [B], seg_clamped [C + 1], lowest [C] (when the caller does not want it), and the
  // world pass's body_pos [B][nbody][3]
  gmr::Carve c;
  const size_t o_rq = c.take((size_t)B * 8), o_rc = c.take((size_t)B * 4), o_sc = c.take((size_t)(C + 1) * 4), o_lo = c.take((size_t)C * 4),
               o_bp = c.take(height ? (size_t)B * k->tree.nbody * 12 : 0);
  hipStream_t st = (hipStream_t)stream;
  const auto ws = k->post_ws.acquire(st, c.total());           // (held until the last launch below is enqueued)
  GMR_NAMED_HIP_TRY("gmr_postprocess_clips_dev: scratch", ws.error());
  char* d = ws.base();
  const double** row_q = (const double**)(d + o_rq);
  int32_t* row_clip = (int32_t*)(d + o_rc);
  int32_t* seg_clamped = (int32_t*)(d + o_sc);
  float* lowest = d_lowest ? d_lowest : (float*)(d + o_lo);
  GMR_HIP_TRY(gmr_launch_post_row_map(&ps, d_seg_start, C, B, nq, row_q, row_clip, seg_clamped, st));
  if (height) {
    GMR_HIP_TRY(gmr_launch_fk_qpos(k->dev(), &k->tree, B, row_q, 1, (float*)(d + o_bp), st));
    GMR_HIP_TRY(gmr_launch_fk_segment_min((const float*)(d + o_bp), k->tree.nbody, seg_clamped, C, lowest, st));
  }
  GMR_HIP_TRY(gmr_launch_fk_qpos(k->dev(), &k->tree, B, row_q, 0, d_local_body_pos, st));
  GMR_HIP_TRY(gmr_launch_post_gather(row_q, row_clip, seg_clamped, lowest, B, nq, flags, ground_offset, d_root_pos, d_root_rot, d_dof_pos, st));
  return GMR_OK;
}

}  // extern "C"
