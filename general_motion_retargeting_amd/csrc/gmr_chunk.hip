// gmr_chunk.hip -- chunked retargeting of long clips (no reference analogue): a clip of n frames is cut
// into K chunks that run as independent IK streams, each chunk k >= 1 preceded by a few warm-up frames, so that a batch of a
// few long clips (LAFAN1: 77 clips of up to 9 855 frames) fills the device like a batch of thousands of short ones.  The IK
// kernels are not involved: chunks are ordinary streams of gmr_retarget_group_dev.  This file holds what surrounds that launch:
//
//   gmr_chunk_plan          (host) the chunk tables of a ragged batch
//   chunk_gather_kernel     clip-major human frames -> chunk-major frames, len_c, q0_c            (pure copy)
//   chunk_stitch_kernel     owned rows of chunk-major q_out_c / nsolve_c -> clip-major q_out / nsolve (pure copy), q_seam
//   chunk_finalize_kernel   per clip: status = first failing chunk, warm-up solves summed
//   chunk_resid_kernel      per seam: | q_seam - q_out at the frame before the chunk | as three numbers
//   chunk_scan_kernel       ordered list of the seams over the tolerance + their count; per-clip maxima
//
// A seam frame is computed twice -- as the last owned frame of chunk k - 1 and as the last warm-up frame of chunk k; the
// difference measures how far chunk k started from where the sequential run would have been.  A chunk whose seam is off is
// re-run from its predecessor's final state (repair mode of the gather), so the mode reports its error and can bound it.
//
// None of the tables is trusted on the device: a chunk record is clamped into its clip's rows and into a chunk's rows
// (load_chunk), a list entry outside [0, nchunk) is skipped, so no access leaves the buffers whatever the tables hold.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

// a - a must be 0 and conj(q) q must have a zero vector part exactly: a repaired seam has residual 0, not 1e-17 (with a
// contracted a*b + c*d the two roundings differ).  In front of the header: its qmul is compiled under this pragma too.
#pragma clang fp contract(off)

#include "../../include/gmr_hip.h"
#include "gmr_device_math.h"
#include "gmr_internal.h"

namespace gmr {

struct ChunkRec {
  int clip, src0, warm, owned;   // frames [src0, src0 + warm) warm up, [src0 + warm, src0 + warm + owned) are owned
  bool ok;
};

__device__ __forceinline__ ChunkRec load_chunk(const int32_t* __restrict__ chunk, int k, int S, int T, int Tc) {
  const int4 r = reinterpret_cast<const int4*>(chunk)[k];
  ChunkRec c;
  c.ok = r.x >= 0 && r.x < S;
  c.clip = min(max(r.x, 0), S - 1);
  c.src0 = min(max(r.y, 0), T);
  c.warm = min(max(r.z, 0), min(Tc, T - c.src0));
  c.owned = min(max(r.w, 0), min(Tc - c.warm, T - c.src0 - c.warm));
  return c;
}

// slot -> chunk: the listed chunk, or the slot itself without a list; -1 for an entry that names no chunk
__device__ __forceinline__ int slot_chunk(const int32_t* __restrict__ list, int slot, int nchunk) {
  const int k = list ? list[slot] : slot;
  return (k >= 0 && k < nchunk) ? k : -1;
}

// One tile of a contiguous run of n doubles: 256 lanes x 4 accesses of V doubles (V = 2: 16 B per lane, one 1 KiB
// instruction per wavefront), all four loads issued before the first store.
constexpr int COPY_ITERS = 4;
template <int V>
__device__ __forceinline__ void copy_tile(const double* __restrict__ src, double* __restrict__ dst, long long n, int tile) {
  const long long base = ((long long)tile * COPY_ITERS * 256 + threadIdx.x) * V;
  if (V == 2) {
    double2 v[COPY_ITERS];
#pragma unroll
    for (int i = 0; i < COPY_ITERS; i++) {
      const long long e = base + (long long)i * 512;
      if (e + 1 < n) v[i] = *reinterpret_cast<const double2*>(src + e);
      else if (e < n) v[i].x = src[e];
    }
#pragma unroll
    for (int i = 0; i < COPY_ITERS; i++) {
      const long long e = base + (long long)i * 512;
      if (e + 1 < n) *reinterpret_cast<double2*>(dst + e) = v[i];
      else if (e < n) dst[e] = v[i].x;
    }
  } else {
    double v[COPY_ITERS];
#pragma unroll
    for (int i = 0; i < COPY_ITERS; i++) {
      const long long e = base + (long long)i * 256;
      if (e < n) v[i] = src[e];
    }
#pragma unroll
    for (int i = 0; i < COPY_ITERS; i++) {
      const long long e = base + (long long)i * 256;
      if (e < n) dst[e] = v[i];
    }
  }
}

// grid (slots, tiles): block (s, t) copies tile t of the frames of slot s; tile 0 also writes the slot's len_c and q0_c row.
// mode 0: warm-up + owned frames, q0_c = the clip's q0;  mode 1 (repair): owned frames only, q0_c = q_seam[k] = clip-major
// q_out at the frame before the chunk (the clip's q0 for a chunk that starts its clip).
template <int V>
__global__ __launch_bounds__(256) void chunk_gather_kernel(int S, int T, int fd /* doubles per frame */, int nq, int nchunk, int Tc,
                                                           const int32_t* __restrict__ chunk, const int32_t* __restrict__ list, int mode,
                                                           const double* __restrict__ human, const double* __restrict__ q0,
                                                           const double* __restrict__ q_out, double* __restrict__ human_c,
                                                           int32_t* __restrict__ len_c, double* __restrict__ q0_c,
                                                           double* __restrict__ q_seam) {
  const int slot = blockIdx.x;
  const int k = slot_chunk(list, slot, nchunk);
  ChunkRec c;
  c.ok = false;
  if (k >= 0) c = load_chunk(chunk, k, S, T, Tc);
  if (!c.ok) {                                 // a slot without a chunk is an empty stream
    if (blockIdx.y == 0 && threadIdx.x == 0) len_c[slot] = 0;
    if (blockIdx.y == 0)
      for (int i = threadIdx.x; i < nq; i += 256) q0_c[(size_t)slot * nq + i] = q0[i];
    return;
  }
  const int first = mode ? c.src0 + c.warm : c.src0, frames = mode ? c.owned : c.warm + c.owned;
  if (blockIdx.y == 0) {
    if (threadIdx.x == 0) len_c[slot] = frames;
    const double* row = q0 + (size_t)c.clip * nq;
    if (mode && first > 0) row = q_out + ((size_t)c.clip * T + first - 1) * nq;
    for (int i = threadIdx.x; i < nq; i += 256) {
      const double v = row[i];
      q0_c[(size_t)slot * nq + i] = v;
      if (mode) q_seam[(size_t)k * nq + i] = v;
    }
  }
  copy_tile<V>(human + ((size_t)c.clip * T + first) * fd, human_c + (size_t)slot * Tc * fd, (long long)frames * fd, blockIdx.y);
}

// grid (slots, tiles_q + tiles_ns): the first tiles_q tiles copy the owned q rows of slot s, the others its owned nsolve rows
// (one 8-byte pair per lane).  Tile 0 also leaves the slot's status word in chunk_status[k] and, in pass 0 (mode 0), the
// chunk's last warm-up row in q_seam[k] (NaN for a chunk without warm-up: a seam nobody measured is not a good seam).
template <int V>
__global__ __launch_bounds__(256) void chunk_stitch_kernel(int S, int T, int nq, int nchunk, int Tc, int tiles_q,
                                                           const int32_t* __restrict__ chunk, const int32_t* __restrict__ list, int mode,
                                                           const double* __restrict__ q_out_c, const int32_t* __restrict__ nsolve_c,
                                                           const int32_t* __restrict__ status_c, double* __restrict__ q_out,
                                                           int32_t* __restrict__ nsolve, int32_t* __restrict__ chunk_status,
                                                           double* __restrict__ q_seam) {
  const int slot = blockIdx.x;
  const int k = slot_chunk(list, slot, nchunk);
  if (k < 0) return;
  const ChunkRec c = load_chunk(chunk, k, S, T, Tc);
  if (!c.ok) return;
  const int skip = mode ? 0 : c.warm, o0 = c.src0 + c.warm;      // owned rows start at row `skip` of the slot
  if (blockIdx.y == 0) {
    if (threadIdx.x == 0) chunk_status[k] = status_c[slot];
    if (!mode)
      for (int i = threadIdx.x; i < nq; i += 256)
        q_seam[(size_t)k * nq + i] = c.warm > 0 ? q_out_c[((size_t)slot * Tc + c.warm - 1) * nq + i] : (double)NAN;
  }
  if ((int)blockIdx.y < tiles_q) {
    copy_tile<V>(q_out_c + ((size_t)slot * Tc + skip) * nq, q_out + ((size_t)c.clip * T + o0) * nq, (long long)c.owned * nq, blockIdx.y);
  } else {
    copy_tile<1>(reinterpret_cast<const double*>(nsolve_c) + (size_t)slot * Tc + skip,
                 reinterpret_cast<double*>(nsolve) + (size_t)c.clip * T + o0, c.owned, blockIdx.y - tiles_q);
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wavefront per clip: status[c] = the first non-OK status of the clip's chunks in order; in pass 0 (nsolve_c given) the
// solves of all warm-up rows of the clip summed into warm_solves[c] (integer sums: the order does not matter).
__global__ __launch_bounds__(256) void chunk_finalize_kernel(int S, int T, int nchunk, int Tc, const int32_t* __restrict__ chunk,
                                                             const int32_t* __restrict__ clip_first, const int32_t* __restrict__ chunk_status,
                                                             const int32_t* __restrict__ nsolve_c, int32_t* __restrict__ status,
                                                             int32_t* __restrict__ warm_solves) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= S) return;
  const int k0 = min(max(clip_first[c], 0), nchunk), k1 = min(max(clip_first[c + 1], k0), nchunk);
  int bad = INT_MAX, sum = 0;
  for (int k = k0 + lane; k < k1; k += 64)
    if (chunk_status[k] != GMR_STATUS_OK) { bad = k; break; }
  bad = wave_min(bad);
  if (nsolve_c) {
    for (int k = k0; k < k1; k++) {
      const ChunkRec r = load_chunk(chunk, k, S, T, Tc);
      for (int t = lane; t < r.warm; t += 64) {
        const int2 n = reinterpret_cast<const int2*>(nsolve_c)[(size_t)k * Tc + t];
        sum += n.x + n.y;
      }
    }
    sum = wave_sum(sum);
  }
  if (lane == 0) {
    status[c] = bad < INT_MAX ? chunk_status[bad] : GMR_STATUS_OK;
    if (nsolve_c) warm_solves[c] = sum;
  }
}

// whether chunk k has a seam in front of it (it does not start its clip), and the row of q_out in front of it
__device__ __forceinline__ bool seam_of(const ChunkRec& c, int k, const int32_t* __restrict__ clip_first, int nchunk) {
  return k > 0 && c.ok && c.src0 + c.warm > 0 && min(max(clip_first[c.clip], 0), nchunk) != k;
}

// One thread per chunk: resid[k] = (max |d joint angle|, max |d root position|, angle between the root orientations) of
// q_seam[k] against clip-major q_out at the frame before the chunk; zeros for a chunk that starts its clip.
__global__ __launch_bounds__(256) void chunk_resid_kernel(int S, int T, int nq, int nchunk, int Tc, const int32_t* __restrict__ chunk,
                                                          const int32_t* __restrict__ clip_first, const double* __restrict__ q_out,
                                                          const double* __restrict__ q_seam, double* __restrict__ resid) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nchunk) return;
  const ChunkRec c = load_chunk(chunk, k, S, T, Tc);
  double r0 = 0.0, r1 = 0.0, r2 = 0.0;
  if (seam_of(c, k, clip_first, nchunk)) {
    const double* a = q_out + ((size_t)c.clip * T + c.src0 + c.warm - 1) * nq;
    const double* b = q_seam + (size_t)k * nq;
    // (d > r || d != d: a NaN difference sticks, whatever comes after it)
    for (int i = 7; i < nq; i++) {
      const double d = fabs(b[i] - a[i]);
      if (d > r0 || d != d) r0 = d;
    }
    for (int i = 0; i < 3; i++) {
      const double d = fabs(b[i] - a[i]);
      if (d > r1 || d != d) r1 = d;
    }
    // angle of a^-1 b = 2 atan2(|vector part|, |scalar part|): the same for b and -b, no cancellation near 0 (acos has)
    const d4 d = qmul(qconj(d4{a[3], a[4], a[5], a[6]}), d4{b[3], b[4], b[5], b[6]});
    const double n = sqrt(d.x * d.x + d.y * d.y + d.z * d.z), w = fabs(d.w);
    r2 = (n > 0.0 || w > 0.0) ? 2.0 * atan2_q1(n, w) : (double)NAN;      // (NaN operands fail both tests)
    // the same four numbers are the same rotation: exactly 0, whatever the products above round to
    if ((n == 0.0 && w > 0.0) || (a[3] == b[3] && a[4] == b[4] && a[5] == b[5] && a[6] == b[6] && w > 0.0)) r2 = 0.0;
  }
  resid[(size_t)k * 3 + 0] = r0;
  resid[(size_t)k * 3 + 1] = r1;
  resid[(size_t)k * 3 + 2] = r2;
}

// Block 0: the chunks whose seam is over the tolerance, in chunk order -- 1 024 chunks per step: a ballot and a prefix
// count per wavefront, the sixteen wavefront totals through LDS -- so the list does not depend on how anything was
// scheduled.  A seam behind a failed chunk is not listed: running it again cannot mend it, and its clip fails anyway.
// Blocks 1 ..: one thread per clip, seam_max[c] = the maxima of its chunks' residuals (NaN sticks).
__global__ __launch_bounds__(1024) void chunk_scan_kernel(int S, int T, int nchunk, int Tc, const int32_t* __restrict__ chunk,
                                                          const int32_t* __restrict__ clip_first, const int32_t* __restrict__ chunk_status,
                                                          const double* __restrict__ resid, double tol, int32_t* __restrict__ bad_list,
                                                          int32_t* __restrict__ nbad, double* __restrict__ seam_max) {
  if (blockIdx.x > 0) {
    const int c = (blockIdx.x - 1) * 1024 + threadIdx.x;
    if (c >= S) return;
    const int k0 = min(max(clip_first[c], 0), nchunk), k1 = min(max(clip_first[c + 1], k0), nchunk);
    double m[3] = {0.0, 0.0, 0.0};
    for (int k = k0; k < k1; k++)
      for (int i = 0; i < 3; i++) {
        const double r = resid[(size_t)k * 3 + i];
        if (r > m[i] || r != r) m[i] = r;
      }
    for (int i = 0; i < 3; i++) seam_max[(size_t)c * 3 + i] = m[i];
    return;
  }
  __shared__ int wave_count[16];
  __shared__ int base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int k0 = 0; k0 < nchunk; k0 += 1024) {
    const int k = k0 + threadIdx.x;
    bool bad = false;
    if (k < nchunk) {
      const ChunkRec c = load_chunk(chunk, k, S, T, Tc);
      if (seam_of(c, k, clip_first, nchunk) && chunk_status[k - 1] == GMR_STATUS_OK) {
        const double r0 = resid[(size_t)k * 3], r1 = resid[(size_t)k * 3 + 1], r2 = resid[(size_t)k * 3 + 2];
        bad = !(r0 <= tol && r1 <= tol && r2 <= tol);               // (a NaN residual is not <= tol)
      }
    }
    const unsigned long long m = __ballot(bad);
    if (lane == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int at = base;
    for (int w = 0; w < wave; w++) at += wave_count[w];
    if (bad) bad_list[at + __popcll(m & ((1ull << lane) - 1ull))] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
      int n = base;
      for (int w = 0; w < 16; w++) n += wave_count[w];
      base = n;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) nbad[0] = base;
}

}  // namespace gmr

namespace {
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

int check_dims(const char* who, int S, int T, int nq, int nchunk, int Tc, int nslot) {
  if (S < 0 || T < 1 || nchunk < 0 || Tc < 1 || nslot < 0 || nslot > nchunk) return gmr_fail(GMR_ERR_ARG, "%s: S >= 0, T >= 1, Tc >= 1, 0 <= slots <= nchunk", who);
  if (nq < 7 || nq > GMR_MAX_NQ) return gmr_fail(GMR_ERR_ARG, "%s: nq = %d (7 .. %d)", who, nq, GMR_MAX_NQ);
  if ((long long)S * T > INT32_MAX || (long long)nchunk * Tc > INT32_MAX) return gmr_fail(GMR_ERR_ARG, "%s: more than 2^31 rows", who);
  return GMR_OK;
}
}  // namespace

extern "C" {

int gmr_chunk_plan(int nclip, const int32_t* len, int L, int W, int capacity, int32_t* chunk, int32_t* clip_first, int* nchunk, int* Tc) {
  if (nclip < 0 || (nclip > 0 && !len)) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_plan: nclip >= 0 and their lengths");
  if (L < 1 || W < 0) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_plan: L = %d (>= 1), W = %d (>= 0)", L, W);
  long long total = 0;
  int longest = 1;
  for (int c = 0; c < nclip; c++) {
    const int n = len[c];
    if (n < 0) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_plan: clip %d has %d frames", c, n);
    const long long K = n > L ? ((long long)n + L - 1) / L : 1;
    if (K > 1 && W < 1) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_plan: clip %d (%d frames) is split at L = %d: that needs W >= 1 warm-up frames", c, n, L);
    total += K;
    if (total > INT32_MAX) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_plan: more than 2^31 chunks");
  }
  if (chunk && capacity < total) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_plan: room for %d chunks, %lld needed", capacity, total);
  int k = 0;
  for (int c = 0; c < nclip; c++) {
    const long long n = len[c], K = n > L ? (n + L - 1) / L : 1;
    if (clip_first) clip_first[c] = k;
    for (long long i = 0; i < K; i++, k++) {
      const int a = (int)(i * n / K), b = (int)((i + 1) * n / K), warm = i > 0 ? (W < a ? W : a) : 0;
      if (warm + b - a > longest) longest = warm + b - a;
      if (chunk) {
        chunk[4 * k + 0] = c;
        chunk[4 * k + 1] = a - warm;
        chunk[4 * k + 2] = warm;
        chunk[4 * k + 3] = b - a;
      }
    }
  }
  if (clip_first) clip_first[nclip] = k;
  if (nchunk) *nchunk = (int)total;
  if (Tc) *Tc = longest;
  return GMR_OK;
}

int gmr_chunk_gather_dev(int S, int T, int nhuman, int nq, int nchunk, int Tc, const int32_t* d_chunk, const int32_t* d_list, int nlist,
                         int mode, const double* d_human, const double* d_q0, const double* d_q_out, double* d_human_c,
                         int32_t* d_len_c, double* d_q0_c, double* d_q_seam, void* stream) {
  const int nslot = d_list ? nlist : nchunk;
  if (int rc = check_dims("gmr_chunk_gather_dev", S, T, nq, nchunk, Tc, nslot)) return rc;
  if (nhuman < 1 || nhuman > GMR_MAX_HUMAN) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_gather_dev: nhuman = %d", nhuman);
  if (mode != GMR_CHUNK_PASS0 && mode != GMR_CHUNK_REPAIR) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_gather_dev: mode %d", mode);
  if (nslot == 0) return GMR_OK;
  if (S < 1 || !d_chunk || !d_human || !d_q0 || !d_human_c || !d_len_c || !d_q0_c || (mode == GMR_CHUNK_REPAIR && (!d_q_out || !d_q_seam)))
    return gmr_fail(GMR_ERR_ARG, "gmr_chunk_gather_dev: null buffer");
  const int fd = nhuman * 7;
  const bool wide = fd % 2 == 0 && aligned16(d_human) && aligned16(d_human_c);
  const int per_tile = 256 * gmr::COPY_ITERS * (wide ? 2 : 1);
  const long long tiles = ((long long)Tc * fd + per_tile - 1) / per_tile;
  if (tiles > 65535) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_gather_dev: chunks of %d frames are too long", Tc);
  const dim3 grid(nslot, (unsigned)tiles);
  if (wide)
    hipLaunchKernelGGL(gmr::chunk_gather_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, S, T, fd, nq, nchunk, Tc, d_chunk, d_list, mode,
                       d_human, d_q0, d_q_out, d_human_c, d_len_c, d_q0_c, d_q_seam);
  else
    hipLaunchKernelGGL(gmr::chunk_gather_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, S, T, fd, nq, nchunk, Tc, d_chunk, d_list, mode,
                       d_human, d_q0, d_q_out, d_human_c, d_len_c, d_q0_c, d_q_seam);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

int gmr_chunk_stitch_dev(int S, int T, int nq, int nchunk, int Tc, const int32_t* d_chunk, const int32_t* d_clip_first,
                         const int32_t* d_list, int nlist, int mode, const double* d_q_out_c, const int32_t* d_nsolve_c,
                         const int32_t* d_status_c, double* d_q_out, int32_t* d_nsolve, int32_t* d_chunk_status, int32_t* d_status,
                         double* d_q_seam, int32_t* d_warm_solves, void* stream) {
  const int nslot = d_list ? nlist : nchunk;
  if (int rc = check_dims("gmr_chunk_stitch_dev", S, T, nq, nchunk, Tc, nslot)) return rc;
  if (mode != GMR_CHUNK_PASS0 && mode != GMR_CHUNK_REPAIR) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_stitch_dev: mode %d", mode);
  if (mode == GMR_CHUNK_PASS0 && d_list) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_stitch_dev: pass 0 takes all chunks (no list)");
  if (S == 0 || nchunk == 0) return GMR_OK;
  if (!d_chunk || !d_clip_first || !d_q_out_c || !d_nsolve_c || !d_status_c || !d_q_out || !d_nsolve || !d_chunk_status || !d_status ||
      (mode == GMR_CHUNK_PASS0 && (!d_q_seam || !d_warm_solves)))
    return gmr_fail(GMR_ERR_ARG, "gmr_chunk_stitch_dev: null buffer");
  if (!aligned8(d_nsolve_c) || !aligned8(d_nsolve)) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_stitch_dev: nsolve rows are 8-byte aligned pairs");
  hipStream_t st = (hipStream_t)stream;
  if (nslot > 0) {
    const bool wide = nq % 2 == 0 && aligned16(d_q_out_c) && aligned16(d_q_out);
    const int per_tile = 256 * gmr::COPY_ITERS * (wide ? 2 : 1);
    const long long tiles_q = ((long long)Tc * nq + per_tile - 1) / per_tile, tiles_ns = (Tc + 256 * gmr::COPY_ITERS - 1) / (256 * gmr::COPY_ITERS);
    if (tiles_q + tiles_ns > 65535) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_stitch_dev: chunks of %d frames are too long", Tc);
    const dim3 grid(nslot, (unsigned)(tiles_q + tiles_ns));
    if (wide)
      hipLaunchKernelGGL(gmr::chunk_stitch_kernel<2>, grid, dim3(256), 0, st, S, T, nq, nchunk, Tc, (int)tiles_q, d_chunk, d_list, mode,
                         d_q_out_c, d_nsolve_c, d_status_c, d_q_out, d_nsolve, d_chunk_status, d_q_seam);
    else
      hipLaunchKernelGGL(gmr::chunk_stitch_kernel<1>, grid, dim3(256), 0, st, S, T, nq, nchunk, Tc, (int)tiles_q, d_chunk, d_list, mode,
                         d_q_out_c, d_nsolve_c, d_status_c, d_q_out, d_nsolve, d_chunk_status, d_q_seam);
    GMR_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(gmr::chunk_finalize_kernel, dim3((S + 3) / 4), dim3(256), 0, st, S, T, nchunk, Tc, d_chunk, d_clip_first, d_chunk_status,
                     mode == GMR_CHUNK_PASS0 ? d_nsolve_c : (const int32_t*)nullptr, d_status, d_warm_solves);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

int gmr_chunk_seams_dev(int S, int T, int nq, int nchunk, int Tc, const int32_t* d_chunk, const int32_t* d_clip_first,
                        const double* d_q_out, const double* d_q_seam, const int32_t* d_chunk_status, double tol, double* d_resid,
                        int32_t* d_bad_list, int32_t* d_nbad, double* d_seam_max, void* stream) {
  if (int rc = check_dims("gmr_chunk_seams_dev", S, T, nq, nchunk, Tc, 0)) return rc;
  if (!(tol >= 0.0)) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_seams_dev: the tolerance is a number >= 0");
  if (!d_nbad) return gmr_fail(GMR_ERR_ARG, "gmr_chunk_seams_dev: null count");
  hipStream_t st = (hipStream_t)stream;
  if (S == 0 || nchunk == 0) {
    GMR_HIP_TRY(hipMemsetAsync(d_nbad, 0, 4, st));
    return GMR_OK;
  }
  if (!d_chunk || !d_clip_first || !d_q_out || !d_q_seam || !d_chunk_status || !d_resid || !d_bad_list || !d_seam_max)
    return gmr_fail(GMR_ERR_ARG, "gmr_chunk_seams_dev: null buffer");
  hipLaunchKernelGGL(gmr::chunk_resid_kernel, dim3((nchunk + 255) / 256), dim3(256), 0, st, S, T, nq, nchunk, Tc, d_chunk, d_clip_first,
                     d_q_out, d_q_seam, d_resid);
  GMR_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(gmr::chunk_scan_kernel, dim3(1 + (S + 1023) / 1024), dim3(1024), 0, st, S, T, nchunk, Tc, d_chunk, d_clip_first,
                     d_chunk_status, d_resid, tol, d_bad_list, d_nbad, d_seam_max);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // extern "C"
