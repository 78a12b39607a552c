// gmr_fk.hip -- post-hoc batched forward kinematics, float32 (rows H8-H9 of SURVEY.md section 8a).
//
// Replaces KinematicsModel.forward_kinematics (reference kinematics_model.py:213-246), which on the
// reference's "cuda:0" path is ~70 tiny ATen launches per body (~2.6k per call), by one kernel.
// This one IS bandwidth-shaped: 4*ndof + 28 B in, 12*nbody (+16*nbody) B out per frame.
//
// Lane mapping: one lane per FRAME, bodies visited in the tree's DFS order by the whole wave
// (wave-uniform control flow, no divergence).  In DFS order a body's first child follows it
// immediately, so the parent transform is usually still in registers; only bodies with two or more
// children are parked in LDS slots [slot][component][lane] (conflict-free; 2-3 slots for a humanoid)
// and reloaded when a later child comes up.  The serial order per frame is exactly the reference's
// (pos_j = pos_p + rot_p * t_j;
// rot_j = rot_p * (r_j * jr_j)), hence the same rounding sequence as its float32 loop.
// Stores: a lane's pieces (12 B of body j) are 456 B apart from its neighbour's, and ~100k frames are
// in flight chip-wide, more than L2 can hold until a line is complete -- written straight from
// registers they reach HBM as partial lines (measured 0.9 TB/s).  The positions-only variant (all the
// dataset scripts consume, smplx_to_robot_dataset.py:110,121) therefore stages the wave's 64 x 456 B
// = 29 KB output block in LDS in its final layout and streams it out with contiguous 16 B-per-lane
// stores, every line written once and whole.  With rotations requested the direct stores are kept.
// The dof row of a frame (116 B) is read element by element but stays L1-resident across the walk.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <new>

#include "../../include/gmr_hip.h"
#include "gmr_fk_tree.h"
#include "gmr_fk_walk.h"      // f4, qmul_xyzw, qrot_xyzw, fk_body: the per-body step
#include "gmr_fk_handle.h"    // struct gmr_fk
#include "gmr_internal.h"
#include "gmr_launch.h"       // the prototypes of the launchers below

// float32 arithmetic here mirrors torch eager ops (one rounding per operation): no FMA contraction,
// which also makes both template variants produce the same bits
#pragma clang fp contract(off)

namespace gmr {

// fminf without the two canonicalising v_max the compiler puts in front of llvm.minnum (one instruction per body
// instead of three; NaN handling as v_min_f32 in IEEE mode: a quiet NaN operand loses)
__device__ __forceinline__ float min1(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

constexpr int FK_BLOCK = 64;  // one wave per block

// Where a lane's root pose and joint angles come from.  The kernels below are written once against this interface; only
// the loads at their top differ between the instantiations, the per-body code, the LDS staging and the flush are shared.
struct FkSrcF32 {      // gmr_fk_batch_dev: three float32 arrays indexed by frame
  const float* __restrict__ root_pos;
  const float* __restrict__ root_rot;
  const float* __restrict__ dof;
  struct Lane {
    const float* rp;
    const float* rr;
    const float* d;
    __device__ __forceinline__ float ang(int k) const { return d[k]; }
    __device__ __forceinline__ void root(float& px, float& py, float& pz, f4& rot) const {
      px = rp[0]; py = rp[1]; pz = rp[2];
      rot = f4{rr[0], rr[1], rr[2], rr[3]};
    }
  };
  __device__ __forceinline__ Lane lane(long long fc, int ndof) const { return Lane{root_pos + fc * 3, root_rot + fc * 4, dof + fc * ndof}; }
};
// gmr_postprocess_clips_dev: frame b is the float64 qpos row row_q[b] of an IK launch's output, read where it lies
// (root position, root quaternion wxyz, joint angles), each value rounded to float32 as the dataset scripts' `.float()` does
// (smplx_to_robot_dataset.py:106-121).  WORLD = false: the identity root of `local_body_pos` (:106-112).
template <bool WORLD>
struct FkSrcQpos {
  const double* const* __restrict__ row_q;
  struct Lane {
    const double* q;
    __device__ __forceinline__ float ang(int k) const { return (float)q[7 + k]; }
    __device__ __forceinline__ void root(float& px, float& py, float& pz, f4& rot) const {
      if (WORLD) {
        px = (float)q[0]; py = (float)q[1]; pz = (float)q[2];
        rot = f4{(float)q[4], (float)q[5], (float)q[6], (float)q[3]};
      } else {
        px = 0.0f; py = 0.0f; pz = 0.0f;
        rot = f4{0.0f, 0.0f, 0.0f, 1.0f};
      }
    }
  };
  __device__ __forceinline__ Lane lane(long long fc, int) const { return Lane{row_q[fc]}; }
};

template <bool STAGED, class Src>
__global__ __launch_bounds__(FK_BLOCK) void fk_batch_kernel(const FkTree* __restrict__ tree, int B, const Src src,
                                                            float* __restrict__ body_pos,
                                                            float* __restrict__ body_rot,
                                                            float* __restrict__ min_part) {
  // slots [nslot][SW][FK_BLOCK], then (STAGED) pos [FK_BLOCK][nb*3], rot [FK_BLOCK][nb*4].  A parked parent needs
  // SW = 7 floats (pos, rot) when results go straight to memory; when they are staged, the parent's position is
  // simply re-read from the staging area and only the rotation is parked (conflict-free columns): SW = 4
  extern __shared__ __align__(16) float fsm[];
  __shared__ float red[FK_BLOCK / 64];
  const int nb = tree->nbody, ndof = tree->ndof;
  const int tid = threadIdx.x;
  const long long f = (long long)blockIdx.x * FK_BLOCK + tid;
  const bool on = f < B;
  const long long fc = on ? f : 0;
  const typename Src::Lane in = src.lane(fc, ndof);
  const int SW = STAGED ? 4 : 7;
  float* stk = fsm + tid;
  const int row = nb * 3;
  float* outb = fsm + tree->nslot * SW * FK_BLOCK;  // used when STAGED
  float* outr = outb + FK_BLOCK * row;             // used when STAGED and body_rot
  const int rrow = nb * 4;
  float zmin = INFINITY;
  float cpx, cpy, cpz;   // transform of the body visited last (the parent of a first child)
  f4 crot;
  if (STAGED && ndof > 0) {
    // Park dof d of this lane's frame in its staging row at the slot of the body it drives: the walk reads it there
    // right before it overwrites the slot with that body's position.  (Read per body during the walk, a lane's 116-B
    // row shares no line with its neighbours': 64 lines per load and 41 KB of lines per CU in flight between two uses
    // -> the vector L1 thrashes, 12x the L2 reads, 42 % of the wave's cycles waiting: profiles/r02_fk_*.)
    // Every lane reads ITS row, all loads issued back to back (independent: one trip to L2, each line fetched once
    // while its 29 users are in flight), and parks the values in its own staging row -- no cross-lane traffic.
    float* orow = outb + tid * row;
#pragma unroll 8
    for (int d = 0; d < ndof; d++) orow[3 * tree->dof_body[d]] = in.ang(d);
  }
  {
    float px, py, pz;
    f4 rot;
    in.root(px, py, pz, rot);
    cpx = px; cpy = py; cpz = pz; crot = rot;
    if (tree->save_slot[0] >= 0 && SW > 0) {
      float* sl = stk + tree->save_slot[0] * SW * FK_BLOCK;
      if (SW == 7) { sl[0] = px; sl[FK_BLOCK] = py; sl[2 * FK_BLOCK] = pz; sl += 3 * FK_BLOCK; }
      sl[0] = rot.x; sl[FK_BLOCK] = rot.y; sl[2 * FK_BLOCK] = rot.z; sl[3 * FK_BLOCK] = rot.w;
    }
    if (STAGED) {
      float* o = outb + tid * row;
      o[0] = px; o[1] = py; o[2] = pz;
      if (body_rot) *reinterpret_cast<float4*>(outr + tid * rrow) = make_float4(rot.x, rot.y, rot.z, rot.w);
      if (on) zmin = pz;
    } else if (on) {
      float* op = body_pos + f * nb * 3;
      op[0] = px; op[1] = py; op[2] = pz;
      if (body_rot) { float* orr = body_rot + f * nb * 4; orr[0] = rot.x; orr[1] = rot.y; orr[2] = rot.z; orr[3] = rot.w; }   // (this variant runs when a destination is not 16-B aligned)
      zmin = pz;
    }
  }
  FkBodyRec nxt = tree->rec[nb > 1 ? 1 : 0];
  float ang_nxt = STAGED ? (outb + tid * row)[nb > 1 ? 3 : 0] : 0.0f;     // parked joint angle of body 1 (garbage if it has no joint: unused)
  for (int j = 1; j < nb; j++) {
    // wave-uniform tree data: ONE 64-byte scalar load per body, issued one body ahead; so is the parked joint angle
    const FkBodyRec cur = nxt;
    nxt = tree->rec[j + 1 < nb ? j + 1 : j];
    const float ang = ang_nxt;
    if (STAGED) ang_nxt = (outb + tid * row)[3 * (j + 1 < nb ? j + 1 : j)];
    const int src = (int)((cur.meta >> 8) & 255u) - 1, dst = (int)((cur.meta >> 16) & 255u) - 1;
    float ppx = cpx, ppy = cpy, ppz = cpz;
    f4 prot = crot;
    if (src >= 0) {   // wave-uniform: this body is not the first child of the body before it
      if (STAGED) {
        const int pj = (int)(cur.meta >> 24);
        const float* po = outb + tid * row + 3 * pj;
        ppx = po[0]; ppy = po[1]; ppz = po[2];
        const float* par = stk + src * 4 * FK_BLOCK;
        prot = f4{par[0], par[FK_BLOCK], par[2 * FK_BLOCK], par[3 * FK_BLOCK]};
      } else {
        const float* par = stk + src * 7 * FK_BLOCK;
        ppx = par[0]; ppy = par[FK_BLOCK]; ppz = par[2 * FK_BLOCK];
        prot = f4{par[3 * FK_BLOCK], par[4 * FK_BLOCK], par[5 * FK_BLOCK], par[6 * FK_BLOCK]};
      }
    }
    float wx, wy, wz;
    f4 rot;
    fk_body(cur, STAGED ? ang : ((cur.meta & 1u) ? in.ang(cur.dof_idx) : 0.0f), prot, wx, wy, wz, rot);
    float px = ppx + wx, py = ppy + wy, pz = ppz + wz;
    cpx = px; cpy = py; cpz = pz; crot = rot;
    if (dst >= 0 && SW > 0) {
      float* cur = stk + dst * SW * FK_BLOCK;
      if (SW == 7) { cur[0] = px; cur[FK_BLOCK] = py; cur[2 * FK_BLOCK] = pz; cur += 3 * FK_BLOCK; }
      cur[0] = rot.x; cur[FK_BLOCK] = rot.y; cur[2 * FK_BLOCK] = rot.z; cur[3 * FK_BLOCK] = rot.w;
    }
    if (STAGED) {
      float* o = outb + tid * row + 3 * j;
      o[0] = px; o[1] = py; o[2] = pz;
      if (body_rot) *reinterpret_cast<float4*>(outr + tid * rrow + 4 * j) = make_float4(rot.x, rot.y, rot.z, rot.w);   // one 16-B store: 2-way instead of 8-way bank conflicts
      if (on) zmin = fminf(zmin, pz);
    } else if (on) {
      float* op = body_pos + (f * nb + j) * 3;
      op[0] = px; op[1] = py; op[2] = pz;
      if (body_rot) { float* orr = body_rot + (f * nb + j) * 4; orr[0] = rot.x; orr[1] = rot.y; orr[2] = rot.z; orr[3] = rot.w; }
      zmin = fminf(zmin, pz);
    }
  }
  if (STAGED) {
    // the block's output is one contiguous range of body_pos: stream it out 16 B per lane
    __syncthreads();
    const long long f0 = (long long)blockIdx.x * FK_BLOCK;
    const long long nfr = (B - f0) < FK_BLOCK ? (B - f0) : FK_BLOCK;
    const int nfloat = (int)(nfr * row);
    float* gdst = body_pos + f0 * row;
    const int nvec = nfloat >> 2;
    {
      // four independent LDS reads in flight per trip (a read -> wait -> store loop costs a full LDS round trip per 16 B)
      const float4* sv = reinterpret_cast<const float4*>(outb);
      float4* dv = reinterpret_cast<float4*>(gdst);
      int i = tid;
      for (; i + 3 * FK_BLOCK < nvec; i += 4 * FK_BLOCK) {
        const float4 a0 = sv[i], a1 = sv[i + FK_BLOCK], a2 = sv[i + 2 * FK_BLOCK], a3 = sv[i + 3 * FK_BLOCK];
        dv[i] = a0; dv[i + FK_BLOCK] = a1; dv[i + 2 * FK_BLOCK] = a2; dv[i + 3 * FK_BLOCK] = a3;
      }
      for (; i < nvec; i += FK_BLOCK) dv[i] = sv[i];
    }
    for (int i = (nvec << 2) + tid; i < nfloat; i += FK_BLOCK) gdst[i] = outb[i];
    if (body_rot) {
      float4* rdst = reinterpret_cast<float4*>(body_rot + f0 * rrow);
      const int nrv = (int)(nfr * nb);
      const float4* sv = reinterpret_cast<const float4*>(outr);
      int i = tid;
      for (; i + 3 * FK_BLOCK < nrv; i += 4 * FK_BLOCK) {
        const float4 a0 = sv[i], a1 = sv[i + FK_BLOCK], a2 = sv[i + 2 * FK_BLOCK], a3 = sv[i + 3 * FK_BLOCK];
        rdst[i] = a0; rdst[i + FK_BLOCK] = a1; rdst[i + 2 * FK_BLOCK] = a2; rdst[i + 3 * FK_BLOCK] = a3;
      }
      for (; i < nrv; i += FK_BLOCK) rdst[i] = sv[i];
    }
  }
  if (min_part) {
    for (int off = 32; off > 0; off >>= 1) zmin = fminf(zmin, __shfl_xor(zmin, off, 64));
    if ((tid & 63) == 0) red[tid >> 6] = zmin;
    __syncthreads();
    if (tid == 0) {
      float m = red[0];
      for (int i = 1; i < FK_BLOCK / 64; i++) m = fminf(m, red[i]);
      min_part[blockIdx.x] = m;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The split walk: a block is still 64 frames (lane = frame) with its outputs staged in LDS, but up to four wavefronts
// walk it, each its part of the tree (FkTree::wrec): the chain of ancestors its subtrees hang from -- recomputed by
// every wavefront that needs it, a handful of bodies -- and then the subtrees themselves.  The staging area (456 B per
// frame for the G1) limits a CU to five blocks whatever the kernel does; with one wavefront per block that is 1.25
// wavefronts per SIMD walking 38 dependent bodies each (the wave issues 43 % of its cycles, profiles/r02_fk_*); with
// four it is 5 per SIMD walking ~12.  Parents that are not the body walked just before come from per-wavefront slots
// (position and rotation): no wavefront reads what another one wrote before the final barrier.
// ---------------------------------------------------------------------------------------------
template <class Src>
__global__ __launch_bounds__(64 * FK_MAX_WAVES) void fk_split_kernel(const FkTree* __restrict__ tree, int B, const Src src,
                                                                     float* __restrict__ body_pos,
                                                                     float* __restrict__ body_rot,
                                                                     float* __restrict__ min_part) {
  extern __shared__ __align__(16) float fsm[];     // slots [nslot_split][7][64], pos [64][nb*3], rot [64][nb*4]
  __shared__ float red[FK_MAX_WAVES];
  const int nb = tree->nbody, ndof = tree->ndof, nwave = tree->nwave;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), tid = threadIdx.x & 63;
  const long long f = (long long)blockIdx.x * 64 + tid;
  const bool on = f < B;
  const long long fc = on ? f : 0;
  float* stk = fsm + tid;
  const int row = nb * 3, rrow = nb * 4;
  float* outb = fsm + tree->nslot_split * 7 * 64;
  float* outr = outb + 64 * row;
  float* xtra = outr + (body_rot ? 64 * rrow : 0) + tid;      // extra angle columns [k][lane] (FkTree::nextra)
  float* orow = outb + tid * row;
  // (the lane's staging rows as 32-bit indices into fsm: through the generic pointers the per-body address is a 64-bit
  //  multiply-add, a quarter-rate instruction)
  const unsigned orow_i = (unsigned)(tree->nslot_split * 7 * 64) + (unsigned)(tid * row);
  const unsigned rrow_i = (unsigned)(tree->nslot_split * 7 * 64 + 64 * row) + (unsigned)(tid * rrow);
  const typename Src::Lane in = src.lane(fc, ndof);
  const int i0 = tree->wave_start[wave], i1 = tree->wave_start[wave + 1];
  float zmin = INFINITY;
  // Every joint angle this wavefront needs, read from the lane's dof row in ONE batch -- all loads issued back to back,
  // one wait -- and parked in LDS (FkTree::wave_park): the x slot of the body's own position in the lane's staging row, a
  // free y / z slot for an ancestor another wavefront stores, or an extra column.  The frame's root pose travels with the
  // same batch.  (The loop this replaces loaded, waited and stored angle by angle behind two dependent scalar loads
  // each -- the compiler could not batch them -- : a quarter of a block's lifetime was that serial chain.  Measured and
  // not kept: the block's 64 dof rows as ONE coalesced read by all wavefronts, scattered to the parking places, then a
  // barrier -- 0.230 against 0.207 ms: the per-lane loads are not what the block waits for, the extra barrier is felt.)
  float rpx, rpy, rpz;
  f4 rrot;
  in.root(rpx, rpy, rpz, rrot);
  {
    const uint32_t* pk = tree->wave_park[wave];
    for (int c = 0; c < 32; c += 16) {
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 16; k++) w[k] = pk[c + k];
      if (w[0] == 0xffffffffu) break;
      float a[16];
#pragma unroll
      for (int k = 0; k < 16; k++) a[k] = w[k] != 0xffffffffu ? in.ang((int)(w[k] & 0xffffu)) : 0.0f;
#pragma unroll
      for (int k = 0; k < 16; k++)
        if (w[k] != 0xffffffffu) *((w[k] >> 31) ? xtra + 64 * ((w[k] >> 16) & 0x7fffu) : orow + (w[k] >> 16)) = a[k];
    }
  }
  float cpx, cpy, cpz;
  f4 crot;
  float spx = 0.0f, spy = 0.0f, spz = 0.0f;        // the wavefront's first parked parent stays in registers (slot code 254):
  f4 srot = {0.0f, 0.0f, 0.0f, 1.0f};              // for the shipped trees no LDS slot is left, one more block fits a CU
  float ang_nxt = 0.0f;
  {
    const FkBodyRec r0 = tree->wrec[i0];           // body 0 opens every list
    if (r0.next_park >> 31) ang_nxt = *((r0.next_park & 0x40000000u) ? xtra + 64 * (r0.next_park & 0xffffu) : orow + (r0.next_park & 0xffffu));
    const float px = rpx, py = rpy, pz = rpz;
    const f4 rot = rrot;
    cpx = px; cpy = py; cpz = pz; crot = rot;
    const int dst = (int)((r0.meta >> 16) & 255u) - 1;
    if (dst == 254) { spx = px; spy = py; spz = pz; srot = rot; }
    else if (dst >= 0) {
      float* sl = stk + dst * 7 * 64;
      sl[0] = px; sl[64] = py; sl[128] = pz; sl[192] = rot.x; sl[256] = rot.y; sl[320] = rot.z; sl[384] = rot.w;
    }
    if (r0.meta & 16u) {
      orow[0] = px; orow[1] = py; orow[2] = pz;
      if (body_rot) *reinterpret_cast<float4*>(&fsm[rrow_i]) = make_float4(rot.x, rot.y, rot.z, rot.w);
      zmin = pz;                                   // (lanes beyond B walk frame 0 again: the minimum over all frames is the same)
    }
  }
  FkBodyRec nxt = tree->wrec[i0 + 1 < i1 ? i0 + 1 : i0];
#ifdef GMR_FK_EXP_NOWALK
  for (int i = i1; i < i1; i++) {
#else
  for (int i = i0 + 1; i < i1; i++) {
#endif
    const FkBodyRec cur = nxt;                     // one 64-byte scalar load per body, issued one body ahead
    // (the same record through the vector memory path -- a broadcast read straight into vector registers, which is
    //  where the packed FP32 instructions need it -- measured slower: 0.294 vs 0.241 ms)
    nxt = tree->wrec[i + 1 < i1 ? i + 1 : i];
    const int j = (int)(cur.meta >> 24);
    const int src = (int)((cur.meta >> 8) & 255u) - 1, dst = (int)((cur.meta >> 16) & 255u) - 1;
    const bool own = cur.meta & 16u;
    if (cur.meta & 32u) __syncthreads();           // shared trunk: the transforms this wavefront continues from are parked (fk_build_split)
    const float ang = ang_nxt;                     // parked angle of this body, read while the previous body was walked
    if (cur.next_park >> 31) ang_nxt = *((cur.next_park & 0x40000000u) ? xtra + 64 * (cur.next_park & 0xffffu) : orow + (cur.next_park & 0xffffu));
    float ppx = cpx, ppy = cpy, ppz = cpz;
    f4 prot = crot;
    if (src == 254) { ppx = spx; ppy = spy; ppz = spz; prot = srot; }
    else if (src >= 0) {                           // wave-uniform: the parent is not the body walked just before
      const float* par = stk + src * 7 * 64;
      ppx = par[0]; ppy = par[64]; ppz = par[128];
      prot = f4{par[192], par[256], par[320], par[384]};
    }
    float wx, wy, wz;
    f4 rot;
    fk_body(cur, ang, prot, wx, wy, wz, rot);
    const float px = ppx + wx, py = ppy + wy, pz = ppz + wz;
    cpx = px; cpy = py; cpz = pz; crot = rot;
    if (dst == 254) { spx = px; spy = py; spz = pz; srot = rot; }
    else if (dst >= 0) {
      float* sl = stk + dst * 7 * 64;
      sl[0] = px; sl[64] = py; sl[128] = pz; sl[192] = rot.x; sl[256] = rot.y; sl[320] = rot.z; sl[384] = rot.w;
    }
    if (const unsigned xd = (cur.meta >> 6) & 3u) {  // a parent other wavefronts continue from after the barrier
      float* sl = stk + (xd - 1) * 7 * 64;
      sl[0] = px; sl[64] = py; sl[128] = pz; sl[192] = rot.x; sl[256] = rot.y; sl[320] = rot.z; sl[384] = rot.w;
    }
    if (own) {
      const unsigned oi = orow_i + 3u * (unsigned)j;
      fsm[oi] = px; fsm[oi + 1] = py; fsm[oi + 2] = pz;
      if (body_rot) *reinterpret_cast<float4*>(&fsm[rrow_i + 4u * (unsigned)j]) = make_float4(rot.x, rot.y, rot.z, rot.w);   // one 16-B store: 2-way instead of 8-way bank conflicts
      zmin = min1(zmin, pz);
    }
  }
  if (tree->wave_tail_barrier[wave]) __syncthreads();   // (a wavefront whose list ended before the block's mid-walk barrier)
  __syncthreads();
#ifdef GMR_FK_EXP_NOFLUSH
  if (B > 0) { if (zmin == 12345.f) body_pos[0] = outb[threadIdx.x]; return; }
#endif
  // the block's output is one contiguous range of body_pos (and body_rot): all wavefronts stream it out, 16 B per lane
  const int nthr = 64 * nwave, t = threadIdx.x;
  const long long f0 = (long long)blockIdx.x * 64;
  const long long nfr = (B - f0) < 64 ? (B - f0) : 64;
  {
    const int nfloat = (int)(nfr * row), nvec = nfloat >> 2;
    float* gdst = body_pos + f0 * row;
    const float4* sv = reinterpret_cast<const float4*>(outb);
    float4* dv = reinterpret_cast<float4*>(gdst);
    int i = t;
    for (; i + 3 * nthr < nvec; i += 4 * nthr) {
      const float4 a0 = sv[i], a1 = sv[i + nthr], a2 = sv[i + 2 * nthr], a3 = sv[i + 3 * nthr];
      dv[i] = a0; dv[i + nthr] = a1; dv[i + 2 * nthr] = a2; dv[i + 3 * nthr] = a3;
    }
    for (; i < nvec; i += nthr) dv[i] = sv[i];
    for (int e = (nvec << 2) + t; e < nfloat; e += nthr) gdst[e] = outb[e];
  }
  if (body_rot) {
    float4* rdst = reinterpret_cast<float4*>(body_rot + f0 * rrow);
    const int nrv = (int)(nfr * nb);
    const float4* sv = reinterpret_cast<const float4*>(outr);
    int i = t;
    for (; i + 3 * nthr < nrv; i += 4 * nthr) {
      const float4 a0 = sv[i], a1 = sv[i + nthr], a2 = sv[i + 2 * nthr], a3 = sv[i + 3 * nthr];
      rdst[i] = a0; rdst[i + nthr] = a1; rdst[i + 2 * nthr] = a2; rdst[i + 3 * nthr] = a3;
    }
    for (; i < nrv; i += nthr) rdst[i] = sv[i];
  }
  if (min_part) {
    for (int off = 32; off > 0; off >>= 1) zmin = fminf(zmin, __shfl_xor(zmin, off, 64));
    if (tid == 0) red[wave] = zmin;
    __syncthreads();
    if (threadIdx.x == 0) {
      float m = red[0];
      for (int w = 1; w < nwave; w++) m = fminf(m, red[w]);
      min_part[blockIdx.x] = m;
    }
  }
}

__global__ __launch_bounds__(256) void min_reduce_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
  __shared__ float red[4];
  float z = INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) z = fminf(z, part[i]);
  for (int off = 32; off > 0; off >>= 1) z = fminf(z, __shfl_xor(z, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = z;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

// min over the frames [seg_start[g], seg_start[g + 1]) and all bodies of body_pos z: one block per segment (clip).
// The dataset scripts' height adjustment is per clip (smplx_to_robot_dataset.py:118-126); with many clips
// concatenated into one FK launch this is their reduction.  An empty segment yields +inf.
__global__ __launch_bounds__(256) void fk_segment_min_kernel(const float* __restrict__ body_pos, int nbody,
                                                              const int32_t* __restrict__ seg_start, float* __restrict__ seg_min) {
  __shared__ float red[4];
  const long long i0 = (long long)seg_start[blockIdx.x] * nbody, i1 = (long long)seg_start[blockIdx.x + 1] * nbody;
  float z = INFINITY;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) z = fminf(z, body_pos[3 * i + 2]);
  for (int off = 32; off > 0; off >>= 1) z = fminf(z, __shfl_xor(z, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = z;
  __syncthreads();
  if (threadIdx.x == 0) seg_min[blockIdx.x] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

}  // namespace gmr

extern "C" hipError_t gmr_launch_fk_segment_min(const float* d_body_pos, int nbody, const int32_t* d_seg_start, int nseg,
                                                float* d_seg_min, hipStream_t stream) {
  if (nseg <= 0) return hipSuccess;
  hipLaunchKernelGGL(gmr::fk_segment_min_kernel, dim3(nseg), dim3(256), 0, stream, d_body_pos, nbody, d_seg_start, d_seg_min);
  return hipGetLastError();
}

// blocks of a launch over B frames: one wave per 64 frames; also the size of the min-z partials
extern "C" int gmr_fk_blocks(int B) { return (B + gmr::FK_BLOCK - 1) / gmr::FK_BLOCK; }

// > 64 KB of dynamic LDS needs an opt-in per kernel and per DEVICE: done once for every device this process uses
template <class Src>
static hipError_t fk_opt_in_large_lds() {
  static unsigned long long done_mask = 0;       // bit = device ordinal (benign if two threads race: the call is idempotent)
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 64 && ((done_mask >> dev) & 1ull)) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(gmr::fk_batch_kernel<true, Src>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(gmr::fk_split_kernel<Src>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024 - 1024);
  if (e == hipSuccess && dev < 64) __atomic_fetch_or(&done_mask, 1ull << dev, __ATOMIC_RELAXED);
  return e;
}

// the choice of kernel for a tree and a destination, the same for every source of frames
template <class Src>
static hipError_t fk_launch(const gmr::FkTree* d_tree, const gmr::FkTree* h_tree, int B, const Src src, float* d_body_pos,
                            float* d_body_rot, float* d_min_part, float* d_min_z, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  const int nbody = h_tree->nbody, nslot = h_tree->nslot;
  const int blocks = gmr_fk_blocks(B);
  size_t smem = (size_t)nslot * 7 * gmr::FK_BLOCK * sizeof(float);   // direct variant: parked (pos, rot)
  // 16-B aligned destinations: LDS-staged, fully coalesced output
  // (the block strides FK_BLOCK * nbody * 12 B and * 16 B are multiples of 16)
  const size_t stage_bytes = (size_t)gmr::FK_BLOCK * nbody * (d_body_rot ? 7 : 3) * sizeof(float);
  bool staged = (reinterpret_cast<uintptr_t>(d_body_pos) & 15u) == 0 && (reinterpret_cast<uintptr_t>(d_body_rot) & 15u) == 0 &&
                stage_bytes <= 160 * 1024 - 8192;
  if (staged) {
    // staged variant: parent positions are re-read from the staging area; only rotations are parked
    smem = (size_t)nslot * 4 * gmr::FK_BLOCK * sizeof(float) + stage_bytes;
    if (smem > 64 * 1024 && fk_opt_in_large_lds<Src>() != hipSuccess) {   // no opt-in on this device: the direct variant still works
      (void)hipGetLastError();
      staged = false;
      smem = (size_t)nslot * 7 * gmr::FK_BLOCK * sizeof(float);
    }
  }
  // several wavefronts per block when the tree splits (gmr_fk_create) and the slots of the split walk fit beside the staging area
  const size_t smem_split = (size_t)h_tree->nslot_split * 7 * 64 * sizeof(float) + stage_bytes + (size_t)h_tree->nextra * 64 * sizeof(float);
  if (staged && h_tree->nwave > 1 && smem_split <= 160 * 1024 - 8192 && (smem_split <= 64 * 1024 || fk_opt_in_large_lds<Src>() == hipSuccess))
    hipLaunchKernelGGL(gmr::fk_split_kernel<Src>, dim3(blocks), dim3(64 * h_tree->nwave), smem_split, stream, d_tree, B, src,
                       d_body_pos, d_body_rot, d_min_z ? d_min_part : nullptr);
  else if (staged)
    hipLaunchKernelGGL((gmr::fk_batch_kernel<true, Src>), dim3(blocks), dim3(gmr::FK_BLOCK), smem, stream, d_tree, B, src,
                       d_body_pos, d_body_rot, d_min_z ? d_min_part : nullptr);
  else
    hipLaunchKernelGGL((gmr::fk_batch_kernel<false, Src>), dim3(blocks), dim3(gmr::FK_BLOCK), smem, stream, d_tree, B, src,
                       d_body_pos, d_body_rot, d_min_z ? d_min_part : nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (d_min_z) {
    hipLaunchKernelGGL(gmr::min_reduce_kernel, dim3(1), dim3(256), 0, stream, d_min_part, blocks, d_min_z);
    e = hipGetLastError();
  }
  return e;
}

extern "C" hipError_t gmr_launch_fk_batch(const gmr::FkTree* d_tree, const gmr::FkTree* h_tree, int B,
                                          const float* d_root_pos, const float* d_root_rot, const float* d_dof,
                                          float* d_body_pos, float* d_body_rot, float* d_min_part, float* d_min_z,
                                          hipStream_t stream) {
  return fk_launch(d_tree, h_tree, B, gmr::FkSrcF32{d_root_pos, d_root_rot, d_dof}, d_body_pos, d_body_rot, d_min_part, d_min_z,
                   stream);
}

// positions of the B frames whose float64 qpos rows d_row_q[b] points at (gmr_post.hip), with their own root (world != 0)
// or the identity root
extern "C" hipError_t gmr_launch_fk_qpos(const gmr::FkTree* d_tree, const gmr::FkTree* h_tree, int B, const double* const* d_row_q,
                                         int world, float* d_body_pos, hipStream_t stream) {
  if (world) return fk_launch(d_tree, h_tree, B, gmr::FkSrcQpos<true>{d_row_q}, d_body_pos, nullptr, nullptr, nullptr, stream);
  return fk_launch(d_tree, h_tree, B, gmr::FkSrcQpos<false>{d_row_q}, d_body_pos, nullptr, nullptr, nullptr, stream);
}

// ---- the C-ABI of the post-hoc FK (include/gmr_hip.h) -------------------------------------------------------------------------
#define fail gmr_fail
extern "C" {

// checks, build (gmr_fk_tree.h: fk_build_tree, which the CPU tests drive too), upload
int gmr_fk_create(int nbody, const int32_t* parent, const float* local_t, const float* local_r,
                  const int32_t* dof_idx, const double* axis, int ndof, gmr_fk_t** out) {
  if (!out || !parent || !local_t || !local_r || !dof_idx || !axis) return fail(GMR_ERR_ARG, "null argument");
  if (nbody < 1 || nbody > gmr::FK_MAX_BODIES) return fail(GMR_ERR_ARG, "nbody out of range");
  if (ndof < 0) return fail(GMR_ERR_ARG, "ndof negative");
  // (every dof drives one body: FkTree::dof_body has FK_MAX_BODIES entries)
  if (ndof > gmr::FK_MAX_BODIES) return fail(GMR_ERR_ARG, "ndof = %d out of range [0, %d]", ndof, gmr::FK_MAX_BODIES);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GMR_ERR_NO_DEVICE, "no HIP device visible");
  gmr_fk* k = new (std::nothrow) gmr_fk;
  if (!k) return fail(GMR_ERR_ARG, "out of host memory");
  if (const char* why = gmr::fk_build_tree(k->tree, nbody, parent, local_t, local_r, dof_idx, axis, ndof)) {
    delete k;
    return fail(GMR_ERR_ARG, "%s", why);
  }
  hipError_t e;
  if ((e = k->d_tree.reserve(sizeof(gmr::FkTree))) != hipSuccess ||
      (e = hipMemcpy(k->d_tree.data(), &k->tree, sizeof(gmr::FkTree), hipMemcpyHostToDevice)) != hipSuccess) {
    delete k;
    return fail(GMR_ERR_HIP, "gmr_fk_create: %s", hipGetErrorString(e));
  }
  *out = k;
  return GMR_OK;
}

int gmr_fk_destroy(gmr_fk_t* k) {
  delete k;                                // (freeing its blocks waits for the device: nothing of the handle is in flight afterwards)
  return GMR_OK;
}

int gmr_fk_batch_dev(gmr_fk_t* k, int B, const float* d_root_pos, const float* d_root_rot, const float* d_dof,
                     float* d_body_pos, float* d_body_rot, float* d_min_z, void* stream) {
  if (!k) return fail(GMR_ERR_ARG, "null fk handle");
  if (B < 0) return fail(GMR_ERR_ARG, "negative B");
  if (B == 0) return GMR_OK;
  if (!d_root_pos || !d_root_rot || !d_body_pos || (k->tree.ndof > 0 && !d_dof)) return fail(GMR_ERR_ARG, "null device buffer");
  // grows only; not graph-capturable on the first call of a size.  Earlier launches on any stream may still read the old
  // block: freeing it waits for the device.
  if (d_min_z) GMR_HIP_TRY(k->min_part.reserve((size_t)gmr_fk_blocks(B) * sizeof(float)));
  GMR_HIP_TRY(gmr_launch_fk_batch(k->dev(), &k->tree, B, d_root_pos, d_root_rot, d_dof, d_body_pos,
                              d_body_rot, (float*)k->min_part.data(), d_min_z, (hipStream_t)stream));
  return GMR_OK;
}

int gmr_fk_segment_min_z_dev(gmr_fk_t* k, const float* d_body_pos, const int32_t* d_seg_start, int nseg, float* d_seg_min,
                             void* stream) {
  if (!k) return fail(GMR_ERR_ARG, "null fk handle");
  if (nseg < 0) return fail(GMR_ERR_ARG, "negative nseg");
  if (nseg == 0) return GMR_OK;
  if (!d_body_pos || !d_seg_start || !d_seg_min) return fail(GMR_ERR_ARG, "null device buffer");
  GMR_HIP_TRY(gmr_launch_fk_segment_min(d_body_pos, k->tree.nbody, d_seg_start, nseg, d_seg_min, (hipStream_t)stream));
  return GMR_OK;
}

int gmr_fk_batch(gmr_fk_t* k, int B, const float* root_pos, const float* root_rot, const float* dof, float* body_pos,
                 float* body_rot, float* min_z) {
  if (!k) return fail(GMR_ERR_ARG, "null fk handle");
  if (B < 0) return fail(GMR_ERR_ARG, "negative B");
  if (B == 0) return GMR_OK;
  if (!root_pos || !root_rot || !body_pos) return fail(GMR_ERR_ARG, "null host buffer");
  const size_t n = (size_t)B, nb = k->tree.nbody, nd = k->tree.ndof;
  gmr::HostStage st;
  const float *d_rp, *d_rr, *d_dof;
  float *d_bp, *d_br, *d_mz;
  st.in(d_rp, root_pos, n * 12); st.in(d_rr, root_rot, n * 16); st.in(d_dof, dof, n * nd * 4);
  st.out(d_bp, body_pos, n * nb * 12); st.out(d_br, body_rot, n * nb * 16); st.out(d_mz, min_z, 4);
  GMR_STAGE_TRY(st, upload);
  if (int rc = gmr_fk_batch_dev(k, B, d_rp, d_rr, d_dof, d_bp, d_br, d_mz, nullptr)) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

// Many clips in one launch: frames of clip g are rows [seg_start[g], seg_start[g + 1]) of the inputs.
int gmr_fk_batch_segments(gmr_fk_t* k, int B, const float* root_pos, const float* root_rot, const float* dof, int nseg,
                          const int32_t* seg_start, float* body_pos, float* seg_min_z) {
  if (!k) return fail(GMR_ERR_ARG, "null fk handle");
  if (B < 0 || nseg < 0) return fail(GMR_ERR_ARG, "negative B / nseg");
  if (B == 0) { for (int g = 0; g < nseg && seg_min_z; g++) seg_min_z[g] = INFINITY; return GMR_OK; }
  if (!root_pos || !root_rot || (k->tree.ndof > 0 && !dof)) return fail(GMR_ERR_ARG, "null host buffer");
  if (nseg > 0 && (!seg_start || !seg_min_z)) return fail(GMR_ERR_ARG, "null segment buffers");
  for (int g = 0; g < nseg; g++)
    if (seg_start[g] < 0 || seg_start[g] > seg_start[g + 1] || seg_start[g + 1] > B) return fail(GMR_ERR_ARG, "seg_start must ascend within [0, B]");
  const size_t n = (size_t)B, nb = k->tree.nbody, nd = k->tree.ndof;
  gmr::HostStage st;
  const float *d_rp, *d_rr, *d_dof;
  const int32_t* d_ss;
  float *d_bp, *d_sm;
  st.in(d_rp, root_pos, n * 12); st.in(d_rr, root_rot, n * 16); st.in(d_dof, dof, n * nd * 4);
  st.in(d_ss, nseg ? seg_start : nullptr, (size_t)(nseg + 1) * 4);
  if (body_pos) st.out(d_bp, body_pos, n * nb * 12);
  else st.scratch(d_bp, n * nb * 12);      // the segment minima are taken from it all the same
  st.out(d_sm, nseg ? seg_min_z : nullptr, (size_t)nseg * 4);
  GMR_STAGE_TRY(st, upload);
  int rc = gmr_fk_batch_dev(k, B, d_rp, d_rr, d_dof, d_bp, nullptr, nullptr, nullptr);
  if (rc == GMR_OK && nseg) rc = gmr_fk_segment_min_z_dev(k, d_bp, d_ss, nseg, d_sm, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}


}  // extern "C"
