// gmr_body_state.hip -- per-body pose and velocity per (clip, time) query of a motion library: the sampler of gmr_motion.hip and
// the float32 tree walk of gmr_fk.hip joined in one launch, with the library's velocities carried through the tree
// (DESIGN.md section 6j).
//
//   body_state_kernel   64 queries per workgroup of ONE wavefront
//     phase 1  lane = query: the scalars of the query (motion_query) and the 13 root values, which go out as they are;
//              then 16 lanes per query stride over the columns of the two dof rows (contiguous reads, contiguous writes of
//              dof_pos / dof_vel) and park the lerped values in an LDS row per query of odd stride
//     phase 2  lane = query: the walk over the ancestor closure of the selected bodies, parents first, records of FkTree one
//              body ahead (scalar loads), fk_body of gmr_fk_walk.h for the pose and, in the same step,
//                v_b = v_p + w_p x (p_b - p_p)      w_b = w_p + (R_b a_b) dof_vel[dof of b]
//              a body with several children parks (p, q, v, w) = 13 floats per lane in an LDS slot
//     phase 3  every G selected bodies the 13 G floats of each query are staged in LDS rows and leave as runs of G k
//              consecutive floats per query (k = 3, 4, 3, 3), consecutive lanes on consecutive addresses
//
// The selection travels as a kernel argument (BodyStatePlan, built and validated on the host): no caller memory is read for
// it on the device.  The library and the tree are only read: calls on different streams may be in flight together.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "../../include/gmr_hip.h"
#include "gmr_fk_walk.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_motion_sample.h"
#include "gmr_workspace.h"

// one rounding per operation, as in the sampler and in the FK walk whose bits this kernel reproduces
#pragma clang fp contract(off)

namespace gmr {

constexpr int BS_BLOCK = 64;   // queries per workgroup = one wavefront
constexpr int BS_G = 4;        // selected bodies staged between two flushes (LDS: 64 x 13 G floats; G = 4 keeps a G1 workgroup
                               // at 37 KB, four workgroups -- one wavefront per SIMD -- per CU; G = 8 would leave three)
constexpr int BS_PARK = 13;    // floats of a parked parent: position, rotation, velocity, angular velocity
constexpr int BS_SP = BS_G * 3 + 1, BS_SR = BS_G * 4 + 1;   // staging row strides in floats: odd, lane = query writes them

// The walk of one call.  step[i] for i < nwalk, ascending bodies (parents first), body 0 first:
//   [7:0] the body   [15:8] its place 0 .. G - 1 in the staging rows, 255: walked for its descendants only
//   [23:16] n > 0: after this step the n staged bodies leave as output rows [31:24] .. [31:24] + n - 1 of every query
struct BodyStatePlan {
  int32_t nwalk, nsel;
  uint32_t step[FK_MAX_BODIES];
};

struct BodyStateOut {
  float *root_pos, *root_rot, *root_vel, *root_ang_vel, *dof_pos, *dof_vel, *body_pos, *body_rot, *body_vel, *body_ang_vel;
  int32_t* status;
};

// staging rows [64][ST] of the wavefront -> rows [slot0, slot0 + nf) of the nq queries from q0 on, K floats per body: lane e
// of a sweep takes float e of the 64 x (G K) block, so a query's nf K floats are one run of consecutive lanes
template <int K, int ST>
__device__ __forceinline__ void bs_flush(const float* st, float* __restrict__ out, long long q0, int nq, int nsel, int slot0, int nf, int tid) {
  if (!out) return;
  constexpr int RL = BS_G * K;
  const int live = nf * K;
  const size_t qstride = (size_t)nsel * K;
  float* base = out + ((size_t)q0 * nsel + slot0) * K;
  for (int e = tid; e < BS_BLOCK * RL; e += BS_BLOCK) {
    const int row = e / RL, col = e - row * RL;
    if (col < live && row < nq) base[row * qstride + col] = st[row * ST + col];
  }
}

__global__ __launch_bounds__(BS_BLOCK) void body_state_kernel(const MotionArrays A, const FkTree* __restrict__ tree, int N,
                                                              const int32_t* __restrict__ clip, const double* __restrict__ time, int loop,
                                                              const BodyStatePlan P, const BodyStateOut O) {
  // rows [64][rs] (dof_pos | dof_vel of a query, rs odd), slots [nslot][13][64], staging pos [64][SP] rot [64][SR] vel [64][SP]
  // ang [64][SP], query scalars rl rh w0 w1 [64] each
  extern __shared__ __align__(16) float bsm[];
  const int tid = threadIdx.x;
  const int ndof = A.ndof, nsel = P.nsel;
  const int rs = (2 * ndof) | 1;
  float* rows = bsm;
  float* slots = rows + BS_BLOCK * rs;
  float* st_pos = slots + tree->nslot * BS_PARK * BS_BLOCK;
  float* st_rot = st_pos + BS_BLOCK * BS_SP;
  float* st_vel = st_rot + BS_BLOCK * BS_SR;
  float* st_ang = st_vel + BS_BLOCK * BS_SP;
  int* s_rl = reinterpret_cast<int*>(st_ang + BS_BLOCK * BS_SP);
  int* s_rh = s_rl + BS_BLOCK;
  float* s_w0 = reinterpret_cast<float*>(s_rh + BS_BLOCK);
  float* s_w1 = s_w0 + BS_BLOCK;
  const long long q0 = (long long)blockIdx.x * BS_BLOCK;
  const int nq = (int)((N - q0) < BS_BLOCK ? (N - q0) : BS_BLOCK);

  // ---- phase 1, lane = query: scalars and root state ----
  const bool in = tid < nq;
  const long long q = q0 + tid;
  const MotionQuery Q = motion_query(A, in ? clip[q] : -1, in ? time[q] : 0.0, loop);     // (a lane beyond N: a bad query that stores nothing)
  const bool ok = Q.ok;
  s_rl[tid] = ok ? (int)Q.rl : -1;
  s_rh[tid] = (int)Q.rh;
  s_w0[tid] = Q.w0;
  s_w1[tid] = Q.w1;
  float rp[3], rv[3], rw[3], rq[4];
#pragma unroll
  for (int l = 0; l < 3; l++) rp[l] = rv[l] = rw[l] = NAN;
#pragma unroll
  for (int l = 0; l < 4; l++) rq[l] = NAN;
  if (ok) {      // neutralised otherwise: nothing of the library is read
#pragma unroll
    for (int l = 0; l < 3; l++) {
      rp[l] = lerp1(A.root_pos, Q.rl * 3 + l, Q.rh * 3 + l, Q.same, Q.w0, Q.w1);
      rv[l] = lerp1(A.root_vel, Q.rl * 3 + l, Q.rh * 3 + l, Q.same, Q.w0, Q.w1);
      rw[l] = lerp1(A.root_ang_vel, Q.rl * 3 + l, Q.rh * 3 + l, Q.same, Q.w0, Q.w1);
    }
#pragma unroll
    for (int l = 0; l < 4; l++) rq[l] = slerp1(A.root_rot, Q.rl, Q.rh, l, Q.same, Q.w0, Q.w1);
  }
  if (in) {
    if (O.status) O.status[q] = ok ? 0 : 1;
#pragma unroll
    for (int l = 0; l < 3; l++) {
      if (O.root_pos) O.root_pos[q * 3 + l] = rp[l];
      if (O.root_vel) O.root_vel[q * 3 + l] = rv[l];
      if (O.root_ang_vel) O.root_ang_vel[q * 3 + l] = rw[l];
    }
#pragma unroll
    for (int l = 0; l < 4; l++)
      if (O.root_rot) O.root_rot[q * 4 + l] = rq[l];
  }
  __syncthreads();
  // ---- phase 1, 16 lanes per query: the two dof rows -> LDS row of the query (and dof_pos / dof_vel) ----
  {
    const int g = tid / MOTION_GROUP, l = tid & (MOTION_GROUP - 1);
#pragma unroll 2
    for (int qi = g; qi < BS_BLOCK; qi += BS_BLOCK / MOTION_GROUP) {
      const int rl = s_rl[qi];
      const bool qok = rl >= 0, qin = qi < nq;
      const size_t zl = qok ? (size_t)rl : 0, zh = qok ? (size_t)s_rh[qi] : 0;
      const bool same = zl == zh;
      const float w0 = s_w0[qi], w1 = s_w1[qi];
      float* row = rows + qi * rs;
      const size_t o = (size_t)(q0 + qi) * ndof;
      for (int k = l; k < ndof; k += MOTION_GROUP) {
        float a = 0.0f, b = 0.0f;      // (a bad query walks the rest pose; its rows leave as NaN)
        if (qok) {
          a = lerp1(A.dof_pos, zl * ndof + k, zh * ndof + k, same, w0, w1);
          b = lerp1(A.dof_vel, zl * ndof + k, zh * ndof + k, same, w0, w1);
        }
        row[k] = a;
        row[ndof + k] = b;
        if (qin) {
          if (O.dof_pos) O.dof_pos[o + k] = qok ? a : NAN;
          if (O.dof_vel) O.dof_vel[o + k] = qok ? b : NAN;
        }
      }
    }
  }
  __syncthreads();
  if (!O.body_pos && !O.body_rot && !O.body_vel && !O.body_ang_vel) return;

  // ---- phase 2 and 3, lane = query ----
  const float* myrow = rows + tid * rs;
  float* stk = slots + tid;
  float* my_pos = st_pos + tid * BS_SP;
  float* my_rot = st_rot + tid * BS_SR;
  float* my_vel = st_vel + tid * BS_SP;
  float* my_ang = st_ang + tid * BS_SP;
  // the body walked last: the parent of a first child
  float cpx = ok ? rp[0] : 0.0f, cpy = ok ? rp[1] : 0.0f, cpz = ok ? rp[2] : 0.0f;
  f4 crot = ok ? f4{rq[0], rq[1], rq[2], rq[3]} : f4{0.0f, 0.0f, 0.0f, 1.0f};
  float cvx = ok ? rv[0] : 0.0f, cvy = ok ? rv[1] : 0.0f, cvz = ok ? rv[2] : 0.0f;
  float cwx = ok ? rw[0] : 0.0f, cwy = ok ? rw[1] : 0.0f, cwz = ok ? rw[2] : 0.0f;
  const int nwalk = P.nwalk;
  FkBodyRec nxt = tree->rec[0];
  for (int i = 0; i < nwalk; i++) {
    const uint32_t sc = P.step[i];
    const FkBodyRec cur = nxt;                     // one 64-byte scalar load per body, issued one body ahead
    nxt = tree->rec[P.step[i + 1 < nwalk ? i + 1 : i] & 255u];
    const int dst = (int)((cur.meta >> 16) & 255u) - 1;
    if (i > 0) {
      // (the closure holds every ancestor, so "parent = the body before" of the whole tree holds in the shortened walk too, and a
      //  parent with a later child was parked whatever the selection)
      const int src = (int)((cur.meta >> 8) & 255u) - 1;
      float ppx = cpx, ppy = cpy, ppz = cpz, pvx = cvx, pvy = cvy, pvz = cvz, pwx = cwx, pwy = cwy, pwz = cwz;
      f4 prot = crot;
      if (src >= 0) {
        const float* par = stk + src * BS_PARK * BS_BLOCK;
        ppx = par[0]; ppy = par[BS_BLOCK]; ppz = par[2 * BS_BLOCK];
        prot = f4{par[3 * BS_BLOCK], par[4 * BS_BLOCK], par[5 * BS_BLOCK], par[6 * BS_BLOCK]};
        pvx = par[7 * BS_BLOCK]; pvy = par[8 * BS_BLOCK]; pvz = par[9 * BS_BLOCK];
        pwx = par[10 * BS_BLOCK]; pwy = par[11 * BS_BLOCK]; pwz = par[12 * BS_BLOCK];
      }
      const bool hinge = cur.meta & 1u;
      const float ang = hinge ? myrow[cur.dof_idx] : 0.0f;
      float wx, wy, wz;      // R_p t_b = p_b - p_p
      f4 rot;
      fk_body(cur, ang, prot, wx, wy, wz, rot);
      cpx = ppx + wx; cpy = ppy + wy; cpz = ppz + wz;
      crot = rot;
      cvx = pvx + (pwy * wz - pwz * wy);
      cvy = pvy + (pwz * wx - pwx * wz);
      cvz = pvz + (pwx * wy - pwy * wx);
      cwx = pwx; cwy = pwy; cwz = pwz;
      if (hinge) {
        const float rate = myrow[ndof + cur.dof_idx];
        float ax, ay, az;      // R_b a_b; a hinge along +-e_k carries its +-1 in axis[0] (fk_body)
        switch ((cur.meta >> 2) & 3u) {
          case 1: qrot_sparse<6>(rot, (float)cur.axis[0], 0.0f, 0.0f, ax, ay, az); break;
          case 2: qrot_sparse<5>(rot, 0.0f, (float)cur.axis[0], 0.0f, ax, ay, az); break;
          case 3: qrot_sparse<3>(rot, 0.0f, 0.0f, (float)cur.axis[0], ax, ay, az); break;
          default: qrot_xyzw(rot, (float)cur.axis[0], (float)cur.axis[1], (float)cur.axis[2], ax, ay, az); break;
        }
        cwx = pwx + ax * rate; cwy = pwy + ay * rate; cwz = pwz + az * rate;
      }
    }
    if (dst >= 0) {
      float* sl = stk + dst * BS_PARK * BS_BLOCK;
      sl[0] = cpx; sl[BS_BLOCK] = cpy; sl[2 * BS_BLOCK] = cpz;
      sl[3 * BS_BLOCK] = crot.x; sl[4 * BS_BLOCK] = crot.y; sl[5 * BS_BLOCK] = crot.z; sl[6 * BS_BLOCK] = crot.w;
      sl[7 * BS_BLOCK] = cvx; sl[8 * BS_BLOCK] = cvy; sl[9 * BS_BLOCK] = cvz;
      sl[10 * BS_BLOCK] = cwx; sl[11 * BS_BLOCK] = cwy; sl[12 * BS_BLOCK] = cwz;
    }
    const unsigned place = (sc >> 8) & 255u;
    if (place != 255u) {
      const float nan = NAN;
      float* o = my_pos + 3 * place;
      o[0] = ok ? cpx : nan; o[1] = ok ? cpy : nan; o[2] = ok ? cpz : nan;
      o = my_rot + 4 * place;
      o[0] = ok ? crot.x : nan; o[1] = ok ? crot.y : nan; o[2] = ok ? crot.z : nan; o[3] = ok ? crot.w : nan;
      o = my_vel + 3 * place;
      o[0] = ok ? cvx : nan; o[1] = ok ? cvy : nan; o[2] = ok ? cvz : nan;
      o = my_ang + 3 * place;
      o[0] = ok ? cwx : nan; o[1] = ok ? cwy : nan; o[2] = ok ? cwz : nan;
    }
    if (const int nf = (int)((sc >> 16) & 255u)) {
      const int slot0 = (int)(sc >> 24);
      __syncthreads();       // the staging rows are read across lanes
      bs_flush<3, BS_SP>(st_pos, O.body_pos, q0, nq, nsel, slot0, nf, tid);
      bs_flush<4, BS_SR>(st_rot, O.body_rot, q0, nq, nsel, slot0, nf, tid);
      bs_flush<3, BS_SP>(st_vel, O.body_vel, q0, nq, nsel, slot0, nf, tid);
      bs_flush<3, BS_SP>(st_ang, O.body_ang_vel, q0, nq, nsel, slot0, nf, tid);
      __syncthreads();       // ... before the next bodies overwrite them
    }
  }
}

// LDS of one workgroup in bytes (the layout at the top of the kernel)
static size_t body_state_lds(int ndof, int nslot) {
  return sizeof(float) * ((size_t)BS_BLOCK * ((2 * ndof) | 1) + (size_t)nslot * BS_PARK * BS_BLOCK + (size_t)BS_BLOCK * (3 * BS_SP + BS_SR) +
                          4 * BS_BLOCK);
}

// The walk for a selection: the ancestor closure in body order, the selected bodies staged in runs of consecutive output rows
// (at most G; a selection in ascending order gives full runs, any other order is served by shorter ones).
static void body_state_plan(const FkTree& t, const int32_t* sel, int nsel, BodyStatePlan* P) {
  int row_of[FK_MAX_BODIES];
  bool walk[FK_MAX_BODIES] = {false};
  for (int b = 0; b < t.nbody; b++) row_of[b] = -1;
  for (int k = 0; k < nsel; k++) {
    const int b = sel ? sel[k] : k;
    row_of[b] = k;
    for (int a = b; !walk[a]; a = t.parent[a]) { walk[a] = true; if (a == 0) break; }
  }
  walk[0] = true;
  P->nsel = nsel;
  P->nwalk = 0;
  int run_row0 = 0, run_n = 0, run_last = -1;      // the open run: first output row, members, step of its last member
  auto close_run = [&]() {
    if (run_n > 0) P->step[run_last] |= ((uint32_t)run_n << 16) | ((uint32_t)run_row0 << 24);
    run_n = 0;
  };
  for (int b = 0; b < t.nbody; b++) {
    if (!walk[b]) continue;
    const int i = P->nwalk++;
    uint32_t place = 255u;
    if (row_of[b] >= 0) {
      if (run_n == BS_G || (run_n > 0 && row_of[b] != run_row0 + run_n)) close_run();
      if (run_n == 0) run_row0 = row_of[b];
      place = (uint32_t)run_n++;
      run_last = i;
    }
    P->step[i] = (uint32_t)b | (place << 8);
  }
  close_run();
}

}  // namespace gmr

extern "C" {

int gmr_motion_body_state_dev(const gmr_motion_lib_t* lib, gmr_fk_t* fk, int N, const int32_t* d_clip, const double* d_time, int flags,
                              const int32_t* body_sel, int nsel, const gmr_body_state_out_t* out, void* stream) {
  if (!lib) return gmr_fail(GMR_ERR_ARG, "null motion library");
  if (!fk) return gmr_fail(GMR_ERR_ARG, "null fk handle");
  if (!out) return gmr_fail(GMR_ERR_ARG, "null output table");
  if (!lib->filled) return gmr_fail(GMR_ERR_ARG, "the motion library has not been filled");
  if (lib->reference_angvel)
    return gmr_fail(GMR_ERR_ARG, "body state needs a library filled with GMR_MOTION_ANGVEL_WORLD: the root_ang_vel of "
                                 "GMR_MOTION_ANGVEL_REFERENCE is not a physical angular velocity and cannot be carried through the tree");
  const gmr::FkTree& t = fk->tree;
  if (t.ndof != lib->A.ndof) return gmr_fail(GMR_ERR_ARG, "the fk handle has %d dofs, the motion library %d", t.ndof, lib->A.ndof);
  if (flags & ~GMR_MOTION_LOOP) return gmr_fail(GMR_ERR_ARG, "unknown sample flag bits 0x%x", flags);
  if (N < 0 || N > (1 << 26)) return gmr_fail(GMR_ERR_ARG, "N = %d out of range", N);
  if (!body_sel) nsel = t.nbody;
  if (nsel < 1 || nsel > gmr::FK_MAX_BODIES) return gmr_fail(GMR_ERR_ARG, "nsel = %d out of range [1, %d]", nsel, gmr::FK_MAX_BODIES);
  if (body_sel) {
    bool seen[gmr::FK_MAX_BODIES] = {false};
    for (int k = 0; k < nsel; k++) {
      if (body_sel[k] < 0 || body_sel[k] >= t.nbody) return gmr_fail(GMR_ERR_ARG, "body_sel[%d] = %d outside [0, %d)", k, body_sel[k], t.nbody);
      if (seen[body_sel[k]]) return gmr_fail(GMR_ERR_ARG, "body_sel names body %d twice", body_sel[k]);
      seen[body_sel[k]] = true;
    }
  }
  const size_t smem = gmr::body_state_lds(t.ndof, t.nslot);
  if (smem > 64 * 1024) return gmr_fail(GMR_ERR_ARG, "a tree of %d dofs and %d parked bodies needs %zu bytes of LDS per workgroup", t.ndof, t.nslot, smem);
  if (N == 0) return GMR_OK;
  if (!d_clip || !d_time) return gmr_fail(GMR_ERR_ARG, "null clip / time");
  gmr::BodyStatePlan P;
  gmr::body_state_plan(t, body_sel, nsel, &P);
  const gmr::BodyStateOut O{out->root_pos, out->root_rot, out->root_vel, out->root_ang_vel, out->dof_pos, out->dof_vel,
                            out->body_pos, out->body_rot, out->body_vel, out->body_ang_vel, out->status};
  hipLaunchKernelGGL(gmr::body_state_kernel, dim3((N + gmr::BS_BLOCK - 1) / gmr::BS_BLOCK), dim3(gmr::BS_BLOCK), smem, (hipStream_t)stream,
                     lib->A, fk->dev(), N, d_clip, d_time, (flags & GMR_MOTION_LOOP) ? 1 : 0, P, O);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

int gmr_motion_body_state(const gmr_motion_lib_t* lib, gmr_fk_t* fk, int N, const int32_t* clip, const double* time, int flags,
                          const int32_t* body_sel, int nsel, const gmr_body_state_out_t* out) {
  if (!lib) return gmr_fail(GMR_ERR_ARG, "null motion library");
  if (!fk) return gmr_fail(GMR_ERR_ARG, "null fk handle");
  if (!out) return gmr_fail(GMR_ERR_ARG, "null output table");
  if (N < 0 || N > (1 << 26)) return gmr_fail(GMR_ERR_ARG, "N = %d out of range", N);
  if (N > 0 && (!clip || !time)) return gmr_fail(GMR_ERR_ARG, "null clip / time");
  const size_t n = (size_t)N, ndof = (size_t)lib->A.ndof;
  const size_t ns = body_sel ? (size_t)(nsel > 0 ? nsel : 0) : (size_t)fk->tree.nbody;
  gmr::HostStage st;
  const int32_t* d_clip;
  const double* d_time;
  gmr_body_state_out_t dev = {};
  st.in(d_clip, clip, n * 4); st.in(d_time, time, n * 8);
  st.out(dev.root_pos, out->root_pos, n * 12); st.out(dev.root_rot, out->root_rot, n * 16); st.out(dev.root_vel, out->root_vel, n * 12);
  st.out(dev.root_ang_vel, out->root_ang_vel, n * 12); st.out(dev.dof_pos, out->dof_pos, n * ndof * 4);
  st.out(dev.dof_vel, out->dof_vel, n * ndof * 4); st.out(dev.body_pos, out->body_pos, n * ns * 12); st.out(dev.body_rot, out->body_rot, n * ns * 16);
  st.out(dev.body_vel, out->body_vel, n * ns * 12); st.out(dev.body_ang_vel, out->body_ang_vel, n * ns * 12); st.out(dev.status, out->status, n * 4);
  GMR_STAGE_TRY(st, upload);
  const int rc = gmr_motion_body_state_dev(lib, fk, N, d_clip, d_time, flags, body_sel, nsel, &dev, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

}  // extern "C"
