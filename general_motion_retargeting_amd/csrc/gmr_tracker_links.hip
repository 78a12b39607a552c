// gmr_tracker_links.hip -- the link step of the motion tracker: a tracker step (gmr_tracker.hip) that also walks the robot's tree
// for the environment's own (clip, clock), so that per-link targets and whole-body tracking terms leave in the same launch
// (DESIGN.md section 6l).
//
//   tracker_links_kernel   64 environments per workgroup of W wavefronts, W = the wavefronts of the link plan (1 .. 4)
//     phase 1  all W x 64 lanes, 16 lanes per environment: the plain step's work with the plain step's lane layout -- the query,
//              the root rows, the mapped dof rows, the six sums, err / term -- and, for the walk, the library-order
//              dof_pos | dof_vel row of the environment (odd stride) and its 13 root floats parked in LDS; with anchors enabled
//              (gmr_tracker_anchor.hip) the four root rows and their terms are the anchored ones, what is parked is not
//     phase 2  lane = environment: wavefront w walks ITS list of the plan (LinkPlan, gmr_link_plan.h) -- the trunk ancestors its
//              subtrees hang from, recomputed by every wavefront that needs them, then the subtrees: the partition of
//              fk_split_tree restricted to the ancestor closure of the selection -- with fk_body of gmr_fk_walk.h for the pose
//              and the two velocity lines of body_state_kernel.  For a selected body it writes the reference row (REFS), loads
//              the simulator's row through sim_body and the strides, applies the frame (and, in the world frame, the anchor) and
//              keeps five partials in registers:
//              four weighted sums of squares and the largest squared distance
//     phase 3  the W x 5 partials of an environment meet in LDS; wavefront 0 finishes sqrt / exp, total and fail, then advances
//              the clock and redraws a finished clip exactly as lane 0 of the plain kernel does (not with NO_ADVANCE)
//
// No wavefront reads what another one parked before the one barrier in front of phase 3.  The plan, the weights and the term
// constants are kernel arguments; the tracker's state is the only memory of either handle that is written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>

#include "../../include/gmr_hip.h"
#include "gmr_fk_walk.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_motion_sample.h"
#include "gmr_philox.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation, as in the sampler, the FK walk and the plain step whose bits this kernel reproduces
#pragma clang fp contract(off)

namespace gmr {

constexpr int TL_BLOCK = 64;       // environments per workgroup
constexpr int TL_PARK = 13;        // floats of a parked body: position, rotation, velocity, angular velocity
constexpr int TL_PART = 5;         // partials of a wavefront per environment: four weighted sums and the largest squared distance

struct LinkSim {
  const float *body_pos, *body_rot, *body_vel, *body_ang_vel;
  long long env_stride[LINK_TERMS], body_stride[LINK_TERMS];      // per array, in floats
};
struct LinkOut {
  float *ref_body_pos, *ref_body_rot, *ref_body_vel, *ref_body_ang_vel, *link_err, *link_term, *max_dist;
  int32_t* fail;
};

// (the heading frame, yaw_of, unyaw_zw and unyaw_q: gmr_tracker_dev.h)

// LDS of one workgroup in floats: rows [64][rs], root [13][64], slots [nslot][13][64], partials [W][5][64], total6 [64], ok [64]
__host__ __device__ inline size_t links_lds_floats(int ndof, int nslot, int nwave) {
  return (size_t)TL_BLOCK * ((2 * ndof) | 1) + (size_t)TL_PARK * TL_BLOCK + (size_t)nslot * TL_PARK * TL_BLOCK +
         (size_t)nwave * TL_PART * TL_BLOCK + 2 * TL_BLOCK;
}

// REFS: ref_body_* rows are written (the training-only variant carries neither their stores nor their frame arithmetic twice)
template <bool REFS>
__global__ __launch_bounds__(64 * FK_MAX_WAVES) void tracker_links_kernel(const MotionArrays A, const FkTree* __restrict__ tree,
                                                                          const TrackerState S, const TrackerTables Tb, const LinkPlan P, int N,
                                                                          int loop, int advance, float dtf, uint32_t key0, uint32_t key1,
                                                                          const TrackerSim X, const LinkSim Y, const TrackerOut O,
                                                                          const LinkOut L) {
  __shared__ int s_map[TRACKER_MAX_DOF];
  __shared__ float s_def[TRACKER_MAX_DOF], s_w[TRACKER_MAX_DOF];
  extern __shared__ __align__(16) float tlm[];
  const int ndof = A.ndof, R = Tb.R, nwave = P.nwave;
  const int rs = (2 * ndof) | 1;
  float* rows = tlm;
  float* s_root = rows + TL_BLOCK * rs;
  float* slots = s_root + TL_PARK * TL_BLOCK;
  float* part = slots + P.nslot * TL_PARK * TL_BLOCK;
  float* s_total = part + nwave * TL_PART * TL_BLOCK;
  int* s_ok = reinterpret_cast<int*>(s_total + TL_BLOCK);
  if (threadIdx.x < TRACKER_MAX_DOF) {      // (the staging of the plain kernel)
    s_map[threadIdx.x] = Tb.map[threadIdx.x];
    s_def[threadIdx.x] = Tb.dof_default[threadIdx.x];
    s_w[threadIdx.x] = Tb.dof_weight[threadIdx.x];
  }
  __syncthreads();
  const long long q0 = (long long)blockIdx.x * TL_BLOCK;
  const bool terms = O.err || O.term || O.total;
  const bool anchored = S.anchor_pos != nullptr;      // tracker anchors: the same in every lane of the launch

  // ---- phase 1: 16 lanes per environment, the plain step ----
  {
    const int l = threadIdx.x & (MOTION_GROUP - 1);
    const int ngroup = (int)blockDim.x / MOTION_GROUP;
    for (int qi = (int)threadIdx.x / MOTION_GROUP; qi < TL_BLOCK; qi += ngroup) {
      const long long e = q0 + qi;
      float* row = rows + qi * rs;
      const bool in = e < N;
      MotionQuery Q;
      Q.ok = false;
      if (in) Q = motion_query(A, S.clip[e], (double)S.time[e], loop);
      if (!Q.ok) {
        // neutralised (or beyond N): nothing of the library is read, the walk gets the rest pose and its rows leave as NaN
        for (int k = l; k < 2 * ndof; k += MOTION_GROUP) row[k] = 0.0f;
        if (l < TL_PARK) s_root[l * TL_BLOCK + qi] = l == 6 ? 1.0f : 0.0f;
        if (l == 0) { s_ok[qi] = 0; s_total[qi] = NAN; }
        if (!in) continue;
        const float nan = NAN;
        if (l < 3) {
          if (O.ref_root_pos) O.ref_root_pos[(size_t)e * 3 + l] = nan;
          if (O.ref_root_vel) O.ref_root_vel[(size_t)e * 3 + l] = nan;
          if (O.ref_root_ang_vel) O.ref_root_ang_vel[(size_t)e * 3 + l] = nan;
        }
        if (l < 4 && O.ref_root_rot) O.ref_root_rot[(size_t)e * 4 + l] = nan;
        for (int j = l; j < R; j += MOTION_GROUP) {
          if (O.ref_dof_pos) O.ref_dof_pos[(size_t)e * R + j] = nan;
          if (O.ref_dof_vel) O.ref_dof_vel[(size_t)e * R + j] = nan;
        }
        if (l < TRACKER_TERMS) {
          if (O.err) O.err[(size_t)e * TRACKER_TERMS + l] = nan;
          if (O.term) O.term[(size_t)e * TRACKER_TERMS + l] = nan;
        }
        continue;
      }
      const bool same = Q.same;
      const size_t rl = Q.rl, rh = Q.rh;
      const float w0 = Q.w0, w1 = Q.w1;
      float acc[TRACKER_TERMS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      Anchor An;
      float at = 0.0f;
      if (anchored) {      // (the plain step's lines; the walk is parked the root as the library has it)
        anchor_turn(S, (size_t)e, An);
        if (l < 3) at = S.anchor_pos[(size_t)e * 3 + l];
      }
      if (l < 3) {
        float p = lerp1(A.root_pos, rl * 3 + l, rh * 3 + l, same, w0, w1);
        float v = lerp1(A.root_vel, rl * 3 + l, rh * 3 + l, same, w0, w1);
        float w = lerp1(A.root_ang_vel, rl * 3 + l, rh * 3 + l, same, w0, w1);
        s_root[l * TL_BLOCK + qi] = p;
        s_root[(7 + l) * TL_BLOCK + qi] = v;
        s_root[(10 + l) * TL_BLOCK + qi] = w;
        if (anchored) {
          p = anchor_point_lane(An, l, p, at);
          v = anchor_vector_lane(An, l, v);
          w = anchor_vector_lane(An, l, w);
        }
        if (O.ref_root_pos) O.ref_root_pos[(size_t)e * 3 + l] = p;
        if (O.ref_root_vel) O.ref_root_vel[(size_t)e * 3 + l] = v;
        if (O.ref_root_ang_vel) O.ref_root_ang_vel[(size_t)e * 3 + l] = w;
        if (terms) {
          if (X.base_pos) { const float d = X.base_pos[(size_t)e * 3 + l] - p; acc[0] = d * d; }
          if (X.base_lin_vel) { const float d = X.base_lin_vel[(size_t)e * 3 + l] - v; acc[2] = d * d; }
          if (X.base_ang_vel) { const float d = X.base_ang_vel[(size_t)e * 3 + l] - w; acc[3] = d * d; }
        }
      }
      if (l < 4) {
        float q = slerp1(A.root_rot, rl, rh, l, same, w0, w1);
        s_root[(3 + l) * TL_BLOCK + qi] = q;
        if (anchored) q = anchor_quat_lane(An, l, q);
        if (O.ref_root_rot) O.ref_root_rot[(size_t)e * 4 + l] = q;
        if (terms && X.base_quat) acc[1] = X.base_quat[(size_t)e * 4 + l] * q;
      }
      for (int k = l; k < ndof; k += MOTION_GROUP) {      // the library's own columns: what the walk reads (the dof_map does not enter)
        row[k] = lerp1(A.dof_pos, rl * ndof + k, rh * ndof + k, same, w0, w1);
        row[ndof + k] = lerp1(A.dof_vel, rl * ndof + k, rh * ndof + k, same, w0, w1);
      }
      for (int j = l; j < R; j += MOTION_GROUP) {
        const int m = s_map[j];
        float p = s_def[j], v = 0.0f;
        if (m >= 0) {
          p = lerp1(A.dof_pos, rl * ndof + m, rh * ndof + m, same, w0, w1);
          v = lerp1(A.dof_vel, rl * ndof + m, rh * ndof + m, same, w0, w1);
        }
        if (O.ref_dof_pos) O.ref_dof_pos[(size_t)e * R + j] = p;
        if (O.ref_dof_vel) O.ref_dof_vel[(size_t)e * R + j] = v;
        if (terms) {
          if (X.dof_pos) { const float d = s_w[j] * (X.dof_pos[(size_t)e * R + j] - p); acc[4] = acc[4] + d * d; }
          if (X.dof_vel) { const float d = s_w[j] * (X.dof_vel[(size_t)e * R + j] - v); acc[5] = acc[5] + d * d; }
        }
      }
      float total = 0.0f;
      if (terms) {
#pragma unroll
        for (int k = 0; k < TRACKER_TERMS; k++) acc[k] = group_sum(acc[k]);
        if (l == 0) {
          const bool given[TRACKER_TERMS] = {X.base_pos != nullptr, X.base_quat != nullptr, X.base_lin_vel != nullptr,
                                             X.base_ang_vel != nullptr, X.dof_pos != nullptr, X.dof_vel != nullptr};
#pragma unroll
          for (int k = 0; k < TRACKER_TERMS; k++) {
            float err = 0.0f, term = 0.0f;
            if (given[k]) {
              if (k == 1) {
                float a = fabsf(acc[1]);
                a = a > 1.0f ? 1.0f : a;
                err = 2.0f * acosf(a);
              } else {
                err = __fsqrt_rn(acc[k]);
              }
              term = expf(-__fdiv_rn(err, Tb.scale[k]));
              if (Tb.weight[k] != 0.0f) total = total + Tb.weight[k] * term;
            }
            if (O.err) O.err[(size_t)e * TRACKER_TERMS + k] = err;
            if (O.term) O.term[(size_t)e * TRACKER_TERMS + k] = term;
          }
        }
      }
      if (l == 0) { s_ok[qi] = 1; s_total[qi] = total; }
    }
  }
  __syncthreads();

  // ---- phase 2: lane = environment, wavefront w walks its list ----
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), tid = (int)threadIdx.x & 63;
  const long long e = q0 + tid;
  const bool in = e < N;
  const bool ok = s_ok[tid] != 0;
  const bool heading = P.frame == GMR_TRACKER_FRAME_HEADING;
  const bool have_sim = Y.body_pos || Y.body_rot || Y.body_vel || Y.body_ang_vel;
  float a_pos = 0.0f, a_rot = 0.0f, a_vel = 0.0f, a_ang = 0.0f, d2max = 0.0f;
  const int i0 = P.wave_start[wave], i1 = P.wave_start[wave + 1];
  if (i1 > i0) {
    const float* myrow = rows + tid * rs;
    float* stk = slots + tid;
    const float* rt = s_root + tid;
    const float rpx = rt[0], rpy = rt[TL_BLOCK], rpz = rt[2 * TL_BLOCK];
    float cpx = rpx, cpy = rpy, cpz = rpz;
    f4 crot = f4{rt[3 * TL_BLOCK], rt[4 * TL_BLOCK], rt[5 * TL_BLOCK], rt[6 * TL_BLOCK]};
    float cvx = rt[7 * TL_BLOCK], cvy = rt[8 * TL_BLOCK], cvz = rt[9 * TL_BLOCK];
    float cwx = rt[10 * TL_BLOCK], cwy = rt[11 * TL_BLOCK], cwz = rt[12 * TL_BLOCK];
    // the two yaws of the heading frame: the sampled root's and the simulator's
    float ryz = 0.0f, ryw = 1.0f, syz = 0.0f, syw = 1.0f, sbx = 0.0f, sby = 0.0f, sbz = 0.0f;
    if (heading) {
      yaw_of(crot.z, crot.w, ryz, ryw);
      if (have_sim && in) {      // (base_pos / base_quat are mandatory here: checked on the host)
        sbx = X.base_pos[(size_t)e * 3]; sby = X.base_pos[(size_t)e * 3 + 1]; sbz = X.base_pos[(size_t)e * 3 + 2];
        yaw_of(X.base_quat[(size_t)e * 4 + 2], X.base_quat[(size_t)e * 4 + 3], syz, syw);
      }
    }
    // the world frame moves with the environment's anchor; the heading frame removes every common x / y / yaw, the anchor's too
    // (its five floats are loaded where a selected body is finished, not carried through the walk: the walk has no registers to spare)
    const bool move = anchored && !heading && in;
    FkBodyRec nxt = tree->rec[P.step[i0] & 255u];
    for (int i = i0; i < i1; i++) {
      const uint32_t sc = P.step[i];
      const FkBodyRec cur = nxt;                   // one 64-byte scalar load per body, issued one body ahead
      nxt = tree->rec[P.step[i + 1 < i1 ? i + 1 : i] & 255u];
      if (i > i0) {                                // (body 0 opens every list)
        const int src = (int)((sc >> 16) & 255u) - 1;
        float ppx = cpx, ppy = cpy, ppz = cpz, pvx = cvx, pvy = cvy, pvz = cvz, pwx = cwx, pwy = cwy, pwz = cwz;
        f4 prot = crot;
        if (src >= 0) {
          const float* par = stk + src * TL_PARK * TL_BLOCK;
          ppx = par[0]; ppy = par[TL_BLOCK]; ppz = par[2 * TL_BLOCK];
          prot = f4{par[3 * TL_BLOCK], par[4 * TL_BLOCK], par[5 * TL_BLOCK], par[6 * TL_BLOCK]};
          pvx = par[7 * TL_BLOCK]; pvy = par[8 * TL_BLOCK]; pvz = par[9 * TL_BLOCK];
          pwx = par[10 * TL_BLOCK]; pwy = par[11 * TL_BLOCK]; pwz = par[12 * TL_BLOCK];
        }
        const bool hinge = cur.meta & 1u;
        const float ang = hinge ? myrow[cur.dof_idx] : 0.0f;
        float wx, wy, wz;      // R_p t_b = p_b - p_p
        f4 rot;
        fk_body(cur, ang, prot, wx, wy, wz, rot);
        // (the velocity lines of body_state_kernel, in its order)
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
      const int dst = (int)(sc >> 24) - 1;
      if (dst >= 0) {
        float* sl = stk + dst * TL_PARK * TL_BLOCK;
        sl[0] = cpx; sl[TL_BLOCK] = cpy; sl[2 * TL_BLOCK] = cpz;
        sl[3 * TL_BLOCK] = crot.x; sl[4 * TL_BLOCK] = crot.y; sl[5 * TL_BLOCK] = crot.z; sl[6 * TL_BLOCK] = crot.w;
        sl[7 * TL_BLOCK] = cvx; sl[8 * TL_BLOCK] = cvy; sl[9 * TL_BLOCK] = cvz;
        sl[10 * TL_BLOCK] = cwx; sl[11 * TL_BLOCK] = cwy; sl[12 * TL_BLOCK] = cwz;
      }
      const int row_s = (int)((sc >> 8) & 255u);
      if (row_s == 255) continue;
      // ---- a selected body this wavefront serves: the reference row in the frame ----
      float px = cpx, py = cpy, pz = cpz, vx = cvx, vy = cvy, vz = cvz, ox = cwx, oy = cwy, oz = cwz;
      f4 q = crot;
      if (heading) {
        px = px - rpx; py = py - rpy; pz = pz - rpz;
        unyaw_zw(ryz, ryw, px, py);
        q = unyaw_q(ryz, ryw, q);
        unyaw_zw(ryz, ryw, vx, vy);
        unyaw_zw(ryz, ryw, ox, oy);
      }
      if (move) {      // the finished world row, after the walk and before it is written and differenced
        const Anchor An = anchor_load(S, (size_t)e);
        anchor_point(An, px, py, pz);
        anchor_quat(An, q.x, q.y, q.z, q.w);
        anchor_vector(An, vx, vy);
        anchor_vector(An, ox, oy);
      }
      if (REFS && in) {
        const float nan = NAN;
        const size_t o = (size_t)e * P.nsel + row_s;
        if (L.ref_body_pos) { float* d = L.ref_body_pos + o * 3; d[0] = ok ? px : nan; d[1] = ok ? py : nan; d[2] = ok ? pz : nan; }
        if (L.ref_body_rot) { float* d = L.ref_body_rot + o * 4; d[0] = ok ? q.x : nan; d[1] = ok ? q.y : nan; d[2] = ok ? q.z : nan; d[3] = ok ? q.w : nan; }
        if (L.ref_body_vel) { float* d = L.ref_body_vel + o * 3; d[0] = ok ? vx : nan; d[1] = ok ? vy : nan; d[2] = ok ? vz : nan; }
        if (L.ref_body_ang_vel) { float* d = L.ref_body_ang_vel + o * 3; d[0] = ok ? ox : nan; d[1] = ok ? oy : nan; d[2] = ok ? oz : nan; }
      }
      const float wb = P.weight[row_s];
      if (!have_sim || !(wb > 0.0f) || !in) continue;      // (a link of weight zero is not read)
      const long long sb = P.sim_body[row_s];
      if (Y.body_pos) {
        const float* s = Y.body_pos + e * Y.env_stride[0] + sb * Y.body_stride[0];
        float x = s[0], y = s[1], z = s[2];
        if (heading) { x = x - sbx; y = y - sby; z = z - sbz; unyaw_zw(syz, syw, x, y); }
        const float dx = x - px, dy = y - py, dz = z - pz;
        const float d2 = dx * dx + dy * dy + dz * dz;
        a_pos = a_pos + wb * d2;
        d2max = (d2 > d2max || d2 != d2) ? d2 : d2max;      // a NaN enters and stays
      }
      if (Y.body_rot) {
        const float* s = Y.body_rot + e * Y.env_stride[1] + sb * Y.body_stride[1];
        f4 sq = f4{s[0], s[1], s[2], s[3]};
        if (heading) sq = unyaw_q(syz, syw, sq);
        float a = fabsf(sq.x * q.x + sq.y * q.y + sq.z * q.z + sq.w * q.w);
        a = a > 1.0f ? 1.0f : a;                   // (a NaN stays one)
        const float th = 2.0f * acosf(a);
        a_rot = a_rot + wb * (th * th);
      }
      if (Y.body_vel) {
        const float* s = Y.body_vel + e * Y.env_stride[2] + sb * Y.body_stride[2];
        float x = s[0], y = s[1];
        if (heading) unyaw_zw(syz, syw, x, y);
        const float dx = x - vx, dy = y - vy, dz = s[2] - vz;
        a_vel = a_vel + wb * (dx * dx + dy * dy + dz * dz);
      }
      if (Y.body_ang_vel) {
        const float* s = Y.body_ang_vel + e * Y.env_stride[3] + sb * Y.body_stride[3];
        float x = s[0], y = s[1];
        if (heading) unyaw_zw(syz, syw, x, y);
        const float dx = x - ox, dy = y - oy, dz = s[2] - oz;
        a_ang = a_ang + wb * (dx * dx + dy * dy + dz * dz);
      }
    }
  }
  {
    float* mine = part + wave * TL_PART * TL_BLOCK + tid;
    mine[0] = a_pos; mine[TL_BLOCK] = a_rot; mine[2 * TL_BLOCK] = a_vel; mine[3 * TL_BLOCK] = a_ang; mine[4 * TL_BLOCK] = d2max;
  }
  __syncthreads();

  // ---- phase 3: wavefront 0, lane = environment ----
  if (wave != 0 || !in) return;
  if (!ok) {
    const float nan = NAN;
    if (L.link_err || L.link_term) {
#pragma unroll
      for (int k = 0; k < LINK_TERMS; k++) {
        if (L.link_err) L.link_err[(size_t)e * LINK_TERMS + k] = nan;
        if (L.link_term) L.link_term[(size_t)e * LINK_TERMS + k] = nan;
      }
    }
    if (L.max_dist) L.max_dist[e] = nan;
    if (L.fail) L.fail[e] = 0;
    if (O.total) O.total[e] = nan;
    if (O.status) O.status[e] = 1;
    if (O.finished) O.finished[e] = 0;
    return;
  }
  if (have_sim || O.total) {
    float acc[LINK_TERMS] = {0.0f, 0.0f, 0.0f, 0.0f};
    float mx = 0.0f;
    for (int w = 0; w < nwave; w++) {             // in the order of the wavefronts
      const float* p = part + w * TL_PART * TL_BLOCK + tid;
#pragma unroll
      for (int k = 0; k < LINK_TERMS; k++) acc[k] = acc[k] + p[k * TL_BLOCK];
      const float d2 = p[4 * TL_BLOCK];
      mx = (d2 > mx || d2 != d2) ? d2 : mx;
    }
    const bool given[LINK_TERMS] = {Y.body_pos != nullptr, Y.body_rot != nullptr, Y.body_vel != nullptr, Y.body_ang_vel != nullptr};
    float total = s_total[tid];
#pragma unroll
    for (int k = 0; k < LINK_TERMS; k++) {
      float err = 0.0f, term = 0.0f;
      if (given[k]) {
        err = __fsqrt_rn(__fdiv_rn(acc[k], P.wsum));
        term = expf(-__fdiv_rn(err, P.scale[k]));
        if (P.term_weight[k] != 0.0f) total = total + P.term_weight[k] * term;
      }
      if (L.link_err) L.link_err[(size_t)e * LINK_TERMS + k] = err;
      if (L.link_term) L.link_term[(size_t)e * LINK_TERMS + k] = term;
    }
    const float md = __fsqrt_rn(mx);
    if (L.max_dist) L.max_dist[e] = md;
    if (L.fail) L.fail[e] = (md <= P.fail_dist) ? 0 : 1;
    if (O.total) O.total[e] = total;
  }
  int finished = 0;
  if (advance) {      // the clock and the redraw of the plain kernel's lane 0
    const int c = S.clip[e];
    float tn = S.time[e] + dtf;
    if (!loop && tn >= S.length[e]) {
      int nc = c;
      tn = tracker_redraw(A, S, key0, key1, (int)e, &nc);
      S.clip[e] = nc;
      S.length[e] = clip_length(A, nc);
      finished = 1;
    }
    S.time[e] = tn;
  }
  if (O.status) O.status[e] = 0;
  if (O.finished) O.finished[e] = finished;
}

// what the two step entry points share once the plan is in hand; every argument check of a link step
static int links_step_launch(gmr_motion_tracker* t, const TrackerState& S, const TrackerTables& T, const LinkPlan& P, const gmr_fk* fk, const gmr_tracker_sim_t* sim,
                             const gmr_tracker_links_sim_t* lsim, const gmr_tracker_out_t* out, const gmr_tracker_links_out_t* lout, int flags,
                             hipStream_t stream) {
  if (flags & ~GMR_TRACKER_NO_ADVANCE) return gmr_fail(GMR_ERR_ARG, "unknown link step flag bits 0x%x", flags);
  const gmr_tracker_out_t none_out = {};
  const gmr_tracker_links_out_t none_lout = {};
  if (!out) out = &none_out;
  if (!lout) lout = &none_lout;
  const bool want_ref = lout->ref_body_pos || lout->ref_body_rot || lout->ref_body_vel || lout->ref_body_ang_vel;
  const bool want_err = lout->link_err || lout->link_term || lout->max_dist || lout->fail;
  if (P.nsel == 0) {
    if (want_ref || want_err) return gmr_fail(GMR_ERR_ARG, "the tracker has no links attached (gmr_motion_tracker_set_links)");
    lsim = nullptr;
  }
  const bool links_given = lsim && (lsim->body_pos || lsim->body_rot || lsim->body_vel || lsim->body_ang_vel);
  if (!sim && (out->err || out->term)) return gmr_fail(GMR_ERR_ARG, "err / term need the simulator's state");
  if (!sim && !links_given && out->total) return gmr_fail(GMR_ERR_ARG, "total needs the simulator's state or its links");
  if (want_err && !links_given) return gmr_fail(GMR_ERR_ARG, "link_err / link_term / max_dist / fail need the simulator's links");
  LinkSim Y = {};
  if (links_given) {
    if (P.frame == GMR_TRACKER_FRAME_HEADING && (!sim || !sim->base_pos || !sim->base_quat))
      return gmr_fail(GMR_ERR_ARG, "the heading frame needs base_pos and base_quat of the simulator's root");
    const long long es = lsim->env_stride, bs = lsim->body_stride;
    if ((es == 0) != (bs == 0) || es < 0 || bs < 0)
      return gmr_fail(GMR_ERR_ARG, "env_stride = %lld, body_stride = %lld: both positive, or both 0 for four contiguous arrays", es, bs);
    Y.body_pos = lsim->body_pos; Y.body_rot = lsim->body_rot; Y.body_vel = lsim->body_vel; Y.body_ang_vel = lsim->body_ang_vel;
    const int width[LINK_TERMS] = {3, 4, 3, 3};
    for (int k = 0; k < LINK_TERMS; k++) {
      Y.env_stride[k] = es ? es : (long long)P.nsel * width[k];
      Y.body_stride[k] = es ? bs : width[k];
    }
  }
  const TrackerSim X = sim ? TrackerSim{sim->base_pos, sim->base_quat, sim->base_lin_vel, sim->base_ang_vel, sim->dof_pos, sim->dof_vel}
                           : TrackerSim{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const TrackerOut O{out->ref_root_pos, out->ref_root_rot, out->ref_root_vel, out->ref_root_ang_vel, out->ref_dof_pos, out->ref_dof_vel,
                     out->err, out->term, out->total, out->status, out->finished};
  const LinkOut L{lout->ref_body_pos, lout->ref_body_rot, lout->ref_body_vel, lout->ref_body_ang_vel,
                  lout->link_err, lout->link_term, lout->max_dist, lout->fail};
  LinkPlan Pw = P;
  if (!want_ref && !links_given) {      // nothing of the links is asked for: an empty walk, the plain step's cost
    Pw.nwave = 1; Pw.nslot = 0;
    for (int w = 0; w <= FK_MAX_WAVES; w++) Pw.wave_start[w] = 0;
  }
  const size_t smem = sizeof(float) * links_lds_floats(t->lib->A.ndof, Pw.nslot, Pw.nwave);
  if (smem > 64 * 1024) return gmr_fail(GMR_ERR_ARG, "a link step of %d dofs and %d parked bodies needs %zu bytes of LDS per workgroup", t->lib->A.ndof, Pw.nslot, smem);
  const dim3 grid((unsigned)((t->N + TL_BLOCK - 1) / TL_BLOCK)), block((unsigned)(64 * Pw.nwave));
  const FkTree* tree = fk ? fk->dev() : nullptr;
  const int advance = (flags & GMR_TRACKER_NO_ADVANCE) ? 0 : 1;
  if (want_ref)
    hipLaunchKernelGGL(tracker_links_kernel<true>, grid, block, smem, stream, t->lib->A, tree, S, T, Pw, t->N, t->loop, advance, t->dtf,
                       t->key[0], t->key[1], X, Y, O, L);
  else
    hipLaunchKernelGGL(tracker_links_kernel<false>, grid, block, smem, stream, t->lib->A, tree, S, T, Pw, t->N, t->loop, advance, t->dtf,
                       t->key[0], t->key[1], X, Y, O, L);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker links") -----------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_links(gmr_motion_tracker_t* t, gmr_fk_t* fk, const int32_t* body_sel, int nsel, const int32_t* sim_body,
                                 const float* link_weight, int frame) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (nsel == 0) {
    std::lock_guard<std::mutex> g(t->mu);
    t->links.nsel = 0; t->links.nwave = 1; t->links.nslot = 0;
    for (int w = 0; w <= gmr::FK_MAX_WAVES; w++) t->links.wave_start[w] = 0;
    t->fk = nullptr;
    return GMR_OK;
  }
  if (!fk) return gmr_fail(GMR_ERR_ARG, "null fk handle");
  if (t->lib->reference_angvel)
    return gmr_fail(GMR_ERR_ARG, "body state needs a library filled with GMR_MOTION_ANGVEL_WORLD: the root_ang_vel of "
                                 "GMR_MOTION_ANGVEL_REFERENCE is not a physical angular velocity and cannot be carried through the tree");
  const gmr::FkTree& tr = fk->tree;
  if (tr.ndof != t->lib->A.ndof) return gmr_fail(GMR_ERR_ARG, "the fk handle has %d dofs, the motion library %d", tr.ndof, t->lib->A.ndof);
  if (frame != GMR_TRACKER_FRAME_WORLD && frame != GMR_TRACKER_FRAME_HEADING) return gmr_fail(GMR_ERR_ARG, "unknown frame %d", frame);
  if (!body_sel && nsel != tr.nbody) return gmr_fail(GMR_ERR_ARG, "without body_sel every body is selected: nsel = %d, the tree has %d", nsel, tr.nbody);
  if (nsel < 1 || nsel > gmr::FK_MAX_BODIES) return gmr_fail(GMR_ERR_ARG, "nsel = %d out of range [1, %d]", nsel, gmr::FK_MAX_BODIES);
  bool seen[gmr::FK_MAX_BODIES] = {false};
  float wsum = 0.0f;
  for (int k = 0; k < nsel; k++) {
    if (body_sel) {
      if (body_sel[k] < 0 || body_sel[k] >= tr.nbody) return gmr_fail(GMR_ERR_ARG, "body_sel[%d] = %d outside [0, %d)", k, body_sel[k], tr.nbody);
      if (seen[body_sel[k]]) return gmr_fail(GMR_ERR_ARG, "body_sel names body %d twice", body_sel[k]);
      seen[body_sel[k]] = true;
    }
    if (sim_body && (sim_body[k] < 0 || sim_body[k] >= (1 << 16))) return gmr_fail(GMR_ERR_ARG, "sim_body[%d] = %d outside [0, 65536)", k, sim_body[k]);
    if (link_weight && (!(link_weight[k] >= 0.0f) || !std::isfinite(link_weight[k])))
      return gmr_fail(GMR_ERR_ARG, "link_weight[%d] = %g, must be finite and not negative", k, (double)link_weight[k]);
    wsum = wsum + (link_weight ? link_weight[k] : 1.0f);
  }
  if (!(wsum > 0.0f) || !std::isfinite(wsum)) return gmr_fail(GMR_ERR_ARG, "the link weights sum to %g", (double)wsum);
  std::lock_guard<std::mutex> g(t->mu);
  gmr::LinkPlan P = t->links;      // (the term constants stay)
  if (const char* why = gmr::link_plan(tr.nbody, tr.parent, body_sel, nsel, &P)) return gmr_fail(GMR_ERR_ARG, "%s (%d bodies)", why, tr.nbody);
  const size_t smem = sizeof(float) * gmr::links_lds_floats(tr.ndof, P.nslot, P.nwave);
  if (smem > 64 * 1024) return gmr_fail(GMR_ERR_ARG, "a link step of %d dofs and %d parked bodies needs %zu bytes of LDS per workgroup", tr.ndof, P.nslot, smem);
  for (int k = 0; k < gmr::FK_MAX_BODIES; k++) {
    P.sim_body[k] = k < nsel ? (sim_body ? sim_body[k] : k) : 0;
    P.weight[k] = k < nsel ? (link_weight ? link_weight[k] : 1.0f) : 0.0f;
  }
  P.wsum = wsum;
  P.frame = frame;
  t->links = P;
  t->fk = fk;
  return GMR_OK;
}

int gmr_motion_tracker_set_link_terms(gmr_motion_tracker_t* t, const float* scale, const float* weight, float fail_dist) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  for (int k = 0; k < gmr::LINK_TERMS; k++) {
    if (scale && (!(scale[k] > 0.0f) || !std::isfinite(scale[k])))
      return gmr_fail(GMR_ERR_ARG, "link scale[%d] = %g, must be positive and finite", k, (double)scale[k]);
    if (weight && !std::isfinite(weight[k])) return gmr_fail(GMR_ERR_ARG, "link weight[%d] is not finite", k);
  }
  if (!(fail_dist > 0.0f)) return gmr_fail(GMR_ERR_ARG, "fail_dist = %g, must be positive (or +inf)", (double)fail_dist);
  std::lock_guard<std::mutex> g(t->mu);
  for (int k = 0; k < gmr::LINK_TERMS; k++) {
    if (scale) t->links.scale[k] = scale[k];
    if (weight) t->links.term_weight[k] = weight[k];
  }
  t->links.fail_dist = fail_dist;
  return GMR_OK;
}

int gmr_motion_tracker_step_links_dev(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, const gmr_tracker_links_sim_t* links_sim,
                                      const gmr_tracker_out_t* out, const gmr_tracker_links_out_t* links_out, int flags, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::TrackerTables T;
  gmr::LinkPlan P;
  gmr::TrackerState S;
  const gmr_fk* fk;
  {
    std::lock_guard<std::mutex> g(t->mu);
    T = t->tab; P = t->links; fk = t->fk; S = t->S;
  }
  return gmr::links_step_launch(t, S, T, P, fk, sim, links_sim, out, links_out, flags, (hipStream_t)stream);
}

int gmr_motion_tracker_step_links(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, const gmr_tracker_links_sim_t* links_sim,
                                  const gmr_tracker_out_t* out, const gmr_tracker_links_out_t* links_out, int flags) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::LinkPlan& P = t->links;
  const size_t n = (size_t)t->N, r = (size_t)t->tab.R, ns = (size_t)P.nsel;
  const gmr_tracker_out_t none_out = {};
  const gmr_tracker_links_out_t none_lout = {};
  if (!out) out = &none_out;
  if (!links_out) links_out = &none_lout;
  if (P.nsel == 0) links_sim = nullptr;
  gmr::HostStage st;
  gmr_tracker_sim_t dsim = {};
  gmr_tracker_links_sim_t dlsim = {};
  gmr_tracker_out_t dout = {};
  gmr_tracker_links_out_t dlout = {};
  if (sim) gmr::stage_tracker_sim(st, dsim, *sim, n, r);
  if (links_sim) {
    // the link arrays (their extent from the strides) may interleave in one tensor
    const long long es = links_sim->env_stride, bs = links_sim->body_stride;
    if ((es == 0) != (bs == 0) || es < 0 || bs < 0)
      return gmr_fail(GMR_ERR_ARG, "env_stride = %lld, body_stride = %lld: both positive, or both 0 for four contiguous arrays", es, bs);
    int maxb = 0;
    for (int k = 0; k < P.nsel; k++) maxb = P.sim_body[k] > maxb ? P.sim_body[k] : maxb;
    auto extent = [&](size_t width) { return 4 * (es ? (n - 1) * (size_t)es + (size_t)maxb * (size_t)bs + width : n * ns * width); };
    st.in_shared(dlsim.body_pos, links_sim->body_pos, extent(3)); st.in_shared(dlsim.body_rot, links_sim->body_rot, extent(4));
    st.in_shared(dlsim.body_vel, links_sim->body_vel, extent(3)); st.in_shared(dlsim.body_ang_vel, links_sim->body_ang_vel, extent(3));
    dlsim.env_stride = es; dlsim.body_stride = bs;
  }
  gmr::stage_tracker_out(st, dout, *out, n, r);
  st.out(dlout.ref_body_pos, links_out->ref_body_pos, n * ns * 12); st.out(dlout.ref_body_rot, links_out->ref_body_rot, n * ns * 16);
  st.out(dlout.ref_body_vel, links_out->ref_body_vel, n * ns * 12); st.out(dlout.ref_body_ang_vel, links_out->ref_body_ang_vel, n * ns * 12);
  st.out(dlout.link_err, links_out->link_err, n * 16); st.out(dlout.link_term, links_out->link_term, n * 16);
  st.out(dlout.max_dist, links_out->max_dist, n * 4); st.out(dlout.fail, links_out->fail, n * 4);
  GMR_STAGE_TRY(st, upload);
  const int rc = gmr::links_step_launch(t, t->S, t->tab, P, t->fk, sim ? &dsim : nullptr, links_sim ? &dlsim : nullptr, &dout, &dlout, flags, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

}  // extern "C"
