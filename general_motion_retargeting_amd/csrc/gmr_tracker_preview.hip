// gmr_tracker_preview.hip -- the preview of the motion tracker: the reference at every environment's clock plus K offsets, packed
// as observation rows, in one launch that writes nothing of the tracker.
//
//   tracker_preview_kernel   the sampler's shape: 16 lanes per (environment, offset) query, 16 queries per workgroup, the K queries
//                            of an environment adjacent.  Lanes l < 3 (l < 4) hold component l of the sampled root rows as in the
//                            step (moved by the environment's anchor in the raw and the sim frame when anchors are enabled,
//                            gmr_tracker_anchor.hip); a 16-lane group is one DPP row, so the components meet by row-local shuffles.  The row of a
//                            query is assembled in LDS and the 16 rows of a workgroup -- one contiguous span of 16 D floats that
//                            starts at a multiple of 64 D bytes -- leave with 16-byte stores.
//
// The offsets, the block table, the body selection and the dof tables are kernel arguments staged in LDS once per workgroup.  The
// tracker's state is read, never written; no device scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_motion_sample.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation, as in the sampler whose bits the raw rows reproduce
#pragma clang fp contract(off)

namespace gmr {

constexpr int PV_ROWS = 256 / MOTION_GROUP;      // queries, and rows, per workgroup
constexpr int PV_ALL_BLOCKS = 255;

// D: the floats of one row
__host__ __device__ inline int preview_width(int blocks, int R, int nsel) {
  int d = 0;
  if (blocks & GMR_PREVIEW_ROOT_POS) d += 3;
  if (blocks & GMR_PREVIEW_ROOT_QUAT) d += 4;
  if (blocks & GMR_PREVIEW_ROOT_ROT6) d += 6;
  if (blocks & GMR_PREVIEW_ROOT_VEL) d += 3;
  if (blocks & GMR_PREVIEW_ROOT_ANG_VEL) d += 3;
  if (blocks & GMR_PREVIEW_DOF_POS) d += R;
  if (blocks & GMR_PREVIEW_DOF_VEL) d += R;
  if (blocks & GMR_PREVIEW_BODY_POS) d += 3 * nsel;
  return d;
}

// x of lane j of this lane's 16-lane group
__device__ __forceinline__ float row_get(float x, int j) { return __shfl(x, j, MOTION_GROUP); }
__device__ __forceinline__ float pick3(int l, float a, float b, float c) { return l == 0 ? a : (l == 1 ? b : c); }

// (the heading frame of the tracker links, yaw_of and unyaw: gmr_tracker_dev.h)

__global__ __launch_bounds__(256) void tracker_preview_kernel(const MotionArrays A, const TrackerState S, const TrackerTables Tb,
                                                              const PreviewPlan P, int N, int loop, const float* __restrict__ base_pos,
                                                              const float* __restrict__ base_quat, float* __restrict__ obs,
                                                              int32_t* __restrict__ valid, int32_t* __restrict__ status) {
  __shared__ int s_map[TRACKER_MAX_DOF], s_body[PREVIEW_MAX_BODIES];
  __shared__ float s_def[TRACKER_MAX_DOF], s_off[PREVIEW_MAX_OFFSETS];
  extern __shared__ __align__(16) float s_rows[];      // [PV_ROWS][D]
  if (threadIdx.x < TRACKER_MAX_DOF) {
    s_map[threadIdx.x] = Tb.map[threadIdx.x];
    s_def[threadIdx.x] = Tb.dof_default[threadIdx.x];
  } else if (threadIdx.x < TRACKER_MAX_DOF + PREVIEW_MAX_OFFSETS) {
    s_off[threadIdx.x - TRACKER_MAX_DOF] = P.offset[threadIdx.x - TRACKER_MAX_DOF];
  } else if (threadIdx.x < TRACKER_MAX_DOF + PREVIEW_MAX_OFFSETS + PREVIEW_MAX_BODIES) {
    s_body[threadIdx.x - TRACKER_MAX_DOF - PREVIEW_MAX_OFFSETS] = P.body[threadIdx.x - TRACKER_MAX_DOF - PREVIEW_MAX_OFFSETS];
  }
  __syncthreads();
  const int K = P.K, R = Tb.R, blocks = P.blocks, nsel = (blocks & GMR_PREVIEW_BODY_POS) ? P.nsel : 0;
  const int ndof = A.ndof;
  const int D = preview_width(blocks, R, nsel);
  const int NK = N * K;                      // N <= 2^26 environments (checked at creation) times K <= 16 offsets: at most 2^30
  const int q0 = (int)blockIdx.x * PV_ROWS;
  const int g = (int)threadIdx.x / MOTION_GROUP, l = (int)threadIdx.x & (MOTION_GROUP - 1);
  const int qn = q0 + g;
  if (qn < NK) {      // (the same for the 16 lanes of a group, as is every branch below that holds a shuffle)
    const int e = qn / K, k = qn - e * K;
    const int c = S.clip[e];
    const float tf = S.time[e];
    const double tq = (double)tf + (double)s_off[k];
    const MotionQuery Q = motion_query(A, c, tq, loop);      // (gmr_motion_sample.h)
#ifdef GMR_PREVIEW_DIRECT_STORES      // (A/B build of DESIGN.md section 6m: every lane stores its floats straight to obs)
    float* row = obs ? obs + (size_t)qn * D : s_rows;
#else
    float* row = s_rows + g * D;
#endif
    if (!Q.ok) {
      // neutralised: a NaN row, nothing of the library is read
      if (obs)
        for (int j = l; j < D; j += MOTION_GROUP) row[j] = NAN;
      if (l == 0) {
        if (valid) valid[qn] = 0;
        if (status && k == 0) status[e] = 1;
      }
    } else {
      if (l == 0) {
        if (valid) {      // inside the clip: the duration and dt of motion_query
          const double fps = A.fps[c];
          const double dt = 1.0 / fps, duration = (double)(A.seg_start[c + 1] - A.seg_start[c]) / fps;
          valid[qn] = (tq >= 0.0 && tq <= duration - dt) ? 1 : 0;
        }
        if (status && k == 0) status[e] = 0;
      }
      if (obs) {
        const bool same = Q.same;
        const size_t rl = Q.rl, rh = Q.rh;
        const float w0 = Q.w0, w1 = Q.w1;
        const bool anchored = P.frame != GMR_PREVIEW_FRAME_RAW;
        const bool body = nsel > 0;
        const bool want_p = (blocks & GMR_PREVIEW_ROOT_POS) || (anchored && body);
        const bool want_q = (blocks & (GMR_PREVIEW_ROOT_QUAT | GMR_PREVIEW_ROOT_ROT6)) || (anchored && body);
        const bool want_v = blocks & GMR_PREVIEW_ROOT_VEL, want_w = blocks & GMR_PREVIEW_ROOT_ANG_VEL;
        // component l of the sampled root rows, as in the step
        float pc = 0.0f, vc = 0.0f, wc = 0.0f, qc = 0.0f;
        if (l < 3) {
          if (want_p) pc = lerp1(A.root_pos, rl * 3 + l, rh * 3 + l, same, w0, w1);
          if (want_v) vc = lerp1(A.root_vel, rl * 3 + l, rh * 3 + l, same, w0, w1);
          if (want_w) wc = lerp1(A.root_ang_vel, rl * 3 + l, rh * 3 + l, same, w0, w1);
        }
        if (l < 4 && want_q) qc = slerp1(A.root_rot, rl, rh, l, same, w0, w1);
        // Tracker anchors: the raw and the sim frame see the reference where the environment's anchor puts it.
        // The reference frame is blind to it, and so is the root-local body block of the raw frame.  The K queries of an
        // environment are adjacent groups: they read the same 20 bytes.
        if (S.anchor_pos != nullptr && P.frame != GMR_PREVIEW_FRAME_REFERENCE) {
          Anchor An;
          anchor_turn(S, (size_t)e, An);
          const float at = l < 3 ? S.anchor_pos[(size_t)e * 3 + l] : 0.0f;
          if (want_p) pc = anchor_point_lane(An, l, pc, at);
          if (want_v) vc = anchor_vector_lane(An, l, vc);
          if (want_w) wc = anchor_vector_lane(An, l, wc);
          if (want_q) qc = anchor_quat_lane(An, l, qc);
        }
        // the anchor: its position in lanes 0 .. 2, z and w of its rotation in lanes 2 and 3
        float cy = 1.0f, sy = 0.0f, yz = 0.0f, yw = 1.0f, pax = 0.0f, pay = 0.0f, paz = 0.0f;
        if (anchored) {
          float ac = 0.0f, aq = 0.0f;
          if (P.frame == GMR_PREVIEW_FRAME_REFERENCE) {
            const MotionQuery Qa = motion_query(A, c, (double)tf, loop);      // the reference root at the environment's own clock
            if (l < 3) ac = lerp1(A.root_pos, Qa.rl * 3 + l, Qa.rh * 3 + l, Qa.same, Qa.w0, Qa.w1);
            if (l == 2 || l == 3) aq = slerp1(A.root_rot, Qa.rl, Qa.rh, l, Qa.same, Qa.w0, Qa.w1);
          } else {
            if (l < 3) ac = base_pos[(size_t)e * 3 + l];
            if (l == 2 || l == 3) aq = base_quat[(size_t)e * 4 + l];
          }
          pax = row_get(ac, 0); pay = row_get(ac, 1); paz = row_get(ac, 2);
          yaw_of(row_get(aq, 2), row_get(aq, 3), yz, yw);
          cy = yw * yw - yz * yz; sy = 2.0f * yz * yw;
        }
        int o = 0;
        float qx = 0.0f, qy = 0.0f, qz = 0.0f, qw = 1.0f, px = 0.0f, py = 0.0f, pz = 0.0f;
        if (want_q && (anchored || (blocks & GMR_PREVIEW_ROOT_ROT6))) {
          qx = row_get(qc, 0); qy = row_get(qc, 1); qz = row_get(qc, 2); qw = row_get(qc, 3);
        }
        if (want_p && anchored) { px = row_get(pc, 0); py = row_get(pc, 1); pz = row_get(pc, 2); }
        if (blocks & GMR_PREVIEW_ROOT_POS) {
          float x = pc;
          if (anchored) {
            float dx = px - pax, dy = py - pay;
            const float dz = pz - paz;
            unyaw(cy, sy, dx, dy);
            x = pick3(l, dx, dy, dz);
          }
          if (l < 3) row[o + l] = x;
          o += 3;
        }
        // q_rel = conj(0, 0, yz, yw) * q
        float rx = qx, ry = qy, rz = qz, rw = qw;
        if (anchored && want_q) {
          rx = yw * qx + yz * qy; ry = yw * qy - yz * qx; rz = yw * qz - yz * qw; rw = yw * qw + yz * qz;
        }
        if (blocks & GMR_PREVIEW_ROOT_QUAT) {
          float x = qc;
          if (anchored) x = l == 3 ? rw : pick3(l, rx, ry, rz);
          if (l < 4) row[o + l] = x;
          o += 4;
        }
        if (blocks & GMR_PREVIEW_ROOT_ROT6) {
          // columns 0 and 1 of R(q), q as it is
          const float c0x = 1.0f - 2.0f * (ry * ry + rz * rz), c0y = 2.0f * (rx * ry + rz * rw), c0z = 2.0f * (rx * rz - ry * rw);
          const float c1x = 2.0f * (rx * ry - rz * rw), c1y = 1.0f - 2.0f * (rx * rx + rz * rz), c1z = 2.0f * (ry * rz + rx * rw);
          if (l < 6) row[o + l] = l < 3 ? pick3(l, c0x, c0y, c0z) : pick3(l - 3, c1x, c1y, c1z);
          o += 6;
        }
        if (blocks & GMR_PREVIEW_ROOT_VEL) {
          float x = vc;
          if (anchored) {
            float vx = row_get(vc, 0), vy = row_get(vc, 1);
            const float vz = row_get(vc, 2);
            unyaw(cy, sy, vx, vy);
            x = pick3(l, vx, vy, vz);
          }
          if (l < 3) row[o + l] = x;
          o += 3;
        }
        if (blocks & GMR_PREVIEW_ROOT_ANG_VEL) {
          float x = wc;
          if (anchored) {
            float wx = row_get(wc, 0), wy = row_get(wc, 1);
            const float wz = row_get(wc, 2);
            unyaw(cy, sy, wx, wy);
            x = pick3(l, wx, wy, wz);
          }
          if (l < 3) row[o + l] = x;
          o += 3;
        }
        // the dofs in robot order, as in the step
        const bool want_dp = blocks & GMR_PREVIEW_DOF_POS, want_dv = blocks & GMR_PREVIEW_DOF_VEL;
        if (want_dp || want_dv) {
          float* rp = row + o;
          float* rv = rp + (want_dp ? R : 0);
          for (int j = l; j < R; j += MOTION_GROUP) {
            const int m = s_map[j];
            float p = s_def[j], v = 0.0f;
            if (m >= 0) {
              if (want_dp) p = lerp1(A.dof_pos, rl * ndof + m, rh * ndof + m, same, w0, w1);
              if (want_dv) v = lerp1(A.dof_vel, rl * ndof + m, rh * ndof + m, same, w0, w1);
            }
            if (want_dp) rp[j] = p;
            if (want_dv) rv[j] = v;
          }
          o += (want_dp ? R : 0) + (want_dv ? R : 0);
        }
        // the selected bodies, one per lane and turn
        if (body) {
          const size_t nb3 = (size_t)A.nbody * 3;
          for (int b = l; b < nsel; b += MOTION_GROUP) {
            const size_t col = (size_t)s_body[b] * 3;
            float lx = lerp1(A.local_body_pos, rl * nb3 + col, rh * nb3 + col, same, w0, w1);
            float ly = lerp1(A.local_body_pos, rl * nb3 + col + 1, rh * nb3 + col + 1, same, w0, w1);
            float lz = lerp1(A.local_body_pos, rl * nb3 + col + 2, rh * nb3 + col + 2, same, w0, w1);
            if (anchored) {
              // p + R(q) l - p_a, then the yaw: R(q) l = l + w t + u x t, t = 2 (u x l)
              const float tx = 2.0f * (qy * lz - qz * ly), ty = 2.0f * (qz * lx - qx * lz), tz = 2.0f * (qx * ly - qy * lx);
              const float wx = lx + qw * tx + (qy * tz - qz * ty), wy = ly + qw * ty + (qz * tx - qx * tz),
                          wz = lz + qw * tz + (qx * ty - qy * tx);
              lx = (px + wx) - pax; ly = (py + wy) - pay; lz = (pz + wz) - paz;
              unyaw(cy, sy, lx, ly);
            }
            float* d = row + o + b * 3;
            d[0] = lx; d[1] = ly; d[2] = lz;
          }
        }
      }
    }
  }
#ifdef GMR_PREVIEW_DIRECT_STORES
  return;
#endif
  if (!obs) return;
  __syncthreads();
  // the rows of this workgroup are one span of obs; it starts at a multiple of 64 D bytes
  const int left = NK - q0;
  const int nfl = (left < PV_ROWS ? left : PV_ROWS) * D;
  float* dst = obs + (size_t)q0 * D;
  if (((uintptr_t)dst & 15) == 0) {
    const int n4 = nfl >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(s_rows)[i];
    for (int i = (n4 << 2) + threadIdx.x; i < nfl; i += 256) dst[i] = s_rows[i];
  } else {
    for (int i = threadIdx.x; i < nfl; i += 256) dst[i] = s_rows[i];
  }
}

// what the two preview entry points share once the tables and the plan are in hand; every argument check of a preview
static int preview_launch(gmr_motion_tracker* t, const TrackerTables& T, const PreviewPlan& P, const gmr_tracker_sim_t* sim, float* obs,
                          int32_t* valid, int32_t* status, hipStream_t stream) {
  if (P.K == 0) return gmr_fail(GMR_ERR_ARG, "the tracker has no preview configured (gmr_motion_tracker_set_preview)");
  const bool from_sim = P.frame == GMR_PREVIEW_FRAME_SIM;
  if (from_sim && (!sim || !sim->base_pos || !sim->base_quat))
    return gmr_fail(GMR_ERR_ARG, "the sim frame needs base_pos and base_quat of the simulator's root");
  if ((P.blocks & GMR_PREVIEW_BODY_POS) && !t->lib->has_body) return gmr_fail(GMR_ERR_ARG, "the motion library holds no local_body_pos");
  if (!obs && !valid && !status) return GMR_OK;
  const int D = preview_width(P.blocks, T.R, P.nsel);
  const long long NK = (long long)t->N * P.K;
  hipLaunchKernelGGL(tracker_preview_kernel, dim3((unsigned)((NK + PV_ROWS - 1) / PV_ROWS)), dim3(256), sizeof(float) * PV_ROWS * D, stream,
                     t->lib->A, t->S, T, P, t->N, t->loop, from_sim ? sim->base_pos : nullptr, from_sim ? sim->base_quat : nullptr, obs, valid,
                     status);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker preview") ---------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_preview(gmr_motion_tracker_t* t, int K, const float* offsets, int blocks, int frame, const int32_t* body_sel,
                                   int nsel, int* row_width) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (row_width) *row_width = 0;
  if (K == 0) {
    std::lock_guard<std::mutex> g(t->mu);
    t->preview = gmr::PreviewPlan{};
    return GMR_OK;
  }
  if (K < 1 || K > GMR_PREVIEW_MAX_OFFSETS) return gmr_fail(GMR_ERR_ARG, "K = %d offsets outside [1, %d]", K, GMR_PREVIEW_MAX_OFFSETS);
  if (!offsets) return gmr_fail(GMR_ERR_ARG, "null offsets");
  for (int k = 0; k < K; k++)
    if (!std::isfinite(offsets[k])) return gmr_fail(GMR_ERR_ARG, "offsets[%d] is not finite", k);
  if (blocks & ~gmr::PV_ALL_BLOCKS) return gmr_fail(GMR_ERR_ARG, "unknown preview block bits 0x%x", blocks & ~gmr::PV_ALL_BLOCKS);
  if (!blocks) return gmr_fail(GMR_ERR_ARG, "a preview needs at least one block");
  if (frame != GMR_PREVIEW_FRAME_RAW && frame != GMR_PREVIEW_FRAME_REFERENCE && frame != GMR_PREVIEW_FRAME_SIM)
    return gmr_fail(GMR_ERR_ARG, "unknown preview frame %d", frame);
  if (frame != GMR_PREVIEW_FRAME_RAW && (blocks & GMR_PREVIEW_ROOT_ANG_VEL) && t->lib->reference_angvel)
    return gmr_fail(GMR_ERR_ARG, "root_ang_vel in an anchored frame needs a library filled with GMR_MOTION_ANGVEL_WORLD: the root_ang_vel of "
                                 "GMR_MOTION_ANGVEL_REFERENCE is not a physical angular velocity and cannot be rotated");
  gmr::PreviewPlan P;
  if (blocks & GMR_PREVIEW_BODY_POS) {
    const int nbody = t->lib->A.nbody;
    if (!t->lib->has_body) return gmr_fail(GMR_ERR_ARG, "the body block needs a library filled with local_body_pos");
    if (!body_sel || nsel < 1 || nsel > GMR_PREVIEW_MAX_BODIES)
      return gmr_fail(GMR_ERR_ARG, "the body block needs a selection of 1 to %d bodies (nsel = %d)", GMR_PREVIEW_MAX_BODIES, nsel);
    for (int k = 0; k < nsel; k++) {
      if (body_sel[k] < 0 || body_sel[k] >= nbody) return gmr_fail(GMR_ERR_ARG, "body_sel[%d] = %d outside [0, %d)", k, body_sel[k], nbody);
      for (int j = 0; j < k; j++)
        if (body_sel[j] == body_sel[k]) return gmr_fail(GMR_ERR_ARG, "body_sel names body %d twice", body_sel[k]);
      P.body[k] = (int16_t)body_sel[k];
    }
    P.nsel = nsel;
  } else if (nsel != 0) {
    return gmr_fail(GMR_ERR_ARG, "a body selection (nsel = %d) without GMR_PREVIEW_BODY_POS", nsel);
  }
  P.K = K; P.blocks = blocks; P.frame = frame;
  for (int k = 0; k < K; k++) P.offset[k] = offsets[k];
  std::lock_guard<std::mutex> g(t->mu);
  t->preview = P;
  if (row_width) *row_width = gmr::preview_width(blocks, t->tab.R, P.nsel);
  return GMR_OK;
}

int gmr_motion_tracker_preview_dev(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, float* d_obs, int32_t* d_valid, int32_t* d_status,
                                   void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::TrackerTables T;
  gmr::PreviewPlan P;
  {
    std::lock_guard<std::mutex> g(t->mu);
    T = t->tab; P = t->preview;
  }
  return gmr::preview_launch(t, T, P, sim, d_obs, d_valid, d_status, (hipStream_t)stream);
}

int gmr_motion_tracker_preview(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, float* obs, int32_t* valid, int32_t* status) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::PreviewPlan& P = t->preview;
  if (P.K == 0) return gmr_fail(GMR_ERR_ARG, "the tracker has no preview configured (gmr_motion_tracker_set_preview)");
  const bool from_sim = P.frame == GMR_PREVIEW_FRAME_SIM;
  if (from_sim && (!sim || !sim->base_pos || !sim->base_quat))
    return gmr_fail(GMR_ERR_ARG, "the sim frame needs base_pos and base_quat of the simulator's root");
  const size_t n = (size_t)t->N, nk = n * (size_t)P.K, d = (size_t)gmr::preview_width(P.blocks, t->tab.R, P.nsel);
  gmr::HostStage st;
  gmr_tracker_sim_t dsim = {};
  float* d_obs;
  int32_t *d_valid, *d_status;
  if (from_sim) {
    st.in(dsim.base_pos, sim->base_pos, n * 12); st.in(dsim.base_quat, sim->base_quat, n * 16);
  }
  st.out(d_obs, obs, nk * d * 4); st.out(d_valid, valid, nk * 4); st.out(d_status, status, n * 4);
  GMR_STAGE_TRY(st, upload);
  const int rc = gmr::preview_launch(t, t->tab, P, from_sim ? &dsim : nullptr, d_obs, d_valid, d_status, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

}  // extern "C"
