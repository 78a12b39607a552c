// gmr_tracker_feet.hip -- feet, contacts and terrain heights of an imitation step on the motion tracker: what
// booster_gym/envs/t1.py::step still did in small framework launches and host round trips after 6q -- the bilinear terrain height of
// booster_gym/utils/terrain.py:101-121 (which copies the positions to the host, interpolates in NumPy and uploads the result), the feet
// pose, roll, yaw and edge contacts of _refresh_feet_state (:529-549), the gait clock (:478, :585-586), the contact-force termination
// (:553), collision (:627-629), the seven feet_* terms (:696-730) and the roll-over of last_feet_pos (:495).  The statement of record is
// tests/feet_mirror.py.
//
//   tracker_terrain_heights_kernel   one lane per point: the height and, counted with an integer atomic, whether the point left the field
//   tracker_feet_kernel              ONE launch per environment step, the shape of tracker_proprio_kernel (16 lanes per environment, 16
//                                    environments per workgroup, the configuration staged in LDS once per workgroup).  Lane l < 2 E owns
//                                    edge point l % E of foot l / E (one rotation, four int16 gathers); the body lists are strided over
//                                    the lanes; any and the counts go through the xor butterfly as integers; the root and feet quantities
//                                    are computed in every lane from broadcast loads; every float sum has at most six summands and runs in
//                                    one lane.
//
// last_feet_pos and gait_process belong to the tracker and are written by tracker_feet_kernel only; the tracker stays single-stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <mutex>

#include "../../include/gmr_hip.h"
#include "gmr_handles.h"
#include "gmr_internal.h"
#include "gmr_tracker_dev.h"
#include "gmr_workspace.h"

// one rounding per operation: tests/feet_mirror.py states every line in float32 (the terrain's weights and products: float64) NumPy
#pragma clang fp contract(off)

#include "gmr_terrain.h"

namespace gmr {

struct FeetIn {
  const float *body_pos, *body_rot;
  long long env_stride[2], body_stride[2];          // of body_pos and body_rot, in floats
  const float *forces, *root, *gait_frequency;
  const int32_t* steps;
};
struct FeetOut {
  float *feet_pos, *feet_roll, *feet_yaw, *ground, *gait, *term, *total;
  int32_t *feet_contact, *done;
};

// (V3, pick, rotate_forward, group_or, group_count: gmr_tracker_dev.h)

__global__ __launch_bounds__(256) void tracker_terrain_heights_kernel(const TerrainTables T, long long M, const float* __restrict__ points,
                                                                      long long stride, float* __restrict__ heights, int32_t* outside) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  bool out;
  const float h = terrain_height(T, points[i * stride], points[i * stride + 1], &out);
  heights[i] = h;
  if (out && outside) atomicAdd(outside, 1);
}

// torch's remainder for a positive divisor: fmod, then the divisor is added to a negative result
__device__ __forceinline__ float remainder_pos(float a, float b) {
  const float r = fmodf(a, b);
  return (r != 0.0f && r < 0.0f) ? r + b : r;
}
constexpr float PI_F = 3.1415927f, TWO_PI_F = 6.2831855f;
// (a + pi) % 2 pi - pi (t1.py:533-534, :713, :717)
__device__ __forceinline__ float wrap_pi(float a) { return remainder_pos(a + PI_F, TWO_PI_F) - PI_F; }
// roll and yaw of get_euler_xyz for an xyzw quaternion, each % 2 pi
__device__ __forceinline__ float euler_roll(float x, float y, float z, float w) {
  return remainder_pos(atan2f(2.0f * (w * x + y * z), ((w * w - x * x) - y * y) + z * z), TWO_PI_F);
}
__device__ __forceinline__ float euler_yaw(float x, float y, float z, float w) {
  return remainder_pos(atan2f(2.0f * (w * z + x * y), ((w * w + x * x) - y * y) - z * z), TWO_PI_F);
}

__global__ __launch_bounds__(256) void tracker_feet_kernel(const FeetTables Ft, const TerrainTables T, const FeetState St, const FeetIn X,
                                                           const FeetOut O, int N, float dtf) {
  __shared__ float s_edge[FEET_MAX_EDGES * 3];
  __shared__ int32_t s_term[FEET_MAX_BODIES], s_pen[FEET_MAX_BODIES];
  if (threadIdx.x < FEET_MAX_EDGES * 3) s_edge[threadIdx.x] = Ft.edge[threadIdx.x];
  if (threadIdx.x < FEET_MAX_BODIES) {
    s_term[threadIdx.x] = Ft.term_body[threadIdx.x];
    s_pen[threadIdx.x] = Ft.pen_body[threadIdx.x];
  }
  __syncthreads();
  const int e = (blockIdx.x * 256 + threadIdx.x) / MOTION_GROUP;
  const int l = threadIdx.x & (MOTION_GROUP - 1);
  if (e >= N) return;
  const int E = Ft.E;

  // ---- the two feet, in every lane of the group from broadcast loads (:530-534) ----
  const float* bp = X.body_pos + (long long)e * X.env_stride[0];
  const float* br = X.body_rot + (long long)e * X.env_stride[1];
  const float* p0 = bp + Ft.feet_body[0] * X.body_stride[0];
  const float* p1 = bp + Ft.feet_body[1] * X.body_stride[0];
  const float* q0 = br + Ft.feet_body[0] * X.body_stride[1];
  const float* q1 = br + Ft.feet_body[1] * X.body_stride[1];
  const V3 f0{p0[0], p0[1], p0[2]}, f1{p1[0], p1[1], p1[2]};
  const float ax = q0[0], ay = q0[1], az = q0[2], aw = q0[3];
  const float bx = q1[0], by = q1[1], bz = q1[2], bw = q1[3];
  const float roll0 = wrap_pi(euler_roll(ax, ay, az, aw)), roll1 = wrap_pi(euler_roll(bx, by, bz, bw));
  const float yaw0 = wrap_pi(euler_yaw(ax, ay, az, aw)), yaw1 = wrap_pi(euler_yaw(bx, by, bz, bw));

  // ---- the edge points, one per lane: edge = foot + quat_rotate(foot_quat, edge_pos[k]); contact = any (edge.z - height < clearance) ----
  int hit = 0;
  if (l < 2 * E) {
    const int f = l >= E ? 1 : 0, k = l - f * E;
    const V3 v{s_edge[3 * k], s_edge[3 * k + 1], s_edge[3 * k + 2]};
    const V3 r = f ? rotate_forward(bx, by, bz, bw, v) : rotate_forward(ax, ay, az, aw, v);
    const V3 c = f ? f1 : f0;
    const float ex = c.x + r.x, ey = c.y + r.y, ez = c.z + r.z;                                           // :543
    bool out;
    const float h = terrain_height(T, ex, ey, &out);
    if (ez - h < Ft.clearance) hit = 1 << f;                                                              // :545; a NaN compares false
  }
  hit = group_or(hit);
  const int c0 = hit & 1, c1 = (hit >> 1) & 1;

  // ---- contact forces: the two body lists strided over the lanes (:553, :629) ----
  int n_term = 0, n_pen = 0;
  if (X.forces) {
    const float* fe = X.forces + (size_t)e * (size_t)Ft.nb * 3;
    for (int j = l; j < Ft.n_term; j += MOTION_GROUP) {
      const float* f = fe + s_term[j] * 3;
      n_term += sqrtf((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]) > Ft.threshold ? 1 : 0;
    }
    for (int j = l; j < Ft.n_pen; j += MOTION_GROUP) {
      const float* f = fe + s_pen[j] * 3;
      n_pen += sqrtf((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]) > Ft.threshold ? 1 : 0;
    }
    n_term = group_count(n_term);
    n_pen = group_count(n_pen);
  }

  // ---- the root: terrain height under it and its yaw (:555, :624, :717, :720) ----
  const float* rs = X.root + (size_t)e * 13;
  bool root_out;
  const float ground = terrain_height(T, rs[0], rs[1], &root_out);
  const float base_yaw = euler_yaw(rs[3], rs[4], rs[5], rs[6]);

  // ---- the gait clock (:478, :585-586) ----
  const float gf = X.gait_frequency ? X.gait_frequency[e] : 0.0f;
  const float gp = fmodf(St.gait_process[e] + dtf * gf, 1.0f);
  const float on = gf > 1.0e-8f ? 1.0f : 0.0f;
  const float ga = TWO_PI_F * gp;
  const float gait_c = cosf(ga) * on, gait_s = sinf(ga) * on;

  // ---- the terms (:629, :696-730); the old feet positions are loaded by every lane ----
  const float* lf = St.last_feet_pos + (size_t)e * 6;
  const float v0x = __fdiv_rn(lf[0] - f0.x, dtf), v0y = __fdiv_rn(lf[1] - f0.y, dtf), v0z = __fdiv_rn(lf[2] - f0.z, dtf);
  const float v1x = __fdiv_rn(lf[3] - f1.x, dtf), v1y = __fdiv_rn(lf[4] - f1.y, dtf), v1z = __fdiv_rn(lf[5] - f1.z, dtf);
  if (O.term || O.total) {
    const float gate = X.steps ? (X.steps[e] > 1 ? 1.0f : 0.0f) : 1.0f;
    const float s0 = (v0x * v0x + v0y * v0y) + v0z * v0z, s1 = (v1x * v1x + v1y * v1y) + v1z * v1z;
    const float slip = (s0 * (float)c0 + s1 * (float)c1) * gate;                                          // :698-704
    const float vel_z = v0z * v0z + v1z * v1z;                                                            // :707
    const float t_roll = roll0 * roll0 + roll1 * roll1;                                                   // :710
    const float yd = wrap_pi(yaw1 - yaw0);                                                                // :713
    const float mean = (yaw0 + yaw1) * 0.5f + (fabsf(yaw1 - yaw0) > PI_F ? PI_F : 0.0f);                  // :716
    const float ym = wrap_pi(base_yaw - mean);                                                            // :717
    const float dist = fabsf(cosf(base_yaw) * (f1.y - f0.y) - sinf(base_yaw) * (f1.x - f0.x));            // :721-724
    float dr = Ft.distance_ref - dist;                                                                    // :725; a NaN stays one
    dr = dr < 0.0f ? 0.0f : dr;
    dr = dr > 0.1f ? 0.1f : dr;
    const bool moving = gf > 1.0e-8f;
    const bool left = fabsf(gp - 0.25f) < Ft.half_swing && moving, right = fabsf(gp - 0.75f) < Ft.half_swing && moving;   // :728-729
    const float swing = ((left && !c0) ? 1.0f : 0.0f) + ((right && !c1) ? 1.0f : 0.0f);                   // :730
    const float t[FEET_TERMS] = {(float)n_pen, slip, vel_z, t_roll, yd * yd, ym * ym, dr, swing};
    float mine = 0.0f, total = 0.0f;
#pragma unroll
    for (int k = 0; k < FEET_TERMS; k++) {
      const bool given = k == 0 ? X.forces != nullptr : true;
      if (given && Ft.scale[k] != 0.0f) total = total + Ft.scale[k] * t[k];
      mine = l == k ? t[k] : mine;
    }
    if (O.term && l < FEET_TERMS) O.term[(size_t)e * FEET_TERMS + l] = mine;
    if (O.total && l == 0) O.total[e] = total;
  }

  // ---- the outputs ----
  if (l < 6) {
    const float v = l < 3 ? pick(f0, l) : pick(f1, l - 3);
    if (O.feet_pos) O.feet_pos[(size_t)e * 6 + l] = v;
  }
  if (l < 2) {
    if (O.feet_roll) O.feet_roll[(size_t)e * 2 + l] = l ? roll1 : roll0;
    if (O.feet_yaw) O.feet_yaw[(size_t)e * 2 + l] = l ? yaw1 : yaw0;
    if (O.feet_contact) O.feet_contact[(size_t)e * 2 + l] = l ? c1 : c0;
    if (O.gait) O.gait[(size_t)e * 2 + l] = l ? gait_s : gait_c;
  }
  if (l == 0) {
    if (O.ground) O.ground[e] = ground;
    if (O.done) O.done[e] = n_term > 0 ? 8 : 0;                                                           // :553; bit 3
  }
  // ---- the roll-over (:495, :478).  Every lane of the group has read the old values and the group is part of ONE wavefront, so the
  // stores below follow the loads in program order; the wait makes sure the loads have also returned (vmcnt(0)), as in 6q. ----
  __builtin_amdgcn_s_waitcnt(0x0F70);
  if (l < 6) St.last_feet_pos[(size_t)e * 6 + l] = l < 3 ? pick(f0, l) : pick(f1, l - 3);
  if (l == 0) St.gait_process[e] = gp;
}

static int feet_set(const FeetTables& Ft) {
  if (Ft.E == 0) return gmr_fail(GMR_ERR_ARG, "feet are not set on this tracker (gmr_motion_tracker_set_feet)");
  return GMR_OK;
}

// what the entry points copy under the mutex: everything a launch carries
struct FeetView {
  FeetTables tab;
  TerrainTables terrain;
  FeetState st;
};
static FeetView feet_view(gmr_motion_tracker* t) { return FeetView{t->feet, t->terrain, t->feet_state}; }

// the checks of a feet call that need no device; fills the strides of X
static int feet_check(const FeetTables& Ft, const gmr_tracker_links_sim_t* bodies, const gmr_feet_in_t* in,
                      const gmr_feet_out_t* out, long long es[2], long long bs[2]) {
  const int rc = feet_set(Ft);
  if (rc != GMR_OK) return rc;
  if (!bodies || !in || !out) return gmr_fail(GMR_ERR_ARG, "null bodies / input / output table");
  if (!bodies->body_pos || !bodies->body_rot || !in->root_states) return gmr_fail(GMR_ERR_ARG, "null body_pos / body_rot / root_states");
  const long long e = bodies->env_stride, b = bodies->body_stride;
  if ((e == 0) != (b == 0) || e < 0 || b < 0)
    return gmr_fail(GMR_ERR_ARG, "env_stride = %lld, body_stride = %lld: both positive, or both 0 for contiguous arrays", e, b);
  if (e && (b < 4 || e < (long long)(Ft.nb - 1) * b + 4))
    return gmr_fail(GMR_ERR_ARG, "env_stride = %lld, body_stride = %lld do not hold %d bodies", e, b, Ft.nb);
  es[0] = e ? e : (long long)Ft.nb * 3; bs[0] = e ? b : 3;
  es[1] = e ? e : (long long)Ft.nb * 4; bs[1] = e ? b : 4;
  return GMR_OK;
}

static int feet_launch(gmr_motion_tracker* t, const FeetView& V, const gmr_tracker_links_sim_t* bodies, const gmr_feet_in_t* in,
                       const gmr_feet_out_t* out, hipStream_t stream) {
  FeetIn X;
  const int rc = feet_check(V.tab, bodies, in, out, X.env_stride, X.body_stride);
  if (rc != GMR_OK) return rc;
  X.body_pos = bodies->body_pos; X.body_rot = bodies->body_rot;
  X.forces = in->contact_forces; X.root = in->root_states; X.gait_frequency = in->gait_frequency; X.steps = in->episode_steps;
  const FeetOut O{out->feet_pos, out->feet_roll, out->feet_yaw, out->ground, out->gait, out->term, out->total, out->feet_contact, out->done};
  hipLaunchKernelGGL(tracker_feet_kernel, dim3(row_blocks(t->N, MOTION_GROUP)), dim3(256), 0, stream, V.tab, V.terrain, V.st, X, O, t->N, t->dtf);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

static int heights_check(long long M, const float* points, long long stride, const float* heights) {
  if (M < 0 || M > (1ll << 31)) return gmr_fail(GMR_ERR_ARG, "M = %lld points out of range", M);
  if (stride < 2) return gmr_fail(GMR_ERR_ARG, "stride = %lld floats: a point has at least x and y", stride);
  if (M > 0 && (!points || !heights)) return gmr_fail(GMR_ERR_ARG, "null points / heights");
  return GMR_OK;
}

static int heights_launch(const TerrainTables& T, long long M, const float* d_points, long long stride, float* d_heights, int32_t* d_outside,
                          hipStream_t stream) {
  const int rc = heights_check(M, d_points, stride, d_heights);
  if (rc != GMR_OK) return rc;
  if (M == 0) return GMR_OK;
  hipLaunchKernelGGL(tracker_terrain_heights_kernel, dim3(lane_blocks(M)), dim3(256), 0, stream, T, M, d_points, stride, d_heights,
                     d_outside);
  GMR_HIP_TRY(hipGetLastError());
  return GMR_OK;
}

}  // namespace gmr

// ---- C-ABI (include/gmr_hip.h, "tracker feet") -----------------------------------------------------------------------------------

extern "C" {

int gmr_motion_tracker_set_terrain(gmr_motion_tracker_t* t, const int16_t* height_field, int nx, int ny, double horizontal_scale,
                                   double vertical_scale, int border_pixels) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!std::isfinite(horizontal_scale) || !(horizontal_scale > 0.0) || !std::isfinite((float)horizontal_scale) || !((float)horizontal_scale > 0.0f))
    return gmr_fail(GMR_ERR_ARG, "horizontal_scale = %g must be positive and finite in float32", horizontal_scale);
  if (!std::isfinite(vertical_scale) || !(vertical_scale > 0.0)) return gmr_fail(GMR_ERR_ARG, "vertical_scale = %g must be positive and finite", vertical_scale);
  if (border_pixels < 0 || border_pixels > (1 << 24)) return gmr_fail(GMR_ERR_ARG, "border_pixels = %d outside [0, 2^24]", border_pixels);
  if (height_field && (nx < 2 || ny < 2 || nx > (1 << 24) || ny > (1 << 24)))
    return gmr_fail(GMR_ERR_ARG, "a height field is [nx][ny] with 2 <= nx, ny <= 2^24, got %d x %d", nx, ny);
  std::lock_guard<std::mutex> g(t->mu);
  GMR_HIP_TRY(hipDeviceSynchronize());               // launches in flight have read the field they were given
  gmr::TerrainTables T;
  if (height_field) {
    const size_t bytes = (size_t)nx * (size_t)ny * 2;
    if (bytes > t->terrain_block.size()) t->terrain = gmr::TerrainTables();      // (the old field goes with the block)
    GMR_HIP_TRY(t->terrain_block.reserve(bytes + 256));
    GMR_HIP_TRY(hipMemcpy(t->terrain_block.data(), height_field, bytes, hipMemcpyHostToDevice));
    GMR_HIP_TRY(hipDeviceSynchronize());
    T.field = (const int16_t*)t->terrain_block.data();
    T.nx = nx; T.ny = ny;
  }
  T.border = (float)border_pixels; T.hs = (float)horizontal_scale; T.vs = vertical_scale;
  t->terrain = T;
  return GMR_OK;
}

int gmr_motion_tracker_terrain_heights_dev(gmr_motion_tracker_t* t, int64_t M, const float* d_points, int64_t stride, float* d_heights,
                                           int32_t* d_outside, void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::TerrainTables T;
  {
    std::lock_guard<std::mutex> g(t->mu);
    T = t->terrain;
  }
  return gmr::heights_launch(T, (long long)M, d_points, (long long)stride, d_heights, d_outside, (hipStream_t)stream);
}

int gmr_motion_tracker_terrain_heights(gmr_motion_tracker_t* t, int64_t M, const float* points, int64_t stride, float* heights, int32_t* outside) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (outside) *outside = 0;
  std::lock_guard<std::mutex> g(t->mu);
  int rc = gmr::heights_check((long long)M, points, (long long)stride, heights);
  if (rc != GMR_OK) return rc;
  if (M == 0) return GMR_OK;
  const size_t m = (size_t)M, nin = ((m - 1) * (size_t)stride + 2) * 4;
  gmr::HostStage st;
  const float* d_points;
  float* d_heights;
  int32_t *d_count, count = 0;
  st.in(d_points, points, nin);
  st.out(d_heights, heights, m * 4); st.out(d_count, &count, 4, outside != nullptr);
  GMR_STAGE_TRY(st, upload);
  GMR_HIP_TRY(hipMemset(d_count, 0, 4));
  rc = gmr::heights_launch(t->terrain, (long long)M, d_points, (long long)stride, d_heights, d_count, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  if (outside) *outside = count;
  return GMR_OK;
}

int gmr_motion_tracker_set_feet(gmr_motion_tracker_t* t, const gmr_feet_config_t* cfg) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  if (!cfg) return gmr_fail(GMR_ERR_ARG, "null configuration");
  if (!cfg->edge_pos || !cfg->scales) return gmr_fail(GMR_ERR_ARG, "null edge_pos / scales");
  if (cfg->num_edges < 1 || cfg->num_edges > GMR_FEET_MAX_EDGES) return gmr_fail(GMR_ERR_ARG, "num_edges = %d outside [1, %d]", cfg->num_edges, GMR_FEET_MAX_EDGES);
  if (cfg->nb < 1 || cfg->nb > (1 << 16)) return gmr_fail(GMR_ERR_ARG, "nb = %d bodies outside [1, 2^16]", cfg->nb);
  gmr::FeetTables Ft;
  for (int f = 0; f < 2; f++) {
    if (cfg->feet_body[f] < 0 || cfg->feet_body[f] >= cfg->nb) return gmr_fail(GMR_ERR_ARG, "feet_body[%d] = %d outside [0, %d)", f, cfg->feet_body[f], cfg->nb);
    Ft.feet_body[f] = cfg->feet_body[f];
  }
  for (int k = 0; k < cfg->num_edges * 3; k++) {
    if (!std::isfinite(cfg->edge_pos[k])) return gmr_fail(GMR_ERR_ARG, "edge_pos[%d][%d] is not finite", k / 3, k % 3);
    Ft.edge[k] = cfg->edge_pos[k];
  }
  const int32_t* lists[2] = {cfg->termination_body, cfg->penalized_body};
  const int counts[2] = {cfg->num_termination, cfg->num_penalized};
  int32_t* dst[2] = {Ft.term_body, Ft.pen_body};
  const char* names[2] = {"termination_body", "penalized_body"};
  for (int w = 0; w < 2; w++) {
    if (counts[w] < 0 || counts[w] > GMR_FEET_MAX_BODIES) return gmr_fail(GMR_ERR_ARG, "%s: %d entries outside [0, %d]", names[w], counts[w], GMR_FEET_MAX_BODIES);
    if (counts[w] > 0 && !lists[w]) return gmr_fail(GMR_ERR_ARG, "%s: null list of %d entries", names[w], counts[w]);
    for (int j = 0; j < counts[w]; j++) {
      if (lists[w][j] < 0 || lists[w][j] >= cfg->nb) return gmr_fail(GMR_ERR_ARG, "%s[%d] = %d outside [0, %d)", names[w], j, lists[w][j], cfg->nb);
      for (int i = 0; i < j; i++)
        if (lists[w][i] == lists[w][j]) return gmr_fail(GMR_ERR_ARG, "%s names body %d twice", names[w], lists[w][j]);
      dst[w][j] = lists[w][j];
    }
  }
  const double sc[4] = {cfg->force_threshold, cfg->contact_clearance, cfg->feet_distance_ref, cfg->swing_period};
  for (int k = 0; k < 4; k++)
    if (!std::isfinite(sc[k]) || !std::isfinite((float)sc[k]))
      return gmr_fail(GMR_ERR_ARG, "force_threshold, contact_clearance, feet_distance_ref and swing_period must be finite");
  for (int k = 0; k < GMR_FEET_TERMS; k++) {
    if (!std::isfinite(cfg->scales[k])) return gmr_fail(GMR_ERR_ARG, "scales[%d] is not finite", k);
    Ft.scale[k] = cfg->scales[k];
  }
  Ft.E = cfg->num_edges; Ft.nb = cfg->nb; Ft.n_term = cfg->num_termination; Ft.n_pen = cfg->num_penalized;
  Ft.threshold = (float)cfg->force_threshold; Ft.clearance = (float)cfg->contact_clearance;
  Ft.distance_ref = (float)cfg->feet_distance_ref; Ft.half_swing = (float)(0.5 * cfg->swing_period);       // t1.py:725, :728
  std::lock_guard<std::mutex> g(t->mu);
  const size_t n = (size_t)t->N;
  gmr::Carve cv;
  const size_t o_last = cv.take(n * 24), o_gait = cv.take(n * 4);
  const int rc = gmr::fresh_block(t->feet_block, cv);
  if (rc != GMR_OK) return rc;
  char* d = t->feet_block.data();
  t->feet = Ft;
  t->feet_state = gmr::FeetState{(float*)(d + o_last), (float*)(d + o_gait)};
  return GMR_OK;
}

int gmr_motion_tracker_feet_dev(gmr_motion_tracker_t* t, const gmr_tracker_links_sim_t* bodies, const gmr_feet_in_t* in, const gmr_feet_out_t* out,
                                void* stream) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  gmr::FeetView V;
  {
    std::lock_guard<std::mutex> g(t->mu);
    V = gmr::feet_view(t);
  }
  return gmr::feet_launch(t, V, bodies, in, out, (hipStream_t)stream);
}

int gmr_motion_tracker_feet(gmr_motion_tracker_t* t, const gmr_tracker_links_sim_t* bodies, const gmr_feet_in_t* in, const gmr_feet_out_t* out) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const gmr::FeetView V = gmr::feet_view(t);
  long long es[2], bs[2];
  int rc = gmr::feet_check(V.tab, bodies, in, out, es, bs);
  if (rc != GMR_OK) return rc;
  const size_t n = (size_t)t->N, nb = (size_t)V.tab.nb;
  gmr::HostStage st;
  gmr_tracker_links_sim_t dbodies{nullptr, nullptr, nullptr, nullptr, bodies->env_stride, bodies->body_stride};
  gmr_feet_in_t din = {};
  gmr_feet_out_t dout = {};
  // the two body arrays (their extent from the strides) may interleave in one tensor
  st.in_shared(dbodies.body_pos, bodies->body_pos, 4 * ((n - 1) * (size_t)es[0] + (nb - 1) * (size_t)bs[0] + 3));
  st.in_shared(dbodies.body_rot, bodies->body_rot, 4 * ((n - 1) * (size_t)es[1] + (nb - 1) * (size_t)bs[1] + 4));
  st.in(din.contact_forces, in->contact_forces, n * nb * 12); st.in(din.root_states, in->root_states, n * 52);
  st.in(din.episode_steps, in->episode_steps, n * 4); st.in(din.gait_frequency, in->gait_frequency, n * 4);
  st.out(dout.feet_pos, out->feet_pos, n * 24); st.out(dout.feet_roll, out->feet_roll, n * 8); st.out(dout.feet_yaw, out->feet_yaw, n * 8);
  st.out(dout.feet_contact, out->feet_contact, n * 8); st.out(dout.ground, out->ground, n * 4); st.out(dout.gait, out->gait, n * 8);
  st.out(dout.term, out->term, n * GMR_FEET_TERMS * 4); st.out(dout.total, out->total, n * 4); st.out(dout.done, out->done, n * 4);
  GMR_STAGE_TRY(st, upload);
  rc = gmr::feet_launch(t, V, &dbodies, &din, &dout, nullptr);
  if (rc != GMR_OK) return rc;
  GMR_STAGE_TRY(st, download);
  return GMR_OK;
}

int gmr_motion_tracker_feet_state(gmr_motion_tracker_t* t, float* last_feet_pos, float* gait_process) {
  if (!t) return gmr_fail(GMR_ERR_ARG, "null motion tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const int rc = gmr::feet_set(t->feet);
  if (rc != GMR_OK) return rc;
  const size_t n = (size_t)t->N;
  return gmr::read_back({{last_feet_pos, t->feet_state.last_feet_pos, n * 24}, {gait_process, t->feet_state.gait_process, n * 4}});
}

}  // extern "C"
