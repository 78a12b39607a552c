// gmr_ik_host.hip -- the IK solver handle and the host side of the IK launches of the C-ABI (include/gmr_hip.h): which kernel
// shape a launch takes, the checks of a job, and the three ways host buffers travel -- directly (pinned staging for small
// calls), in slices of streams and in windows of frames.  What the arrays of a job are, where they lie in a workspace and which
// copies move them is stated in gmr_ik_stage.h; the launchers are declared in gmr_launch.h.  No compute happens here.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_ik_layout.h"
#include "gmr_ik_stage.h"
#include "gmr_ik_weight_stage.h"
#include "gmr_ik_wide_layout.h"
#include "gmr_internal.h"
#include "gmr_launch.h"
#include "gmr_workspace.h"

#define fail gmr_fail

struct gmr_solver {
  gmr_model_t model;
  gmr_taskset_t ts;
  gmr::IkLayout layout;          // one wave per stream (many streams)
  gmr::IkLayout layout4;         // main wave + 3 helpers per stream (few streams: latency shape)
  gmr::DeviceBlock image4;
  int force_waves = 0;           // 0 = choose by stream count, 1 or 4 = forced (gmr_solver_set_waves)
  double vmax[GMR_MAX_HINGES];   // velocity limit of every hinge, rad/s; +inf = none (gmr_solver_set_velocity_limits)
  int vlim = 0;                  // some hinge has a finite one: the latency kernel's instances that clamp (gmr_ik.hip: VLIM)
  double fvmax[GMR_MAX_HINGES];  // frame velocity limit of every hinge, rad/s; +inf = none (gmr_solver_set_frame_velocity_limits)
  double frame_dt = 0.0;         // seconds between two frames of a stream; 0 while no hinge has a finite frame limit
  int flim = 0;                  // some hinge has a finite one: the VLIM instances again, and the throughput kernel's with GMR_FWIN
  gmr::IkParams params;
  gmr::DeviceBlock image;        // host-built LDS image of the constants (gmr_ik_layout.h)
  gmr::WideLayout wide;          // throughput shape (gmr_ik_wide.hip): ok = 0 when the robot does not fit it
  gmr::DeviceBlock wide_image;   // its global image of the constants
  void* wide_pool = nullptr;     // queue workspaces of its queued dispatch mode (one per HIP stream)
  gmr::DeviceBlock ws;           // grow-only device workspace of the host-buffer entry point
  char* pin = nullptr;           // pinned host staging for small calls (one H2D + one D2H per call)
  static constexpr size_t kPinBytes = 1u << 20;
  // the sliced host pipeline (gmr_retarget_group): HIP streams and one device workspace per slice in flight
  static constexpr int kPipe = 4;
  hipStream_t pipe_stream[kPipe] = {nullptr, nullptr, nullptr, nullptr};
  gmr::DeviceBlock pipe_ws[kPipe];
};

extern "C" {

// ---- solver ---------------------------------------------------------------------------------
static int validate(const gmr_model_t* m, const gmr_taskset_t* t) {
  if (!m || !t) return fail(GMR_ERR_ARG, "null model/taskset");
  if (m->magic != GMR_MAGIC_MODEL || m->version != GMR_ABI_VERSION) return fail(GMR_ERR_ARG, "bad model blob");
  if (t->magic != GMR_MAGIC_TASKSET || t->version != GMR_ABI_VERSION) return fail(GMR_ERR_ARG, "bad taskset blob");
  if (m->nbody < 1 || m->nbody > GMR_MAX_BODIES || m->nbody > 64) return fail(GMR_ERR_ARG, "nbody out of range");
  if (m->nhinge < 0 || m->nhinge > GMR_MAX_HINGES) return fail(GMR_ERR_ARG, "nhinge out of range");
  if (m->nv != m->nhinge + 6 || m->nq != m->nhinge + 7 || m->nv > GMR_MAX_DOF) return fail(GMR_ERR_ARG, "nq/nv inconsistent");
  if (!(m->timestep > 0.0)) return fail(GMR_ERR_ARG, "timestep must be positive");
  if (m->parent[0] != -1) return fail(GMR_ERR_ARG, "body 0 must be the root");
  for (int b = 1; b < m->nbody; b++) {
    if (m->parent[b] < 0 || m->parent[b] >= b) return fail(GMR_ERR_ARG, "parent[%d] invalid", b);
    if (m->depth[b] != m->depth[m->parent[b]] + 1 || m->depth[b] >= GMR_MAX_DEPTH)
      return fail(GMR_ERR_ARG, "depth[%d] invalid", b);
    for (int d = 0; d <= m->depth[b]; d++)
      if (m->chain[b][d] < 0 || m->chain[b][d] >= m->nbody) return fail(GMR_ERR_ARG, "chain[%d][%d] invalid", b, d);
    if (m->chain[b][m->depth[b]] != b) return fail(GMR_ERR_ARG, "chain[%d] does not end at the body", b);
    if (m->body_hinge[b] < -1 || m->body_hinge[b] >= m->nhinge) return fail(GMR_ERR_ARG, "body_hinge[%d] invalid", b);
  }
  for (int h = 0; h < m->nhinge; h++)
    if (m->hinge_body[h] < 1 || m->hinge_body[h] >= m->nbody || m->body_hinge[m->hinge_body[h]] != h)
      return fail(GMR_ERR_ARG, "hinge_body[%d] invalid", h);
  if (t->nhuman < 1 || t->nhuman > GMR_MAX_HUMAN || t->human_root < 0 || t->human_root >= t->nhuman)
    return fail(GMR_ERR_ARG, "nhuman/human_root out of range");
  for (int s = 0; s < 2; s++) {
    if (t->ntask[s] < 0 || t->ntask[s] > GMR_MAX_TASKS) return fail(GMR_ERR_ARG, "ntask out of range");
    if (t->use_stage[s] && t->ntask[s] == 0) return fail(GMR_ERR_ARG, "stage %d enabled without tasks", s + 1);
    if (t->npair[s] < 0 || t->npair[s] > GMR_MAX_PAIRS) return fail(GMR_ERR_ARG, "npair out of range");
    int p = 0;
    for (int k = 0; k < t->ntask[s]; k++) {
      if (t->task_body[s][k] < 0 || t->task_body[s][k] >= m->nbody) return fail(GMR_ERR_ARG, "task body invalid");
      if (t->task_human[s][k] < 0 || t->task_human[s][k] >= t->nhuman) return fail(GMR_ERR_ARG, "task human invalid");
      if (t->task_col0[s][k] != p) return fail(GMR_ERR_ARG, "task_col0 not contiguous");
      int n = t->task_ncol[s][k];
      if (n < 3 || p + n > t->npair[s]) return fail(GMR_ERR_ARG, "task_ncol invalid");   // (base translations may be pruned)
      for (int c = 0; c < n; c++) {
        int d = t->pair_dof[s][p + c];
        if (t->pair_task[s][p + c] != k || d < 0 || d >= m->nv) return fail(GMR_ERR_ARG, "pair table invalid");
        if (c > 0 && d <= t->pair_dof[s][p + c - 1]) return fail(GMR_ERR_ARG, "pair dofs not ascending");
        if (t->pair_index[s][k][d] != p + c) return fail(GMR_ERR_ARG, "pair_index inconsistent");
      }
      p += n;
    }
    if (p != t->npair[s]) return fail(GMR_ERR_ARG, "npair inconsistent");
  }
  if (t->max_iter < 0 || t->max_iter > 1000) return fail(GMR_ERR_ARG, "max_iter out of range");
  return GMR_OK;
}

int gmr_solver_create(const gmr_model_t* model, const gmr_taskset_t* taskset, gmr_solver_t** out) {
  if (!out) return fail(GMR_ERR_ARG, "null out pointer");
  int rc = validate(model, taskset);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GMR_ERR_NO_DEVICE, "no HIP device visible");
  gmr_solver* s = new (std::nothrow) gmr_solver;
  if (!s) return fail(GMR_ERR_ARG, "out of host memory");
  s->model = *model;
  s->ts = *taskset;
  std::fill(s->vmax, s->vmax + GMR_MAX_HINGES, (double)INFINITY);
  std::fill(s->fvmax, s->fvmax + GMR_MAX_HINGES, (double)INFINITY);
  if (gmr::ik_padded_nv(s->model.nv) < 0) { delete s; return fail(GMR_ERR_ARG, "nv = %d > 48 is not supported", s->model.nv); }
  s->params = gmr::make_ik_params(s->model, s->ts);
  hipError_t e = hipSuccess;
  for (int v = 0; v < 2 && e == hipSuccess; v++) {
    const int nw = v == 0 ? 1 : 4;
    gmr::IkSchedule sch = gmr::make_ik_schedule(s->model, s->ts, v == 0 ? 64 : 64 * (nw - 1));
    gmr::IkLayout& lay = v == 0 ? s->layout : s->layout4;
    lay = gmr::make_ik_layout(s->model, s->ts, sch, nw);
    // a robot that does not decompose is never launched with helpers (gmr_retarget_streams_dev): its 4-wavefront layout,
    // whose schedule lives in LDS and grows with the task set, is neither checked nor uploaded.  layout4 keeps tree_ok = 0.
    if (nw == 4 && !lay.tree_ok) continue;
    if (lay.smem_bytes > 160 * 1024 - 1024) {
      delete s;
      return fail(GMR_ERR_ARG, "robot too large for LDS: the %d-wavefront layout needs %d bytes of %d", nw, lay.smem_bytes, 160 * 1024 - 1024);
    }
    std::vector<char> img = gmr::make_ik_image(s->model, s->ts, sch, lay);
    gmr::DeviceBlock& dst = v == 0 ? s->image : s->image4;
    if ((e = dst.reserve(img.size())) != hipSuccess) break;
    if ((e = hipMemcpy(dst.data(), img.data(), img.size(), hipMemcpyHostToDevice)) != hipSuccess) break;
    e = gmr_ik_set_max_smem(lay.nvp, nw, lay.tree_small, lay.smem_bytes);
  }
  s->wide = gmr::WideLayout{};
  if (e == hipSuccess && !getenv("GMR_IK_NO_WIDE")) {   // (diagnostic switch: A/B against the one-wavefront kernel of gmr_ik.hip)
    std::vector<char> img;
    s->wide = gmr::make_wide_layout(s->model, s->ts, &img);
    if (s->wide.ok) {
      if ((e = s->wide_image.reserve(img.size())) == hipSuccess)
        e = hipMemcpy(s->wide_image.data(), img.data(), img.size(), hipMemcpyHostToDevice);
      if (e == hipSuccess) s->wide_pool = gmr_ik_wide_pool_create();
    }
  }
  if (e != hipSuccess) {
    gmr_ik_wide_pool_destroy(s->wide_pool);
    delete s;
    return fail(GMR_ERR_HIP, "gmr_solver_create: %s", hipGetErrorString(e));
  }
  *out = s;
  return GMR_OK;
}

int gmr_solver_destroy(gmr_solver_t* s) {
  if (!s) return GMR_OK;
  gmr_ik_wide_pool_destroy(s->wide_pool);
  if (s->pin) (void)hipHostFree(s->pin);
  for (int i = 0; i < gmr_solver::kPipe; i++)
    if (s->pipe_stream[i]) { (void)hipStreamSynchronize(s->pipe_stream[i]); (void)hipStreamDestroy(s->pipe_stream[i]); }
  delete s;
  return GMR_OK;
}

int gmr_solver_dims(const gmr_solver_t* s, int* nq, int* nv, int* nhuman) {
  if (!s) return fail(GMR_ERR_ARG, "null solver");
  if (nq) *nq = s->model.nq;
  if (nv) *nv = s->model.nv;
  if (nhuman) *nhuman = s->ts.nhuman;
  return GMR_OK;
}

int gmr_solver_set_waves(gmr_solver_t* s, int waves_per_stream) {
  if (!s) return fail(GMR_ERR_ARG, "null solver");
  if (waves_per_stream != 0 && waves_per_stream != 1 && waves_per_stream != 4)
    return fail(GMR_ERR_ARG, "waves_per_stream must be 0 (auto), 1 or 4");
  s->force_waves = waves_per_stream;
  return GMR_OK;
}

int gmr_solver_set_dispatch(gmr_solver_t* s, int frames_per_item) {
  if (!s) return fail(GMR_ERR_ARG, "null solver");
  if (frames_per_item < 0) return fail(GMR_ERR_ARG, "frames_per_item must be >= 0");
  if (s->wide_pool) gmr_ik_wide_pool_set_chunk(s->wide_pool, frames_per_item);
  return GMR_OK;
}

// The velocity bounds are one table of vmax * timestep per dof in each of the solver's device images (gmr_ik_layout.h:
// IK_VDT_N, gmr_ik_wide_layout.h: WideImg::vdt), written in place: the images keep their addresses, so a job table that
// names them needs no rebuilding.  Launches issued before this call finish on the old table.
int gmr_solver_set_velocity_limits(gmr_solver_t* s, const double* vmax, int n) {
  if (!s) return fail(GMR_ERR_ARG, "null solver");
  const int nh = s->model.nhinge;
  if (vmax ? n != nh : (n != 0 && n != nh)) return fail(GMR_ERR_ARG, "velocity limits: n = %d, the robot has %d hinges", n, nh);
  for (int h = 0; vmax && h < nh; h++)
    if (!(vmax[h] > 0.0)) return fail(GMR_ERR_ARG, "velocity limit of hinge %d is %g: must be positive (+inf = none)", h, vmax[h]);
  double next[GMR_MAX_HINGES];
  for (int h = 0; h < GMR_MAX_HINGES; h++) next[h] = vmax && h < nh ? vmax[h] : (double)INFINITY;
  double vdt[64];
  gmr::ik_fill_vdt(s->model, next, vdt, 64);
  GMR_NAMED_HIP_TRY("velocity limits", hipDeviceSynchronize());
  if (s->image.data()) GMR_NAMED_HIP_TRY("velocity limits", hipMemcpy(s->image.data() + s->layout.smem_bytes, vdt, gmr::IK_VDT_N * 8, hipMemcpyHostToDevice));
  if (s->layout4.tree_ok && s->image4.data())
    GMR_NAMED_HIP_TRY("velocity limits", hipMemcpy(s->image4.data() + s->layout4.smem_bytes, vdt, gmr::IK_VDT_N * 8, hipMemcpyHostToDevice));
  if (s->wide.ok) GMR_NAMED_HIP_TRY("velocity limits", hipMemcpy(s->wide_image.data() + gmr::wide_img().vdt, vdt, 64 * 8, hipMemcpyHostToDevice));
  memcpy(s->vmax, next, sizeof next);
  s->vlim = 0;
  for (int h = 0; h < nh; h++) s->vlim |= std::isfinite(next[h]) ? 1 : 0;
  return GMR_OK;
}

int gmr_solver_velocity_limits(const gmr_solver_t* s, double* vmax_out, int n) {
  if (!s) return fail(GMR_ERR_ARG, "null solver");
  if (!vmax_out || n != s->model.nhinge) return fail(GMR_ERR_ARG, "velocity limits: n = %d, the robot has %d hinges", n, s->model.nhinge);
  memcpy(vmax_out, s->vmax, (size_t)n * sizeof(double));
  return GMR_OK;
}

// The frame windows are a second table per dof, vmax_frame * frame_dt, right behind the velocity bounds in the latency images
// and in WideImg::fw of the throughput image.  Written in place under the contract of gmr_solver_set_velocity_limits above.
int gmr_solver_set_frame_velocity_limits(gmr_solver_t* s, const double* vmax, int n, double frame_dt) {
  if (!s) return fail(GMR_ERR_ARG, "null solver");
  const int nh = s->model.nhinge;
  if (vmax ? n != nh : (n != 0 && n != nh)) return fail(GMR_ERR_ARG, "frame velocity limits: n = %d, the robot has %d hinges", n, nh);
  int finite = 0;
  for (int h = 0; vmax && h < nh; h++) {
    if (!(vmax[h] > 0.0)) return fail(GMR_ERR_ARG, "frame velocity limit of hinge %d is %g: must be positive (+inf = none)", h, vmax[h]);
    finite |= std::isfinite(vmax[h]) ? 1 : 0;
  }
  if (finite && !(std::isfinite(frame_dt) && frame_dt > 0.0))
    return fail(GMR_ERR_ARG, "frame_dt is %g: must be finite and positive while a frame velocity limit is", frame_dt);
  double next[GMR_MAX_HINGES];
  for (int h = 0; h < GMR_MAX_HINGES; h++) next[h] = vmax && h < nh ? vmax[h] : (double)INFINITY;
  double fw[64];
  gmr::ik_fill_frame_window(s->model, next, frame_dt, fw, 64);
  GMR_NAMED_HIP_TRY("frame velocity limits", hipDeviceSynchronize());
  if (s->image.data())
    GMR_NAMED_HIP_TRY("frame velocity limits", hipMemcpy(s->image.data() + s->layout.smem_bytes + gmr::IK_VDT_N * 8, fw, gmr::IK_VDT_N * 8, hipMemcpyHostToDevice));
  if (s->layout4.tree_ok && s->image4.data())
    GMR_NAMED_HIP_TRY("frame velocity limits", hipMemcpy(s->image4.data() + s->layout4.smem_bytes + gmr::IK_VDT_N * 8, fw, gmr::IK_VDT_N * 8, hipMemcpyHostToDevice));
  if (s->wide.ok) GMR_NAMED_HIP_TRY("frame velocity limits", hipMemcpy(s->wide_image.data() + gmr::wide_img().fw, fw, 64 * 8, hipMemcpyHostToDevice));
  memcpy(s->fvmax, next, sizeof next);
  s->frame_dt = finite ? frame_dt : 0.0;
  s->flim = finite;
  return GMR_OK;
}

int gmr_solver_frame_velocity_limits(const gmr_solver_t* s, double* vmax_out, int n, double* frame_dt_out) {
  if (!s) return fail(GMR_ERR_ARG, "null solver");
  if (!vmax_out || n != s->model.nhinge) return fail(GMR_ERR_ARG, "frame velocity limits: n = %d, the robot has %d hinges", n, s->model.nhinge);
  memcpy(vmax_out, s->fvmax, (size_t)n * sizeof(double));
  if (frame_dt_out) *frame_dt_out = s->frame_dt;
  return GMR_OK;
}

int gmr_retarget_lds_bytes(const gmr_solver_t* s) { return !s ? 0 : s->layout4.tree_ok ? s->layout4.smem_bytes : s->layout.smem_bytes; }


// ---- one job: its checks, its launch ----------------------------------------------------------------------------------------
static bool has_work(const gmr_job_t& J) { return J.S > 0 && J.T > 0; }

// What every entry point asks of a job, in this order: a solver, S and T not negative -- a job without streams or frames is
// not looked at further -- every mandatory buffer, and, for host buffers (the device entry points cannot look), every entry of
// a scale table finite and positive and every body weight finite and not negative.  j >= 0 puts "job j: " in front of the message.
// `weight`: the job's per-frame body weights [S][T][nhuman] or null; they travel beside the job (gmr_ik_weight_stage.h).
static int check_job(const gmr_job_t& J, const double* weight, bool host, int j) {
  char pre[24] = "";
  if (j >= 0) snprintf(pre, sizeof pre, "job %d: ", j);
  if (!J.solver) return fail(GMR_ERR_ARG, "%snull solver", pre);
  if (J.S < 0 || J.T < 0) return fail(GMR_ERR_ARG, "%snegative S/T", pre);
  if (!has_work(J)) return GMR_OK;
  for (int f = 0; f < gmr::IK_NFIELD; f++)
    if (!gmr::kIkFields[f].optional && !gmr::ik_ptr(J, f)) return fail(GMR_ERR_ARG, "%snull %s buffer", pre, host ? "host" : "device");
  const size_t nh = (size_t)J.solver->ts.nhuman;
  for (size_t i = 0; host && J.scale && i < (size_t)J.S * nh; i++)
    if (!(J.scale[i] > 0.0) || !std::isfinite(J.scale[i]))
      return fail(GMR_ERR_ARG, "%sscale of stream %d, body %d is %g: must be finite and positive", pre, (int)(i / nh), (int)(i % nh), J.scale[i]);
  // (only the frames a stream has: rows at or beyond len[s] are padding that no kernel reads, like the human rows there)
  for (int s = 0; host && weight && s < J.S; s++) {
    const size_t Ts = (size_t)(J.len ? std::min(std::max(J.len[s], 0), J.T) : J.T);
    const double* w = weight + (size_t)s * J.T * nh;
    for (size_t i = 0; i < Ts * nh; i++)
      if (!(w[i] >= 0.0) || !std::isfinite(w[i]))
        return fail(GMR_ERR_ARG, "%sweight of stream %d, frame %d, body %d is %g: must be finite and not negative", pre, s, (int)(i / nh),
                    (int)(i % nh), w[i]);
  }
  return GMR_OK;
}

// a list of jobs: the first bad one reports; what the jobs with work add up to
struct Batch {
  long long total = 0;           // streams
  size_t in_bytes = 0;           // of the per-frame inputs: the human frames and the body weights a job carries
  int njobs = 0, maxT = 0;
  gmr_solver* owner = nullptr;   // the first of their solvers: its pipeline streams, workspaces and queue pool serve the batch
};
static const double* weight_of(const double* const* weight, int j) { return weight ? weight[j] : nullptr; }
static int check_jobs(const gmr_job_t* jobs, int njobs, const double* const* weight, bool host, Batch* b) {
  if (njobs < 0 || (njobs > 0 && !jobs)) return fail(GMR_ERR_ARG, "bad job list");
  for (int j = 0; j < njobs; j++) {
    const gmr_job_t& J = jobs[j];
    if (int rc = check_job(J, weight_of(weight, j), host, j)) return rc;
    if (!has_work(J)) continue;
    if (!b->owner) b->owner = J.solver;
    b->total += J.S;
    b->in_bytes += (size_t)J.S * J.T * (gmr::kIkFields[gmr::IK_HUMAN].per_nhuman + (weight_of(weight, j) ? 8 : 0)) * J.solver->ts.nhuman;
    b->njobs++;
    b->maxT = std::max(b->maxT, (int)J.T);
  }
  return GMR_OK;
}

// the throughput shape (two resident wavefronts per SIMD, gmr_ik_wide.hip) at a launch width of `streams`
static bool job_takes_wide_shape(const gmr_solver* s, long long streams) {
  return gmr::ik_throughput_shape(s->layout4.tree_ok, s->force_waves, streams, s->wide.ok);
}
static gmr_wide_job_desc wide_desc(const gmr_job_t& J, const double* d_weight) {
  gmr_solver* s = J.solver;
  return gmr_wide_job_desc{s->wide_image.data(), &s->wide, &s->params, J.S, J.T, J.q0, J.human, J.len, J.q_out, J.nsolve, J.status,
                           J.tgt_out, J.err_out, J.scale, s->flim, d_weight};
}
// a checked job with work, by itself (d_weight: its body weights on the device or null; d_prof: diagnostic builds)
static int launch_job(const gmr_job_t& J, const double* d_weight, int flags, hipStream_t stream, unsigned long long* d_prof = nullptr) {
  gmr_solver* s = J.solver;
  const bool helpers = gmr::ik_helpers_shape(s->layout4.tree_ok, s->force_waves, J.S);
  if (job_takes_wide_shape(s, J.S))
    GMR_HIP_TRY(gmr_launch_ik_wide(s->wide_image.data(), &s->wide, &s->params, J.S, J.T, J.q0, J.human, J.len, J.scale, flags, J.q_out,
                                   J.nsolve, J.status, J.tgt_out, J.err_out, stream, d_prof, d_prof ? nullptr : s->wide_pool, s->flim, d_weight));
  else
    GMR_HIP_TRY(gmr_launch_ik_streams((const uint4*)(helpers ? s->image4 : s->image).data(), helpers ? &s->layout4 : &s->layout, &s->params,
                                      J.S, J.T, J.q0, J.human, J.len, J.scale, flags, J.q_out, J.nsolve, J.status, J.tgt_out, J.err_out,
                                      stream, d_prof, s->vlim | s->flim, d_weight));
  return GMR_OK;
}

int gmr_retarget_streams_dev(gmr_solver_t* s, int S, int T, const double* d_q0, const double* d_human, const int32_t* d_len, int flags,
                             double* d_q_out, int32_t* d_nsolve, int32_t* d_status, double* d_tgt_out, double* d_err_out, void* stream) {
  return gmr_retarget_streams_weighted_dev(s, S, T, d_q0, d_human, d_len, nullptr, nullptr, flags, d_q_out, d_nsolve, d_status, d_tgt_out, d_err_out, stream);
}

int gmr_retarget_streams_scaled_dev(gmr_solver_t* s, int S, int T, const double* d_q0, const double* d_human, const int32_t* d_len,
                                    const double* d_scale, int flags, double* d_q_out, int32_t* d_nsolve, int32_t* d_status,
                                    double* d_tgt_out, double* d_err_out, void* stream) {
  return gmr_retarget_streams_weighted_dev(s, S, T, d_q0, d_human, d_len, d_scale, nullptr, flags, d_q_out, d_nsolve, d_status, d_tgt_out, d_err_out, stream);
}

int gmr_retarget_streams_weighted_dev(gmr_solver_t* s, int S, int T, const double* d_q0, const double* d_human, const int32_t* d_len,
                                      const double* d_scale, const double* d_weight, int flags, double* d_q_out, int32_t* d_nsolve,
                                      int32_t* d_status, double* d_tgt_out, double* d_err_out, void* stream) {
  const gmr_job_t job{s, S, T, d_q0, d_human, d_len, d_q_out, d_nsolve, d_status, d_tgt_out, d_err_out, d_scale};
  if (int rc = check_job(job, d_weight, false, -1)) return rc;
  return has_work(job) ? launch_job(job, d_weight, flags, (hipStream_t)stream) : GMR_OK;
}

#ifdef GMR_IK_PROFILE
// diagnostic builds only (tools/phase_profile.py): per-stream phase cycle counters
int gmr_retarget_streams_prof(gmr_solver_t* s, int S, int T, const double* d_q0, const double* d_human, int flags,
                              double* d_q_out, int32_t* d_nsolve, int32_t* d_status, unsigned long long* d_prof) {
  return launch_job(gmr_job_t{s, S, T, d_q0, d_human, nullptr, d_q_out, d_nsolve, d_status, nullptr, nullptr, nullptr}, nullptr, flags, nullptr, d_prof);
}
#endif

// ---- group launches: several (robot, task set) jobs as one scheduling domain ---------------------------------------
int gmr_retarget_group_dev(const gmr_job_t* jobs, int njobs, int flags, void* stream) {
  return gmr_retarget_group_weighted_dev(jobs, njobs, nullptr, flags, stream);
}

// weight: null, or njobs entries, each null or the job's body weights [S][T][nhuman] on the device
int gmr_retarget_group_weighted_dev(const gmr_job_t* jobs, int njobs, const double* const* weight, int flags, void* stream) {
  Batch b;
  if (int rc = check_jobs(jobs, njobs, weight, false, &b)) return rc;
  // The throughput kernel is one instance for every robot of its size class: all jobs that take that shape at this
  // width (the width of the GROUP decides, not a job's own) go out as launches of up to 8 jobs; the others -- robots
  // that do not decompose, solvers forced to the latency shape, groups too small for the throughput shape -- one by one.
  gmr_wide_job_desc wd[8];
  int nw = 0;
  void* pool = nullptr;
  auto flush = [&]() -> int {
    if (nw == 0) return GMR_OK;
    hipError_t e = gmr_launch_ik_wide_group(wd, nw, flags, (hipStream_t)stream, nullptr, pool);
    nw = 0;
    if (e != hipSuccess) return fail(GMR_ERR_HIP, "group launch: %s", hipGetErrorString(e));
    return GMR_OK;
  };
  for (int j = 0; j < njobs; j++) {
    const gmr_job_t& J = jobs[j];
    if (!has_work(J)) continue;
    if (njobs > 1 && job_takes_wide_shape(J.solver, b.total)) {
      if (nw == 0) pool = J.solver->wide_pool;
      wd[nw++] = wide_desc(J, weight_of(weight, j));
      if (nw == 8) { int rc = flush(); if (rc) return rc; }
    } else if (int rc = launch_job(J, weight_of(weight, j), flags, (hipStream_t)stream)) {
      return rc;
    }
  }
  return flush();
}

// One WINDOW of every stream's frames: [t_begin, t_end).  The windows of a batch must be launched in order on ONE stream,
// starting at t_begin = 0; the per-stream state between them (QP bound sets, status) stays in the first job's workspace of
// that stream; q continues from the previous window's last q_out row.  Only batches that take the throughput shape as a
// whole (every job's robot decomposes, more than 300 streams, no solver forced to four wavefronts) can be windowed.
static bool group_is_windowable(const gmr_job_t* jobs, int njobs, const Batch& b) {
  if (b.njobs == 0 || b.njobs > 8) return false;
  for (int j = 0; j < njobs; j++)
    if (has_work(jobs[j]) && !job_takes_wide_shape(jobs[j].solver, b.total)) return false;
  return true;
}

int gmr_retarget_group_window_dev(const gmr_job_t* jobs, int njobs, int flags, int t_begin, int t_end, void* stream) {
  return gmr_retarget_group_weighted_window_dev(jobs, njobs, nullptr, flags, t_begin, t_end, stream);
}

int gmr_retarget_group_weighted_window_dev(const gmr_job_t* jobs, int njobs, const double* const* weight, int flags, int t_begin,
                                           int t_end, void* stream) {
  const bool list_ok = njobs >= 0 && (njobs == 0 || jobs);       // (a bad list reports first, from check_jobs)
  if (list_ok && (t_begin < 0 || t_end <= t_begin)) return fail(GMR_ERR_ARG, "bad window [%d, %d)", t_begin, t_end);
  Batch b;
  if (int rc = check_jobs(jobs, njobs, weight, false, &b)) return rc;
  if (!group_is_windowable(jobs, njobs, b)) return fail(GMR_ERR_ARG, "this batch does not take the throughput shape as a whole: launch it unwindowed");
  gmr_wide_job_desc wd[8];
  int nw = 0;
  for (int j = 0; j < njobs; j++)
    if (has_work(jobs[j])) wd[nw++] = wide_desc(jobs[j], weight_of(weight, j));
  hipError_t e = gmr_launch_ik_wide_window(wd, nw, flags, (hipStream_t)stream, nullptr, b.owner->wide_pool, t_begin, t_end);
  if (e != hipSuccess) return fail(GMR_ERR_HIP, "window launch: %s", hipGetErrorString(e));
  return GMR_OK;
}

// ---- host buffers -------------------------------------------------------------------------------------------------------------
static gmr::IkJobOff carve_job(gmr::Carve& c, const gmr_job_t& J, size_t S) {
  return gmr::ik_carve_job(c, J, (size_t)J.solver->model.nq, (size_t)J.solver->ts.nhuman, S);
}
// S streams of a job's body weights, in front of the job's own arrays (gmr_ik_weight_stage.h)
static gmr::IkWeightOff carve_weight(gmr::Carve& c, const gmr_job_t& J, const double* weight, size_t S) {
  return gmr::ik_carve_weight(c, weight, (size_t)J.solver->ts.nhuman, S, (size_t)J.T);
}
// n (0 or 1) copies of the host array `weight` into the device block d, on `st`
static int issue_weight(const gmr::IkCopy* c, int n, const double* weight, char* d, hipStream_t st, const char* what) {
  for (int i = 0; i < n; i++) {
    const char* h = reinterpret_cast<const char*>(weight) + c[i].host;
    const hipError_t e = c[i].rows == 1 ? hipMemcpyAsync(d + c[i].dev, h, c[i].width, hipMemcpyHostToDevice, st)
                                        : hipMemcpy2DAsync(d + c[i].dev, c[i].pitch, h, c[i].pitch, c[i].width, c[i].rows, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(GMR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  }
  return GMR_OK;
}
// the copies c[0 .. n) between the host arrays of J and the device block d, on `st`; a failure reports as "<what>: ..."
static int issue(const gmr::IkCopy* c, int n, const gmr_job_t& J, char* d, hipStream_t st, const char* what) {
  for (int i = 0; i < n; i++) {
    const bool out = gmr::kIkFields[c[i].field].out;
    char *h = gmr::ik_ptr(J, c[i].field) + c[i].host, *dev = d + c[i].dev;
    const hipMemcpyKind kind = out ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    const hipError_t e = c[i].rows == 1 ? hipMemcpyAsync(out ? h : dev, out ? dev : h, c[i].width, kind, st)
                                        : hipMemcpy2DAsync(out ? h : dev, c[i].pitch, out ? dev : h, c[i].pitch, c[i].width, c[i].rows, kind, st);
    if (e != hipSuccess) return fail(GMR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  }
  return GMR_OK;
}
// Frames at or beyond len[s] are not touched by the kernel, nor are the tgt_out / err_out rows of the frames after a stream's
// status turned non-OK (err_out: including the failing frame): they go back as zeros, never as what an earlier call left in
// a grow-only workspace.  On the stream the kernel runs on, before the launch.
static int zero_outputs(const gmr_job_t& J, char* d, const gmr::IkJobOff& o, hipStream_t st) {
  if (J.len || J.tgt_out || J.err_out) GMR_NAMED_HIP_TRY("memset", hipMemsetAsync(d + o.out_begin(), 0, o.end - o.out_begin(), st));
  return GMR_OK;
}

// Host buffers of a LONG, NARROW batch (a few thousand streams of hundreds of frames: BASELINE.json configs[3], a dataset
// batch), overlapped in TIME: the batch is launched as W consecutive windows of frames; the H2D copies of window w + 1
// (strided: a window of a stream's frames is one piece of its row) run under the kernel of window w, the D2H copies of
// window w - 1 likewise.  (Cutting such a batch by streams loses: launches narrower than the resident width are bound by
// their longest stream.)  Three HIP streams, one device workspace holding the whole batch; results are bit-identical to
// one launch -- the per-stream state travels from window to window in device memory.
static int retarget_group_windows(const gmr_job_t* jobs, int njobs, const double* const* weight, int flags, const Batch& b, int W) {
  gmr_solver* owner = b.owner;
  std::vector<gmr::IkJobOff> off((size_t)njobs);
  std::vector<gmr::IkWeightOff> woff((size_t)njobs);
  std::vector<const double*> dw((size_t)njobs, nullptr);      // the jobs' weights on the device
  gmr::Carve need;
  for (int j = 0; j < njobs; j++)
    if (has_work(jobs[j])) {
      woff[j] = carve_weight(need, jobs[j], weight_of(weight, j), (size_t)jobs[j].S);
      off[j] = carve_job(need, jobs[j], (size_t)jobs[j].S);
    }
  for (int i = 0; i < 3; i++)
    if (!owner->pipe_stream[i]) GMR_HIP_TRY(hipStreamCreateWithFlags(&owner->pipe_stream[i], hipStreamNonBlocking));
  hipStream_t s_in = owner->pipe_stream[0], s_k = owner->pipe_stream[1], s_out = owner->pipe_stream[2];
  if (need.total() > owner->pipe_ws[0].size())
    for (int i = 0; i < 3; i++) GMR_HIP_TRY(hipStreamSynchronize(owner->pipe_stream[i]));
  GMR_HIP_TRY(owner->pipe_ws[0].reserve(need.total()));       // exact: this block holds a whole batch
  char* d = owner->pipe_ws[0].data();
  const int wl = gmr::ik_window_frames(b.maxT, W);
  std::vector<gmr_job_t> dj(jobs, jobs + njobs);
  std::vector<hipEvent_t> ev;
  gmr::IkCopy c[gmr::IK_NFIELD], cw;
  int rc = GMR_OK;
  hipError_t e = hipSuccess;
  // an event recorded on `from` that `to` waits for
  auto order = [&](hipStream_t from, hipStream_t to) {
    hipEvent_t x = nullptr;
    if ((e = hipEventCreateWithFlags(&x, hipEventDisableTiming)) != hipSuccess) return e;
    ev.push_back(x);
    if ((e = hipEventRecord(x, from)) == hipSuccess) e = hipStreamWaitEvent(to, x, 0);
    return e;
  };
  // the inputs or the outputs of every job that has frames at tb, in job order: the frames [tb, te), or (te = 0) the per-stream arrays
  auto move = [&](bool out, int tb, int te, hipStream_t st, const char* what) {
    for (int j = 0; j < njobs && rc == GMR_OK; j++)
      if (has_work(jobs[j]) && tb < jobs[j].T) {
        rc = issue(c, te ? gmr::ik_window_copies(off[j], out, tb, te, c) : gmr::ik_slice_copies(off[j], out, 0, c, gmr::IK_PER_STREAM), jobs[j], d, st, what);
        if (rc == GMR_OK && !out && te) rc = issue_weight(&cw, gmr::ik_weight_window_copy(woff[j], tb, te, &cw), weight_of(weight, j), d, st, what);
      }
  };
  move(false, 0, 0, s_in, "H2D copy");                // q0, len, scale: once, before the first window
  for (int j = 0; j < njobs && rc == GMR_OK; j++) {
    if (!has_work(jobs[j])) continue;
    dj[j] = gmr::ik_job_at(jobs[j], d, off[j]);
    dw[j] = gmr::ik_weight_at(d, woff[j]);
    rc = zero_outputs(jobs[j], d, off[j], s_k);
  }
  for (int tb = 0; tb < b.maxT && rc == GMR_OK; tb += wl) {
    const int te = std::min(tb + wl, b.maxT);
    move(false, tb, te, s_in, "H2D window copy");
    if (rc == GMR_OK && (e = order(s_in, s_k)) != hipSuccess) rc = fail(GMR_ERR_HIP, "window events: %s", hipGetErrorString(e));
    if (rc == GMR_OK) rc = gmr_retarget_group_weighted_window_dev(dj.data(), njobs, dw.data(), flags, tb, te, s_k);
    if (rc == GMR_OK && (e = order(s_k, s_out)) != hipSuccess) rc = fail(GMR_ERR_HIP, "window events: %s", hipGetErrorString(e));
    move(true, tb, te, s_out, "D2H window copy");
  }
  move(true, 0, 0, s_out, "D2H copy");                // status: once, at the end
  for (int i = 0; i < 3; i++)                         // on every exit: drain whatever was started, then release the events
    if ((e = hipStreamSynchronize(owner->pipe_stream[i])) != hipSuccess && rc == GMR_OK) rc = fail(GMR_ERR_HIP, "kernel / copies: %s", hipGetErrorString(e));
  for (hipEvent_t x : ev) (void)hipEventDestroy(x);
  return rc;
}

// Host buffers, sliced and overlapped: slice k holds the streams [S_j k / n, S_j (k + 1) / n) of every job; its H2D
// copies, its (group) launch and its D2H copies go to HIP stream k mod 4 in that order, so the copies of one slice run
// under the kernels of its neighbours.  Slices are cut only while every slice still has a few thousand streams: a
// launch narrower than the resident width is bound by its longest stream, and slices that share a HIP stream would
// run those one after the other.  Pinned host memory (gmr_host_alloc / gmr_host_register) makes the copies truly
// asynchronous; pageable memory works, staged by the runtime.
int gmr_retarget_group(const gmr_job_t* jobs, int njobs, int flags, int slices) {
  return gmr_retarget_group_weighted(jobs, njobs, nullptr, flags, slices);
}

// weight: null, or njobs entries, each null or the job's body weights [S][T][nhuman] in host memory: checked here, cut with the
// slices and the windows like the human frames
int gmr_retarget_group_weighted(const gmr_job_t* jobs, int njobs, const double* const* weight, int flags, int slices) {
  Batch b;
  if (int rc = check_jobs(jobs, njobs, weight, true, &b)) return rc;
  gmr_solver* owner = b.owner;
  if (!owner) return GMR_OK;
  const int n = gmr::ik_slice_count(slices, b.total, b.in_bytes);
  // (slices < 0: |slices| windows, the caller's choice)
  if (gmr::ik_cut_in_time(slices, n, b.maxT, b.in_bytes) && group_is_windowable(jobs, njobs, b) && !getenv("GMR_NO_WINDOWS"))
    return retarget_group_windows(jobs, njobs, weight, flags, b, slices < 0 ? -slices : (int)std::min<size_t>(8, b.in_bytes >> 26));
  int rc = GMR_OK;
  hipError_t e = hipSuccess;
  const int nslot = std::min(n, (int)gmr_solver::kPipe);
  for (int i = 0; i < nslot; i++)
    if (!owner->pipe_stream[i]) GMR_HIP_TRY(hipStreamCreateWithFlags(&owner->pipe_stream[i], hipStreamNonBlocking));
  std::vector<gmr_job_t> dj((size_t)njobs);
  std::vector<gmr::IkJobOff> off((size_t)njobs);
  std::vector<int> s0((size_t)njobs);
  std::vector<gmr::IkWeightOff> woff((size_t)njobs);
  std::vector<const double*> dw((size_t)njobs, nullptr);
  gmr::IkCopy c[gmr::IK_NFIELD], cw;
  for (int k = 0; k < n && rc == GMR_OK; k++) {
    const int slot = k % gmr_solver::kPipe;
    hipStream_t st = owner->pipe_stream[slot];
    // layout of this slice in the slot's workspace (a job with fewer streams than slices is absent from some: S = 0)
    gmr::Carve need;
    for (int j = 0; j < njobs; j++) {
      int S = 0;
      if (has_work(jobs[j])) gmr::ik_slice_range(jobs[j].S, k, n, &s0[j], &S);
      woff[j] = carve_weight(need, jobs[j], weight_of(weight, j), (size_t)S);
      off[j] = carve_job(need, jobs[j], (size_t)S);
    }
    if (need.total() > owner->pipe_ws[slot].size()) GMR_HIP_TRY(hipStreamSynchronize(st));
    GMR_HIP_TRY(owner->pipe_ws[slot].reserve(need.total()));
    char* d = owner->pipe_ws[slot].data();
    for (int j = 0; j < njobs && rc == GMR_OK; j++) {
      gmr_job_t& D = dj[j];
      D = jobs[j];
      D.S = (int32_t)off[j].S;
      dw[j] = nullptr;
      if (D.S == 0) continue;
      rc = issue(c, gmr::ik_slice_copies(off[j], false, (size_t)s0[j], c), jobs[j], d, st, "H2D copy");
      if (rc == GMR_OK) rc = issue_weight(&cw, gmr::ik_weight_slice_copy(woff[j], (size_t)s0[j], &cw), weight_of(weight, j), d, st, "H2D copy");
      dw[j] = gmr::ik_weight_at(d, woff[j]);
      if (rc == GMR_OK) rc = zero_outputs(jobs[j], d, off[j], st);
      D = gmr::ik_job_at(D, d, off[j]);
    }
    if (rc == GMR_OK) rc = gmr_retarget_group_weighted_dev(dj.data(), njobs, dw.data(), flags, st);
    for (int j = 0; j < njobs && rc == GMR_OK; j++)
      if (off[j].S) rc = issue(c, gmr::ik_slice_copies(off[j], true, (size_t)s0[j], c), jobs[j], d, st, "D2H copy");
  }
  for (int i = 0; i < nslot; i++)
    if ((e = hipStreamSynchronize(owner->pipe_stream[i])) != hipSuccess && rc == GMR_OK)
      rc = fail(GMR_ERR_HIP, "kernel / copies: %s", hipGetErrorString(e));
  return rc;
}

int gmr_retarget_streams(gmr_solver_t* s, int S, int T, const double* q0, const double* human, const int32_t* len,
                         int flags, double* q_out, int32_t* nsolve, int32_t* status, double* tgt_out, double* err_out) {
  return gmr_retarget_streams_scaled(s, S, T, q0, human, len, nullptr, flags, q_out, nsolve, status, tgt_out, err_out);
}

// One job, directly on the null stream.  Small calls (the per-frame API) go through pinned staging, so that a call is
// 1 H2D of [0, q_out) + 1 launch + 1 D2H of [q_out, end) + 1 sync; large batches take the sliced path above.
int gmr_retarget_streams_scaled(gmr_solver_t* s, int S, int T, const double* q0, const double* human, const int32_t* len,
                                const double* scale, int flags, double* q_out, int32_t* nsolve, int32_t* status, double* tgt_out,
                                double* err_out) {
  return gmr_retarget_streams_weighted(s, S, T, q0, human, len, scale, nullptr, flags, q_out, nsolve, status, tgt_out, err_out);
}

// (the body weights lie in front of the job's arrays: with none the layout is the one it was, and [0, out_begin) is all input)
int gmr_retarget_streams_weighted(gmr_solver_t* s, int S, int T, const double* q0, const double* human, const int32_t* len,
                                  const double* scale, const double* weight, int flags, double* q_out, int32_t* nsolve, int32_t* status,
                                  double* tgt_out, double* err_out) {
  const gmr_job_t job{s, S, T, q0, human, len, q_out, nsolve, status, tgt_out, err_out, scale};
  if (int rc = check_job(job, weight, true, -1)) return rc;
  if (!has_work(job)) return GMR_OK;
  gmr::Carve layout;
  const gmr::IkWeightOff wo = carve_weight(layout, job, weight, (size_t)S);
  const gmr::IkJobOff o = carve_job(layout, job, (size_t)S);
  if (o.S * o.stride(gmr::IK_HUMAN) + wo.S * wo.stride() >= ((size_t)32 << 20)) return gmr_retarget_group_weighted(&job, 1, &weight, flags, 0);
  // grow-only workspace kept on the handle: a per-frame caller (retarget() once per frame) pays no
  // hipMalloc/hipFree per call.  Like the reference object, a handle is not re-entrant on this path.
  GMR_HIP_TRY(s->ws.reserve(o.end, 0, 1u << 20));
  char* d = s->ws.data();
  const size_t ob = o.out_begin();
  const bool small = o.end <= gmr_solver::kPinBytes;
  if (small && !s->pin) GMR_HIP_TRY(hipHostMalloc((void**)&s->pin, gmr_solver::kPinBytes, hipHostMallocDefault));
  gmr::IkCopy ci[gmr::IK_NFIELD], co[gmr::IK_NFIELD], cw;
  const int ni = gmr::ik_slice_copies(o, false, 0, ci), no = gmr::ik_slice_copies(o, true, 0, co), nw = gmr::ik_weight_slice_copy(wo, 0, &cw);
  for (int i = 0; small && i < ni; i++) memcpy(s->pin + ci[i].dev, gmr::ik_ptr(job, ci[i].field) + ci[i].host, ci[i].width);
  if (small && nw) memcpy(s->pin + cw.dev, reinterpret_cast<const char*>(weight) + cw.host, cw.width);
  if (small) GMR_NAMED_HIP_TRY("H2D copy", hipMemcpyAsync(d, s->pin, ob, hipMemcpyHostToDevice, nullptr));
  else {
    if (int rc = issue(ci, ni, job, d, nullptr, "H2D copy")) return rc;
    if (int rc = issue_weight(&cw, nw, weight, d, nullptr, "H2D copy")) return rc;
  }
  if (int rc = zero_outputs(job, d, o, nullptr)) return rc;
  if (int rc = launch_job(gmr::ik_job_at(job, d, o), gmr::ik_weight_at(d, wo), flags, nullptr)) return rc;
  if (small) GMR_NAMED_HIP_TRY("kernel / D2H copy", hipMemcpyAsync(s->pin + ob, d + ob, o.end - ob, hipMemcpyDeviceToHost, nullptr));
  else if (int rc = issue(co, no, job, d, nullptr, "kernel / D2H copy")) return rc;
  GMR_NAMED_HIP_TRY("kernel / D2H copy", hipStreamSynchronize(nullptr));
  for (int i = 0; small && i < no; i++) memcpy(gmr::ik_ptr(job, co[i].field) + co[i].host, s->pin + co[i].dev, co[i].width);
  return GMR_OK;
}

}  // extern "C"
