// gmr_ik_wide_kernels.inc -- the two kernels of the throughput shape, included THREE times by gmr_ik_wide.hip:
//   1. as ik_wide_kernel / ik_wide_group_kernel with GMR_FWIN false and GMR_WGT 0: the kernels of launches none of whose solvers
//      has a finite frame window (gmr_solver_set_frame_velocity_limits) and none of whose jobs carries body weights;
//   2. as ik_wide_fw_kernel / ik_wide_group_fw_kernel with GMR_FWIN true and GMR_WGT 0, which clamp the QP box into the frame window;
//   3. as ik_wide_group_w_kernel with GMR_FWIN true and GMR_WGT 1, the group kernel alone (GMR_WIDE_KERNEL is not defined, so the
//      plain kernel is left out): per-frame body weights from the job table (gmr_retarget_streams_weighted).
// Instances, not a test in one kernel: with the window behind a wave-uniform test in the only instance, the register pair of
// theta0 and 9 more spilled SGPRs cost the 1M-frame batch 0.85 % with no limit set, the same sign in five alternated runs out of
// five (DESIGN.md 6zd); with GMR_FWIN false and GMR_WGT 0 both features fold away and the instance is the code it was without
// them.  Textual, like gmr_ik_wide_item.inc and for its reason.
// Plain launch: ONE job without per-stream scale tables, its fields are individual kernel arguments.  That matters: with ~100 SGPRs for ~350
// wave-uniform values the compiler re-loads a kernel ARGUMENT where it is used (s_load from the kernarg segment: no VALU
// slot), while a value it cannot re-load is parked in a VGPR lane and comes back through v_readlane.  Passing the job as
// one by-value struct (or reading it through a pointer to the kernarg segment) loses that property: measured, +500
// v_readlane instructions in the code object and -4 % frames/s.  For the same reason this instance has no scale
// argument: GMR_SCALE is a literal null here and the branch in preprocess_wide folds away; a job that carries scale
// rows runs the group instance, alone if need be.
#ifdef GMR_WIDE_KERNEL
__global__ __launch_bounds__(64, GMR_WIDE_MIN_WAVES) void GMR_WIDE_KERNEL(
    const char* __restrict__ img, WideDims D, int max_iter, int human_root, int use0, int use1, int S, int T,
    const double* __restrict__ q0, const double* __restrict__ human, const int32_t* __restrict__ len, int flags,
    double* q_out, int32_t* __restrict__ nsolve, int32_t* __restrict__ status, double* __restrict__ tgt_out,
    double* __restrict__ err_out, WideQueue Q, unsigned long long* __restrict__ prof_out) {
  extern __shared__ __align__(16) double sm[];
  const int lane = threadIdx.x;
  const bool queued = Q.ring != nullptr;
  if (!queued && (int)blockIdx.x >= S) return;
  Prof pr;
#ifdef GMR_IK_PROFILE
  for (int i = 0; i < PH_COUNT; i++) pr.acc[i] = 0;
  const unsigned long long k_t0 = __builtin_amdgcn_s_memtime(), k_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int nq = D.nq, nhum = D.nhum;
  const double* prm = img_at<double>(img, IM.prm);   // damping, lm_damping, tol, limit_gain, ground_offset, dt
  const unsigned nchunk = queued ? Q.hdr[2] : 0u;
  const size_t fstride = (size_t)nhum * 7;
  for (;;) {
  int s = blockIdx.x, t0 = 0, stat = GMR_STATUS_OK;
  RowState bounds = {0ull, 0ull};
  if (queued) {
    unsigned ticket = 0;
    if (lane == 0) ticket = __hip_atomic_fetch_add(&Q.hdr[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    if (ticket >= nchunk) break;
    unsigned v = 0;
    for (;;) {
      if (lane == 0) v = __hip_atomic_load(&Q.ring[ticket], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      v = __builtin_amdgcn_readfirstlane(v);
      if (v) break;
      __builtin_amdgcn_s_sleep(64);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the producer's q_out row and state are visible from here
    s = (int)v - 1;
    const WideStreamState st = Q.state[s];
    bounds.lower = uniform64(st.lower); bounds.upper = uniform64(st.upper);
    t0 = __builtin_amdgcn_readfirstlane(st.t_next);
    stat = __builtin_amdgcn_readfirstlane(st.stat);
  }
  const int gs = s;
#define GMR_DIMS_T const WideDims&
#define GMR_T_END T
#define GMR_WINDOWED false
#define GMR_SCALE static_cast<const double*>(nullptr)
#include "gmr_ik_wide_item.inc"
#undef GMR_SCALE
#undef GMR_WINDOWED
#undef GMR_T_END
#undef GMR_DIMS_T
  }
#ifdef GMR_IK_PROFILE
  pr.acc[PH_TICKS] = __builtin_amdgcn_s_memtime() - k_t0;
  pr.acc[PH_REALTIME] = __builtin_amdgcn_s_memrealtime() - k_r0;
  if (lane == 0 && prof_out && !queued)
    for (int i = 0; i < PH_COUNT; i++) prof_out[(size_t)blockIdx.x * PH_COUNT + i] = pr.acc[i];
#else
  (void)prof_out;
#endif
}
#endif  // GMR_WIDE_KERNEL

// Group launch: the job of an item comes from the table in device memory, by scalar loads through a constant-memory
// pointer (wave-uniform, like kernel arguments, but not re-loadable for free: this instance keeps a few more values in
// registers than the plain one).
__global__ __launch_bounds__(64, GMR_WIDE_MIN_WAVES) void GMR_WIDE_GROUP_KERNEL(const WideJob* __restrict__ jobs, int njobs,
                                                                               int total, int flags, WideQueue Q) {
  extern __shared__ __align__(16) double sm[];
  const int lane = threadIdx.x;
  const bool queued = Q.ring != nullptr;
  if (!queued && (int)blockIdx.x >= total) return;
  Prof pr;
#ifdef GMR_IK_PROFILE
  for (int i = 0; i < PH_COUNT; i++) pr.acc[i] = 0;
#endif
  const unsigned nchunk = queued ? Q.hdr[2] : 0u;
  for (;;) {
  int gs = blockIdx.x, t0 = 0, stat = GMR_STATUS_OK;
  RowState bounds = {0ull, 0ull};
  if (queued) {
    if (!queue_pop(Q, nchunk, lane, gs, t0, stat, bounds)) break;
  } else if (Q.windowed && Q.t_begin > 0) {           // a later window of a direct launch: continue from the parked state
    const WideStreamState st = Q.state[gs];
    bounds.lower = uniform64(st.lower); bounds.upper = uniform64(st.upper);
    t0 = __builtin_amdgcn_readfirstlane(st.t_next);
    stat = __builtin_amdgcn_readfirstlane(st.stat);
  }
  typedef const WideJob __attribute__((address_space(4))) CJob;
  const int j = __builtin_amdgcn_readfirstlane(job_of(jobs, njobs, gs, lane));
  CJob* cj = reinterpret_cast<CJob*>(reinterpret_cast<uintptr_t>(jobs + j));
  const WideDims __attribute__((address_space(4)))& D = cj->D;
  const char* __restrict__ img = cj->img;
  const int max_iter = cj->max_iter, human_root = cj->human_root, use0 = cj->use0, use1 = cj->use1, T = cj->T;
  const double* __restrict__ q0 = cj->q0;
  const double* __restrict__ human = cj->human;
  const int32_t* __restrict__ len = cj->len;
  double* q_out = cj->q_out;
  int32_t* __restrict__ nsolve = cj->nsolve;
  int32_t* __restrict__ status = cj->status;
  double* __restrict__ tgt_out = cj->tgt_out;
  double* __restrict__ err_out = cj->err_out;
  const double* __restrict__ scale = cj->scale;
#if GMR_WGT
  const double* __restrict__ weight = cj->weight;
#endif
  const int s = gs - cj->first;
  const int nq = D.nq, nhum = D.nhum;
  const double* prm = img_at<double>(img, IM.prm);
  const size_t fstride = (size_t)nhum * 7;
#define GMR_DIMS_T const WideDims __attribute__((address_space(4)))&
#define GMR_T_END Q.t_end
#define GMR_WINDOWED (Q.windowed != 0)
#define GMR_SCALE scale
#include "gmr_ik_wide_item.inc"
#undef GMR_SCALE
#undef GMR_WINDOWED
#undef GMR_T_END
#undef GMR_DIMS_T
  }
}

