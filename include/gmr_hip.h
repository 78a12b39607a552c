/*
 * gmr_hip.h -- C-ABI of libgmrhip.so: the MI355X (gfx950) implementation of GMR's retargeting
 * hot path.  Plain C, plain pointers and sizes, no torch / no C++ types: this is exactly what a
 * ctypes (or cffi / cgo / JNI) binding in the reference would bind.  INTEGRATION.md shows the
 * reference-side stub.
 *
 * Conventions: every function returns 0 on success and a negative code on error
 * (gmr_last_error() returns a thread-local message); what a handle describes is immutable after
 * creation, so batch calls on different HIP streams are re-entrant.  "dev" entry points take device
 * pointers and a hipStream_t (as void*; NULL = the default stream).  Those that need scratch memory
 * (gmr_postprocess_clips_dev, gmr_smplx_joints_dev, gmr_smplx_batch_frames_dev, gmr_bvh_frames_dev)
 * keep it on the handle, one grow-only block per HIP stream that has called, freed when the handle is
 * destroyed: calls on different streams may be in flight together, and the only time such a call
 * waits is when its block has to grow -- for its own stream alone.  The entry points without the
 * suffix take host pointers, copy, launch and synchronise; they stage through ONE device workspace
 * per handle, so at most one host-pointer call per handle at a time (like the reference object,
 * which is not thread-safe either: SURVEY.md section 8b).
 *
 * Row IDs (H1..H10) refer to SURVEY.md section 8(a).
 */
#ifndef GMR_HIP_H
#define GMR_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "gmr_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GMR_OK 0
#define GMR_ERR_ARG (-1)     /* bad argument / bad blob                                   */
#define GMR_ERR_HIP (-2)     /* a HIP runtime call failed                                  */
#define GMR_ERR_NO_DEVICE (-3)
#define GMR_ERR_COMM (-4)    /* RCCL / bootstrap failure                                   */

/* retarget flags */
#define GMR_FLAG_OFFSET_TO_GROUND 1 /* retarget(human_data, offset_to_ground=True), motion_retarget.py:139 */
#define GMR_FLAG_EVAL_ONLY 2        /* update_targets() without solve: preprocess + residual norms only, q_out = q in
                                       (motion_retarget.py:117-136 followed by error1()/error2(), :188-200)          */
#define GMR_FLAG_FRAME_LIMIT_FIRST 4 /* q0 is the pose of the frame BEFORE frame 0: the frame velocity limit
                                       (gmr_solver_set_frame_velocity_limits) bounds frame 0 around q0 as well; without it
                                       frame 0 of a stream is free.  No effect without such a limit or with EVAL_ONLY      */

/* per-stream status written by the IK kernel */
#define GMR_STATUS_OK 0
#define GMR_STATUS_QP_FAILED (-1)   /* Cholesky breakdown / non-finite input; mink would raise (section 8b) */
#define GMR_STATUS_QP_MAXITER (-2)  /* active-set iteration cap hit                                         */

typedef struct gmr_solver gmr_solver_t; /* device-resident (model, task set)                    */
typedef struct gmr_fk gmr_fk_t;         /* device-resident KinematicsModel tree (float32 path)  */

/* ---- library / device ------------------------------------------------------------------- */
const char* gmr_last_error(void);
const char* gmr_backend_info(void);     /* "hip:gfx950 ..." ; replaces nothing, diagnostic      */
int gmr_device_count(void);
int gmr_set_device(int device);
size_t gmr_sizeof_model(void);          /* ABI check against the Python-side struct layouts      */
size_t gmr_sizeof_taskset(void);

/* ---- device memory / streams / events (so that the Python host needs no torch) ----------- */
int gmr_malloc(void** ptr, size_t bytes);
int gmr_free(void* ptr);
int gmr_memset(void* ptr, int value, size_t bytes, void* stream);
int gmr_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int gmr_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int gmr_stream_create(void** stream);
int gmr_stream_destroy(void* stream);
int gmr_stream_sync(void* stream);      /* NULL = device synchronize                             */
int gmr_event_create(void** event);
int gmr_event_destroy(void* event);
int gmr_event_record(void* event, void* stream);
int gmr_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop`          */

/* ---- H1: solver state ------------------------------------------------------------------- */
/* Replaces GeneralMotionRetargeting.__init__ + setup_retarget_configuration
 * (motion_retarget.py:13-114): uploads the packed robot model and task set.  The blobs are the
 * same bytes rank 0 broadcasts to its peers. */
int gmr_solver_create(const gmr_model_t* model, const gmr_taskset_t* taskset, gmr_solver_t** out);
int gmr_solver_destroy(gmr_solver_t* solver);
int gmr_solver_dims(const gmr_solver_t* solver, int* nq, int* nv, int* nhuman);
/* Launch shape of the IK kernel: 1 = one wavefront per stream (most streams resident), 4 = one main
 * wavefront + 3 helper wavefronts per stream (shortest per-frame latency), 0 = automatic (4 up to 300
 * streams per launch, 1 above).  The 4-wavefront shape needs a robot whose dofs split into <= 4 limbs of <= 8
 * and a trunk of <= 10 (all shipped robots do); other robots always run the 1-wavefront shape.  Results agree
 * to rounding between the shapes; no reference analogue. */
int gmr_solver_set_waves(gmr_solver_t* solver, int waves_per_stream);
/* Dispatch of the 1-wavefront shape when streams outnumber the GPU's resident wavefronts (9 per CU):
 * frames_per_item > 0 = a resident set of wavefronts serves (stream, frames_per_item frames) items from a device-side
 * FIFO, so all streams advance together and the launch does not end on a few late, long streams (default 4);
 * 0 = one workgroup per stream for all of its frames.  Results are bit-identical either way.  The reference's analogue
 * is the chunking of `mp.Pool.map` over files (scripts/smplx_to_robot_dataset.py:241-242). */
int gmr_solver_set_dispatch(gmr_solver_t* solver, int frames_per_item);
/* Per-joint velocity limits in the QP box: mink.VelocityLimit, what GeneralMotionRetargeting(use_velocity_limit=True)
 * appends to the limits of every solve_ik call upstream.  vmax f64 [nhinge], rad/s, in hinge order; +inf = no limit for
 * that hinge; NULL (n = 0 or nhinge) = none at all, the state of a new solver.  Every solve then keeps
 *     |dq_h| <= vdt_h = vmax_h * timestep
 * on top of the joint-range box: lo = min(max(lo_cfg, -vdt_h), vdt_h), hi likewise, so that a joint that starts outside
 * its range by more than vdt_h walks back at full rate (mink raises there).  This bounds ONE solve, as in mink -- a frame
 * runs up to 2 * (max_iter + 1) solves, so it is NOT a bound on the joint velocity between frames: that one is
 * gmr_solver_set_frame_velocity_limits below.  The six dofs of the
 * free joint are never bounded.  A property of the handle: every launch from this solver issued after the call returns
 * uses it (streams, scaled streams, group jobs -- each job its own solver's table --, windows, queued or direct
 * dispatch); launches issued before finish on the old table.  n != nhinge, a NaN or a value <= 0 is GMR_ERR_ARG.
 * With no finite limit the kernels compute the bits they compute without this call. */
int gmr_solver_set_velocity_limits(gmr_solver_t* solver, const double* vmax, int n);
int gmr_solver_velocity_limits(const gmr_solver_t* solver, double* vmax_out, int n);
/* Per-FRAME joint velocity limits: the retargeted clip itself keeps |theta_h(t) - theta_h(t - 1)| <= w_h = vmax[h] * frame_dt
 * for every hinge (what a PD controller or hardware that plays the clip needs).  vmax f64 [nhinge] rad/s in hinge order,
 * +inf = none for that hinge, NULL (n = 0 or nhinge) = none at all, the state of a new solver; frame_dt in seconds, one per
 * handle; w_h is computed once, here, in double.  With theta0_h the hinge's angle when the frame starts (the previous
 * frame's result; q0 for frame 0) every solve of the frame, at its current iterate theta_h, takes the box of the limits
 * above (joint range, then the per-solve bound) and clamps it last into the window:
 *     lf = (theta0_h - w_h) - theta_h,  hf = (theta0_h + w_h) - theta_h,
 *     lo = min(max(lo, lf), hf),        hi = min(max(hi, lf), hf)
 * -- the clamp form, so the box is never empty, and the window is the bound that always holds: a hinge outside its range
 * walks back by w_h per frame.  A hinge without a range is bounded by the window alone; the free joint never is.
 * Frame 0 of a stream is free unless the launch carries GMR_FLAG_FRAME_LIMIT_FIRST; frames t >= 1 are bounded around frame
 * t - 1 by their index in the stream, so later windows of gmr_retarget_group_window_dev and later queue items continue
 * under the bound with no flag.  Same contract as gmr_solver_set_velocity_limits: written in place into the images the
 * solver owns (job tables stay valid), earlier launches finish on the old table, every launch path reads it.  n != nhinge,
 * a NaN, a value <= 0, or a frame_dt that is not finite and positive while some vmax is finite: GMR_ERR_ARG, and nothing
 * reaches the device.  With no finite entry the kernels compute the bits they compute without this call.
 * NOT for chunked retargeting (chunking.py: gmr_chunk_*): every chunk starts from qpos0 and seams are repaired by
 * re-running, so a seam would not carry the bound; the Python layer refuses chunk= while a finite frame limit is set.
 * The getter returns the table and, where frame_dt_out is not NULL, frame_dt (0 while no entry is finite). */
int gmr_solver_set_frame_velocity_limits(gmr_solver_t* solver, const double* vmax, int n, double frame_dt);
int gmr_solver_frame_velocity_limits(const gmr_solver_t* solver, double* vmax_out, int n, double* frame_dt_out);

/* ---- H2-H7: the retargeting loop ---------------------------------------------------------- */
/* Replaces the caller loop `for frame in frames: qpos = retargeter.retarget(frame)`
 * (scripts/smplx_to_robot_dataset.py:85-87) around GeneralMotionRetargeting.retarget
 * (motion_retarget.py:139-185) for S independent streams of up to T frames each, with the time
 * loop on the device (frames of one stream are sequentially dependent: warm start, :75).
 *
 *   q0      f64 [S][nq]            configuration before the first frame (qpos0 for a fresh object)
 *   human   f64 [S][T][nhuman][7]  raw human_data of the bodies of the scale table, packed order
 *                                  (pos xyz, quat wxyz); a body absent from the caller's dict is
 *                                  encoded with pos[0] = NaN
 *   len     i32 [S] or NULL        frames of stream s (<= T); NULL = all T
 *   q_out   f64 [S][T][nq]         qpos after each frame (what retarget() returns, :185)
 *   nsolve  i32 [S][T][2]          solve_ik calls per stage (1 + loop iterations, :147-161)
 *   status  i32 [S]                GMR_STATUS_*
 *   tgt_out f64 [S][T][nhuman][7]  or NULL: the preprocessed targets of every frame, i.e. `scaled_human_data`
 *                                  = the poses handed to task.set_target (:117-136, :203-270), as the kernel
 *                                  computed them (absent bodies stay NaN rows)
 *   err_out f64 [S][T][2]          or NULL: error1() / error2() (:188-200) at the configuration each frame
 *                                  ends with (0 for a stage the config does not use)
 * Rows the kernel does not write: frames at or beyond len[s]; and, for a stream whose status is not GMR_STATUS_OK,
 * the tgt_out rows of the frames AFTER the failing one and the err_out rows from the failing frame on (q_out keeps the
 * last good configuration for those frames, nsolve 0).  The host entry point returns such rows as zeros; the device
 * entry point leaves the caller's memory untouched there -- clear tgt_out / err_out first if stale bytes matter.
 */
int gmr_retarget_streams_dev(gmr_solver_t* solver, int S, int T, const double* d_q0, const double* d_human,
                             const int32_t* d_len, int flags, double* d_q_out, int32_t* d_nsolve,
                             int32_t* d_status, double* d_tgt_out, double* d_err_out, void* stream);
int gmr_retarget_streams(gmr_solver_t* solver, int S, int T, const double* q0, const double* human,
                         const int32_t* len, int flags, double* q_out, int32_t* nsolve, int32_t* status,
                         double* tgt_out, double* err_out);
/* The same pair with a human scale table PER STREAM, so that subjects of different heights (or limb proportions)
 * share one solver and one launch:
 *
 *   scale   f64 [S][nhuman] or NULL  row s replaces, for stream s, the scale entries of the solver's task set
 *                                    (gmr_taskset_t's human scale table, packed human-body order, the entry of the
 *                                    human root included); NULL = the solver's own table, i.e. the pair above
 *
 * The reference folds `human_scale_table * actual_human_height / human_height_assumption` into the object
 * (motion_retarget.py:13-114), one object per height; here that product is the caller's row.  A stream with row r gives
 * the bits of a solver whose table is r.  The host entry point rejects a non-finite or non-positive entry with
 * GMR_ERR_ARG, naming the stream and the body; the device entry point cannot look: the values are the caller's
 * responsibility.  In the 1-wavefront shape a launch with scale rows runs the group instance of the throughput kernel. */
int gmr_retarget_streams_scaled_dev(gmr_solver_t* solver, int S, int T, const double* d_q0, const double* d_human,
                                    const int32_t* d_len, const double* d_scale, int flags, double* d_q_out,
                                    int32_t* d_nsolve, int32_t* d_status, double* d_tgt_out, double* d_err_out,
                                    void* stream);
int gmr_retarget_streams_scaled(gmr_solver_t* solver, int S, int T, const double* q0, const double* human,
                                const int32_t* len, const double* scale, int flags, double* q_out, int32_t* nsolve,
                                int32_t* status, double* tgt_out, double* err_out);
/* ---- several (robot, task set) jobs as ONE scheduling domain -------------------------------------------------------
 * BASELINE.json configs[3] ("all 6 robots mixed-DoF batch"; SURVEY.md section 8d: "per-robot kernels or one kernel
 * with per-stream model index"): the reference would run one mp.Pool worker per file whatever its robot
 * (scripts/smplx_to_robot_dataset.py:241-242).  Every robot of the throughput kernel's size class runs the same
 * kernel instance, so the jobs of a group share one resident grid and one device-side queue of (job, stream, chunk)
 * items: the group is balanced as a whole and its launch ends within one chunk of its last stream.  Results are
 * bit-identical to launching every job by itself.  Jobs that do not take the throughput shape (a robot that does not
 * decompose, a solver forced to 4 wavefronts, a group of <= 300 streams) are launched one by one on the same stream. */
typedef struct gmr_job {
  gmr_solver_t* solver;
  int32_t S, T;
  const double* q0;        /* [S][nq]              the buffers of gmr_retarget_streams, per job                     */
  const double* human;     /* [S][T][nhuman][7]                                                                      */
  const int32_t* len;      /* [S] or NULL                                                                            */
  double* q_out;           /* [S][T][nq]                                                                             */
  int32_t* nsolve;         /* [S][T][2]                                                                              */
  int32_t* status;         /* [S]                                                                                    */
  double* tgt_out;         /* [S][T][nhuman][7] or NULL                                                              */
  double* err_out;         /* [S][T][2] or NULL                                                                      */
  const double* scale;     /* [S][nhuman] or NULL  per-stream human scale tables (gmr_retarget_streams_scaled); the   */
                           /* host entry point checks them, slices copy their rows, every window reads the same rows */
} gmr_job_t;
/* device pointers, asynchronous on `stream` */
int gmr_retarget_group_dev(const gmr_job_t* jobs, int njobs, int flags, void* stream);
/* device pointers, ONE WINDOW of every stream's frames, [t_begin, t_end): the windows of a batch are launched in order on one
 * stream starting at t_begin = 0; q continues from the previous window's last q_out row, the QP's bound sets and the status
 * travel in device memory.  Bit-identical to one launch.  Only for batches that take the throughput shape as a whole (every
 * robot decomposes, more than 300 streams in total, at most 8 jobs); GMR_ERR_ARG otherwise. */
int gmr_retarget_group_window_dev(const gmr_job_t* jobs, int njobs, int flags, int t_begin, int t_end, void* stream);
/* HOST pointers: the streams are cut into `slices` slices (0 = automatic: about 64 MB of input each, never fewer than
 * 4 096 streams per slice, at most 16; > 0: exactly that many, at most one per stream) whose H2D copies, launch and D2H copies go to one of four HIP streams, so that
 * copy(k+1) || kernel(k) || copy-back(k-1); synchronises before returning.  A batch too narrow for that (fewer than 8 192
 * streams) but long (>= 32 frames, >= 64 MB of input) is cut in TIME instead: consecutive windows of frames
 * (gmr_retarget_group_window_dev), the strided copies of window w + 1 under the kernel of window w; slices < 0 asks for
 * |slices| windows explicitly.  Use pinned host memory (below) for the
 * copies to be asynchronous.  gmr_retarget_streams takes this path by itself for inputs of 32 MB and more. */
int gmr_retarget_group(const gmr_job_t* jobs, int njobs, int flags, int slices);
/* Per-frame BODY WEIGHTS on the cost side of the QP: one multiplier per (stream, frame, human body), so that a caller can say
 * "the left wrist is occluded in frames 212-230" (weight 0) or "trust the feet more while they are in contact" (weight > 1)
 * without editing the clip or building a second solver.
 *
 *   weight  f64 [S][T][nhuman] or NULL  m = weight[s][t][b], in the packed human-body order of `human`; NULL = the entry
 *                                       points above, bit for bit
 *
 * Present tasks: every task k of either table whose human body is b uses w_pos[k] * m and w_rot[k] * m in that frame --
 * one IEEE double product each, formed once per frame from the solver's own weights -- wherever the weights occur: the
 * weighted Jacobian columns, c, and the LM term mu = lm_damping |W e|^2.  The structural pair lists of the task set depend
 * on the configured weights only.  A body with m > 0 enters the (unweighted) residual norm of the stop rule and of err_out
 * as it does without weights.
 * Missing tasks, m == 0: the body is missing in that frame.  Its tasks add exact zeros to H, c and mu, and their residuals
 * are LEFT OUT of the residual norm that the stop rule (curr - next > tol) and err_out use.  The `human` row of a missing
 * body that is not the human root is never read into a result: it may hold NaN, zeros or garbage; it is kept out of the
 * lowest-foot search of GMR_FLAG_OFFSET_TO_GROUND (a frame whose feet are ALL missing behaves like a frame whose feet are
 * all NaN: out of scope); its target is the identity pose, which no output depends on; its tgt_out row is seven NaNs, the
 * row of an absent body.  The human root's row is always read -- every other body is moved relative to it --, so a weight
 * of 0 there removes the root's task only, and a non-finite root row fails the stream as it does without weights.
 * A frame with every body missing is a plain damped solve: one solve per stage, q stays where it is inside its ranges.
 * GMR_FLAG_EVAL_ONLY applies the weights to err_out and tgt_out in the same way.
 * The host entry points reject an entry that is NaN, infinite or negative with GMR_ERR_ARG, naming stream, frame and body,
 * before anything reaches the device (only the frames t < len[s] are looked at: rows beyond a stream's length are padding
 * that is never read, like the human rows there); the device entry points cannot look: the values are the caller's responsibility.
 * gmr_job_t is closed, so group launches take the arrays BESIDE the job list: `weight` is NULL or has njobs entries, each
 * NULL or that job's array; a job without weights is not changed by a neighbour that has them.  Slices copy the rows of
 * their streams, windows the rows of their frames (the row of frame t is found by t: no state travels between windows).
 * The latency shape runs its instances with the velocity-limit box (+inf tables where the solver has none: the same bits),
 * the throughput shape the group instance, alone if need be.
 * NOT for chunked retargeting (chunking.py): the Python layer refuses chunk= together with weights. */
int gmr_retarget_streams_weighted_dev(gmr_solver_t* solver, int S, int T, const double* d_q0, const double* d_human,
                                      const int32_t* d_len, const double* d_scale, const double* d_weight, int flags,
                                      double* d_q_out, int32_t* d_nsolve, int32_t* d_status, double* d_tgt_out,
                                      double* d_err_out, void* stream);
int gmr_retarget_streams_weighted(gmr_solver_t* solver, int S, int T, const double* q0, const double* human,
                                  const int32_t* len, const double* scale, const double* weight, int flags, double* q_out,
                                  int32_t* nsolve, int32_t* status, double* tgt_out, double* err_out);
int gmr_retarget_group_weighted_dev(const gmr_job_t* jobs, int njobs, const double* const* weight, int flags, void* stream);
int gmr_retarget_group_weighted_window_dev(const gmr_job_t* jobs, int njobs, const double* const* weight, int flags,
                                           int t_begin, int t_end, void* stream);
int gmr_retarget_group_weighted(const gmr_job_t* jobs, int njobs, const double* const* weight, int flags, int slices);
/* pinned (page-locked) host memory for the host-pointer entry points; gmr_host_register pins a caller's own buffer */
int gmr_host_alloc(void** ptr, size_t bytes);
int gmr_host_free(void* ptr);
int gmr_host_register(void* ptr, size_t bytes);
int gmr_host_unregister(void* ptr);

/* LDS bytes per stream of the IK kernel for this solver (occupancy reporting): of the 4-wavefront layout when the robot
 * decomposes into trunk and limbs, else of the one-wavefront layout, the only one such a robot is launched with. */
int gmr_retarget_lds_bytes(const gmr_solver_t* solver);

/* ---- H8-H9: post-hoc batched FK (float32) ------------------------------------------------- */
/* Replaces KinematicsModel(xml, device="cuda:0") + forward_kinematics
 * (kinematics_model.py:69-170, 213-246), i.e. ~2.6k ATen launches per call -> one kernel.
 * Tree arrays are those of the reference's own XML reader (mjcf.parse_kinematics_tree):
 * local_r xyzw un-normalised, axis f64 per body (zeros where dof_idx < 0). */
int gmr_fk_create(int nbody, const int32_t* parent, const float* local_t, const float* local_r,
                  const int32_t* dof_idx, const double* axis, int ndof, gmr_fk_t** out);
int gmr_fk_destroy(gmr_fk_t* fk);
/*   root_pos f32 [B][3], root_rot f32 [B][4] xyzw, dof f32 [B][ndof]
 *   body_pos f32 [B][nbody][3], body_rot f32 [B][nbody][4] (may be NULL)
 *   min_z    f32 [1] (may be NULL): min over all frames and bodies of body_pos z -- the reduction
 *            of the dataset scripts' height adjustment (smplx_to_robot_dataset.py:118-126)        */
int gmr_fk_batch_dev(gmr_fk_t* fk, int B, const float* d_root_pos, const float* d_root_rot, const float* d_dof,
                     float* d_body_pos, float* d_body_rot, float* d_min_z, void* stream);
int gmr_fk_batch(gmr_fk_t* fk, int B, const float* root_pos, const float* root_rot, const float* dof,
                 float* body_pos, float* body_rot, float* min_z);

/* Many clips in ONE launch (the dataset drivers): the frames of clip g are rows [seg_start[g], seg_start[g + 1]) of the
 * inputs; seg_min_z[g] = min over the clip's frames and bodies of body_pos z -- the per-clip reduction of the height
 * adjustment (smplx_to_robot_dataset.py:118-126), +inf for an empty clip.  body_pos may be NULL (only the minima wanted). */
int gmr_fk_segment_min_z_dev(gmr_fk_t* fk, const float* d_body_pos, const int32_t* d_seg_start, int nseg, float* d_seg_min,
                             void* stream);
int gmr_fk_batch_segments(gmr_fk_t* fk, int B, const float* root_pos, const float* root_rot, const float* dof, int nseg,
                          const int32_t* seg_start /* [nseg + 1] */, float* body_pos, float* seg_min_z /* [nseg] */);

/* ---- H10: the dataset drivers' post-processing, on the device ------------------------------------------------------
 * Replaces what `process_file` does between the retargeting loop and pickle.dump (scripts/smplx_to_robot_dataset.py:97-131;
 * bvh_to_robot_dataset.py:111-139, which has both adjustments off) for ALL clips of a batch, reading the IK launch's output where
 * it lies -- no round trip of q_out through the host, no float32 copies of it, no second upload:
 *   root_pos = q[0:3], root_rot = q[4,5,6,3] (wxyz -> xyzw), dof_pos = q[7:]                         (:97-102)
 *   local_body_pos = forward_kinematics(0, identity, float32(dof_pos))                               (:106-112)
 *   GMR_POST_HEIGHT_ADJUST:      lowest[c] = min over the clip's frames and bodies of the z of
 *                                forward_kinematics(float32(root_pos), float32(root_rot), float32(dof_pos));
 *                                root_pos.z = root_pos.z - (double)lowest[c] + ground_offset          (:118-126)
 *   GMR_POST_ROOT_ORIGIN_OFFSET: root_pos.xy -= root_pos.xy of the clip's first frame                (:128-131)
 * Both FK passes are the walk of gmr_fk_batch_dev (the world pass is a walk of its own, not root + R * local: the chained
 * products round differently, and `lowest` moves every root_pos.z of its clip), so the results are the bytes of
 * gmr_fk_batch_segments on the host-converted arrays followed by the NumPy lines above. */
#define GMR_POST_HEIGHT_ADJUST      1
#define GMR_POST_ROOT_ORIGIN_OFFSET 2
typedef struct gmr_post_src {      /* one IK job's output, as gmr_retarget_*_dev left it */
  int32_t S, T;                    /* T >= 1 when S > 0 */
  const double* q_out;             /* [S][T][nq]   */
  const int32_t* len;              /* [S] or NULL (= all T) */
} gmr_post_src_t;
/* device pointers, asynchronous on `stream`.  The clips of src[0], then src[1], ... (nsrc <= 8) are numbered 0 .. C-1;
 * seg_start i32 [C+1] ascending from 0 is the exclusive prefix sum of their lengths, B = seg_start[C] (the host passes B:
 * the kernels clamp what they read from seg_start to it, and a frame index to the rows of its stream, so no read leaves
 * the sources even for an inconsistent seg_start; rows at or beyond len[s] are never read).
 * outputs: root_pos f64[B][3], root_rot f64[B][4] xyzw, dof_pos f64[B][ndof], local_body_pos f32[B][nbody][3] (16-byte
 * aligned for the coalesced flush; any alignment works), lowest f32[C] (may be NULL; written only with
 * GMR_POST_HEIGHT_ADJUST; +inf for an empty clip).
 * The scratch memory of a call (16 B per row, and nbody * 12 B per row with GMR_POST_HEIGHT_ADJUST) belongs to the handle,
 * one block per HIP stream that has called, grown on demand (the only time the call waits: for its own stream) and freed
 * by gmr_fk_destroy: calls on different streams may be in flight together. */
int gmr_postprocess_clips_dev(gmr_fk_t* fk, const gmr_post_src_t* src, int nsrc, int nq,
                              const int32_t* d_seg_start, int C, int B, int flags, double ground_offset,
                              double* d_root_pos, double* d_root_rot, double* d_dof_pos,
                              float* d_local_body_pos, float* d_lowest, void* stream);

/* ---- chunked retargeting of long clips (opt-in, NOT parity) ---------------------------------
 * Frames of a clip depend on each other (warm start), so a batch of few, long clips (LAFAN1: 77 clips of up to 9 855
 * frames) leaves most of the device idle.  Here clip c of n frames is cut into K = max(1, ceil(n / L)) chunks that
 * partition [0, n) in order and evenly -- chunk i owns [floor(i n / K), floor((i + 1) n / K)) -- and run as ordinary,
 * independent streams of gmr_retarget_group_dev: chunk i >= 1 starts from the clip's q0 and first runs
 * warm = min(W, first owned frame) warm-up frames whose results are dropped.  The frame in front of a chunk is thus
 * computed twice; the difference (the seam residual) measures how far the chunk started from where the sequential run
 * would have been, and a chunk whose seam is off can be run again from its predecessor's final state (repair), which
 * makes its residual 0 until the predecessor itself changes.  Clips with n <= L are one chunk without warm-up: their
 * results are the bits of the unchunked launch.
 *
 * Tables (host: from the plan; device: copies of them, NOT trusted -- every record is clamped into its clip's rows and a
 * chunk's rows, a list entry outside [0, nchunk) names no chunk, so no access leaves the buffers whatever they hold):
 *   chunk      i32 [nchunk][4]   clip, first source frame (warm-up included), warm, owned; chunks of a clip consecutive
 *   clip_first i32 [nclip + 1]   first chunk of every clip; clip_first[nclip] = nchunk
 *   Tc                           the longest chunk, warm + owned (>= 1)
 * Plan: `chunk` == NULL sizes only (nchunk, Tc; clip_first is filled when given); otherwise `capacity` is the room in `chunk`.
 * L >= 1; W >= 1 when any clip is split (GMR_ERR_ARG otherwise).  Host code, no GPU needed. */
int gmr_chunk_plan(int nclip, const int32_t* len, int L, int W, int capacity, int32_t* chunk, int32_t* clip_first,
                   int* nchunk, int* Tc);
/* The three steps around the IK launch of a pass: device pointers, asynchronous on `stream`, no scratch memory, no
 * synchronisation.  A pass works on SLOTS: slot i is chunk i (d_list == NULL: all nchunk chunks) or chunk d_list[i]
 * (i < nlist), and is stream i of the pass's IK job  { S = slots, T = Tc, q0 = q0_c, human = human_c, len = len_c }.
 *   GMR_CHUNK_PASS0   warm-up and owned frames, q0_c[i] = the clip's q0 row
 *   GMR_CHUNK_REPAIR  owned frames only, q0_c[i] = q_seam[k] = clip-major q_out at the frame before the chunk
 * gather:  human f64[S][T][nhuman][7] (clip-major, where the front ends and the host copies put it), q0 f64[S][nq],
 *          q_out f64[S][T][nq] (repair only) -> human_c f64[slots][Tc][nhuman][7], len_c i32[slots], q0_c f64[slots][nq]
 *          (a slot that names no chunk gets len 0).  A pure copy, 16 bytes per lane when a frame is a multiple of 16 bytes
 *          and the buffers are 16-byte aligned (8 otherwise). */
#define GMR_CHUNK_PASS0 0
#define GMR_CHUNK_REPAIR 1
int gmr_chunk_gather_dev(int S, int T, int nhuman, int nq, int nchunk, int Tc, const int32_t* d_chunk, const int32_t* d_list, int nlist,
                         int mode, const double* d_human, const double* d_q0, const double* d_q_out, double* d_human_c,
                         int32_t* d_len_c, double* d_q0_c, double* d_q_seam, void* stream);
/* stitch:  the owned rows of q_out_c f64[slots][Tc][nq] / nsolve_c i32[slots][Tc][2] -> clip-major q_out f64[S][T][nq],
 *          nsolve i32[S][T][2]: the layout gmr_post_src_t and every consumer of gmr_retarget_streams_dev read; rows of other
 *          chunks are not touched.  chunk_status i32[nchunk] keeps every chunk's status word across passes, and
 *          status i32[S] = the first non-OK status of the clip's chunks in order.  Pass 0 (no list) also writes
 *          q_seam f64[nchunk][nq] = the chunk's last warm-up row (NaN without warm-up) and warm_solves i32[S] = the solves
 *          of the clip's warm-up rows, which are the overhead of the mode and are NOT part of nsolve. */
int gmr_chunk_stitch_dev(int S, int T, int nq, int nchunk, int Tc, const int32_t* d_chunk, const int32_t* d_clip_first,
                         const int32_t* d_list, int nlist, int mode, const double* d_q_out_c, const int32_t* d_nsolve_c,
                         const int32_t* d_status_c, double* d_q_out, int32_t* d_nsolve, int32_t* d_chunk_status, int32_t* d_status,
                         double* d_q_seam, int32_t* d_warm_solves, void* stream);
/* seams:   for every chunk that does not start its clip, q_seam[k] against q_out at the frame before the chunk:
 *          resid f64[nchunk][3] = max |d joint angle| (rad), max |d root position| (m), angle between the root orientations
 *          (rad; the same for q and -q, 2 atan2(|vector|, |scalar|) of the relative rotation); zeros for first chunks.
 *          A seam is over the tolerance when a component is > tol or not finite.  bad_list i32[nchunk] receives those
 *          chunks in ascending order (whatever the scheduling), nbad i32[1] their number -- the one word a pass loop reads
 *          back; a seam behind a chunk that FAILED is not listed (a re-run cannot mend it; its clip fails through `status`).
 *          seam_max f64[S][3] = the maxima of resid over the clip's chunks (NaN sticks). */
int gmr_chunk_seams_dev(int S, int T, int nq, int nchunk, int Tc, const int32_t* d_chunk, const int32_t* d_clip_first,
                        const double* d_q_out, const double* d_q_seam, const int32_t* d_chunk_status, double tol, double* d_resid,
                        int32_t* d_bad_list, int32_t* d_nbad, double* d_seam_max, void* stream);

/* ---- N1: SMPL-X frame extraction (the step in front of the loop) ---------- */
/* A kinematic tree of J <= 64 joints (parents[j] < j, joint 0 the root) and the joints whose poses are
 * wanted: sel[nsel] (one output row each, in this order; nsel = 0 -> all J joints, row = joint).  For the
 * retargeting loop sel lists the SMPL-X joints of the solver's packed human bodies, so that the output IS
 * the `human` argument of gmr_retarget_streams. */
typedef struct gmr_smplx gmr_smplx_t;
int gmr_smplx_create(int J, const int32_t* parents, int nsel, const int32_t* sel, gmr_smplx_t** out);
int gmr_smplx_destroy(gmr_smplx_t* h);
int gmr_smplx_rows(const gmr_smplx_t* h);   /* rows per output frame (nsel, or J) */
/* Replaces the joints of `body_model(betas, global_orient, body_pose, transl, ...)` as called at
 * general_motion_retargeting/utils/smpl.py:12-34, without the mesh: joints f32[N][J][3] from the rest
 * joints j_rest f64[J][3] (J_regressor applied to the shaped template, once per clip), the axis-angle
 * poses full_pose f32[N][J][3] and transl f32[N][3].  (The body model is third-party: parity unpinned.)
 * The device entry point is asynchronous; its scratch (the poses and joints as frame-minor planes, 24 J B per frame) is a
 * block per HIP stream like that of the other dev entry points: one handle may be used on several streams at once. */
int gmr_smplx_joints_dev(gmr_smplx_t* h, int N, const double* d_j_rest, const float* d_full_pose,
                         const float* d_transl, float* d_joints, void* stream);
int gmr_smplx_joints(gmr_smplx_t* h, int N, const double* j_rest, const float* full_pose, const float* transl,
                     float* joints);
/* Replaces get_smplx_data_offline_fast (utils/smpl.py:109-197) for one clip -- and get_smplx_data
 * (:44-73) when target_time is NULL (then Nout == N, no interpolation):
 *   full_pose f32[N][J][3], joints f32[N][jstride][3] (jstride >= J: the model appends landmark joints),
 *   target_time f64[Nout] = np.linspace(0, N-1, Nout), Nout = N // int(src_fps / tgt_fps) (:120-127)
 *   out f64[Nout][rows][7] = position xyz, global orientation quaternion wxyz per selected joint. */
int gmr_smplx_align_dev(gmr_smplx_t* h, int N, int jstride, const float* d_full_pose, const float* d_joints,
                        int Nout, const double* d_target_time, double* d_out, void* stream);
int gmr_smplx_align(gmr_smplx_t* h, int N, int jstride, const float* full_pose, const float* joints, int Nout,
                    const double* target_time, double* out);
/* Both steps for one clip in one call, host buffers: the body model's joints (all J) and the alignment of the selected rows,
 * nothing but out f64[Nout][rows][7] coming back (no joints on the host, no gather between the steps).  Replaces
 * load_smplx_file's forward pass + get_smplx_data_offline_fast (utils/smpl.py:12-41, :109-197) for a dataset driver that
 * needs only the packed frames.  target_time == NULL: no fps alignment, Nout == N. */
int gmr_smplx_frames(gmr_smplx_t* h, int N, const double* j_rest, const float* full_pose, const float* transl, int Nout,
                     const double* target_time, double* out);
/* The same on COMPACT inputs -- only what the alignment reads, FRAME-MINOR: pose_c f32[npose][3][N] = the axis-angle poses
 * of the selection's ancestor closure in walk order, joints_c f32[nrow][3][N] = the joint of every output row (numpy:
 * full_pose[:, pose_joints].transpose(1, 2, 0)); the two joint lists come from gmr_smplx_compact_layout (either output may
 * be NULL).  The host entry point gmr_smplx_align gathers these itself, so only 34 of the 110 joint triples of a G1 frame
 * cross the bus, and a wavefront's load of one component reads one contiguous run of source frames. */
int gmr_smplx_compact_layout(const gmr_smplx_t* h, int32_t* pose_joints, int* npose, int32_t* row_joints, int* nrow);
int gmr_smplx_align_compact_dev(gmr_smplx_t* h, int N, const float* d_pose_c, const float* d_joints_c, int Nout,
                                const double* d_target_time, double* d_out, void* stream);

/* A ragged batch of clips straight from the arrays an AMASS file holds, written where the IK kernels read them: replaces, for
 * nclip clips in one call, load_smplx_file's forward pass + get_smplx_data_offline_fast (utils/smpl.py:12-41, :109-197), i.e.
 * one gmr_smplx_frames call per clip, with the SAME BITS on every frame.  B source frames in total, concatenated, float32 as the
 * reference casts them (:27-31):
 *   root_orient f32 [B][3]      pose_body f32 [B][63]      trans f32 [B][3]
 *   src_start   i32 [nclip + 1]     source frames of clip c = [src_start[c], src_start[c + 1]); ascending from 0 to B
 *   nout        i32 [nclip]         output frames of clip c: N // int(src_fps / tgt_fps) with alignment, else N (<= N always)
 *   align       u8  [nclip]         1: fps alignment (tgt_fps < src_fps; also when nout == N, e.g. 50 -> 30 fps), 0: frame by frame
 *   j_rest      f64 [nclip][J][3]   rest joints of the clip's subject (J_regressor on the shaped template)
 *   clip_out    f64* [nclip]        where frame 0 of clip c goes (room for nout[c] frames of nsel x 7 doubles): a row of some
 *                                   job's human f64[S][T][nsel][7]; the clips of one call may belong to different jobs
 * Only joints 0 .. 21 have poses here (the hands, jaw and eyes are zero in load_smplx_file), so the handle's selection and its
 * ancestors must lie inside them (gmr_smplx_batch_takes; every shipped smplx ik_config does) -- otherwise GMR_ERR_ARG before
 * any launch.  The target times np.linspace(0, N - 1, nout) are computed on the device (gmr_smplx_target_times is the same
 * inline on the host).  Frames t >= nout[c] are not written by the device entry point (the IK kernels never read them); a clip
 * with nout == 0, or with alignment and fewer than two source frames, writes nothing.  The two tables are not trusted: whatever
 * they hold, no load leaves the inputs and a store goes to frame o < min(nout[c], N_c) of clip_out[c].
 * The scratch of a call (12 (npose + nsel) B per source frame: the poses of the closure and the joints of the rows as
 * frame-minor planes) belongs to the handle, one block per HIP stream that has called, grown on demand (the only time the call
 * waits: for its own stream) and freed by gmr_smplx_destroy: calls on different streams may be in flight together. */
int gmr_smplx_batch_takes(const gmr_smplx_t* h);          /* 1: the batch entry points take this handle's selection */
int gmr_smplx_target_times(int N, int Nout, double* out); /* out f64[Nout] = np.linspace(0, N - 1, Nout), bit for bit; host only */
int gmr_smplx_batch_frames_dev(gmr_smplx_t* h, int nclip, int B, const float* d_root_orient, const float* d_pose_body,
                               const float* d_trans, const int32_t* d_src_start, const int32_t* d_nout, const uint8_t* d_align,
                               const double* d_j_rest, double* const* d_clip_out, void* stream);   /* asynchronous */
/* host buffers; checks the tables (src_start ascending from 0 to B, 0 <= nout <= min(N, T), nout == N without alignment,
 * alignment needs two source frames) before anything is launched; human f64[nclip][T][nsel][7], frames t >= nout[c] come back
 * as zeros.  One call per handle at a time. */
int gmr_smplx_batch_frames(gmr_smplx_t* h, int nclip, int B, const float* root_orient, const float* pose_body,
                           const float* trans, const int32_t* src_start, const int32_t* nout, const uint8_t* align,
                           const double* j_rest, int T, double* human);

/* ---- N2: BVH frame extraction (LAFAN1; the step in front of the loop of the BVH dataset driver) -------------------- */
/* The topology of a BVH skeleton and the rows wanted per frame.  J <= 256 joints in file order (parents[0] = -1,
 * 0 <= parents[j] < j: a BVH hierarchy is written depth first, so every parent precedes its children); `channels` is the
 * layout of a motion row as extract.py:99-166 parses it -- 3: root translation, then 3 rotations per joint (ncol = 3 + 3 J;
 * LAFAN1), 6: 3 translations and 3 rotations per joint (ncol = 6 J); `order` the Euler order of the rotation channels, a
 * permutation of "xyz" ("zyx" for LAFAN1).  Output row k of a frame takes its position from joint sel_pos[k] and its
 * orientation from joint sel_rot[k] (nsel <= 64): a body of the ik_config is (j, j), `LeftFootMod` (lafan1.py:28-33: foot
 * position, toe orientation) is (LeftFoot, LeftToe).  Only the ancestor closure of the selected joints (<= 64 joints) is
 * walked.  Clips with another topology use another handle. */
typedef struct gmr_bvh gmr_bvh_t;
int gmr_bvh_create(int J, const int32_t* parents, int channels, const char* order /* "zyx" ... */,
                   int nsel, const int32_t* sel_pos, const int32_t* sel_rot, gmr_bvh_t** out);
int gmr_bvh_destroy(gmr_bvh_t* h);
int gmr_bvh_columns(const gmr_bvh_t* h);   /* doubles per motion row (ncol) */
/* Replaces, for nclip clips in one call, the numeric half of load_lafan1_file (general_motion_retargeting/utils/lafan1.py:8-41):
 * read_bvh's euler_to_quat + remove_quat_discontinuities (lafan_vendor/extract.py:155-166, lafan_vendor/utils.py:137-162,
 * 251-268), quat_fk (utils.py:88-103), the Y-up cm -> Z-up m change of axes and units (lafan1.py:20-27) and the packing of
 * the selected bodies:
 *   rows      f64 [B][ncol]          the motion rows of the clips, concatenated, as the text parses (degrees, centimetres)
 *   seg_start i32 [nclip + 1]        rows of clip c = [seg_start[c], seg_start[c + 1]); ascending from 0 to B
 *   offsets   f64 [nclip][J][3]      the OFFSET of every joint, per clip (LAFAN1's subjects differ in bone lengths)
 *   human     f64 [nclip][T][nsel][7] position xyz, orientation wxyz: the padded layout of gmr_job_t.human
 * Frames t >= the clip's length are not written by the device entry point (the IK kernels never read them); frames beyond
 * T are dropped.  seg_start is not trusted: whatever it holds, no access leaves the buffers.  The de-flip along time
 * (sign_t = prod_{u <= t} sign <q_{u-1}, q_u>, strict) is a prefix scan inside the call, exact across any clip length.
 * Results are the NumPy path's bits except for the last place of sin / cos (<= 1e-12 on every output).
 * The scratch of a call (12 B per row) belongs to the handle, one block per HIP stream that has called, grown on demand
 * (the only time the call waits: for its own stream) and freed by gmr_bvh_destroy: no allocation in steady state, and calls
 * on different streams may be in flight together. */
int gmr_bvh_frames_dev(gmr_bvh_t* h, int nclip, int B, const double* d_rows, const int32_t* d_seg_start,
                       const double* d_offsets, int T, double* d_human, void* stream);    /* asynchronous */
/* host buffers; checks seg_start (ascending from 0 to B, no clip longer than T); frames t >= a clip's length come back as
 * zeros.  One call per handle at a time. */
int gmr_bvh_frames(gmr_bvh_t* h, int nclip, int B, const double* rows, const int32_t* seg_start,
                   const double* offsets, int T, double* human);

/* ---- N3: motion library (the training-side loader: derivatives, statistics, batched sampling) ---------------------- */
/* What booster_gym/utils/motion_loader.py:100-247 does with the arrays of a motion pkl -- _compute_motion_stats,
 * _compute_derivatives, get_motion_state -- for C clips (B frames in total, clip-contiguous) held in ONE block of device
 * memory, with the per-frame and per-query Python loops replaced by three kernels.  Per clip c: T = seg_start[c + 1] -
 * seg_start[c] frames at fps[c], dt = 1 / fps (double), duration = T / fps.
 *   stored      float32 root_pos [B][3], root_rot [B][4] xyzw, dof_pos [B][ndof], local_body_pos [B][nbody][3] (optional)
 *   derivatives root_vel, dof_vel: (x[i] - x[i - 1]) / (float)dt inside the clip, [0] = [1]; root_ang_vel [B][3]:
 *               rotvec(r_i r_{i-1}^-1) / dt in float64 from the float32 quaternions, [0] = [1]; all zero for T == 1
 *   stats       float32 [C][4][3 + ndof]: mean, unbiased std (NaN for T == 1), min, max of (root_pos | dof_pos) per column;
 *               a NaN in a column makes that column's four values NaN; an empty clip (T == 0, which create accepts and a
 *               query refuses) has no statistics: all four rows are NaN, never a std of zero
 * GMR_MOTION_ANGVEL_REFERENCE reproduces the reference's arithmetic, which reorders the quaternion to wxyz and then hands it
 * to a scalar-LAST constructor (:131-135) -- the log of another rotation; the default is the physical world-frame angular
 * velocity.  A library is immutable once its fill has completed, so sample calls on different streams may be in flight
 * together; a sample must not be enqueued where it could run before the fill has finished. */
typedef struct gmr_motion_lib gmr_motion_lib_t;
#define GMR_MOTION_ANGVEL_WORLD     0   /* fill flags */
#define GMR_MOTION_ANGVEL_REFERENCE 1
#define GMR_MOTION_LOOP             1   /* sample flag: time modulo the clip's duration; without it, time clamped to duration - dt */
/* array ids of gmr_motion_lib_array */
#define GMR_MOTION_ROOT_POS       0
#define GMR_MOTION_ROOT_ROT       1
#define GMR_MOTION_DOF_POS        2
#define GMR_MOTION_LOCAL_BODY_POS 3
#define GMR_MOTION_ROOT_VEL       4
#define GMR_MOTION_ROOT_ANG_VEL   5
#define GMR_MOTION_DOF_VEL        6
#define GMR_MOTION_STATS          7
#define GMR_MOTION_SEG_START      8   /* i32 [C + 1] */
#define GMR_MOTION_FPS            9   /* f64 [C]     */
/* seg_start i32[C + 1] and fps f64[C] are HOST arrays, checked here (seg_start from 0, not descending, seg_start[C] == B; fps
 * positive and finite; C, B >= 1) and uploaded: the kernels trust the library's own copy, never a caller's table. */
int gmr_motion_lib_create(int C, int B, int ndof, int nbody, const int32_t* seg_start, const double* fps, gmr_motion_lib_t** out);
int gmr_motion_lib_destroy(gmr_motion_lib_t* lib);
/* The inputs as gmr_postprocess_clips_dev leaves them: root_pos f64[B][3], root_rot f64[B][4] xyzw, dof_pos f64[B][ndof],
 * local_body_pos f32[B][nbody][3] (16-byte aligned) or NULL.  Two launches (fill, stats), asynchronous on `stream`; no load
 * leaves rows [0, B) of the inputs. */
int gmr_motion_lib_fill_dev(gmr_motion_lib_t* lib, const double* d_root_pos, const double* d_root_rot_xyzw,
                            const double* d_dof_pos, const float* d_local_body_pos, int flags, void* stream);
int gmr_motion_lib_fill(gmr_motion_lib_t* lib, const double* root_pos, const double* root_rot_xyzw, const double* dof_pos,
                        const float* local_body_pos, int flags);   /* host buffers; synchronises */
/* device address and size of one array of the library (local_body_pos: NULL / 0 when the fill had none) */
int gmr_motion_lib_array(const gmr_motion_lib_t* lib, int which, void** d_ptr, size_t* bytes);
/* N queries (clip i32[N], time f64[N]) in one launch.  t = time mod duration with GMR_MOTION_LOOP (Python's %), else
 * min(time, duration - dt); x = t fps, lo = floor(x), hi = min(lo + 1, T - 1), blend = x - lo; lo == hi: the frame itself,
 * otherwise (float)(1 - blend) a[lo] + (float)blend a[hi] (multiply and add rounded separately) and the reference's
 * float32 slerp for root_rot (:205-233).  A frame index outside the clip (negative time without loop, t fps rounding up
 * to T) is clamped to the nearest frame.  Outputs row-major [N][3] [N][4] [N][3] [N][3] [N][ndof] [N][ndof] [N][nbody][3];
 * any of them may be NULL and is skipped.  A clip id outside [0, C), an empty clip or a non-finite time: that query's rows
 * are NaN and status[i] = 1 (else 0); nothing of the library is read for it. */
int gmr_motion_sample_dev(const gmr_motion_lib_t* lib, int N, const int32_t* d_clip, const double* d_time, int flags,
                          float* d_root_pos, float* d_root_rot, float* d_root_vel, float* d_root_ang_vel, float* d_dof_pos,
                          float* d_dof_vel, float* d_local_body_pos, int32_t* d_status, void* stream);
int gmr_motion_sample(const gmr_motion_lib_t* lib, int N, const int32_t* clip, const double* time, int flags, float* root_pos,
                      float* root_rot, float* root_vel, float* root_ang_vel, float* dof_pos, float* dof_vel,
                      float* local_body_pos, int32_t* status);   /* host buffers; synchronises */

/* Per-body state per query: one launch samples N (clip, time) queries as gmr_motion_sample_dev does and walks the FK tree
 * of `fk` on the sampled state.  All outputs float32, world frame, rows in the order of the selection:
 *   body_pos [N][nsel][3], body_rot [N][nsel][4] xyzw   the float32 FK of (root_pos, root_rot, dof_pos) as gmr_fk_batch_dev
 *                                                      computes it (the same per-body code: bit-equal)
 *   body_vel [N][nsel][3]      velocity of the body frame's origin:  v_0 = root_vel,      v_b = v_p + w_p x (p_b - p_p)
 *   body_ang_vel [N][nsel][3]  angular velocity of the body:         w_0 = root_ang_vel,  w_b = w_p + (R_b a_b) dof_vel[dof of b]
 *                              (p: the parent, a_b: the normalised hinge axis, R_b: the body's world rotation; w_b = w_p for a
 *                              body without a hinge)
 * and the six arrays of the sampler, bit-equal to gmr_motion_sample_dev's.  The velocities are the library's own (backward
 * differences, lerped) carried through the tree, not a derivative of the interpolated pose.  Any output pointer may be NULL
 * and is skipped.  body_sel: HOST array i32[nsel] of distinct bodies in [0, nbody), 1 <= nsel <= 64, in any order, or NULL
 * for all bodies in tree order (nsel is then ignored); it is validated here and travels as a kernel argument.  A bad query
 * (as in the sampler): every requested row of it NaN, status[i] = 1, nothing of the library read.  GMR_ERR_ARG when the
 * library was filled with GMR_MOTION_ANGVEL_REFERENCE (that root_ang_vel is not a physical angular velocity: propagating it
 * through the tree would be meaningless) and when fk's ndof is not the library's.  Asynchronous on `stream`; no device
 * scratch, nothing of either handle is written: calls on different streams may be in flight together. */
typedef struct {            /* device pointers (gmr_motion_body_state: host pointers), each may be NULL */
  float *root_pos, *root_rot, *root_vel, *root_ang_vel, *dof_pos, *dof_vel;   /* = gmr_motion_sample_dev, same bits */
  float *body_pos, *body_rot, *body_vel, *body_ang_vel;                        /* [N][nsel][3|4|3|3], world frame    */
  int32_t* status;                                                            /* [N]                                */
} gmr_body_state_out_t;
int gmr_motion_body_state_dev(const gmr_motion_lib_t* lib, gmr_fk_t* fk, int N, const int32_t* d_clip, const double* d_time,
                              int flags, const int32_t* body_sel, int nsel, const gmr_body_state_out_t* out, void* stream);
int gmr_motion_body_state(const gmr_motion_lib_t* lib, gmr_fk_t* fk, int N, const int32_t* clip, const double* time, int flags,
                          const int32_t* body_sel, int nsel, const gmr_body_state_out_t* out);   /* host buffers; synchronises */

/* ---- N4: motion tracker (the reference source of an imitation environment: clocks, reference rows, tracking terms) -- */
/* What booster_gym/envs/t1_imitation.py does per environment and per step in Python -- _update_reference_motion (:103-200),
 * _reset_finished_motions / _reset_idx (:201-235) and the six _reward_imitation_* terms (:249-309) -- for N environments
 * bound to one motion library, ONE kernel launch per step.  Per environment e the tracker holds, on the
 * device: clip i32, time f32 (the reference's motion_times is a float32 tensor), length f32 = (float)(T / fps) of that clip
 * and draws u32, the random draws made for e so far.  A new tracker has every environment on clip 0 at time 0.
 * A step, per environment and in the order of :103-207:
 *   1. the library is sampled at (clip, (double)time), GMR_MOTION_LOOP or clamp as given at creation: the same code as
 *      gmr_motion_sample_dev, the same bits
 *   2. ref_root_pos [N][3], ref_root_rot [N][4] xyzw, ref_root_vel, ref_root_ang_vel [N][3] as sampled; ref_dof_pos / ref_dof_vel
 *      [N][R] in ROBOT dof order: robot dof j takes column dof_map[j] of the library, or, for dof_map[j] = -1, dof_default[j]
 *      and velocity 0 (:139-161: head zero, stage-1 legs at their default pose)
 *   3. with simulator state: err [N][6] = |base_pos - ref|, 2 acos(min(|<base_quat, ref_root_rot>|, 1)) (the w of
 *      conj(q) * q_ref, :256-270), |base_lin_vel - ref|, |base_ang_vel - ref|, |w (dof_pos - ref)|, |w (dof_vel - ref)| in
 *      float32 (w: dof_weight, ones = the reference's formula); term [N][6] = exp(-err / scale); total [N] = the sum of
 *      weight_k term_k over the terms whose weight is not zero and whose simulator array was given (:341-345).  err and
 *      term of an array that was not given are 0.
 *   4. time = time + (float)dt, in float32
 *   5. without GMR_MOTION_LOOP: time >= length redraws the clip, sets time = 0 and finished[e] = 1 (else 0)
 *   6. a clip id outside [0, C), an empty clip or a non-finite time: every requested row of e is NaN, status[e] = 1 (else 0),
 *      finished[e] = 0, nothing of the library is read and the clock does not move
 * A random draw is one Philox4x32-10 call with key = seed (low word first) and counter = (e, draws[e], 0, 0), after which
 * draws[e] += 1: the result depends on neither the launch shape nor the order of calls on other environments.  Word 0
 * chooses the clip -- (word0 * C) >> 32, or with clip_weights the largest k with cdf[k] <= word0 2^-32, cdf[k] = (w_0 + ..
 * + w_{k-1}) / sum in float64 (a clip of weight zero is never drawn) -- and word 1 gives u = (word1 >> 8) 2^-24 in [0, 1).
 * A tracker is SINGLE-STREAM: its kernels read and write its own state, so every *_dev call on one tracker goes to one stream
 * (or the caller orders the streams); a step must not run before the library's fill has finished.  The plain entry points
 * take host buffers, run on the default stream, synchronise the device and hold the tracker's mutex throughout.  The
 * library must outlive the tracker. */
typedef struct gmr_motion_tracker gmr_motion_tracker_t;
#define GMR_TRACKER_MAX_DOF 64
typedef struct {            /* outputs of a step: device pointers (gmr_motion_tracker_step: host pointers), each may be NULL */
  float *ref_root_pos, *ref_root_rot, *ref_root_vel, *ref_root_ang_vel;   /* [N][3|4|3|3]                       */
  float *ref_dof_pos, *ref_dof_vel;                                       /* [N][R], robot dof order            */
  float *err, *term;                                                      /* [N][6]; need the simulator state   */
  float *total;                                                           /* [N];    needs the simulator state  */
  int32_t *status, *finished;                                             /* [N]                                */
} gmr_tracker_out_t;
typedef struct {            /* simulator state of a step: device pointers (host for the plain call), each may be NULL */
  const float *base_pos, *base_quat /* xyzw */, *base_lin_vel, *base_ang_vel;   /* [N][3|4|3|3] */
  const float *dof_pos, *dof_vel;                                               /* [N][R]       */
} gmr_tracker_sim_t;
/* HOST arrays, validated here: dof_map i32[R] with entries in [-1, ndof) or NULL for the identity (R = the library's ndof),
 * dof_default f32[R] or NULL (zeros), dof_weight f32[R] finite or NULL (ones), clip_weights f64[C] finite, not negative and
 * not all zero, or NULL (uniform).  1 <= R <= GMR_TRACKER_MAX_DOF, 1 <= N <= 2^26, dt finite; flags: GMR_MOTION_LOOP.
 * The terms start with the scales of T1Imitation.yaml:327-332 (0.5, 0.5, 2.0, 1.0, 1.0, 0.1) and weights of one. */
int gmr_motion_tracker_create(const gmr_motion_lib_t* lib, int N, double dt, int flags, int R, const int32_t* dof_map,
                              const float* dof_default, const float* dof_weight, const double* clip_weights, uint64_t seed,
                              gmr_motion_tracker_t** out);
int gmr_motion_tracker_destroy(gmr_motion_tracker_t* t);
/* Replaces the dof tables (a curriculum changes them between stages, :145-158); R may change with them.  The tables travel with
 * every launch, so steps already enqueued keep the ones they were launched with. */
int gmr_motion_tracker_set_dof_map(gmr_motion_tracker_t* t, int R, const int32_t* dof_map, const float* dof_default,
                                   const float* dof_weight);
/* scale f32[6] positive and finite, weight f32[6] finite (0 skips the term); either may be NULL and is then kept (:249-309) */
int gmr_motion_tracker_set_terms(gmr_motion_tracker_t* t, const float* scale, const float* weight);
/* (clip, time) of the n listed environments, or of all N in order with env_ids = NULL (n = N); ids outside [0, N) are ignored
 * and counted, an id listed twice takes one of its two rows.  A clip id outside [0, C) is stored as it is (step 6). */
int gmr_motion_tracker_assign_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_clip,
                                  const float* d_time, void* stream);            /* asynchronous */
int gmr_motion_tracker_assign(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* clip, const float* time,
                              int* ignored /* ids of this call outside [0, N), or NULL */);
/* _reset_idx (:215-235) for the n listed environments, or for all with env_ids = NULL: one draw each; with `resample` its
 * word 0 redraws the clip, and in either case time = lo + (hi - lo) u in float32 (time_offset_range).  Ids outside [0, N)
 * are ignored and counted.  An id listed twice in one call gives that environment one of the two possible outcomes (one or
 * two draws) and touches no other: list every environment once.  gmr_motion_tracker_reset_done_dev (N7) takes the done flags
 * themselves instead of a list and cannot have that problem. */
int gmr_motion_tracker_reset_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, int resample, float lo, float hi,
                                 void* stream);                                  /* asynchronous */
int gmr_motion_tracker_reset(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, int resample, float lo, float hi,
                             int* ignored /* ids of this call outside [0, N), or NULL */);
/* One environment step (:103-207, :249-309) in one launch; sim may be NULL (then err, term and total must be). */
int gmr_motion_tracker_step_dev(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, const gmr_tracker_out_t* out,
                                void* stream);                                   /* asynchronous */
int gmr_motion_tracker_step(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, const gmr_tracker_out_t* out);
/* the state on the host: clip i32[N], time f32[N], length f32[N], draws u32[N] (each may be NULL) and the ids ignored since
 * creation; synchronises */
int gmr_motion_tracker_state(gmr_motion_tracker_t* t, int32_t* clip, float* time, float* length, uint32_t* draws,
                             uint32_t* ignored);

/* ---- N5: tracker links (per-link targets and whole-body tracking terms of a motion tracker) ---- */
/* A tracker may have LINKS attached: an FK handle of the robot and a selection of 1 <= nsel <= 64 distinct bodies in any order.
 * The library must have been filled in GMR_MOTION_ANGVEL_WORLD mode and the handle's ndof must be the library's: the rules, and
 * the errors, of gmr_motion_body_state_dev.  A LINK STEP does everything gmr_motion_tracker_step_dev does -- the same bits in the
 * same outputs, the same clock / redraw / finished / status -- and, in the same launch, per environment e:
 *   1. ref_body_pos [N][nsel][3], ref_body_rot [N][nsel][4] xyzw, ref_body_vel, ref_body_ang_vel [N][nsel][3]: the float32 FK and
 *      velocity propagation of gmr_motion_body_state_dev applied to the library's own sampled state at (clip, (double)time), rows
 *      in selection order.  In GMR_TRACKER_FRAME_WORLD they are bit-equal to what gmr_motion_body_state_dev returns for that
 *      (clip, (double)time) and selection.  The dof_map does NOT enter: link targets come from the motion as retargeted, in the
 *      library's dof order -- also while a curriculum stage parks the legs at their defaults in ref_dof_pos.
 *   2. with simulator link state, in float32, w_b >= 0 the link weights and W = sum w_b > 0:
 *        d_b = |p_b - ref p_b|                          theta_b = 2 acos(min(|<q_b, ref q_b>|, 1))
 *        link_err [N][4] = sqrt(sum_b w_b x_b^2 / W) for x_b = d_b, theta_b, |v_b - ref v_b|, |om_b - ref om_b|
 *        link_term [N][4] = exp(-link_err / link_scale)
 *        max_dist [N] = the largest d_b over the links with w_b > 0 (NaN if any such d_b is NaN)
 *        fail [N] = !(max_dist <= fail_dist): with fail_dist = +inf only a non-finite distance fails
 *        total [N] (of gmr_tracker_out_t) = the six weighted terms + sum_k link_weight_k link_term_k
 *      A link of weight zero is not read.  As for the six terms: a term whose weight is zero or whose array was not given stays
 *      out of the total; err and term of an array that was not given are 0 (max_dist 0 and fail 0 without body_pos).
 *   3. GMR_TRACKER_FRAME_HEADING: each side is expressed relative to its OWN root with the root's yaw removed, before
 *      differencing and before ref_body_* is written:
 *        p' = Rz(-psi)(p - p_root)   q' = conj(q_psi) q   v' = Rz(-psi) v   om' = Rz(-psi) om
 *        q_psi = normalize(0, 0, q_root.z, q_root.w), the identity when z = w = 0
 *      The reference side takes the sampled root, the simulator side base_pos / base_quat of gmr_tracker_sim_t, which are then
 *      mandatory.  The link terms do not see drift in x, y and yaw; they do see a tilted or sunken robot.
 *   4. a bad assignment (step 6 of the tracker): every requested link row is NaN, fail = 0, status = 1, the clock stays.
 * GMR_TRACKER_NO_ADVANCE computes every output at the current clocks and leaves the tracker's state as it is (no clock advance,
 * no redraw, finished = 0): after gmr_motion_tracker_reset_dev that is reference-state initialisation.
 * The link scales start at (0.3 m, 0.8 rad, 2.0 m/s, 4.0 rad/s) with weights of one and fail_dist = +inf: a choice of this
 * library, the reference has no link terms.  The plan of the walk, the weights and the term constants travel with every launch,
 * so launches already enqueued keep theirs.  The FK handle must outlive the tracker; the tracker stays single-stream. */
#define GMR_TRACKER_FRAME_WORLD 0
#define GMR_TRACKER_FRAME_HEADING 1
#define GMR_TRACKER_NO_ADVANCE 1
#define GMR_TRACKER_LINK_TERMS 4
typedef struct {            /* link outputs of a step: device pointers (gmr_motion_tracker_step_links: host), each may be NULL */
  float *ref_body_pos, *ref_body_rot, *ref_body_vel, *ref_body_ang_vel;   /* [N][nsel][3|4|3|3]                  */
  float *link_err, *link_term;                                            /* [N][4]; need the simulator's links  */
  float *max_dist;                                                        /* [N];    needs the simulator's links */
  int32_t *fail;                                                          /* [N];    needs the simulator's links */
} gmr_tracker_links_out_t;
/* The simulator's rigid-body state: selection row s of environment e is read at base[e * env_stride + sim_body[s] * body_stride],
 * strides in floats.  A packed [N][nb][13] tensor (pos 3, quat xyzw 4, vel 3, ang vel 3) is the four pointers at offsets
 * 0 / 3 / 7 / 10 with strides 13 nb and 13.  env_stride = body_stride = 0 stands for four separate contiguous arrays
 * [N][nsel][3|4|3|3] with their natural strides (nsel k and k).  Both layouts give the same bits. */
typedef struct {
  const float *body_pos, *body_rot /* xyzw */, *body_vel, *body_ang_vel;   /* each may be NULL */
  int64_t env_stride, body_stride;
} gmr_tracker_links_sim_t;
/* HOST arrays, validated here: body_sel i32[nsel] distinct bodies of the tree, or NULL for all of them in order (nsel = nbody);
 * sim_body i32[nsel] in [0, 2^16) or NULL for the identity; link_weight f32[nsel] finite, not negative and not all zero, or NULL
 * (ones); frame GMR_TRACKER_FRAME_*.  nsel = 0 detaches the links (the other arguments are ignored). */
int gmr_motion_tracker_set_links(gmr_motion_tracker_t* t, gmr_fk_t* fk, const int32_t* body_sel, int nsel, const int32_t* sim_body,
                                 const float* link_weight, int frame);
/* scale f32[4] positive and finite, weight f32[4] finite (0 skips the term), either may be NULL and is then kept; fail_dist > 0
 * (+inf allowed) is set by every call */
int gmr_motion_tracker_set_link_terms(gmr_motion_tracker_t* t, const float* scale, const float* weight, float fail_dist);
/* One link step in one launch.  sim, links_sim, out and links_out may each be NULL; err / term need sim, total needs sim or
 * links_sim, link_err / link_term / max_dist / fail need links_sim.  Without attached links every pointer of links_out must be
 * NULL and links_sim is not looked at: a plain step with flags.  flags: GMR_TRACKER_NO_ADVANCE. */
int gmr_motion_tracker_step_links_dev(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, const gmr_tracker_links_sim_t* links_sim,
                                      const gmr_tracker_out_t* out, const gmr_tracker_links_out_t* links_out, int flags,
                                      void* stream);                             /* asynchronous */
/* host buffers; synchronises and holds the tracker's mutex.  Each given array of links_sim is copied from its first float to the
 * last one the strides reach (arrays that interleave in one tensor are copied once). */
int gmr_motion_tracker_step_links(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, const gmr_tracker_links_sim_t* links_sim,
                                  const gmr_tracker_out_t* out, const gmr_tracker_links_out_t* links_out, int flags);

/* ---- N6: tracker preview (future reference frames as observation rows of a motion tracker) ---- */
/* The observation half of an imitation environment (the stub `include_reference_in_obs` of t1_imitation.py:236-245): a tracker
 * may have a PREVIEW configured -- 1 <= K <= 16 clock offsets in seconds (finite, any sign, any order; typically 0, dt, 2 dt ..),
 * a set of blocks, a frame and, for the body block, 1 <= nsel <= 32 distinct rows of the library's local_body_pos.  A preview
 * call is ONE launch that reads the tracker's state and WRITES NOTHING of the tracker (no clock, no draw counter) and nothing of
 * the library: observations are taken after the resets that follow a step, at the clocks the next step will sample.
 * Per environment e and offset k: tq = (double)time[e] + (double)offset[k]; the library is sampled at (clip[e], tq) with the
 * tracker's loop flag by the code of gmr_motion_sample_dev (the same bits), so with offset 0 a preview shows the reference rows
 * the next step will emit.  obs f32 [N][K][D]: the selected blocks in this order, a block that is not selected takes no room,
 * D = the sum of the widths (R: the robot dofs of the tables the launch travels with):
 *   block          width    GMR_PREVIEW_FRAME_RAW             GMR_PREVIEW_FRAME_REFERENCE / _SIM
 *   ROOT_POS       3        sampled root_pos                  Rz(-psi_a) (p - p_a)
 *   ROOT_QUAT      4        sampled root_rot xyzw             q_rel = conj(q_psi_a) q, xyzw
 *   ROOT_ROT6      6        columns 0 and 1 of R(q)           columns 0 and 1 of R(q_rel)
 *   ROOT_VEL       3        sampled root_vel                  Rz(-psi_a) v
 *   ROOT_ANG_VEL   3        sampled root_ang_vel              Rz(-psi_a) w
 *   DOF_POS        R        robot dof order through dof_map, dof_default[j] where the map is -1 (as in a step); every frame
 *   DOF_VEL        R        through dof_map, 0 where the map is -1; every frame
 *   BODY_POS       3 nsel   sampled local_body_pos rows       Rz(-psi_a) (p + R(q) l_b - p_a)
 * (p, q, v, w, l_b): the sampled root position, quaternion, velocity, angular velocity and local body position at tq.
 * q_psi = normalize(0, 0, q.z, q.w), the identity where z = w = 0; Rz(-psi) from it as c = w'^2 - z'^2, s = 2 z' w',
 * (x, y, z) -> (c x + s y, c y - s x, z): the heading frame of the tracker links.  R(q), q xyzw NOT renormalised:
 * col0 = (1 - 2(y^2 + z^2), 2(xy + zw), 2(xz - yw)), col1 = (2(xy - zw), 1 - 2(x^2 + z^2), 2(yz + xw)), written col0 then col1;
 * R(q) l = l + w t + u x t, t = 2 (u x l), u = (x, y, z).  All of it float32 with one rounding per operation.
 * The anchor (p_a, q_a): FRAME_REFERENCE -- the reference root at the environment's current clock (the query at offset 0, whether
 * or not 0 is among the offsets); FRAME_SIM -- base_pos[e], base_quat[e] of gmr_tracker_sim_t, the only two members read and
 * then mandatory.
 *   valid i32 [N][K]  1 iff 0 <= tq <= duration - 1 / fps of the clip in float64 (inside the clip: neither wrapped by the loop
 *                     nor clamped), else 0.  The values of a wrapped or clamped frame are written all the same.
 *   status i32 [N]    step 6 of the tracker: a clip id outside [0, C), an empty clip or a non-finite clock -- every obs float of
 *                     e NaN, its valid 0, status 1 (else 0), nothing of the library read.
 * obs, valid and status may each be NULL.  The configuration is host state that travels with each launch as a kernel argument:
 * replacing it needs no copy and no synchronisation, launches already enqueued keep theirs; gmr_motion_tracker_set_dof_map may
 * change R and with it D.  The tracker stays single-stream: a preview reads what a step or reset writes. */
#define GMR_PREVIEW_ROOT_POS 1
#define GMR_PREVIEW_ROOT_QUAT 2
#define GMR_PREVIEW_ROOT_ROT6 4
#define GMR_PREVIEW_ROOT_VEL 8
#define GMR_PREVIEW_ROOT_ANG_VEL 16
#define GMR_PREVIEW_DOF_POS 32
#define GMR_PREVIEW_DOF_VEL 64
#define GMR_PREVIEW_BODY_POS 128
#define GMR_PREVIEW_FRAME_RAW 0
#define GMR_PREVIEW_FRAME_REFERENCE 1
#define GMR_PREVIEW_FRAME_SIM 2
#define GMR_PREVIEW_MAX_OFFSETS 16
#define GMR_PREVIEW_MAX_BODIES 32
/* HOST arrays, validated here: offsets f32[K], body_sel i32[nsel] rows of local_body_pos (looked at only with BODY_POS, and
 * then mandatory).  K = 0 removes the configuration (the other arguments are ignored).  GMR_ERR_ARG: K or nsel out of range, a
 * non-finite offset, unknown block bits, no block, an unknown frame, BODY_POS without a selection or on a library filled without
 * local_body_pos, a body outside [0, nbody) or listed twice, a selection without BODY_POS, ROOT_ANG_VEL in an anchored frame on
 * a library filled with GMR_MOTION_ANGVEL_REFERENCE (that row is not a vector to rotate).  *row_width (may be NULL) = D under
 * the current dof tables. */
int gmr_motion_tracker_set_preview(gmr_motion_tracker_t* t, int K, const float* offsets, int blocks, int frame, const int32_t* body_sel,
                                   int nsel, int* row_width);
/* One preview in one launch; GMR_ERR_ARG without a configured preview and in FRAME_SIM without base_pos / base_quat. */
int gmr_motion_tracker_preview_dev(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, float* d_obs, int32_t* d_valid,
                                   int32_t* d_status, void* stream);             /* asynchronous */
/* host buffers; default stream, synchronises and holds the tracker's mutex */
int gmr_motion_tracker_preview(gmr_motion_tracker_t* t, const gmr_tracker_sim_t* sim, float* obs, int32_t* valid, int32_t* status);

/* ---- N7: tracker adaptive sampling (failure-driven episode starts and masked resets of a motion tracker) ---- */
/* Opt-in, a capability of this library (the reference resets in a Python loop and starts every finished motion at time 0).  The
 * statement of record is tests/adaptive_mirror.py; this is the same in words.
 * BINS, in frames.  Clip c has T_c frames at fps_c.  F_c = max(1, llround(bin_seconds fps_c)) frames per bin, nb_c = ceil(T_c / F_c)
 * bins (none for T_c = 0); bin k covers frames [k F_c, min((k + 1) F_c, T_c)).  bin_start i32[C + 1] is the prefix sum of nb_c,
 * Bt = bin_start[C], 1 <= Bt <= 2^22.  The bin of an environment is bin_start[clip] + min(lo / F_c, nb_c - 1) in integers, lo being
 * the lower frame of the sampler's query at (clip, (double)time, loop), counted from the clip's first frame; a bad assignment (step 6
 * of the tracker) has no bin.
 * BASE.  base[b] = Wn_c frames(b) / T_c in float64 on the host; Wn_c = w_c / (the sum of w over the clips that have frames, added in
 * clip order), w = the tracker's clip_weights or ones.  base sums to 1; a clip of weight zero has base 0.
 * RECORDING.  fail_now u32[Bt]: a masked reset adds 1 (an integer atomic) to the bin of every done environment whose failed flag is
 * not zero, at the clock it has when the reset runs.
 * ADAPT, all float64, one rounding per operation, in this order:
 *   1. ema[b] = (1 - alpha) ema[b] + alpha (double)fail_now[b]; fail_now[b] = 0
 *   2. s[b] = sum over u = 0 .. K-1, ascending, of g[u] ema[min(b + u, last bin of b's clip)], g[u] = gamma^u by repeated
 *      multiplication on the host; s[b] = 0 for a clip of weight zero.  A failure in bin b raises the K - 1 bins in front of it,
 *      inside its clip: an episode has to start before the point where it falls.
 *   3. S = sum of s (order: DESIGN.md 6n); p[b] = base[b] if S == 0, else ((1 - uniform) s[b]) / S + uniform base[b]
 *   4. cdf[b] = p[0] + .. + p[b-1] (order: DESIGN.md 6n): cdf[0] = 0, cdf never decreases, a bin of p = 0 has cdf[b + 1] == cdf[b]
 * DRAW from the bins: the Philox call of the tracker (counter (e, draws[e], 0, 0), draws[e] += 1); b = the largest bin with
 * cdf[b] <= word0 2^-32; clip = the clip of b, k = b - bin_start[clip]; u from word 1;
 * time = (float)(((double)(k F_c) + (double)u (double)frames(b)) / fps_c); length as everywhere.
 * A step of an adaptive tracker redraws a finished clip (GMR_MOTION_LOOP off) with this draw -- clip and start time from the bins,
 * nothing recorded -- instead of "clip by weight, time 0".  gmr_motion_tracker_reset[_dev] and assign[_dev] are unchanged: on an
 * adaptive tracker they still draw from the clip weights and the offset range and do not read the bins. */
/* bin_seconds > 0 builds the bins (synchronous: reads the library's seg_start / fps back, allocates once, runs one Adapt, so a fresh
 * configuration draws from base); called again with the same bin_seconds it only replaces alpha, uniform, K and gamma -- a host
 * assignment, no Adapt, ema is kept, Adapts already enqueued keep the parameters they were launched with.  bin_seconds <= 0 turns
 * adaptive sampling off (synchronises; the tracker draws as a plain one again).  GMR_ERR_ARG: alpha or uniform outside [0, 1],
 * K outside [1, 16], gamma outside (0, 1], Bt outside [1, 2^22], every clip with frames of weight zero. */
int gmr_motion_tracker_set_adaptive(gmr_motion_tracker_t* t, double bin_seconds, double alpha, double uniform, int K, double gamma);
/* One Adapt, three launches; GMR_ERR_ARG on a plain tracker.  Typically once per rollout. */
int gmr_motion_tracker_adapt_dev(gmr_motion_tracker_t* t, void* stream);          /* asynchronous */
int gmr_motion_tracker_adapt(gmr_motion_tracker_t* t);                            /* default stream, synchronises */
/* The MASKED RESET, one launch, no allocation, no synchronisation, no read-back.  d_done / d_failed are i32 masks on the device.
 *   with d_env_ids   i32[n]: entry i is environment d_env_ids[i]; d_done[i] / d_failed[i] belong to entry i
 *   without          n = N: environment e is reset iff d_done[e] != 0
 * d_done = NULL resets every entry; d_failed = NULL records nothing.  An entry that is not done is not looked at (no draw, and its id
 * is not read); ids of done entries outside [0, N) are ignored and counted.  Every environment at most once in a list.
 *   plain tracker     the draw, clip and time = lo + (hi - lo) u of gmr_motion_tracker_reset_dev, the same bits; d_failed is ignored
 *   adaptive tracker  record (failed), then the draw from the bins; needs resample = 1 and lo = hi = 0, else GMR_ERR_ARG */
int gmr_motion_tracker_reset_done_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_done,
                                      const int32_t* d_failed, int resample, float lo, float hi, void* stream);   /* asynchronous */
int gmr_motion_tracker_reset_done(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* done, const int32_t* failed,
                                  int resample, float lo, float hi, int* ignored /* ids of this call outside [0, N), or NULL */);
/* the adaptive state on the host: bin_start i32[C + 1], fail_now u32[Bt], ema / prob / cdf f64[Bt], each may be NULL (ask for bin_start
 * first: Bt = bin_start[C]); synchronises; GMR_ERR_ARG on a plain tracker */
int gmr_motion_tracker_adaptive_state(gmr_motion_tracker_t* t, int32_t* bin_start, uint32_t* fail_now, double* ema, double* prob,
                                      double* cdf);

/* ---- N8: tracker anchors (a per-environment rigid move of the reference about the vertical) ---- */
/* Opt-in, a capability of this library.  A simulator spreads its N environments over a grid of origins and a robot faces wherever it
 * faces after a reset; the clips of a library all live in the coordinates of their files.  An anchor is what lies between the two: per
 * environment a yaw psi_e about z, then a translation t_e, kept on the device beside the clocks and applied to every world-frame
 * quantity the tracker emits or compares.  The statement of record is tests/anchor_mirror.py; this is the same in words.
 * STATE per environment: anchor_pos f32[3] = t, anchor_yaw f32[2] = (z, w) of the unit quaternion (0, 0, z, w).  Identity: (0, 0, 0),
 * (0, 1).
 * ARITHMETIC, float32, one rounding per operation, in exactly this order:
 *   c = w w - z z, s = 2 z w
 *   position    x' = (c x - s y) + tx, y' = (s x + c y) + ty, z' = z + tz
 *   vector      x' = c x - s y, y' = s x + c y, z untouched (linear and angular velocity)
 *   quaternion  xyzw, not renormalised: (w qx - z qy, w qy + z qx, w qz + z qw, w qw - z qz)
 * WHERE.
 *   1. gmr_motion_tracker_step[_dev] / step_links[_dev]: ref_root_pos and ref_root_rot are anchored, ref_root_vel and ref_root_ang_vel
 *      rotated; the four root terms compare against those rows.  Dof rows and dof terms are untouched.
 *   2. step_links, GMR_TRACKER_FRAME_WORLD: the finished world row of every selected body -- after the walk, before it is written and
 *      differenced -- so ref_body_* and the link terms, max_dist and fail are the anchored ones.  GMR_TRACKER_FRAME_HEADING removes
 *      every common x / y / yaw: its link rows and link terms are bit-identical to an unanchored tracker's.
 *   3. preview: GMR_PREVIEW_FRAME_RAW anchors the root blocks (root_pos, root_quat, root_vel, root_ang_vel; root_rot6 is the matrix
 *      of the anchored quaternion), the root-local body block keeps its bits; GMR_PREVIEW_FRAME_SIM expresses the ANCHORED reference
 *      (root and bodies) relative to the simulator's root; GMR_PREVIEW_FRAME_REFERENCE keeps its bits.
 * A tracker on which anchors were never enabled (or are disabled again) runs the code it ran before they existed: the two arrays are
 * null and the test is one branch, uniform over the launch.  A redraw (GMR_MOTION_LOOP off) and a loop wrap leave the anchor as it is.
 * A yaw is refused (GMR_ERR_ARG) on a library filled with GMR_MOTION_ANGVEL_REFERENCE, whose root_ang_vel cannot be rotated; a
 * translation is fine there.  The angle of set_anchor becomes (sin(psi / 2), cos(psi / 2)) in float32 by a routine of this library
 * made of +, -, * and floor only (gmr_tracker_anchor.hip, anchor_half_angle; tests/anchor_mirror.py half_angle), on the host for the
 * synchronous entry point and in the kernel for _dev: the same bits both ways. */
#define GMR_ANCHOR_YAW 1   /* anchor_to_root: take the yaw from the given root (else it is kept) */
#define GMR_ANCHOR_Z   2   /* anchor_to_root: take t_z too (else it is kept) */
/* on != 0: allocates the two arrays and fills them with the identity (synchronous; the only allocation of the feature; nothing happens
 * when they are there already).  on == 0: synchronises, frees them, the tracker is a plain one again. */
int gmr_motion_tracker_enable_anchors(gmr_motion_tracker_t* t, int on);
/* Sets the anchors of the n listed environments (d_env_ids NULL: all of them, in order, n = N): pos f32[n][3] and / or yaw f32[n] in
 * radians, a NULL part is kept.  Ids outside [0, N) are dropped and counted as gmr_motion_tracker_reset counts them.  One launch.
 * _dev: GMR_ERR_ARG unless anchors are enabled; values are not looked at.  The synchronous twin enables anchors first, refuses
 * non-finite input before anything is touched and reports the ids of this call that were dropped. */
int gmr_motion_tracker_set_anchor_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const float* d_pos, const float* d_yaw,
                                      void* stream);                                                       /* asynchronous */
int gmr_motion_tracker_set_anchor(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const float* pos, const float* yaw,
                                  int* ignored /* or NULL */);
/* Anchors the reference to where the robot is.  ONE launch, no allocation, no synchronisation, no read-back.  Entry i is environment
 * d_env_ids[i] (without a list: environment i, n = N); d_mask i32[n] (NULL: every entry), d_root_pos f32[n][3] and d_root_quat
 * f32[n][4] xyzw belong to entry i, as the masks of gmr_motion_tracker_reset_done_dev do.  For every entry whose mask is not zero:
 *   (p_r, q_r) = the reference root at (clip, (double)time) under the tracker's loop mode, the sampler's bits
 *   (z_r, w_r) = yaw(q_r), (z_s, w_s) = yaw(q_s): normalize(0, 0, q.z, q.w), the identity for z = w = 0; here with a correctly
 *     rounded float32 square root and division (the heading frame of N5 / N6 takes the hardware's square root, good to one ulp)
 *   GMR_ANCHOR_YAW: (z, w) = yaw(z_s w_r - w_s z_r, w_s w_r + z_s z_r); else (z, w) stays
 *   t_x = p_s.x - (c p_r.x - s p_r.y), t_y = p_s.y - (s p_r.x + c p_r.y) with c, s of the new (z, w)
 *   GMR_ANCHOR_Z: t_z = p_s.z - p_r.z; else t_z stays
 * A bad assignment (step 6 of the tracker) or a root that is not finite leaves that environment's anchor as it was.  Ids of masked
 * entries outside [0, N) are dropped and counted.  Every environment at most once in a list.  _dev: GMR_ERR_ARG unless anchors are
 * enabled; the synchronous twin enables them first. */
int gmr_motion_tracker_anchor_to_root_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_mask,
                                          const float* d_root_pos, const float* d_root_quat, int flags, void* stream);   /* asynchronous */
int gmr_motion_tracker_anchor_to_root(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* mask, const float* root_pos,
                                      const float* root_quat, int flags, int* ignored /* or NULL */);
/* the anchors on the host: pos f32[N][3], yaw_zw f32[N][2], each may be NULL; synchronises; GMR_ERR_ARG unless anchors are enabled */
int gmr_motion_tracker_anchor_state(gmr_motion_tracker_t* t, float* pos, float* yaw_zw);

/* ---- N9: tracker control (joint targets and the actuator model of a motion tracker) ---- */
/* The control half of an imitation step: the PD targets of booster_gym/envs/t1_imitation.py:386-415 -- the reference's joint row at the
 * environment's clock, eased in from the default pose over the first seconds of an episode, plus the clipped policy action as a
 * residual -- in ONE launch, and the actuator model that runs `decimation` times per step between physics substeps (:449-462,
 * t1.py:443-456) -- actuator delay, PD law, Coulomb friction, torque clip, running mean -- in ONE launch per substep.  The statement
 * of record is tests/control_mirror.py; this is the same in words.  Everything is float32 with one rounding per operation.
 * CONFIGURATION (a host assignment that travels with every launch): default_pos f32[R] d, action_scale k, clip_actions c,
 * startup_seconds D, gain_startup g0, gain_run g1, decimation M.  STATE (device, owned by the tracker, zero after set_control):
 * held f32[N][R], the targets the actuators hold (last_dof_targets), and torque_acc f32[N][R], the running sum of a step's torques.
 * TARGETS, for environment e and robot dof j:
 *   r       = what gmr_motion_tracker_step_dev would write to ref_dof_pos[e][j] at the environment's present (clip, clock): the same
 *             code, the same bits; the clock does not move, no draw is made, no tracker state is written
 *   te      = (float)episode_steps[e] * (float)dt; startup = te < D; p = min(max(te / D, 0), 1);
 *   s       = 0.5 * (1 - cosf(p * 3.14159f))   (the reference's literal, :403); without episode_steps: startup = false
 *   base    = startup ? d_j * (1 - s) + r * s : r
 *   a       = min(max(action, -c), c), a NaN stays one (t1.py:439); target = base + (k * a) * (startup ? g0 : g1); without actions
 *             target = base
 *   a bad assignment (step 6 of the tracker): status[e] = 1 (else 0), the target row is NaN, nothing of the library is read;
 *   actions_clipped is written all the same
 * TORQUES of substep i, per element: if (delay_steps ? delay_steps[e] : 0) == i then held = dof_targets (a delay outside [0, M)
 * never matches); tau = kp * (held - q) - kd * qd; with friction f = min(fr, |tau|) (a NaN propagates), tau = tau - f * sgn(tau),
 * sgn = +1, -1 or +0; with a limit tau = min(max(tau, -lim), lim); dof_torques = tau; torque_acc = (i == 0 ? 0 : torque_acc) + tau;
 * for i == M - 1 mean_torques = torque_acc / (float)M.
 * The tracker stays SINGLE-STREAM: targets reads its state, hold and torques write held / torque_acc.  Every call below is
 * GMR_ERR_ARG, before a device is touched, on a tracker whose control was never set, or whose dof map has changed R since. */
#define GMR_CONTROL_MAX_DECIMATION 64
typedef struct {            /* the actuators of a torques call: device pointers (gmr_motion_tracker_torques: host pointers) of the user */
  const float *stiffness, *damping;   /* kp, kd: [N][R] with per_env = 1, [R] with per_env = 0                         */
  const float *friction;              /* fr, shaped as the gains; NULL: no friction                                   */
  const float *torque_limit;          /* lim [R]; NULL: no clip                                                       */
  int32_t per_env;
} gmr_tracker_actuator_t;
/* HOST array default_dof_pos f32[R] finite (t1.py:264-272; R is the tracker's), action_scale and the gains finite, clip_actions > 0
 * (inf: no clipping), startup_seconds >= 0 and finite (0: no start-up phase; the reference's 2.0 at :388, gains 0.1 / 0.2 at :414),
 * 1 <= decimation <= GMR_CONTROL_MAX_DECIMATION.  Allocates held and torque_acc and fills them with zeros (the reference's
 * last_dof_targets and torques start as zeros); synchronises the device.  Launches in flight keep the configuration they carry. */
int gmr_motion_tracker_set_control(gmr_motion_tracker_t* t, const float* default_dof_pos, float action_scale, float clip_actions,
                                   float startup_seconds, float gain_startup, float gain_run, int decimation);
/* The joint targets (t1_imitation.py:386-415 with the clip of t1.py:439), ONE launch: actions f32[N][R] or NULL, episode_steps
 * i32[N] or NULL (the simulator's episode_length_buf; it stays the environment's); outputs dof_targets f32[N][R], actions_clipped
 * f32[N][R] (needs actions), status i32[N], each may be NULL. */
int gmr_motion_tracker_targets_dev(gmr_motion_tracker_t* t, const float* d_actions, const int32_t* d_episode_steps, float* d_dof_targets,
                                   float* d_actions_clipped, int32_t* d_status, void* stream);      /* asynchronous */
int gmr_motion_tracker_targets(gmr_motion_tracker_t* t, const float* actions, const int32_t* episode_steps, float* dof_targets,
                               float* actions_clipped, int32_t* status);
/* last_dof_targets[env_ids] = dof_pos[env_ids] after a reset (t1.py:309), ONE launch: entry i -- environment env_ids[i], or i with
 * env_ids = NULL (n = N), the convention of reset_done and anchor_to_root -- whose mask i32[n] is not zero (NULL: every entry) gets
 * held[e][:] = dof_pos[i][:] and torque_acc[e][:] = 0.  Ids of such entries outside [0, N) are dropped and counted.  Every
 * environment at most once in a list. */
int gmr_motion_tracker_hold_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_mask, const float* d_dof_pos,
                                void* stream);                                                      /* asynchronous */
int gmr_motion_tracker_hold(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* mask, const float* dof_pos,
                            int* ignored /* ids of this call outside [0, N), or NULL */);
/* The actuator model of physics substep i (t1_imitation.py:449-462, t1.py:443-456), ONE launch: dof_targets, dof_pos, dof_vel
 * f32[N][R], delay_steps i32[N] or NULL (no delay); writes dof_torques f32[N][R] and, when given and i = M - 1, mean_torques
 * f32[N][R].  0 <= substep < M, else GMR_ERR_ARG and no launch. */
int gmr_motion_tracker_torques_dev(gmr_motion_tracker_t* t, int substep, const float* d_dof_targets, const float* d_dof_pos,
                                   const float* d_dof_vel, const gmr_tracker_actuator_t* act, const int32_t* d_delay_steps,
                                   float* d_dof_torques, float* d_mean_torques, void* stream);      /* asynchronous */
int gmr_motion_tracker_torques(gmr_motion_tracker_t* t, int substep, const float* dof_targets, const float* dof_pos, const float* dof_vel,
                               const gmr_tracker_actuator_t* act, const int32_t* delay_steps, float* dof_torques, float* mean_torques);
/* held and torque_acc on the host (last_dof_targets, t1.py:309; the sum behind torques, t1.py:449-456): f32[N][R] each, either may
 * be NULL; synchronises */
int gmr_motion_tracker_control_state(gmr_motion_tracker_t* t, float* held, float* torque_acc);

/* ---- N10: tracker proprioception (observation rows, penalty terms and termination of a motion tracker) ---- */
/* What booster_gym/envs/t1.py::step does between "physics is done" and "the policy gets its next input", ONE launch per step: the
 * body-frame base state and the two filtered velocities (t1.py:463-473), the proprioceptive observation row and the privileged block
 * with sensor noise (:574-603, utils/utils.py:5-30), the fourteen regularisation penalties (:622-625, :631-694), the state-based
 * termination (:554-557) and the roll-over of last_actions / last_dof_vel / last_root_vel (:492-494).  The statement of record is
 * tests/proprio_mirror.py; this is the same in words.  Everything is float32 with one rounding per operation.
 * STATE (device, owned by the tracker, zero after set_proprio): filtered_lin_vel, filtered_ang_vel f32[N][3], last_root_vel f32[N][6],
 * last_actions, last_dof_vel f32[N][R], noise_tick u32[N].
 * THE STEP, for environment e (p, q = (qv, w), v, om: position, xyzw quaternion, world linear and angular velocity of root_states[e];
 * h = p.z - (ground ? ground[e] : 0)):
 *   rot(u)  = u * (2 * (w * w) - 1) - cross(qv, u) * w * 2 + qv * ((qv.x * u.x + qv.y * u.y) + qv.z * u.z) * 2   (quat_rotate_inverse,
 *             general_motion_retargeting/torch_utils.py:78-87, in this grouping; q is used as given, not normalised)
 *   base_lin_vel = rot(v), base_ang_vel = rot(om), projected_gravity = rot((0, 0, -1))
 *   filtered = base * (float)fw + filtered * (float)(1.0 - fw), written to the state and to the outputs
 *   obs[e]  = [noisy(projected_gravity) * s_g | noisy(base_ang_vel) * s_w | extra[e] | noisy(dof_pos - default) * s_q |
 *              noisy(dof_vel) * s_qd | actions (zeros without)], W = 6 + C + 3 R columns
 *   priv[e] = [noisy(base_lin_vel) * s_v | noisy(h)]
 *   term[e] = lin_vel_z: filtered_lin_vel.z^2; ang_vel_xy: base_ang_vel.x^2 + .y^2; orientation: projected_gravity.x^2 + .y^2;
 *             torques: sum tau^2; dof_vel: sum qd^2; dof_acc: sum ((last_dof_vel - qd) / (float)dt)^2; root_acc: sum over the six of
 *             ((last_root_vel - (v, om)) / (float)dt)^2 in rising order; action_rate: sum (last_actions - a)^2; dof_pos_limits: the
 *             count of q < lower or q > upper; dof_vel_limits: sum min(max(|qd| - vel_limit * soft, 0), 1); torque_limits: sum
 *             max(|tau| - torque_limit * soft, 0); torque_tiredness: sum min((tau / torque_limit)^2, 1); power: sum max(tau * qd, 0);
 *             base_height: (h - target)^2.  A min / max keeps a NaN.  A sum over the dofs: lane l of the environment's 16 adds the
 *             columns l, l + 16, .. in rising order, then x = x + x[lane ^ m] for m = 1, 2, 4, 8 (tracker_step_kernel's order).  A term
 *             without its input (tau: mean_torques, a: actions) is 0.
 *   total[e] = sum of scale_k * term_k in rising k over the terms with scale_k != 0 whose input is there
 *   done[e] = 1 * (sum over the six of (v, om)^2 in rising order > terminate_vel) | 2 * (h < terminate_height) |
 *             4 * (episode_steps[e] > max_episode_steps); a NaN compares false
 *   then last_actions = actions (kept without actions), last_dof_vel = dof_vel, last_root_vel = (v, om), noise_tick[e] += 1 if noise
 *   was applied.  No clock moves, no draw counter of the tracker moves, nothing of the library is read.
 * NOISE of element i of environment e (i: the obs column, or W + k for priv column k), when the launch's noise flag is set and the
 * block of the element has a spec: (w0, w1, w2, w3) = philox4x32(counter (e, noise_tick[e], i >> 1, 1), the tracker's key); an even i
 * takes (wa, wb) = (w0, w1), an odd i (w2, w3).  uniform: n = a + (float)(b - a) * philox_unit(wa).  gaussian: u1 = (float)((wa >> 8) +
 * 1) * 2^-24, u2 = philox_unit(wb), z = sqrtf(-2 * logf(u1)) * cosf(6.2831855f * u2), n = a + b * z.  additive: x + n, scaling: x * n
 * (utils/utils.py:9-25).  Word 3 = 1 of the counter keeps these draws apart from the (e, draws, 0, 0) of the tracker's resets.
 * The tracker stays SINGLE-STREAM.  Every call below is GMR_ERR_ARG, before a device is touched, on a tracker whose proprio was never
 * set, or whose dof map has changed R since. */
#define GMR_PROPRIO_TERMS 14
#define GMR_PROPRIO_MAX_EXTRA 16
#define GMR_PROPRIO_NOISE_BLOCKS 6     /* gravity, ang_vel, dof_pos, dof_vel, lin_vel, height */
#define GMR_NOISE_NONE 0
#define GMR_NOISE_GAUSSIAN 1
#define GMR_NOISE_UNIFORM 2
#define GMR_NOISE_ADDITIVE 0
#define GMR_NOISE_SCALING 1
typedef struct {            /* apply_randomization (utils/utils.py:5-30): range (a, b) is (mean, deviation) or (lower, upper) */
  int32_t distribution, operation;
  double a, b;
} gmr_proprio_noise_t;
typedef struct {            /* the configuration of set_proprio: HOST pointers and values */
  const float *default_dof_pos;       /* [R] (t1.py:264-272)                                                          */
  const float *dof_pos_limits;        /* [R][2] lower, upper (t1.py:665-670)                                          */
  const float *dof_vel_limits;        /* [R] (t1.py:677)                                                              */
  const float *torque_limits;         /* [R] (t1.py:684, :690)                                                        */
  const float *scales;                /* [GMR_PROPRIO_TERMS] the weights of the total                                 */
  int32_t extra_cols, max_episode_steps;
  double filter_weight;
  double soft_dof_pos_limit, soft_dof_vel_limit, soft_torque_limit;
  float scale_gravity, scale_lin_vel, scale_ang_vel, scale_dof_pos, scale_dof_vel;
  float base_height_target, terminate_vel, terminate_height;
  gmr_proprio_noise_t noise[GMR_PROPRIO_NOISE_BLOCKS];
} gmr_proprio_config_t;
typedef struct {            /* the inputs of a proprio call: device pointers (gmr_motion_tracker_proprio: host pointers) of the user */
  const float *root_states;           /* [N][13] position, xyzw quaternion, world linear and angular velocity         */
  const float *dof_pos, *dof_vel;     /* [N][R]                                                                       */
  const float *actions;               /* [N][R] the clipped actions, or NULL                                          */
  const float *mean_torques;          /* [N][R] or NULL                                                               */
  const float *extra;                 /* [N][C]; there if and only if C > 0                                           */
  const float *ground;                /* [N] terrain height under the base, or NULL: 0                                */
  const int32_t *episode_steps;       /* [N] or NULL: no time-out                                                     */
} gmr_proprio_in_t;
typedef struct {            /* the outputs of a proprio call, each an address or NULL */
  float *base_lin_vel, *base_ang_vel, *projected_gravity, *filtered_lin_vel, *filtered_ang_vel;   /* [N][3] */
  float *obs;                         /* [N][6 + C + 3 R]                                                             */
  float *priv;                        /* [N][4]                                                                       */
  float *term;                        /* [N][GMR_PROPRIO_TERMS]                                                       */
  float *total;                       /* [N]                                                                          */
  int32_t *done;                      /* [N]                                                                          */
} gmr_proprio_out_t;
/* The configuration (t1.py:264-272 for the pose, :468-472 the filter, :582-597 scales and noise, :665-690 the limits, :554-556 the
 * thresholds): every value finite, 0 <= extra_cols <= GMR_PROPRIO_MAX_EXTRA, b >= 0 for a gaussian, upper >= lower after the soft
 * factor, max_episode_steps >= 0 (the caller's ceil(episode_length_s / dt)).  The host forms lower = lim0 + (float)(0.5 * (1 - soft))
 * * (lim1 - lim0) and upper = lim1 - the same in float32.  Allocates the six state arrays and fills them with zeros; synchronises the
 * device.  Launches in flight keep the configuration they carry. */
int gmr_motion_tracker_set_proprio(gmr_motion_tracker_t* t, const gmr_proprio_config_t* cfg);
/* The step (t1.py:463-473, :554-557, :574-603, :622-694, :492-494), ONE launch; noise: 0 or 1 */
int gmr_motion_tracker_proprio_dev(gmr_motion_tracker_t* t, const gmr_proprio_in_t* in, int noise, const gmr_proprio_out_t* out,
                                   void* stream);                                                   /* asynchronous */
int gmr_motion_tracker_proprio(gmr_motion_tracker_t* t, const gmr_proprio_in_t* in, int noise, const gmr_proprio_out_t* out);
/* After a reset (t1.py:310-313), ONE launch: entry i -- environment env_ids[i], or i with env_ids = NULL (n = N), the convention of
 * hold and anchor_to_root -- whose mask i32[n] is not zero (NULL: every entry) gets filtered_lin_vel = filtered_ang_vel = 0 and
 * last_root_vel[e] = root_states[i][7:13] (root_states f32[n][13]); last_actions and last_dof_vel stay, as in the reference.  Ids of
 * such entries outside [0, N) are dropped and counted.  Every environment at most once in a list. */
int gmr_motion_tracker_proprio_reset_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_mask,
                                         const float* d_root_states, void* stream);                 /* asynchronous */
int gmr_motion_tracker_proprio_reset(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* mask, const float* root_states,
                                     int* ignored /* ids of this call outside [0, N), or NULL */);
/* the six state arrays on the host (filtered velocities t1.py:468-473, the three last_* of :492-494), each may be NULL; synchronises */
int gmr_motion_tracker_proprio_state(gmr_motion_tracker_t* t, float* filtered_lin_vel, float* filtered_ang_vel, float* last_root_vel,
                                     float* last_actions, float* last_dof_vel, uint32_t* noise_tick);

/* ---- N11: tracker feet (terrain heights, feet pose and contacts, the gait clock, contact-force termination, collision and the feet_*
 * terms of a motion tracker) ---- */
/* What booster_gym/envs/t1.py::step still did in small launches and host round trips: Terrain.terrain_heights
 * (booster_gym/utils/terrain.py:101-121, which copies the positions to the host, interpolates in NumPy and uploads the result, several
 * times per step), _refresh_feet_state (t1.py:529-549), the gait clock (:478, :585-586), the contact-force termination (:553),
 * collision (:627-629), the seven feet_* terms (:696-730) and the roll-over of last_feet_pos (:495), ONE launch per step.  The statement
 * of record is tests/feet_mirror.py; this is the same in words.
 * TERRAIN.  A field int16 [nx][ny], the first index is x (terrain.py:113), with horizontal_scale hs, vertical_scale vs and border_pixels
 * b; without a field the terrain is the plane: height 0, nothing loaded, nothing counted.  height(px, py), in the reference's NumPy
 * type promotion:
 *   x = (float)b + px / (float)hs, y likewise, in float32; x1 = floor(x), x2 = x1 + 1, y1, y2 likewise
 *   the four weights (x2 - x), (x - x1), (y2 - y), (y - y1) in float64 (exact)
 *   s = (((x2 - x) * (y2 - y)) * h[x1][y1] + ((x - x1) * (y2 - y)) * h[x2][y1]) + ((x2 - x) * (y - y1)) * h[x1][y2]
 *       + ((x - x1) * (y - y1)) * h[x2][y2] in float64, the sum from the left; height = (float)(s * vs): ONE rounding to float32
 * The reference wraps a negative index silently and raises past the edge; here each of the four indices is clamped to the field, the
 * weights stay as computed, and the point is counted in `outside`.  A coordinate x or y that is not finite gives NaN and is counted too.
 * FEET.  CONFIGURATION (a host struct that travels with every launch): gmr_feet_config_t.  STATE (device, owned by the tracker, zero after
 * set_feet): last_feet_pos f32[N][2][3], gait_process f32[N].  Everything below is float32 with one rounding per operation; T = 6.2831855f,
 * P = 3.1415927f; rem(a, T) = fmodf(a, T), plus T when that is negative (torch's remainder); wrap(a) = rem(a + P, T) - P.
 * THE STEP, for environment e (pos_f, q_f = (x, y, z, w): position and xyzw quaternion of body feet_body[f], f = 0 left, 1 right):
 *   feet_pos     = pos_f (:530)
 *   roll_f       = wrap(rem(atan2f(2 * (w * x + y * z), ((w * w - x * x) - y * y) + z * z), T))            (:532-533)
 *   yaw_f        = wrap(rem(atan2f(2 * (w * z + x * y), ((w * w + x * x) - y * y) - z * z), T))            (:534)
 *                  the roll and yaw of isaacgym's get_euler_xyz as restated here; not pinned to isaacgym, which no test machine has
 *   rot(q, v)    = (v * (2 * (w * w) - 1) + cross(qv, v) * w * 2) + qv * ((qv.x * v.x + qv.y * v.y) + qv.z * v.z) * 2   (quat_rotate,
 *                  general_motion_retargeting/torch_utils.py:66-75, a + b + c in this grouping; q as given, not normalised)
 *   edge_fk      = pos_f + rot(q_f, edge_pos[k]); contact_f = any over k of (edge_fk.z - height(edge_fk) < (float)clearance)   (:535-549)
 *   ground       = height(root position) (:555, :597, :624): what gmr_proprio_in_t takes as `ground`
 *   gait_process = fmodf(gait_process + (float)dt * gf, 1), gf = gait_frequency[e] or 0 (:478)
 *   gait         = (cosf(T * gait_process) * on, sinf(T * gait_process) * on), on = gf > 1e-8f ? 1 : 0 (:585-586)
 *   |F_b|        = sqrtf((F.x * F.x + F.y * F.y) + F.z * F.z) of contact_forces[e][b]
 *   d_f          = (last_feet_pos_f - pos_f) / (float)dt per component
 *   base_yaw     = rem(atan2f(..), T) of the root quaternion, the yaw formula above without the wrap (:717, :720)
 *   term[e]      = collision: the count of penalized bodies with |F_b| > (float)threshold (:629);
 *                  feet_slip: (s_0 * contact_0 + s_1 * contact_1) * gate, s_f = (d_f.x^2 + d_f.y^2) + d_f.z^2, gate = episode_steps[e] > 1
 *                  ? 1 : 0, 1 without episode_steps (:698-704); feet_vel_z: d_0.z^2 + d_1.z^2 (:707); feet_roll: roll_0^2 + roll_1^2
 *                  (:710); feet_yaw_diff: wrap(yaw_1 - yaw_0)^2 (:713); feet_yaw_mean: wrap(base_yaw - m)^2, m = (yaw_0 + yaw_1) / 2 +
 *                  (|yaw_1 - yaw_0| > P ? P : 0) (:716-717); feet_distance: min(max((float)feet_distance_ref - |cosf(base_yaw) * (pos_1.y -
 *                  pos_0.y) - sinf(base_yaw) * (pos_1.x - pos_0.x)|, 0), 0.1f), a NaN stays one (:721-725); feet_swing: (left and not
 *                  contact_0) + (right and not contact_1), left = |gait_process - 0.25f| < (float)(0.5 * swing_period) and gf > 1e-8f,
 *                  right with 0.75f (:728-730).  Without contact_forces collision is 0 and stays out of the total.
 *   total[e]     = sum of scale_k * term_k in rising k over the terms with scale_k != 0 whose input is there
 *   done[e]      = 8 if any termination body has |F_b| > (float)threshold, else 0 (:553; a NaN compares false): bit 3, so that the word
 *                  can be OR-ed with the bits 0 to 2 of gmr_proprio_out_t.done
 *   then last_feet_pos = feet_pos (:495).  Nothing is reset on an episode reset, as in the reference.  No clock moves, no draw is made.
 * Commands, curriculum, kicks and pushes act on the simulator and stay the caller's.  The tracker stays SINGLE-STREAM. */
#define GMR_FEET_TERMS 8
#define GMR_FEET_MAX_EDGES 8
#define GMR_FEET_MAX_BODIES 64
#define GMR_FEET_DONE_CONTACT 8
typedef struct {            /* the configuration of set_feet: HOST pointers and values */
  const float *edge_pos;              /* [num_edges][3] in the foot's frame (t1.py:536)                               */
  const int32_t *termination_body;    /* [num_termination] distinct, in [0, nb) (t1.py:553)                           */
  const int32_t *penalized_body;      /* [num_penalized] distinct, in [0, nb) (t1.py:629)                             */
  const float *scales;                /* [GMR_FEET_TERMS] the weights of the total                                    */
  int32_t feet_body[2];               /* left, right (t1.py:713-730 hard-codes two feet)                              */
  int32_t num_edges, nb, num_termination, num_penalized;
  double force_threshold, contact_clearance;   /* 1.0 (t1.py:553, :629) and 0.01 (:545) in the reference              */
  double feet_distance_ref, swing_period;
} gmr_feet_config_t;
typedef struct {            /* the inputs of a feet call beside the bodies: device pointers (gmr_motion_tracker_feet: host pointers) */
  const float *contact_forces;        /* [N][nb][3] or NULL: no collision term, done = 0                              */
  const float *root_states;           /* [N][13] position, xyzw quaternion, world linear and angular velocity         */
  const int32_t *episode_steps;       /* [N] or NULL: feet_slip is not gated                                          */
  const float *gait_frequency;        /* [N] or NULL: 0                                                               */
} gmr_feet_in_t;
typedef struct {            /* the outputs of a feet call, each an address or NULL */
  float *feet_pos;                    /* [N][2][3]                                                                    */
  float *feet_roll, *feet_yaw;        /* [N][2]                                                                       */
  int32_t *feet_contact;              /* [N][2]                                                                       */
  float *ground;                      /* [N] terrain height under the root                                            */
  float *gait;                        /* [N][2] the cos and sin columns of t1.py:585-586                              */
  float *term;                        /* [N][GMR_FEET_TERMS]                                                          */
  float *total;                       /* [N]                                                                          */
  int32_t *done;                      /* [N] 0 or GMR_FEET_DONE_CONTACT                                               */
} gmr_feet_out_t;
/* The terrain (terrain.py:30-45, :105-118): height_field int16 [nx][ny] on the HOST, copied to the device, or NULL for the plane (nx and
 * ny are then not looked at).  GMR_ERR_ARG: a scale that is not finite or not positive (horizontal_scale also as a float32), a negative
 * border, nx or ny below 2.  Synchronises the device: launches already in flight keep the field they were given. */
int gmr_motion_tracker_set_terrain(gmr_motion_tracker_t* t, const int16_t* height_field, int nx, int ny, double horizontal_scale,
                                   double vertical_scale, int border_pixels);
/* Terrain.terrain_heights (terrain.py:101-121; also what _reset_root_states needs, t1.py:331), ONE launch: point i is (points[i * stride],
 * points[i * stride + 1]), stride >= 2 in floats; heights f32[M].  _dev ADDS the number of points outside the field to *d_outside (one
 * int32 the caller has zeroed; may be NULL); the synchronous twin sets *outside (may be NULL) to the count of its call. */
int gmr_motion_tracker_terrain_heights_dev(gmr_motion_tracker_t* t, int64_t M, const float* d_points, int64_t stride, float* d_heights,
                                           int32_t* d_outside, void* stream);                      /* asynchronous */
int gmr_motion_tracker_terrain_heights(gmr_motion_tracker_t* t, int64_t M, const float* points, int64_t stride, float* heights,
                                       int32_t* outside);
/* The feet configuration (t1.py:529-549, :553, :627-629, :696-730): 1 <= num_edges <= GMR_FEET_MAX_EDGES finite edge points, feet_body and
 * the two lists (0 to GMR_FEET_MAX_BODIES entries each, distinct) in [0, nb), the four scalars finite in float32, scales finite.
 * Allocates last_feet_pos and gait_process and fills them with zeros; synchronises the device.  Launches in flight keep the configuration
 * they carry. */
int gmr_motion_tracker_set_feet(gmr_motion_tracker_t* t, const gmr_feet_config_t* cfg);
/* The step (t1.py:474-478, :495, :529-549, :553, :627-629, :696-730), ONE launch.  bodies: body_pos and body_rot of the simulator's rigid
 * bodies in the convention of gmr_tracker_links_sim_t -- body b of environment e at base[e * env_stride + b * body_stride], strides in
 * floats, or both 0 for two contiguous arrays [N][nb][3] and [N][nb][4]; body_vel and body_ang_vel are not read.  GMR_ERR_ARG, before a
 * device is touched, on a tracker whose feet were never set. */
int gmr_motion_tracker_feet_dev(gmr_motion_tracker_t* t, const gmr_tracker_links_sim_t* bodies, const gmr_feet_in_t* in,
                                const gmr_feet_out_t* out, void* stream);                           /* asynchronous */
int gmr_motion_tracker_feet(gmr_motion_tracker_t* t, const gmr_tracker_links_sim_t* bodies, const gmr_feet_in_t* in,
                            const gmr_feet_out_t* out);
/* the two state arrays on the host (last_feet_pos t1.py:495, gait_process :478), either may be NULL; synchronises */
int gmr_motion_tracker_feet_state(gmr_motion_tracker_t* t, float* last_feet_pos, float* gait_process);

/* ---- N12: tracker commands (velocity commands and their resampling, the command curriculum, kicks and pushes of a motion tracker,
 * DESIGN.md section 6s) ---- */
/* What booster_gym/envs/t1.py::step still left to the caller after N10 and N11: _resample_commands / _resample_curriculum_commands
 * (t1.py:362-389, :415-435), _update_curriculum (:391-413, a Python loop over the reset environments with one device read each), the
 * three command-tracking rewards and survival (:606-620), the command columns of the observation row (:584), _kick_robots and _push_robots
 * (:499-527) with the push columns of the privileged block (:598-599).  The statement of record is tests/commands_mirror.py; this is the
 * same in words.  Everything is float32 with one rounding per operation; a Python number is rounded to float32 where torch rounds it; the
 * span (upper - lower) of a uniform is formed in double and rounded once.
 * A. COMMANDS.  CONFIGURATION (a host struct that travels with every launch): gmr_commands_config_t.  STATE (device, owned by the tracker,
 * one block made by set_commands): commands f32[N][3], gait_frequency f32[N], cmd_resample_time i32[N], cmd_draws u32[N], all zero; with a
 * curriculum also env_level i32[N][2] (zero), curriculum_prob f32[2L+1][2A+1] (zero, the centre cell 1, t1.py:245-251; the first index is
 * the linear level), hits u32[G] and cum f64[G + 1] (zero), G = (2L+1)(2A+1).
 * THE CALL, for environment e (steps = episode_steps[e] after the caller's increment and before any reset; d = done && done[e] != 0;
 * f = lin_vel[e], g = ang_vel[e]: the filtered velocities gmr_proprio_out_t writes; c = commands[e] of the episode that is ending):
 *   1. term[e]  = (1, expf(-((c0 - f0) * (c0 - f0)) / (float)sigma), the same with c1, f1, the same with c2, g2) (:606-620); a term whose
 *                 velocity is absent is 0.  total[e] = sum of scale_k * term_k in rising k over the terms with scale_k != 0 whose input
 *                 is there.
 *   2. flags bit 0 (GMR_CMD_BOUNDARY) = steps == cmd_resample_time[e], before any reset: what the caller ORs into time_outs (:558).
 *   3. with a curriculum and d (:391-413): success = steps > min_success_steps && |f0 - c0| < (float)tol_x && |f1 - c1| < (float)tol_y &&
 *      |g2 - c2| < (float)tol_yaw; with x = env_level[e][0] + L, y = env_level[e][1] + A a success adds 1 to hits of the cells (x, y),
 *      (x -+ 1, y), (x, y -+ 1) that lie inside the grid (unsigned integer atomics: arrival order cannot matter).  flags bit 2
 *      (GMR_CMD_SUCCESS) = success.
 *   4. with d: cmd_resample_time[e] = 0 and steps = 0 from here on (:314).
 *   5. with a curriculum, once every environment has done 3: prob[g] = min(prob[g] + (float)rate * (float)hits[g], 1), hits[g] = 0.  THE
 *      REFERENCE adds rate once per success and clamps at the end: the two differ by float32 rounding unless the sums are exact (they are
 *      for a rate that is a power of two).  Then cum: lane k sums the GMR_CMD_CHUNK = 8 cells 8k .. 8k + 7 of the flattened grid in rising
 *      order in double, s_0 = 0, s_{i+1} = s_i + (double)prob[8k + i]; base_0 = 0, base_{k+1} = base_k + s_8 of chunk k, chained in rising
 *      k; cum[8k + i] = base_k + s_i and cum[G] = base + s of the last chunk's end.  cum is non-decreasing and a cell with prob = 0 has
 *      cum[g + 1] == cum[g] by construction.
 *   6. where steps == cmd_resample_time[e] (:362-389): (w0..w3) = philox4x32(counter (e, cmd_draws[e], 0, 2), key), (v0..v3) = the same
 *      with word 2 = 1; u_k = philox_unit(w_k), u4 = philox_unit(v0); cmd_draws[e] += 1.  Word 3 = 2 keeps these draws apart from the
 *      resets (0) and the sensor noise (1).
 *      without a curriculum: c_k = (float)(hi_k - lo_k) * u_k + (float)lo_k, k = 0, 1, 2 (isaacgym's torch_rand_float as restated here;
 *      not pinned to isaacgym, which no test machine has).
 *      with one: the cell is the largest g with cum[g] <= (double)v2 * 2^-32 * cum[G]; GMR_CMD_ORDER_REFERENCE splits it as the reference
 *      does (:417-418), lin = g % ny - L, ang = g / ny - A with ny = 2A + 1 -- the transpose of how _update_curriculum indexes the grid,
 *      kept as a mode and refused unless L == A --, GMR_CMD_ORDER_GRID is the consistent lin = g / ny - L, ang = g % ny - A;
 *      env_level[e] = (lin, ang); c0 = ((float)lin + (u0 + -0.5f)) * (float)res_x, c1 = ((float)|lin| * (2.0f * u1 + -1.0f)) *
 *      (float)res_y, c2 = ((float)ang + (u2 + -0.5f)) * (float)res_yaw (:425-435).
 *      gait_frequency[e] = (float)(hi - lo) * u3 + (float)lo.  u4 < (float)still_proportion zeroes the three commands and the gait
 *      frequency.  THE REFERENCE picks exactly int(p n) of the n resampling environments with randperm, a global selection; here every
 *      environment decides alone: the expected count is the same, the variance binomial.  cmd_resample_time[e] += lo + philox_below(v1,
 *      hi - lo) of resample_steps.  flags bit 1 (GMR_CMD_RESAMPLED).
 *   7. the outputs, each an address or NULL, written for every environment: commands, gait_frequency (what gmr_feet_in_t takes next
 *      step), flags, and cmd_obs[e * cmd_obs_stride + k] = commands[e][k] * obs_scale[k] (point it at obs + 6 with the row's width as
 *      stride: the row gmr_proprio_out_t.obs got earlier in the step then carries the commands after the resample, as :584 does).
 * Without a curriculum ONE launch, one lane per environment; with one THREE launches enqueued by the one call (1-4; one workgroup for 5;
 * 6-7), no host synchronisation between them.  No clock moves and no draw counter of the tracker moves.
 * B. KICKS AND PUSHES.  No device state.  The host decides from common_step what the step does -- kick: common_step % kick_every == 0;
 * push start: common_step % push_every == 0; push stop: common_step % push_every == push_duration and not a push start (the elif of
 * :517) -- and launches nothing on an idle step.  On a step that acts, ONE launch: element i (kick 0..5 = root_states[e][7 + i], push
 * 6..11 = force then torque) of environment e takes philox4x32(counter (e, common_step, i >> 1, 3), key), words (0, 1) for an even i,
 * (2, 3) for an odd one, and the recipe of N10 (uniform, gaussian, additive, scaling).  A kick replaces root_states[e][7:13] in place
 * (:502-503); an element whose block has no spec is left alone and costs no Philox call.  A push start applies the randomisation to zero
 * (:509-516; a block without a spec gives zero) and writes push_force[e * stride + k], push_torque likewise, and push_obs[e] = (force *
 * scale_force, torque * scale_torque) (:598-599); a push stop zeroes the same three.  THE REFERENCE reads the observation columns from
 * body 0 while it pushes base_indice; here push_obs is always the applied push.
 * The tracker stays SINGLE-STREAM. */
#define GMR_CMD_TERMS 4                /* survival, tracking_lin_vel_x, tracking_lin_vel_y, tracking_ang_vel */
#define GMR_CMD_MAX_LEVELS 20
#define GMR_CMD_CHUNK 8
#define GMR_CMD_BOUNDARY 1
#define GMR_CMD_RESAMPLED 2
#define GMR_CMD_SUCCESS 4
#define GMR_CMD_ORDER_GRID 0
#define GMR_CMD_ORDER_REFERENCE 1
#define GMR_DISTURB_KICK 1
#define GMR_DISTURB_PUSH_START 2
#define GMR_DISTURB_PUSH_STOP 4
typedef struct {            /* the configuration of set_commands: values */
  double lin_vel_x[2], lin_vel_y[2], ang_vel_yaw[2], gait_frequency[2];   /* (lower, upper) (t1.py:369-380)               */
  double still_proportion;            /* in [0, 1] (:381)                                                             */
  double tracking_sigma;              /* > 0 (:612)                                                                   */
  double update_rate;                 /* (:404), like everything below looked at with a curriculum only               */
  double toler[3];                    /* lin_vel_x_toler, lin_vel_y_toler, ang_vel_yaw_toler (:397-399)               */
  double resolution[3];               /* lin_vel_x_resolution, lin_vel_y_resolution, ang_vel_resolution (:427-435)    */
  float scales[GMR_CMD_TERMS];        /* the weights of the total                                                     */
  float obs_scale[3];                 /* lin_vel, lin_vel, ang_vel of the normalisation (:584)                        */
  int32_t resample_steps[2];          /* int(resampling_time_s / dt): hi > lo >= 1 (:385-386)                         */
  int32_t curriculum;                 /* 0 or 1                                                                       */
  int32_t lin_vel_levels, ang_vel_levels;   /* L, A in [0, GMR_CMD_MAX_LEVELS]                                        */
  int32_t min_success_steps;          /* floor(ceil(episode_length_s / dt) * (1 - episode_length_toler)) (:394-396)   */
  int32_t index_order;                /* GMR_CMD_ORDER_*                                                              */
} gmr_commands_config_t;
typedef struct {            /* the inputs of a commands call: device pointers (gmr_motion_tracker_commands: host pointers) */
  const int32_t *episode_steps;       /* [N]                                                                          */
  const int32_t *done;                /* [N] or NULL: nobody resets                                                   */
  const float *lin_vel, *ang_vel;     /* [N][3] the filtered velocities, or NULL (GMR_ERR_ARG with a curriculum)      */
} gmr_commands_in_t;
typedef struct {            /* the outputs of a commands call, each an address or NULL */
  float *term;                        /* [N][GMR_CMD_TERMS]                                                           */
  float *total;                       /* [N]                                                                          */
  float *commands;                    /* [N][3]                                                                       */
  float *gait_frequency;              /* [N]                                                                          */
  int32_t *flags;                     /* [N] GMR_CMD_BOUNDARY | GMR_CMD_RESAMPLED | GMR_CMD_SUCCESS                   */
  float *cmd_obs;                     /* row e at cmd_obs + e * cmd_obs_stride, three floats                          */
  int64_t cmd_obs_stride;             /* in floats, >= 3 when cmd_obs is given                                        */
} gmr_commands_out_t;
typedef struct {            /* the configuration of set_disturbances */
  gmr_proprio_noise_t kick_lin_vel, kick_ang_vel, push_force, push_torque;   /* (t1.py:502-503, :509-516)             */
  int32_t kick_every, push_every;     /* ceil(kick_interval_s / dt), ceil(push_interval_s / dt): >= 1 (:501, :508)    */
  int32_t push_duration;              /* ceil(push_duration_s / dt): >= 0 (:517)                                      */
  float scale_push_force, scale_push_torque;   /* (:598-599)                                                          */
} gmr_disturb_config_t;
typedef struct {            /* what a disturb call writes: device pointers (gmr_motion_tracker_disturb: host pointers) */
  float *root_states;                 /* [N][13], columns 7..12 replaced by a kick; needed on a kick step             */
  float *push_force, *push_torque;    /* row e at base + e * stride, three floats; each may be NULL                   */
  int64_t push_force_stride, push_torque_stride;   /* in floats, >= 3 where the address is given                     */
  float *push_obs;                    /* [N][6] or NULL                                                               */
} gmr_disturb_io_t;
/* The command configuration (t1.py:362-435, :606-620): every value finite (in float32 too), upper >= lower, still_proportion in [0, 1],
 * resample_steps hi > lo >= 1, tracking_sigma > 0 as a float32; with a curriculum L, A in [0, GMR_CMD_MAX_LEVELS], update_rate >= 0, the
 * tolerances and resolutions finite, min_success_steps >= 0, GMR_CMD_ORDER_REFERENCE only with L == A.  keep_state = 0 allocates the state
 * and gives it its initial values (synchronises the device); keep_state = 1 replaces the configuration alone and is GMR_ERR_ARG when
 * commands were never set or curriculum, L or A differ.  Launches in flight keep the configuration they carry. */
int gmr_motion_tracker_set_commands(gmr_motion_tracker_t* t, const gmr_commands_config_t* cfg, int keep_state);
/* The call (t1.py:362-435, :558, :584, :606-620): ONE launch, THREE with a curriculum */
int gmr_motion_tracker_commands_dev(gmr_motion_tracker_t* t, const gmr_commands_in_t* in, const gmr_commands_out_t* out,
                                    void* stream);                                                  /* asynchronous */
int gmr_motion_tracker_commands(gmr_motion_tracker_t* t, const gmr_commands_in_t* in, const gmr_commands_out_t* out);
/* the state arrays on the host (t1.py:240-251), each may be NULL; the last four are GMR_ERR_ARG to ask for without a curriculum;
 * synchronises.  mean and max of |env_level| (:421-424) are the caller's to form from env_level. */
int gmr_motion_tracker_command_state(gmr_motion_tracker_t* t, float* commands, float* gait_frequency, int32_t* cmd_resample_time,
                                     uint32_t* cmd_draws, int32_t* env_level, float* curriculum_prob, uint32_t* hits, double* cum);
/* The kicks and pushes (t1.py:499-527): each spec as in N10 (b >= 0 for a gaussian), kick_every and push_every >= 1, push_duration >= 0,
 * the two scales finite.  Touches no device. */
int gmr_motion_tracker_set_disturbances(gmr_motion_tracker_t* t, const gmr_disturb_config_t* cfg);
/* _kick_robots and _push_robots (t1.py:499-527, :598-599) at common_step, ONE launch or none.  Returns GMR_DISTURB_KICK |
 * GMR_DISTURB_PUSH_START | GMR_DISTURB_PUSH_STOP, what the step did (0: idle, nothing launched, nothing written), or a negative GMR_ERR_*;
 * with the kick bit the caller hands root_states back to the simulator. */
int gmr_motion_tracker_disturb_dev(gmr_motion_tracker_t* t, uint32_t common_step, const gmr_disturb_io_t* io, void* stream);   /* asynchronous */
int gmr_motion_tracker_disturb(gmr_motion_tracker_t* t, uint32_t common_step, const gmr_disturb_io_t* io);

/* ---- N13: tracker episode (reset states, the reward total and the episode statistics of a motion tracker) ---- */
/* What booster_gym/envs/t1.py::step still left to the caller after N12: _reset_dofs, _reset_root_states and the delay_steps draw
 * (t1.py:316-340), the sum over the blocks' weighted terms with its clip (t1.py:560-572), the two-group reward of
 * t1_imitation.py:323-352, the reset and time-out words (t1.py:556-558) and the per-episode sums of utils/recorder.py:36-53, a Python loop
 * with one device read per finished environment and reward term.  The statement of record is tests/episode_mirror.py; this is the same
 * in words.  Everything is float32 with one rounding per operation unless it says double; a Python number is rounded to float32 where
 * torch rounds it; the span (upper - lower) of a uniform is formed in double and rounded once.
 * A. RESET STATES.  CONFIGURATION: gmr_reset_config_t -- base_init_state, default_dof_pos f32[R], env_origins f32[N][2] or NULL, copied to
 * the device by the set_ call, three specs of the kind of N10, the yaw range, decimation, use_terrain.  STATE: reset_draws u32[N], zero.
 * THE CALL takes the masked list of N9's hold: entry i is environment env_ids[i] (i without env_ids, then n = N), served when mask is NULL
 * or mask[i] != 0; ids of served entries outside [0, N) are dropped and counted; every environment at most once in a list (the host twin
 * refuses a repeated id, the device call cannot look).  No nonzero, no compaction.  It writes the simulator's own arrays in place, rows
 * of served entries only -- root_states [N][13], dof_pos and dof_vel [N][R], optionally delay_steps and episode_steps i32[N] -- in the
 * reference's order (t1.py:319-340, :311, :316), n = reset_draws[e]:
 *   1. dof_pos[e][j] = randomise(default_dof_pos[j]) by init_dof_pos, dof_vel[e][j] = 0.
 *   2. the root row = base_init_state; x, y += env_origins[e]; x, y = randomise(x, y) by init_base_pos_xy.
 *   3. with use_terrain: z += the tracker's terrain height at (x, y), bit-equal to what terrain_heights returns there (N11); the plane adds
 *      (float)0.
 *   4. with a yaw range: yaw = (float)lo + (float)(hi - lo) * u, half = 0.5f * yaw, the quaternion (0, 0, sinf(half), cosf(half)):
 *      isaacgym's quat_from_euler_xyz at zero roll and pitch as restated here; not pinned to isaacgym, which no test machine has.  Without
 *      one the row's quaternion stays.
 *   5. vx, vy = randomise(0) by init_base_lin_vel_xy (0 without a spec); the other velocities are the row's.
 *   6. delay_steps[e] = philox_below(word, decimation) (decimation > 0 and the array given).
 *   7. episode_steps[e] = 0 (the array given).
 *   8. reset_draws[e] = n + 1.
 * init_root_states [n][13], init_dof_pos [n][R], init_dof_vel [n][R], each or NULL, are indexed by LIST POSITION and replace
 * base_init_state, default_dof_pos and the zero velocity of that entry (the rows step_links returns without advancing can be fed in:
 * reference-state initialisation); a given root row keeps its quaternion unless a yaw range is set, and its vx, vy take the place of the
 * zero of 5.
 * DRAWS: environment e has R + 6 elements -- dofs 0..R-1, x, y, yaw, vx, vy, delay; element i takes philox4x32(counter (e, n, i >> 1, 4),
 * key), words (0, 1) for an even i, (2, 3) for an odd one, and the recipe of N10 (uniform from the first word, gaussian from both,
 * additive, scaling); the yaw is philox_unit and the delay philox_below of the first word.  Word 3 = 4 is a counter domain of its own
 * next to 0 (clips), 1 (sensor noise), 2 (commands), 3 (kicks).  A block without a spec makes no Philox call.  THE REFERENCE draws ONE
 * dof-noise row per call for all reset environments (default_dof_pos is [1, R], t1.py:320); here every environment draws its own: a draw
 * depends on (seed, environment, its reset count, element) alone.
 * chain = 1: the same launch also does what hold (N9; held = the new dof_pos, torque_acc = 0) and proprio_reset (N10; filtered velocities
 * 0, last_root_vel = the new root_states[e][7:13]) would do afterwards (t1.py:309-313), each for the half that is configured.
 * ONE launch, 16 lanes per list entry: the lanes stride over the dofs, lane 0 does the root.
 * B. THE REWARD.  COLUMNS: the term rows of the blocks configured on the tracker when set_rewards is called, in the fixed order TERMS (6,
 * N4), LINK_TERMS (4, N5; with links attached), PROPRIO_TERMS (14, N10; with set_proprio), FEET_TERMS (8, N11; with set_feet), CMD_TERMS
 * (4, N12; with set_commands), then extra_cols <= GMR_REWARD_MAX_EXTRA columns of the caller's; C <= GMR_REWARD_MAX_COLS in all.
 * gmr_reward_config_t.blocks names the configured blocks and is GMR_ERR_ARG when the tracker disagrees; a call is GMR_ERR_ARG when a block
 * was configured or links were detached since.  WEIGHTS: the weight of a block's column is the one that block is configured with (the
 * weights of N4 and N5, the scales of N10 to N12), copied from the handle when the call is enqueued; a caller column takes
 * extra_weights.  groups[c] is GMR_REWARD_LOCOMOTION | GMR_REWARD_IMITATION, the groups column c feeds: one, both -- how the reference's
 * double count of the imitation terms (t1_imitation.py:323-352: they enter the clipped locomotion sum and then the imitation sum) is
 * expressed -- or none.
 * THE CALL, for environment e, the inputs as the blocks' calls left them (an array that is NULL keeps its columns out; the array of a
 * block that is not configured is never read):
 *   1. scaled[e][c] = w_c * term_c; a column with w_c == 0 or an absent array is +0 and out.
 *   2. S_g = the sum of scaled[e][c] over the columns of group g that are in, from +0 in rising c.
 *   3. with only_positive[g]: S_g < 0 ? 0 : S_g (a NaN stays, as torch.clip keeps it; t1.py:571-572).  group_total[e] = (S_0, S_1).
 *   4. reward[e] = group_weight[0] * S_0 + group_weight[1] * S_1, each product rounded, then the sum (t1_imitation.py:349-350).
 *   5. reset[e] = done[e] != 0 and time_outs[e] = ((done[e] & GMR_REWARD_DONE_TIME_OUT) | (flags[e] & GMR_CMD_BOUNDARY)) != 0
 *      (t1.py:556-558): done is the caller's OR of the done words of N10 and N11, flags the word of N12, both read as they lie; NULL is 0.
 * ONE launch, 16 lanes per environment, lane l holds the columns l, l + 16, ..; every lane of the sixteen gathers the row through the
 * group's permutes and adds it in the plain rising order of 2.  No clock, draw counter or state of another block is touched.
 * C. THE EPISODE STATISTICS (gmr_reward_config_t.stats = 1).  STATE (device, owned by the tracker, one block made by set_rewards, zero):
 * ep_steps i32[N], ep_sum f32[N][C + 1] (column 0 is the reward, column 1 + c is scaled column c), fin_count u32, fin_steps u64, fin_sum
 * f64[C + 1], a started flag.  PER REWARD CALL (recorder.py:36-53), in the same launch:
 *   6. ep_steps[e] += 1, except in the very first call after set_rewards: the reference starts from zeros there (:37-40), so its first
 *      episode counts one step fewer; kept.
 *   7. ep_sum[e][k] += value (a float32 add).
 *   8. where reset[e]: fin_count += 1 and fin_steps += ep_steps[e] (unsigned integer atomics), the row ep_sum[e] goes into fin_sum, then
 *      ep_steps[e] = 0 and ep_sum[e] = 0.
 * fin_sum does not depend on arrival order: workgroup w holds the environments 16 w .. 16 w + 15; its partial of column k is
 * p = +0, p = p + (double)ep_sum[e][k] over its reset environments in rising e; a SECOND small launch of one workgroup then chains
 * fin_sum[k] = fin_sum[k] + p_w over the workgroups that have a reset environment, in rising w.  No floating-point atomics.
 * READING OUT: reward_stats copies out[0] = fin_count (as u64), out[1] = fin_steps, out[2 + k] = fin_sum[k] as f64, and with clear = 1
 * zeroes the three, in one launch; ep_steps, ep_sum and the started flag stay.  The means are the caller's divisions.
 * The tracker stays SINGLE-STREAM. */
#define GMR_REWARD_MAX_EXTRA 16
#define GMR_REWARD_MAX_COLS 52
#define GMR_REWARD_BLOCK_TERMS 1
#define GMR_REWARD_BLOCK_LINKS 2
#define GMR_REWARD_BLOCK_PROPRIO 4
#define GMR_REWARD_BLOCK_FEET 8
#define GMR_REWARD_BLOCK_COMMANDS 16
#define GMR_REWARD_LOCOMOTION 1
#define GMR_REWARD_IMITATION 2
#define GMR_REWARD_DONE_TIME_OUT 4     /* bit 2 of gmr_proprio_out_t.done */
typedef struct {            /* the configuration of set_reset_states: values and two host addresses */
  float base_init_state[13];          /* pos, quat xyzw, lin vel, ang vel (t1.py:328)                                 */
  const float *default_dof_pos;       /* [R] (t1.py:320)                                                              */
  const float *env_origins;           /* [N][2] or NULL (t1.py:329)                                                   */
  gmr_proprio_noise_t init_dof_pos, init_base_pos_xy, init_base_lin_vel_xy;   /* (t1.py:320, :330, :337-340)          */
  double yaw_range[2];                /* (lower, upper), looked at with yaw = 1; the reference: (0, 2 pi) (t1.py:335) */
  int32_t yaw;                        /* 0 or 1: draw the yaw                                                         */
  int32_t decimation;                 /* in [0, GMR_CONTROL_MAX_DECIMATION]; 0: no delay draw (t1.py:316)             */
  int32_t use_terrain;                /* 0 or 1 (t1.py:331)                                                           */
} gmr_reset_config_t;
typedef struct {            /* the arrays of a reset_states call: device pointers (gmr_motion_tracker_reset_states: host pointers) */
  float *root_states;                 /* [N][13], rows of served entries written                                      */
  float *dof_pos, *dof_vel;           /* [N][R]                                                                       */
  int32_t *delay_steps;               /* [N] or NULL                                                                  */
  int32_t *episode_steps;             /* [N] or NULL                                                                  */
  const float *init_root_states;      /* [n][13] by list position, or NULL                                            */
  const float *init_dof_pos, *init_dof_vel;   /* [n][R] by list position, or NULL                                     */
} gmr_reset_io_t;
typedef struct {            /* the configuration of set_rewards: values */
  float group_weight[2];              /* locomotion_weight, imitation_weight (t1_imitation.py:349-350)                */
  float extra_weights[GMR_REWARD_MAX_EXTRA];   /* of the caller's columns                                            */
  int32_t only_positive[2];           /* 0 or 1 per group (t1.py:571)                                                 */
  int32_t blocks;                     /* GMR_REWARD_BLOCK_*: the blocks configured on the tracker                     */
  int32_t extra_cols;                 /* E in [0, GMR_REWARD_MAX_EXTRA]                                               */
  int32_t stats;                      /* 0 or 1: keep the episode statistics                                          */
  uint8_t groups[GMR_REWARD_MAX_COLS];   /* per column GMR_REWARD_LOCOMOTION | GMR_REWARD_IMITATION                  */
} gmr_reward_config_t;
typedef struct {            /* the inputs of a rewards call: device pointers (gmr_motion_tracker_rewards: host pointers), each or NULL */
  const float *term;                  /* [N][6]  gmr_tracker_out_t.term                                               */
  const float *link_term;             /* [N][4]  gmr_tracker_links_out_t.link_term                                    */
  const float *proprio_term;          /* [N][14] gmr_proprio_out_t.term                                               */
  const float *feet_term;             /* [N][8]  gmr_feet_out_t.term                                                  */
  const float *cmd_term;              /* [N][4]  gmr_commands_out_t.term                                              */
  const float *extra;                 /* [N][E]                                                                       */
  const int32_t *done;                /* [N] the OR of the done words; NULL: nobody resets                            */
  const int32_t *flags;               /* [N] gmr_commands_out_t.flags; NULL: no boundary                              */
} gmr_reward_in_t;
typedef struct {            /* the outputs of a rewards call, each an address or NULL */
  float *reward;                      /* [N]                                                                          */
  float *scaled;                      /* [N][C] what the reference puts into extras["rew_terms"] (t1.py:570)          */
  float *group_total;                 /* [N][2]                                                                       */
  int32_t *reset;                     /* [N] 0 or 1                                                                   */
  int32_t *time_outs;                 /* [N] 0 or 1                                                                   */
} gmr_reward_out_t;
/* The reset-state configuration (t1.py:316-340): every number finite (in float32 too), each spec as in N10 (b >= 0 for a gaussian),
 * upper >= lower, decimation in [0, GMR_CONTROL_MAX_DECIMATION].  Allocates reset_draws (zero) and the device copy of env_origins;
 * synchronises the device.  Launches in flight keep the configuration they carry. */
int gmr_motion_tracker_set_reset_states(gmr_motion_tracker_t* t, const gmr_reset_config_t* cfg);
/* _reset_dofs, _reset_root_states and the delay draw (t1.py:316-340), chained also t1.py:309-313: ONE launch */
int gmr_motion_tracker_reset_states_dev(gmr_motion_tracker_t* t, int n, const int32_t* d_env_ids, const int32_t* d_mask,
                                        const gmr_reset_io_t* io, int chain, void* stream);         /* asynchronous */
int gmr_motion_tracker_reset_states(gmr_motion_tracker_t* t, int n, const int32_t* env_ids, const int32_t* mask, const gmr_reset_io_t* io,
                                    int chain, int* ignored);
/* reset_draws u32[N] on the host (the count behind the draws of t1.py:316-340); synchronises */
int gmr_motion_tracker_reset_state(gmr_motion_tracker_t* t, uint32_t* reset_draws);
/* The reward configuration (t1.py:560-572, t1_imitation.py:323-352): the weights finite, extra_cols in [0, GMR_REWARD_MAX_EXTRA], the
 * flags 0 or 1, blocks what the tracker has configured, groups[c] <= 3 for c < C.  With stats = 1 allocates the state and zeroes it;
 * synchronises the device either way.  Launches in flight keep the configuration they carry. */
int gmr_motion_tracker_set_rewards(gmr_motion_tracker_t* t, const gmr_reward_config_t* cfg);
/* The call (t1.py:556-572, t1_imitation.py:323-352, recorder.py:36-53): ONE launch, TWO with the statistics */
int gmr_motion_tracker_rewards_dev(gmr_motion_tracker_t* t, const gmr_reward_in_t* in, const gmr_reward_out_t* out,
                                   void* stream);                                                   /* asynchronous */
int gmr_motion_tracker_rewards(gmr_motion_tracker_t* t, const gmr_reward_in_t* in, const gmr_reward_out_t* out);
/* The read-out of the statistics (recorder.py:55-62, what t1.py:556-558 hands the Recorder through the runner): out u64[C + 3] -- episodes,
 * steps, then C + 1 doubles -- or NULL; clear = 1 zeroes the accumulators in the same launch.  GMR_ERR_ARG without statistics. */
int gmr_motion_tracker_reward_stats_dev(gmr_motion_tracker_t* t, uint64_t* out, int clear, void* stream);   /* asynchronous */
int gmr_motion_tracker_reward_stats(gmr_motion_tracker_t* t, uint64_t* out, int clear);
/* the running sums of the open episodes on the host (recorder.py:36-53: episode_steps and episode_statistics), either may be NULL;
 * synchronises.  GMR_ERR_ARG without statistics. */
int gmr_motion_tracker_reward_state(gmr_motion_tracker_t* t, int32_t* ep_steps, float* ep_sum);

/* ---- N14: tracker rollout (rollout storage, GAE, returns and normalised advantages of a motion tracker) ---- */
/* What booster_gym/utils/runner.py still does with the outputs of a step after N13: the six indexed assignments into its ExperienceBuffer
 * per step (runner.py:107-108, :115-118, utils/buffer.py:15-16) and, per mini-epoch, the bootstrap of the timed-out rewards, discount_values
 * -- a Python loop over the horizon, utils/utils.py:33-44 --, the returns, the mean, the deviation and the normalisation
 * (runner.py:135-145).  The statement of record is tests/rollout_mirror.py; this is the same in words.
 * STORAGE: the caller's, as everywhere in the tracker; H = horizon, N environments, O, P, A columns: obs f32[H][N][O], priv f32[H][N][P]
 * (NULL when P = 0), actions f32[H][N][A], rewards f32[H][N], dones and time_outs u8[H][N].  The tracker owns the configuration and the
 * scratch of the partial sums alone.
 * RECORD, slot n in [0, H): slot n of each array receives the N rows handed in; done and time_outs are the int32 words N13 emits and
 * are stored as bytes, nonzero as 1.  An input that is NULL leaves its slot as it is -- obs before the step and the rest after it, as the
 * reference orders them, are two calls.  Nothing outside slot n is written.  ONE launch.
 * ADVANTAGES, from values f32[H][N] and last_values f32[N], float32 with one rounding per operation, e an environment, t a slot:
 *   1. where time_outs[t][e]: rewards[t][e] = values[t][e], written into the caller's array as the reference mutates its buffer
 *      (runner.py:135); a second call with other values overwrites it again.  (The launch stores every reward back, the others with the
 *      bits they had.)
 *   2. nn = 1 - (dones[t][e] | time_outs[t][e]) (runner.py:138, utils.py:37).
 *   3. g = (float)gamma, gl = (float)(gamma * lam), the product formed in double (what Python hands torch, utils.py:42-43).
 *   4. for t = H - 1 .. 0: nv = t == H - 1 ? last_values[e] : values[t + 1][e]; delta = (rewards[t][e] + (g * nn) * nv) - values[t][e];
 *      advantages[t][e] = last = delta + (gl * nn) * last, from last = +0 (utils.py:36-43).
 *   5. returns[t][e] = values[t][e] + advantages[t][e] (runner.py:144).
 *   6. with normalize: S1 = the sum of (double)adv and S2 = the sum of (double)adv * (double)adv (each product exact), both in this
 *      order: per environment from +0 in the scan's falling t; the environments of a group -- GMR_ROLLOUT_ENVS consecutive ones, an
 *      absent one counting +0 -- by the balanced tree x[i] = x[i] + x[i + s] for s = 1, 2, 4, .. (i a multiple of 2 s); the groups from
 *      +0 in rising order.  M = H N; mean = S1 / M; std = sqrt((S2 - S1 * S1 / M) / (M - 1)), torch's unbiased std, in double;
 *      normalized[t][e] = (adv - (float)mean) / ((float)std + 1e-8f) (runner.py:145).  M < 2 with normalize is GMR_ERR_ARG (the
 *      reference: NaN).  stats = (S1, S2, mean, std).  Without normalize, normalized and stats stay as they are.
 * Every output is an address or NULL.  NO OVERLAP: advantages, returns, normalized and stats must not overlap one another, values,
 * last_values, rewards, dones or time_outs -- rows are requested ahead of the stores, so an output laid over an input changes results
 * and nothing checks it; the slots of a record call must not overlap its inputs either.
 * One lane per environment walks t downward, sixteen rows requested ahead of the sixteen it works on.
 * No floating-point atomics.  TWO launches while there are at most GMR_ROLLOUT_FOLD groups -- every workgroup of the normalisation adds
 * the partials itself, in the same order --, THREE beyond (a chain of one workgroup between them); ONE without normalize.
 * The tracker stays SINGLE-STREAM; no call waits for the host. */
#define GMR_ROLLOUT_ENVS 64
#define GMR_ROLLOUT_FOLD 64
typedef struct {            /* the caller's rollout arrays: device pointers (the synchronous twins: host pointers) */
  float *obs;                         /* [H][N][O]                                                                    */
  float *priv;                        /* [H][N][P], NULL when P = 0                                                   */
  float *actions;                     /* [H][N][A]                                                                    */
  float *rewards;                     /* [H][N]                                                                       */
  uint8_t *dones, *time_outs;         /* [H][N] 0 or 1                                                                */
} gmr_rollout_io_t;
typedef struct {            /* the outputs of an advantages call, each an address or NULL */
  float *advantages;                  /* [H][N]                                                                       */
  float *returns;                     /* [H][N]                                                                       */
  float *normalized;                  /* [H][N], written with normalize                                               */
  double *stats;                      /* [4] S1, S2, mean, std, written with normalize                                */
} gmr_rollout_out_t;
/* The rollout configuration (runner.py:36-42, the horizon and the two discounts of runner.py:141-142): horizon >= 1, obs_cols >= 1,
 * act_cols >= 1, priv_cols >= 0, gamma and lam finite and in [0, 1].  Allocates the scratch of the partial sums; synchronises the device. */
int gmr_motion_tracker_set_rollout(gmr_motion_tracker_t* t, int horizon, int obs_cols, int priv_cols, int act_cols, double gamma, double lam);
/* The six assignments of a step (runner.py:107-108, :115-118): ONE launch.  n outside [0, H) is GMR_ERR_ARG. */
int gmr_motion_tracker_record_dev(gmr_motion_tracker_t* t, int n, const gmr_rollout_io_t* io, const float* d_obs, const float* d_priv,
                                  const float* d_actions, const float* d_reward, const int32_t* d_done, const int32_t* d_time_outs,
                                  void* stream);                                                    /* asynchronous */
int gmr_motion_tracker_record(gmr_motion_tracker_t* t, int n, const gmr_rollout_io_t* io, const float* obs, const float* priv,
                              const float* actions, const float* reward, const int32_t* done, const int32_t* time_outs);
/* The bootstrap, discount_values, the returns and the normalisation of a mini-epoch (runner.py:135-145, utils.py:33-44): at most THREE
 * launches.  io names rewards, dones and time_outs; normalize is 0 or 1. */
int gmr_motion_tracker_advantages_dev(gmr_motion_tracker_t* t, const gmr_rollout_io_t* io, const float* d_values, const float* d_last_values,
                                      const gmr_rollout_out_t* out, int normalize, void* stream);  /* asynchronous */
int gmr_motion_tracker_advantages(gmr_motion_tracker_t* t, const gmr_rollout_io_t* io, const float* values, const float* last_values,
                                  const gmr_rollout_out_t* out, int normalize);

/* ---- N15: tracker loss (the PPO loss head of a motion tracker, its gradients and the KL step) ---- */
/* What booster_gym/utils/runner.py still does between the outputs of its two networks and its optimiser after N14: old_actions_log_prob
 * (runner.py:123-125), the value, surrogate, bound and entropy terms and their sum (runner.py:146-161, utils/utils.py:47-52), the backward
 * pass of that sum down to loc, logstd and values (what runner.py:163 delivers at the outputs of the networks), the KL between the old
 * and the new policy (runner.py:168-174) and the learning-rate rule (runner.py:175-178).  The statement of record is tests/ppo_mirror.py;
 * this is the same in words.  M = H N rows and A = act_cols columns, both from gmr_motion_tracker_set_rollout.
 * Float32 with one rounding per operation, the sums over rows float64.  Per column a: scale = expf(logstd[a]), var = scale * scale,
 * log_scale = logf(scale) (the reference takes the log of the exp) -- these exp and log, and the log of the KL, with ONE rounding: formed
 * in double and rounded once --; C = (float)log(sqrt(2 pi)), E0 = (float)(0.5 + 0.5 log(2 pi)),
 * lo = (float)(1 - e_clip), hi = (float)(1 + e_clip).
 * LOG_PROB: d = actions - loc; per element ((-(d * d)) / (2 * var) - log_scale) - C; the row value lp is the sum over rising a from the
 * first element.
 * LOSS, per row: ratio = expf(lp - old_log_prob); s = (-adv) * ratio; sc = (-adv) * min(max(ratio, lo), hi); surr = max(s, sc); the weight
 * w is what torch's backward of max and clamp amounts to: 1 where lo <= ratio <= hi (sc is s bit for bit there: a tie with both halves
 * alive); outside, 1 where s > sc, 0.5 where s == sc, 0 where s < sc; glp = (w * s) / (float)M.
 *   grad_values = (2 * (values - returns)) / (float)M
 *   grad_loc    = glp * (d / var) + cb * (2 * max(loc - 1, 0) + 2 * min(loc + 1, 0)), cb = (float)(bound_coef / (M A))
 *   grad_logstd[a] = (float)(S_a + entropy_coef), S_a the sum over the rows of (double)glp * (double)((d * d) / var - 1)
 *   terms = value_loss = sum((values - returns)^2) / M, actor_loss = sum(surr) / M, bound_loss = sum(max(loc - 1, 0)^2) / (M A) +
 *           sum(min(loc + 1, 0)^2) / (M A) (the squares float32, added within a row from +0 over rising a), entropy = the sum from +0 over
 *           rising a of (double)(E0 + log_scale[a]), loss = ((value_loss + actor_loss) + bound_coef * bound_loss) + entropy_coef * entropy,
 *           kl_mean (0 without the old policy), the learning rate after this call, clip_fraction = the share of rows with w = 0
 *   KL, per element (logf(scale / old_scale) + (0.5 * (old_var + (loc - old_loc)^2)) / var) - 0.5, the row value the float32 sum over
 *           rising a from the first element, kl_mean = sum / M
 *   LEARNING RATE, with update_lr, in double: kl_mean > 2 desired_kl: lr = max(lr_min, lr / lr_factor); else kl_mean < desired_kl / 2:
 *           lr = min(lr_max, lr * lr_factor).  The comparison is made in double; the reference compares a float32 kl_mean, so the two can
 *           differ only when kl_mean lies within float32 rounding of a threshold.  The rate stays on the device for the next call.
 * EVERY SUM OVER ROWS is float64 in one association, a function of M alone (ppo_mirror.sums): the rows of a group -- GMR_LOSS_ROWS
 * consecutive ones, an absent one counting +0 -- by the balanced tree x[i] = x[i] + x[i + s] for s = 1, 2, 4, .. (i a multiple of 2 s);
 * the groups of a block -- GMR_LOSS_FOLD consecutive ones, an absent one counting +0 -- by the same tree; the blocks from +0 in rising
 * order.  No floating-point atomics.  Inputs are taken as finite.
 * NO OVERLAP: no output may overlap another one or an input; nothing checks it.
 * ONE launch for the log-probability; at most TWO for the loss (the fold writes grad_logstd and terms and steps the rate; there is no
 * third).  Everything is enqueued on the caller's stream; no call waits for the host.  The tracker stays SINGLE-STREAM. */
#define GMR_LOSS_ROWS 64
#define GMR_LOSS_FOLD 64
#define GMR_LOSS_MAX_ACT 32
typedef struct {            /* the inputs of a loss call: device pointers (the synchronous twin: host pointers) */
  const float *loc;                   /* [M][A] the actor's output                                                    */
  const float *logstd;                /* [A]                                                                          */
  const float *actions;               /* [M][A] the rollout array                                                     */
  const float *old_log_prob;          /* [M]                                                                          */
  const float *values;                /* [M] the critic's output                                                      */
  const float *returns;               /* [M]                                                                          */
  const float *advantages;            /* [M] the normalised ones                                                      */
  const float *old_loc;               /* [M][A], or NULL together with old_logstd: no KL                              */
  const float *old_logstd;            /* [A]                                                                          */
} gmr_loss_in_t;
typedef struct {            /* the outputs of a loss call, each an address or NULL */
  float *grad_loc;                    /* [M][A]                                                                       */
  float *grad_logstd;                 /* [A]                                                                          */
  float *grad_values;                 /* [M]                                                                          */
  float *log_prob;                    /* [M]                                                                          */
  double *terms;                      /* [8] value_loss, actor_loss, bound_loss, entropy, loss, kl_mean, lr, clip_fraction */
} gmr_loss_out_t;
/* The coefficients of runner.py:156-161, the clip of utils.py:47, the rule of runner.py:175-178 and its starting rate: bound_coef and
 * entropy_coef finite, desired_kl and learning_rate finite and above 0, e_clip in (0, 1), 0 < lr_min <= lr_max, lr_factor >= 1.  Needs
 * gmr_motion_tracker_set_rollout first (and again after the rollout is set again); act_cols above GMR_LOSS_MAX_ACT is GMR_ERR_ARG.
 * Allocates the partial sums and the learning rate, one double on the device; synchronises the device. */
int gmr_motion_tracker_set_loss(gmr_motion_tracker_t* t, double bound_coef, double entropy_coef, double desired_kl, double learning_rate,
                                double e_clip, double lr_min, double lr_max, double lr_factor);
/* out f64[8]: bound_coef, entropy_coef, desired_kl, the learning rate as the last update_lr of runner.py:175-178 left it, e_clip, lr_min,
 * lr_max, lr_factor; synchronises the device. */
int gmr_motion_tracker_loss_state(gmr_motion_tracker_t* t, double* out);
/* old_actions_log_prob (runner.py:123-125): out f32[M].  ONE launch. */
int gmr_motion_tracker_log_prob_dev(gmr_motion_tracker_t* t, const float* d_loc, const float* d_logstd, const float* d_actions, float* d_out,
                                    void* stream);                                                  /* asynchronous */
int gmr_motion_tracker_log_prob(gmr_motion_tracker_t* t, const float* loc, const float* logstd, const float* actions, float* out);
/* The loss head (runner.py:146-180 without the networks and the optimiser): at most TWO launches.  update_lr is 0 or 1; 1 without
 * old_loc and old_logstd is GMR_ERR_ARG. */
int gmr_motion_tracker_loss_dev(gmr_motion_tracker_t* t, const gmr_loss_in_t* in, const gmr_loss_out_t* out, int update_lr,
                                void* stream);                                                      /* asynchronous */
int gmr_motion_tracker_loss(gmr_motion_tracker_t* t, const gmr_loss_in_t* in, const gmr_loss_out_t* out, int update_lr);

/* ---- N16: tracker optimiser (the clip of the gradient norm and the Adam step of a motion tracker) ---- */
/* What booster_gym/utils/runner.py does with the gradients of a mini-epoch: clip_grad_norm_(model.parameters(), 1.0) and optimizer.step()
 * (runner.py:164-165) of the torch.optim.Adam of runner.py:33 -- torch's defaults: no weight decay, no amsgrad, not maximising --, at the
 * learning rate the rule of runner.py:175-180 left in the param groups.  The statement of record is tests/optim_mirror.py; this is the
 * same in words.  K tensors of fixed sizes n_k, float32; one rounding per operation.
 * CLIP: ss_k = the sum over tensor k of (double)g * (double)g (the products are exact), float64 in ONE association that is a function of
 * the sizes alone: the elements go in chunks of GMR_OPT_CHUNK, a chunk never spans two tensors (the last chunk of a tensor is short);
 * within a chunk the balanced tree x[i] = x[i] + x[i + s] for s = 1, 2, 4, .. over the element index (i a multiple of 2 s), an absent
 * element counting +0; the chunks are added from +0 in rising order, tensor after tensor.  No floating-point atomics.
 * total_norm = sqrt(total) in double; coef = (float)min(1, max_norm / (total_norm + 1e-6)); the clipped gradient is gc = g * coef.
 * torch adds float32 norms of the tensors instead: the difference is measured by the fixture, not reproduced.
 * ADAM, per element, in the operator order of torch's single-tensor path (torch/optim/adam.py: lerp_, mul_ / addcmul_,
 * sqrt / bias_correction2_sqrt + eps, addcdiv_), t the step count after this step:
 *   m = m + w1 * (gc - m)                        w1 = (float)(1 - beta1)
 *   v = v * b2;  v = v + (c2 * gc) * gc          b2 = (float)beta2, c2 = (float)(1 - beta2)
 *   den = sqrtf(v) / bc2s + e                    bc2s = (float)sqrt(1 - beta2^t), e = (float)eps
 *   p = p + (ns * m) / den                       ns = (float)(-(lr / (1 - beta1^t)))
 * The scalars are formed in double and rounded once; beta^t is the product of t factors beta from 1, in double (kept on the device from
 * step to step, so that no pow of any library decides a bit).
 * A tensor whose gradient pointer is NULL is skipped in the norm and in the update, like p.grad is None: its parameters and its state
 * stay bit for bit.  THE GRADIENTS ARE READ-ONLY: the clipped gradient is never stored -- clip_grad_norm_ scales in place, and nothing
 * in runner.py reads the gradients after the step.  Inputs are taken as finite; a non-finite gradient makes the norm and with it every
 * parameter non-finite, as in the reference.
 * LEARNING RATE: the optimiser keeps its own double on the device.  A step uses it; then, in FOLLOW mode (learning_rate NaN at
 * gmr_motion_tracker_set_optimizer), the fold of that step copies the loss block's current rate (N15) into it, for the next step.  THE
 * CONTRACT is the order of INTEGRATION.md: in every mini-epoch gmr_motion_tracker_loss_dev with update_lr is enqueued BEFORE the step, so
 * the step of mini-epoch n runs at the rate the rule left at the end of mini-epoch n - 1, which is the reference's order
 * (runner.py:165 before :175-180).  With a finite learning_rate the rate is fixed and the loss block is not looked at.
 * AT MOST THREE launches per step -- the norm pass (a workgroup per chunk, one double each), the fold (one workgroup: the total, the step
 * count, coef and the Adam scalars, info, the rate for the next step), the update pass (a workgroup per chunk) --, all on the caller's
 * stream; no call waits for the host.  The K parameter and K gradient addresses travel by value in the kernel arguments: no copy is
 * enqueued for them.  The tracker stays SINGLE-STREAM. */
#define GMR_OPT_CHUNK 1024
#define GMR_OPT_MAX_TENSORS 32
/* The optimiser of runner.py:33: K tensors of sizes[k] >= 1 elements, K in 1 .. GMR_OPT_MAX_TENSORS; learning_rate finite and above 0,
 * or NaN: follow the loss block, which needs gmr_motion_tracker_set_loss first; beta1, beta2 in [0, 1), eps and max_norm finite and
 * above 0.  Allocates exp_avg and exp_avg_sq (every tensor on 256 bytes of one block each), zeroes them, sets the step count to 0 and
 * builds the chunk table on the device; synchronises the device. */
int gmr_motion_tracker_set_optimizer(gmr_motion_tracker_t* t, int K, const int64_t* sizes, double learning_rate, double beta1, double beta2,
                                     double eps, double max_norm);
/* clip_grad_norm_ and optimizer.step (runner.py:164-165): params and grads are HOST arrays of K device addresses (a NULL gradient: the
 * tensor is skipped); info f64[4] on the device, or NULL: total_norm, coef, the rate used, the step count.  At most THREE launches. */
int gmr_motion_tracker_optimizer_step_dev(gmr_motion_tracker_t* t, float* const* d_params, const float* const* d_grads, double* d_info,
                                          void* stream);                                            /* asynchronous */
int gmr_motion_tracker_optimizer_step(gmr_motion_tracker_t* t, float* const* params, const float* const* grads, double* info);
/* The state of the Adam of runner.py:33 as its state_dict holds it (runner.py:95, :207-214): the step count and exp_avg, exp_avg_sq as
 * flat host arrays of sum(sizes) floats in tensor order; synchronises the device. */
int gmr_motion_tracker_optimizer_state(gmr_motion_tracker_t* t, int64_t* step, float* exp_avg, float* exp_avg_sq);
/* Continues a checkpoint (runner.py:95): step >= 0 and the two flat arrays; in follow mode the rate of the next step is the loss block's
 * current one; synchronises the device. */
int gmr_motion_tracker_optimizer_load_state(gmr_motion_tracker_t* t, int64_t step, const float* exp_avg, const float* exp_avg_sq);

/* ---- N17: tracker policy (the forward pass of the actor and of the critic of a motion tracker) ---- */
/* What booster_gym/utils/model.py computes without autograd: model.act(obs).loc and .sample() (model.py:29-32, runner.py:109-111 and :123-124,
 * the whole of Runner.play, :225-226), and model.est_value(obs, privileged_obs) (model.py:34-36, runner.py:133).  The statement of record is
 * tests/policy_mirror.py; this is the same in words.
 * A NETWORK is an MLP in -> h_1 -> .. -> h_L -> out, 1 <= L <= GMR_POLICY_MAX_HIDDEN: y = x W^T + b with W [out][in] row-major float32,
 * the layout of torch.nn.Linear; ELU (alpha 1) after every hidden layer, none after the last.  Per output element, in float32:
 *   z = b_j + sum_k x_k W_jk,   elu(z) = z > 0 ? z : expm1f(z).
 * THE SUM is a chain of fused multiply-adds from +0, one rounding per term, the bias added last; its order over k is a function of the
 * layer's shape alone: a hidden layer takes the k in blocks of eight, within a block 0, 4, 1, 5, 2, 6, 3, 7 (the two halves of a
 * wavefront hold four consecutive k each and the matrix instruction takes one of either per step); the last layer takes them in rising
 * order.  No floating-point atomics.  A row's result depends on nothing but that row: not on rows, not on the tile the row falls in,
 * not on the optional outputs asked for, not on the alignment of a tensor.
 * CAPACITIES: hidden widths are multiples of GMR_POLICY_WIDTH_STEP in GMR_POLICY_WIDTH_STEP .. GMR_POLICY_MAX_WIDTH; obs_cols >= 1,
 * priv_cols >= 0, obs_cols + priv_cols <= GMR_POLICY_MAX_IN; act_cols in 1 .. GMR_LOSS_MAX_ACT; the critic's output width is 1.
 * Anything else is GMR_ERR_ARG.
 * THE PARAMETERS travel by address in the kernel arguments with every call, as the optimiser's do (N16): params is a HOST array of
 * device addresses in the order of model.parameters() -- logstd [act_cols], the critic's (W, b) pairs, the actor's (W, b) pairs: the
 * very list gmr_motion_tracker_optimizer_step_dev takes.  Nothing is copied or cached: a step of the optimiser between two calls is
 * seen by the next one.  Any 4-byte-aligned address is taken; a weight tensor on 16 bytes whose rows are a multiple of 16 bytes is read
 * 16 bytes at a time, with the same bits.
 * THE ACTOR reads obs [rows][obs_cols] and writes loc [rows][act_cols].  With sample != 0 it also writes
 *   actions[e][i] = loc[e][i] + exp(logstd[i]) * r(e, i),
 * r the Gaussian draw of the tracker's noise (N10): Box-Muller on the two Philox words of element i of environment e at its count,
 * counter domain 5 (the sampled actions), keyed by the tracker's seed.  The policy block keeps one uint32 count per environment;
 * sampling needs rows == N (row e is environment e) and advances every count by one.  Without sample, actions is not written, no
 * count is touched and any rows >= 1 is taken.
 * THE CRITIC reads its input from TWO arrays, obs [rows][obs_cols] and priv [rows][priv_cols] (model.py:35, concatenated in LDS; priv
 * may be NULL when priv_cols is 0), and writes values [rows].
 * hidden, when given, is a HOST array of L addresses, each NULL or [rows][h_l]: the activations after the ELU of hidden layer l.
 * ONE launch per call: a workgroup owns GMR_POLICY_TILE rows, whose activations stay in LDS from the first layer to the last; rows
 * beyond `rows` in the last tile are neither read nor written.  Everything is enqueued on the caller's stream; no call waits for the
 * host.  NO OVERLAP: no output may overlap another one, an input or a parameter; nothing checks it.  The tracker stays SINGLE-STREAM. */
#define GMR_POLICY_TILE 32
#define GMR_POLICY_MAX_HIDDEN 4
#define GMR_POLICY_WIDTH_STEP 32
#define GMR_POLICY_MAX_WIDTH 256
#define GMR_POLICY_MAX_IN 512
#define GMR_POLICY_MAX_TENSORS 21
/* The two networks of model.py:9-27: n_*_hidden widths each.  Allocates the counts, zero; a second call replaces the block and zeroes
 * the counts again; synchronises the device. */
int gmr_motion_tracker_set_policy(gmr_motion_tracker_t* t, int obs_cols, int priv_cols, int act_cols, int n_actor_hidden, const int* actor_hidden,
                                  int n_critic_hidden, const int* critic_hidden);
/* model.act(obs) (model.py:29-32): loc, and with sample the action of runner.py:111.  ONE launch. */
int gmr_motion_tracker_act_dev(gmr_motion_tracker_t* t, const float* const* d_params, int64_t rows, const float* d_obs, float* d_loc, float* d_actions,
                               float* const* d_hidden, int sample, void* stream);                   /* asynchronous */
int gmr_motion_tracker_act(gmr_motion_tracker_t* t, const float* const* params, int64_t rows, const float* obs, float* loc, float* actions,
                           float* const* hidden, int sample);
/* model.est_value(obs, privileged_obs) (model.py:34-36).  ONE launch. */
int gmr_motion_tracker_values_dev(gmr_motion_tracker_t* t, const float* const* d_params, int64_t rows, const float* d_obs, const float* d_priv,
                                  float* d_values, float* const* d_hidden, void* stream);           /* asynchronous */
int gmr_motion_tracker_values(gmr_motion_tracker_t* t, const float* const* params, int64_t rows, const float* obs, const float* priv, float* values,
                              float* const* hidden);
/* The shapes of model.py:9-27 as given -- shape i32[16]: obs_cols, priv_cols, act_cols, the actor's L and four widths (0 beyond L),
 * the critic's L and four widths, GMR_POLICY_TILE, 0, 0 -- and counts u32[N] (or NULL); synchronises the device. */
int gmr_motion_tracker_policy_state(gmr_motion_tracker_t* t, int32_t* shape, uint32_t* counts);

/* ---- N18: tracker policy backward (loss.backward() through the actor and the critic of a motion tracker) ---- */
/* What torch.autograd computes behind runner.py:163 through the two ELU MLPs of booster_gym/utils/model.py:9-27, from the gradients at
 * the networks' outputs (grad_loc [rows][act_cols] and grad_values [rows] of N15) to one gradient per weight and bias, in the layout of
 * the parameter list of N17.  The statement of record is tests/policy_bwd_mirror.py; this is the same in words, in the notation of N17:
 * layer l = 0 .. L maps width[l] -> width[l + 1], hidden[l] is the activation after layer l's ELU, a_0 the input row (the critic's: obs
 * and priv side by side, never concatenated in memory), a_l = hidden[l - 1].  Given g_L = grad_loc or grad_values, in float32:
 *   for l = L .. 1:   dA[m][i] = sum_j g_l[m][j] W_l[j][i],    g_{l-1}[m][i] = dA[m][i] * d(hidden[l-1][m][i]),   d(y) = y > 0 ? 1 : y + 1
 *   for every l:      dW_l[j][i] = sum_m g_l[m][j] a_l[m][i],  db_l[j] = sum_m g_l[m][j];      dA_0 is not formed.
 * d IS ELU'S DERIVATIVE FROM ITS OUTPUT: the forward stores y = expm1f(z), and exp(z) = y + 1 up to one rounding (torch takes exp of the
 * saved input).
 * THE SUM OVER j (the sweep) is a chain of fused multiply-adds from +0, one rounding per term: the last layer's A or one outputs in rising
 * order, a hidden layer's in blocks of eight, within a block 0, 4, 1, 5, 2, 6, 3, 7, as N17's.  A delta row depends on that row alone.
 * THE SUMS OVER ROWS: rows are cut into chunks of GMR_POLICY_BWD_CHUNK; inside a chunk the sum is ONE float32 chain of fused multiply-adds
 * from +0 over the rows in rising order (db: the chain of fma(g, 1, .)); across chunks the partial sums are added in double, in rising
 * chunk order, and rounded to float32 once.  The association is a function of rows and of the shape alone.  No floating-point atomics.
 * grads is a HOST array of device addresses in the order of params.  The entries of the network's own tensors are OVERWRITTEN, not
 * accumulated into (no zero_grad); grads[0] (logstd, whose gradient N15 writes) and the other network's entries are not looked at.
 * hidden is the forward's list, needed in full; delta is a HOST array of L addresses [rows][width[l + 1]], needed in full: it receives
 * g_0 .. g_{L-1} and is read back by the weight-gradient launch.  Rows at and beyond `rows` of any array are neither read nor written.
 * THREE launches per call on the caller's stream -- the sweep (a workgroup per GMR_POLICY_TILE rows, g_l in LDS, v_mfma_f32_32x32x2_f32),
 * the weight gradients (a wavefront per 64 x 64 block of one dW and one chunk, through the tile table) and the fold --, no wait for the
 * host.  NO OVERLAP between an output and anything else; the tracker stays SINGLE-STREAM: both calls share one workspace. */
#ifndef GMR_POLICY_BWD_CHUNK               /* (a diagnostic build of csrc/gmr_tracker_policy_bwd.hip alone may set another: tools/tracker_backward_probe.py) */
#define GMR_POLICY_BWD_CHUNK 256
#endif
/* 131072 rows are 512 chunks; the widest networks (512 inputs, four layers of 256, 32 outputs) have 512*256 + 3*256*256 + 32*256 + 4*256
 * + 32 = 336 928 weights and biases, so the workspace stays at 512 * 336 928 * 4 = 690 028 544 bytes, below 1 GB */
#define GMR_POLICY_BWD_MAX_ROWS 131072
/* Needs set_policy first; allocates the workspace for any rows in 1 .. max_rows and builds the tile tables; a set_policy with other
 * shapes afterwards makes every backward call GMR_ERR_ARG until set_backward runs again; synchronises the device. */
int gmr_motion_tracker_set_backward(gmr_motion_tracker_t* t, int64_t max_rows);
/* the actor: grads[actor's pairs] from grad_loc */
int gmr_motion_tracker_act_backward_dev(gmr_motion_tracker_t* t, const float* const* d_params, float* const* d_grads, int64_t rows, const float* d_obs,
                                        const float* const* d_hidden, const float* d_grad_loc, float* const* d_delta, void* stream);   /* asynchronous */
int gmr_motion_tracker_act_backward(gmr_motion_tracker_t* t, const float* const* params, float* const* grads, int64_t rows, const float* obs,
                                    const float* const* hidden, const float* grad_loc, float* const* delta);
/* the critic: grads[critic's pairs] from grad_values */
int gmr_motion_tracker_values_backward_dev(gmr_motion_tracker_t* t, const float* const* d_params, float* const* d_grads, int64_t rows, const float* d_obs,
                                           const float* d_priv, const float* const* d_hidden, const float* d_grad_values, float* const* d_delta,
                                           void* stream);                                                                                /* asynchronous */
int gmr_motion_tracker_values_backward(gmr_motion_tracker_t* t, const float* const* params, float* const* grads, int64_t rows, const float* obs,
                                       const float* priv, const float* const* hidden, const float* grad_values, float* const* delta);
/* state i64[6]: GMR_POLICY_BWD_CHUNK, the chunks of max_rows, the bytes of the workspace block, max_rows, the tiles of the actor's table,
 * of the critic's. */
int gmr_motion_tracker_backward_state(gmr_motion_tracker_t* t, int64_t* state);

/* ---- multi-GPU: one rank per GPU, ONE broadcast, no per-step collective ------------ */
/* The reference parallelises over files with mp.Pool on one CPU (scripts/smplx_to_robot_dataset.py:241-242); here
 * streams shard over the ranks of one node and the only data that crosses ranks is the packed robot model + task set.
 * RCCL is opened at run time (dlopen of librccl.so; GMR_RCCL_LIBRARY overrides); no PyTorch involved. */
typedef struct gmr_comm gmr_comm_t;
/* The ranks form a control star over TCP at master_addr:port (the launcher's MASTER_ADDR and a port derived from
 * MASTER_PORT); rank 0's ncclUniqueId travels over it and every step of the RCCL bring-up is agreed on by ALL ranks,
 * so a failure on one rank is the same error (GMR_ERR_COMM, gmr_last_error names the rank and the reason) on every
 * rank -- never a hang in a half-formed communicator.  Call after gmr_set_device(local_rank).
 * Environment: GMR_COMM_BACKEND=tcp -- the star alone carries the (job-level, host-buffer) operations below: the CPU
 * rehearsal of the N > 1 path; GMR_COMM_FALLBACK=tcp -- a job whose RCCL bring-up fails continues on the star, decided
 * collectively, and gmr_comm_backend() says so; GMR_COMM_TIMEOUT (s, default 120) bounds the rendezvous. */
int gmr_comm_create(int rank, int world, const char* master_addr, int port, gmr_comm_t** out);
/* "rccl-<version>", "tcp" or "tcp (fallback: <why RCCL could not be brought up>)"; valid until gmr_comm_destroy */
const char* gmr_comm_backend(const gmr_comm_t* comm);
int gmr_comm_destroy(gmr_comm_t* comm);
int gmr_comm_rank(const gmr_comm_t* comm);
int gmr_comm_world(const gmr_comm_t* comm);
/* `gmr_broadcast_model` of SURVEY.md section 8(b): `bytes` host bytes (gmr_model_t + gmr_taskset_t, 24 KB) of rank
 * `root` into the same buffer on every rank (H2D, ncclBroadcast over xGMI, D2H, synchronised). */
int gmr_comm_broadcast(gmr_comm_t* comm, void* buf, size_t bytes, int root);
int gmr_comm_broadcast_dev(gmr_comm_t* comm, void* d_buf, size_t bytes, int root, void* stream);
/* job-level plumbing of the drivers (not in the data path): device-synchronising barrier, timing reductions */
int gmr_comm_barrier(gmr_comm_t* comm);
int gmr_comm_allreduce_max(gmr_comm_t* comm, double* inout, int n);
int gmr_comm_allreduce_sum(gmr_comm_t* comm, double* inout, int n);
int gmr_comm_allgather(gmr_comm_t* comm, const double* in, double* out /* [world][n] */, int n);
/* the bootstrap alone (plain TCP, no GPU): rank 0 hands `bytes` bytes to every peer */
int gmr_bootstrap_exchange(int rank, int world, const char* addr, int port, void* payload, size_t bytes, double timeout_s);

#ifdef __cplusplus
}
#endif
#endif /* GMR_HIP_H */
