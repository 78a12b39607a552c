// gmr_handles.h -- the handles of the C-ABI that more than one translation unit of libgmrhip.so looks into (not part of the
// C-ABI): the FK tree (gmr_fk_handle.h: created in gmr_fk.hip) and the motion library (gmr_motion.hip), both read by gmr_body_state.hip, and
// the motion tracker (gmr_tracker.hip), which is bound to a library and, with links attached (gmr_tracker_links.hip), to an FK tree;
// gmr_tracker_preview.hip reads its state and tables, gmr_tracker_adaptive.hip owns its bins (adaptive sampling, masked resets),
// gmr_tracker_anchor.hip its anchors, gmr_tracker_control.hip its control tables and the two arrays of the actuator model,
// gmr_tracker_proprio.hip its proprioception tables and the six arrays behind them, gmr_tracker_feet.hip its terrain, its feet tables and
// the two arrays behind them, gmr_tracker_commands.hip its command and disturbance tables and the arrays of the velocity commands,
// gmr_tracker_episode.hip its reset-state and reward tables, the reset counters and the arrays of the episode statistics,
// gmr_tracker_rollout.hip its rollout configuration and the partial sums of an advantages call, gmr_tracker_loss.hip its loss configuration,
// the partial sums of a loss call and the learning rate, gmr_tracker_optim.hip its optimiser configuration, the Adam state, the chunk table
// and the scalars of a step, gmr_tracker_policy.hip the shapes of its two networks and the counts of the sampled actions.  What those
// translation units share beyond the structs lives beside them: gmr_tracker_host.h (host: the
// checks of a noise spec and of a list of environments, grid sizes, the ignored-id count, the allocation and the read-back of a block's
// state; also the noise spec itself, ProprioNoise) and gmr_tracker_dev.h (device: draws, noise, heading, small vectors, group reductions).
#pragma once
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/gmr_hip.h"
#include "gmr_fk_handle.h"    // struct gmr_fk
#include "gmr_fk_tree.h"
#include "gmr_internal.h"
#include "gmr_link_plan.h"
#include "gmr_tracker_host.h"
#include "gmr_tracker_policy_plan.h"
#include "gmr_tracker_policy_bwd_plan.h"
#include "gmr_workspace.h"

namespace gmr {
// the arrays of a motion library as its kernels see them (device pointers into the library's one block)
struct MotionArrays {
  int C, B, ndof, nbody;
  const int32_t* seg_start;   // [C + 1], validated on the host when the library was created
  const double* fps;          // [C]
  float *root_pos, *root_rot, *dof_pos, *local_body_pos, *root_vel, *root_ang_vel, *dof_vel, *stats;
};
}  // namespace gmr

struct gmr_motion_lib {
  gmr::MotionArrays A;
  gmr::DeviceBlock block;        // every array of the library: one allocation
  size_t off[GMR_MOTION_FPS + 1], bytes[GMR_MOTION_FPS + 1];
  int filled = 0;                // 1 once a fill has been enqueued
  int has_body = 0;              // the fill was given local_body_pos
  int reference_angvel = 0;      // the fill was asked for GMR_MOTION_ANGVEL_REFERENCE: root_ang_vel is not a physical angular velocity
};

namespace gmr {
constexpr int TRACKER_MAX_DOF = 64;   // robot dofs of a tracker
constexpr int TRACKER_TERMS = 6;      // root pos, root rot, root vel, root ang vel, dof pos, dof vel
// what every workgroup of a step reads alike; travels as a kernel argument, so replacing it never touches a launch in flight
struct TrackerTables {
  int32_t R;                          // robot dofs
  int8_t map[TRACKER_MAX_DOF];        // robot dof j <- column map[j] of the library, -1: dof_default[j] / velocity 0
  float dof_default[TRACKER_MAX_DOF], dof_weight[TRACKER_MAX_DOF];
  float scale[TRACKER_TERMS], weight[TRACKER_TERMS];
};
// What a draw from the bins of adaptive sampling reads.  The step kernels reach it through ONE pointer of TrackerState, so that a plain
// step carries eight more bytes of kernel arguments than before and nothing else; the adaptive kernels take it by value.
struct AdaptiveBins {
  int32_t nbins;                 // Bt
  const double* cdf;             // [Bt] cdf[b] = p[0] + .. + p[b-1], written by tracker_adapt_cdf_kernel
  const int32_t* start;          // [C + 1] first bin of every clip
  const int32_t* clip;           // [Bt] the clip of a bin
  const int32_t* frames;         // [C] F_c, frames per bin (at most max(T_c, 1))
};
// the tracker's own device memory (one block)
struct TrackerState {
  int32_t* clip;       // [N]
  float *time, *length;   // [N] the clock and (float)(T / fps) of the assigned clip (0 for a clip id outside [0, C))
  uint32_t* draws;     // [N] Philox draws made for the environment so far
  uint32_t* ignored;   // [1] environment ids outside [0, N) met by reset / assign since creation
  const double* cdf;   // [C] with clip weights: cdf[k] = (w_0 + .. + w_{k-1}) / sum, else null
  const AdaptiveBins* bins;   // adaptive sampling: the table a draw from the bins reads, ON THE DEVICE; null on a plain tracker
  float* anchor_pos;   // [N][3] tracker anchors: the translation of every environment; null until they are enabled
  float* anchor_yaw;   // [N][2] (z, w) of the unit quaternion (0, 0, z, w) of its yaw; null exactly when anchor_pos is
};
constexpr int ADAPT_MAX_K = 16;       // look-ahead of adaptive sampling, in bins
constexpr int ADAPT_CHUNK = 64;       // bins one lane sums in order (tracker_adapt_cdf_kernel)
constexpr int ADAPT_TILE = 4096;      // bins per workgroup of tracker_adapt_score_kernel: one partial sum each
constexpr int ADAPT_MAX_BINS = 1 << 22;
// the parameters of an Adapt; travel as a kernel argument like TrackerTables, so replacing them never touches a launch in flight
struct AdaptivePlan {
  int32_t Bt = 0;                // bins; 0: adaptive sampling is off
  int32_t K = 1;                 // look-ahead, 1 .. ADAPT_MAX_K
  double alpha = 0.0, uniform = 1.0;
  double g[ADAPT_MAX_K] = {};    // g[u] = gamma^u by repeated multiplication
};
// what only the adaptive kernels touch (device pointers into the tracker's adaptive block)
struct AdaptiveArrays {
  const double* base;            // [Bt] Wn_c frames(b) / T_c
  uint32_t* fail_now;            // [Bt] failures recorded since the last Adapt
  double *ema, *prob;            // [Bt]
  double* cdf;                   // [Bt] (AdaptiveBins::cdf, writable)
  double *part, *tot;            // [ceil(Bt / ADAPT_TILE)], [ceil(Bt / ADAPT_CHUNK)] scratch of an Adapt
};
constexpr int PREVIEW_MAX_OFFSETS = 16;   // clock offsets of a preview
constexpr int PREVIEW_MAX_BODIES = 32;    // library bodies of its body block
// the preview of a tracker: validated on the host, travels as a kernel argument like TrackerTables
struct PreviewPlan {
  int32_t K = 0;                            // offsets; 0: no preview configured
  int32_t blocks = 0, frame = 0, nsel = 0;  // GMR_PREVIEW_* block bits, GMR_PREVIEW_FRAME_*, bodies of the body block
  float offset[PREVIEW_MAX_OFFSETS] = {};   // seconds, finite
  int16_t body[PREVIEW_MAX_BODIES] = {};    // rows of the library's local_body_pos, distinct
};
// the control configuration of a tracker: validated on the host, travels as a kernel argument like TrackerTables
struct ControlTables {
  int32_t R = 0;                            // the robot dofs it was set for; 0: control was never set
  int32_t M = 0;                            // decimation: physics substeps per environment step, 1 .. CONTROL_MAX_DECIMATION
  float action_scale = 0.0f, clip = 0.0f;   // k, c (c may be inf)
  float startup = 0.0f, gain_startup = 0.0f, gain_run = 0.0f;   // D seconds, g0, g1
  float default_pos[TRACKER_MAX_DOF] = {};  // the robot's default pose, where the start-up easing begins (NOT TrackerTables::dof_default)
};
constexpr int CONTROL_MAX_DECIMATION = 64;
constexpr int PROPRIO_TERMS = 14;         // lin_vel_z .. base_height, the order of include/gmr_hip.h N10
constexpr int PROPRIO_MAX_EXTRA = 16;     // pass-through columns of the observation row
constexpr int PROPRIO_NOISE_BLOCKS = 6;   // gravity, ang_vel, dof_pos, dof_vel, lin_vel, height
// (one noise spec as the kernels apply it, ProprioNoise: gmr_tracker_host.h)
// the proprioception configuration of a tracker: validated on the host, travels as a kernel argument like TrackerTables
struct ProprioTables {
  int32_t R = 0;                            // the robot dofs it was set for; 0: proprio was never set
  int32_t C = 0;                            // pass-through columns, 0 .. PROPRIO_MAX_EXTRA
  int32_t max_steps = 0;                    // the time-out: episode_steps > max_steps
  int32_t any_noise = 0;                    // some spec is not GMR_NOISE_NONE
  float fw = 0.0f, fw1 = 0.0f;              // (float)filter_weight, (float)(1.0 - filter_weight)
  float s_g = 0.0f, s_v = 0.0f, s_w = 0.0f, s_q = 0.0f, s_qd = 0.0f;      // the normalisation scales
  float height_target = 0.0f, term_vel = 0.0f, term_height = 0.0f;
  ProprioNoise noise[PROPRIO_NOISE_BLOCKS];
  float scale[PROPRIO_TERMS] = {};          // the weights of the total; zero: the term stays out
  float default_pos[TRACKER_MAX_DOF] = {};  // (a table of its own: not ControlTables::default_pos)
  float lower[TRACKER_MAX_DOF] = {}, upper[TRACKER_MAX_DOF] = {};      // the soft position limits, formed on the host in the order of t1.py:665-670
  float vel_soft[TRACKER_MAX_DOF] = {};     // dof_vel_limits * (float)soft_dof_vel_limit
  float tq_lim[TRACKER_MAX_DOF] = {}, tq_soft[TRACKER_MAX_DOF] = {};   // torque_limits and torque_limits * (float)soft_torque_limit
};
// the proprioception state of a tracker (device pointers into its proprio block; zero after set_proprio)
struct ProprioState {
  float *filtered_lin_vel = nullptr, *filtered_ang_vel = nullptr;      // [N][3]
  float* last_root_vel = nullptr;                                      // [N][6]
  float *last_actions = nullptr, *last_dof_vel = nullptr;              // [N][R]
  uint32_t* noise_tick = nullptr;                                      // [N] launches that applied noise to the environment
};
constexpr int FEET_TERMS = 8;             // collision, feet_slip .. feet_swing, the order of include/gmr_hip.h N11
constexpr int FEET_MAX_EDGES = 8;         // edge points of one foot
constexpr int FEET_MAX_BODIES = 64;       // entries of the termination / penalised body lists
// the terrain of a tracker: travels as a kernel argument; field = null is the plane of height 0
struct TerrainTables {
  const int16_t* field = nullptr;           // [nx][ny] on the device, the first index is x (terrain.py:113)
  int32_t nx = 0, ny = 0;
  float border = 0.0f, hs = 1.0f;           // (float)border_pixels, (float)horizontal_scale
  double vs = 1.0;                          // vertical_scale
};
// the feet configuration of a tracker: validated on the host, travels as a kernel argument like ControlTables
struct FeetTables {
  int32_t E = 0;                            // edge points per foot, 1 .. FEET_MAX_EDGES; 0: feet were never set
  int32_t nb = 0;                           // bodies of the contact-force tensor
  int32_t feet_body[2] = {};                // left, right
  int32_t n_term = 0, n_pen = 0;
  float threshold = 0.0f, clearance = 0.0f; // (float)force_threshold, (float)contact_clearance
  float distance_ref = 0.0f;                // (float)feet_distance_ref
  float half_swing = 0.0f;                  // (float)(0.5 * swing_period)
  float scale[FEET_TERMS] = {};             // the weights of the total; zero: the term stays out
  float edge[FEET_MAX_EDGES * 3] = {};      // edge_pos [E][3] in the foot's frame
  int32_t term_body[FEET_MAX_BODIES] = {}, pen_body[FEET_MAX_BODIES] = {};
};
// the feet state of a tracker (device pointers into its feet block; zero after set_feet)
struct FeetState {
  float* last_feet_pos = nullptr;           // [N][2][3]
  float* gait_process = nullptr;            // [N]
};
constexpr int CMD_TERMS = 4;              // survival, tracking_lin_vel_x, tracking_lin_vel_y, tracking_ang_vel, the order of include/gmr_hip.h N12
constexpr int CMD_MAX_LEVELS = 20;        // curriculum levels per axis: a grid of at most 41 x 41 cells
constexpr int CMD_CHUNK = 8;              // grid cells one lane sums in order (tracker_commands_grid_kernel)
// the command configuration of a tracker: validated on the host, travels as a kernel argument like ControlTables
struct CommandTables {
  int32_t on = 0;                           // 0: commands were never set
  int32_t curriculum = 0, L = 0, A = 0;     // the grid is [2 L + 1][2 A + 1], the first index is the linear level
  int32_t G = 0;                            // its cells
  int32_t order = 0;                        // GMR_CMD_ORDER_GRID / _REFERENCE
  int32_t min_success = 0;                  // success needs episode_steps > min_success
  int32_t rs_lo = 1, rs_span = 1;           // cmd_resample_time grows by rs_lo + a draw below rs_span
  float lo[4] = {}, span[4] = {};           // lin_vel_x, lin_vel_y, ang_vel_yaw, gait_frequency: (float)lower, (float)(upper - lower), the span formed in double
  float still = 0.0f, sigma = 1.0f;         // (float)still_proportion, (float)tracking_sigma
  float scale[CMD_TERMS] = {};              // the weights of the total; zero: the term stays out
  float obs_scale[3] = {};
  float rate = 0.0f, tol[3] = {}, res[3] = {};
};
// the command state of a tracker (device pointers into its command block; see include/gmr_hip.h N12 for the initial values)
struct CommandState {
  float* commands = nullptr;                // [N][3]
  float* gait_frequency = nullptr;          // [N]
  int32_t* resample_time = nullptr;         // [N]
  uint32_t* draws = nullptr;                // [N]
  int32_t* carry = nullptr;                 // [N] the flag bits the first launch of a curriculum call hands to its third
  int32_t* level = nullptr;                 // [N][2], curriculum only, like the three below
  float* prob = nullptr;                    // [G]
  uint32_t* hits = nullptr;                 // [G]
  double* cum = nullptr;                    // [G + 1]
};
// the kicks and pushes of a tracker: travel as a kernel argument; no device state
struct DisturbTables {
  int32_t on = 0;                           // 0: disturbances were never set
  int32_t kick_every = 1, push_every = 1, push_duration = 0;
  ProprioNoise spec[4];                     // kick_lin_vel, kick_ang_vel, push_force, push_torque
  float s_force = 1.0f, s_torque = 1.0f;    // the two privileged-observation scales
};
constexpr int RESET_SPECS = 3;            // init_dof_pos, init_base_pos_xy, init_base_lin_vel_xy
// the reset-state configuration of a tracker: validated on the host, travels as a kernel argument like ControlTables
struct ResetTables {
  int32_t R = 0;                            // the robot dofs it was set for; 0: reset states were never set
  int32_t yaw = 0;                          // the yaw is drawn
  int32_t decimation = 0;                   // delay_steps is drawn below it; 0: no draw
  int32_t use_terrain = 0;
  float yaw_lo = 0.0f, yaw_span = 0.0f;     // (float)lo, (float)(hi - lo), the span formed in double
  const float* origins = nullptr;           // [N][2] on the device, or null
  ProprioNoise spec[RESET_SPECS];
  float base[13] = {};                      // base_init_state
  float default_pos[TRACKER_MAX_DOF] = {};  // (a table of its own, like ControlTables::default_pos)
};
constexpr int REWARD_BLOCKS = 5;          // TERMS, LINK_TERMS, PROPRIO_TERMS, FEET_TERMS, CMD_TERMS: the column order of include/gmr_hip.h N13
constexpr int REWARD_MAX_EXTRA = 16;      // caller columns behind them
constexpr int REWARD_MAX_COLS = 52;       // 6 + 4 + 14 + 8 + 4 + 16
// the reward configuration of a tracker: validated on the host, travels as a kernel argument like ControlTables.  The
// handle keeps the weights of the caller's columns alone: those of the blocks' columns are copied from the blocks' tables into the copy
// a call carries, when an entry point enqueues it.
struct RewardTables {
  int32_t on = 0;                           // 0: rewards were never set
  int32_t mask = 0;                         // GMR_REWARD_BLOCK_*: the blocks the columns were laid out for
  int32_t C = 0, E = 0;                     // columns, the caller's among them
  int32_t stats = 0;                        // the episode statistics are kept
  int32_t pos[2] = {};                      // only_positive of the two groups
  float gw[2] = {};                         // group_weight
  float w[REWARD_MAX_COLS] = {};            // the weight of a column; zero: the column stays out
  uint8_t group[REWARD_MAX_COLS] = {};      // GMR_REWARD_LOCOMOTION | GMR_REWARD_IMITATION
  uint8_t block[REWARD_MAX_COLS] = {}, off[REWARD_MAX_COLS] = {};      // column c is term off[c] of input array block[c] (REWARD_BLOCKS: extra)
  int32_t width[REWARD_BLOCKS + 1] = {};    // the row length of every input array
};
// the episode statistics of a tracker (device pointers into its reward block, all zero after set_rewards; null without statistics)
struct RewardState {
  int32_t* ep_steps = nullptr;              // [N]
  float* ep_sum = nullptr;                  // [N][C + 1], column 0 is the reward
  uint32_t* fin_count = nullptr;            // [1] episodes finished since the last clear
  unsigned long long* fin_steps = nullptr;  // [1] their steps
  double* fin_sum = nullptr;                // [C + 1] their sums
  uint32_t* started = nullptr;              // [1] a reward call has been made
  double* part = nullptr;                   // [ceil(N / 16)][C + 1] the partials of one call
  uint32_t* wg_any = nullptr;               // [ceil(N / 16)] the workgroup finished an episode in this call
};
// the rollout configuration of a tracker and its scratch: device pointers into the rollout block
struct RolloutTables {
  int32_t H = 0;                            // the horizon; 0: the rollout was never set
  int32_t O = 0, P = 0, A = 0;              // columns of obs, priv and actions
  double gamma = 0.0, lam = 0.0;            // as given
  float g = 0.0f, gl = 0.0f;                // (float)gamma, (float)(gamma * lam)
  double* part = nullptr;                   // [ceil(N / GMR_ROLLOUT_ENVS)][2] the partial sums of one call
  double* sums = nullptr;                   // [4] S1, S2, mean, std of one call beyond GMR_ROLLOUT_FOLD groups
};
// the loss configuration of a tracker and its scratch: device pointers into the loss block
struct LossTables {
  int32_t on = 0;                           // 0: the loss was never set
  int32_t A = 0;                            // columns, the rollout's act_cols when the loss was set
  int64_t M = 0;                            // rows, the rollout's H * N when the loss was set
  double bound_coef = 0.0, entropy_coef = 0.0, desired_kl = 0.0, e_clip = 0.0, lr_min = 0.0, lr_max = 0.0, lr_factor = 0.0;   // as given
  double* part = nullptr;                   // [A + 6][ceil(M / GMR_LOSS_ROWS)] the partial sums of one call
  double* lr = nullptr;                     // [1] the learning rate
};
// one chunk of the optimiser's passes: GMR_OPT_CHUNK consecutive elements of one tensor, fewer at the tensor's end
struct OptimChunk {
  int64_t first;                            // the first element, inside its tensor
  int64_t state;                            // the same element inside exp_avg / exp_avg_sq (floats from the block's start)
  int32_t tensor, count;
};
// the optimiser of a tracker: the configuration as given and device pointers into the optimiser block
struct OptimTables {
  int32_t K = 0;                            // tensors; 0: the optimiser was never set
  int32_t follow = 0;                       // the rate follows the loss block
  int64_t chunks = 0, total = 0;            // chunks and elements of all tensors
  int64_t size[GMR_OPT_MAX_TENSORS] = {};   // elements per tensor
  int64_t off[GMR_OPT_MAX_TENSORS] = {};    // where a tensor's state starts in exp_avg / exp_avg_sq, in floats: on 256 bytes
  int64_t state_floats = 0;                 // the length of exp_avg and of exp_avg_sq with the padding
  double beta1 = 0.0, beta2 = 0.0, eps = 0.0, max_norm = 0.0;      // as given
  const OptimChunk* table = nullptr;        // [chunks]
  float *exp_avg = nullptr, *exp_avg_sq = nullptr;      // [state_floats]
  double* part = nullptr;                   // [chunks] the partial sums of one step
  double* state = nullptr;                  // [4] the rate of the next step, the step count, beta1^t, beta2^t
  float* scal = nullptr;                    // [4] coef, bc2s, ns of the step in flight
};
// the two networks of a tracker: their shapes as given and the device pointer into the policy block
struct PolicyTables {
  int32_t on = 0;                           // 0: the policy was never set
  int32_t obs_cols = 0, priv_cols = 0, act_cols = 0;
  PolicyShape actor, critic;
  uint32_t* counts = nullptr;               // [N] the actions sampled for the environment so far
};
// the backward pass through them: the plan, the shapes it was made for and the device pointers into its block
struct PolicyBwdTables {
  int32_t on = 0;                           // 0: set_backward never ran
  PolicyBwdPlan plan;
  PolicyShape actor, critic;                // as the policy stood at set_backward: a set_policy with other shapes invalidates the plan
  int32_t obs_cols = 0, priv_cols = 0;
  float* part = nullptr;                    // [chunks][elems of the larger network]
  const PolicyBwdTile *tab_actor = nullptr, *tab_critic = nullptr;
};
}  // namespace gmr

struct gmr_motion_tracker {
  const gmr_motion_lib* lib;     // not owned: the library outlives its trackers
  int N, loop;
  float dtf;                     // (float)dt: the clock is float32
  uint32_t key[2];               // the seed, low word first
  gmr::TrackerTables tab;
  gmr::LinkPlan links;           // links.nsel = 0 until gmr_motion_tracker_set_links attaches a selection
  const gmr_fk* fk = nullptr;    // not owned: the tree of the attached links outlives the tracker
  gmr::PreviewPlan preview;      // preview.K = 0 until gmr_motion_tracker_set_preview configures one
  gmr::TrackerState S;
  gmr::DeviceBlock block;
  gmr::AdaptivePlan adaptive;    // adaptive.Bt = 0 until gmr_motion_tracker_set_adaptive configures the bins
  gmr::AdaptiveBins bin_tab = {}; // the host's copy of *S.bins
  gmr::AdaptiveArrays bins = {};
  gmr::DeviceBlock bin_block;    // every array of adaptive sampling: one allocation, made by set_adaptive
  double bin_seconds = 0.0;      // what the bins were built with
  gmr::DeviceBlock anchor_block; // S.anchor_pos / S.anchor_yaw: one allocation, made by gmr_motion_tracker_enable_anchors
  gmr::ControlTables control;    // control.R = 0 until gmr_motion_tracker_set_control configures it
  float* held = nullptr;         // [N][R] the targets the actuators hold (the reference's last_dof_targets); null until control is set
  float* torque_acc = nullptr;   // [N][R] the running sum of the torques of an environment step
  gmr::DeviceBlock control_block; // held and torque_acc: one allocation, made by gmr_motion_tracker_set_control
  gmr::ProprioTables proprio;    // proprio.R = 0 until gmr_motion_tracker_set_proprio configures it
  gmr::ProprioState proprio_state;
  gmr::DeviceBlock proprio_block; // the six arrays of proprio_state: one allocation, made by gmr_motion_tracker_set_proprio
  gmr::TerrainTables terrain;    // the plane until gmr_motion_tracker_set_terrain uploads a field
  gmr::DeviceBlock terrain_block; // the int16 field
  gmr::FeetTables feet;          // feet.E = 0 until gmr_motion_tracker_set_feet configures them
  gmr::FeetState feet_state;
  gmr::DeviceBlock feet_block;   // last_feet_pos and gait_process: one allocation, made by gmr_motion_tracker_set_feet
  gmr::CommandTables commands;   // commands.on = 0 until gmr_motion_tracker_set_commands configures them
  gmr::CommandState command_state;
  gmr::DeviceBlock command_block; // the arrays of command_state: one allocation, made by gmr_motion_tracker_set_commands
  gmr::DisturbTables disturb;    // disturb.on = 0 until gmr_motion_tracker_set_disturbances configures them
  gmr::ResetTables resets;       // resets.R = 0 until gmr_motion_tracker_set_reset_states configures them
  uint32_t* reset_draws = nullptr; // [N] resets drawn for the environment so far
  gmr::DeviceBlock reset_block;  // reset_draws and the copy of env_origins: one allocation, made by gmr_motion_tracker_set_reset_states
  gmr::RewardTables rewards;     // rewards.on = 0 until gmr_motion_tracker_set_rewards configures them
  gmr::RewardState reward_state;
  gmr::DeviceBlock reward_block; // the arrays of reward_state: one allocation, made by gmr_motion_tracker_set_rewards with statistics
  gmr::RolloutTables rollout;    // rollout.H = 0 until gmr_motion_tracker_set_rollout configures it
  gmr::DeviceBlock rollout_block; // the partial sums of an advantages call: one allocation, made by gmr_motion_tracker_set_rollout
  gmr::LossTables loss;          // loss.on = 0 until gmr_motion_tracker_set_loss configures it
  gmr::DeviceBlock loss_block;   // the partial sums of a loss call and the learning rate: one allocation, made by gmr_motion_tracker_set_loss
  gmr::OptimTables optim;        // optim.K = 0 until gmr_motion_tracker_set_optimizer configures it
  gmr::DeviceBlock optim_block;  // the Adam state, the chunk table, the partial sums and the scalars of a step: one allocation, made by gmr_motion_tracker_set_optimizer
  gmr::PolicyTables policy;      // policy.on = 0 until gmr_motion_tracker_set_policy configures it
  gmr::DeviceBlock policy_block; // the per-environment counts of the sampled actions: one allocation, made by gmr_motion_tracker_set_policy
  gmr::PolicyBwdTables bwd;      // bwd.on = 0 until gmr_motion_tracker_set_backward configures it
  gmr::DeviceBlock bwd_block;    // the partial sums of dW and db per row chunk and the tile tables: one allocation, made by gmr_motion_tracker_set_backward
  std::vector<double> clip_w;    // the clip weights as given at creation (empty: uniform)
  std::mutex mu;                 // the tables, and the whole of every synchronous entry point
};

namespace gmr {
// the simulator state and the outputs of a step (n environments, r robot dofs) as a synchronous step or link step stages them:
// h holds the caller's host pointers, d gets the device pointers
inline void stage_tracker_sim(HostStage& st, gmr_tracker_sim_t& d, const gmr_tracker_sim_t& h, size_t n, size_t r) {
  st.in(d.base_pos, h.base_pos, n * 12); st.in(d.base_quat, h.base_quat, n * 16); st.in(d.base_lin_vel, h.base_lin_vel, n * 12);
  st.in(d.base_ang_vel, h.base_ang_vel, n * 12); st.in(d.dof_pos, h.dof_pos, n * r * 4); st.in(d.dof_vel, h.dof_vel, n * r * 4);
}
inline void stage_tracker_out(HostStage& st, gmr_tracker_out_t& d, const gmr_tracker_out_t& h, size_t n, size_t r) {
  st.out(d.ref_root_pos, h.ref_root_pos, n * 12); st.out(d.ref_root_rot, h.ref_root_rot, n * 16); st.out(d.ref_root_vel, h.ref_root_vel, n * 12);
  st.out(d.ref_root_ang_vel, h.ref_root_ang_vel, n * 12); st.out(d.ref_dof_pos, h.ref_dof_pos, n * r * 4);
  st.out(d.ref_dof_vel, h.ref_dof_vel, n * r * 4); st.out(d.err, h.err, n * 24); st.out(d.term, h.term, n * 24); st.out(d.total, h.total, n * 4);
  st.out(d.status, h.status, n * 4); st.out(d.finished, h.finished, n * 4);
}
}  // namespace gmr
