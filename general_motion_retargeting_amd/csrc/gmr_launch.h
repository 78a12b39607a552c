// gmr_launch.h -- the launchers the host entry points of libgmrhip.so call, declared ONCE (not part of the C-ABI).  Every file
// that defines one of them and every file that calls one includes this header: the symbols are extern "C", so the linker would
// join a definition and a prototype that disagree without a word, and only the compiler, seeing both, can refuse.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gmr {
struct IkLayout;
struct IkParams;
struct WideLayout;
struct FkTree;
struct PostSources;
}  // namespace gmr

// one job of a throughput-shape launch as the host side hands it over (device pointers)
struct gmr_wide_job_desc {
  const char* d_image; const gmr::WideLayout* L; const gmr::IkParams* P;
  int S, T;
  const double* d_q0; const double* d_human; const int32_t* d_len;
  double* d_q_out; int32_t* d_nsolve; int32_t* d_status; double* d_tgt_out; double* d_err_out;
  const double* d_scale;         // [S][nhum] or null
  int fwin;                      // the image's frame windows are not all +inf
  const double* d_weight;        // [S][T][nhum] per-frame body weights, or null
};

extern "C" {
// gmr_ik.hip
hipError_t gmr_launch_ik_streams(const uint4* d_image, const gmr::IkLayout* L, const gmr::IkParams* P, int S, int T, const double* d_q0,
                                 const double* d_human, const int32_t* d_len, const double* d_scale, int flags, double* d_q_out,
                                 int32_t* d_nsolve, int32_t* d_status, double* d_tgt_out, double* d_err_out, hipStream_t stream,
                                 unsigned long long* d_prof, int vlim,     // vlim: the image's velocity bounds are not all +inf
                                 const double* d_weight);                  // [S][T][nhum] per-frame body weights, or null
hipError_t gmr_ik_set_max_smem(int nvp, int nw, int tree_small, int bytes);
// gmr_ik_wide.hip
hipError_t gmr_launch_ik_wide(const char* d_image, const gmr::WideLayout* L, const gmr::IkParams* P, int S, int T, const double* d_q0,
                              const double* d_human, const int32_t* d_len, const double* d_scale, int flags, double* d_q_out,
                              int32_t* d_nsolve, int32_t* d_status, double* d_tgt_out, double* d_err_out, hipStream_t stream,
                              unsigned long long* d_prof, void* pool, int fwin, const double* d_weight);    // fwin, d_weight: as in gmr_wide_job_desc
hipError_t gmr_launch_ik_wide_group(const gmr_wide_job_desc* jd, int njobs, int flags, hipStream_t stream, unsigned long long* d_prof,
                                    void* pool);
hipError_t gmr_launch_ik_wide_window(const gmr_wide_job_desc* jd, int njobs, int flags, hipStream_t stream, unsigned long long* d_prof,
                                     void* pool, int t_begin, int t_end);
void* gmr_ik_wide_pool_create();
void gmr_ik_wide_pool_destroy(void* pool);
void gmr_ik_wide_pool_set_chunk(void* pool, int chunk);
hipError_t gmr_ik_wide_attributes(int* num_regs, int* lds_bytes, int* max_waves_per_cu);
// gmr_fk.hip
hipError_t gmr_launch_fk_batch(const gmr::FkTree* d_tree, const gmr::FkTree* h_tree, int B, const float* d_root_pos, const float* d_root_rot,
                               const float* d_dof, float* d_body_pos, float* d_body_rot, float* d_min_part, float* d_min_z,
                               hipStream_t stream);
int gmr_fk_blocks(int B);
hipError_t gmr_launch_fk_segment_min(const float* d_body_pos, int nbody, const int32_t* d_seg_start, int nseg, float* d_seg_min,
                                     hipStream_t stream);
hipError_t gmr_launch_fk_qpos(const gmr::FkTree* d_tree, const gmr::FkTree* h_tree, int B, const double* const* d_row_q, int world,
                              float* d_body_pos, hipStream_t stream);
// gmr_post.hip
hipError_t gmr_launch_post_row_map(const gmr::PostSources* src, const int32_t* d_seg_start, int C, int B, int nq, const double** d_row_q,
                                   int32_t* d_row_clip, int32_t* d_seg_clamped, hipStream_t stream);
hipError_t gmr_launch_post_gather(const double* const* d_row_q, const int32_t* d_row_clip, const int32_t* d_seg_clamped,
                                  const float* d_lowest, int B, int nq, int flags, double ground_offset, double* d_root_pos,
                                  double* d_root_rot, double* d_dof_pos, hipStream_t stream);
}
