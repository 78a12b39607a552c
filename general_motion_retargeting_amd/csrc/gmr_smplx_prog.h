// gmr_smplx_prog.h -- the walk programs of the SMPL-X ingest kernels (gmr_smplx.hip) and the LDS sizes of their launches, as
// gmr_smplx_create builds them.  Plain C++ with no HIP types, so that tests/cpp/ingest_prog_check.cpp compiles the same lines
// under g++ and replays the programs without a device.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#define SX_MAX_JOINTS 64
#define SX_BLOCK 64
#define SX_BODY_JOINTS 22            // root_orient + pose_body: joints 0 .. 21
#define SX_BODY_POSE 63              // floats per pose_body row

namespace gmr {

constexpr int SX_LDS_LIMIT = 160 * 1024 - 1024;      // what a workgroup may ask of the 160 KB of a CU
constexpr int SX_LDS_DEFAULT = 48 * 1024;            // dynamic LDS a kernel gets without hipFuncSetAttribute

struct SmplxProg {
  int n;                         // joints visited (DFS order)
  int J;                         // joints per pose row
  int nrow;                      // rows written per frame
  int max_depth;                 // stack levels
  short joint[SX_MAX_JOINTS];    // joint index of step k
  short depth[SX_MAX_JOINTS];    // its depth (root = 0)
  short row[SX_MAX_JOINTS];      // output row or -1
  short parent[SX_MAX_JOINTS];   // parent JOINT index of step k (joints kernel: rest offsets)
  // joints kernel: the parent's transform is the previous step's (still in registers: load = -1) or parked in an LDS slot;
  // only joints with two or more visited children are parked (save >= 0).  SMPL-X: 3 slots instead of 11 stack levels
  short load[SX_MAX_JOINTS], save[SX_MAX_JOINTS];
  int nslot;
};

// DFS program over the joints in `keep` (all when empty); rows from `row_of` (-1 = not written)
inline bool make_prog(int J, const int32_t* parents, const std::vector<char>& keep, const std::vector<int>& row_of,
                      int nrow, SmplxProg* P) {
  memset(P, 0, sizeof *P);
  P->J = J;
  P->nrow = nrow;
  std::vector<std::vector<int>> kids(J);
  int root = -1;
  for (int j = 0; j < J; j++) {
    if (parents[j] < 0) { if (root >= 0) return false; root = j; }
    else kids[parents[j]].push_back(j);
  }
  if (root < 0) return false;
  std::vector<std::pair<int, int>> st;     // (joint, depth)
  st.push_back({root, 0});
  int n = 0, md = 0;
  while (!st.empty()) {
    auto [j, d] = st.back();
    st.pop_back();
    if (!keep[j]) continue;
    P->joint[n] = (short)j; P->depth[n] = (short)d; P->row[n] = (short)row_of[j];
    P->parent[n] = (short)(parents[j] < 0 ? 0 : parents[j]);
    n++;
    md = std::max(md, d + 1);
    for (int c = (int)kids[j].size() - 1; c >= 0; c--) st.push_back({kids[j][c], d + 1});
  }
  P->n = n;
  P->max_depth = md;
  // parking slots of the joints kernel: slot of a joint = the number of parked ancestors above it
  std::vector<int> nkept(J, 0), parked_above(J, 0), slot_of(J, -1);
  for (int k = 0; k < n; k++) if (k > 0) nkept[P->parent[k]]++;
  int ns = 0;
  for (int k = 0; k < n; k++) {
    const int j = P->joint[k], p = P->parent[k];
    parked_above[j] = k == 0 ? 0 : parked_above[p] + (nkept[p] >= 2 ? 1 : 0);
    P->save[k] = -1;
    if (nkept[j] >= 2) { slot_of[j] = parked_above[j]; P->save[k] = (short)slot_of[j]; ns = std::max(ns, slot_of[j] + 1); }
    P->load[k] = (short)((k == 0 || P->joint[k - 1] == p) ? -1 : slot_of[p]);
    if (k > 0 && P->joint[k - 1] != p && slot_of[p] < 0) return false;      // (cannot happen in DFS preorder)
  }
  P->nslot = std::max(ns, 1);
  return true;
}

// the two programs of a handle: every joint (rows = joint index) / the ancestor closure of the selection (all joints when
// nsel == 0).  false: a bad tree or a duplicate / out-of-range selection.  The caller has checked 1 <= J <= SX_MAX_JOINTS,
// 0 <= nsel <= J and that parents precede children with joint 0 the only root.
inline bool smplx_make_progs(int J, const int32_t* parents, int nsel, const int32_t* sel, SmplxProg* all, SmplxProg* selp) {
  std::vector<char> keep(J, 1);
  std::vector<int> row(J);
  for (int j = 0; j < J; j++) row[j] = j;
  bool ok = make_prog(J, parents, keep, row, J, all);
  if (ok && nsel > 0) {
    std::fill(keep.begin(), keep.end(), 0);
    std::fill(row.begin(), row.end(), -1);
    for (int r = 0; r < nsel && ok; r++) {
      int j = sel[r];
      if (j < 0 || j >= J || row[j] >= 0) { ok = false; break; }
      row[j] = r;
      for (int a = j; a >= 0; a = parents[a]) keep[a] = 1;
    }
    ok = ok && make_prog(J, parents, keep, row, nsel, selp);
  } else if (ok) {
    *selp = *all;
  }
  return ok;
}

// dynamic LDS of the launches of a handle, in bytes
struct SmplxLds {
  int align = 0;                 // smplx_align_kernel: [max_depth][4][SX_BLOCK] doubles (sized for the all-joints program)
  int joints = 0;                // smplx_joints_kernel: [max(nslot - 1, 1)][12][SX_BLOCK] doubles
  bool batch_ok = false;         // the selection's ancestor closure lies inside the body joints and its LDS fits
  int batch_nslot = 1;           // LDS slots in front of the pose tile of smplx_batch_joints_kernel
  int batch_joints = 0, batch_align = 0;
};

inline SmplxLds smplx_lds(const SmplxProg& all, const SmplxProg& sel, int nsel) {
  SmplxLds L;
  L.align = all.max_depth * 4 * SX_BLOCK * 8;
  L.joints = std::max(all.nslot - 1, 1) * 12 * SX_BLOCK * 8;
  // the batch entry points read root_orient + pose_body, the poses of joints 0 .. 21
  L.batch_ok = nsel > 0;
  for (int k = 0; k < sel.n; k++)
    if (sel.joint[k] >= SX_BODY_JOINTS) L.batch_ok = false;
  L.batch_nslot = std::max(sel.nslot - 1, 1);
  L.batch_joints = L.batch_nslot * 12 * SX_BLOCK * 8 + SX_BLOCK * SX_BODY_POSE * (int)sizeof(float);
  L.batch_align = sel.max_depth * 4 * SX_BLOCK * 8;
  if (L.batch_joints > SX_LDS_LIMIT) L.batch_ok = false;
  return L;
}

}  // namespace gmr
