// gmr_bvh_prog.h -- the walk program of the BVH ingest kernels (gmr_bvh.hip) and the LDS size of bvh_frames_kernel, as
// gmr_bvh_create builds them.  Plain C++ with no HIP types, so that tests/cpp/ingest_prog_check.cpp compiles the same lines
// under g++ and replays the program without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#define BVH_MAX_JOINTS 256
#define BVH_MAX_STEPS 64        // joints walked: one bit each in a frame's flip mask
#define BVH_MAX_ROWS 64
#define BVH_BLOCK 64            // frames kernel: one wavefront, lane = frame

namespace gmr {

constexpr size_t BVH_LDS_LIMIT = 160 * 1024 - 1024;   // what a workgroup may ask of the 160 KB of a CU
constexpr size_t BVH_LDS_DEFAULT = 48 * 1024;         // dynamic LDS a kernel gets without hipFuncSetAttribute

struct BvhProg {
  int n;                              // joints walked: the ancestor closure of the selection, in joint order (parents first)
  int J, ncol, nrow, nslot;
  int ax[3];                          // axis (0, 1, 2 = x, y, z) of the three Euler channels, in channel order
  short joint[BVH_MAX_STEPS];         // joint index of step k
  short rcol[BVH_MAX_STEPS];          // column of its first rotation channel
  short pcol[BVH_MAX_STEPS];          // column of its first translation channel, or -1: the clip's offset of the joint
  signed char load[BVH_MAX_STEPS];    // parent transform: -2 none (root), -1 the previous step's, >= 0 an LDS slot
  signed char save[BVH_MAX_STEPS];    // slot this step's transform is parked in, or -1
  unsigned char ent0[BVH_MAX_STEPS + 1];   // outputs of step k: ent[ent0[k] .. ent0[k + 1])
  short ent[2 * BVH_MAX_ROWS];        // row * 2 + (0: position, 1: orientation)
};

enum BvhProgStatus { BVH_PROG_OK = 0, BVH_PROG_STEPS = 1, BVH_PROG_LDS = 2 };

// The program of a selection and the bytes of dynamic LDS its launch asks for.  The caller has checked 1 <= J <= BVH_MAX_JOINTS,
// channels (3 or 6), ax (a permutation of 0, 1, 2), that parents precede children with joint 0 the only root,
// 1 <= nsel <= BVH_MAX_ROWS and every selected joint in [0, J).  BVH_PROG_STEPS: the closure needs more than BVH_MAX_STEPS
// joints; BVH_PROG_LDS: rows and parked joints do not fit the LDS (*P and *lds_bytes then say how many).
inline BvhProgStatus bvh_make_prog(int J, const int32_t* parents, int channels, const int* ax, int nsel, const int32_t* sel_pos,
                                   const int32_t* sel_rot, BvhProg* Pout, size_t* lds_bytes) {
  std::vector<char> keep(J, 0);
  for (int r = 0; r < nsel; r++) {
    for (int a = sel_pos[r]; a >= 0 && !keep[a]; a = parents[a]) keep[a] = 1;
    for (int a = sel_rot[r]; a >= 0 && !keep[a]; a = parents[a]) keep[a] = 1;
  }
  BvhProg& P = *Pout;
  memset(&P, 0, sizeof P);
  P.J = J;
  P.ncol = channels == 3 ? 3 + 3 * J : 6 * J;
  P.nrow = nsel;
  for (int i = 0; i < 3; i++) P.ax[i] = ax[i];
  std::vector<int> step_of(J, -1);
  int n = 0;
  for (int j = 0; j < J; j++) {
    if (!keep[j]) continue;
    if (n == BVH_MAX_STEPS) return BVH_PROG_STEPS;
    step_of[j] = n;
    P.joint[n] = (short)j;
    P.rcol[n] = (short)(channels == 3 ? 3 + 3 * j : 6 * j + 3);
    P.pcol[n] = (short)(channels == 3 ? (j == 0 ? 0 : -1) : 6 * j);
    n++;
  }
  P.n = n;
  // parent transforms: in registers when the parent is the previous step, else parked in an LDS slot that is free again
  // after the last child that reads it
  std::vector<int> last_use(n, -1), slot(n, -1);
  for (int k = 1; k < n; k++) {
    const int pk = step_of[parents[P.joint[k]]];
    if (pk != k - 1) last_use[pk] = k;
  }
  std::vector<int> busy_until;      // per slot
  for (int k = 0; k < n; k++) {
    P.save[k] = -1;
    if (k == 0) {
      P.load[k] = -2;
    } else {
      const int pk = step_of[parents[P.joint[k]]];
      P.load[k] = (signed char)(pk == k - 1 ? -1 : slot[pk]);
    }
    if (last_use[k] >= 0) {
      int sidx = -1;
      for (size_t i = 0; i < busy_until.size(); i++)
        if (busy_until[i] < k) { sidx = (int)i; break; }
      if (sidx < 0) { sidx = (int)busy_until.size(); busy_until.push_back(0); }
      busy_until[sidx] = last_use[k];
      slot[k] = sidx;
      P.save[k] = (signed char)sidx;
    }
  }
  P.nslot = (int)busy_until.size();
  int ne = 0;
  for (int k = 0; k < n; k++) {
    P.ent0[k] = (unsigned char)ne;
    for (int r = 0; r < nsel; r++) {
      if (sel_pos[r] == P.joint[k]) P.ent[ne++] = (short)(r * 2);
      if (sel_rot[r] == P.joint[k]) P.ent[ne++] = (short)(r * 2 + 1);
    }
  }
  P.ent0[n] = (unsigned char)ne;
  // bvh_frames_kernel: stage [BVH_BLOCK][nrow * 7], slots [nslot][7][BVH_BLOCK] doubles
  *lds_bytes = ((size_t)BVH_BLOCK * nsel * 7 + (size_t)P.nslot * 7 * BVH_BLOCK) * sizeof(double);
  return *lds_bytes > BVH_LDS_LIMIT ? BVH_PROG_LDS : BVH_PROG_OK;
}

}  // namespace gmr
