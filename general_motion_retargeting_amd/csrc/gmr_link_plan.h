// gmr_link_plan.h -- the link plan of a motion tracker: what tracker_links_kernel (gmr_tracker_links.hip)
// walks, and the host function that builds it from a tree and a selection.  Plain C++ over gmr_fk_tree.h, so that
// tests/cpp/link_plan_check.cpp compiles the same lines under g++.
#pragma once
#include <stdint.h>

#include "gmr_fk_tree.h"

namespace gmr {

constexpr int LINK_TERMS = 4;         // link pos, link rot, link vel, link ang vel
// every wavefront re-walks the trunk its subtrees hang from, so a tree with a long trunk in front of the branching costs up to
// FK_MAX_WAVES full walks: the true worst case, and link_plan still counts before it writes
constexpr int LINK_MAX_STEPS = FK_MAX_WAVES * FK_MAX_BODIES;
// The links of a tracker: the split walk over the ancestor closure of the selection and everything else a
// link step reads alike in every workgroup.  Built and validated on the host, travels as a kernel argument like TrackerTables.
// Wavefront w of a workgroup walks step[wave_start[w] .. wave_start[w + 1]), parents first, body 0 first:
//   [7:0] the body   [15:8] its row in the selection, 255: walked for its descendants only (or a row another wavefront serves)
//   [23:16] slot + 1 its parent's state is loaded from, 0: the parent is the body before   [31:24] slot + 1 its own state is parked in
struct LinkPlan {
  int32_t nsel = 0, nwave = 1, nslot = 0, frame = 0;   // nsel = 0: no links attached; frame: GMR_TRACKER_FRAME_*
  int32_t wave_start[FK_MAX_WAVES + 1] = {};
  uint32_t step[LINK_MAX_STEPS] = {};
  int32_t sim_body[FK_MAX_BODIES] = {};     // selection row s reads simulator body sim_body[s]
  float weight[FK_MAX_BODIES] = {};         // w_b >= 0 per selection row
  float wsum = 1.0f;                        // their float32 sum in row order, > 0
  // the link terms: a choice of this library (the reference has no link terms), 0.3 m, 0.8 rad, 2 m/s, 4 rad/s, weights of one
  float scale[LINK_TERMS] = {0.3f, 0.8f, 2.0f, 4.0f}, term_weight[LINK_TERMS] = {1.0f, 1.0f, 1.0f, 1.0f};
  float fail_dist = __builtin_inff();       // fail[e] = !(max_dist[e] <= fail_dist)
};

// The plan of a selection (host): fk_split_tree's partition of the whole tree, every list cut down to the bodies a selected body
// of that wavefront hangs from (a selected trunk body is served by the first wavefront that walks it), wavefronts left with
// nothing dropped; a parent that is not the body walked just before is parked in a slot, and a slot is free again after the
// last child that reads it.  Returns nullptr, or why the selection cannot be planned (nothing of *P is then to be used).
inline const char* link_plan(int nbody, const short* parent, const int32_t* sel, int nsel, LinkPlan* P) {
  int par[FK_MAX_BODIES], row_of[FK_MAX_BODIES];
  for (int b = 0; b < nbody; b++) { par[b] = b == 0 ? -1 : parent[b]; row_of[b] = -1; }
  for (int k = 0; k < nsel; k++) row_of[sel ? sel[k] : k] = k;
  int lists[FK_MAX_WAVES][FK_MAX_BODIES], nlist[FK_MAX_WAVES] = {0};
  int nw = nbody >= 8 ? fk_split_tree(nbody, par, FK_MAX_WAVES, lists, nlist) : 1;
  if (nw == 1) { nlist[0] = nbody; for (int b = 0; b < nbody; b++) lists[0][b] = b; }
  bool served[FK_MAX_BODIES] = {false};
  int n = 0, nslot = 0, wave = 0;
  for (int w = 0; w < nw; w++) {
    bool need[FK_MAX_BODIES] = {false}, mine[FK_MAX_BODIES] = {false};
    bool any = false;
    for (int i = 0; i < nlist[w]; i++) {
      const int b = lists[w][i];
      if (row_of[b] < 0 || served[b]) continue;
      served[b] = mine[b] = any = true;
      for (int a = b; a >= 0 && !need[a]; a = par[a]) need[a] = true;
    }
    if (!any) continue;
    int L[FK_MAX_BODIES], m = 0;
    for (int i = 0; i < nlist[w]; i++) if (need[lists[w][i]]) L[m++] = lists[w][i];
    // slots: last[i] = the last step that loads body L[i] from a slot, -1: never parked
    int last[FK_MAX_BODIES], slot_of[FK_MAX_BODIES], free_[FK_MAX_BODIES], nfree = 0;
    for (int i = 0; i < m; i++) { last[i] = -1; slot_of[i] = -1; }
    for (int i = 1; i < m; i++) {
      if (L[i - 1] == par[L[i]]) continue;
      for (int j = 0; j < i; j++) if (L[j] == par[L[i]]) last[j] = i;
    }
    if (n + m > LINK_MAX_STEPS) return "the walk of this selection needs more steps than a link plan holds";
    P->wave_start[wave] = n;
    for (int i = 0; i < m; i++) {
      uint32_t src = 0, dst = 0;
      if (i > 0 && L[i - 1] != par[L[i]]) {
        for (int j = 0; j < i; j++) {
          if (L[j] != par[L[i]]) continue;
          src = (uint32_t)slot_of[j] + 1;
          if (last[j] == i) free_[nfree++] = slot_of[j];
        }
      }
      if (last[i] >= 0) {
        slot_of[i] = nfree > 0 ? free_[--nfree] : nslot++;
        dst = (uint32_t)slot_of[i] + 1;
      }
      P->step[n++] = (uint32_t)L[i] | ((mine[L[i]] ? (uint32_t)row_of[L[i]] : 255u) << 8) | (src << 16) | (dst << 24);
    }
    wave++;
  }
  for (int w = wave; w <= FK_MAX_WAVES; w++) P->wave_start[w] = n;
  P->nsel = nsel; P->nwave = wave; P->nslot = nslot;
  return nullptr;
}

}  // namespace gmr
