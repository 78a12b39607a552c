// Prints what the IK kernels' host side (csrc/gmr_ik_layout.h) decides for a packed (gmr_model_t, gmr_taskset_t) pair
// read from a file: the limb / trunk decomposition of the tree solver and which of its instances the layout selects, the
// size class, whether the task set fits the throughput kernel (gmr_ik_wide_layout.h), the stage switches of
// make_ik_params and the tasks / (task, dof) pairs per stage.
//   tree_ok=1 tree_small=1 tree_class=36 tree_wide_fits=1 tree_use0=1 tree_use1=3 K=14,14 P=124,154 trunk=0,1,...
//   limb0=... limb1=... limb2=... limb3=... tree_nbody=38 tree_nhinge=29 tree_nhuman=14 tree_maxd=12 tree_nhop=4
//   tree_smem1=40624 tree_smem4=62896
// (bodies, hinges, human bodies, bodies on the longest root -> leaf path, FK rounds, LDS bytes of the one- and the
// 4-wavefront layout; the latter is stated for a robot that does not decompose too, although it is never launched)
#include <cstdio>

#include "../../general_motion_retargeting_amd/csrc/gmr_ik_layout.h"
#include "../../general_motion_retargeting_amd/csrc/gmr_ik_wide_layout.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  static gmr_model_t m;
  static gmr_taskset_t ts;
  if (std::fread(&m, sizeof m, 1, f) != 1 || std::fread(&ts, sizeof ts, 1, f) != 1) return 2;
  std::fclose(f);
  const gmr::IkTree tr = gmr::make_ik_tree(m);
  const gmr::IkSchedule sch = gmr::make_ik_schedule(m, ts, 192);
  const gmr::IkLayout L = gmr::make_ik_layout(m, ts, sch, 4);
  const gmr::IkParams prm = gmr::make_ik_params(m, ts);
  std::printf("tree_ok=%d tree_small=%d tree_class=%d tree_wide_fits=%d tree_use0=%d tree_use1=%d K=%d,%d P=%d,%d trunk=", L.tree_ok,
              L.tree_small, L.nvp, gmr::wide_fits(m, ts) ? 1 : 0, prm.use0, prm.use1, L.K[0], L.K[1], L.P[0], L.P[1]);
  for (int t = 0, k = 0; t < 10; t++) if (tr.trunk[t] >= 0) std::printf(k++ ? ",%d" : "%d", tr.trunk[t]);
  for (int l = 0; l < 4; l++) {
    std::printf(" limb%d=", l);
    for (int a = 0, k = 0; a < 8; a++) if (tr.limb[l][a] >= 0) std::printf(k++ ? ",%d" : "%d", tr.limb[l][a]);
  }
  // sizes: bodies, hinges, human bodies, bodies on the longest path, FK rounds, LDS bytes of the two launch shapes
  const gmr::IkLayout L1 = gmr::make_ik_layout(m, ts, gmr::make_ik_schedule(m, ts, 64), 1);
  std::printf(" tree_nbody=%d tree_nhinge=%d tree_nhuman=%d tree_maxd=%d tree_nhop=%d tree_smem1=%d tree_smem4=%d", L.nb, L.nh, L.nhum,
              L.maxd, L.nhop, L1.smem_bytes, L.smem_bytes);
  std::printf("\n");
  return 0;
}
