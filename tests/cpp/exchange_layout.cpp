// Where the tree solver's exchange buffers (Schur parts, right-hand-side shares, multiplier shares) lie in the LDS
// layout of csrc/gmr_ik_layout.h, for a packed (gmr_model_t, gmr_taskset_t) pair read from a file and for both launch
// shapes.  One line per shape, offsets in doubles:
//   nw=4 nvp=36 Kt=1270 H=2958 c=4292 n_double=4918 spart=4438 rpart=4838 gpart=4878 smem=62896
// (nw = 1: the buffers alias the dead assembly scratch behind 4 x 16 x 19 doubles of [Kt, H); gpart is unused there)
#include <cstdio>

#include "../../general_motion_retargeting_amd/csrc/gmr_ik_layout.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  static gmr_model_t m;
  static gmr_taskset_t ts;
  if (std::fread(&m, sizeof m, 1, f) != 1 || std::fread(&ts, sizeof ts, 1, f) != 1) return 2;
  std::fclose(f);
  for (int nw : {4, 1}) {
    const gmr::IkLayout L = gmr::make_ik_layout(m, ts, gmr::make_ik_schedule(m, ts, nw == 1 ? 64 : 192), nw);
    std::printf("nw=%d nvp=%d Kt=%d H=%d c=%d n_double=%d spart=%d rpart=%d gpart=%d smem=%d\n", nw, L.nvp, L.o.Kt, L.o.H, L.o.c,
                L.o.n_double, L.o.tr_spart, L.o.tr_rpart, L.o.tr_gpart, L.smem_bytes);
  }
  return 0;
}
