// Host check of the link plan behind tracker_links_kernel (csrc/gmr_link_plan.h: link_plan): reads "nbody p0 p1 .. nsel s0 s1 .."
// from stdin (nsel = 0: every body in order), builds the plan and replays it the way the kernel walks it: every list opens with
// the root, every body's parent is the body before or sits in the slot the step names, every selected body is served exactly
// once, and the step, slot and wavefront counts stay inside what LinkPlan holds.  Prints "steps=.. waves=.. slots=.. ok", or
// "refused: <why>" when link_plan says the selection cannot be planned.
#include <cstdio>
#include <cstdlib>

#include "../../general_motion_retargeting_amd/csrc/gmr_link_plan.h"

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s : ", #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main() {
  int nb = 0, nsel = 0;
  if (std::scanf("%d", &nb) != 1 || nb < 1 || nb > gmr::FK_MAX_BODIES) return 2;
  short parent[gmr::FK_MAX_BODIES];
  for (int b = 0; b < nb; b++) { int p; if (std::scanf("%d", &p) != 1) return 2; parent[b] = (short)(b == 0 ? 0 : p); }
  if (std::scanf("%d", &nsel) != 1 || nsel < 0 || nsel > nb) return 2;
  int32_t sel[gmr::FK_MAX_BODIES];
  for (int k = 0; k < nsel; k++) if (std::scanf("%d", &sel[k]) != 1) return 2;
  // guard words around the plan: an overrun of step[] shows
  struct { uint32_t before[64]; gmr::LinkPlan P; uint32_t after[64]; } g;
  for (int i = 0; i < 64; i++) g.before[i] = g.after[i] = 0xA5A5A5A5u;
  g.P = gmr::LinkPlan();
  const char* why = gmr::link_plan(nb, parent, nsel ? sel : nullptr, nsel ? nsel : nb, &g.P);
  for (int i = 0; i < 64; i++) CHECK(g.before[i] == 0xA5A5A5A5u && g.after[i] == 0xA5A5A5A5u, "guard word %d", i);
  if (why) { std::printf("refused: %s\n", why); return 0; }
  const gmr::LinkPlan& P = g.P;
  if (!nsel) { nsel = nb; for (int k = 0; k < nb; k++) sel[k] = k; }
  CHECK(P.nsel == nsel && P.nwave >= 1 && P.nwave <= gmr::FK_MAX_WAVES, "nsel %d nwave %d", P.nsel, P.nwave);
  CHECK(P.wave_start[0] == 0 && P.wave_start[P.nwave] <= gmr::LINK_MAX_STEPS, "steps %d", P.wave_start[P.nwave]);
  int served[gmr::FK_MAX_BODIES] = {0};
  for (int w = 0; w < P.nwave; w++) {
    const int i0 = P.wave_start[w], i1 = P.wave_start[w + 1];
    CHECK(i1 > i0 && (P.step[i0] & 255u) == 0u, "list %d must open with the root", w);
    int in_slot[256];
    for (int s = 0; s < 256; s++) in_slot[s] = -1;
    int prev = -1;
    for (int i = i0; i < i1; i++) {
      const uint32_t sc = P.step[i];
      const int b = (int)(sc & 255u), row = (int)((sc >> 8) & 255u), src = (int)((sc >> 16) & 255u) - 1, dst = (int)(sc >> 24) - 1;
      CHECK(b < nb && b > prev, "list %d: body %d after %d", w, b, prev);
      if (i > i0) {
        if (src < 0) CHECK(parent[b] == prev, "list %d: body %d follows %d, its parent is %d", w, b, prev, parent[b]);
        else CHECK(src < P.nslot && in_slot[src] == parent[b], "list %d: body %d loads slot %d holding %d", w, b, src, in_slot[src]);
      }
      if (dst >= 0) { CHECK(dst < P.nslot, "slot %d of %d", dst, P.nslot); in_slot[dst] = b; }
      if (row != 255) { CHECK(row < nsel && sel[row] == b, "row %d names body %d, walked at body %d", row, row < nsel ? sel[row] : -1, b); served[row]++; }
      prev = b;
    }
  }
  for (int k = 0; k < nsel; k++) CHECK(served[k] == 1, "selection row %d served %d times", k, served[k]);
  std::printf("steps=%d waves=%d slots=%d ok\n", P.wave_start[P.nwave], P.nwave, P.nslot);
  return 0;
}
