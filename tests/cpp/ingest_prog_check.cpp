// Host check of the walk programs behind the clip ingest kernels (csrc/gmr_smplx_prog.h: make_prog, smplx_make_progs, smplx_lds;
// csrc/gmr_bvh_prog.h: bvh_make_prog).  Reads cases from stdin, one per line:
//   S name J parent[0..J) nsel sel[0..nsel)                       (nsel = 0: the all-joints handle)
//   B name J parent[0..J) nsel sel_pos[0..nsel) sel_rot[0..nsel)
// builds the programs the way gmr_smplx_create / gmr_bvh_create do and replays them symbolically, the way the kernels walk them:
// which JOINT's transform sits in "the previous step", in the register slot, in every LDS slot and -- for the align kernels --
// at every depth level of the stack.  Asserted, per program:
//   - the transform a step loads is that of the step's actual parent joint (SMPL-X joints / batch walk: load == -1, == rslot,
//     >= 0; align walk: stack[depth - 1]; BVH: -2, -1, a slot);
//   - every slot index is >= 0 and below the number of slots the LDS size pays for (SMPL-X joints: max(nslot - 1, 1); the batch
//     kernel: batch_nslot; BVH: nslot), and nslot is not larger than what the program uses;
//   - a slot is written only at a step AFTER the last reader of what it holds (the allocators' own rule: "free again after the
//     last child that reads it");
//   - n, max_depth, joint[], depth[], row[], parent[] agree with the tree and the selection; every kept joint is walked once,
//     parents first;
//   - BVH: every (row, position / orientation) pair is in ent exactly once, under the step of its joint; ent0[n] fits its
//     unsigned char; n <= 64; rcol / pcol lie inside a row for both channel layouts;
//   - the LDS byte counts are those of the launches (restated here with literal sizes), and a case is refused exactly when
//     they exceed 160 * 1024 - 1024 or the closure exceeds 64 steps.
// One line per case on stdout; "ok <cases>" at the end.  Exit status 1 with the reason on stderr otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../general_motion_retargeting_amd/csrc/gmr_bvh_prog.h"
#include "../../general_motion_retargeting_amd/csrc/gmr_smplx_prog.h"

using gmr::BvhProg;
using gmr::SmplxProg;

static std::string g_what;
#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "%s: CHECK failed: %s : ", g_what.c_str(), #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return false; } } while (0)

static const int LDS_LIMIT = 160 * 1024 - 1024;

static std::vector<int> depths(const std::vector<int32_t>& par) {
  std::vector<int> d(par.size(), 0);
  for (size_t j = 1; j < par.size(); j++) d[j] = d[par[j]] + 1;
  return d;
}

// the last step whose parent is joint j, per joint (-1: none), over the steps of a program
static std::vector<int> last_child_step(int J, const std::vector<int32_t>& par, const short* joint, int n) {
  std::vector<int> last(J, -1);
  for (int k = 0; k < n; k++)
    if (par[joint[k]] >= 0) last[par[joint[k]]] = k;
  return last;
}

// one SMPL-X program against the tree and the rows it must write; nlds = the LDS slots its joints-type launch pays for
static bool replay_smplx(const SmplxProg& P, const std::vector<int32_t>& par, const std::vector<char>& keep, const std::vector<int>& row_of,
                         int nrow, int nlds, const char* what) {
  const int J = (int)par.size();
  const std::vector<int> dep = depths(par);
  int nkeep = 0, md = 0;
  for (int j = 0; j < J; j++) if (keep[j]) { nkeep++; md = std::max(md, dep[j] + 1); }
  CHECK(P.J == J && P.nrow == nrow, "%s: J = %d, nrow = %d", what, P.J, P.nrow);
  CHECK(P.n == nkeep && P.n >= 1 && P.n <= SX_MAX_JOINTS, "%s: n = %d, %d joints kept", what, P.n, nkeep);
  CHECK(P.max_depth == md, "%s: max_depth = %d, the tree's %d", what, P.max_depth, md);
  CHECK(P.nslot >= 1 && P.nslot <= SX_MAX_JOINTS, "%s: nslot = %d", what, P.nslot);
  CHECK(nlds == std::max(P.nslot - 1, 1), "%s: %d LDS slots for nslot = %d", what, nlds, P.nslot);
  const int rslot = P.nslot - 1;
  const std::vector<int> last = last_child_step(J, par, P.joint, P.n);
  std::vector<int> seen(J, 0), row_seen(nrow, 0), lds(nlds, -1), stack(P.max_depth, -1);
  int prev = -1, reg = -1, top = -1;
  for (int k = 0; k < P.n; k++) {
    const int j = P.joint[k], d = P.depth[k];
    CHECK(j >= 0 && j < J && keep[j] && !seen[j], "%s: step %d walks joint %d", what, k, j);
    seen[j] = 1;
    CHECK(d == dep[j] && d < P.max_depth, "%s: step %d: depth %d of joint %d (%d)", what, k, d, j, dep[j]);
    CHECK((k == 0) == (d == 0) && (d == 0) == (par[j] < 0), "%s: step %d: joint %d at depth %d", what, k, j, d);
    CHECK(P.parent[k] == (par[j] < 0 ? 0 : par[j]), "%s: step %d: parent %d of joint %d", what, k, P.parent[k], j);
    CHECK(P.row[k] == row_of[j], "%s: step %d: row %d of joint %d (%d)", what, k, P.row[k], j, row_of[j]);
    if (P.row[k] >= 0) { CHECK(P.row[k] < nrow && !row_seen[P.row[k]], "%s: row %d", what, P.row[k]); row_seen[P.row[k]] = 1; }
    // the joints / batch walk
    const int ld = P.load[k], sv = P.save[k];
    if (d > 0) {
      int src;
      CHECK(ld >= -1, "%s: step %d: load %d", what, k, ld);
      if (ld == rslot) src = reg;
      else if (ld >= 0) { CHECK(ld < nlds, "%s: step %d loads LDS slot %d of %d", what, k, ld, nlds); src = lds[ld]; }
      else src = prev;
      CHECK(src == par[j], "%s: step %d (joint %d, parent %d) loads the transform of joint %d (load = %d)", what, k, j, par[j], src, ld);
    }
    CHECK(sv >= -1, "%s: step %d: save %d", what, k, sv);
    if (sv >= 0) {
      int* cell = nullptr;
      if (sv == rslot) cell = &reg;
      else { CHECK(sv < nlds, "%s: step %d saves to LDS slot %d of %d", what, k, sv, nlds); cell = &lds[sv]; }
      CHECK(*cell < 0 || last[*cell] < k, "%s: step %d overwrites slot %d (joint %d, read until step %d)", what, k, sv, *cell, *cell < 0 ? -1 : last[*cell]);
      *cell = j;
      top = std::max(top, sv);
    }
    prev = j;
    // the align walk
    if (d > 0) CHECK(stack[d - 1] == par[j], "%s: step %d: stack[%d] holds joint %d, the parent is %d", what, k, d - 1, stack[d - 1], par[j]);
    stack[d] = j;
  }
  for (int r = 0; r < nrow; r++) CHECK(row_seen[r], "%s: row %d is never written", what, r);
  CHECK(P.nslot == std::max(top + 1, 1), "%s: nslot = %d, slots used up to %d", what, P.nslot, top);
  return true;
}

static bool check_smplx(const std::string& name, const std::vector<int32_t>& par, const std::vector<int32_t>& sel) {
  const int J = (int)par.size(), nsel = (int)sel.size();
  if (J < 1 || J > SX_MAX_JOINTS || nsel > J) { std::printf("%s kind=S J=%d nsel=%d refused=3\n", name.c_str(), J, nsel); return true; }
  static SmplxProg all, selp;
  const bool ok = gmr::smplx_make_progs(J, par.data(), nsel, nsel ? sel.data() : nullptr, &all, &selp);
  bool dup = false;
  std::vector<char> keep_all(J, 1), keep(J, 0);
  std::vector<int> row_all(J), row(J, -1);
  for (int j = 0; j < J; j++) row_all[j] = j;
  for (int r = 0; r < nsel; r++) {
    if (sel[r] < 0 || sel[r] >= J || row[sel[r]] >= 0) { dup = true; break; }
    row[sel[r]] = r;
    for (int a = sel[r]; a >= 0; a = par[a]) keep[a] = 1;
  }
  CHECK(ok == !dup, "smplx_make_progs returned %d for a selection that is %s", (int)ok, dup ? "bad" : "good");
  if (!ok) { std::printf("%s kind=S J=%d nsel=%d refused=2\n", name.c_str(), J, nsel); return true; }
  if (nsel == 0) { keep = keep_all; row = row_all; }
  const gmr::SmplxLds L = gmr::smplx_lds(all, selp, nsel);
  if (!replay_smplx(all, par, keep_all, row_all, J, std::max(all.nslot - 1, 1), "all")) return false;
  if (!replay_smplx(selp, par, keep, row, nsel ? nsel : J, L.batch_nslot, "sel")) return false;
  // the launches: 2048 B per stack level, 6144 B per parked transform, the 64 x 63 float tile of the batch kernel
  CHECK(L.align == all.max_depth * 2048 && L.joints == std::max(all.nslot - 1, 1) * 6144, "lds align %d joints %d", L.align, L.joints);
  CHECK(L.batch_nslot == std::max(selp.nslot - 1, 1) && L.batch_joints == L.batch_nslot * 6144 + 16128 && L.batch_align == selp.max_depth * 2048,
        "batch lds: %d slots, %d, %d", L.batch_nslot, L.batch_joints, L.batch_align);
  CHECK(selp.max_depth <= all.max_depth, "the selection is deeper (%d) than the tree (%d): the align launch sizes by the tree", selp.max_depth, all.max_depth);
  CHECK(L.align <= LDS_LIMIT, "align LDS %d", L.align);
  bool inside = nsel > 0;
  for (int j = 0; j < J; j++) if (keep[j] && j >= SX_BODY_JOINTS) inside = false;
  CHECK(L.batch_ok == (inside && L.batch_joints <= LDS_LIMIT), "batch_ok = %d", (int)L.batch_ok);
  if (L.batch_ok) CHECK(L.batch_align <= SX_BODY_JOINTS * 2048, "batch align LDS %d", L.batch_align);
  const int refused = L.joints > gmr::SX_LDS_LIMIT ? 1 : 0;
  CHECK(refused == (L.joints > LDS_LIMIT), "refused = %d at %d bytes", refused, L.joints);
  std::printf("%s kind=S J=%d nsel=%d n=%d nslot=%d max_depth=%d sel_n=%d sel_nslot=%d sel_depth=%d lds_align=%d lds_joints=%d batch_ok=%d "
              "batch_nslot=%d batch_lds_joints=%d batch_lds_align=%d refused=%d\n", name.c_str(), J, nsel, all.n, all.nslot, all.max_depth, selp.n,
              selp.nslot, selp.max_depth, L.align, L.joints, (int)L.batch_ok, L.batch_nslot, L.batch_joints, L.batch_align, refused);
  return true;
}

static bool check_bvh(const std::string& name, const std::vector<int32_t>& par, const std::vector<int32_t>& sp, const std::vector<int32_t>& sr) {
  const int J = (int)par.size(), nsel = (int)sp.size();
  if (J < 1 || J > BVH_MAX_JOINTS || nsel < 1 || nsel > BVH_MAX_ROWS) { std::printf("%s kind=B J=%d nsel=%d refused=3\n", name.c_str(), J, nsel); return true; }
  std::vector<char> keep(J, 0);
  for (int r = 0; r < nsel; r++) {
    CHECK(sp[r] >= 0 && sp[r] < J && sr[r] >= 0 && sr[r] < J, "row %d", r);
    for (int a = sp[r]; a >= 0; a = par[a]) keep[a] = 1;
    for (int a = sr[r]; a >= 0; a = par[a]) keep[a] = 1;
  }
  int nkeep = 0;
  for (int j = 0; j < J; j++) nkeep += keep[j];
  int nslot_out = 0, reuse = 0, status_out = 0;
  size_t lds_out = 0;
  for (int channels = 3; channels <= 6; channels += 3) {
    static BvhProg P;
    const int ax[3] = {2, 1, 0};
    size_t lds = 0;
    const gmr::BvhProgStatus st = gmr::bvh_make_prog(J, par.data(), channels, ax, nsel, sp.data(), sr.data(), &P, &lds);
    CHECK((st == gmr::BVH_PROG_STEPS) == (nkeep > BVH_MAX_STEPS), "status %d for a closure of %d joints", (int)st, nkeep);
    status_out = (int)st;
    if (st == gmr::BVH_PROG_STEPS) continue;
    CHECK(P.n == nkeep && P.n >= 1 && P.n <= 64, "n = %d, closure %d", P.n, nkeep);
    CHECK(P.J == J && P.nrow == nsel && P.ncol == (channels == 3 ? 3 + 3 * J : 6 * J), "J %d nrow %d ncol %d", P.J, P.nrow, P.ncol);
    CHECK(P.ax[0] == 2 && P.ax[1] == 1 && P.ax[2] == 0, "ax");
    CHECK(P.nslot >= 0 && P.nslot <= 64, "nslot = %d", P.nslot);
    const std::vector<int> last = last_child_step(J, par, P.joint, P.n);
    std::vector<int> slots(P.nslot, -1), nwrite(P.nslot, 0), seen(2 * nsel, 0);
    int prev = -1, pj = -1, top = -1;
    CHECK(P.ent0[0] == 0, "ent0[0] = %d", P.ent0[0]);
    for (int k = 0; k < P.n; k++) {
      const int j = P.joint[k];
      CHECK(j > pj && j < J && keep[j], "step %d walks joint %d after %d", k, j, pj);
      pj = j;
      CHECK(P.rcol[k] == (channels == 3 ? 3 + 3 * j : 6 * j + 3) && P.rcol[k] >= 0 && P.rcol[k] + 3 <= P.ncol, "step %d: rcol %d of %d", k, P.rcol[k], P.ncol);
      CHECK(P.pcol[k] == (channels == 3 ? (j == 0 ? 0 : -1) : 6 * j) && P.pcol[k] + 3 <= P.ncol, "step %d: pcol %d", k, P.pcol[k]);
      const int ld = P.load[k], sv = P.save[k];
      CHECK((ld == -2) == (k == 0) && (k == 0) == (j == 0), "step %d (joint %d): load %d", k, j, ld);
      if (k > 0) {
        int src = prev;
        CHECK(ld >= -1, "step %d: load %d", k, ld);
        if (ld >= 0) { CHECK(ld < P.nslot, "step %d loads slot %d of %d", k, ld, P.nslot); src = slots[ld]; }
        CHECK(src == par[j], "step %d (joint %d, parent %d) loads the transform of joint %d (load = %d)", k, j, par[j], src, ld);
      }
      CHECK(sv >= -1, "step %d: save %d", k, sv);
      if (sv >= 0) {
        CHECK(sv < P.nslot, "step %d saves to slot %d of %d", k, sv, P.nslot);
        CHECK(slots[sv] < 0 || last[slots[sv]] < k, "step %d overwrites slot %d (joint %d, read until step %d)", k, sv, slots[sv], slots[sv] < 0 ? -1 : last[slots[sv]]);
        slots[sv] = j;
        if (++nwrite[sv] > 1) reuse = 1;
        top = std::max(top, sv);
      }
      prev = j;
      CHECK(P.ent0[k + 1] >= P.ent0[k] && P.ent0[k + 1] <= 2 * nsel, "ent0[%d] = %d", k + 1, P.ent0[k + 1]);
      for (int e = P.ent0[k]; e < P.ent0[k + 1]; e++) {
        const int r = P.ent[e] >> 1, o = P.ent[e] & 1;
        CHECK(P.ent[e] >= 0 && r < nsel && !seen[P.ent[e]], "ent[%d] = %d", e, P.ent[e]);
        CHECK((o ? sr[r] : sp[r]) == j, "ent[%d]: row %d %s under joint %d", e, r, o ? "orientation" : "position", j);
        seen[P.ent[e]] = 1;
      }
    }
    CHECK(P.ent0[P.n] == 2 * nsel && 2 * nsel <= 255, "ent0[n] = %d for %d rows", P.ent0[P.n], nsel);
    for (int e = 0; e < 2 * nsel; e++) CHECK(seen[e], "row %d %s is never written", e >> 1, e & 1 ? "orientation" : "position");
    CHECK(P.nslot == top + 1, "nslot = %d, slots used up to %d", P.nslot, top);
    // the launch: 64 lanes x 7 doubles = 3584 B per output row and per parked joint
    CHECK(lds == (size_t)3584 * (nsel + P.nslot), "lds %zu for %d rows and %d slots", lds, nsel, P.nslot);
    CHECK((st == gmr::BVH_PROG_LDS) == (lds > (size_t)LDS_LIMIT), "status %d at %zu bytes", (int)st, lds);
    if (channels == 6) CHECK(nslot_out == P.nslot && lds_out == lds, "the two channel layouts differ in slots");
    nslot_out = P.nslot; lds_out = lds;
  }
  std::printf("%s kind=B J=%d nsel=%d n=%d nslot=%d lds=%zu reuse=%d refused=%d\n", name.c_str(), J, nsel, nkeep, nslot_out, lds_out, reuse, status_out);
  return true;
}

int main() {
  std::string line;
  long ncase = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string kind, name;
    int J = 0, nsel = 0;
    in >> kind >> name >> J;
    g_what = name;
    if (!in || J < 0 || J > 4096) { std::fprintf(stderr, "%s: bad line\n", name.c_str()); return 1; }
    std::vector<int32_t> par(J);
    for (int j = 0; j < J; j++) in >> par[j];
    in >> nsel;
    if (!in || nsel < 0 || nsel > 4096) { std::fprintf(stderr, "%s: bad line\n", name.c_str()); return 1; }
    std::vector<int32_t> a(nsel), b(nsel);
    for (int r = 0; r < nsel; r++) in >> a[r];
    if (kind == "B") for (int r = 0; r < nsel; r++) in >> b[r];
    if (!in) { std::fprintf(stderr, "%s: short line\n", name.c_str()); return 1; }
    for (int j = 0; j < J; j++)
      if ((j == 0) != (par[j] < 0) || par[j] >= j) { std::fprintf(stderr, "%s: parents must precede children\n", name.c_str()); return 1; }
    const bool ok = kind == "S" ? check_smplx(name, par, a) : kind == "B" ? check_bvh(name, par, a, b) : false;
    if (!ok) return 1;
    ncase++;
  }
  std::printf("ok %ld\n", ncase);
  return 0;
}
