// Host check of the plan behind fk_split_kernel (csrc/gmr_fk_tree.h: fk_build_split).  Reads trees from stdin, one per line:
//   name nbody parent[0..nbody) dof_idx[0..nbody)
// fills FkTree::rec the way gmr_fk_create does (meta bit 0 and dof_idx are what the plan reads; the other flag bits get a
// pattern that must survive), and for every wavefront limit 1..4, with and without GMR_FK_NO_SHARE, replays wrec the way the
// kernel walks it -- per wavefront and step: [barrier] -> read the NEXT record's parked angle -> load the parent -> save to
// spare / private slot / shared slot -> store the outputs -- asserting what the kernel takes for granted:
//   - every body is stored by exactly one wavefront, every list opens with body 0;
//   - the transform a record's `src` yields (previous body, spare, private slot, shared slot) is the body's parent;
//   - a slot is written by one wavefront only; one that others read is written before the writer's barrier and read at or
//     after the reader's;
//   - all wavefronts execute the same number of barriers (record flag bit 5 plus wave_tail_barrier; never on a first record);
//   - a parked angle is read before its parking word is overwritten, the word lies in a body the wavefront itself stores
//     (so no two wavefronts write one staging word), an extra column lies below nextra and belongs to one angle;
//   - slots, extra columns and records are within nslot_split, nextra and wrec;
//   - a tree that fell back has nwave == 1; rec is never touched.
// One line per (tree, limit, sharing) on stdout; "ok" at the end.  Exit status 1 with the reason on stderr otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../general_motion_retargeting_amd/csrc/gmr_fk_tree.h"

using gmr::FkBodyRec;
using gmr::FkTree;

static std::string g_what;
#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "%s: CHECK failed: %s : ", g_what.c_str(), #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return false; } } while (0)

struct SlotWrite { int wave, step, body; };

// where a parked angle lives: an extra column (0x8000 | index) or a float offset in the lane's staging row
static int park_key(uint32_t next_park) { return (next_park & 0x40000000u) ? (int)(0x8000u | (next_park & 0x7fffu)) : (int)(next_park & 0xffffu); }

static bool replay(const FkTree& t, const int* parent, const int32_t* dof_idx, int* nprivate, int* spare_any, int* maxpark) {
  const int nb = t.nbody, nw = t.nwave;
  CHECK(nw >= 1 && nw <= gmr::FK_MAX_WAVES, "nwave = %d", nw);
  CHECK(t.wave_start[0] == 0, "wave_start[0] = %d", t.wave_start[0]);
  for (int w = 0; w < nw; w++) CHECK(t.wave_start[w + 1] > t.wave_start[w], "wavefront %d has an empty list", w);
  for (int w = nw; w <= gmr::FK_MAX_WAVES; w++) CHECK(t.wave_start[w] == t.wave_start[nw], "wave_start[%d]", w);
  const int nrec = t.wave_start[nw];
  CHECK(nrec <= 2 * gmr::FK_MAX_BODIES, "%d records", nrec);
  CHECK(t.nslot_split >= 0 && t.nslot_split <= 253, "nslot_split = %d", t.nslot_split);
  CHECK(t.nextra >= 0 && t.nextra < 0x8000, "nextra = %d", t.nextra);

  int owner[gmr::FK_MAX_BODIES], own_step[gmr::FK_MAX_BODIES];
  for (int b = 0; b < nb; b++) owner[b] = -1;
  int barrier_step[gmr::FK_MAX_WAVES], nbarrier[gmr::FK_MAX_WAVES];
  std::map<int, std::vector<SlotWrite>> writes;       // slot -> writes
  // pass 1: ownership, barriers, slot writes
  for (int w = 0; w < nw; w++) {
    const int i0 = t.wave_start[w], i1 = t.wave_start[w + 1];
    barrier_step[w] = -1; nbarrier[w] = 0;
    CHECK((int)(t.wrec[i0].meta >> 24) == 0, "list %d opens with body %u", w, t.wrec[i0].meta >> 24);
    CHECK(!(t.wrec[i0].meta & 32u), "barrier flag on the first record of list %d (the kernel ignores it there)", w);
    CHECK(((t.wrec[i0].meta >> 6) & 3u) == 0, "shared save on the first record of list %d (the kernel ignores it there)", w);
    for (int i = i0; i < i1; i++) {
      const FkBodyRec& r = t.wrec[i];
      const int s = i - i0, b = (int)(r.meta >> 24);
      CHECK(b < nb, "body %d", b);
      const FkBodyRec& o = t.rec[b];
      CHECK((r.meta & 0xFu) == (o.meta & 0xFu) && !memcmp(r.t, o.t, sizeof r.t) && !memcmp(r.r, o.r, sizeof r.r) && !memcmp(r.axis, o.axis, sizeof r.axis) &&
            r.dof_idx == o.dof_idx && ((r.next_park ^ o.next_park) & 0x70000u) == 0, "record %d is not body %d's", i, b);
      if (r.meta & 16u) { CHECK(owner[b] < 0, "body %d stored by wavefronts %d and %d", b, owner[b], w); owner[b] = w; own_step[b] = s; }
      if (i > i0 && (r.meta & 32u)) { barrier_step[w] = s; nbarrier[w]++; }
      const int dst = (int)((r.meta >> 16) & 255u) - 1;
      if (dst >= 0 && dst != 254) { CHECK(dst < t.nslot_split, "save slot %d of %d", dst, t.nslot_split); writes[dst].push_back({w, s, b}); }
      const int xd = (int)((r.meta >> 6) & 3u);
      if (xd) { CHECK(xd - 1 < t.nslot_split, "shared slot %d of %d", xd - 1, t.nslot_split); writes[xd - 1].push_back({w, s, b}); }
    }
    CHECK(t.wave_tail_barrier[w] == 0 || t.wave_tail_barrier[w] == 1, "wave_tail_barrier[%d] = %d", w, t.wave_tail_barrier[w]);
    if (t.wave_tail_barrier[w]) { CHECK(barrier_step[w] < 0, "list %d: a flagged record and a tail barrier", w); barrier_step[w] = i1 - i0; nbarrier[w]++; }
  }
  for (int w = nw; w < gmr::FK_MAX_WAVES; w++) CHECK(t.wave_tail_barrier[w] == 0, "tail barrier of an absent wavefront %d", w);
  for (int b = 0; b < nb; b++) CHECK(owner[b] >= 0, "body %d is stored by no wavefront", b);
  for (int w = 1; w < nw; w++) CHECK(nbarrier[w] == nbarrier[0], "wavefront %d executes %d barriers, wavefront 0 %d: a hang", w, nbarrier[w], nbarrier[0]);
  CHECK(nbarrier[0] <= 1, "%d mid-walk barriers", nbarrier[0]);
  for (auto& kv : writes) {
    std::set<int> ws;
    for (auto& x : kv.second) ws.insert(x.wave);
    CHECK(ws.size() == 1, "slot %d is written by %zu wavefronts", kv.first, ws.size());
  }
  // pass 2: parents
  *nprivate = 0; *spare_any = 0;
  std::set<int> shared_slots;
  for (int w = 0; w < nw; w++) {
    const int i0 = t.wave_start[w], i1 = t.wave_start[w + 1];
    int prev = -1, spare = -1;
    for (int i = i0; i < i1; i++) {
      const FkBodyRec& r = t.wrec[i];
      const int s = i - i0, b = (int)(r.meta >> 24);
      const int src = (int)((r.meta >> 8) & 255u) - 1, dst = (int)((r.meta >> 16) & 255u) - 1;
      if (i > i0) {
        const int p = parent[b];
        int got = -2;
        if (src < 0) got = prev;
        else if (src == 254) got = spare;
        else {
          CHECK(src < t.nslot_split, "load slot %d of %d", src, t.nslot_split);
          const auto it = writes.find(src);
          CHECK(it != writes.end(), "list %d step %d reads slot %d that nobody writes", w, s, src);
          const int ow = it->second[0].wave;
          if (ow == w) {
            for (auto& x : it->second) if (x.step < s) got = x.body;        // (in step order)
          } else {
            shared_slots.insert(src);
            CHECK(barrier_step[ow] >= 0 && barrier_step[w] >= 0, "slot %d crosses wavefronts %d -> %d without a barrier", src, ow, w);
            for (auto& x : it->second) {
              CHECK(x.step < barrier_step[ow], "slot %d: wavefront %d writes it in step %d, at or after its barrier (step %d)", src, ow, x.step, barrier_step[ow]);
              got = x.body;
            }
            CHECK(s >= barrier_step[w], "slot %d: wavefront %d reads it in step %d, before its barrier (step %d)", src, w, s, barrier_step[w]);
          }
        }
        CHECK(got == p, "list %d step %d: body %d continues from body %d (src %d), its parent is %d", w, s, b, got, src, p);
      }
      if (dst == 254) { spare = b; *spare_any = 1; }
      prev = b;
    }
  }
  for (auto& kv : writes) if (!shared_slots.count(kv.first)) {
    bool read = false;                                   // (a slot only its writer reads is a private one)
    for (int i = 0; i < nrec && !read; i++) read = (int)((t.wrec[i].meta >> 8) & 255u) - 1 == kv.first;
    if (read) (*nprivate)++;
  }
  // pass 3: parked angles
  *maxpark = 0;
  std::set<int> extra_seen;
  std::map<int, int> word_writer;
  for (int w = 0; w < nw; w++) {
    const int i0 = t.wave_start[w], i1 = t.wave_start[w + 1];
    std::map<int, int> dof_at;                             // parking place -> dof
    int n = 0;
    while (n < 32 && t.wave_park[w][n] != 0xffffffffu) n++;
    for (int k = n; k < 32; k++) CHECK(t.wave_park[w][k] == 0xffffffffu, "wave_park[%d] continues behind its end", w);
    *maxpark = n > *maxpark ? n : *maxpark;
    for (int k = 0; k < n; k++) {
      const uint32_t e = t.wave_park[w][k];
      const int dof = (int)(e & 0xffffu);
      CHECK(dof < t.ndof, "parked dof %d of %d", dof, t.ndof);
      int key;
      if (e >> 31) {
        const int idx = (int)((e >> 16) & 0x7fffu);
        CHECK(idx < t.nextra, "extra column %d of %d", idx, t.nextra);
        CHECK(extra_seen.insert(idx).second, "extra column %d holds two angles", idx);
        key = 0x8000 | idx;
      } else {
        key = (int)(e >> 16);
        CHECK(key < 3 * nb, "parking offset %d outside the staging row of %d floats", key, 3 * nb);
        CHECK(owner[key / 3] == w, "wavefront %d parks an angle in body %d, which wavefront %d stores", w, key / 3, owner[key / 3]);
        CHECK(word_writer.emplace(key, w).second, "staging word %d is a parking place twice", key);
      }
      CHECK(dof_at.emplace(key, dof).second, "parking place %d used twice by wavefront %d", key, w);
    }
    std::set<int> consumed;
    for (int i = i0; i < i1; i++) {
      const int s = i - i0;
      const uint32_t np = t.wrec[i].next_park;
      if (i + 1 >= i1) { CHECK(!(np >> 31), "the last record of list %d expects another angle", w); break; }
      const FkBodyRec& nx = t.wrec[i + 1];
      const int b = (int)(nx.meta >> 24);
      CHECK((bool)(np >> 31) == (bool)(nx.meta & 1u), "list %d step %d: angle announced %u, body %d has a hinge %u", w, s, np >> 31, b, nx.meta & 1u);
      if (!(np >> 31)) continue;
      const int key = park_key(np);
      const auto it = dof_at.find(key);
      CHECK(it != dof_at.end(), "list %d step %d: nothing is parked at %d", w, s + 1, key);
      CHECK(it->second == dof_idx[b] && nx.dof_idx == dof_idx[b], "list %d: body %d gets dof %d, its joint is dof %d", w, b, it->second, dof_idx[b]);
      CHECK(consumed.insert(key).second, "parking place %d read twice", key);
      // read in step s, before step s stores anything: the word must still be untouched (a staging word is overwritten
      // when the body it belongs to is stored)
      if (!(key & 0x8000)) CHECK(own_step[key / 3] >= s, "list %d: the angle of body %d is read in step %d, its parking word (body %d) was overwritten in step %d", w, b, s, key / 3, own_step[key / 3]);
    }
    CHECK(consumed.size() == dof_at.size(), "list %d parks %zu angles and reads %zu", w, dof_at.size(), consumed.size());
  }
  return true;
}

int main() {
  char name[256];
  int nb = 0, ntree = 0;
  while (std::scanf("%255s %d", name, &nb) == 2) {
    if (nb < 1 || nb > gmr::FK_MAX_BODIES) { std::fprintf(stderr, "%s: nbody %d\n", name, nb); return 2; }
    int parent[gmr::FK_MAX_BODIES];
    int32_t parent32[gmr::FK_MAX_BODIES], dof_idx[gmr::FK_MAX_BODIES];
    for (int b = 0; b < nb; b++) { if (std::scanf("%d", &parent[b]) != 1) return 2; parent32[b] = parent[b]; }
    int ndof = 0;
    for (int b = 0; b < nb; b++) { int d; if (std::scanf("%d", &d) != 1) return 2; dof_idx[b] = d; if (d >= 0) ndof++; }
    for (int b = 1; b < nb; b++) if (parent[b] < 0 || parent[b] >= b || dof_idx[b] >= ndof) { std::fprintf(stderr, "%s: bad tree\n", name); return 2; }
    for (int share = 1; share >= 0; share--) {
      if (share) unsetenv("GMR_FK_NO_SHARE"); else setenv("GMR_FK_NO_SHARE", "1", 1);
      for (int maxw = 1; maxw <= gmr::FK_MAX_WAVES; maxw++) {
        g_what = std::string(name) + " maxw=" + std::to_string(maxw) + (share ? "" : " no-share");
        static FkTree t, before;
        memset(&t, 0, sizeof t);
        t.nbody = nb; t.ndof = ndof;
        for (int b = 0; b < nb; b++) {
          FkBodyRec& r = t.rec[b];
          for (int a = 0; a < 3; a++) { r.t[a] = 0.25f * (float)(b + a); r.axis[a] = (double)(b - a); }
          for (int a = 0; a < 4; a++) r.r[a] = 0.5f * (float)(b * 4 + a);
          r.dof_idx = dof_idx[b];
          r.meta = (dof_idx[b] >= 0 ? 1u : 0u) | ((uint32_t)(b * 3) & 0xEu) | ((uint32_t)(b == 0 ? 0 : parent[b]) << 24);
          r.next_park = (uint32_t)((b * 5) & 7) << 16;
        }
        before = t;
        const char* why = gmr::fk_build_split(t, parent32, maxw);
        if (why) { std::fprintf(stderr, "%s: fk_build_split refuses a valid tree: %s\n", g_what.c_str(), why); return 1; }
        if (memcmp(t.rec, before.rec, sizeof t.rec) != 0) { std::fprintf(stderr, "%s: fk_build_split changed rec\n", g_what.c_str()); return 1; }
        // what the partition alone would have given: a tree that splits there and ends with one wavefront fell back
        int lists[gmr::FK_MAX_WAVES][gmr::FK_MAX_BODIES], nlist[gmr::FK_MAX_WAVES] = {0};
        const int nw_tree = nb >= 8 ? gmr::fk_split_tree(nb, parent, maxw, lists, nlist) : 1;
        const bool fallback = nw_tree > 1 && t.nwave == 1;
        if (t.nwave < 1 || t.nwave > maxw || (nw_tree == 1 && t.nwave != 1)) { std::fprintf(stderr, "%s: nwave = %d\n", g_what.c_str(), t.nwave); return 1; }
        int nprivate = 0, spare = 0, maxpark = 0;
        bool shared = false;
        if (fallback) {
          for (int w = 0; w < nw_tree; w++) {
            int h = 0;
            for (int i = 0; i < nlist[w]; i++) h += dof_idx[lists[w][i]] >= 0;
            maxpark = h > maxpark ? h : maxpark;
          }
        } else {
          bool park_complete = true;                     // (one wavefront whose list needs more than 32 parked angles: the kernel that
          if (t.nwave == 1) {                            //  runs then reads rec, not wrec)
            int h = 0;
            for (int b = 1; b < nb; b++) h += dof_idx[b] >= 0;
            park_complete = h <= 32;
          }
          if (park_complete && !replay(t, parent, dof_idx, &nprivate, &spare, &maxpark)) return 1;
          for (int i = 0; i < t.wave_start[t.nwave]; i++) shared = shared || ((t.wrec[i].meta >> 6) & 3u);
        }
        std::printf("%s maxw=%d share=%d nwave=%d shared=%d nslot=%d private=%d spare=%d nextra=%d maxpark=%d fallback=%d nrec=%d\n", name, maxw, share,
                    t.nwave, shared ? 1 : 0, t.nslot_split, nprivate, spare, t.nextra, maxpark, fallback ? 1 : 0, t.wave_start[t.nwave]);
      }
    }
    ntree++;
  }
  std::printf("ok %d\n", ntree);
  return 0;
}
