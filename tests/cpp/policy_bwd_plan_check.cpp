// The host's plan of the backward pass through the motion tracker's two networks (csrc/gmr_tracker_policy_bwd_plan.h) driven on the CPU
// (plain C++, no HIP), with a gmr_fail of its own that records the message:
//   * policy_bwd_chunks at 1, chunk - 1, chunk, chunk + 1 rows and at the cap;
//   * policy_bwd_plan for tiny, odd, wide and the reference's shapes: chunk counts, tile counts, the floats of a chunk's record, the
//     offsets of every tensor in it, the LDS of the sweep and the bytes of the block;
//   * the tile tables: every element of every dW covered exactly once, the bias flag on the tiles at i0 = 0 and only there;
//   * the widest admissible shape at the cap stays below 1 GB and inside the capacity of the tile table;
//   * every refusal: the return code and the whole message.
// Prints "ok"; exit code 0 = all good.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../general_motion_retargeting_amd/csrc/gmr_tracker_policy_bwd_plan.h"

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "CHECK failed (line %d): %s : ", __LINE__, #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

static char g_message[512];
static int g_calls = 0;

int gmr_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_message, sizeof g_message, fmt, ap);
  va_end(ap);
  g_calls++;
  return code;
}

struct Case {
  const char* name;
  int O, P, A, na;
  int ah[4];
  int nc;
  int ch[4];
  int tiles_a, tiles_c;
  long long elems_a, elems_c;
  int stride_a[2], stride_c[2];
};

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// every element of every dW of the network covered by exactly one tile, db by the tiles at i0 = 0
static int check_cover(const gmr::PolicyShape& s, const gmr::PolicyBwdNet& n, const std::vector<gmr::PolicyBwdTile>& tab) {
  for (int l = 0; l <= s.L; l++) {
    const int K = s.width[l], N = s.width[l + 1];
    std::vector<int> w((size_t)N * K, 0), b(N, 0);
    for (int k = 0; k < n.tiles; k++) {
      const gmr::PolicyBwdTile& t = tab[k];
      if (t.layer != l) continue;
      CHECK(t.j0 % 64 == 0 && t.i0 % 64 == 0 && t.j0 < N && t.i0 < K && t.bias == (t.i0 == 0), "tile %d of layer %d", k, l);
      for (int j = t.j0; j < t.j0 + 64 && j < N; j++) {
        for (int i = t.i0; i < t.i0 + 64 && i < K; i++) w[(size_t)j * K + i]++;
        if (t.bias) b[j]++;
      }
    }
    for (int x : w) CHECK(x == 1, "layer %d: an element of dW covered %d times", l, x);
    for (int x : b) CHECK(x == 1, "layer %d: an element of db covered %d times", l, x);
  }
  for (int k = 1; k < n.tiles; k++) CHECK(tab[k].layer >= tab[k - 1].layer, "the tiles of a layer follow one another");
  return 0;
}

static int check_plans() {
  const int C = GMR_POLICY_BWD_CHUNK;
  CHECK(C == 256 && C % 32 == 0 && GMR_POLICY_BWD_MAX_ROWS == 131072, "the constants");
  CHECK(gmr::policy_bwd_chunks(1) == 1 && gmr::policy_bwd_chunks(C - 1) == 1 && gmr::policy_bwd_chunks(C) == 1 && gmr::policy_bwd_chunks(C + 1) == 2 &&
            gmr::policy_bwd_chunks(2 * C + 3) == 3 && gmr::policy_bwd_chunks(GMR_POLICY_BWD_MAX_ROWS) == 512,
        "chunks");
  const Case cases[] = {
      {"tiny", 1, 0, 1, 1, {32}, 1, {32}, 2, 2, 97, 97, {4, 8}, {4, 8}},
      {"odd", 5, 2, 3, 4, {64, 32, 256, 96}, 4, {64, 32, 256, 96}, 16, 16, 35875, 35809, {260, 100}, {260, 100}},
      {"wide", 512, 0, 32, 3, {256, 128, 128}, 1, {32}, 46, 9, 184864, 16449, {132, 132}, {4, 8}},
      {"model", 5, 2, 3, 3, {256, 128, 128}, 3, {256, 256, 128}, 18, 30, 51331, 100865, {132, 132}, {132, 260}},
  };
  for (const Case& c : cases) {
    gmr::PolicyShape a, cr;
    CHECK(gmr::policy_plan(c.O, c.P, c.A, c.na, c.ah, c.nc, c.ch, &a, &cr) == GMR_OK, "%s: %s", c.name, g_message);
    for (long long rows : {1LL, (long long)C - 1, (long long)C, (long long)C + 1, 2LL * C + 3, 4096LL, (long long)GMR_POLICY_BWD_MAX_ROWS}) {
      gmr::PolicyBwdPlan p;
      g_calls = 0;
      CHECK(gmr::policy_bwd_plan(a, cr, rows, &p) == GMR_OK && g_calls == 0, "%s: %s", c.name, g_message);
      CHECK(p.max_rows == rows && p.chunks == (rows + C - 1) / C, "%s: %d chunks for %lld rows", c.name, p.chunks, rows);
      CHECK(p.actor.tiles == c.tiles_a && p.critic.tiles == c.tiles_c, "%s: tiles %d %d", c.name, p.actor.tiles, p.critic.tiles);
      CHECK(p.actor.elems == c.elems_a && p.critic.elems == c.elems_c, "%s: elems %lld %lld", c.name, (long long)p.actor.elems, (long long)p.critic.elems);
      CHECK(p.actor.stride[0] == c.stride_a[0] && p.actor.stride[1] == c.stride_a[1] && p.critic.stride[0] == c.stride_c[0] && p.critic.stride[1] == c.stride_c[1],
            "%s: strides %d %d %d %d", c.name, p.actor.stride[0], p.actor.stride[1], p.critic.stride[0], p.critic.stride[1]);
      CHECK(p.actor.lds == 32u * 4u * (size_t)(c.stride_a[0] + c.stride_a[1]) && p.critic.lds == 32u * 4u * (size_t)(c.stride_c[0] + c.stride_c[1]), "%s: lds", c.name);
      const long long most = c.elems_a > c.elems_c ? c.elems_a : c.elems_c;
      CHECK(p.o_part == 0 && p.o_tab_actor == up256((size_t)p.chunks * most * 4) && p.o_tab_critic == p.o_tab_actor + up256((size_t)c.tiles_a * 16) &&
                p.bytes == p.o_tab_critic + up256((size_t)c.tiles_c * 16),
            "%s: the block: %zu %zu %zu %zu", c.name, p.o_part, p.o_tab_actor, p.o_tab_critic, p.bytes);
    }
    // the record of a chunk: W_0, b_0, W_1, b_1, .. without gaps
    gmr::PolicyBwdNet n;
    std::vector<gmr::PolicyBwdTile> tab(gmr::PBW_MAX_TILES);
    for (const gmr::PolicyShape* s : {&a, &cr}) {
      gmr::policy_bwd_net(*s, &n, tab.data());
      long long at = 0;
      for (int l = 0; l <= s->L; l++) {
        CHECK(n.off[2 * l] == at, "%s: W_%d at %lld", c.name, l, (long long)n.off[2 * l]);
        at += (long long)s->width[l] * s->width[l + 1];
        CHECK(n.off[2 * l + 1] == at, "%s: b_%d at %lld", c.name, l, (long long)n.off[2 * l + 1]);
        at += s->width[l + 1];
      }
      CHECK(at == n.elems && n.tiles <= gmr::PBW_MAX_TILES, "%s: %lld floats", c.name, at);
      if (check_cover(*s, n, tab)) return 1;
    }
  }
  // pinned outright: the reference's model at 4 096 rows -- 16 chunks of the critic's 100 865 floats, then two tables of 18 and 30 tiles
  {
    gmr::PolicyShape a, cr;
    const int ah[3] = {256, 128, 128}, ch[3] = {256, 256, 128};
    gmr::PolicyBwdPlan p;
    CHECK(gmr::policy_plan(5, 2, 3, 3, ah, 3, ch, &a, &cr) == GMR_OK && gmr::policy_bwd_plan(a, cr, 4096, &p) == GMR_OK, "%s", g_message);
    CHECK(p.chunks == 16 && p.o_tab_actor == 6455552 && p.o_tab_critic == 6455552 + 512 && p.bytes == 6455552 + 512 + 512, "the block: %zu %zu %zu", p.o_tab_actor,
          p.o_tab_critic, p.bytes);
  }
  // the widest admissible shape at the cap: below 1 GB, the table inside its capacity, the sweep inside the LDS of a compute unit
  {
    gmr::PolicyShape a, cr;
    const int wide[4] = {256, 256, 256, 256};
    gmr::PolicyBwdPlan p;
    CHECK(gmr::policy_plan(512, 0, 32, 4, wide, 4, wide, &a, &cr) == GMR_OK && gmr::policy_bwd_plan(a, cr, GMR_POLICY_BWD_MAX_ROWS, &p) == GMR_OK, "%s", g_message);
    CHECK(p.actor.elems == 336928 && p.critic.elems == 336928 - 32 * 256 - 32 + 256 + 1 && p.chunks == 512, "widest: %lld", (long long)p.actor.elems);
    CHECK(p.o_tab_actor == 690028544u && p.bytes < 1000000000u, "widest: %zu bytes", p.bytes);
    CHECK(p.actor.tiles == gmr::PBW_MAX_TILES && p.actor.tiles == 84 && p.critic.tiles == 84, "widest: %d tiles", p.actor.tiles);
    CHECK(p.actor.lds == 32u * 520 * 4 && p.actor.lds <= 160u * 1024, "widest: %zu", p.actor.lds);
  }
  return 0;
}

static int check_refusals() {
  gmr::PolicyShape a, cr;
  const int one[1] = {32};
  CHECK(gmr::policy_plan(1, 0, 1, 1, one, 1, one, &a, &cr) == GMR_OK, "%s", g_message);
  const struct {
    long long rows;
    const char* message;
  } cases[] = {{0, "max_rows = 0, 1 .. GMR_POLICY_BWD_MAX_ROWS = 131072 are taken"},
               {-5, "max_rows = -5, 1 .. GMR_POLICY_BWD_MAX_ROWS = 131072 are taken"},
               {131073, "max_rows = 131073, 1 .. GMR_POLICY_BWD_MAX_ROWS = 131072 are taken"},
               {9223372036854775807LL, "max_rows = 9223372036854775807, 1 .. GMR_POLICY_BWD_MAX_ROWS = 131072 are taken"}};
  for (const auto& r : cases) {
    gmr::PolicyBwdPlan p;
    g_calls = 0;
    g_message[0] = 0;
    const int rc = gmr::policy_bwd_plan(a, cr, r.rows, &p);
    CHECK(rc == GMR_ERR_ARG && g_calls == 1 && std::strcmp(g_message, r.message) == 0, "\"%s\" instead of \"%s\"", g_message, r.message);
  }
  return 0;
}

int main() {
  if (check_plans() || check_refusals()) return 1;
  std::printf("ok\n");
  return 0;
}
