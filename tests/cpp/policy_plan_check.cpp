// The host's plan of the motion tracker's two networks (csrc/gmr_tracker_policy_plan.h) driven on the CPU (plain C++, no HIP), with a
// gmr_fail of its own that records the message:
//   * policy_plan: the widths, the place of either network's (W, b) pairs in the parameter list, the two LDS strides and the bytes, for the
//     reference's model, for the smallest and for the widest networks the capacities allow;
//   * every refusal: the return code and the whole message;
//   * the widest plan stays inside the 160 KB of LDS of a compute unit.
// Prints "ok"; exit code 0 = all good.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../general_motion_retargeting_amd/csrc/gmr_tracker_policy_plan.h"

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

static int check_plans() {
  gmr::PolicyShape a, c;
  const int ah[3] = {256, 128, 128}, ch[3] = {256, 256, 128};
  g_calls = 0;
  CHECK(gmr::policy_plan(5, 2, 3, 3, ah, 3, ch, &a, &c) == GMR_OK && g_calls == 0, "%s", g_message);
  const int aw[5] = {5, 256, 128, 128, 3}, cw[5] = {7, 256, 256, 128, 1};
  for (int l = 0; l < 5; l++) CHECK(a.width[l] == aw[l] && c.width[l] == cw[l], "width %d: %d %d", l, a.width[l], c.width[l]);
  CHECK(a.L == 3 && c.L == 3 && c.first == 1 && a.first == 9 && gmr::policy_tensors(a, c) == 17, "first %d %d", c.first, a.first);
  // buffer 0 holds the padded input and h_2, buffer 1 h_1 and h_3; four floats more per row
  CHECK(a.stride[0] == 132 && a.stride[1] == 260 && c.stride[0] == 260 && c.stride[1] == 260, "strides %d %d %d %d", a.stride[0], a.stride[1], c.stride[0], c.stride[1]);
  CHECK(a.lds == 32u * (132 + 260) * 4 && c.lds == 32u * 520 * 4, "lds %zu %zu", a.lds, c.lds);
  CHECK(gmr::policy_padded(1) == 8 && gmr::policy_padded(8) == 8 && gmr::policy_padded(9) == 16 && gmr::policy_padded(512) == 512, "padded");
  // the smallest: one input, one hidden layer of 32, one action, no privileged columns
  const int one[1] = {32};
  CHECK(gmr::policy_plan(1, 0, 1, 1, one, 1, one, &a, &c) == GMR_OK, "%s", g_message);
  CHECK(a.stride[0] == 12 && a.stride[1] == 36 && a.first == 5 && gmr::policy_tensors(a, c) == 9 && c.width[0] == 1 && c.width[2] == 1, "smallest");
  // the widest: 512 inputs, four layers of 256, 32 actions -- and it fits the LDS of a compute unit
  const int wide[4] = {256, 256, 256, 256};
  CHECK(gmr::policy_plan(512, 0, 32, 4, wide, 4, wide, &a, &c) == GMR_OK, "%s", g_message);
  CHECK(a.stride[0] == 516 && a.stride[1] == 260 && a.lds == 32u * 776 * 4 && a.lds <= 160u * 1024 && c.lds == a.lds, "widest %zu", a.lds);
  CHECK(gmr::policy_tensors(a, c) == GMR_POLICY_MAX_TENSORS && a.width[5] == 32 && c.width[5] == 1, "tensors");
  CHECK(gmr::policy_plan(500, 12, 32, 4, wide, 1, one, &a, &c) == GMR_OK && c.width[0] == 512 && a.width[0] == 500 && a.stride[0] == 508, "%s", g_message);
  // rows of either buffer stay on sixteen bytes
  CHECK(a.stride[0] % 4 == 0 && a.stride[1] % 4 == 0, "alignment");
  return 0;
}

struct Refusal {
  int O, P, A, na;
  int ah[5];
  int nc;
  int ch[5];
  const char* message;
};

static int check_refusals() {
  const Refusal cases[] = {
      {0, 0, 3, 1, {32}, 1, {32}, "obs_cols = 0 and priv_cols = 0: obs_cols at least 1, priv_cols at least 0 and at most 512 together are taken"},
      {513, 0, 3, 1, {32}, 1, {32}, "obs_cols = 513 and priv_cols = 0: obs_cols at least 1, priv_cols at least 0 and at most 512 together are taken"},
      {500, 13, 3, 1, {32}, 1, {32}, "obs_cols = 500 and priv_cols = 13: obs_cols at least 1, priv_cols at least 0 and at most 512 together are taken"},
      {5, -1, 3, 1, {32}, 1, {32}, "obs_cols = 5 and priv_cols = -1: obs_cols at least 1, priv_cols at least 0 and at most 512 together are taken"},
      {2147483647, 2147483647, 3, 1, {32}, 1, {32},
       "obs_cols = 2147483647 and priv_cols = 2147483647: obs_cols at least 1, priv_cols at least 0 and at most 512 together are taken"},
      {5, 2, 0, 1, {32}, 1, {32}, "act_cols = 0, 1 .. GMR_LOSS_MAX_ACT = 32 are taken"},
      {5, 2, 33, 1, {32}, 1, {32}, "act_cols = 33, 1 .. GMR_LOSS_MAX_ACT = 32 are taken"},
      {5, 2, 3, 0, {32}, 1, {32}, "actor: 0 hidden layers, 1 .. 4 are taken"},
      {5, 2, 3, 5, {32, 32, 32, 32, 32}, 1, {32}, "actor: 5 hidden layers, 1 .. 4 are taken"},
      {5, 2, 3, 1, {32}, 5, {32, 32, 32, 32, 32}, "critic: 5 hidden layers, 1 .. 4 are taken"},
      {5, 2, 3, 2, {256, 100}, 1, {32}, "actor: hidden[1] = 100, a multiple of 32 in 32 .. 256 is needed"},
      {5, 2, 3, 1, {0}, 1, {32}, "actor: hidden[0] = 0, a multiple of 32 in 32 .. 256 is needed"},
      {5, 2, 3, 1, {32}, 3, {64, 64, 288}, "critic: hidden[2] = 288, a multiple of 32 in 32 .. 256 is needed"},
      {5, 2, 3, 1, {-32}, 1, {32}, "actor: hidden[0] = -32, a multiple of 32 in 32 .. 256 is needed"},
  };
  for (const Refusal& r : cases) {
    gmr::PolicyShape a, c;
    g_calls = 0;
    g_message[0] = 0;
    const int rc = gmr::policy_plan(r.O, r.P, r.A, r.na, r.ah, r.nc, r.ch, &a, &c);
    CHECK(rc == GMR_ERR_ARG && g_calls == 1 && std::strcmp(g_message, r.message) == 0, "\"%s\" instead of \"%s\"", g_message, r.message);
  }
  gmr::PolicyShape a, c;
  const int one[1] = {32};
  CHECK(gmr::policy_plan(5, 2, 3, 1, nullptr, 1, one, &a, &c) == GMR_ERR_ARG && std::strcmp(g_message, "actor: null hidden widths") == 0, "%s", g_message);
  return 0;
}

int main() {
  if (check_plans() || check_refusals()) return 1;
  std::printf("ok\n");
  return 0;
}
