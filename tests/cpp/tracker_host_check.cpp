// The host helpers of the motion tracker's entry points (csrc/gmr_tracker_host.h) driven on the CPU (plain C++, no HIP), with a gmr_fail
// of its own that records the message:
//   * noise_spec: for every kind of spec the struct the kernels read, and for every refusal the return code, the whole message under
//     the caller's name and the struct it leaves;
//   * subset_check: the range of n, and for every phrase an entry point passes the whole message of a missing list with n != N;
//     a null phrase checks the range alone;
//   * aligned16 and the two grid sizes at their edges.
// Prints "ok"; exit code 0 = all good.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../../general_motion_retargeting_amd/csrc/gmr_tracker_host.h"

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

static void forget() {
  g_message[0] = 0;
  g_calls = 0;
}

struct SpecCase {
  const char* name;
  gmr_proprio_noise_t in;
  int rc;
  gmr::ProprioNoise want;      // a refusal before the struct is filled leaves "no noise"
  const char* message;         // after a refusal
};

static int check_noise_spec() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const gmr::ProprioNoise none{};
  const SpecCase cases[] = {
      // accepted: none (operation and range are not looked at), gaussian (mu, sigma), uniform (lower, upper - lower), either operation
      {"kick_lin_vel", {GMR_NOISE_NONE, 7, nan, -inf}, GMR_OK, none, ""},
      {"noise[2]", {GMR_NOISE_GAUSSIAN, GMR_NOISE_ADDITIVE, 0.25, 0.5}, GMR_OK, {GMR_NOISE_GAUSSIAN, GMR_NOISE_ADDITIVE, 0.25f, 0.5f}, ""},
      {"noise[0]", {GMR_NOISE_GAUSSIAN, GMR_NOISE_SCALING, 1.0, 0.0}, GMR_OK, {GMR_NOISE_GAUSSIAN, GMR_NOISE_SCALING, 1.0f, 0.0f}, ""},
      {"push_force", {GMR_NOISE_UNIFORM, GMR_NOISE_ADDITIVE, -1.5, 2.5}, GMR_OK, {GMR_NOISE_UNIFORM, GMR_NOISE_ADDITIVE, -1.5f, 4.0f}, ""},
      {"init_dof_pos", {GMR_NOISE_UNIFORM, GMR_NOISE_SCALING, 0.9, 1.1}, GMR_OK, {GMR_NOISE_UNIFORM, GMR_NOISE_SCALING, 0.9f, (float)(1.1 - 0.9)}, ""},
      // (the span is formed in double and rounded once: not (float)1.1 - (float)0.9)
      {"init_base_pos_xy", {GMR_NOISE_UNIFORM, GMR_NOISE_ADDITIVE, 2.0, 1.0}, GMR_OK, {GMR_NOISE_UNIFORM, GMR_NOISE_ADDITIVE, 2.0f, -1.0f}, ""},
      // refused
      {"noise[5]", {GMR_NOISE_GAUSSIAN, GMR_NOISE_ADDITIVE, 0.0, -0.5}, GMR_ERR_ARG, none, "noise[5]: a gaussian's deviation -0.5 is negative"},
      {"kick_ang_vel", {GMR_NOISE_UNIFORM, GMR_NOISE_ADDITIVE, 0.0, inf}, GMR_ERR_ARG, none, "kick_ang_vel: range (0, inf) is not finite"},
      {"push_torque", {GMR_NOISE_GAUSSIAN, GMR_NOISE_SCALING, nan, 1.0}, GMR_ERR_ARG, none, "push_torque: range (nan, 1) is not finite"},
      {"noise[1]", {GMR_NOISE_UNIFORM, GMR_NOISE_ADDITIVE, 0.0, 1e39}, GMR_ERR_ARG, none, "noise[1]: range (0, 1e+39) is not finite"},      // finite, not as a float32
      // each bound fits, the span does not: the one refusal that comes after the struct is filled (no caller keeps it after an error)
      {"init_base_lin_vel_xy", {GMR_NOISE_UNIFORM, GMR_NOISE_ADDITIVE, -3e38, 3e38}, GMR_ERR_ARG, {GMR_NOISE_UNIFORM, GMR_NOISE_ADDITIVE, -3e38f, (float)inf},
       "init_base_lin_vel_xy: range (-3e+38, 3e+38) is too wide"},
      {"noise[3]", {3, GMR_NOISE_ADDITIVE, 0.0, 1.0}, GMR_ERR_ARG, none, "noise[3]: distribution = 3"},
      {"noise[4]", {-1, GMR_NOISE_ADDITIVE, 0.0, 1.0}, GMR_ERR_ARG, none, "noise[4]: distribution = -1"},
      {"push_force", {GMR_NOISE_UNIFORM, 2, 0.0, 1.0}, GMR_ERR_ARG, none, "push_force: operation = 2"},
      {"push_force", {GMR_NOISE_GAUSSIAN, -1, 0.0, 1.0}, GMR_ERR_ARG, none, "push_force: operation = -1"},
  };
  int k = 0;
  for (const SpecCase& c : cases) {
    forget();
    gmr::ProprioNoise got{9, 9, 9.0f, 9.0f};
    const int rc = gmr::noise_spec(c.in, c.name, &got);
    CHECK(rc == c.rc, "case %d (%s): returned %d, \"%s\"", k, c.name, rc, g_message);
    CHECK(g_calls == (c.rc == GMR_OK ? 0 : 1), "case %d: %d messages", k, g_calls);
    CHECK(!std::strcmp(g_message, c.message), "case %d: \"%s\", not \"%s\"", k, g_message, c.message);
    CHECK(got.dist == c.want.dist && got.op == c.want.op && got.a == c.want.a && got.m == c.want.m,
          "case %d (%s): (%d, %d, %a, %a), not (%d, %d, %a, %a)", k, c.name, got.dist, got.op, got.a, got.m, c.want.dist, c.want.op, c.want.a, c.want.m);
    k++;
  }
  CHECK((float)(1.1 - 0.9) != 1.1f - 0.9f, "the span case does not tell the two roundings apart");
  CHECK(gmr::fits(3.4e38) && !gmr::fits(3.5e38) && !gmr::fits(inf) && !gmr::fits(nan) && gmr::fits(-1e-300), "fits");
  return 0;
}

static int check_subset() {
  // every phrase an entry point passes: assign, reset_done, set_anchor, anchor_to_root, hold, proprio_reset, reset_states
  const char* const phrases[] = {"every environment is assigned",
                                 "the masks cover every environment",
                                 "every environment is set",
                                 "the mask and the roots cover every environment",
                                 "the mask and dof_pos cover every environment",
                                 "the mask and root_states cover every environment",
                                 "the mask and the init rows cover every environment"};
  const int ids[3] = {0, 1, 2};
  for (const char* phrase : phrases) {
    forget();
    CHECK(gmr::subset_check(5, 5, nullptr, phrase) == GMR_OK && gmr::subset_check(5, 3, ids, phrase) == GMR_OK && gmr::subset_check(5, 0, ids, phrase) == GMR_OK &&
              gmr::subset_check(5, 9, ids, phrase) == GMR_OK && gmr::subset_check(1 << 26, 1 << 26, nullptr, phrase) == GMR_OK && g_calls == 0,
          "\"%s\": a good list was refused: \"%s\"", phrase, g_message);
    CHECK(gmr::subset_check(5, 3, nullptr, phrase) == GMR_ERR_ARG, "\"%s\": n = 3 without a list over N = 5", phrase);
    const std::string want = std::string("without env_ids ") + phrase + ": n = 3, N = 5";
    CHECK(want == g_message, "\"%s\", not \"%s\"", g_message, want.c_str());
    CHECK(gmr::subset_check(5, 0, nullptr, phrase) == GMR_ERR_ARG && std::string(g_message) == std::string("without env_ids ") + phrase + ": n = 0, N = 5",
          "\"%s\"", g_message);
    // the range comes first, with or without a list
    CHECK(gmr::subset_check(5, -1, nullptr, phrase) == GMR_ERR_ARG && !std::strcmp(g_message, "n = -1 out of range"), "\"%s\"", g_message);
    CHECK(gmr::subset_check(5, (1 << 26) + 1, ids, phrase) == GMR_ERR_ARG && !std::strcmp(g_message, "n = 67108865 out of range"), "\"%s\"", g_message);
  }
  // reset and reset_dev have a rule of their own for a missing list: the range alone
  forget();
  CHECK(gmr::subset_check(5, 3, nullptr, nullptr) == GMR_OK && gmr::subset_check(5, 0, nullptr, nullptr) == GMR_OK && gmr::subset_check(5, 1 << 26, ids, nullptr) == GMR_OK &&
            g_calls == 0, "the range half refused \"%s\"", g_message);
  CHECK(gmr::subset_check(5, -7, ids, nullptr) == GMR_ERR_ARG && !std::strcmp(g_message, "n = -7 out of range"), "\"%s\"", g_message);
  return 0;
}

static int check_small() {
  alignas(16) char buf[32];
  CHECK(gmr::aligned16(buf) && gmr::aligned16(buf + 16) && !gmr::aligned16(buf + 4) && !gmr::aligned16(buf + 15) && gmr::aligned16(nullptr), "aligned16");
  CHECK(gmr::lane_blocks(0) == 0 && gmr::lane_blocks(1) == 1 && gmr::lane_blocks(256) == 1 && gmr::lane_blocks(257) == 2, "lane_blocks");
  CHECK(gmr::lane_blocks((1ll << 26) * 16) == (1u << 22) && gmr::lane_blocks((1ll << 31) + 1) == (1u << 23) + 1, "lane_blocks beyond 32 bits");
  CHECK(gmr::row_blocks(0, 16) == 0 && gmr::row_blocks(1, 16) == 1 && gmr::row_blocks(16, 16) == 1 && gmr::row_blocks(17, 16) == 2 &&
            gmr::row_blocks(1 << 26, 16) == (1u << 22), "row_blocks");
  return 0;
}

int main() {
  if (check_noise_spec() || check_subset() || check_small()) return 1;
  std::printf("ok\n");
  return 0;
}
