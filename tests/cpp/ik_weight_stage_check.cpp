// The per-frame body weights of an IK job (csrc/gmr_ik_weight_stage.h) driven on the CPU with literal values (plain C++, no HIP),
// for a job with the array and for one without:
//   * the carve: 8 nhuman bytes per frame on a 256-byte boundary IN FRONT of the job's own arrays, so that [0, out_begin) of a
//     workspace is all input; without the array no byte, a null device pointer, and the job's offsets as without the feature;
//   * the slice copies and the strided window copies, applied with memcpy between a vector of distinct bytes and a "device"
//     block: every weight byte of every stream arrives exactly once, equals the host array, and no descriptor leaves the
//     host array or the field.
// Prints "ok"; exit code 0 = all good.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../general_motion_retargeting_amd/csrc/gmr_ik_weight_stage.h"

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "CHECK failed (line %d): %s : ", __LINE__, #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

using namespace gmr;
static const size_t NQ = 36, NH = 14;

static std::vector<unsigned char> host_weights(size_t S, size_t T, unsigned char salt) {
  std::vector<unsigned char> w(S * T * NH * 8);
  for (size_t i = 0; i < w.size(); i++) w[i] = (unsigned char)(i * 29 + salt);
  return w;
}

// applies a descriptor with memcpy after checking that it stays inside the host array and inside the field; counts the bytes
static int apply(const IkCopy& c, const std::vector<unsigned char>& host, const IkWeightOff& o, std::vector<unsigned char>& dev, std::vector<int>& hits) {
  CHECK(c.field == IK_WEIGHT, "a weight copy names field %d", c.field);
  CHECK(c.rows >= 1 && c.width > 0, "an empty descriptor");
  CHECK(c.rows == 1 || c.pitch >= c.width, "pitch %zu under width %zu", c.pitch, c.width);
  const size_t span = (c.rows - 1) * c.pitch + c.width, field_bytes = o.S * o.stride();
  CHECK(c.host + span <= host.size(), "host bytes [%zu, %zu) of %zu", c.host, c.host + span, host.size());
  CHECK(c.dev >= o.at && c.dev + span <= o.at + field_bytes && c.dev + span <= dev.size(), "device bytes [%zu, %zu) outside the field at %zu of %zu", c.dev,
        c.dev + span, o.at, field_bytes);
  for (size_t r = 0; r < c.rows; r++) {
    memcpy(dev.data() + c.dev + r * c.pitch, host.data() + c.host + r * c.pitch, c.width);
    for (size_t i = 0; i < c.width; i++) hits[c.dev + r * c.pitch + i]++;
  }
  return 0;
}

static gmr_job_t some_job(int S, int T) {
  gmr_job_t J;
  memset(&J, 0, sizeof J);
  J.S = S; J.T = T;
  for (int f = 0; f < IK_NFIELD; f++) ik_set_ptr(J, f, &J);      // (any non-null pointer: every array counts as present)
  return J;
}

static int check_carve() {
  const gmr_job_t J = some_job(3, 5);
  const std::vector<unsigned char> w = host_weights(3, 5, 1);
  Carve plain;
  const IkJobOff p = ik_carve_job(plain, J, NQ, NH, 3);
  {
    Carve c;
    const IkWeightOff wo = ik_carve_weight(c, reinterpret_cast<const double*>(w.data()), NH, 3, 5);
    const IkJobOff o = ik_carve_job(c, J, NQ, NH, 3);
    CHECK(wo.row == 8 * NH && wo.stride() == 5 * 8 * NH && wo.at == 0 && wo.S == 3 && wo.T == 5, "row %zu, stride %zu at %zu", wo.row, wo.stride(), wo.at);
    CHECK(o.at[IK_Q0] == (3 * 5 * 8 * NH + 255) / 256 * 256 && o.at[IK_Q0] % 256 == 0, "the job starts at %zu", o.at[IK_Q0]);
    for (int f = 0; f < IK_NFIELD; f++) CHECK(o.at[f] == p.at[f] + o.at[IK_Q0] && o.row[f] == p.row[f], "field %d moved by something else than the weights", f);
    CHECK(wo.at + wo.S * wo.stride() <= o.out_begin() && o.end == c.total(), "the weights lie in front of the outputs");
    std::vector<char> block(o.end);
    CHECK(ik_weight_at(block.data(), wo) == reinterpret_cast<const double*>(block.data() + wo.at), "the device pointer");
  }
  {
    Carve c;
    const IkWeightOff wo = ik_carve_weight(c, nullptr, NH, 3, 5);
    const IkJobOff o = ik_carve_job(c, J, NQ, NH, 3);
    CHECK(wo.row == 0 && wo.stride() == 0 && c.total() == plain.total() && o.end == p.end, "a job without weights takes no byte for them");
    for (int f = 0; f < IK_NFIELD; f++) CHECK(o.at[f] == p.at[f], "field %d of a job without weights moved", f);
    std::vector<char> block(o.end + 1);
    IkCopy cp;
    CHECK(ik_weight_at(block.data(), wo) == nullptr, "a job without weights got a device pointer");
    CHECK(ik_weight_slice_copy(wo, 0, &cp) == 0 && ik_weight_window_copy(wo, 0, 4, &cp) == 0, "a job without weights has no copies");
  }
  return 0;
}

static int check_slices() {
  const int cases[][2] = {{7, 3}, {1, 1}, {5, 5}, {2, 3}};
  for (const auto& cs : cases) {
    const int S = cs[0], n = cs[1], T = 5;
    const gmr_job_t J = some_job(S, T);
    const std::vector<unsigned char> w = host_weights(S, T, 3);
    std::vector<unsigned char> seen(w.size(), 0);
    for (int k = 0; k < n; k++) {
      int s0, cnt;
      ik_slice_range(S, k, n, &s0, &cnt);
      Carve cv;
      const IkWeightOff wo = ik_carve_weight(cv, reinterpret_cast<const double*>(w.data()), NH, (size_t)cnt, (size_t)T);
      const IkJobOff o = ik_carve_job(cv, J, NQ, NH, (size_t)cnt);
      std::vector<unsigned char> dev(o.end, 0xCD);
      std::vector<int> hits(o.end, 0);
      IkCopy c;
      const int nc = ik_weight_slice_copy(wo, (size_t)s0, &c);
      CHECK(nc == (cnt ? 1 : 0), "(%d, %d): slice %d has %d copies", S, n, k, nc);
      if (!nc) continue;
      CHECK(c.rows == 1, "a slice is one plain piece");
      if (apply(c, w, wo, dev, hits)) return 1;
      const size_t bytes = (size_t)cnt * wo.stride();
      for (size_t i = 0; i < o.end; i++) CHECK(hits[i] == (i >= wo.at && i < wo.at + bytes ? 1 : 0), "(%d, %d): device byte %zu written %d times", S, n, i, hits[i]);
      CHECK(memcmp(dev.data() + wo.at, w.data() + (size_t)s0 * wo.stride(), bytes) == 0, "(%d, %d): slice %d holds other bytes", S, n, k);
      for (size_t i = 0; i < bytes; i++) seen[(size_t)s0 * wo.stride() + i]++;
    }
    for (size_t i = 0; i < seen.size(); i++) CHECK(seen[i] == 1, "(%d, %d): host byte %zu went up %d times", S, n, i, seen[i]);
  }
  return 0;
}

static int check_windows() {
  const int S[2] = {3, 2}, T[2] = {10, 6}, maxT = 10, wl = 4;
  const gmr_job_t J[2] = {some_job(S[0], T[0]), some_job(S[1], T[1])};
  const std::vector<unsigned char> w0 = host_weights(S[0], T[0], 5);
  const unsigned char* hw[2] = {w0.data(), nullptr};      // job 1 carries no weights
  Carve cv;
  IkWeightOff wo[2];
  IkJobOff off[2];
  for (int j = 0; j < 2; j++) {
    wo[j] = ik_carve_weight(cv, reinterpret_cast<const double*>(hw[j]), NH, (size_t)S[j], (size_t)T[j]);
    off[j] = ik_carve_job(cv, J[j], NQ, NH, (size_t)S[j]);
  }
  std::vector<unsigned char> dev(cv.total(), 0xCD);
  std::vector<int> hits(cv.total(), 0);
  int nwin = 0;
  for (int tb = 0; tb < maxT; tb += wl, nwin++) {
    const int te = tb + wl < maxT ? tb + wl : maxT;
    for (int j = 0; j < 2; j++) {
      IkCopy c;
      const int n = ik_weight_window_copy(wo[j], (size_t)tb, (size_t)te, &c);
      CHECK(n == (j == 0 ? 1 : 0), "job %d, window %d: %d copies", j, nwin, n);
      if (!n) continue;
      const size_t row = 8 * NH, frames = (size_t)((te < T[j] ? te : T[j]) - tb);
      CHECK(c.pitch == (size_t)T[j] * row && c.width == frames * row && c.rows == (size_t)S[j] && c.host == (size_t)tb * row, "the window of the weights");
      if (apply(c, w0, wo[j], dev, hits)) return 1;
    }
  }
  CHECK(nwin == 3, "%d windows", nwin);
  IkCopy c;
  CHECK(ik_weight_window_copy(wo[0], 10, 14, &c) == 0, "a window behind the last frame has no copy");
  const size_t bytes = wo[0].S * wo[0].stride();
  for (size_t i = 0; i < dev.size(); i++) CHECK(hits[i] == (i >= wo[0].at && i < wo[0].at + bytes ? 1 : 0), "device byte %zu written %d times", i, hits[i]);
  CHECK(memcmp(dev.data() + wo[0].at, w0.data(), bytes) == 0, "the windows together hold other bytes than the array");
  CHECK(wo[1].row == 0 && off[1].at[IK_Q0] == off[0].end, "the job without weights follows the first job directly");
  return 0;
}

int main() {
  if (check_carve() || check_slices() || check_windows()) return 1;
  std::printf("ok\n");
  return 0;
}
