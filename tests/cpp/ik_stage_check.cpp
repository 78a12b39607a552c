// The arrays of an IK job (csrc/gmr_ik_stage.h) driven on the CPU with literal values (plain C++, no HIP):
//   * the bytes and offsets of the nine arrays, with every optional array present, each one absent, and all absent;
//   * the copy descriptors of slices and of windows, applied with memcpy between vectors of distinct bytes and a malloc'd
//     "device" block around a host-loop kernel: every output byte arrives exactly once and equals an unsliced pass, no
//     descriptor leaves its host array or its device field;
//   * the integer rules that cut a batch, and the launch-shape predicate.
// Prints "ok"; exit code 0 = all good.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../general_motion_retargeting_amd/csrc/gmr_ik_stage.h"

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "CHECK failed (line %d): %s : ", __LINE__, #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

using namespace gmr;
static const size_t NQ = 36, NH = 14;

// the host arrays of one job as byte vectors, and how often a copy wrote each output byte
struct HostJob {
  std::vector<unsigned char> a[IK_NFIELD];
  std::vector<int> hits[IK_NFIELD];
  gmr_job_t J;
  HostJob(int S, int T, unsigned absent_mask, unsigned char salt) {
    memset(&J, 0, sizeof J);
    J.S = S; J.T = T;
    Carve c;
    gmr_job_t all = J;
    for (int f = 0; f < IK_NFIELD; f++) ik_set_ptr(all, f, &all);      // (any non-null pointer: every array counts as present)
    const IkJobOff o = ik_carve_job(c, all, NQ, NH, (size_t)S);
    for (int f = 0; f < IK_NFIELD; f++) {
      if (absent_mask & (1u << f)) continue;
      a[f].resize((size_t)S * o.stride(f));
      hits[f].assign(a[f].size(), 0);
      for (size_t i = 0; i < a[f].size(); i++) a[f][i] = kIkFields[f].out ? 0xEE : (unsigned char)(i * 31 + f * 17 + salt);
      ik_set_ptr(J, f, a[f].data());
    }
  }
};

// Applies a descriptor with memcpy, after checking that it stays inside the host array and inside its device field.
static int apply(const IkCopy& c, HostJob& h, const IkJobOff& o, unsigned char* dev, size_t dev_bytes) {
  const bool out = kIkFields[c.field].out;
  const size_t field_bytes = o.S * o.stride(c.field);
  CHECK(c.rows >= 1 && c.width > 0, "an empty descriptor for field %d", c.field);
  CHECK(c.rows == 1 || c.pitch >= c.width, "pitch %zu under width %zu", c.pitch, c.width);
  const size_t span = (c.rows - 1) * c.pitch + c.width;
  CHECK(c.host + span <= h.a[c.field].size(), "field %d: host bytes [%zu, %zu) of %zu", c.field, c.host, c.host + span, h.a[c.field].size());
  CHECK(c.dev >= o.at[c.field] && c.dev + span <= o.at[c.field] + field_bytes && c.dev + span <= dev_bytes, "field %d: device bytes [%zu, %zu) outside the field at %zu of %zu",
        c.field, c.dev, c.dev + span, o.at[c.field], field_bytes);
  for (size_t r = 0; r < c.rows; r++) {
    unsigned char *hp = h.a[c.field].data() + c.host + r * c.pitch, *dp = dev + c.dev + r * c.pitch;
    if (out) { memcpy(hp, dp, c.width); for (size_t i = 0; i < c.width; i++) h.hits[c.field][c.host + r * c.pitch + i]++; }
    else memcpy(dp, hp, c.width);
  }
  return 0;
}

// The host-loop kernel over the device job D: frames [tb, te) of each of its streams; stream s of D is stream g0 + s of the job.
// Every output byte is a known function of the input bytes and of the stream's global index.
static void kernel(const gmr_job_t& D, size_t g0, size_t tb, size_t te) {
  const size_t T = (size_t)D.T;
  const unsigned char *q0 = (const unsigned char*)D.q0, *hu = (const unsigned char*)D.human, *len = (const unsigned char*)D.len, *sc = (const unsigned char*)D.scale;
  for (size_t s = 0; s < (size_t)D.S; s++) {
    const unsigned char mix = (unsigned char)((g0 + s) * 5 + (len ? len[s * 4] : 1) + (sc ? sc[s * NH * 8 + 3] : 2));
    for (size_t t = tb; t < te && t < T; t++) {
      const unsigned char in = (unsigned char)(hu[(s * T + t) * NH * 56 + 9] + q0[s * NQ * 8 + 1] + mix);
      for (size_t i = 0; i < NQ * 8; i++) ((unsigned char*)D.q_out)[(s * T + t) * NQ * 8 + i] = (unsigned char)(in + i);
      for (size_t i = 0; i < 8; i++) ((unsigned char*)D.nsolve)[(s * T + t) * 8 + i] = (unsigned char)(in ^ i);
      for (size_t i = 0; D.tgt_out && i < NH * 56; i++) ((unsigned char*)D.tgt_out)[(s * T + t) * NH * 56 + i] = (unsigned char)(in * 3 + i);
      for (size_t i = 0; D.err_out && i < 16; i++) ((unsigned char*)D.err_out)[(s * T + t) * 16 + i] = (unsigned char)(in + 7 * i);
    }
    if (te >= T) for (size_t i = 0; i < 4; i++) ((unsigned char*)D.status)[s * 4 + i] = (unsigned char)(mix + i);
  }
}

// every output byte written exactly once, and equal to what one unsliced pass over the host arrays gives
static int check_outputs(HostJob& h, const char* what) {
  HostJob ref(h.J.S, h.J.T, 0, 0);
  for (int f = 0; f < IK_NFIELD; f++) {
    if (h.a[f].empty()) { ik_set_ptr(ref.J, f, nullptr); continue; }
    if (!kIkFields[f].out) memcpy(ref.a[f].data(), h.a[f].data(), h.a[f].size());      // (in place: ref.J points at the storage)
  }
  kernel(ref.J, 0, 0, (size_t)h.J.T);
  for (int f = 0; f < IK_NFIELD; f++) {
    if (!kIkFields[f].out || h.a[f].empty()) continue;
    for (size_t i = 0; i < h.a[f].size(); i++) {
      CHECK(h.hits[f][i] == 1, "%s: byte %zu of field %d was copied back %d times", what, i, f, h.hits[f][i]);
      CHECK(h.a[f][i] == ref.a[f][i], "%s: byte %zu of field %d is %u, one pass gives %u", what, i, f, h.a[f][i], ref.a[f][i]);
    }
  }
  return 0;
}

static int check_layout() {
  const size_t want[IK_NFIELD] = {864, 11760, 12, 336, 4320, 120, 12, 11760, 240};
  const unsigned optional[] = {1u << IK_LEN, 1u << IK_SCALE, 1u << IK_TGT_OUT, 1u << IK_ERR_OUT};
  const unsigned masks[] = {0, optional[0], optional[1], optional[2], optional[3], optional[0] | optional[1] | optional[2] | optional[3]};
  for (unsigned mask : masks) {
    HostJob h(3, 5, mask, 1);
    Carve c;
    const IkJobOff o = ik_carve_job(c, h.J, NQ, NH, 3);
    size_t prev_end = 0, out_bytes = 0;
    for (int f = 0; f < IK_NFIELD; f++) {
      const size_t bytes = o.S * o.stride(f);
      CHECK(bytes == ((mask >> f) & 1u ? 0 : want[f]), "mask %x: field %d has %zu bytes", mask, f, bytes);
      CHECK(o.at[f] % 256 == 0 && o.at[f] >= prev_end && (prev_end == 0 || o.at[f] - prev_end < 256), "mask %x: field %d at %zu, the one before ends at %zu", mask, f, o.at[f], prev_end);
      if (bytes) prev_end = o.at[f] + bytes;
      if (f >= IK_Q_OUT) out_bytes += (bytes + 255) / 256 * 256;
    }
    CHECK(o.end == c.total() && o.end % 256 == 0 && o.end >= prev_end && o.end - prev_end < 256, "mask %x: end %zu after %zu", mask, o.end, prev_end);
    CHECK(o.out_begin() == o.at[IK_Q_OUT] && o.end - o.out_begin() == out_bytes, "mask %x: [q_out, end) holds %zu bytes, the outputs present %zu", mask, o.end - o.out_begin(), out_bytes);
    std::vector<char> block(o.end + 1);
    const gmr_job_t D = ik_job_at(h.J, block.data(), o);
    for (int f = 0; f < IK_NFIELD; f++) {
      if ((mask >> f) & 1u) CHECK(ik_ptr(D, f) == nullptr, "mask %x: the absent field %d got a device pointer", mask, f);
      else CHECK(ik_ptr(D, f) == block.data() + o.at[f], "mask %x: field %d points elsewhere", mask, f);
    }
    CHECK(D.S == 3 && D.T == 5 && D.solver == h.J.solver, "the rest of the job is kept");
  }
  for (int f = 0; f < IK_NFIELD; f++)
    CHECK(kIkFields[f].out == (f >= IK_Q_OUT) && kIkFields[f].optional == (f == IK_LEN || f == IK_SCALE || f == IK_TGT_OUT || f == IK_ERR_OUT), "table row %d", f);
  return 0;
}

static int check_slices() {
  const int cases[][2] = {{7, 3}, {1, 1}, {5, 5}, {2, 3}};
  for (const auto& cs : cases) {
    const int S = cs[0], n = cs[1], T = 5;
    HostJob h(S, T, 0, 3);
    int next = 0, empty = 0;
    IkCopy c[IK_NFIELD];
    for (int k = 0; k < n; k++) {
      int s0, cnt;
      ik_slice_range(S, k, n, &s0, &cnt);
      CHECK(s0 == next && cnt >= 0, "(%d, %d): slice %d starts at %d after %d", S, n, k, s0, next);
      next = s0 + cnt;
      if (cnt == 0) { empty++; continue; }
      Carve cv;
      const IkJobOff o = ik_carve_job(cv, h.J, NQ, NH, (size_t)cnt);
      std::vector<unsigned char> dev(o.end, 0xCD);
      const int ni = ik_slice_copies(o, false, (size_t)s0, c);
      CHECK(ni == 4, "(%d, %d): %d input copies", S, n, ni);
      for (int i = 0; i < ni; i++) { CHECK(c[i].rows == 1 && !kIkFields[c[i].field].out, "an input copy"); if (apply(c[i], h, o, dev.data(), dev.size())) return 1; }
      gmr_job_t D = h.J;
      D.S = cnt;
      D = ik_job_at(D, (char*)dev.data(), o);
      kernel(D, (size_t)s0, 0, (size_t)T);
      const int no = ik_slice_copies(o, true, (size_t)s0, c);
      CHECK(no == 5, "(%d, %d): %d output copies", S, n, no);
      for (int i = 0; i < no; i++) { CHECK(c[i].rows == 1 && kIkFields[c[i].field].out, "an output copy"); if (apply(c[i], h, o, dev.data(), dev.size())) return 1; }
    }
    CHECK(next == S, "(%d, %d): the slices end at %d", S, n, next);
    CHECK(empty == (S == 2 && n == 3 ? 1 : 0), "(%d, %d): %d empty slices", S, n, empty);
    if (check_outputs(h, "slices")) return 1;
  }
  return 0;
}

static int check_windows() {
  HostJob jobs[2] = {HostJob(3, 10, 0, 5), HostJob(2, 6, (1u << IK_SCALE) | (1u << IK_ERR_OUT), 9)};
  const int maxT = 10, wl = 4;
  Carve cv;
  IkJobOff off[2];
  for (int j = 0; j < 2; j++) off[j] = ik_carve_job(cv, jobs[j].J, NQ, NH, (size_t)jobs[j].J.S);
  std::vector<unsigned char> dev(cv.total(), 0xCD);
  gmr_job_t D[2];
  IkCopy c[IK_NFIELD];
  int per_stream_in = 0, per_stream_out = 0;
  for (int j = 0; j < 2; j++) {
    const int n = ik_slice_copies(off[j], false, 0, c, IK_PER_STREAM);
    CHECK(n == (j == 0 ? 3 : 2), "job %d: %d per-stream inputs", j, n);
    for (int i = 0; i < n; i++) { CHECK(!kIkFields[c[i].field].per_frame, "a per-stream array"); per_stream_in++; if (apply(c[i], jobs[j], off[j], dev.data(), dev.size())) return 1; }
    D[j] = ik_job_at(jobs[j].J, (char*)dev.data(), off[j]);
  }
  int nwin = 0;
  for (int tb = 0; tb < maxT; tb += wl, nwin++) {
    const int te = tb + wl < maxT ? tb + wl : maxT;
    CHECK((nwin == 0 && tb == 0 && te == 4) || (nwin == 1 && tb == 4 && te == 8) || (nwin == 2 && tb == 8 && te == 10), "window %d is [%d, %d)", nwin, tb, te);
    for (int j = 0; j < 2; j++) {
      const int n = ik_window_copies(off[j], false, (size_t)tb, (size_t)te, c);
      CHECK(n == (tb < jobs[j].J.T ? 1 : 0), "job %d, window %d: %d input copies", j, nwin, n);
      for (int i = 0; i < n; i++) {
        const size_t row = NH * 56, frames = (size_t)((te < jobs[j].J.T ? te : jobs[j].J.T) - tb);
        CHECK(c[i].field == IK_HUMAN && c[i].pitch == (size_t)jobs[j].J.T * row && c[i].width == frames * row && c[i].rows == (size_t)jobs[j].J.S, "the window of the human frames");
        if (apply(c[i], jobs[j], off[j], dev.data(), dev.size())) return 1;
      }
    }
    for (int j = 0; j < 2; j++) if (tb < jobs[j].J.T) kernel(D[j], 0, (size_t)tb, (size_t)te);
    for (int j = 0; j < 2; j++) {
      const int n = ik_window_copies(off[j], true, (size_t)tb, (size_t)te, c);
      CHECK(n == (tb >= jobs[j].J.T ? 0 : j == 0 ? 4 : 3), "job %d, window %d: %d output copies", j, nwin, n);
      for (int i = 0; i < n; i++) { CHECK(kIkFields[c[i].field].per_frame, "a per-frame array"); if (apply(c[i], jobs[j], off[j], dev.data(), dev.size())) return 1; }
    }
  }
  CHECK(nwin == 3, "%d windows", nwin);
  for (int j = 0; j < 2; j++) {
    const int n = ik_slice_copies(off[j], true, 0, c, IK_PER_STREAM);
    CHECK(n == 1 && c[0].field == IK_STATUS, "job %d: status comes back once", j);
    per_stream_out++;
    if (apply(c[0], jobs[j], off[j], dev.data(), dev.size())) return 1;
  }
  CHECK(per_stream_in == 5 && per_stream_out == 2, "per-stream arrays move exactly once");
  for (int j = 0; j < 2; j++) if (check_outputs(jobs[j], j == 0 ? "windows, job 0" : "windows, job 1")) return 1;
  return 0;
}

static int check_rules() {
  CHECK(ik_window_frames(4, 8) == 4 && ik_window_frames(300, 3) == 100 && ik_window_frames(33, 2) == 20, "window frames: %d %d %d", ik_window_frames(4, 8), ik_window_frames(300, 3), ik_window_frames(33, 2));
  CHECK(ik_slice_count(0, 8640, (size_t)200 << 20) == 2, "8640 streams, 200 MiB: %d", ik_slice_count(0, 8640, (size_t)200 << 20));
  CHECK(ik_slice_count(0, 4095, (size_t)200 << 20) == 1, "4095 streams: %d", ik_slice_count(0, 4095, (size_t)200 << 20));
  CHECK(ik_slice_count(0, 1000000, (size_t)4 << 30) == 16, "10^6 streams, 4 GiB: %d", ik_slice_count(0, 1000000, (size_t)4 << 30));
  CHECK(ik_slice_count(5, 3, 0) == 3 && ik_slice_count(-2, 100000, (size_t)4 << 30) == 1, "the caller's choice");
  CHECK(ik_cut_in_time(-2, 1, 4, 0) && !ik_cut_in_time(-2, 1, 3, 0), "windows on request need 4 frames");
  CHECK(ik_cut_in_time(0, 1, 32, (size_t)64 << 20) && !ik_cut_in_time(0, 2, 32, (size_t)64 << 20) && !ik_cut_in_time(0, 1, 31, (size_t)64 << 20) &&
        !ik_cut_in_time(0, 1, 32, ((size_t)64 << 20) - 1) && !ik_cut_in_time(3, 1, 320, (size_t)1 << 30), "automatic windows");
  CHECK(ik_helpers_shape(true, 0, 300) && !ik_helpers_shape(true, 0, 301), "automatic: helpers up to 300 streams");
  CHECK(!ik_helpers_shape(true, 1, 300) && !ik_helpers_shape(true, 1, 301), "forced to one wavefront");
  CHECK(ik_helpers_shape(true, 4, 300) && ik_helpers_shape(true, 4, 301), "forced to four");
  for (int force : {0, 1, 4}) CHECK(!ik_helpers_shape(false, force, 300) && !ik_helpers_shape(false, force, 301), "a robot that does not decompose never gets helpers");
  CHECK(ik_throughput_shape(true, 0, 301, true) && !ik_throughput_shape(true, 0, 300, true) && !ik_throughput_shape(true, 0, 301, false) &&
        ik_throughput_shape(false, 4, 300, true) && ik_throughput_shape(true, 1, 300, true) && !ik_throughput_shape(true, 4, 301, true), "throughput shape: not helpers, and the robot fits");
  return 0;
}

int main() {
  if (check_layout() || check_slices() || check_windows() || check_rules()) return 1;
  std::printf("ok\n");
  return 0;
}
