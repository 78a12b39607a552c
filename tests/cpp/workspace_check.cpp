// The host side's device-memory helpers (csrc/gmr_workspace.h: Carve, DeviceBlock, StreamWorkspace, HostStage) driven on the CPU
// with a backend that records what the library would ask of the HIP runtime (plain C++, no HIP):
//   * Carve: offsets are multiples of 256, ascending, non-overlapping; total() covers the last field; empty fields are legal;
//   * DeviceBlock: grow-only, the requested headroom and floor, freed exactly once;
//   * StreamWorkspace: a call that fits asks nothing of the runtime; growth is synchronise(own stream), free, allocate
//     (bytes + bytes / 4) and touches no other stream; a failed allocation leaves the entry empty and the next call
//     retries; the lease excludes other threads until it is released;
//   * HostStage: one allocation per call and one copy per present non-empty input; null stays null, empty gets an address and no
//     copy; fields at multiples of 256 that do not overlap; download is synchronise, then the copies of the outputs that are
//     neither skipped nor empty; the bytes a "kernel" (a host loop over the device pointers) wrote come back; arrays that
//     interleave in one tensor travel as one copy of their hull, arrays apart as one copy each; a failed allocation copies
//     nothing and writes no host output; a scratch field (no host array) has bytes of its own and is copied neither way;
//     the block is freed exactly once.  The fake's memory is malloc'd and its copies are
//     memcpy, so real bytes make the round trip.
// Prints "ok"; exit code 0 = all good.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../general_motion_retargeting_amd/csrc/gmr_workspace.h"

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "CHECK failed (line %d): %s : ", __LINE__, #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

struct Op {
  char what;                 // 'a'lloc, 'f'ree, 's'ync of a stream, 'S'ync of the device, 'u'pload (host to device), 'd'ownload
  void* p;                   // the block (alloc / free), the stream (sync) or the device address (copies)
  size_t bytes;
  bool operator==(const Op& o) const { return what == o.what && p == o.p && bytes == o.bytes; }
};

struct Fake {
  using error_t = int;
  using stream_t = void*;
  static constexpr int success = 0;
  static std::vector<Op> log;
  static std::set<void*> live;
  static int fail_allocs;    // this many coming allocations fail with error 2
  static int double_frees;
  static int alloc(void** p, size_t bytes) {
    if (fail_allocs > 0) { fail_allocs--; log.push_back({'a', nullptr, bytes}); return 2; }
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    log.push_back({'a', *p, bytes});
    return 0;
  }
  static int free(void* p) {
    if (!live.erase(p)) double_frees++;
    else std::free(p);
    log.push_back({'f', p, 0});
    return 0;
  }
  static int sync(void* s) { log.push_back({'s', s, 0}); return 0; }
  static int sync_device() { log.push_back({'S', nullptr, 0}); return 0; }
  static int to_device(void* d, const void* h, size_t bytes) { std::memcpy(d, h, bytes); log.push_back({'u', d, bytes}); return 0; }
  static int to_host(void* h, const void* d, size_t bytes) { std::memcpy(h, d, bytes); log.push_back({'d', const_cast<void*>(d), bytes}); return 0; }
  static size_t count(char what) { size_t n = 0; for (const Op& o : log) n += o.what == what; return n; }
};
std::vector<Op> Fake::log;
std::set<void*> Fake::live;
int Fake::fail_allocs = 0;
int Fake::double_frees = 0;

using Block = gmr::DeviceBlockT<Fake>;
using Workspace = gmr::StreamWorkspaceT<Fake>;
using Stage = gmr::HostStageT<Fake>;

static int check_carve() {
  gmr::Carve c;
  const size_t sizes[] = {1, 0, 256, 257, 0, 0, 1000000, 255, 4};
  size_t prev_end = 0;
  for (size_t b : sizes) {
    const size_t at = c.take(b);
    CHECK(at % 256 == 0, "offset %zu", at);
    CHECK(at >= prev_end, "field at %zu overlaps the one ending at %zu", at, prev_end);
    CHECK(c.total() >= at + b && c.total() % 256 == 0 && c.total() - (at + b) < 256, "total %zu after a field of %zu at %zu", c.total(), b, at);
    prev_end = at + b;
  }
  CHECK(gmr::Carve{}.total() == 0, "an empty layout");
  return 0;
}

static int check_block() {
  Fake::log.clear();
  {
    Block b;
    CHECK(b.data() == nullptr && b.size() == 0, "a new block is empty");
    CHECK(b.reserve(1000) == 0 && b.size() == 1000 && b.data(), "exact size");
    char* first = b.data();
    CHECK(b.reserve(1000) == 0 && b.reserve(10) == 0 && b.data() == first && Fake::log.size() == 1, "a block that fits is left alone");
    CHECK(b.reserve(2000, 4) == 0 && b.size() == 2500, "a quarter of headroom: %zu", b.size());
    CHECK(Fake::log.size() == 3 && Fake::log[1] == (Op{'f', first, 0}) && Fake::log[2].what == 'a', "growth frees, then allocates");
    Block small;
    CHECK(small.reserve(100, 0, 1u << 20) == 0 && small.size() == (1u << 20), "floor");
    CHECK(small.reserve((1u << 20) + 1, 0, 1u << 20) == 0 && small.size() == (1u << 20) + 1, "above the floor: exact");
    Fake::fail_allocs = 1;
    CHECK(b.reserve(5000) == 2 && b.data() == nullptr && b.size() == 0, "a failed allocation leaves the block empty");
    CHECK(b.reserve(5000) == 0 && b.size() == 5000, "and the next call retries");
  }
  CHECK(Fake::live.empty() && Fake::double_frees == 0, "destruction frees every block exactly once (%zu live, %d double)", Fake::live.size(), Fake::double_frees);
  return 0;
}

static int check_workspace() {
  int s1 = 0, s2 = 0;        // two streams: only their addresses matter
  Fake::log.clear();
  {
    Workspace ws;
    char *a1, *a2;
    { auto l = ws.acquire(&s1, 1024); CHECK(l.error() == 0 && l.base(), "first acquire"); a1 = l.base(); }
    CHECK(Fake::log.size() == 1 && Fake::log[0].what == 'a' && Fake::log[0].bytes == 1024 + 256, "the first block needs no synchronise: one allocation of bytes + bytes / 4");
    { auto l = ws.acquire(&s1, 1280); CHECK(l.base() == a1, "same stream, fits: same base"); }
    { auto l = ws.acquire(&s1, 16); CHECK(l.base() == a1, "same stream, smaller: same base"); }
    CHECK(Fake::log.size() == 1, "a call that fits performs no backend call");
    { auto l = ws.acquire(&s2, 512); CHECK(l.error() == 0 && l.base() && l.base() != a1, "a second stream gets its own block"); a2 = l.base(); }
    CHECK(Fake::log.size() == 2 && Fake::log[1].what == 'a', "and no synchronise either");
    Fake::log.clear();
    char* b1;
    { auto l = ws.acquire(&s1, 4096); CHECK(l.error() == 0 && l.base(), "growth"); b1 = l.base(); }
    CHECK(Fake::log.size() == 3 && Fake::log[0] == (Op{'s', &s1, 0}) && Fake::log[1] == (Op{'f', a1, 0}) && Fake::log[2] == (Op{'a', b1, 4096 + 1024}),
          "growth is synchronise(own stream), free(old), allocate(bytes + bytes / 4), nothing else");
    { auto l = ws.acquire(&s2, 512); CHECK(l.base() == a2, "growing one stream's block leaves the other's alone"); }
    Fake::log.clear();
    Fake::fail_allocs = 1;
    { auto l = ws.acquire(&s2, 1 << 20); CHECK(l.error() == 2 && l.base() == nullptr, "a failed allocation is reported"); }
    CHECK(Fake::log.size() == 3 && Fake::log[0] == (Op{'s', &s2, 0}) && Fake::log[1] == (Op{'f', a2, 0}), "after the stream's synchronise and the free");
    Fake::log.clear();
    { auto l = ws.acquire(&s2, 64); CHECK(l.error() == 0 && l.base(), "the entry was left empty: the next call allocates again"); }
    CHECK(Fake::log.size() == 1 && Fake::log[0].what == 'a' && Fake::log[0].bytes == 64 + 16, "without a synchronise or a free of the lost block");
    { auto l = ws.acquire(&s1, 4096); CHECK(l.base() == b1, "the other stream never noticed"); }

    // the lease is the lock: a second thread's acquire returns only after the first lease is gone
    std::atomic<int> stage{0};
    std::thread other;
    {
      auto l = ws.acquire(&s1, 16);
      other = std::thread([&] { stage = 1; auto m = ws.acquire(&s2, 16); stage = 2; });
      while (stage.load() == 0) std::this_thread::yield();
      std::this_thread::sleep_for(std::chrono::milliseconds(100));
      CHECK(stage.load() == 1, "a second acquire went through while a lease was held");
    }
    other.join();
    CHECK(stage.load() == 2, "the second acquire after the release");
  }
  CHECK(Fake::live.empty() && Fake::double_frees == 0, "destruction frees every block exactly once (%zu live, %d double)", Fake::live.size(), Fake::double_frees);
  return 0;
}

static int check_stage() {
  // every kind of array in one call: present, null and empty inputs; present, null, skipped and empty outputs
  std::vector<unsigned char> a(100), d(300), o1(64, 0), o3(32, 0x11), o5(257, 0);
  for (size_t i = 0; i < a.size(); i++) a[i] = (unsigned char)(i * 7 + 1);
  for (size_t i = 0; i < d.size(); i++) d[i] = (unsigned char)(i * 13 + 5);
  char empty_in = 0, empty_out = 0x22;       // only their addresses are used
  Fake::log.clear();
  {
    Stage st;
    const unsigned char *d_a, *d_b, *d_c, *d_d;
    unsigned char *d_o1, *d_o2, *d_o3, *d_o4, *d_o5;
    st.in(d_a, a.data(), a.size());
    st.in(d_b, nullptr, 999);
    st.in(d_c, &empty_in, 0);
    st.in(d_d, d.data(), d.size());
    st.out(d_o1, o1.data(), o1.size());
    st.out(d_o2, nullptr, 999);
    st.out(d_o3, o3.data(), o3.size(), false);
    st.out(d_o5, o5.data(), o5.size());
    st.out(d_o4, &empty_out, 0);             // (a trailing empty field)
    CHECK(Fake::log.empty(), "declaring asks nothing of the runtime");
    CHECK(st.upload() == 0, "upload");
    CHECK(Fake::log.size() == 3 && Fake::log[0].what == 'a' && Fake::count('u') == 2, "one allocation, then one copy per present non-empty input (%zu ops)", Fake::log.size());
    CHECK(d_b == nullptr && d_o2 == nullptr, "null in gives null out");
    CHECK(d_c != nullptr && d_o4 != nullptr, "non-null with 0 bytes gives an address");
    const char* base = (const char*)Fake::log[0].p;
    const size_t cap = Fake::log[0].bytes;
    CHECK(cap > 0, "the allocation is never empty");
    const struct { const void* p; size_t bytes; } f[] = {{d_a, a.size()}, {d_c, 0}, {d_d, d.size()}, {d_o1, o1.size()}, {d_o3, o3.size()}, {d_o5, o5.size()}, {d_o4, 0}};
    size_t prev_end = 0;
    for (const auto& x : f) {
      const size_t at = (size_t)((const char*)x.p - base);
      CHECK(at % 256 == 0 && at >= prev_end && at + x.bytes <= cap && at < cap, "a field of %zu bytes at %zu (the one before ends at %zu, the block at %zu)", x.bytes, at, prev_end, cap);
      prev_end = at + x.bytes;
    }
    CHECK(Fake::log[1] == (Op{'u', (void*)d_a, a.size()}) && Fake::log[2] == (Op{'u', (void*)d_d, d.size()}), "the copies are of the inputs, at their size");
    CHECK(!std::memcmp(d_a, a.data(), a.size()) && !std::memcmp(d_d, d.data(), d.size()), "the device sees the inputs");
    // the "kernel"
    for (size_t i = 0; i < o1.size(); i++) d_o1[i] = d_a[i] ^ 0x5a;
    for (size_t i = 0; i < o3.size(); i++) d_o3[i] = 0xee;
    for (size_t i = 0; i < o5.size(); i++) d_o5[i] = (unsigned char)(d_d[i] + 1);
    CHECK(o1[0] == 0 && o5[0] == 0, "nothing reaches the host before download");
    Fake::log.clear();
    CHECK(st.download() == 0, "download");
    CHECK(Fake::log.size() == 3 && Fake::log[0] == (Op{'S', nullptr, 0}) && Fake::log[1] == (Op{'d', d_o1, o1.size()}) && Fake::log[2] == (Op{'d', d_o5, o5.size()}),
          "download is synchronise, then one copy per output that is neither skipped nor empty (%zu ops)", Fake::log.size());
    for (size_t i = 0; i < o1.size(); i++) CHECK(o1[i] == (unsigned char)(a[i] ^ 0x5a), "o1[%zu]", i);
    for (size_t i = 0; i < o5.size(); i++) CHECK(o5[i] == (unsigned char)(d[i] + 1), "o5[%zu]", i);
    for (size_t i = 0; i < o3.size(); i++) CHECK(o3[i] == 0x11, "a skipped output was written at %zu", i);
    CHECK(empty_out == 0x22, "an empty output was written");
    Fake::log.clear();
  }
  CHECK(Fake::log.size() == 1 && Fake::log[0].what == 'f' && Fake::live.empty() && Fake::double_frees == 0, "the block is freed exactly once");
  {
    Stage st;
    CHECK(st.upload() == 0 && st.download() == 0 && Fake::count('a') == 0, "a call without arrays allocates nothing");
  }

  // a field without a host array: what the first "launch" of a call leaves for its second
  Fake::log.clear();
  {
    std::vector<unsigned char> in(70), res(70, 0);
    for (size_t i = 0; i < in.size(); i++) in[i] = (unsigned char)(i * 3 + 2);
    Stage st;
    const unsigned char* d_in;
    unsigned char *d_mid, *d_none, *d_res;
    st.in(d_in, in.data(), in.size());
    st.scratch(d_mid, 300);
    st.scratch(d_none, 0);
    st.out(d_res, res.data(), res.size());
    CHECK(st.upload() == 0, "upload");
    CHECK(Fake::log.size() == 2 && Fake::log[0].what == 'a' && Fake::log[1] == (Op{'u', (void*)d_in, in.size()}), "one allocation and the one input's copy: nothing is copied into a scratch field (%zu ops)", Fake::log.size());
    const unsigned char* base = (const unsigned char*)Fake::log[0].p;
    const size_t at_in = (size_t)(d_in - base), at_mid = (size_t)(d_mid - base), at_none = (size_t)(d_none - base), at_res = (size_t)(d_res - base);
    CHECK(d_mid && at_mid % 256 == 0 && at_mid >= at_in + in.size() && at_none >= at_mid + 300 && at_res >= at_mid + 300 && at_res + res.size() <= Fake::log[0].bytes,
          "the scratch field has 300 bytes of its own (in %zu, scratch %zu, out %zu)", at_in, at_mid, at_res);
    CHECK(d_none != nullptr, "a scratch field of 0 bytes gets an address");
    for (size_t i = 0; i < 300; i++) d_mid[i] = (unsigned char)(d_in[i % in.size()] + 1);      // launch 1
    for (size_t i = 0; i < res.size(); i++) d_res[i] = (unsigned char)(d_mid[i] ^ d_mid[i + 230]);      // launch 2
    Fake::log.clear();
    CHECK(st.download() == 0, "download");
    CHECK(Fake::log.size() == 2 && Fake::log[0] == (Op{'S', nullptr, 0}) && Fake::log[1] == (Op{'d', d_res, res.size()}), "download copies the output alone (%zu ops)", Fake::log.size());
    for (size_t i = 0; i < res.size(); i++) CHECK(res[i] == (unsigned char)((in[i] + 1) ^ (in[(i + 230) % in.size()] + 1)), "res[%zu]", i);
  }
  CHECK(Fake::live.empty() && Fake::double_frees == 0, "the block is freed exactly once");

  // arrays that interleave in one tensor: [n][7] (pos 3, quat 4) and [n][13] (pos 3, quat 4, vel 3, ang vel 3, the vel left out)
  const size_t n = 5;
  std::vector<float> t7(n * 7), t13(n * 13);
  for (size_t i = 0; i < t7.size(); i++) t7[i] = (float)i;
  for (size_t i = 0; i < t13.size(); i++) t13[i] = 1000.0f + (float)i;
  Fake::log.clear();
  {
    Stage st;
    const float *d_pos, *d_rot;
    st.in_shared(d_pos, t7.data(), ((n - 1) * 7 + 3) * 4);
    st.in_shared(d_rot, t7.data() + 3, ((n - 1) * 7 + 4) * 4);
    CHECK(st.upload() == 0, "upload");
    CHECK(Fake::count('a') == 1 && Fake::count('u') == 1 && Fake::log[1] == (Op{'u', (void*)d_pos, n * 7 * 4}), "two interleaved arrays: one copy of hi - lo bytes");
    CHECK(d_rot == d_pos + 3, "each at its own offset in the hull");
    for (size_t e = 0; e < n; e++) CHECK(d_pos[e * 7 + 2] == t7[e * 7 + 2] && d_rot[e * 7 + 3] == t7[e * 7 + 6], "row %zu", e);
  }
  Fake::log.clear();
  {
    Stage st;
    const float *d_pos, *d_rot, *d_vel, *d_ang, *d_other;
    const float other[2] = {7.0f, 8.0f};
    st.in(d_other, other, sizeof other);                // (a plain input beside the group)
    st.in_shared(d_rot, t13.data() + 3, ((n - 1) * 13 + 4) * 4);      // (in any order)
    st.in_shared(d_pos, t13.data(), ((n - 1) * 13 + 3) * 4);
    st.in_shared(d_vel, nullptr, ((n - 1) * 13 + 3) * 4);
    st.in_shared(d_ang, t13.data() + 10, ((n - 1) * 13 + 3) * 4);
    CHECK(st.upload() == 0, "upload");
    CHECK(Fake::count('a') == 1 && Fake::count('u') == 2, "four interleaved arrays and one plain: two copies, got %zu", Fake::count('u'));
    bool hull_copied = false;
    for (const Op& o : Fake::log) hull_copied |= o == (Op{'u', (void*)d_pos, n * 13 * 4});
    CHECK(hull_copied, "one of them the hull, of hi - lo bytes");
    CHECK(d_vel == nullptr, "a null member is left out");
    CHECK(d_rot == d_pos + 3 && d_ang == d_pos + 10 && ((const char*)d_pos - (const char*)Fake::log[0].p) % 256 == 0, "each at its own offset in the hull");
    for (size_t e = 0; e < n; e++)
      CHECK(d_pos[e * 13] == t13[e * 13] && d_rot[e * 13 + 3] == t13[e * 13 + 6] && d_ang[e * 13 + 2] == t13[e * 13 + 12], "row %zu", e);
    CHECK(d_other[0] == 7.0f && d_other[1] == 8.0f, "the plain input");
  }
  // arrays of one group in separate allocations: one copy each
  Fake::log.clear();
  {
    std::vector<float> p(n * 3, 1.0f), q(n * 4, 2.0f);
    const uintptr_t lo = std::min((uintptr_t)p.data(), (uintptr_t)q.data()), hi = std::max((uintptr_t)(p.data() + p.size()), (uintptr_t)(q.data() + q.size()));
    CHECK(hi - lo > (p.size() + q.size()) * 4, "the two arrays of this case must lie apart");
    Stage st;
    const float *d_p, *d_q;
    st.in_shared(d_p, p.data(), p.size() * 4);
    st.in_shared(d_q, q.data(), q.size() * 4);
    CHECK(st.upload() == 0, "upload");
    CHECK(Fake::count('a') == 1 && Fake::count('u') == 2 && Fake::log[1] == (Op{'u', (void*)d_p, p.size() * 4}) && Fake::log[2] == (Op{'u', (void*)d_q, q.size() * 4}),
          "arrays apart: one copy each");
    const size_t at_p = (size_t)((const char*)d_p - (const char*)Fake::log[0].p), at_q = (size_t)((const char*)d_q - (const char*)Fake::log[0].p);
    CHECK(at_p % 256 == 0 && at_q % 256 == 0 && at_q >= at_p + p.size() * 4, "as fields of their own");
    CHECK(d_p[n * 3 - 1] == 1.0f && d_q[n * 4 - 1] == 2.0f, "their data");
  }
  CHECK(Fake::live.empty() && Fake::double_frees == 0, "every block freed exactly once");

  // a failed allocation: the error comes back, nothing is copied, no host output is written
  Fake::log.clear();
  {
    std::vector<unsigned char> in(40, 3), out(40, 0x44);
    Stage st;
    const unsigned char* d_in;
    unsigned char* d_out;
    st.in(d_in, in.data(), in.size());
    st.out(d_out, out.data(), out.size());
    Fake::fail_allocs = 1;
    CHECK(st.upload() == 2, "a failed allocation is reported");
    CHECK(st.failed()[0] != 0, "and the failing operation named");
    CHECK(Fake::log.size() == 1 && Fake::log[0].what == 'a', "with no copy (%zu ops)", Fake::log.size());
    for (unsigned char c : out) CHECK(c == 0x44, "a host output was written after a failed upload");
  }
  CHECK(Fake::live.empty() && Fake::double_frees == 0 && Fake::count('f') == 0, "nothing to free after a failed allocation");
  return 0;
}

int main() {
  if (check_carve() || check_block() || check_workspace() || check_stage()) return 1;
  std::printf("ok\n");
  return 0;
}
