// gmr_workspace.h -- how the host side of libgmrhip.so owns and carves device memory (not part of the C-ABI).
//
//   Carve            a running offset: the fields of one block, each starting on a 256-byte boundary
//   DeviceBlock      one grow-only device allocation, freed by its destructor: a member of a handle (scratch of an entry
//                    point that is serialised per handle) or a local (scratch of one synchronous call)
//   StreamWorkspace  one DeviceBlock per HIP stream that has called: scratch of an asynchronous, stream-taking entry point
//   HostStage        the scratch of one synchronous entry point: host arrays in, device pointers for the launch, host arrays out
//
// The runtime operations they need (allocate, free, synchronise a stream or the device, copy either way) come from a backend type, so that
// tests/cpp/workspace_check.cpp drives the same code with a recording fake under plain g++: this header pulls in the HIP
// runtime only when HIP compiles it.
#ifndef GMR_WORKSPACE_H
#define GMR_WORKSPACE_H
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <list>
#include <mutex>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace gmr {

struct Carve {
  size_t end = 0;
  size_t take(size_t bytes) {    // the offset of a field of `bytes` bytes (0 is legal: it shares the next field's offset)
    const size_t at = end;
    end += (bytes + 255) / 256 * 256;
    return at;
  }
  size_t total() const { return end; }
};

template <class B>
class DeviceBlockT {
 public:
  DeviceBlockT() = default;
  DeviceBlockT(const DeviceBlockT&) = delete;
  DeviceBlockT& operator=(const DeviceBlockT&) = delete;
  ~DeviceBlockT() { (void)release(); }
  char* data() const { return d_; }
  size_t size() const { return bytes_; }
  // Big enough: nothing happens.  Else the old memory is freed and max(floor, bytes + bytes / headroom_div) bytes are
  // allocated (headroom_div = 0: none); after a failure the block is empty.  Freeing does not wait for work that still
  // uses the old memory: that is the caller's to order (StreamWorkspace does it for blocks that live on a stream).
  typename B::error_t reserve(size_t bytes, size_t headroom_div = 0, size_t floor = 0) {
    if (bytes <= bytes_) return B::success;
    typename B::error_t e = release();
    if (e != B::success) return e;
    size_t want = bytes + (headroom_div ? bytes / headroom_div : 0);
    if (want < floor) want = floor;
    void* p = nullptr;
    if ((e = B::alloc(&p, want)) != B::success) return e;
    d_ = static_cast<char*>(p);
    bytes_ = want;
    return B::success;
  }
  typename B::error_t release() {
    char* old = d_;
    d_ = nullptr;
    bytes_ = 0;
    return old ? B::free(old) : B::success;
  }

 private:
  char* d_ = nullptr;
  size_t bytes_ = 0;
};

// Scratch of an entry point that enqueues on the caller's stream and returns.  Work that still reads a block was enqueued
// on the block's own stream, so growing a block waits for THAT stream alone and never frees memory another stream's
// kernels use.  Two calls on one stream share a block, and only contiguous enqueueing keeps the second call's kernels
// behind the first's: the lease holds the workspace's mutex, and the caller keeps the lease until its last launch is
// enqueued.
template <class B>
class StreamWorkspaceT {
 public:
  class Lease {
   public:
    typename B::error_t error() const { return err_; }
    char* base() const { return base_; }

   private:
    friend class StreamWorkspaceT;
    explicit Lease(std::mutex& mu) : lock_(mu) {}
    std::unique_lock<std::mutex> lock_;
    typename B::error_t err_ = B::success;
    char* base_ = nullptr;
  };

  // the block of `stream`, at least `bytes` bytes (grown with a quarter of headroom); on an error base() is null
  Lease acquire(typename B::stream_t stream, size_t bytes) {
    Lease l(mu_);
    Entry* w = nullptr;
    for (Entry& e : entries_)
      if (e.stream == stream) w = &e;
    if (!w) {
      entries_.emplace_back();
      w = &entries_.back();
      w->stream = stream;
    }
    if (bytes > w->block.size() && w->block.data()) l.err_ = B::sync(stream);
    if (l.err_ == B::success) l.err_ = w->block.reserve(bytes, 4);
    if (l.err_ == B::success) l.base_ = w->block.data();
    return l;
  }

 private:
  struct Entry {
    typename B::stream_t stream;
    DeviceBlockT<B> block;
  };
  std::mutex mu_;
  std::list<Entry> entries_;     // (a list: blocks do not move)
};

// The scratch of one synchronous call.  The entry point declares its host arrays, each with the variable (or the field of a C-ABI
// struct) that is to hold the array's device address; upload() makes ONE allocation, every field on a 256-byte boundary, points
// the variables into it and copies the inputs; the entry point launches; download() waits for the device and copies the outputs back.
//   null host pointer          null device pointer, no copy
//   non-null, 0 bytes          a valid device pointer, no copy either way
//   scratch                    a field without a host array: a valid device pointer, no copy either way
//   in_shared                  arrays that may interleave in one tensor: when the hull of those present is no longer than the sum of
//                              their extents it is copied once and each device pointer keeps its array's offset inside it
// The variables must stay where they are until upload() has returned.  On an error, failed() names the operation; after a failed
// upload() nothing has been copied back, and the destructor frees the block either way.
template <class B>
class HostStageT {
 public:
  using error_t = typename B::error_t;
  static constexpr int kMaxArrays = 48;      // per call; an entry point declares a fixed few, so running over is a bug: abort()

  template <class T> void in(T*& d, const void* h, size_t bytes) { d = nullptr; add(&d, h, bytes, kIn); }
  template <class T> void in_shared(T*& d, const void* h, size_t bytes) { d = nullptr; add(&d, h, bytes, kShared); }
  // copy_back = false: the kernels get the memory, the host array stays as it is
  template <class T> void out(T*& d, void* h, size_t bytes, bool copy_back = true) { d = nullptr; add(&d, h, bytes, copy_back ? kOut : kScratch); }
  // a field no host array stands behind: what one launch of the call leaves for the next
  template <class T> void scratch(T*& d, size_t bytes) { d = nullptr; add(&d, nullptr, bytes, kDevice); }

  error_t upload() {
    if (n_ == 0) return B::success;          // nothing to stage: no allocation
    uintptr_t lo = UINTPTR_MAX, hi = 0;      // (addresses as integers: the shared arrays may be separate objects)
    size_t sum = 0;
    for (int k = 0; k < n_; k++) {
      const Array& a = arrays_[k];
      if (a.kind != kShared) continue;
      const uintptr_t p = (uintptr_t)a.host;
      if (p < lo) lo = p;
      if (p + a.bytes > hi) hi = p + a.bytes;
      sum += a.bytes;
    }
    const bool hull = hi > lo && hi - lo <= sum;
    Carve cv;
    const size_t o_hull = hull ? cv.take(hi - lo) : 0;
    for (int k = 0; k < n_; k++) {
      Array& a = arrays_[k];
      a.off = (hull && a.kind == kShared) ? o_hull + ((uintptr_t)a.host - lo) : cv.take(a.bytes);
    }
    what_ = "allocating the device scratch of the call";
    error_t e = block_.reserve(cv.total() + 256);      // (+ 256: never empty, and a trailing empty field has an address inside)
    if (e != B::success) return e;
    what_ = "copying an input to the device";
    if (hull && (e = B::to_device(block_.data() + o_hull, (const void*)lo, hi - lo)) != B::success) return e;
    for (int k = 0; k < n_; k++) {
      const Array& a = arrays_[k];
      char* d = block_.data() + a.off;
      memcpy(a.var, &d, sizeof d);           // (the variable is a T* of some T: every object pointer is stored alike)
      const bool copy = a.bytes && (a.kind == kIn || (a.kind == kShared && !hull));
      if (copy && (e = B::to_device(d, a.host, a.bytes)) != B::success) return e;
    }
    return B::success;
  }

  error_t download() {
    what_ = "waiting for the device";
    error_t e = B::sync_device();
    if (e != B::success) return e;
    what_ = "copying an output to the host";
    for (int k = 0; k < n_; k++) {
      const Array& a = arrays_[k];
      if (a.kind == kOut && a.bytes && (e = B::to_host(a.host, block_.data() + a.off, a.bytes)) != B::success) return e;
    }
    return B::success;
  }

  const char* failed() const { return what_; }      // the operation that upload() or download() reported an error from

 private:
  enum Kind { kIn, kShared, kOut, kScratch, kDevice };
  struct Array {
    void* var;       // the caller's pointer variable
    void* host;
    size_t bytes, off;
    Kind kind;
  };
  void add(void* var, const void* h, size_t bytes, Kind kind) {
    if (!h && kind != kDevice) return;
    if (n_ == kMaxArrays) abort();
    arrays_[n_++] = Array{var, const_cast<void*>(h), bytes, 0, kind};
  }
  Array arrays_[kMaxArrays];
  int n_ = 0;
  const char* what_ = "";
  DeviceBlockT<B> block_;
};

#ifdef __HIPCC__
struct HipBackend {
  using error_t = hipError_t;
  using stream_t = hipStream_t;
  static constexpr hipError_t success = hipSuccess;
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }       // (waits for the device: destroying a handle needs no sync)
  static hipError_t sync(hipStream_t s) { return hipStreamSynchronize(s); }
  static hipError_t sync_device() { return hipDeviceSynchronize(); }
  static hipError_t to_device(void* d, const void* h, size_t bytes) { return hipMemcpy(d, h, bytes, hipMemcpyHostToDevice); }
  static hipError_t to_host(void* h, const void* d, size_t bytes) { return hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost); }
};
using DeviceBlock = DeviceBlockT<HipBackend>;
using StreamWorkspace = StreamWorkspaceT<HipBackend>;
using HostStage = HostStageT<HipBackend>;
#endif

}  // namespace gmr
#endif
