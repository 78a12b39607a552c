// gmr_workspace.h -- how the host side of libgmrhip.so owns and carves device memory (not part of the C-ABI).
//
//   Carve            a running offset: the fields of one block, each starting on a 256-byte boundary
//   DeviceBlock      one grow-only device allocation, freed by its destructor: a member of a handle (scratch of an entry
//                    point that is serialised per handle) or a local (scratch of one synchronous call)
//   StreamWorkspace  one DeviceBlock per HIP stream that has called: scratch of an asynchronous, stream-taking entry point
//
// The three runtime operations they need (allocate, free, synchronise a stream) come from a backend type, so that
// tests/cpp/workspace_check.cpp drives the same code with a recording fake under plain g++: this header pulls in the HIP
// runtime only when HIP compiles it.
#ifndef GMR_WORKSPACE_H
#define GMR_WORKSPACE_H
#include <stddef.h>

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

#ifdef __HIPCC__
struct HipBackend {
  using error_t = hipError_t;
  using stream_t = hipStream_t;
  static constexpr hipError_t success = hipSuccess;
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }       // (waits for the device: destroying a handle needs no sync)
  static hipError_t sync(hipStream_t s) { return hipStreamSynchronize(s); }
};
using DeviceBlock = DeviceBlockT<HipBackend>;
using StreamWorkspace = StreamWorkspaceT<HipBackend>;
#endif

}  // namespace gmr
#endif
