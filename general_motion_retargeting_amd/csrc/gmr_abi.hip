// gmr_abi.hip -- what every part of the C-ABI of libgmrhip.so (include/gmr_hip.h) shares: the error message behind
// gmr_last_error(), the description of the backend, and the device, memory, stream and event helpers.  The entry points of a
// module live beside its kernels (IK: gmr_ik_host.hip, FK: gmr_fk.hip, post-processing: gmr_post.hip, ...).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/gmr_hip.h"
#include "gmr_internal.h"

static_assert(sizeof(gmr_model_t) % 8 == 0, "gmr_model_t must be 8-byte sized");
static_assert(sizeof(gmr_taskset_t) % 8 == 0, "gmr_taskset_t must be 8-byte sized");
static_assert(offsetof(gmr_model_t, timestep) % 8 == 0, "double block of gmr_model_t misaligned");
static_assert(offsetof(gmr_taskset_t, damping) % 8 == 0, "double block of gmr_taskset_t misaligned");

namespace {
thread_local char g_err[512] = "";
}
int gmr_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
#define fail gmr_fail

extern "C" {

const char* gmr_last_error(void) { return g_err; }

const char* gmr_backend_info(void) {
  static thread_local char buf[256];
  int dev = -1;
  hipDeviceProp_t p;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess)
    snprintf(buf, sizeof buf, "hip:%s device=%d name=%s CUs=%d", p.gcnArchName, dev, p.name, p.multiProcessorCount);
  else
    snprintf(buf, sizeof buf, "hip:no-device");
  return buf;
}

int gmr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int gmr_set_device(int device) { GMR_HIP_TRY(hipSetDevice(device)); return GMR_OK; }
size_t gmr_sizeof_model(void) { return sizeof(gmr_model_t); }
size_t gmr_sizeof_taskset(void) { return sizeof(gmr_taskset_t); }

int gmr_malloc(void** ptr, size_t bytes) {
  if (!ptr) return fail(GMR_ERR_ARG, "gmr_malloc: null out pointer");
  GMR_HIP_TRY(hipMalloc(ptr, bytes ? bytes : 8));
  return GMR_OK;
}
int gmr_free(void* ptr) { if (ptr) GMR_HIP_TRY(hipFree(ptr)); return GMR_OK; }
int gmr_host_alloc(void** ptr, size_t bytes) {
  if (!ptr) return fail(GMR_ERR_ARG, "gmr_host_alloc: null out pointer");
  GMR_HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 8, hipHostMallocDefault));
  return GMR_OK;
}
int gmr_host_free(void* ptr) { if (ptr) GMR_HIP_TRY(hipHostFree(ptr)); return GMR_OK; }
int gmr_host_register(void* ptr, size_t bytes) {
  if (!ptr) return fail(GMR_ERR_ARG, "gmr_host_register: null pointer");
  GMR_HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  return GMR_OK;
}
int gmr_host_unregister(void* ptr) { if (ptr) GMR_HIP_TRY(hipHostUnregister(ptr)); return GMR_OK; }
int gmr_memset(void* ptr, int value, size_t bytes, void* stream) {
  GMR_HIP_TRY(hipMemsetAsync(ptr, value, bytes, (hipStream_t)stream));
  return GMR_OK;
}
int gmr_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  GMR_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return GMR_OK;
}
int gmr_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  GMR_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  return GMR_OK;
}
int gmr_stream_create(void** stream) {
  hipStream_t s;
  GMR_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = (void*)s;
  return GMR_OK;
}
int gmr_stream_destroy(void* stream) { GMR_HIP_TRY(hipStreamDestroy((hipStream_t)stream)); return GMR_OK; }
int gmr_stream_sync(void* stream) {
  if (stream) GMR_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  else GMR_HIP_TRY(hipDeviceSynchronize());
  return GMR_OK;
}
int gmr_event_create(void** event) {
  hipEvent_t e;
  GMR_HIP_TRY(hipEventCreate(&e));
  *event = (void*)e;
  return GMR_OK;
}
int gmr_event_destroy(void* event) { GMR_HIP_TRY(hipEventDestroy((hipEvent_t)event)); return GMR_OK; }
int gmr_event_record(void* event, void* stream) {
  GMR_HIP_TRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
  return GMR_OK;
}
int gmr_event_elapsed_ms(void* start, void* stop, float* ms) {
  GMR_HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
  GMR_HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return GMR_OK;
}

}  // extern "C"
