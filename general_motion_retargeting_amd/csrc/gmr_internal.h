// gmr_internal.h -- shared by the translation units of libgmrhip.so, not part of the C-ABI.
#ifndef GMR_INTERNAL_H
#define GMR_INTERNAL_H
// records the thread-local message returned by gmr_last_error() and returns `code`
__attribute__((visibility("hidden"))) int gmr_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// returns GMR_ERR_HIP from the enclosing function, with the message "<what>: <HIP's error string>", when `call` fails
#define GMR_NAMED_HIP_TRY(what, call)                                                               \
  do {                                                                                              \
    hipError_t _e = (call);                                                                         \
    if (_e != hipSuccess) return gmr_fail(GMR_ERR_HIP, "%s: %s", what, hipGetErrorString(_e));      \
  } while (0)
#define GMR_HIP_TRY(call) GMR_NAMED_HIP_TRY(#call, call)
// the same for st.upload() / st.download() of a gmr::HostStage: the message names the operation inside that failed
#define GMR_STAGE_TRY(st, step) GMR_NAMED_HIP_TRY((st).failed(), (st).step())
#endif
