// mc_host.h — what the host side of every C ABI file (mc_capi.hip,
// mc_super.hip) shares: the thread's error message, HIP_TRY, the typed device
// allocation of a handle's arrays and a device buffer that a handle may grow.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "marlcov.h"
#include "mc_msg.h"

namespace mc {

// mc_last_error()'s message: one per thread for the whole library
inline thread_local std::string g_last_error;

// sets the message and returns `code`; an argument may be g_last_error's own
// text (a prefix put in front of a callee's message)
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vmsgf(g_last_error, fmt, ap);
  va_end(ap);
  return code;
}

// the same from a call that returns a string: sets the message and returns ""
inline const char* fail_str(int code, const char* msg) { return fail(code, "%s", msg), ""; }

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) return mc::fail(MC_EHIP, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// two of the three spellings of a switch in use (the third is mere presence)
inline bool env_is_1(const char* name) {
  const char* v = getenv(name);
  return v && atoi(v) == 1;
}
inline bool env_starts_0(const char* name) {
  const char* v = getenv(name);
  return v && v[0] == '0';
}

// `count` elements of T on the device, every byte `fill` (at least 16 bytes),
// freed with the handle's other arrays in `allocs`
template <class T>
int dev_alloc(std::vector<void*>& allocs, T*& dst, size_t count, int fill = 0) {
  const size_t bytes = count * sizeof(T) < 16 ? 16 : count * sizeof(T);
  void* q = nullptr;
  HIP_TRY(hipMalloc(&q, bytes));
  allocs.push_back(q);
  HIP_TRY(hipMemset(q, fill, bytes));
  dst = static_cast<T*>(q);
  return MC_OK;
}

// A handle under construction: an error return destroys what it holds so far
// (std::unique_ptr<Env, HandleDeleter<mc_destroy>>, released into *out_env).
template <void (*Destroy)(void*)>
struct HandleDeleter {
  void operator()(void* p) const { Destroy(p); }
};

// A device buffer that its handle owns alone and re-sizes between calls.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;  // bytes
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  // room for `bytes`: a smaller buffer is freed first (its contents are lost);
  // on failure the buffer is empty
  hipError_t reserve(size_t bytes) {
    if (p && bytes <= cap) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p, bytes);
    cap = e == hipSuccess ? bytes : 0;
    if (e != hipSuccess) p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace mc
