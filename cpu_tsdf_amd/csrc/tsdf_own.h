// Internal: the three owners of what the host code allocates while it runs -- device memory that grows on demand or lives
// for one function (DevBuf), events created on first use (EventSet), and the pinned two-slot staged copy between device
// memory and a caller's host memory (PinnedStage) -- and the error plumbing they report through.  Their destructors do the
// freeing, so a return through TSDF_HIP_TRY releases what the function holds.  Included by tsdf_common.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string>

#include "tsdf_hip.h"

// Error plumbing -------------------------------------------------------------------------------
void tsdf_set_error(const std::string &msg);
int tsdf_hip_fail(hipError_t e, const char *what, const char *file, int line);

#define TSDF_HIP_TRY(expr)                                              \
  do {                                                                  \
    hipError_t _e = (expr);                                             \
    if (_e != hipSuccess) return tsdf_hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while (0)

// Device memory.  Frees on destruction, on the device that is current then: a member of a handle or of a feature state goes
// inside free_volume's device scope, a function's temporary before the scope it was declared after.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;  // bytes
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr, cap = 0;
  }
  template <typename T>
  T *as() const { return static_cast<T *>(p); }
  // one allocation of exactly `bytes` (a function's temporary); whatever was held goes first
  int alloc(size_t bytes) {
    release();
    TSDF_HIP_TRY(hipMalloc(&p, bytes));
    cap = bytes;
    return TSDF_HIP_OK;
  }
  // Room for `need` bytes; grows only, and never keeps the contents.  Work queued on `s` may still use the memory held, so
  // growing waits for the stream, frees, and allocates exactly `need` (slack is the caller's to add).  Empty on failure: with
  // a `who`, TSDF_HIP_E_NOMEM and a message that names it; without, what tsdf_hip_fail makes of the error.
  int reserve(size_t need, hipStream_t s, const char *who = nullptr) {
    if (need <= cap) return TSDF_HIP_OK;
    if (p) {
      TSDF_HIP_TRY(hipStreamSynchronize(s));
      release();
    }
    const hipError_t e = hipMalloc(&p, need);
    if (e != hipSuccess) {
      p = nullptr;
      if (!who) return tsdf_hip_fail(e, "hipMalloc", __FILE__, __LINE__);
      (void)hipGetLastError();
      tsdf_set_error(std::string(who) + ": " + std::to_string(need) + " bytes of device memory for the working set are not available");
      return TSDF_HIP_E_NOMEM;
    }
    cap = need;
    return TSDF_HIP_OK;
  }
};

// Up to N events, created on first use.
template <int N>
struct EventSet {
  hipEvent_t e[N] = {};
  EventSet() = default;
  EventSet(const EventSet &) = delete;
  EventSet &operator=(const EventSet &) = delete;
  ~EventSet() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  int ensure(int n, unsigned flags = hipEventDefault) {  // the first n exist
    for (int i = 0; i < n; ++i)
      if (!e[i]) TSDF_HIP_TRY(hipEventCreateWithFlags(&e[i], flags));
    return TSDF_HIP_OK;
  }
  hipEvent_t operator[](int i) const { return e[i]; }
};

// Is `p` host memory the runtime knows as pinned?  (What PinnedStage copies directly.)
bool tsdf_is_pinned_host(const void *p);

// Copies between DEVICE memory and the CALLER's host memory, through two pinned slots of `chunk` bytes, the host memcpy of
// one chunk overlapping the DMA of the next; memory of at least 64 KiB that the runtime knows as pinned is copied directly.
// to_host returns with the data in `dst` (everything queued on `s` before it has completed); to_device returns as soon as
// `src` has been consumed, the device copy being ordered on `s` like any other work.  A slot is reused only after the event
// behind its last copy, whichever call queued it.  Defined in tsdf_core.hip.
class PinnedStage {
 public:
  explicit PinnedStage(size_t chunk) : chunk(chunk) {}
  PinnedStage(const PinnedStage &) = delete;
  PinnedStage &operator=(const PinnedStage &) = delete;
  ~PinnedStage() {
    if (slots) (void)hipHostFree(slots);
  }
  int to_host(void *dst, const void *dev_src, size_t bytes, hipStream_t s);
  int to_device(void *dev_dst, const void *src, size_t bytes, hipStream_t s);

 private:
  const size_t chunk;
  char *slots = nullptr;
  EventSet<2> ev;
  bool busy[2] = {false, false};
  unsigned turn = 0;  // slot of the next chunk: consecutive small transfers alternate instead of queueing on one slot
  int ready();
  int wait(int slot);
};
