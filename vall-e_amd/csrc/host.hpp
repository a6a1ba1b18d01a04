// Host-side support shared by the translation units of libvallex.so: error reporting, the head of a *_create, the device guard,
// VX_POISON, an owner of one device block, the staging protocol of a ragged call, the table most ragged calls stage and the lazy
// device side of a handle.  Host code only: no kernel, no kernel header.  A new handle derives from LazyDev<its Dev>, keeps a
// CallStage named `stage` and DevBufs in that Dev, opens its *_init_device with open_device, and writes its entry points as
//   create_head;  host-side checks;  ensure_device;  ON_DEVICE;  drain before a table is replaced;  begin .. upload .. kernels .. finish
// with destroy_handle as its destroy (fbank.hip is the shortest example).  A call whose per-utterance arrays are pointer columns,
// tile0 and int columns lays them out with RaggedTable.  A handle that takes weights keeps its table with weights_host.hpp.
// One handle is not lazy: vx_codec names its device in its config and makes its device side (DevBufs and a CallStage, too) at
// vx_codec_finalize; its calls run on a stream of its own, handed over from and back to the caller's around begin .. finish.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <memory>

#include "../../include/vallex.h"

// Nothing here is part of the C ABI: hidden, so the library's export list stays the header's.
namespace vx __attribute__((visibility("hidden"))) {

// Sets the thread-local message vx_last_error() returns and hands `code` back.  Defined once, in engine.hip.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3), visibility("hidden")));

#define HIPC(expr)                                                                                                        \
  do {                                                                                                                    \
    hipError_t e_ = (expr);                                                                                               \
    if (e_ != hipSuccess)                                                                                                 \
      return ::vx::fail(VX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);           \
  } while (0)
#define VXC(expr)               \
  do {                          \
    int r_ = (expr);            \
    if (r_ != VX_OK) return r_; \
  } while (0)

// The head of a *_create whose config carries its struct_size: `fn` is the entry point's name.
template <class Cfg, class Handle>
int create_head(const char* fn, const Cfg* cfg, Handle** out) {
  if (!cfg || !out) return fail(VX_ERR_ARG, "%s: null argument", fn);
  if (cfg->struct_size != (int32_t)sizeof(Cfg)) return fail(VX_ERR_ARG, "%s: struct_size %d, expected %zu", fn, cfg->struct_size, sizeof(Cfg));
  return VX_OK;
}

// Every entry point runs on its handle's device and leaves the caller's current device as it found it.
struct DevGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DevGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
    else if (err == hipSuccess) prev = -1;  // already current: nothing to restore
  }
  ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define ON_DEVICE(dev)      \
  DevGuard dev_guard_(dev); \
  HIPC(dev_guard_.err)

// VX_POISON=1 (tests): every fresh device allocation is filled with 0xFF bytes (NaN as bf16 / fp32, -1 as integers) before its
// owner initialises it, so a read of memory nothing wrote shows up as NaN output instead of depending on what the allocator
// happened to hand back.  Read once per process.
inline bool poison_on() {
  static const bool on = [] { const char* v = getenv("VX_POISON"); return v && atoi(v) != 0; }();
  return on;
}

// The caller's file and line, for the HIP calls DevBuf and CallStage make on its behalf: their failures read as HIPC's do and
// name the unit that asked, not this header.
struct Site {
  const char* file;
  int line;
  Site(const char* f = __builtin_FILE(), int l = __builtin_LINE()) : file(f), line(l) {}
  int check(hipError_t e, const char* call) const {
    return e == hipSuccess ? VX_OK : fail(VX_ERR_HIP, "%s failed: %s (%s:%d)", call, hipGetErrorString(e), file, line);
  }
};

// 0xFF over a fresh block when poison_on(); finished before the block is handed out, whatever stream uses it next.
inline int poison_fill(void* p, size_t bytes, Site at) {
  if (!poison_on()) return VX_OK;
  VXC(at.check(hipMemsetAsync(p, 0xFF, bytes, nullptr), "hipMemsetAsync"));
  return at.check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
}

// Owner of one hipMalloc block of n elements; freed on every way out of its scope.
template <typename T>
struct DevBuf {
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  int alloc(size_t n, Site at = Site()) {  // a block it already holds is freed first
    reset();
    VXC(at.check(hipMalloc((void**)&p_, n * sizeof(T)), "hipMalloc"));
    return poison_fill(p_, n * sizeof(T), at);
  }
  int upload(const T* host, size_t n, hipStream_t s, Site at = Site()) {
    return at.check(hipMemcpyAsync(p_, host, n * sizeof(T), hipMemcpyHostToDevice, s), "hipMemcpyAsync");
  }

 private:
  T* p_ = nullptr;
};

// The staging of a ragged call: the per-call arrays are written into a pinned host block and copied to its device twin on the
// caller's stream.  ev_copy: the previous call's copy out of the pinned block is done (the host may rewrite it).  ev_done: the
// previous call, on whatever stream it ran, is done with the device block and with the owner's tables and workspace.
//   per call:  begin(s);  fill host<T>();  upload(bytes, s);  kernels on s reading dev<T>();  finish(s)
struct CallStage {
  CallStage() = default;
  CallStage(const CallStage&) = delete;
  CallStage& operator=(const CallStage&) = delete;
  ~CallStage() { release(); }

  int init(size_t nbytes, Site at = Site()) {
    bytes = nbytes;
    VXC(at.check(hipMalloc((void**)&dev_, bytes), "hipMalloc"));
    VXC(poison_fill(dev_, bytes, at));
    VXC(at.check(hipHostMalloc((void**)&host_, bytes), "hipHostMalloc"));
    VXC(at.check(hipEventCreateWithFlags(&ev_copy, hipEventDisableTiming), "hipEventCreateWithFlags"));
    return at.check(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming), "hipEventCreateWithFlags");
  }
  void release() {  // safe on a half-initialised object
    if (dev_) (void)hipFree(dev_);
    if (host_) (void)hipHostFree(host_);
    if (ev_copy) (void)hipEventDestroy(ev_copy);
    if (ev_done) (void)hipEventDestroy(ev_done);
    dev_ = host_ = nullptr;
    ev_copy = ev_done = nullptr;
    bytes = 0;
  }
  int begin(hipStream_t s, Site at = Site()) {
    VXC(at.check(hipEventSynchronize(ev_copy), "hipEventSynchronize"));
    return at.check(hipStreamWaitEvent(s, ev_done, 0), "hipStreamWaitEvent");
  }
  // The host waits for the previous call: before the owner replaces a table or a workspace, and before destroy.
  int drain(Site at = Site()) { return at.check(hipEventSynchronize(ev_done), "hipEventSynchronize"); }
  int upload(size_t nbytes, hipStream_t s, Site at = Site()) {
    VXC(at.check(hipMemcpyAsync(dev_, host_, nbytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync"));
    return at.check(hipEventRecord(ev_copy, s), "hipEventRecord");
  }
  int finish(hipStream_t s, Site at = Site()) { return at.check(hipEventRecord(ev_done, s), "hipEventRecord"); }
  template <typename T> T* host(size_t byte_off = 0) const { return (T*)(host_ + byte_off); }
  template <typename T> T* dev(size_t byte_off = 0) const { return (T*)(dev_ + byte_off); }

  size_t bytes = 0;
  hipEvent_t ev_copy = nullptr, ev_done = nullptr;

 private:
  char *host_ = nullptr, *dev_ = nullptr;
};

// The block most ragged calls stage: P pointer columns [max_batch] | tile0 [max_batch + 1] | K int columns [max_batch].  The one
// place that knows the offsets; host and device accessors over the CallStage that holds the block at its start.
struct RaggedTable {
  RaggedTable(int max_batch, int n_ptr_cols, int n_int_cols) : mb_((size_t)max_batch), p_((size_t)n_ptr_cols), k_((size_t)n_int_cols) {}
  size_t bytes() const { return int_off(k_); }
  template <typename T> T* host_ptrs(const CallStage& st, int k) const { return st.host<T>(ptr_off(k)); }
  template <typename T> T* dev_ptrs(const CallStage& st, int k) const { return st.dev<T>(ptr_off(k)); }
  int* host_tile0(const CallStage& st) const { return st.host<int>(ptr_off(p_)); }
  const int* dev_tile0(const CallStage& st) const { return st.dev<const int>(ptr_off(p_)); }
  int* host_ints(const CallStage& st, int k) const { return st.host<int>(int_off(k)); }
  const int* dev_ints(const CallStage& st, int k) const { return st.dev<const int>(int_off(k)); }

 private:
  size_t ptr_off(size_t k) const { return k * mb_ * sizeof(void*); }
  size_t int_off(size_t k) const { return ptr_off(p_) + (mb_ + 1 + k * mb_) * sizeof(int); }
  size_t mb_, p_, k_;
};

// The lazy device side of a handle: nothing touches a device until the first call that needs one; that call makes `Dev` (the
// DevBufs and a CallStage named `stage`) on the device that is current then, and every later call runs there (ON_DEVICE).
template <class Dev>
struct LazyDev {
  typedef Dev dev_type;
  int device = -1;  // >= 0: `dev` is complete
  std::unique_ptr<Dev> dev;
};

// The opening of a unit's *_init_device: the current device becomes the handle's, with a fresh Dev to fill.
template <class H>
int open_device(H* h, Site at = Site()) {
  int dev = 0;
  VXC(at.check(hipGetDevice(&dev), "hipGetDevice(&dev)"));
  h->device = dev;
  h->dev.reset(new typename H::dev_type());
  return VX_OK;
}

template <class H, class Init>
int ensure_device(H* h, Init init) {
  if (h->device >= 0) return VX_OK;
  const int rc = init(h);
  if (rc != VX_OK) {  // a failed first use leaves the handle as it was before it
    h->dev.reset();
    h->device = -1;
  }
  return rc;
}

// vx_*_destroy: waits for the last call on the handle's device; a handle that never reached a device makes no HIP call.
template <class H>
void destroy_handle(H* h) {
  if (!h) return;
  if (h->device >= 0) {
    DevGuard guard(h->device);
    (void)h->dev->stage.drain();
    h->dev.reset();
  }
  delete h;
}

}  // namespace vx
