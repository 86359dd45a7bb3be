// orbx_host.h — host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

#include "../../include/orbx.h"
#include "orbx_stage.h"

#define ORBX_MAX_DEVICES 64  // per-device kernel attribute caches (prepare_kernels, kfdb)

namespace orbx {

// Text of the first failing HIP call on this thread (orbx_last_error()).
extern thread_local char g_err[256];
// Records a failing HIP call into g_err; returns e == hipSuccess.
bool hip_ok(hipError_t e, const char* what);
#define HIPOK(call) ::orbx::hip_ok((call), #call)

// A growable device allocation (contents are not preserved across growth), or a view of
// part of another one (view(): never freed through this object).
struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
    bool own = true;
    void release() {
        if (p && own) (void)hipFree(p);
        p = nullptr;
        n = 0;
        own = true;
    }
    void view(void* base, size_t bytes) {
        release();
        p = base;
        n = bytes;
        own = false;
    }
    bool ensure(size_t bytes) {
        if (bytes <= n && p && own) return true;
        release();
        if (bytes == 0) bytes = 16;
        if (!HIPOK(hipMalloc(&p, bytes))) { p = nullptr; return false; }
        n = bytes;
        return true;
    }
    template <class T> T* as() const { return (T*)p; }
};

// Sizes inside a device block, rounded as StagePlan rounds its parts (also used on the device).
__host__ __device__ inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// Device staging of the host-array entry points: a pool of (device, non-blocking stream,
// growable device buffer, staging plan) slots taken for the length of one call.  After warm-up a
// call allocates nothing, and it waits only for its own stream, never for the device (the
// reference calls these from the Tracking thread while LocalMapping / LoopClosing run matchers).
// The pool is defined in orbx_host.hip; slots live for the process (no teardown-order hazards).
struct Scratch {
    int device = -1;
    hipStream_t st = nullptr;
    DevBuf buf;
    StagePlan plan;
};
struct ScratchLease {
    Scratch* s = nullptr;     // nullptr: `device` is out of range or no stream could be created
    // makes `device` the calling thread's current device first
    explicit ScratchLease(int device);
    ~ScratchLease();
    ScratchLease(const ScratchLease&) = delete;
    ScratchLease& operator=(const ScratchLease&) = delete;
};

// One host-array call: makes `device` current, leases a slot, and moves the plan's two spans
// with one copy each.  An entry point checks its arguments, declares its parts on plan(), calls
// upload(), hands dev<T>() pointers and st() to the device form and returns finish(status).
// Large strided images bypass the host block: a scratch part and a hipMemcpy2DAsync on st().
class HostCall {
  public:
    explicit HostCall(int device) : lease_(device) {
        if (lease_.s) lease_.s->plan.reset();
    }
    bool ok() const { return lease_.s; }   // else the entry point returns ORBX_ERR_DEVICE
    StagePlan& plan() { return lease_.s->plan; }
    hipStream_t st() const { return lease_.s->st; }
    // sizes the device block and sends the upload span; false (recorded) on failure
    bool upload();
    template <class T> T* dev(size_t part) { return StagePlan::dev<T>(part, base_); }
    // status still ORBX_OK: fetches the download span.  Always drains the stream, so a slot never
    // returns to the pool with work in flight; then the copy-outs, on success only.
    orbx_status finish(orbx_status status);

  private:
    ScratchLease lease_;
    void* base_ = nullptr;
};

}  // namespace orbx
