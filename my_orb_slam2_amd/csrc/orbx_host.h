// orbx_host.h — host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

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

// Offsets inside one staging block: every part starts on a 256-byte boundary.
__host__ __device__ inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Layout {
    size_t end = 0;
    size_t add(size_t bytes) {   // the offset of a part of `bytes` bytes, put behind the last one
        const size_t o = end;
        end += al256(bytes);
        return o;
    }
};

// (int) of a double as x86-64 converts it (cvttsd2si; cvttss2si for a widened float): NaN and
// everything outside int's range give INT_MIN
inline int cvtt(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN; }

// Device staging of the host-array entry points: a pool of (device, non-blocking stream,
// growable buffer) slots taken for the length of one call.  After warm-up a call allocates
// nothing, and it waits only for its own stream, never for the device (the reference calls
// these from the Tracking thread while LocalMapping / LoopClosing run matchers).  The pool is
// defined in orbx_frame.hip; slots live for the process (no teardown-order hazards).
struct Scratch {
    int device = -1;
    hipStream_t st = nullptr;
    DevBuf buf;
};
struct ScratchLease {
    Scratch* s = nullptr;                  // nullptr: no stream could be created
    explicit ScratchLease(int device);     // the calling thread's current device is `device`
    ~ScratchLease();
    ScratchLease(const ScratchLease&) = delete;
    ScratchLease& operator=(const ScratchLease&) = delete;
};

}  // namespace orbx
