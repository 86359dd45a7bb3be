// orbx_stage.h — the staging plan of one host-array call: pure host code, no HIP include.
//
// A plan owns a growable host block that mirrors the call's device block.  A part is its offset
// in both (always a multiple of 256); NONE is an absent optional part.  Declare the parts, fill
// what the entry point composes itself through host<T>(), move [up_lo, up_hi) up and
// [dn_lo, dn_hi) down (orbx_host.h, HostCall), then copy_out().
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace orbx {

struct StagePlan {
    static constexpr size_t NONE = ~(size_t)0;
    // every part starts on a 256-byte boundary
    static size_t align(size_t v) { return (v + 255) & ~(size_t)255; }
    std::vector<uint8_t> block;     // only grows; holds every part but trailing scratch
    size_t end = 0;                 // the size of the device block
    size_t up_lo = 0, up_hi = 0;    // smallest range over the in / inout parts and zeroed words
    size_t dn_lo = 0, dn_hi = 0;    // smallest range over the inout / out parts
    struct CopyOut { size_t part; void* dst; size_t bytes; };
    std::vector<CopyOut> outs;

    void reset() {
        end = up_lo = up_hi = dn_lo = dn_hi = 0;
        outs.clear();
    }
    // `src` (zeros when null) as a part of `bytes` bytes
    size_t in(const void* src, size_t bytes) { return add(src, bytes, nullptr, true, false); }
    // as in(), but a null `src` is an absent part: dev() gives nullptr and nothing is occupied
    size_t in_opt(const void* src, size_t bytes) { return src ? in(src, bytes) : NONE; }
    // goes up as the caller passed it and comes back to `p`
    size_t inout(void* p, size_t bytes) { return add(p, bytes, p, true, true); }
    // zero in the block; comes back to `dst`, or to the block alone (host<T>()) when null.
    // zeroed: the device must see the zeros too (a word a kernel only accumulates into)
    size_t out(void* dst, size_t bytes, bool zeroed = false) {
        return add(nullptr, bytes, dst, zeroed, true);
    }
    // device only: neither copied nor zeroed
    size_t scratch(size_t bytes) {
        const size_t o = end;
        end += align(bytes);
        return o;
    }
    // host<T>() holds until the next part is declared (the block may move when it grows)
    template <class T> T* host(size_t part) { return (T*)(block.data() + part); }
    template <class T> static T* dev(size_t part, void* base) {
        return part == NONE ? nullptr : (T*)((uint8_t*)base + part);
    }
    // the downloaded parts to their callers; nothing after a failure
    void copy_out(bool ok) {
        if (!ok) return;
        for (const CopyOut& c : outs) std::memcpy(c.dst, block.data() + c.part, c.bytes);
    }

  private:
    static void cover(size_t& lo, size_t& hi, size_t a, size_t b) {
        if (a == b) return;
        if (lo == hi) lo = a, hi = b;
        else lo = a < lo ? a : lo, hi = b > hi ? b : hi;
    }
    size_t add(const void* src, size_t bytes, void* dst, bool up, bool down) {
        const size_t o = scratch(bytes);
        if (block.size() < end) block.resize(end);
        if (src && bytes) std::memcpy(block.data() + o, src, bytes);
        else if (end > o) std::memset(block.data() + o, 0, end - o);
        if (up) cover(up_lo, up_hi, o, end);
        if (down) cover(dn_lo, dn_hi, o, end);
        if (dst && bytes) outs.push_back({o, dst, bytes});
        return o;
    }
};

}  // namespace orbx
