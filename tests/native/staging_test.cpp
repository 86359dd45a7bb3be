// staging_test.cpp — the staging plan of the host-array entry points (csrc/orbx_stage.h) on its
// own: no HIP, no liborbx, no GPU.  Built with -fsanitize=address,undefined
// (my_orb_slam2_amd/build.py, build_staging_test) and run by tests/test_staging_plan.py.
//
// Every expectation is worked out here with plain arithmetic, not read back from the plan.  The
// "device" is a second host array that moves the two spans as HostCall does.
//
//   staging_test          run every check; prints "ok <name>" per check, exit 1 at the first miss
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_stage.h"

using orbx::StagePlan;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// what HostCall::upload() / finish() move, between the plan's block and a stand-in device block
static void move_up(const StagePlan& p, std::vector<uint8_t>& dev) {
    dev.assign(p.end, 0xEE);   // what a part that never went up looks like
    if (p.up_hi > p.up_lo) std::memcpy(dev.data() + p.up_lo, p.block.data() + p.up_lo, p.up_hi - p.up_lo);
}
static void move_down(StagePlan& p, const std::vector<uint8_t>& dev) {
    if (p.dn_hi > p.dn_lo) std::memcpy(p.block.data() + p.dn_lo, dev.data() + p.dn_lo, p.dn_hi - p.dn_lo);
}

static void test_alignment() {
    const size_t sizes[5] = {0, 1, 255, 256, 257};
    const size_t start[5] = {0, 0, 256, 512, 768};   // 0 + 0, + 256, + 256, + 256; then + 512
    std::vector<uint8_t> src(257, 0x5A);
    StagePlan p;
    p.reset();
    for (int kind = 0; kind < 4; ++kind) {   // the same sizes as in, inout, out and scratch parts
        const size_t base = 1280 * (size_t)kind;
        for (int i = 0; i < 5; ++i) {
            std::vector<uint8_t> io(sizes[i] + 1, 0x11);
            const size_t o = kind == 0   ? p.in(src.data(), sizes[i])
                             : kind == 1 ? p.inout(io.data(), sizes[i])
                             : kind == 2 ? p.out(nullptr, sizes[i])
                                         : p.scratch(sizes[i]);
            CHECK(o == base + start[i]);
            CHECK(o % 256 == 0);
            CHECK(p.end == o + up256(sizes[i]));   // the next part starts behind this one
        }
    }
    CHECK(p.end == 4 * 1280);
    std::puts("ok alignment");
}

static void test_absent() {
    StagePlan p;
    p.reset();
    const uint8_t one = 7;
    const size_t a = p.in(&one, 1);
    const size_t before = p.end;
    const size_t skip = p.in_opt(nullptr, 100);
    CHECK(skip == StagePlan::NONE);
    CHECK(p.end == before && p.up_hi == 256);   // occupies nothing
    uint8_t dev[512];
    CHECK(StagePlan::dev<uint8_t>(skip, dev) == nullptr);
    CHECK(StagePlan::dev<uint8_t>(a, dev) == dev);
    const size_t given = p.in_opt(&one, 1);
    CHECK(given == 256 && StagePlan::dev<uint8_t>(given, dev) == dev + 256);
    // a null source of an ordinary in part is zeros, not absent
    const size_t z = p.in(nullptr, 3);
    CHECK(z == 512 && p.host<uint8_t>(z)[0] == 0 && p.host<uint8_t>(z)[2] == 0);
    std::puts("ok absent");
}

// parts of 300 (in), 10 (inout), 600 (out), 4 (zeroed out), 1000 (scratch) bytes in `order`
static void spans_case(const int order[5], const char* name) {
    const size_t bytes[5] = {300, 10, 600, 4, 1000};
    uint8_t src[300], io[10], dst[600];
    std::memset(src, 1, sizeof(src));
    std::memset(io, 2, sizeof(io));
    StagePlan p;
    p.reset();
    size_t off[5], expect = 0;
    size_t up_lo = SIZE_MAX, up_hi = 0, dn_lo = SIZE_MAX, dn_hi = 0;
    for (int k = 0; k < 5; ++k) {
        const int part = order[k];
        off[part] = part == 0   ? p.in(src, 300)
                    : part == 1 ? p.inout(io, 10)
                    : part == 2 ? p.out(dst, 600)
                    : part == 3 ? p.out(nullptr, 4, true)
                                : p.scratch(1000);
        CHECK(off[part] == expect);
        const size_t lo = expect, hi = expect + up256(bytes[part]);
        expect = hi;
        if (part == 0 || part == 1 || part == 3) up_lo = lo < up_lo ? lo : up_lo, up_hi = hi > up_hi ? hi : up_hi;
        if (part == 1 || part == 2 || part == 3) dn_lo = lo < dn_lo ? lo : dn_lo, dn_hi = hi > dn_hi ? hi : dn_hi;
    }
    CHECK(p.end == expect);
    CHECK(p.up_lo == up_lo && p.up_hi == up_hi);
    CHECK(p.dn_lo == dn_lo && p.dn_hi == dn_hi);
    // every part that has to move lies inside its span, and the block holds both spans
    CHECK(p.block.size() >= up_hi && p.block.size() >= dn_hi);
    std::printf("ok spans %s\n", name);
}

static void test_spans() {
    const int canonical[5] = {0, 1, 2, 3, 4}, shuffled[5] = {2, 4, 0, 3, 1};
    spans_case(canonical, "canonical");
    // in the canonical order both spans are tight and the scratch lies outside them:
    // in [0, 512), inout [512, 768), out [768, 1536), zeroed [1536, 1792), scratch [1792, 2816)
    {
        uint8_t src[300] = {0}, io[10] = {0}, dst[600];
        StagePlan p;
        p.reset();
        p.in(src, 300), p.inout(io, 10), p.out(dst, 600), p.out(nullptr, 4, true);
        const size_t s = p.scratch(1000);
        CHECK(p.up_lo == 0 && p.up_hi == 1792 && p.dn_lo == 512 && p.dn_hi == 1792);
        CHECK(s == 1792 && s >= p.up_hi && s >= p.dn_hi && p.end == 2816);
        CHECK(p.block.size() == 1792);   // no host bytes for the trailing scratch
    }
    spans_case(shuffled, "shuffled");
    std::puts("ok spans");
}

static void test_copy_out() {
    // destinations with 16 guard bytes on both sides
    struct Guarded {
        std::vector<uint8_t> v;
        size_t n;
        explicit Guarded(size_t bytes) : v(bytes + 32, 0xC3), n(bytes) {}
        uint8_t* p() { return v.data() + 16; }
        bool guards() const {
            for (size_t i = 0; i < 16; ++i)
                if (v[i] != 0xC3 || v[16 + n + i] != 0xC3) return false;
            return true;
        }
        bool all(uint8_t b) const {
            for (size_t i = 0; i < n; ++i)
                if (v[16 + i] != b) return false;
            return true;
        }
    };
    for (int ok = 1; ok >= 0; --ok) {
        Guarded a(257), b(1), io(5);
        StagePlan p;
        p.reset();
        const size_t pio = p.inout(io.p(), 5), pa = p.out(a.p(), 257), pb = p.out(b.p(), 1),
                     pt = p.out(nullptr, 8);   // read through host<T>() only: no copy-out
        std::vector<uint8_t> dev;
        move_up(p, dev);
        CHECK(std::memcmp(dev.data() + pio, io.p(), 5) == 0);
        std::memset(dev.data() + pio, 0x21, 256);   // the "kernel" fills whole parts
        std::memset(dev.data() + pa, 0x22, 512);
        std::memset(dev.data() + pb, 0x23, 256);
        std::memset(dev.data() + pt, 0x24, 256);
        move_down(p, dev);
        p.copy_out(ok != 0);
        CHECK(a.guards() && b.guards() && io.guards());
        if (ok) {
            CHECK(io.all(0x21) && a.all(0x22) && b.all(0x23));
            CHECK(p.host<uint8_t>(pt)[0] == 0x24 && p.host<uint8_t>(pt)[7] == 0x24);
        } else {
            CHECK(io.all(0xC3) && a.all(0xC3) && b.all(0xC3));   // nothing after a failure
        }
    }
    std::puts("ok copy_out");
}

static void test_block_reuse() {
    StagePlan p;
    std::vector<uint8_t> dev;
    // first call: an inout part no kernel touches returns the caller's bytes
    uint8_t io[7] = {9, 8, 7, 6, 5, 4, 3}, want[7];
    std::memcpy(want, io, 7);
    uint8_t res[300];
    p.reset();
    p.inout(io, 7);
    const size_t r1 = p.out(res, 300);
    move_up(p, dev);
    CHECK(dev[r1] == 0xEE);   // an out part is not uploaded unless asked
    std::memset(dev.data() + r1, 0x77, 300);
    move_down(p, dev);
    std::memset(io, 0, 7);    // whatever the caller's array held, the block's bytes come back
    p.copy_out(true);
    CHECK(std::memcmp(io, want, 7) == 0);
    CHECK(res[0] == 0x77 && res[299] == 0x77);
    const size_t size1 = p.block.size();
    CHECK(size1 == 256 + 512);

    // a second, larger call on the same block grows it and keeps working
    std::vector<uint8_t> big(5000, 0x42), bigout(5000, 0);
    p.reset();
    const size_t b_in = p.in(big.data(), 5000), b_out = p.out(bigout.data(), 5000, true);
    CHECK(b_in == 0 && b_out == 5120 && p.end == 10240 && p.block.size() == 10240);
    CHECK(p.outs.size() == 1);   // the first call's copy-outs are gone
    move_up(p, dev);
    CHECK(dev[4999] == 0x42 && dev[b_out] == 0 && dev[b_out + 4999] == 0);   // zeroed: went up as zeros
    std::memset(dev.data() + b_out, 0x55, 5120);
    move_down(p, dev);
    p.copy_out(true);
    CHECK(bigout[0] == 0x55 && bigout[4999] == 0x55);

    // a later, smaller call reuses it: the out part reads zeros, not the previous call's 0x42 / 0x55
    uint8_t small_out[100];
    std::memset(small_out, 0xAB, sizeof(small_out));
    p.reset();
    const size_t s_out = p.out(small_out, 100);
    const size_t s_in = p.in(nullptr, 50);
    CHECK(p.block.size() == 10240);   // only grows
    for (size_t i = 0; i < 256; ++i) CHECK(p.host<uint8_t>(s_out)[i] == 0 && p.host<uint8_t>(s_in)[i] == 0);
    p.copy_out(true);         // with nothing moved, the caller gets those zeros
    for (size_t i = 0; i < 100; ++i) CHECK(small_out[i] == 0);
    std::puts("ok block_reuse");
}

int main() {
    test_alignment();
    test_absent();
    test_spans();
    test_copy_out();
    test_block_reuse();
    std::puts("all ok");
    return 0;
}
