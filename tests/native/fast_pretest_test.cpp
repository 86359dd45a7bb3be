// fast_pretest_test.cpp — k_fast's 4-pixel compass pre-test (csrc/orbx_fast_pretest.h) on its
// own: no HIP, no liborbx, no GPU.  Built with -fsanitize=address,undefined
// (my_orb_slam2_amd/build.py, build_fast_pretest_test) and run by tests/test_fast_pretest.py.
//
// The closed form of the pre-test, per pixel, with x7 = x >> 1 and tb = (t + 1) >> 1:
//   bright(n) = n7 >= v7 + tb      dark(n) = n7 <= v7 - tb
//   flag = (bright(n0) || bright(n8)) && (bright(n4) || bright(n12))
//       || (dark(n0) || dark(n8)) && (dark(n4) || dark(n12))
// and the exact compass test is the same with n > v + t and n < v - t.  The pre-test must equal
// its closed form in every byte whatever the neighbouring bytes hold, and flag every pixel the
// exact test passes.
//
//   fast_pretest_test    run every check; prints "ok <name>" per check, exit 1 at the first miss
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_fast_pretest.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static bool closed(int t, int v, int n0, int n4, int n8, int n12) {
    const int tb = (t + 1) >> 1, v7 = v >> 1;
    auto br = [&](int n) { return (n >> 1) >= v7 + tb; };
    auto dk = [&](int n) { return (n >> 1) <= v7 - tb; };
    return ((br(n0) || br(n8)) && (br(n4) || br(n12))) || ((dk(n0) || dk(n8)) && (dk(n4) || dk(n12)));
}

static bool exact(int t, int v, int n0, int n4, int n8, int n12) {
    auto br = [&](int n) { return n > v + t; };
    auto dk = [&](int n) { return n < v - t; };
    return ((br(n0) || br(n8)) && (br(n4) || br(n12))) || ((dk(n0) || dk(n8)) && (dk(n4) || dk(n12)));
}

static int byte_of(uint32_t x, int j) { return (int)((x >> (8 * j)) & 0xFFu); }

static uint32_t rng_state = 0x2545F491u;
static uint32_t rng() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

// The flags of one call against the closed form of each of its four bytes.
static void check_dwords(int t, uint32_t V, uint32_t N0, uint32_t N4, uint32_t N8, uint32_t N12) {
    const uint32_t f = orbx::pt_flags(orbx::pt_h(V), orbx::pt_h(N0), orbx::pt_h(N4), orbx::pt_h(N8),
                                      orbx::pt_h(N12), orbx::pt_T(t), orbx::pt_T1(t));
    for (int j = 0; j < 4; ++j) {
        const int v = byte_of(V, j), n0 = byte_of(N0, j), n4 = byte_of(N4, j), n8 = byte_of(N8, j),
                  n12 = byte_of(N12, j);
        const bool got = (f >> (8 * j + 7)) & 1u;
        if (got != closed(t, v, n0, n4, n8, n12) || (exact(t, v, n0, n4, n8, n12) && !got)) {
            std::printf("FAIL t=%d byte %d: v=%d n0=%d n4=%d n8=%d n12=%d flag=%d\n", t, j, v, n0, n4,
                        n8, n12, (int)got);
            std::exit(1);
        }
    }
}

// Every t, every (v, n): the neighbours of subset s hold n, the others v (which never passes).
// Four values of n share a dword, so neighbouring bytes differ.
static void test_all_byte_pairs() {
    for (int t = 1; t <= 255; ++t)
        for (int v = 0; v < 256; ++v) {
            const uint32_t V = (uint32_t)v * orbx::PT_ONES;
            for (int n = 0; n < 256; n += 4) {
                // bytes n, n + 1, n + 2, n + 3 rotated by v so every value meets every byte
                const int r = v & 3;
                uint32_t N = 0;
                for (int j = 0; j < 4; ++j) N |= (uint32_t)(n + ((j + r) & 3)) << (8 * j);
                const int s = (v + (n >> 2) + t) & 15;
                const int subsets[4] = {15, s, 5, 10};   // all; a varying one; {n0, n8}; {n4, n12}
                for (int k = 0; k < 4; ++k) {
                    const int m = subsets[k];
                    check_dwords(t, V, m & 1 ? N : V, m & 2 ? N : V, m & 4 ? N : V, m & 8 ? N : V);
                }
            }
        }
    std::puts("ok all_byte_pairs");
}

// Random dwords, and dwords mixing 0 / 255 / t-boundary bytes in adjacent positions: nothing
// crosses a byte.
static void test_no_byte_crossing() {
    const int ts[] = {1, 2, 7, 20, 100, 127, 128, 254, 255};
    for (int t : ts) {
        for (int i = 0; i < 200000; ++i) check_dwords(t, rng(), rng(), rng(), rng(), rng());
        for (int i = 0; i < 200000; ++i) {
            uint32_t w[5];
            const int v = (int)(rng() & 0xFF);
            for (int k = 0; k < 5; ++k) {
                w[k] = 0;
                for (int j = 0; j < 4; ++j) {
                    int b;
                    switch (rng() % 6) {
                        case 0: b = 0; break;
                        case 1: b = 255; break;
                        case 2: b = v; break;
                        case 3: b = v + t + (int)(rng() % 5) - 2; break;
                        case 4: b = v - t + (int)(rng() % 5) - 2; break;
                        default: b = (int)(rng() & 1) ? 1 : 254; break;
                    }
                    b = b < 0 ? 0 : b > 255 ? 255 : b;
                    w[k] |= (uint32_t)b << (8 * j);
                }
            }
            check_dwords(t, w[0], w[1], w[2], w[3], w[4]);
        }
    }
    std::puts("ok no_byte_crossing");
}

// pt_unit on three image rows: bit i is the closed form of pixel i, with the +-3 pixel
// neighbours taken across the dword boundaries.
template <int DW>
static void test_unit(const char* name) {
    const int ts[] = {1, 7, 20, 255};
    std::vector<uint8_t> c(4 * (DW + 2)), d(4 * DW), u(4 * DW);   // exact sizes: ASan sees overreads
    std::vector<uint32_t> C(DW + 2), D(DW), U(DW);
    for (int t : ts)
        for (int it = 0; it < 100000; ++it) {
            const int base = (int)(rng() & 0xFF), amp = (it & 1) ? t + 3 : 255;
            auto px = [&]() {
                const int b = base + (int)(rng() % (2 * amp + 1)) - amp;
                return (uint8_t)(b < 0 ? 0 : b > 255 ? 255 : b);
            };
            for (auto& x : c) x = px();
            for (auto& x : d) x = px();
            for (auto& x : u) x = px();
            auto pack = [](const std::vector<uint8_t>& b, std::vector<uint32_t>& w) {
                for (size_t i = 0; i < w.size(); ++i)
                    w[i] = b[4 * i] | b[4 * i + 1] << 8 | b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
            };
            pack(c, C); pack(d, D); pack(u, U);
            const uint32_t m = orbx::pt_unit<DW>(C.data(), D.data(), U.data(), orbx::pt_T(t), orbx::pt_T1(t));
            CHECK((m >> (4 * DW)) == 0);
            for (int i = 0; i < 4 * DW; ++i) {
                const int v = c[4 + i], n0 = d[i], n8 = u[i], n4 = c[4 + i + 3], n12 = c[4 + i - 3];
                const bool got = (m >> i) & 1u;
                CHECK(got == closed(t, v, n0, n4, n8, n12));
                CHECK(got || !exact(t, v, n0, n4, n8, n12));
            }
        }
    std::printf("ok %s\n", name);
}

static void test_gather() {
    for (int a = 0; a < 256; ++a) {
        uint32_t f0 = 0x7F7F7F7Fu & rng(), f1 = 0x7F7F7F7Fu & rng();   // the other bits are noise
        for (int j = 0; j < 4; ++j) {
            f0 |= (uint32_t)((a >> j) & 1) << (8 * j + 7);
            f1 |= (uint32_t)((a >> (4 + j)) & 1) << (8 * j + 7);
        }
        CHECK(orbx::pt_gather2(f0, f1) == (uint32_t)a);
    }
    std::puts("ok gather");
}

int main() {
    test_gather();
    test_all_byte_pairs();
    test_no_byte_crossing();
    test_unit<4>("unit4");
    test_unit<2>("unit2");
    test_unit<1>("unit1");
    std::puts("all ok");
    return 0;
}
