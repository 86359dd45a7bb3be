// orbx_layout.h — byte layouts of the extractor's output blocks, device and pinned alike (no HIP:
// also compiled on its own by tests/native/layout_test.cpp).  Every part starts 256-aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/orbx.h"

namespace orbx {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The extraction outputs of a workspace of B images, KC keypoint slots each:
//   [nkp[B] | kps[B][KC] | desc[B][KC][32]]
// One DMA of [0, desc_end(1)) returns a lone image's results.
struct OutLayout {
    size_t B, KC, o_kps, o_desc;
    OutLayout(size_t b = 0, size_t kc = 0)
        : B(b), KC(kc), o_kps(align_up(b * 4, 256)),
          o_desc(o_kps + align_up(b * kc * sizeof(orbx_keypoint), 256)) {}
    // where the first n images' keypoints / descriptors end, i.e. where image n's begin
    size_t kps_end(size_t n) const { return o_kps + n * KC * sizeof(orbx_keypoint); }
    size_t desc_end(size_t n) const { return o_desc + n * KC * 32; }
    // the aligned offset behind n images' descriptors: a stereo block goes there
    size_t after(size_t n) const { return align_up(desc_end(n), 256); }
};

// The stereo outputs of m pairs: [nvalid[m] | uRight[m][KC] | depth[m][KC]]
struct StereoLayout {
    size_t o_u, o_d, end;
    StereoLayout(size_t m = 0, size_t kc = 0)
        : o_u(align_up(4 * m, 256)), o_d(o_u + m * kc * 4), end(o_d + m * kc * 4) {}
};

// k_octree's dynamic LDS for node lists of up to ncap nodes and candidate arrays of kcap keys:
// every region's byte offset from the base (each 16-aligned) and the size to launch with.  The
// kernel builds its pointers from it and the plan sizes kcap and the launch from it.  (constexpr:
// the one definition serves the host, the device and a plain C++ program.)
//   tmp | sortb | node lists A, B | cpos | npos | pord | pre | pre2 | cc | kdata | knode
// The child counts cc come last but the candidate arrays, for the one overlap: candidates in LDS
// (ncand <= kcap) take [ncap][2] packed or [ncap][4] wide counts, then kdata and knode; candidates
// in global scratch take the wide counts whatever `packed` says, which then run on over the unused
// kdata / knode.  `bytes` holds the longer of the two.
struct OctreeCarve {
    static constexpr int TMP_INTS = 224;          // scan scratch + scalars, phase 2's bucket arrays
    enum { X0, Y0, X1, Y1, CNT, SEQ, NODE_ARRAYS };   // a node list: four i16 and two i32 arrays
    uint32_t tmp = 0, sortb = 0, node[2][NODE_ARRAYS] = {}, cpos = 0, npos = 0, pord = 0, pre = 0,
             pre2 = 0, cc = 0, kdata = 0, knode = 0;
    size_t bytes = 0;
    constexpr OctreeCarve(int ncap, int kcap, bool packed) {
        const uint32_t n = (uint32_t)ncap, k = (uint32_t)kcap;
        uint32_t np2 = 1, p = 0;
        while (np2 < n) np2 <<= 1;
        tmp = take(p, TMP_INTS * 4);
        sortb = take(p, np2 * 8);                 // u64 sort keys, a power of two of them
        for (int l = 0; l < 2; ++l)
            for (int a = 0; a < NODE_ARRAYS; ++a) node[l][a] = take(p, n * (a < CNT ? 2 : 4));
        cpos = take(p, n * 8);                    // i16 [ncap][4]
        npos = take(p, n * 2); pord = take(p, n * 2);
        pre = take(p, n * 4); pre2 = take(p, n * 4);
        cc = take(p, n * (packed ? 8 : 16));
        kdata = take(p, k * 4); knode = take(p, k * 2);
        uint32_t wide = cc;                       // where the global-scratch path's counts end
        take(wide, n * 16);
        bytes = p > wide ? p : wide;
    }

private:
    static constexpr uint32_t take(uint32_t& p, uint32_t b) {
        const uint32_t at = p;
        p += (b + 15) & ~15u;
        return at;
    }
};

}  // namespace orbx
