// orbx_layout.h — byte layouts of the extractor's output blocks, device and pinned alike (no HIP:
// also compiled on its own by tests/native/layout_test.cpp).  Every part starts 256-aligned.
#pragma once
#include <stddef.h>

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

}  // namespace orbx
