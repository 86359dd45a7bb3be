// layout_test.cpp — the output-block layouts of the extractor (csrc/orbx_layout.h) on their own:
// no HIP, no liborbx, no GPU.  Built with -fsanitize=address,undefined
// (my_orb_slam2_amd/build.py, build_layout_test) and run by tests/test_layout.py.
//
// The expressions the host code spelled out at each use before the header existed are restated
// here literally; the header must give the same numbers, since the graph keys and the DMA sizes
// depend on them.
//
//   layout_test          run every check; prints "ok <name>" per check, exit 1 at the first miss
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include "orbx_layout.h"

using orbx::OutLayout;
using orbx::StereoLayout;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static const size_t BS[5] = {1, 2, 3, 16, 512};
static const size_t KCS[5] = {1, 63, 64, 2000, 32767};
static const size_t FS_MAX_FRAMES = 8;

static void test_keypoint_size() {
    CHECK(sizeof(orbx_keypoint) == 28);   // what the served copy used to hard-code
    std::puts("ok keypoint_size");
}

// ensure_workspace: [nkp[B] | kps[B][KC] | desc[B][KC][32]], then one pair's stereo block
static void test_workspace() {
    for (size_t B : BS)
        for (size_t KC : KCS) {
            const size_t o_kps = align_up(B * 4, 256);
            const size_t o_desc = o_kps + align_up(B * KC * sizeof(orbx_keypoint), 256);
            const size_t o_end = o_desc + B * KC * 32;
            const size_t o_stereo = align_up(o_end, 256);
            const size_t total = o_stereo + 256 + 8 * KC;
            const OutLayout L(B, KC);
            CHECK(L.B == B && L.KC == KC);
            CHECK(L.o_kps == o_kps);
            CHECK(L.o_desc == o_desc);
            CHECK(L.kps_end(B) == o_kps + B * KC * sizeof(orbx_keypoint));
            CHECK(L.desc_end(B) == o_end);
            CHECK(L.after(B) == o_stereo);
            CHECK(L.after(B) + StereoLayout(1, KC).end == total);
            // a lone image's and a stereo frame's DMA ends (extract_host, stereo_frame_solo)
            CHECK(L.desc_end(1) == o_desc + KC * 32);
            if (B >= 2) CHECK(L.desc_end(2) == o_desc + 2 * KC * 32);
            // image i's keypoints and descriptors
            for (size_t i = 0; i < B && i < 4; ++i) {
                CHECK(L.kps_end(i) == o_kps + i * KC * sizeof(orbx_keypoint));
                CHECK(L.desc_end(i) == o_desc + i * KC * 32);
            }
            // the parts do not overlap and start 256-aligned
            CHECK(B * 4 <= L.o_kps);
            CHECK(L.kps_end(B) <= L.o_desc);
            CHECK(L.desc_end(B) <= L.after(B));
            CHECK(L.o_kps % 256 == 0 && L.o_desc % 256 == 0 && L.after(B) % 256 == 0);
        }
    std::puts("ok workspace");
}

// one pair (stereo_frame_solo, orbx_stereo_match): so_u = 256, so_d = 256 + 4 KC
static void test_stereo_one_pair() {
    for (size_t KC : KCS) {
        const size_t so_u = 256, so_d = 256 + 4 * KC, s_end = so_d + KC * 4;
        const StereoLayout S(1, KC);
        CHECK(S.o_u == so_u);
        CHECK(S.o_d == so_d);
        CHECK(S.end == s_end);
        CHECK(S.end == 256 + 8 * KC);   // as ensure_workspace sized it
    }
    std::puts("ok stereo_one_pair");
}

// m pairs (run_served, copy_served): [nvalid[m] | uRight[m][KC] | depth[m][KC]]
static void test_stereo_batch() {
    for (size_t KC : KCS)
        for (size_t m = 1; m <= 8; ++m) {
            const size_t so_u = align_up(4 * m, 256), so_d = so_u + m * KC * 4;
            const size_t s_end = so_d + m * KC * 4;
            const StereoLayout S(m, KC);
            CHECK(S.o_u == so_u);
            CHECK(S.o_d == so_d);
            CHECK(S.end == s_end);
            CHECK(4 * m <= S.o_u);              // the counts end before uRight begins,
            CHECK(S.o_u + m * KC * 4 <= S.o_d); // uRight before depth
            CHECK(S.o_u % 256 == 0);
            CHECK(S.o_u == 256);                // align_up(4 m, 256) for every m the server forms
        }
    std::puts("ok stereo_batch");
}

// the frame server's blocks: the server handle's workspace (B = 2 FS_MAX_FRAMES), the stereo
// block of a batch of m behind its 2m images, both sized for the largest batch
static void test_server() {
    const size_t B = 2 * FS_MAX_FRAMES;
    for (size_t KC : KCS) {
        const OutLayout L(B, KC);
        const size_t o_desc = L.o_desc;
        const size_t s_max = align_up(4 * FS_MAX_FRAMES, 256) + 8 * FS_MAX_FRAMES * KC;
        const size_t o_max = align_up(o_desc + 2 * FS_MAX_FRAMES * KC * 32, 256);
        CHECK(StereoLayout(FS_MAX_FRAMES, KC).end == s_max);
        CHECK(L.after(2 * FS_MAX_FRAMES) == o_max);
        for (size_t m = 1; m <= 8; ++m) {
            const size_t o_end = o_desc + 2 * m * KC * 32;
            const size_t o_st = align_up(o_end, 256);
            CHECK(L.desc_end(2 * m) == o_end);
            CHECK(L.after(2 * m) == o_st);
            CHECK(L.kps_end(2 * m) <= L.o_desc);
            CHECK(o_st % 256 == 0);
            CHECK(o_st <= o_max && StereoLayout(m, KC).end <= s_max);   // inside the pinned block
        }
    }
    std::puts("ok server");
}

int main() {
    test_keypoint_size();
    test_workspace();
    test_stereo_one_pair();
    test_stereo_batch();
    test_server();
    std::puts("all ok");
    return 0;
}
