// layout_test.cpp — the output-block layouts of the extractor and k_octree's LDS carve
// (csrc/orbx_layout.h) on their own: no HIP, no liborbx, no GPU.  Built with -fsanitize=address,undefined
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
#include <vector>

#include "orbx_layout.h"

using orbx::OctreeCarve;
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

// k_octree's LDS (OctreeCarve): the size as the host's octree_lds_bytes spelled it and the
// offsets as the kernel's take() sequence gave them, both restated literally from the code that
// kept them apart; every region 16-aligned, and disjoint but for the one stated overlap (the
// global-scratch path's wide child counts run on over kdata / knode).
static size_t parent_octree_lds_bytes(int ncap, int kcap, bool packed) {
    auto r = [](size_t b) { return (b + 15) & ~(size_t)15; };
    int np2 = 1;
    while (np2 < ncap) np2 <<= 1;
    size_t s = r(224 * 4) + r((size_t)np2 * 8);
    s += 2 * (4 * r((size_t)ncap * 2) + 2 * r((size_t)ncap * 4));
    s += r((size_t)ncap * 8) + 2 * r((size_t)ncap * 2) + 2 * r((size_t)ncap * 4);
    // the LDS path's packed counts + candidates, or the global path's wide counts
    const size_t lds_path = r((size_t)ncap * (packed ? 8 : 16)) + r((size_t)kcap * 4) + r((size_t)kcap * 2);
    const size_t glb_path = r((size_t)ncap * 16);
    return s + (lds_path > glb_path ? lds_path : glb_path);
}

static void test_octree_carve() {
    struct Region { size_t at, bytes; };
    static const int NCAPS[6] = {16, 112, 128, 256, 2016, 8192};
    static const int KCAPS[3] = {64, 1536, 8192};
    for (int NCAP : NCAPS)
        for (int KCAP : KCAPS)
            for (int packed = 0; packed < 2; ++packed) {
                // the kernel's carve, as it stood
                std::vector<Region> regs;
                size_t p = 0;
                auto take = [&](size_t bytes) {
                    size_t r = p; p += (bytes + 15) & ~(size_t)15;
                    regs.push_back({r, bytes});
                    return r;
                };
                int NP2 = 1;
                while (NP2 < NCAP) NP2 <<= 1;
                const size_t tmp = take(224 * sizeof(int));
                const size_t sortb = take((size_t)NP2 * 8);
                const size_t A_x0 = take(NCAP * 2), A_y0 = take(NCAP * 2);
                const size_t A_x1 = take(NCAP * 2), A_y1 = take(NCAP * 2);
                const size_t A_cnt = take(NCAP * 4), A_seq = take(NCAP * 4);
                const size_t B_x0 = take(NCAP * 2), B_y0 = take(NCAP * 2);
                const size_t B_x1 = take(NCAP * 2), B_y1 = take(NCAP * 2);
                const size_t B_cnt = take(NCAP * 4), B_seq = take(NCAP * 4);
                const size_t cpos = take((size_t)NCAP * 8);
                const size_t npos = take(NCAP * 2);
                const size_t pord = take(NCAP * 2);
                const size_t pre = take(NCAP * 4);
                const size_t pre2 = take(NCAP * 4);
                const size_t cc = take((size_t)NCAP * (packed ? 8 : 16));
                const size_t l_kdata = take((size_t)KCAP * 4);
                const size_t l_knode = take((size_t)KCAP * 2);

                const OctreeCarve C(NCAP, KCAP, packed != 0);
                CHECK(C.bytes == parent_octree_lds_bytes(NCAP, KCAP, packed != 0));
                CHECK(C.tmp == tmp && C.sortb == sortb);
                const uint32_t *A = C.node[0], *B = C.node[1];
                CHECK(A[OctreeCarve::X0] == A_x0 && A[OctreeCarve::Y0] == A_y0);
                CHECK(A[OctreeCarve::X1] == A_x1 && A[OctreeCarve::Y1] == A_y1);
                CHECK(A[OctreeCarve::CNT] == A_cnt && A[OctreeCarve::SEQ] == A_seq);
                CHECK(B[OctreeCarve::X0] == B_x0 && B[OctreeCarve::Y0] == B_y0);
                CHECK(B[OctreeCarve::X1] == B_x1 && B[OctreeCarve::Y1] == B_y1);
                CHECK(B[OctreeCarve::CNT] == B_cnt && B[OctreeCarve::SEQ] == B_seq);
                CHECK(C.cpos == cpos && C.npos == npos && C.pord == pord);
                CHECK(C.pre == pre && C.pre2 == pre2 && C.cc == cc);
                CHECK(C.kdata == l_kdata && C.knode == l_knode);
                // the carve's own offsets, in its order: 16-aligned, each region's bytes (what the
                // kernel keeps there) ending before the next begins, the last inside the launch size
                const uint32_t own[] = {C.tmp, C.sortb, A[0], A[1], A[2], A[3], A[4], A[5],
                                        B[0], B[1], B[2], B[3], B[4], B[5], C.cpos, C.npos,
                                        C.pord, C.pre, C.pre2, C.cc, C.kdata, C.knode};
                const size_t n_own = sizeof(own) / sizeof(own[0]);
                CHECK(n_own == regs.size());
                for (size_t i = 0; i < n_own; ++i) {
                    CHECK(own[i] % 16 == 0);
                    const size_t next = i + 1 < n_own ? own[i + 1] : C.bytes;
                    CHECK(own[i] + regs[i].bytes <= next);
                }
                CHECK(C.bytes % 16 == 0);
                // the one overlap: the global-scratch path's wide counts start at cc, run past its
                // packed end over kdata / knode, and still fit the launch size
                CHECK(C.cc + (size_t)NCAP * 16 <= C.bytes);
                if (packed) CHECK(C.cc + (size_t)NCAP * 16 > C.kdata);
                CHECK(OctreeCarve::TMP_INTS == 224);
            }
    std::puts("ok octree_carve");
}

int main() {
    test_keypoint_size();
    test_workspace();
    test_stereo_one_pair();
    test_stereo_batch();
    test_server();
    test_octree_carve();
    std::puts("all ok");
    return 0;
}
