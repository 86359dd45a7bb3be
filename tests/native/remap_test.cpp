// The rectifier glue compiled as ORB-SLAM2's stereo programs would use it: orbx_glue::Rectifier
// (integration/orbx_slam2_glue.h) in place of cv::remap (Examples/Stereo/stereo_euroc.cc:136-137),
// on the cv stand-in headers.
//
//   remap_test nogpu      on a host without a GPU the glue must throw, naming the failing call
//   remap_test run DIR    DIR/params.txt: "src_w src_h src_step dst_w dst_h dst_step"; DIR/src.raw
//                         (src_h x src_step bytes), DIR/map1.bin, DIR/map2.bin (dst_h x dst_w
//                         floats), DIR/dst.raw (dst_h x dst_step bytes, pre-filled by the caller).
//                         Remaps through cv::Mat headers over the padded rows and rewrites
//                         DIR/dst.raw; then once more into an empty cv::Mat (allocated by the
//                         glue) and checks that both agree.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbx_slam2_glue.h"

static std::vector<uint8_t> slurp(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    std::vector<uint8_t> b;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    std::fclose(f);
    return b;
}

static void dump(const std::string& path, const void* p, size_t bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) throw std::runtime_error("cannot write " + path);
    std::fclose(f);
}

static int nogpu() {
    cv::Mat M1 = cv::Mat::zeros(4, 4, CV_32F), M2 = cv::Mat::zeros(4, 4, CV_32F);
    try {
        orbx_glue::Rectifier r(M1, M2, 4, 4);
    } catch (const std::runtime_error& e) {
        std::printf("threw: %s\n", e.what());
        return std::strstr(e.what(), "orbx_rectifier_create") ? 0 : 1;
    }
    std::printf("no exception\n");
    return 1;
}

static int run(const std::string& dir) {
    int sw, sh, dw, dh;
    long sstep, dstep;
    {
        FILE* f = std::fopen((dir + "/params.txt").c_str(), "r");
        if (!f || std::fscanf(f, "%d %d %ld %d %d %ld", &sw, &sh, &sstep, &dw, &dh, &dstep) != 6)
            throw std::runtime_error("params.txt");
        std::fclose(f);
    }
    std::vector<uint8_t> src = slurp(dir + "/src.raw"), m1 = slurp(dir + "/map1.bin"),
                         m2 = slurp(dir + "/map2.bin"), dst = slurp(dir + "/dst.raw");
    if (src.size() != (size_t)sh * sstep || m1.size() != 4 * (size_t)dw * dh ||
        m2.size() != m1.size() || dst.size() != (size_t)dh * dstep)
        throw std::runtime_error("input sizes");
    cv::Mat M1(dh, dw, CV_32F, m1.data()), M2(dh, dw, CV_32F, m2.data());
    orbx_glue::Rectifier rect(M1, M2, sw, sh);
    const cv::Mat imRaw(sh, sw, CV_8UC1, src.data(), (size_t)sstep);
    cv::Mat imRect(dh, dw, CV_8UC1, dst.data(), (size_t)dstep);
    rect.remap(imRaw, imRect);
    if (imRect.data != dst.data()) return 2;      // a matching destination is written in place
    dump(dir + "/dst.raw", dst.data(), dst.size());
    cv::Mat fresh;
    rect.remap(imRaw, fresh);
    if (fresh.rows != dh || fresh.cols != dw || fresh.type() != CV_8UC1) return 3;
    int bad = 0;
    for (int r = 0; r < dh; ++r) bad += std::memcmp(fresh.ptr(r), imRect.ptr(r), (size_t)dw) != 0;
    std::printf("rows %d cols %d bad %d\n", dh, dw, bad);
    return bad == 0 ? 0 : 4;
}

int main(int argc, char** argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "nogpu") return nogpu();
        if (mode == "run" && argc > 2) return run(argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "remap_test: %s\n", e.what());
        return 10;
    }
    std::fprintf(stderr, "usage: remap_test nogpu | run DIR\n");
    return 64;
}
