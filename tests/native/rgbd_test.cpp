// The RGB-D glue compiled as ORB-SLAM2 would include it: orbx_glue::ComputeStereoFromRGBD
// (integration/orbx_slam2_glue.h) on a Frame stand-in and the cv stand-in headers.
//
//   rgbd_test nogpu      on a host without a GPU the glue must throw, naming the failing call
//   rgbd_test run DIR    DIR/params.txt: "width height type(0 = CV_16U, 1 = CV_32F) step_bytes
//                        alloc_rows factor mbf n"; DIR/depth.raw (alloc_rows x step_bytes),
//                        DIR/kps.bin, DIR/kps_un.bin (n cv::KeyPoint each).  Writes
//                        DIR/uRight.bin, DIR/depth.bin (the glue) and checks them here against
//                        the reference's statements (Tracking.cc:244-245 on the whole image,
//                        then Frame.cc:689-710) for the keypoints inside the image.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "rgbd_standin.h"

#include "orbx_slam2_glue.h"

using rgbd_standin::Frame;

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
    Frame F;
    F.N = 1;
    F.mbf = 40.f;
    F.mvKeys.resize(1);
    F.mvKeysUn.resize(1);
    cv::Mat depth = cv::Mat::ones(4, 4, CV_32F);
    try {
        orbx_glue::ComputeStereoFromRGBD(F, depth, 1.0f);
    } catch (const std::runtime_error& e) {
        std::printf("threw: %s\n", e.what());
        return std::strstr(e.what(), "orbx_compute_stereo_from_rgbd") ? 0 : 1;
    }
    std::printf("no exception\n");
    return 1;
}

static int run(const std::string& dir) {
    int w, h, type, rows, n;
    long step;
    float factor, mbf;
    {
        FILE* f = std::fopen((dir + "/params.txt").c_str(), "r");
        if (!f || std::fscanf(f, "%d %d %d %ld %d %a %a %d", &w, &h, &type, &step, &rows, &factor,
                              &mbf, &n) != 8)
            throw std::runtime_error("params.txt");
        std::fclose(f);
    }
    std::vector<uint8_t> img = slurp(dir + "/depth.raw"), k = slurp(dir + "/kps.bin"),
                         ku = slurp(dir + "/kps_un.bin");
    if (img.size() != (size_t)rows * step || k.size() != sizeof(cv::KeyPoint) * (size_t)n ||
        ku.size() != k.size())
        throw std::runtime_error("input sizes");
    Frame F;
    F.N = n;
    F.mbf = mbf;
    F.mvKeys.resize((size_t)n);
    F.mvKeysUn.resize((size_t)n);
    if (n) {
        std::memcpy(static_cast<void*>(F.mvKeys.data()), k.data(), k.size());
        std::memcpy(static_cast<void*>(F.mvKeysUn.data()), ku.data(), ku.size());
    }
    int nvalid;
    if (type == 1) {   // a cv::Mat header over the padded rows
        cv::Mat imDepth(h, w, CV_32F, img.data(), (size_t)step);
        nvalid = orbx_glue::ComputeStereoFromRGBD(F, imDepth, factor);
    } else {
        nvalid = orbx_glue::ComputeStereoFromRGBD(F, img.data(), ORBX_DEPTH_U16, (size_t)step, w, h,
                                                  factor);
    }
    if ((int)F.mvuRight.size() != n || (int)F.mvDepth.size() != n) return 2;
    dump(dir + "/uRight.bin", F.mvuRight.data(), 4 * (size_t)n);
    dump(dir + "/depth.bin", F.mvDepth.data(), 4 * (size_t)n);

    // Tracking.cc:244-245: imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor), the whole image
    std::vector<float> conv((size_t)w * h);
    const bool scale = std::fabs(factor - 1.0f) > 1e-5 || type != 1;
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const uint8_t* row = img.data() + (size_t)r * step;
            float v;
            if (type == 1) std::memcpy(&v, row + 4 * (size_t)c, 4);
            else {
                uint16_t u;
                std::memcpy(&u, row + 2 * (size_t)c, 2);
                v = (float)u;
            }
            conv[(size_t)r * w + c] = scale ? v * factor : v;
        }
    // Frame.cc:689-710
    int checked = 0, bad = 0, valid_ref = 0;
    for (int i = 0; i < n; i++) {
        const cv::KeyPoint& kp = F.mvKeys[(size_t)i];
        const cv::KeyPoint& kpU = F.mvKeysUn[(size_t)i];
        const float& v = kp.pt.y;
        const float& u = kp.pt.x;
        if (!(u > -1.0f && u < (float)w && v > -1.0f && v < (float)h)) {
            bad += F.mvDepth[(size_t)i] != -1.0f || F.mvuRight[(size_t)i] != -1.0f;
            continue;   // at<float>(v, u) would read outside the image
        }
        const float d = conv[(size_t)(int)v * w + (int)u];
        float de = -1.0f, ur = -1.0f;
        if (d > 0) {
            de = d;
            ur = kpU.pt.x - F.mbf / d;
            ++valid_ref;
        }
        ++checked;
        bad += std::memcmp(&de, &F.mvDepth[(size_t)i], 4) != 0 ||
               std::memcmp(&ur, &F.mvuRight[(size_t)i], 4) != 0;
    }
    std::printf("n %d valid %d checked %d bad %d\n", n, nvalid, checked, bad);
    return bad == 0 && valid_ref == nvalid ? 0 : 3;
}

int main(int argc, char** argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "nogpu") return nogpu();
        if (mode == "run" && argc > 2) return run(argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rgbd_test: %s\n", e.what());
        return 10;
    }
    std::fprintf(stderr, "usage: rgbd_test nogpu | run DIR\n");
    return 64;
}
