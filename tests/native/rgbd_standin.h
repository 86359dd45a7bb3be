// What tests/native/rgbd_test.cpp needs beyond the cv stand-in of tests/native/cv_standin: the
// members of ORB-SLAM2's Frame that orbx_glue::ComputeStereoFromRGBD names (include/Frame.h).
// The stand-in's cv::Mat holds CV_8UC1 and CV_32FC1 only, so a 16-bit depth image reaches the
// glue through its raw-pointer form.
#ifndef ORBX_RGBD_STANDIN_H
#define ORBX_RGBD_STANDIN_H

#include <vector>

#include <opencv2/core/core.hpp>

namespace rgbd_standin {

struct Frame {
    int N = 0;
    float mbf = 0.f;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
};

}  // namespace rgbd_standin

#endif  // ORBX_RGBD_STANDIN_H
