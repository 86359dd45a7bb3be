// orbx_slam2_glue.h — the Frame / ORBmatcher side of the drop-in, as
// templates over the reference's own Frame, KeyFrame and MapPoint classes so that this header
// needs nothing from ORB-SLAM2 beyond the members it names.
//
//   ComputeStereoMatches(F)         replaces Frame::ComputeStereoMatches (src/Frame.cc:496-686)
//   ExtractStereo(F, imL, imR)      replaces Frame.cc:89-102 (both ExtractORB threads + the
//                                   stereo match) by one two-image submission
//   ComputeStereoFromRGBD(F, imDepth, depthFactor)
//                                   replaces Frame::ComputeStereoFromRGBD (src/Frame.cc:689-710)
//                                   and the whole-image imDepth.convertTo in front of it
//                                   (src/Tracking.cc:244-245)
//   Rectifier(M1, M2, srcSize)     replaces the per-frame cv::remap(imRaw, imRect, M1, M2,
//                                   cv::INTER_LINEAR) of Examples/Stereo/stereo_euroc.cc:136-137
//                                   (maps from cv::initUndistortRectifyMap, :96-98)
//   OrbxView / BuildView(f, view)   the orbx_featureset of a Frame / KeyFrame (mFeatVec, mGrid)
//   SearchByBoW(m, pKF, F, out)     ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (:182-319)
//
// ORB_SLAM2::ORBextractor is the one of integration/ORBextractor.h (handle()).
#ifndef ORBX_INTEGRATION_SLAM2_GLUE_H
#define ORBX_INTEGRATION_SLAM2_GLUE_H

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "orbx.h"
#include "orbx_frame.h"
#include "orbx_match.h"

namespace orbx_glue {

// CV_16U (core/hal/interface.h: 2), also where a cv header without 16-bit types is in use
#ifdef CV_16U
constexpr int kCv16U = CV_16U;
#else
constexpr int kCv16U = 2;
#endif

inline void check(orbx_status s, const char* what) {
    if (s != ORBX_OK) throw std::runtime_error(std::string(what) + ": " + orbx_last_error());
}

// Frame.cc:496-686 for the last extraction of both cameras.  The reference reads the member
// mb uninitialised at Frame.cc:534 (it is set only after ComputeStereoMatches returns in the
// stereo constructor, Frame.cc:66-120); the intended value mbf / fx is passed instead.
// It reads the device pyramids, so it turns the extractors' host pyramid copy off for the
// frames after this one (integration/ORBextractor.h, the opt-out).
template <class Frame>
int ComputeStereoMatches(Frame& F) {
    if (F.mpORBextractorLeft->HostPyramid()) F.mpORBextractorLeft->SetHostPyramid(false);
    if (F.mpORBextractorRight->HostPyramid()) F.mpORBextractorRight->SetHostPyramid(false);
    F.mvuRight = std::vector<float>(F.N, -1.0f);
    F.mvDepth = std::vector<float>(F.N, -1.0f);
    int nvalid = 0;
    check(orbx_stereo_match(F.mpORBextractorLeft->handle(), F.mpORBextractorRight->handle(),
                            F.mbf, F.mbf / F.fx, F.mvuRight.data(), F.mvDepth.data(), F.N,
                            &nvalid),
          "orbx_stereo_match");
    return nvalid;
}

// Frame.cc:89-102 in one call (the stereo Frame constructor's two ExtractORB threads, then
// ComputeStereoMatches): both views as one two-image batch on the LEFT extractor's handle with
// the stereo match appended, one submission and one wait (orbx_stereo_frame_view).  Fills
// mvKeys / mDescriptors, mvKeysRight / mDescriptorsRight, N, mvuRight / mvDepth with the same
// values as the two-thread form.  The right extractor's handle is not used.
//
// An empty image: each ExtractORB returns without touching its outputs (ORBextractor.cc:
// 1068-1069), so the views go through the extractors' operator() one by one and no stereo
// match is made (the reference would take the median of an empty vector, Frame.cc:673).
// mvImagePyramid afterwards: see integration/ORBextractor.h (KeepPyramid on the left one).
template <class Frame>
int ExtractStereo(Frame& F, const cv::Mat& imLeft, const cv::Mat& imRight) {
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint layout");
    if (imLeft.empty() || imRight.empty()) {
        (*F.mpORBextractorLeft)(imLeft, cv::Mat(), F.mvKeys, F.mDescriptors);
        (*F.mpORBextractorRight)(imRight, cv::Mat(), F.mvKeysRight, F.mDescriptorsRight);
        F.N = (int)F.mvKeys.size();
        F.mvuRight.assign((size_t)F.N, -1.0f);
        F.mvDepth.assign((size_t)F.N, -1.0f);
        return 0;
    }
    if (imLeft.rows != imRight.rows || imLeft.cols != imRight.cols)
        throw std::invalid_argument("ExtractStereo: left and right sizes differ");
    // the match reads the device pyramids: no host copy from the extractors' operator()
    // (empty images above) either
    if (F.mpORBextractorLeft->HostPyramid()) F.mpORBextractorLeft->SetHostPyramid(false);
    if (F.mpORBextractorRight->HostPyramid()) F.mpORBextractorRight->SetHostPyramid(false);
    orbx_stereo_frame_out o{};
    check(orbx_stereo_frame_view(F.mpORBextractorLeft->handle(), imLeft.data,
                                 (size_t)imLeft.step, imRight.data, (size_t)imRight.step,
                                 imLeft.cols, imLeft.rows, F.mbf, F.mbf / F.fx, &o),
          "orbx_stereo_frame_view");
    F.mpORBextractorLeft->SetPyramidSource(F.mpORBextractorLeft, 0);
    F.mpORBextractorRight->SetPyramidSource(F.mpORBextractorLeft, 1);
    auto keys = [](const orbx_keypoint* k, int n) {
        const cv::KeyPoint* c = reinterpret_cast<const cv::KeyPoint*>(k);
        return std::vector<cv::KeyPoint>(c, c + n);
    };
    auto desc = [](const uint8_t* d, int n, cv::Mat& m) {
        if (n == 0) {
            m.release();
            return;
        }
        m.create(n, 32, CV_8U);
        if (m.isContinuous())
            std::memcpy(m.data, d, (size_t)n * 32);
        else
            for (int i = 0; i < n; ++i) std::memcpy(m.ptr(i), d + (size_t)i * 32, 32);
    };
    F.mvKeys = keys(o.kps[0], o.n[0]);
    F.mvKeysRight = keys(o.kps[1], o.n[1]);
    desc(o.desc[0], o.n[0], F.mDescriptors);
    desc(o.desc[1], o.n[1], F.mDescriptorsRight);
    F.N = o.n[0];
    F.mvuRight.assign(o.u_right, o.u_right + o.n[0]);
    F.mvDepth.assign(o.depth, o.depth + o.n[0]);
    return o.n_valid;
}

// Frame.cc:689-710 on the RAW depth image (CV_16U or CV_32F, any row step): mvuRight / mvDepth
// from mvKeys (the sampled pixel) and mvKeysUn (uRight).  depthFactor is mDepthMapFactor after
// Tracking.cc:159-163.  The caller drops Tracking.cc:244-245: only the ~N sampled pixels are
// scaled, with the rounding of convertTo.  A keypoint outside the image gives -1 / -1 (the
// reference reads out of bounds).  Returns the number of features with depth.
template <class Frame>
int ComputeStereoFromRGBD(Frame& F, const void* depth, orbx_depth_type type, size_t step,
                          int cols, int rows, float depthFactor, int device = 0) {
    static_assert(sizeof(*F.mvKeys.data()) == sizeof(orbx_keypoint), "cv::KeyPoint layout");
    if ((int)F.mvKeys.size() != F.N || (int)F.mvKeysUn.size() != F.N)
        throw std::invalid_argument("ComputeStereoFromRGBD: mvKeys / mvKeysUn do not hold N keypoints");
    F.mvuRight = std::vector<float>((size_t)F.N, -1.0f);
    F.mvDepth = std::vector<float>((size_t)F.N, -1.0f);
    check(orbx_compute_stereo_from_rgbd(depth, type, step, cols, rows, depthFactor, F.mbf,
                                        reinterpret_cast<const orbx_keypoint*>(F.mvKeys.data()),
                                        reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data()),
                                        F.N, F.mvuRight.data(), F.mvDepth.data(), device),
          "orbx_compute_stereo_from_rgbd");
    int nvalid = 0;
    for (float d : F.mvDepth) nvalid += d > 0;
    return nvalid;
}

template <class Frame>
int ComputeStereoFromRGBD(Frame& F, const cv::Mat& imDepth, float depthFactor, int device = 0) {
    if (imDepth.type() != kCv16U && imDepth.type() != CV_32F)
        throw std::invalid_argument("ComputeStereoFromRGBD: CV_16U or CV_32F depth expected");
    return ComputeStereoFromRGBD(F, imDepth.data,
                                 imDepth.type() == kCv16U ? ORBX_DEPTH_U16 : ORBX_DEPTH_F32,
                                 (size_t)imDepth.step, imDepth.cols, imDepth.rows, depthFactor,
                                 device);
}

// stereo_euroc.cc:136-137 (ros_stereo.cc:161-162): cv::remap(imRaw, imRect, M1, M2,
// cv::INTER_LINEAR) of one 8UC1 image on the device.  M1 / M2 are the CV_32FC1 maps
// cv::initUndistortRectifyMap(..., CV_32F, M1, M2) wrote (:96-98); srcCols x srcRows is the raw
// image's size.  One Rectifier per camera, built once; remap() may be called from several threads.
class Rectifier {
public:
    Rectifier(const cv::Mat& M1, const cv::Mat& M2, int srcCols, int srcRows, int device = 0) {
        if (M1.empty() || M1.type() != CV_32F || M2.type() != CV_32F || M1.rows != M2.rows ||
            M1.cols != M2.cols)
            throw std::invalid_argument("Rectifier: two CV_32FC1 maps of one size expected");
        const cv::Mat a = M1.isContinuous() ? M1 : M1.clone(), b = M2.isContinuous() ? M2 : M2.clone();
        check(orbx_rectifier_create(reinterpret_cast<const float*>(a.data),
                                    reinterpret_cast<const float*>(b.data), M1.cols, M1.rows,
                                    srcCols, srcRows, device, &r_),
              "orbx_rectifier_create");
        cols_ = M1.cols;
        rows_ = M1.rows;
        src_cols_ = srcCols;
        src_rows_ = srcRows;
    }
    ~Rectifier() { orbx_rectifier_destroy(r_); }
    Rectifier(const Rectifier&) = delete;
    Rectifier& operator=(const Rectifier&) = delete;

    // dst is (re)allocated as cv::remap does unless it already is a rows x cols CV_8UC1 image
    // (then its rows may be padded: bytes past the last column are left untouched)
    void remap(const cv::Mat& src, cv::Mat& dst) const {
        if (src.type() != CV_8UC1 || src.cols != src_cols_ || src.rows != src_rows_)
            throw std::invalid_argument("Rectifier::remap: CV_8UC1 image of the source size expected");
        if (dst.empty() || dst.type() != CV_8UC1 || dst.rows != rows_ || dst.cols != cols_)
            dst.create(rows_, cols_, CV_8UC1);
        check(orbx_remap(r_, src.data, (size_t)src.step, dst.data, (size_t)dst.step), "orbx_remap");
    }
    const orbx_rectifier* handle() const { return r_; }

private:
    orbx_rectifier* r_ = nullptr;
    int cols_ = 0, rows_ = 0, src_cols_ = 0, src_rows_ = 0;
};

// CSR copies of mFeatVec (after ComputeBoW) and mGrid (after AssignFeaturesToGrid); the other
// arrays are the frame's own (mvKeysUn, mDescriptors, mvuRight).  Rebuild after either changes.
struct OrbxView {
    std::vector<uint32_t> node_id;
    std::vector<int32_t> node_off, node_feat;
    std::vector<int32_t> grid_off, grid_feat;
    orbx_featureset fs{};
};

template <class F>
void BuildView(const F& f, OrbxView& v, int grid_cols, int grid_rows) {
    v.node_id.clear();
    v.node_off.assign(1, 0);
    v.node_feat.clear();
    for (const auto& kv : f.mFeatVec) {  // std::map: ascending node id
        v.node_id.push_back((uint32_t)kv.first);
        for (auto i : kv.second) v.node_feat.push_back((int32_t)i);
        v.node_off.push_back((int32_t)v.node_feat.size());
    }
    v.grid_off.assign(1, 0);
    v.grid_feat.clear();
    for (int ix = 0; ix < grid_cols; ++ix)  // cell c = ix * rows + iy
        for (int iy = 0; iy < grid_rows; ++iy) {
            for (auto i : f.mGrid[ix][iy]) v.grid_feat.push_back((int32_t)i);
            v.grid_off.push_back((int32_t)v.grid_feat.size());
        }
    static_assert(sizeof(*f.mvKeysUn.data()) == sizeof(orbx_keypoint),
                  "mvKeysUn elements must be cv::KeyPoint (orbx_keypoint's layout)");
    orbx_featureset& s = v.fs;
    s.n = f.N;
    s.keys = reinterpret_cast<const orbx_keypoint*>(f.mvKeysUn.data());
    s.desc = f.mDescriptors.data;  // N x 32, continuous
    s.u_right = f.mvuRight.empty() ? nullptr : f.mvuRight.data();
    s.n_nodes = (int32_t)v.node_id.size();
    s.node_id = v.node_id.data();
    s.node_off = v.node_off.data();
    s.node_feat = v.node_feat.data();
    s.grid_cols = grid_cols;
    s.grid_rows = grid_rows;
    s.grid_off = v.grid_off.data();
    s.grid_feat = v.grid_feat.data();
    s.min_x = f.mnMinX;
    s.min_y = f.mnMinY;
    s.max_x = f.mnMaxX;
    s.max_y = f.mnMaxY;
    s.grid_inv_w = f.mfGridElementWidthInv;
    s.grid_inv_h = f.mfGridElementHeightInv;
}

// ORBmatcher.cc:182-319.  `m` is the ORBmatcher's orbx_matcher (one per thread); kf_view /
// f_view are the BuildView results of pKF and F.
template <class KeyFrame, class Frame, class MapPoint>
int SearchByBoW(orbx_matcher* m, KeyFrame* pKF, const OrbxView& kf_view, Frame& F,
                const OrbxView& f_view, std::vector<MapPoint*>& vpMapPointMatches) {
    const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
    std::vector<uint8_t> valid((size_t)pKF->N);
    for (int i = 0; i < pKF->N; ++i)
        valid[(size_t)i] = vpMapPointsKF[(size_t)i] && !vpMapPointsKF[(size_t)i]->isBad();
    std::vector<int32_t> match((size_t)F.N);
    int32_t n = 0;
    check(orbx_search_by_bow_kf_frame(m, &kf_view.fs, valid.data(), &f_view.fs, match.data(), &n),
          "orbx_search_by_bow_kf_frame");
    vpMapPointMatches.assign((size_t)F.N, static_cast<MapPoint*>(nullptr));
    for (int i = 0; i < F.N; ++i)
        if (match[(size_t)i] >= 0) vpMapPointMatches[(size_t)i] = vpMapPointsKF[(size_t)match[(size_t)i]];
    return n;
}

}  // namespace orbx_glue

#endif  // ORBX_INTEGRATION_SLAM2_GLUE_H
