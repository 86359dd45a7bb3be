// A second restatement of the six projection loops orbx_project_map_points* runs on the GPU,
// written with cv::Mat expressions in the way src/ORBmatcher.cc writes them (Rcw*x3Dw+tcw,
// -Rcw.t()*tcw is the caller's, cv::norm, PO.dot(Pn), 1.0/x3Dc.at<float>(2)), over the cv stand-in
// of tests/native/cv_standin.  No liborbx, no GPU: only the record layouts of include/orbx_frame.h.
// tests/test_projection_cases.py compares it bit for bit with the numpy restatement of
// tests/projection_cases.py.
//
//   project_ref <cases.bin> <out.bin>
// cases.bin: int32 ncases, then per case int32 {mode, n, has_keys, has_skip}, the orbx_proj_job,
// n orbx_map_point, [n orbx_keypoint], [n skip bytes].  out.bin: per case n orbx_proj_query and
// the int32 active count.
#include <opencv2/core/core.hpp>
#include <xmmintrin.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx_frame.h"

static_assert(sizeof(orbx_proj_job) == 240 && sizeof(orbx_proj_job) % 16 == 0 &&
                  sizeof(orbx_map_point) == 32 && sizeof(orbx_proj_query) == 32,
              "record layouts of include/orbx_frame.h");

namespace {

// (int) of a float on x86-64 (cvttss2si): INT_MIN for NaN / out of range
int to_int(float f) { return _mm_cvttss_si32(_mm_set_ss(f)); }

cv::Mat mat(const float* p, int rows, int cols) {
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) m.at<float>(r, c) = p[r * cols + c];
    return m;
}

// the members of Frame / KeyFrame the loops read
struct View {
    float fx, fy, cx, cy, mbf, mb;
    float mnMinX, mnMaxX, mnMinY, mnMaxY;
    float mfLogScaleFactor;
    int mnScaleLevels;
    std::vector<float> mvScaleFactors;
    explicit View(const orbx_proj_job& J)
        : fx(J.cam.fx), fy(J.cam.fy), cx(J.cam.cx), cy(J.cam.cy), mbf(J.cam.mbf), mb(J.mb),
          mnMinX(J.cam.min_x), mnMaxX(J.cam.max_x), mnMinY(J.cam.min_y), mnMaxY(J.cam.max_y),
          mfLogScaleFactor(J.cam.log_scale_factor), mnScaleLevels(J.cam.nlevels),
          mvScaleFactors(J.cam.scale, J.cam.scale + 16) {}
    // KeyFrame::IsInImage (KeyFrame.cc:624-627)
    bool IsInImage(const float& x, const float& y) const {
        return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY);
    }
};

// the members of MapPoint the loops read (MapPoint.cc:394-404, 430-444)
struct Point {
    cv::Mat mWorldPos, mNormalVector;
    float mfMinDistance, mfMaxDistance;
    explicit Point(const orbx_map_point& m)
        : mWorldPos(mat(m.pos, 3, 1)), mNormalVector(mat(m.normal, 3, 1)),
          mfMinDistance(m.min_dist), mfMaxDistance(m.max_dist) {}
    cv::Mat GetWorldPos() const { return mWorldPos.clone(); }
    cv::Mat GetNormal() const { return mNormalVector.clone(); }
    float GetMinDistanceInvariance() const { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() const { return 1.2f * mfMaxDistance; }
    int PredictScale(const float& currentDist, const View* pKF) const {
        float ratio = mfMaxDistance / currentDist;
        int nScale = to_int(std::ceil(std::log(ratio) / pKF->mfLogScaleFactor));
        if (nScale < 0) nScale = 0;
        else if (nScale >= pKF->mnScaleLevels) nScale = pKF->mnScaleLevels - 1;
        return nScale;
    }
};

const orbx_proj_query INACTIVE = {0.f, 0.f, 0.f, -1.f, -1, -1, -1, 0.f};

// ORBmatcher.cc:1402-1458
bool last_frame(const orbx_proj_job& J, const View& CurrentFrame, const cv::Mat& Rcw,
                const cv::Mat& tcw, const Point& MP, const orbx_keypoint& key, orbx_proj_query& q) {
    const cv::Mat twc = mat(J.cam.Ow, 3, 1);   // -Rcw.t()*tcw, the caller's
    const cv::Mat Rlw = mat(J.pre_R, 3, 3);
    const cv::Mat tlw = mat(J.pre_t, 3, 1);
    const cv::Mat tlc = Rlw * twc + tlw;
    const bool bMono = J.mono != 0;
    const bool bForward = tlc.at<float>(2) > CurrentFrame.mb && !bMono;
    const bool bBackward = -tlc.at<float>(2) > CurrentFrame.mb && !bMono;
    const float th = J.th;

    cv::Mat x3Dw = MP.GetWorldPos();
    cv::Mat x3Dc = Rcw * x3Dw + tcw;
    const float xc = x3Dc.at<float>(0);
    const float yc = x3Dc.at<float>(1);
    const float invzc = 1.0 / x3Dc.at<float>(2);
    if (invzc < 0) return false;
    float u = CurrentFrame.fx * xc * invzc + CurrentFrame.cx;
    float v = CurrentFrame.fy * yc * invzc + CurrentFrame.cy;
    if (u < CurrentFrame.mnMinX || u > CurrentFrame.mnMaxX) return false;
    if (v < CurrentFrame.mnMinY || v > CurrentFrame.mnMaxY) return false;
    int nLastOctave = key.octave;
    float radius = th * CurrentFrame.mvScaleFactors[(size_t)nLastOctave];
    int minL = nLastOctave - 1, maxL = nLastOctave + 1;
    if (bForward) {
        minL = nLastOctave;
        maxL = -1;
    } else if (bBackward) {
        minL = 0;
        maxL = nLastOctave;
    }
    const float ur = u - CurrentFrame.mbf * invzc;
    q = {u, v, ur, radius, minL, maxL, nLastOctave, key.angle};
    return true;
}

// ORBmatcher.cc:1544-1596
bool keyframe(const orbx_proj_job& J, const View& CurrentFrame, const cv::Mat& Rcw,
              const cv::Mat& tcw, const cv::Mat& Ow, const Point& MP, const orbx_keypoint& key,
              orbx_proj_query& q) {
    const float th = J.th;
    cv::Mat x3Dw = MP.GetWorldPos();
    cv::Mat x3Dc = Rcw * x3Dw + tcw;
    const float xc = x3Dc.at<float>(0);
    const float yc = x3Dc.at<float>(1);
    const float invzc = 1.0 / x3Dc.at<float>(2);
    const float u = CurrentFrame.fx * xc * invzc + CurrentFrame.cx;
    const float v = CurrentFrame.fy * yc * invzc + CurrentFrame.cy;
    if (u < CurrentFrame.mnMinX || u > CurrentFrame.mnMaxX) return false;
    if (v < CurrentFrame.mnMinY || v > CurrentFrame.mnMaxY) return false;
    cv::Mat PO = x3Dw - Ow;
    float dist3D = cv::norm(PO);
    const float maxDistance = MP.GetMaxDistanceInvariance();
    const float minDistance = MP.GetMinDistanceInvariance();
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    int nPredictedLevel = MP.PredictScale(dist3D, &CurrentFrame);
    const float radius = th * CurrentFrame.mvScaleFactors[(size_t)nPredictedLevel];
    q = {u, v, 0.f, radius, nPredictedLevel - 1, nPredictedLevel + 1, nPredictedLevel, key.angle};
    return true;
}

// ORBmatcher.cc:321-390 (th is an int there), :881-946 (Fuse), :1035-1105 (Fuse with Scw)
bool kf_modes(int mode, const orbx_proj_job& J, const View& KF, const cv::Mat& Rcw,
              const cv::Mat& tcw, const cv::Mat& Ow, const Point& MP, orbx_proj_query& q) {
    const float &fx = KF.fx, &fy = KF.fy, &cx = KF.cx, &cy = KF.cy, &bf = KF.mbf;
    const float th = J.th;
    cv::Mat p3Dw = MP.GetWorldPos();
    cv::Mat p3Dc = Rcw * p3Dw + tcw;
    float invz;
    if (mode == ORBX_PROJ_KF_SCW) {
        if (p3Dc.at<float>(2) < 0.0) return false;
        invz = 1 / p3Dc.at<float>(2);
    } else if (mode == ORBX_PROJ_FUSE) {
        if (p3Dc.at<float>(2) < 0.0f) return false;
        invz = 1 / p3Dc.at<float>(2);
    } else {
        if (p3Dc.at<float>(2) < 0.0f) return false;
        invz = 1.0 / p3Dc.at<float>(2);
    }
    const float x = p3Dc.at<float>(0) * invz;
    const float y = p3Dc.at<float>(1) * invz;
    const float u = fx * x + cx;
    const float v = fy * y + cy;
    if (!KF.IsInImage(u, v)) return false;
    const float ur = mode == ORBX_PROJ_FUSE ? u - bf * invz : 0.f;
    const float maxDistance = MP.GetMaxDistanceInvariance();
    const float minDistance = MP.GetMinDistanceInvariance();
    cv::Mat PO = p3Dw - Ow;
    const float dist3D = cv::norm(PO);
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    cv::Mat Pn = MP.GetNormal();
    if (PO.dot(Pn) < 0.5 * dist3D) return false;
    int nPredictedLevel = MP.PredictScale(dist3D, &KF);
    const float radius = th * KF.mvScaleFactors[(size_t)nPredictedLevel];
    q = {u, v, ur, radius, -1, -1, nPredictedLevel, 0.f};
    return true;
}

// ORBmatcher.cc:1204-1247 (one direction; :1284-1327 mirrors it)
bool sim3(const orbx_proj_job& J, const View& KF2, const cv::Mat& sR21, const cv::Mat& t21,
          const Point& MP, orbx_proj_query& q) {
    const float &fx = KF2.fx, &fy = KF2.fy, &cx = KF2.cx, &cy = KF2.cy;
    const cv::Mat R1w = mat(J.pre_R, 3, 3);
    const cv::Mat t1w = mat(J.pre_t, 3, 1);
    const float th = J.th;
    cv::Mat p3Dw = MP.GetWorldPos();
    cv::Mat p3Dc1 = R1w * p3Dw + t1w;
    cv::Mat p3Dc2 = sR21 * p3Dc1 + t21;
    if (p3Dc2.at<float>(2) < 0.0) return false;
    const float invz = 1.0 / p3Dc2.at<float>(2);
    const float x = p3Dc2.at<float>(0) * invz;
    const float y = p3Dc2.at<float>(1) * invz;
    const float u = fx * x + cx;
    const float v = fy * y + cy;
    if (!KF2.IsInImage(u, v)) return false;
    const float maxDistance = MP.GetMaxDistanceInvariance();
    const float minDistance = MP.GetMinDistanceInvariance();
    const float dist3D = cv::norm(p3Dc2);
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    const int nPredictedLevel = MP.PredictScale(dist3D, &KF2);
    const float radius = th * KF2.mvScaleFactors[(size_t)nPredictedLevel];
    q = {u, v, 0.f, radius, -1, -1, nPredictedLevel, 0.f};
    return true;
}

template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: project_ref cases.bin out.bin\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t ncases = 0;
    if (!rd(in, &ncases, 1)) return 2;
    for (int c = 0; c < ncases; ++c) {
        int32_t hdr[4];
        orbx_proj_job J;
        if (!rd(in, hdr, 4) || !rd(in, &J, 1)) return 2;
        const int mode = hdr[0], n = hdr[1];
        std::vector<orbx_map_point> mps((size_t)n);
        std::vector<orbx_keypoint> keys(hdr[2] ? (size_t)n : 0);
        std::vector<uint8_t> skip(hdr[3] ? (size_t)n : 0);
        if (!rd(in, mps.data(), mps.size()) || !rd(in, keys.data(), keys.size()) ||
            !rd(in, skip.data(), skip.size()))
            return 2;
        const View V(J);
        const cv::Mat Rcw = mat(J.cam.Rcw, 3, 3), tcw = mat(J.cam.tcw, 3, 1), Ow = mat(J.cam.Ow, 3, 1);
        std::vector<orbx_proj_query> q((size_t)n, INACTIVE);
        int32_t nactive = 0;
        // library-defined: a job whose nlevels is outside [1, 16] produces nothing
        const bool job_ok = J.cam.nlevels >= 1 && J.cam.nlevels <= 16;
        for (int i = 0; job_ok && i < n; ++i) {
            if (!skip.empty() && skip[(size_t)i]) continue;
            const Point MP(mps[(size_t)i]);
            orbx_proj_query r = INACTIVE;
            bool ok = false;
            switch (mode) {
                case ORBX_PROJ_LAST_FRAME: ok = last_frame(J, V, Rcw, tcw, MP, keys[(size_t)i], r); break;
                case ORBX_PROJ_KEYFRAME: ok = keyframe(J, V, Rcw, tcw, Ow, MP, keys[(size_t)i], r); break;
                case ORBX_PROJ_KF_SCW:
                case ORBX_PROJ_FUSE:
                case ORBX_PROJ_FUSE_SCW: ok = kf_modes(mode, J, V, Rcw, tcw, Ow, MP, r); break;
                case ORBX_PROJ_SIM3: ok = sim3(J, V, Rcw, tcw, MP, r); break;
                default: return 3;
            }
            if (ok) {
                q[(size_t)i] = r;
                nactive++;
            }
        }
        fwrite(q.data(), sizeof(orbx_proj_query), q.size(), out);
        fwrite(&nactive, 4, 1, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
