// A second restatement of the loop body of LocalMapping::CreateNewMapPoints
// (src/LocalMapping.cc:356-507) that orbx_triangulate_matches* runs on the GPU, written with the
// cv::Mat expressions the reference uses (Rwc1*xn1, ray1.dot(ray2), cv::norm, Rcw1.row(2).dot(x3Dt),
// x3D.rowRange(0,3)/w, x3D-Ow1) over the cv stand-in of tests/native/cv_standin.  No liborbx, no
// GPU: only the record layouts of include/orbx_frame.h.  tests/test_triangulate_cases.py compares
// it bit for bit with the numpy restatement of tests/triangulate_cases.py.
//
// What the stand-in has no form for is restated here, written on its own and not from the numpy
// text [unverified-OpenCV]: cv::addWeighted (the rows of A) and cv::SVD::compute (svd_compute,
// after OpenCV 3.2's modules/core/src/lapack.cpp: _SVDcompute and JacobiSVDImpl_<float>).
//
//   triangulate_ref <cases.bin> <out.bin>
// cases.bin: int32 ncases, then per case int32 {n1, n2, npairs, flags} (flags: 1 raw1, 2 raw2,
// 4 ur1, 8 ur2), float ratio_factor, two orbx_frame_pose, keys1[n1], keys2[n2], [raw1], [raw2],
// [ur1], [ur2], depth1[n1], depth2[n2], cos1[n1], cos2[n2] (the cosParallaxStereo tables),
// pairs[2*npairs].  out.bin: per case int32 status[npairs], float x3d[3*npairs] (zeros where the
// pair failed).  The time spent in the loop body is printed as "loop_seconds <s> pairs <n>"
// (tools/triangulate_step.py reads it).
//
//   triangulate_ref --hypot <count> <seed>
// compares hypot_235 (glibc 2.35's algorithm, as the kernel restates it) with the C library's
// hypot on <count> random pairs over the whole exponent range; exit status 1 on a difference.
#include <opencv2/core/core.hpp>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "orbx_frame.h"

namespace {

enum { OK_TRIANGULATED = 0, OK_STEREO1, OK_STEREO2, NO_MATCH, LOW_PARALLAX, W_ZERO, BEHIND_1,
       BEHIND_2, REPROJ_1, REPROJ_2, DIST_ZERO, SCALE };
static_assert((int)SCALE == (int)ORBX_TRI_SCALE && (int)W_ZERO == (int)ORBX_TRI_W_ZERO,
              "orbx_tri_code");

cv::Mat mat(const float* p, int rows, int cols) {
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) m.at<float>(r, c) = p[r * cols + c];
    return m;
}
cv::Mat vec3(float a, float b, float c) {
    const float v[3] = {a, b, c};
    return mat(v, 3, 1);
}

// the 3x4 [R | t] the reference fills through colRange / col views
cv::Mat hcat(const cv::Mat& R, const cv::Mat& t) {
    cv::Mat T(3, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T.at<float>(r, c) = R.at<float>(r, c);
        T.at<float>(r, 3) = t.at<float>(r);
    }
    return T;
}

// cv::addWeighted(src1, alpha, src2, beta, gamma, dst) for CV_32F: addWeighted_<float, double>
void addWeighted(const cv::Mat& src1, double alpha, const cv::Mat& src2, double beta, double gamma,
                 cv::Mat dst) {
    for (int r = 0; r < src1.rows; ++r)
        for (int x = 0; x < src1.cols; ++x)
            dst.at<float>(r, x) =
                (float)(src1.at<float>(r, x) * alpha + src2.at<float>(r, x) * beta + gamma);
}
// A.row(i) = s * T.row(2) - T.row(r): MatOp_AddEx::subtract folds the two operands into one
// expression (a, alpha = s, b, beta = -1), which MatOp_AddEx::assign hands to cv::addWeighted
void assign_row(cv::Mat row, float s, const cv::Mat& a, const cv::Mat& b) {
    addWeighted(a, (double)s, b, -1.0, 0.0, row);
}

// JacobiSVDImpl_<float> (lapack.cpp) up to the sort; the part that normalises and completes the
// left vectors changes neither W nor Vt and is left out.
void JacobiSVD(float* At, size_t astep, float* _W, float* Vt, size_t vstep, int m, int n) {
    const float eps = FLT_EPSILON * 2;
    std::vector<double> W((size_t)n);
    int i, j, k, iter, max_iter = std::max(m, 30);
    float c, s;
    double sd;
    astep /= sizeof(At[0]);
    vstep /= sizeof(Vt[0]);
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            float t = At[i * astep + k];
            sd += (double)t * t;
        }
        W[(size_t)i] = sd;
        for (k = 0; k < n; k++) Vt[i * vstep + k] = 0;
        Vt[i * vstep + i] = 1;
    }
    for (iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (i = 0; i < n - 1; i++)
            for (j = i + 1; j < n; j++) {
                float *Ai = At + i * astep, *Aj = At + j * astep;
                double a = W[(size_t)i], p = 0, b = W[(size_t)j];
                for (k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (std::abs(p) <= eps * std::sqrt((double)a * b)) continue;
                p *= 2;
                double beta = a - b, gamma = hypot((double)p, beta);
                if (beta < 0) {
                    double delta = (gamma - beta) * 0.5;
                    s = (float)std::sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)std::sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (k = 0; k < m; k++) {
                    float t0 = c * Ai[k] + s * Aj[k];
                    float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += (double)t0 * t0;
                    b += (double)t1 * t1;
                }
                W[(size_t)i] = a;
                W[(size_t)j] = b;
                changed = true;
                float *Vi = Vt + i * vstep, *Vj = Vt + j * vstep;
                for (k = 0; k < n; k++) {
                    float t0 = c * Vi[k] + s * Vj[k];
                    float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0;
                    Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            float t = At[i * astep + k];
            sd += (double)t * t;
        }
        W[(size_t)i] = std::sqrt(sd);
    }
    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++)
            if (W[(size_t)j] < W[(size_t)k]) j = k;
        if (i != j) {
            std::swap(W[(size_t)i], W[(size_t)j]);
            for (k = 0; k < m; k++) std::swap(At[i * astep + k], At[j * astep + k]);
            for (k = 0; k < n; k++) std::swap(Vt[i * vstep + k], Vt[j * vstep + k]);
        }
    }
    for (i = 0; i < n; i++) _W[i] = (float)W[(size_t)i];
}

// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for a square CV_32F A: _SVDcompute copies the
// transpose of A into temp_a and passes it with temp_v to JacobiSVD; vt = temp_v.  (u is not read
// by the caller and not formed.)
void svd_compute(const cv::Mat& A, cv::Mat& w, cv::Mat& vt) {
    const int n = A.cols;
    cv::Mat temp_a = A.t(), temp_w(n, 1, CV_32F), temp_v(n, n, CV_32F);
    JacobiSVD(temp_a.ptr<float>(), temp_a.step, temp_w.ptr<float>(), temp_v.ptr<float>(),
              temp_v.step, A.rows, n);
    w = temp_w;
    vt = temp_v;
}

// the members of KeyFrame the loop reads
struct KF {
    cv::Mat Rcw, tcw, Ow, Twc_R;
    float fx, fy, cx, cy, invfx, invfy, mbf;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvuRight, mvDepth, cosStereo;
    std::vector<orbx_keypoint> mvKeysUn, mvKeys;
    explicit KF(const orbx_frame_pose& P)
        : Rcw(mat(P.Rcw, 3, 3)), tcw(mat(P.tcw, 3, 1)), Ow(mat(P.Ow, 3, 1)), fx(P.fx), fy(P.fy),
          cx(P.cx), cy(P.cy), invfx(1.0f / P.fx), invfy(1.0f / P.fy), mbf(P.mbf) {
        Twc_R = Rcw.t();
        for (int i = 0; i < P.nlevels; ++i) {
            mvScaleFactors.push_back(P.scale[i]);
            mvLevelSigma2.push_back(P.scale[i] * P.scale[i]);   // ORBextractor.cc:422
        }
    }
    cv::Mat GetRotation() const { return Rcw.clone(); }
    cv::Mat GetTranslation() const { return tcw.clone(); }
    cv::Mat GetCameraCenter() const { return Ow.clone(); }
    // KeyFrame.cc:629-645
    cv::Mat UnprojectStereo(int i) const {
        const float z = mvDepth[(size_t)i];
        if (z > 0) {
            const float u = mvKeys[(size_t)i].x;
            const float v = mvKeys[(size_t)i].y;
            const float x = (u - cx) * z * invfx;
            const float y = (v - cy) * z * invfy;
            cv::Mat x3Dc = vec3(x, y, z);
            return Twc_R * x3Dc + Ow;
        }
        return cv::Mat();
    }
};

int triangulate(const KF* mpCurrentKeyFrame, const KF* pKF2, int idx1, int idx2, float ratioFactor,
                float* out) {
    cv::Mat Rcw1 = mpCurrentKeyFrame->GetRotation();
    cv::Mat Rwc1 = Rcw1.t();
    cv::Mat tcw1 = mpCurrentKeyFrame->GetTranslation();
    cv::Mat Tcw1 = hcat(Rcw1, tcw1);   // Rcw1.copyTo(Tcw1.colRange(0,3)); tcw1.copyTo(Tcw1.col(3))
    cv::Mat Ow1 = mpCurrentKeyFrame->GetCameraCenter();
    const float &fx1 = mpCurrentKeyFrame->fx, &fy1 = mpCurrentKeyFrame->fy;
    const float &cx1 = mpCurrentKeyFrame->cx, &cy1 = mpCurrentKeyFrame->cy;
    const float &invfx1 = mpCurrentKeyFrame->invfx, &invfy1 = mpCurrentKeyFrame->invfy;
    cv::Mat Ow2 = pKF2->GetCameraCenter();
    cv::Mat Rcw2 = pKF2->GetRotation();
    cv::Mat Rwc2 = Rcw2.t();
    cv::Mat tcw2 = pKF2->GetTranslation();
    cv::Mat Tcw2 = hcat(Rcw2, tcw2);
    const float &fx2 = pKF2->fx, &fy2 = pKF2->fy, &cx2 = pKF2->cx, &cy2 = pKF2->cy;
    const float &invfx2 = pKF2->invfx, &invfy2 = pKF2->invfy;

    const orbx_keypoint& kp1 = mpCurrentKeyFrame->mvKeysUn[(size_t)idx1];
    const float kp1_ur = mpCurrentKeyFrame->mvuRight[(size_t)idx1];
    bool bStereo1 = kp1_ur >= 0;
    const orbx_keypoint& kp2 = pKF2->mvKeysUn[(size_t)idx2];
    const float kp2_ur = pKF2->mvuRight[(size_t)idx2];
    bool bStereo2 = kp2_ur >= 0;

    cv::Mat xn1 = vec3((kp1.x - cx1) * invfx1, (kp1.y - cy1) * invfy1, 1.0);
    cv::Mat xn2 = vec3((kp2.x - cx2) * invfx2, (kp2.y - cy2) * invfy2, 1.0);
    cv::Mat ray1 = Rwc1 * xn1;
    cv::Mat ray2 = Rwc2 * xn2;
    const float cosParallaxRays = ray1.dot(ray2) / (cv::norm(ray1) * cv::norm(ray2));

    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo;
    float cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1)
        cosParallaxStereo1 = mpCurrentKeyFrame->cosStereo[(size_t)idx1];
    else if (bStereo2)
        cosParallaxStereo2 = pKF2->cosStereo[(size_t)idx2];
    cosParallaxStereo = std::min(cosParallaxStereo1, cosParallaxStereo2);

    cv::Mat x3D;
    int code;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 &&
        (bStereo1 || bStereo2 || cosParallaxRays < 0.9998)) {
        cv::Mat A(4, 4, CV_32F);
        assign_row(A.row(0), xn1.at<float>(0), Tcw1.row(2), Tcw1.row(0));
        assign_row(A.row(1), xn1.at<float>(1), Tcw1.row(2), Tcw1.row(1));
        assign_row(A.row(2), xn2.at<float>(0), Tcw2.row(2), Tcw2.row(0));
        assign_row(A.row(3), xn2.at<float>(1), Tcw2.row(2), Tcw2.row(1));
        cv::Mat w, vt;
        svd_compute(A, w, vt);
        x3D = vt.row(3).t();
        if (x3D.at<float>(3) == 0) return W_ZERO;
        x3D = x3D.rowRange(0, 3) / x3D.at<float>(3);
        code = OK_TRIANGULATED;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        x3D = mpCurrentKeyFrame->UnprojectStereo(idx1);
        code = OK_STEREO1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        x3D = pKF2->UnprojectStereo(idx2);
        code = OK_STEREO2;
    } else {
        return LOW_PARALLAX;
    }
    if (x3D.empty()) return LOW_PARALLAX;   // the library's code for UnprojectStereo's empty Mat

    cv::Mat x3Dt = x3D.t();
    float z1 = Rcw1.row(2).dot(x3Dt) + tcw1.at<float>(2);
    if (z1 <= 0) return BEHIND_1;
    float z2 = Rcw2.row(2).dot(x3Dt) + tcw2.at<float>(2);
    if (z2 <= 0) return BEHIND_2;

    const float& sigmaSquare1 = mpCurrentKeyFrame->mvLevelSigma2[(size_t)kp1.octave];
    const float x1 = Rcw1.row(0).dot(x3Dt) + tcw1.at<float>(0);
    const float y1 = Rcw1.row(1).dot(x3Dt) + tcw1.at<float>(1);
    const float invz1 = 1.0 / z1;
    if (!bStereo1) {
        float u1 = fx1 * x1 * invz1 + cx1;
        float v1 = fy1 * y1 * invz1 + cy1;
        float errX1 = u1 - kp1.x;
        float errY1 = v1 - kp1.y;
        if ((errX1 * errX1 + errY1 * errY1) > 5.991 * sigmaSquare1) return REPROJ_1;
    } else {
        float u1 = fx1 * x1 * invz1 + cx1;
        float u1_r = u1 - mpCurrentKeyFrame->mbf * invz1;
        float v1 = fy1 * y1 * invz1 + cy1;
        float errX1 = u1 - kp1.x;
        float errY1 = v1 - kp1.y;
        float errX1_r = u1_r - kp1_ur;
        if ((errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r) > 7.8 * sigmaSquare1) return REPROJ_1;
    }

    const float sigmaSquare2 = pKF2->mvLevelSigma2[(size_t)kp2.octave];
    const float x2 = Rcw2.row(0).dot(x3Dt) + tcw2.at<float>(0);
    const float y2 = Rcw2.row(1).dot(x3Dt) + tcw2.at<float>(1);
    const float invz2 = 1.0 / z2;
    if (!bStereo2) {
        float u2 = fx2 * x2 * invz2 + cx2;
        float v2 = fy2 * y2 * invz2 + cy2;
        float errX2 = u2 - kp2.x;
        float errY2 = v2 - kp2.y;
        if ((errX2 * errX2 + errY2 * errY2) > 5.991 * sigmaSquare2) return REPROJ_2;
    } else {
        float u2 = fx2 * x2 * invz2 + cx2;
        float u2_r = u2 - mpCurrentKeyFrame->mbf * invz2;
        float v2 = fy2 * y2 * invz2 + cy2;
        float errX2 = u2 - kp2.x;
        float errY2 = v2 - kp2.y;
        float errX2_r = u2_r - kp2_ur;
        if ((errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r) > 7.8 * sigmaSquare2) return REPROJ_2;
    }

    cv::Mat normal1 = x3D - Ow1;
    float dist1 = cv::norm(normal1);
    cv::Mat normal2 = x3D - Ow2;
    float dist2 = cv::norm(normal2);
    if (dist1 == 0 || dist2 == 0) return DIST_ZERO;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = mpCurrentKeyFrame->mvScaleFactors[(size_t)kp1.octave] /
                              pKF2->mvScaleFactors[(size_t)kp2.octave];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return SCALE;
    for (int k = 0; k < 3; ++k) out[k] = x3D.at<float>(k);
    return code;
}

// glibc 2.35, sysdeps/ieee754/dbl-64/e_hypot.c, the kernel without a fused multiply-add
double hypot_kernel(double ax, double ay) {
    double t1, t2;
    double h = std::sqrt(ax * ax + ay * ay);
    if (h <= 2.0 * ay) {
        double delta = h - ay;
        t1 = ax * (2.0 * delta - ax);
        t2 = (delta - 2.0 * (ax - ay)) * delta;
    } else {
        double delta = h - ax;
        t1 = 2.0 * delta * (ax - 2.0 * ay);
        t2 = (4.0 * delta - ay) * ay + delta * delta;
    }
    h -= (t1 + t2) / (2.0 * h);
    return h;
}
double hypot_235(double x, double y) {
    const double SCALE_ = 0x1p-600, LARGE_VAL = 0x1p+511, TINY_VAL = 0x1p-459, EPS = 0x1p-54;
    if (!std::isfinite(x) || !std::isfinite(y)) {
        if (std::isinf(x) || std::isinf(y)) return INFINITY;
        return x + y;
    }
    x = std::fabs(x);
    y = std::fabs(y);
    double ax = x < y ? y : x, ay = x < y ? x : y;
    if (ax > LARGE_VAL) {
        if (ay <= ax * EPS) return ax + ay;
        return hypot_kernel(ax * SCALE_, ay * SCALE_) / SCALE_;
    }
    if (ay < TINY_VAL) {
        if (ax >= ay / EPS) return ax + ay;
        return hypot_kernel(ax / SCALE_, ay / SCALE_) * SCALE_;
    }
    if (ax >= ay / EPS) return ax + ay;
    return hypot_kernel(ax, ay);
}

int hypot_check(long count, unsigned long seed) {
    std::mt19937_64 g(seed);
    long bad = 0;
    auto bits = [](double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; };
    for (long i = 0; i < count; ++i) {
        // random mantissas; exponents over the whole range in a third of the draws, else close
        double x, y;
        uint64_t a = g(), b = g();
        if (i % 3 == 0) {
            std::memcpy(&x, &a, 8);
            std::memcpy(&y, &b, 8);
        } else {
            const int e = (int)(g() % 2000) - 1000, de = (int)(g() % 120) - 60;
            x = std::ldexp(1.0 + (double)(a >> 12) * 0x1p-52, e);
            y = std::ldexp(1.0 + (double)(b >> 12) * 0x1p-52, std::max(-1070, std::min(1020, e + de)));
            if (a & 1) x = -x;
        }
        volatile double xv = x, yv = y;
        const double r = hypot(xv, yv), p = hypot_235(x, y);
        if (bits(r) != bits(p) && !(std::isnan(r) && std::isnan(p))) {
            if (bad++ < 5) fprintf(stderr, "hypot(%a, %a) = %a, restated %a\n", x, y, r, p);
        }
    }
    printf("%ld of %ld differ\n", bad, count);
    return bad ? 1 : 0;
}

template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "--hypot") == 0)
        return hypot_check(std::atol(argv[2]), std::strtoul(argv[3], nullptr, 10));
    if (argc != 3) {
        fprintf(stderr, "usage: triangulate_ref cases.bin out.bin | --hypot count seed\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t ncases = 0;
    if (!rd(in, &ncases, 1)) return 2;
    double loop_seconds = 0;
    long loop_pairs = 0;
    for (int c = 0; c < ncases; ++c) {
        int32_t hdr[4];
        float ratio_factor;
        orbx_frame_pose P[2];
        if (!rd(in, hdr, 4) || !rd(in, &ratio_factor, 1) || !rd(in, P, 2)) return 2;
        const size_t n[2] = {(size_t)hdr[0], (size_t)hdr[1]};
        const int npairs = hdr[2], flags = hdr[3];
        KF kf[2] = {KF(P[0]), KF(P[1])};
        for (int k = 0; k < 2; ++k) {
            kf[k].mvKeysUn.resize(n[k]);
            if (!rd(in, kf[k].mvKeysUn.data(), n[k])) return 2;
        }
        for (int k = 0; k < 2; ++k) {
            kf[k].mvKeys = kf[k].mvKeysUn;
            if ((flags & (1 << k)) && !rd(in, kf[k].mvKeys.data(), n[k])) return 2;
        }
        for (int k = 0; k < 2; ++k) {
            kf[k].mvuRight.assign(n[k], -1.0f);
            if ((flags & (4 << k)) && !rd(in, kf[k].mvuRight.data(), n[k])) return 2;
        }
        for (int k = 0; k < 2; ++k) {
            kf[k].mvDepth.resize(n[k]);
            if (!rd(in, kf[k].mvDepth.data(), n[k])) return 2;
        }
        for (int k = 0; k < 2; ++k) {
            kf[k].cosStereo.resize(n[k]);
            if (!rd(in, kf[k].cosStereo.data(), n[k])) return 2;
        }
        std::vector<int32_t> pairs(2 * (size_t)npairs), status((size_t)npairs);
        std::vector<float> x3d(3 * (size_t)npairs, 0.0f);
        if (!rd(in, pairs.data(), pairs.size())) return 2;
        const auto t0 = std::chrono::steady_clock::now();
        for (int p = 0; p < npairs; ++p)
            status[(size_t)p] = triangulate(&kf[0], &kf[1], pairs[2 * (size_t)p],
                                            pairs[2 * (size_t)p + 1], ratio_factor,
                                            &x3d[3 * (size_t)p]);
        loop_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        loop_pairs += npairs;
        fwrite(status.data(), 4, status.size(), out);
        fwrite(x3d.data(), 4, x3d.size(), out);
    }
    fclose(in);
    printf("loop_seconds %.6f pairs %ld\n", loop_seconds, loop_pairs);
    return fclose(out) == 0 ? 0 : 2;
}
