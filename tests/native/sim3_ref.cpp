// Sim3Solver (src/Sim3Solver.cc) restated over the cv stand-in: the CPU reference of
// orbx_sim3_iterate*, independent of the kernels and of tests/sim3_cases.py, which is compared with
// it bit for bit (tests/test_sim3_cases.py).  The loops are the reference's, as cv::Mat
// statements; what the stand-in of tests/native/cv_standin lacks comes from cv_sim3_standin.hpp.
// Where the stand-in's operators would evaluate a MatExpr differently from OpenCV 3.2 as
// DESIGN.md §2 reads it (a product with a transposed operand; a matrix minus a scaled product;
// Mat::dot over nine elements), the statement is written as the cv::gemm / dot call it compiles to.
// The caller's side of the boundary is the library's: the correspondences arrive filtered, the
// minimal sets arrive as indices, max_its arrives through SetRansacParameters.
//
//   sim3_ref cases.bin out.bin        the cases of tests/sim3_cases.py (write_cases / read_results)
//   sim3_ref --atan2 in.bin out.bin   pairs of doubles (y, x) -> orbx_atan2_f64, libm atan2
//   sim3_ref --time cases.bin reps    one thread, the cases' calls `reps` times: ms per pass
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "cv_sim3_standin.hpp"
#include "orbx_frame.h"
#include "orbx_match.h"

namespace {

// (size_t)(9.210 * sigmaSquare) (:87-88); a product without a size_t value gives 0 (orbx_match.h)
size_t max_error(float sigmaSquare) {
    const double v = 9.210 * sigmaSquare;
    if (!(v >= 0)) return 0;
    if (v >= 18446744073709551615.0) return SIZE_MAX;
    return (size_t)v;
}

cv::Mat mat3(const float* p, int rows, int cols) {
    cv::Mat m(rows, cols, CV_32F);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) m.at<float>(r, c) = p[r * cols + c];
    return m;
}

struct Sim3Solver {
    int N = 0, mN1 = 0;
    bool mbFixScale = false;
    int mRansacMinInliers = 0, mRansacMaxIts = 0, mnIterations = 0, mnBestInliers = 0;
    std::vector<cv::Mat> mvX3Dc1, mvX3Dc2, mvP1im1, mvP2im2;
    std::vector<size_t> mvnMaxError1, mvnMaxError2, mvnIndices1;
    std::vector<int32_t> triples;
    cv::Mat mK1, mK2;
    cv::Mat mR12i, mt12i, mT12i, mT21i;
    float ms12i = 0;
    std::vector<bool> mvbInliersi;
    int mnInliersi = 0;
    cv::Mat mBestT12, mBestRotation, mBestTranslation;
    float mBestScale = 0;
    bool best_updated = false;

    static cv::Mat K_of(const orbx_frame_pose& F) {
        cv::Mat K = cv::Mat::eye(3, 3, CV_32F);
        K.at<float>(0, 0) = F.fx, K.at<float>(1, 1) = F.fy;
        K.at<float>(0, 2) = F.cx, K.at<float>(1, 2) = F.cy;
        return K;
    }

    // :37-112 from the records
    Sim3Solver(const orbx_frame_pose& F1, const orbx_frame_pose& F2, const float* sigma2_1,
               const float* sigma2_2, const std::vector<orbx_sim3_corr>& corr, int mN1_, bool fix)
        : mN1(mN1_), mbFixScale(fix) {
        cv::Mat Rcw1 = mat3(F1.Rcw, 3, 3), tcw1 = mat3(F1.tcw, 3, 1);
        cv::Mat Rcw2 = mat3(F2.Rcw, 3, 3), tcw2 = mat3(F2.tcw, 3, 1);
        for (const orbx_sim3_corr& c : corr) {
            mvnMaxError1.push_back(max_error(sigma2_1[c.octave1]));
            mvnMaxError2.push_back(max_error(sigma2_2[c.octave2]));
            mvnIndices1.push_back(c.i1);
            cv::Mat X3D1w = mat3(c.X1w, 3, 1);
            mvX3Dc1.push_back(Rcw1 * X3D1w + tcw1);
            cv::Mat X3D2w = mat3(c.X2w, 3, 1);
            mvX3Dc2.push_back(Rcw2 * X3D2w + tcw2);
        }
        mK1 = K_of(F1);
        mK2 = K_of(F2);
        FromCameraToImage(mvX3Dc1, mvP1im1, mK1);
        FromCameraToImage(mvX3Dc2, mvP2im2, mK2);
        N = (int)corr.size();
        mvbInliersi.resize(N);
    }

    // :140-207; returns the model when one is returned
    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers,
                    int& returned_at) {
        bNoMore = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        returned_at = 0;
        best_updated = false;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return cv::Mat();
        }
        cv::Mat P3Dc1i(3, 3, CV_32F), P3Dc2i(3, 3, CV_32F);
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            mnIterations++;
            for (short i = 0; i < 3; ++i) {
                const int idx = triples[3 * (size_t)(mnIterations - 1) + i];
                cv::Mat c1 = P3Dc1i.col(i), c2 = P3Dc2i.col(i);
                mvX3Dc1[idx].copyTo(c1);
                mvX3Dc2[idx].copyTo(c2);
            }
            ComputeSim3(P3Dc1i, P3Dc2i);
            CheckInliers();
            if (mnInliersi >= mnBestInliers) {
                mnBestInliers = mnInliersi;
                mBestT12 = mT12i.clone();
                mBestRotation = mR12i.clone();
                mBestTranslation = mt12i.clone();
                mBestScale = ms12i;
                best_updated = true;
                if (mnInliersi > mRansacMinInliers) {
                    nInliers = mnInliersi;
                    for (int i = 0; i < N; i++)
                        if (mvbInliersi[i]) vbInliers[mvnIndices1[i]] = true;
                    returned_at = mnIterations;
                    return mBestT12;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return cv::Mat();
    }

    // :215-224
    void ComputeCentroid(cv::Mat& P, cv::Mat& Pr, cv::Mat& C) {
        cv::reduce(P, C, 1, CV_REDUCE_SUM);
        C = C / P.cols;
        for (int i = 0; i < P.cols; i++) {
            cv::Mat col = Pr.col(i);
            (P.col(i) - C).copyTo(col);
        }
    }

    // :226-337
    void ComputeSim3(cv::Mat& P1, cv::Mat& P2) {
        cv::Mat Pr1(3, 3, CV_32F), Pr2(3, 3, CV_32F), O1(3, 1, CV_32F), O2(3, 1, CV_32F);
        ComputeCentroid(P1, Pr1, O1);
        ComputeCentroid(P2, Pr2, O2);
        cv::Mat M;
        cv::gemm(Pr2, Pr1, 1.0, cv::Mat(), 0.0, M, cv::GEMM_2_T);   // Pr2*Pr1.t()
        double N11, N12, N13, N14, N22, N23, N24, N33, N34, N44;
        N11 = M.at<float>(0, 0) + M.at<float>(1, 1) + M.at<float>(2, 2);
        N12 = M.at<float>(1, 2) - M.at<float>(2, 1);
        N13 = M.at<float>(2, 0) - M.at<float>(0, 2);
        N14 = M.at<float>(0, 1) - M.at<float>(1, 0);
        N22 = M.at<float>(0, 0) - M.at<float>(1, 1) - M.at<float>(2, 2);
        N23 = M.at<float>(0, 1) + M.at<float>(1, 0);
        N24 = M.at<float>(2, 0) + M.at<float>(0, 2);
        N33 = -M.at<float>(0, 0) + M.at<float>(1, 1) - M.at<float>(2, 2);
        N34 = M.at<float>(1, 2) + M.at<float>(2, 1);
        N44 = -M.at<float>(0, 0) - M.at<float>(1, 1) + M.at<float>(2, 2);
        const float n[16] = {(float)N11, (float)N12, (float)N13, (float)N14, (float)N12, (float)N22,
                             (float)N23, (float)N24, (float)N13, (float)N23, (float)N33, (float)N34,
                             (float)N14, (float)N24, (float)N34, (float)N44};
        cv::Mat Nm = mat3(n, 4, 4);
        cv::Mat eval, evec;
        cv::eigen(Nm, eval, evec);
        cv::Mat vec(1, 3, CV_32F);
        (evec.row(0).colRange(1, 4)).copyTo(vec);
        const double ang = orbx::orbx_atan2_f64(cv::norm(vec), evec.at<float>(0, 0));
        vec = 2 * ang * vec / cv::norm(vec);
        mR12i.create(3, 3, CV_32F);
        cv::Rodrigues(vec, mR12i);
        cv::Mat P3 = mR12i * Pr2;
        if (!mbFixScale) {
            const double nom = cv::dot32f(Pr1, P3);
            cv::Mat aux_P3(3, 3, CV_32F);
            cv::pow(P3, 2, aux_P3);
            double den = 0;
            for (int i = 0; i < aux_P3.rows; i++)
                for (int j = 0; j < aux_P3.cols; j++) den += aux_P3.at<float>(i, j);
            ms12i = nom / den;
        } else
            ms12i = 1.0f;
        cv::gemm(mR12i, O2, -(double)ms12i, O1, 1.0, mt12i);   // O1 - ms12i*mR12i*O2
        mT12i = cv::Mat::eye(4, 4, CV_32F);
        cv::Mat sR = ms12i * mR12i;
        cv::Mat b12 = mT12i.rowRange(0, 3).colRange(0, 3), c12 = mT12i.rowRange(0, 3).col(3);
        sR.copyTo(b12);
        mt12i.copyTo(c12);
        mT21i = cv::Mat::eye(4, 4, CV_32F);
        cv::Mat sRinv = (1.0 / ms12i) * mR12i.t();
        cv::Mat b21 = mT21i.rowRange(0, 3).colRange(0, 3), c21 = mT21i.rowRange(0, 3).col(3);
        sRinv.copyTo(b21);
        cv::Mat tinv = -sRinv * mt12i;
        tinv.copyTo(c21);
    }

    // :340-364
    void CheckInliers() {
        std::vector<cv::Mat> vP1im2, vP2im1;
        Project(mvX3Dc2, vP2im1, mT12i, mK1);
        Project(mvX3Dc1, vP1im2, mT21i, mK2);
        mnInliersi = 0;
        for (size_t i = 0; i < mvP1im1.size(); i++) {
            cv::Mat dist1 = mvP1im1[i] - vP2im1[i];
            cv::Mat dist2 = vP1im2[i] - mvP2im2[i];
            const float err1 = dist1.dot(dist1);
            const float err2 = dist2.dot(dist2);
            if (err1 < mvnMaxError1[i] && err2 < mvnMaxError2[i]) {
                mvbInliersi[i] = true;
                mnInliersi++;
            } else
                mvbInliersi[i] = false;
        }
    }

    // :382-403
    void Project(const std::vector<cv::Mat>& vP3Dw, std::vector<cv::Mat>& vP2D, cv::Mat Tcw, cv::Mat K) {
        cv::Mat Rcw = Tcw.rowRange(0, 3).colRange(0, 3);
        cv::Mat tcw = Tcw.rowRange(0, 3).col(3);
        const float fx = K.at<float>(0, 0), fy = K.at<float>(1, 1);
        const float cx = K.at<float>(0, 2), cy = K.at<float>(1, 2);
        vP2D.clear();
        for (size_t i = 0, iend = vP3Dw.size(); i < iend; i++) {
            cv::Mat P3Dc = Rcw * vP3Dw[i] + tcw;
            const float invz = 1 / (P3Dc.at<float>(2));
            const float x = P3Dc.at<float>(0) * invz;
            const float y = P3Dc.at<float>(1) * invz;
            cv::Mat p(2, 1, CV_32F);
            p.at<float>(0) = fx * x + cx;
            p.at<float>(1) = fy * y + cy;
            vP2D.push_back(p);
        }
    }

    // :405-423
    void FromCameraToImage(const std::vector<cv::Mat>& vP3Dc, std::vector<cv::Mat>& vP2D, cv::Mat K) {
        const float fx = K.at<float>(0, 0), fy = K.at<float>(1, 1);
        const float cx = K.at<float>(0, 2), cy = K.at<float>(1, 2);
        vP2D.clear();
        for (size_t i = 0, iend = vP3Dc.size(); i < iend; i++) {
            const float invz = 1 / (vP3Dc[i].at<float>(2));
            const float x = vP3Dc[i].at<float>(0) * invz;
            const float y = vP3Dc[i].at<float>(1) * invz;
            cv::Mat p(2, 1, CV_32F);
            p.at<float>(0) = fx * x + cx;
            p.at<float>(1) = fy * y + cy;
            vP2D.push_back(p);
        }
    }
};

struct Case {
    int32_t hdr[10];   // N, mN1, fix_scale, min_inliers, max_its, ncalls, state0[2], nlevels1, nlevels2
    orbx_frame_pose F1, F2;
    float sigma2_1[16], sigma2_2[16];
    std::vector<orbx_sim3_corr> corr;
    std::vector<int32_t> triples, calls;
};

bool read_cases(const char* path, std::vector<Case>& cases) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t n = 0;
    bool ok = std::fread(&n, 4, 1, f) == 1;
    for (int32_t k = 0; ok && k < n; ++k) {
        Case c;
        ok = std::fread(c.hdr, 4, 10, f) == 10 && std::fread(&c.F1, sizeof(c.F1), 1, f) == 1 &&
             std::fread(&c.F2, sizeof(c.F2), 1, f) == 1 && std::fread(c.sigma2_1, 4, 16, f) == 16 &&
             std::fread(c.sigma2_2, 4, 16, f) == 16;
        if (!ok) break;
        c.corr.resize(c.hdr[0]);
        c.triples.resize(3 * (size_t)c.hdr[4]);
        c.calls.resize(c.hdr[5]);
        ok = std::fread(c.corr.data(), sizeof(orbx_sim3_corr), c.corr.size(), f) == c.corr.size() &&
             std::fread(c.triples.data(), 4, c.triples.size(), f) == c.triples.size() &&
             std::fread(c.calls.data(), 4, c.calls.size(), f) == c.calls.size();
        cases.push_back(c);
    }
    std::fclose(f);
    return ok;
}

// One case's calls; out (may be null) receives per call the result record (0xCC where nothing is
// written), the mN1 inlier bytes and the state.
void run_case(const Case& c, FILE* out) {
    Sim3Solver s(c.F1, c.F2, c.sigma2_1, c.sigma2_2, c.corr, c.hdr[1], c.hdr[2] != 0);
    s.mRansacMinInliers = c.hdr[3];
    s.mRansacMaxIts = c.hdr[4];
    s.mnIterations = c.hdr[6];
    s.mnBestInliers = c.hdr[7];
    s.triples = c.triples;
    for (int32_t n_iterations : c.calls) {
        bool bNoMore;
        std::vector<bool> vbInliers;
        int nInliers, at;
        cv::Mat T = s.iterate(n_iterations, bNoMore, vbInliers, nInliers, at);
        orbx_sim3_result r;
        std::memset(&r, 0xCC, sizeof(r));
        r.found = !T.empty();
        r.iteration = at;
        r.n_inliers = nInliers;
        r.no_more = bNoMore;
        r.info = 0;
        r.best_updated = s.best_updated;
        if (s.best_updated) {
            r.best_inliers = s.mnBestInliers;
            for (int k = 0; k < 9; ++k) r.R12[k] = s.mBestRotation.fel(k);
            for (int k = 0; k < 3; ++k) r.t12[k] = s.mBestTranslation.fel(k);
            r.s12 = s.mBestScale;
            for (int k = 0; k < 16; ++k) r.T12[k] = s.mBestT12.fel(k);
        }
        if (!out) continue;
        std::fwrite(&r, sizeof(r), 1, out);
        for (int i = 0; i < s.mN1; ++i) std::fputc(vbInliers[i] ? 1 : 0, out);
        const int32_t st[2] = {s.mnIterations, s.mnBestInliers};
        std::fwrite(st, 4, 2, out);
    }
}

int run_atan2(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    FILE* g = std::fopen(out, "wb");
    if (!f || !g) return 2;
    double yx[2];
    while (std::fread(yx, 8, 2, f) == 2) {
        const double r[2] = {orbx::orbx_atan2_f64(yx[0], yx[1]), std::atan2(yx[0], yx[1])};
        std::fwrite(r, 8, 2, g);
    }
    std::fclose(f);
    std::fclose(g);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "--atan2") return run_atan2(argv[2], argv[3]);
    if (argc == 4 && std::string(argv[1]) == "--time") {
        std::vector<Case> cases;
        if (!read_cases(argv[2], cases)) return 2;
        const int reps = std::atoi(argv[3]);
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; ++r)
            for (const Case& c : cases) run_case(c, nullptr);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%.6f\n", ms / (reps > 0 ? reps : 1));
        return 0;
    }
    if (argc != 3) {
        std::fprintf(stderr, "usage: sim3_ref cases.bin out.bin | --atan2 in out | --time cases reps\n");
        return 2;
    }
    std::vector<Case> cases;
    if (!read_cases(argv[1], cases)) return 2;
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    for (const Case& c : cases) run_case(c, out);
    std::fclose(out);
    return 0;
}
