// What Sim3Solver.cc calls in OpenCV 3.2 beyond tests/native/cv_standin (which stays as it is):
// cv::reduce, cv::gemm with flags, cv::eigen, cv::Rodrigues, cv::pow and the unrolled Mat::dot, for
// CV_32F matrices of the solver's sizes.  The arithmetic is this repository's reading of OpenCV 3.2
// (PARITY UNPINNED), written here independently of the kernels and of the numpy
// restatement; sin / cos are orbx_sincos_f64 (csrc/orbx_math.h), shared by all three.
#ifndef ORBX_CV_SIM3_STANDIN_HPP
#define ORBX_CV_SIM3_STANDIN_HPP

#include <cfloat>
#include <cmath>
#include <utility>
#include <vector>

#include <opencv2/core/core.hpp>

#include "orbx_math.h"

#define CV_REDUCE_SUM 0

namespace cv {

enum { GEMM_2_T = 2 };

// MatExpr / s = MatExpr * (1 / s): the scale of the expression takes the factor 1.0 / s
inline MatExpr operator/(const MatExpr& e, double s) { return e * (1.0 / s); }

// cv::reduce(src, dst, 1, CV_REDUCE_SUM) on CV_32F with three columns: reduceC_ starts from the
// first element, adds the elements two by two from the second on (here: none), then the rest of
// its unrolled pair, which for three columns gives (p0 + p2) + p1
inline void reduce(const Mat& src, Mat& dst, int dim, int op) {
    if (dim != 1 || op != CV_REDUCE_SUM || src.type() != CV_32F || src.cols != 3)
        throw std::invalid_argument("cv sim3 stand-in: reduce(3 columns, 1, CV_REDUCE_SUM)");
    dst.create(src.rows, 1, CV_32F);
    for (int r = 0; r < src.rows; ++r) {
        const float* p = src.ptr<float>(r);
        float a0 = p[0], a1 = p[1];
        a0 = a0 + p[2];
        dst.at<float>(r, 0) = a0 + a1;
    }
}

// cv::gemm(A, B, alpha, C, beta, D, flags).  flags == 0 with an inner length of 2..4: the
// small-matrix path (float products and sums, then (float)(t*alpha + c*beta) in double).  With
// GEMM_2_T: GEMMSingleMul<float, double>, a double sum of double products in k order.
inline void gemm(const Mat& A, const Mat& B, double alpha, const Mat& C, double beta, Mat& D,
                 int flags = 0) {
    const bool bt = flags & GEMM_2_T;
    const int m = A.rows, len = A.cols, n = bt ? B.rows : B.cols;
    if ((bt ? B.cols : B.rows) != len) throw std::invalid_argument("cv sim3 stand-in: gemm sizes");
    Mat out(m, n, CV_32F);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j) {
            const double c = C.empty() ? 0.0 : (double)C.at<float>(i, j) * beta;
            if (bt) {
                double s = 0;
                for (int k = 0; k < len; ++k) s += (double)A.at<float>(i, k) * (double)B.at<float>(j, k);
                out.at<float>(i, j) = C.empty() ? (float)(s * alpha) : (float)(s * alpha + c);
            } else {
                float t = A.at<float>(i, 0) * B.at<float>(0, j);
                for (int k = 1; k < len; ++k) t = t + A.at<float>(i, k) * B.at<float>(k, j);
                out.at<float>(i, j) = C.empty() ? (float)(t * alpha) : (float)(t * alpha + c);
            }
        }
    D = out;
}

// Mat::dot for CV_32F as dotProd_<float, double> sums it: four products per step, then the tail
inline double dot32f(const Mat& a, const Mat& b) {
    const int n = (int)a.total();
    double result = 0;
    int i = 0;
    for (; i <= n - 4; i += 4)
        result += (double)a.fel(i) * b.fel(i) + (double)a.fel(i + 1) * b.fel(i + 1) +
                  (double)a.fel(i + 2) * b.fel(i + 2) + (double)a.fel(i + 3) * b.fel(i + 3);
    for (; i < n; ++i) result += (double)a.fel(i) * b.fel(i);
    return result;
}

// cv::pow(src, 2, dst) on CV_32F: x * x
inline void pow(const Mat& src, double power, Mat& dst) {
    if (power != 2) throw std::invalid_argument("cv sim3 stand-in: pow(., 2)");
    Mat out(src.rows, src.cols, CV_32F);
    for (int r = 0; r < src.rows; ++r)
        for (int c = 0; c < src.cols; ++c) out.at<float>(r, c) = src.at<float>(r, c) * src.at<float>(r, c);
    dst = out;
}

namespace sim3_detail {
inline float hypot_(float a, float b) {
    a = std::abs(a);
    b = std::abs(b);
    if (a > b) {
        b /= a;
        return a * std::sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * std::sqrt(1 + a * a);
    }
    return 0;
}
}  // namespace sim3_detail

// cv::eigen(src, eigenvalues, eigenvectors) for a symmetric CV_32F matrix: JacobiImpl_<float>
// (lapack.cpp): the pivot is the largest off-diagonal element found through the per-row and
// per-column index tables, which are refreshed for the two rotated indices only; eps = FLT_EPSILON,
// at most n*n*30 rotations; eigenvalues sorted descending with their eigenvector rows.
inline bool eigen(const Mat& src, Mat& evals, Mat& evects) {
    const int n = src.rows;
    std::vector<float> A((size_t)n * n), V((size_t)n * n, 0.f), W(n);
    std::vector<int> indR(n, 0), indC(n, 0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) A[(size_t)i * n + j] = src.at<float>(i, j);
        V[(size_t)i * n + i] = 1.f;
    }
    const float eps = FLT_EPSILON;
    int i, k, m;
    float mv;
    for (k = 0; k < n; k++) {
        W[k] = A[(size_t)(n + 1) * k];
        if (k < n - 1) {
            for (m = k + 1, mv = std::abs(A[(size_t)n * k + m]), i = k + 2; i < n; i++) {
                const float val = std::abs(A[(size_t)n * k + i]);
                if (mv < val) mv = val, m = i;
            }
            indR[k] = m;
        }
        if (k > 0) {
            for (m = 0, mv = std::abs(A[k]), i = 1; i < k; i++) {
                const float val = std::abs(A[(size_t)n * i + k]);
                if (mv < val) mv = val, m = i;
            }
            indC[k] = m;
        }
    }
    if (n > 1)
        for (int iters = 0, maxIters = n * n * 30; iters < maxIters; iters++) {
            for (k = 0, mv = std::abs(A[indR[0]]), i = 1; i < n - 1; i++) {
                const float val = std::abs(A[(size_t)n * i + indR[i]]);
                if (mv < val) mv = val, k = i;
            }
            int l = indR[k];
            for (i = 1; i < n; i++) {
                const float val = std::abs(A[(size_t)n * indC[i] + i]);
                if (mv < val) mv = val, k = indC[i], l = i;
            }
            const float p = A[(size_t)n * k + l];
            if (std::abs(p) <= eps) break;
            const float y = (float)((W[l] - W[k]) * 0.5);
            float t = std::abs(y) + sim3_detail::hypot_(p, y);
            float s = sim3_detail::hypot_(p, t);
            const float c = t / s;
            s = p / s;
            t = (p / t) * p;
            if (y < 0) s = -s, t = -t;
            A[(size_t)n * k + l] = 0;
            W[k] -= t;
            W[l] += t;
            float a0, b0;
#define ORBX_ROTATE(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
            for (i = 0; i < k; i++) ORBX_ROTATE(A[(size_t)n * i + k], A[(size_t)n * i + l]);
            for (i = k + 1; i < l; i++) ORBX_ROTATE(A[(size_t)n * k + i], A[(size_t)n * i + l]);
            for (i = l + 1; i < n; i++) ORBX_ROTATE(A[(size_t)n * k + i], A[(size_t)n * l + i]);
            for (i = 0; i < n; i++) ORBX_ROTATE(V[(size_t)n * k + i], V[(size_t)n * l + i]);
#undef ORBX_ROTATE
            for (int j = 0; j < 2; j++) {
                const int idx = j == 0 ? k : l;
                if (idx < n - 1) {
                    for (m = idx + 1, mv = std::abs(A[(size_t)n * idx + m]), i = idx + 2; i < n; i++) {
                        const float val = std::abs(A[(size_t)n * idx + i]);
                        if (mv < val) mv = val, m = i;
                    }
                    indR[idx] = m;
                }
                if (idx > 0) {
                    for (m = 0, mv = std::abs(A[idx]), i = 1; i < idx; i++) {
                        const float val = std::abs(A[(size_t)n * i + idx]);
                        if (mv < val) mv = val, m = i;
                    }
                    indC[idx] = m;
                }
            }
        }
    for (k = 0; k < n - 1; k++) {
        m = k;
        for (i = k + 1; i < n; i++)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            std::swap(W[m], W[k]);
            for (i = 0; i < n; i++) std::swap(V[(size_t)n * m + i], V[(size_t)n * k + i]);
        }
    }
    evals.create(n, 1, CV_32F);
    evects.create(n, n, CV_32F);
    for (i = 0; i < n; ++i) {
        evals.at<float>(i, 0) = W[i];
        for (int j = 0; j < n; ++j) evects.at<float>(i, j) = V[(size_t)n * i + j];
    }
    return true;
}

// cv::Rodrigues(src, dst) for a 1x3 or 3x1 CV_32F rotation vector (calib3d, cvRodrigues2): the
// components widened to double, theta = sqrt(x*x + y*y + z*z); below DBL_EPSILON the identity,
// otherwise R = c*I + (1 - c)*r*rT + s*[r]x in double, stored as floats.  A NaN theta takes the
// second branch with s = c = NaN (orbx_sincos_f64 reports it).
inline void Rodrigues(const Mat& src, Mat& dst) {
    double rx = src.fel(0), ry = src.fel(1), rz = src.fel(2);
    const double theta = std::sqrt(rx * rx + ry * ry + rz * rz);
    dst.create(3, 3, CV_32F);
    if (theta < DBL_EPSILON) {
        Mat::eye(3, 3, CV_32F).copyTo(dst);
        return;
    }
    double s, c;
    if (!orbx::orbx_sincos_f64(theta, &s, &c)) s = c = std::nan("");
    const double c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    rx *= itheta;
    ry *= itheta;
    rz *= itheta;
    const double I[] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double rrt[] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; ++k) dst.at<float>(k / 3, k % 3) = (float)(c * I[k] + c1 * rrt[k] + s * r_x[k]);
}

}  // namespace cv

#endif  // ORBX_CV_SIM3_STANDIN_HPP
