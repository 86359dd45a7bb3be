// orbx_cv.h — the small arithmetic forms of OpenCV 3.2 that the geometry kernels restate, once
// (orbx_frame.hip, orbx_triangulate.hip, orbx_sim3.hip, orbx_sim3opt.hip, orbx_poseopt.hip,
// orbx_pnp.hip, orbx_localmap.hip), and the exactly rounded one-line wrappers they and orbx_lm.h / orbx_hypot.h are
// written with.  Device code.  Every form is restated from the library's sources and PARITY
// UNPINNED [unverified-OpenCV]: one found wrong against the real library is fixed
// here.  The x86 integer conversions (x86_trunc, cv_round) are orbx_math.h's, which host code
// shares.  The forms are spelled with the _rn intrinsics, one operation and one rounding each; the
// callers' own arithmetic keeps its spelling (with -ffp-contract=off a * b + c is two roundings too).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbx_frame.h"
#include "orbx_math.h"

namespace orbx {

// ---- one operation, one rounding ----------------------------------------------------------------
__device__ __forceinline__ float fm(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float fa(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float fs(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double dm(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double da(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double ds(double a, double b) { return __dsub_rn(a, b); }
// IEEE division and square root whatever the compiler's defaults
__device__ __forceinline__ double dv(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ double sq(double a) { return __dsqrt_rn(a); }
__device__ __forceinline__ float fdiv(float a, float b) { return __fdiv_rn(a, b); }
// sqrtf correctly rounded whatever the compiler's defaults (__fsqrt_rn is the native, approximate
// instruction unless the headers are configured otherwise): the double square root of a float,
// rounded to float, is the correctly rounded float square root (53 >= 2 * 24 + 2 bits)
__device__ __forceinline__ float fsqrt(float a) { return (float)__dsqrt_rn((double)a); }

// ---- cv::gemm, the small-matrix path (len 3, one column) ----------------------------------------
// t_r = a_r0*b0 + a_r1*b1 + a_r2*b2 in float, then d_r = (float)(t_r*alpha + c_r*beta) in double.
// row3 is t_r for a 3x3 A (row-major) and a 3-vector, for the callers with an alpha or beta of
// their own.
__device__ __forceinline__ float row3(const float* A, int r, const float* b) {
    float t = fm(A[3 * r], b[0]);
    t = fa(t, fm(A[3 * r + 1], b[1]));
    return fa(t, fm(A[3 * r + 2], b[2]));
}
// the same row of A.t() (GEMM_1_T)
__device__ __forceinline__ float row3t(const float* A, int r, const float* b) {
    float t = fm(A[r], b[0]);
    t = fa(t, fm(A[3 + r], b[1]));
    return fa(t, fm(A[6 + r], b[2]));
}
// R*P + t: cv::gemm(R, P, 1, t, 1), d_r = (float)(t_r*1.0 + c_r*1.0); gemm3_row is d_r, for
// k_sim3_opt, which takes the rows of its two products in turn
__device__ __forceinline__ float gemm3_row(const float* R, int r, const float* P, const float* t) {
    return (float)((double)row3(R, r, P) + (double)t[r]);
}
__device__ __forceinline__ void gemm3(const float* __restrict__ R, const float* P,
                                      const float* __restrict__ t, float* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = gemm3_row(R, r, P, t);
}
// R.t()*c + t, and R.t()*c with no added term: d_r = t_r
__device__ __forceinline__ void gemm3t(const float* R, const float* c, const float* t, float* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = (float)((double)row3t(R, r, c) + (double)t[r]);
}
__device__ __forceinline__ void gemm3t(const float* R, const float* c, float* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = row3t(R, r, c);
}

// ---- cv::norm, Mat::dot, Mat::convertTo ---------------------------------------------------------
// (float)cv::norm(a), NORM_L2 on CV_32F: squares accumulated in double (normL2Sqr<float,
// double>), sqrt, stored in a float; norm3d is the double cv::norm returns
__device__ __forceinline__ double norm3d(const float* a) {
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) ss = da(ss, dm((double)a[k], (double)a[k]));
    return sq(ss);
}
__device__ __forceinline__ float norm3(const float* a) { return (float)norm3d(a); }

// a.dot(b) of two CV_32F 3-vectors: Mat::dot in double (dotProd_<float, double>; below four
// elements there is no 4-at-a-time step)
__device__ __forceinline__ double dot3(const float* a, const float* b) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) s = da(s, dm((double)a[k], (double)b[k]));
    return s;
}

// Mat::convertTo(alpha) on a CV_32F value: a plain copy when |alpha - 1| < DBL_EPSILON, otherwise
// x * (float)alpha + 0.0f
__device__ __forceinline__ float cvt_scale(float x, double alpha) {
    if (fabs(ds(alpha, 1.0)) < 2.220446049250313e-16) return x;
    return fa(fm(x, (float)alpha), 0.0f);
}

// b + a / s for CV_32F a, b and a double s: MatOp_AddEx::add folds the scaled operand into
// cv::scaleAdd(a, 1. / s, b) (matop.cpp), whose CV_32F kernel takes alpha as a float and computes
// a * alpha + b with the product and the sum rounded on their own (scaleAdd_32f, matmul.cpp).
// scale_add_alpha is (float)(1. / s); one element is scale_add_sum(scale_add_term(a, alpha), b),
// in two steps for k_refresh_map_points, which takes the products of a sum's terms in parallel.
__device__ __forceinline__ float scale_add_alpha(double s) { return (float)dv(1.0, s); }
__device__ __forceinline__ float scale_add_term(float a, float alpha) { return fm(a, alpha); }
__device__ __forceinline__ float scale_add_sum(float term, float b) { return fa(term, b); }

// ---- the pinhole, PredictScale, UnprojectStereo, the camera centre -------------------------------
// One image coordinate from a camera-frame coordinate X and invz = 1 / z.  Frame's loops write
// fx*X*invz + cx (Frame::isInFrustum, SearchByProjection from a Frame, CreateNewMapPoints),
// KeyFrame's and Sim3Solver's x = X*invz; fx*x + cx (Fuse, SearchBySim3, the Scw search,
// Sim3Solver::Project / FromCameraToImage).
__device__ __forceinline__ float pinhole_frame(float f, float c, float X, float invz) {
    return fa(fm(fm(f, X), invz), c);
}
__device__ __forceinline__ float pinhole_kf(float f, float c, float X, float invz) {
    return fa(fm(f, fm(X, invz)), c);
}

// MapPoint::PredictScale (MapPoint.cc:430-444) and the clamp of its callers:
// ceil(log(max_dist / dist) / mfLogScaleFactor) on floats (std::log / std::ceil, glibc's logf
// restated in orbx_math.h), the reference's (int), then [0, nlevels - 1].  The caller passes
// log_ratio = glibc_logf(max_dist / dist): as the first argument it is evaluated ahead of the
// frame's two fields, which k_frustum and k_project load behind the logarithm.
__device__ __forceinline__ int predict_level(float log_ratio, float log_scale_factor, int nlevels) {
    const int lvl = x86_trunc(ceilf(fdiv(log_ratio, log_scale_factor)));
    return lvl < 0 ? 0 : lvl >= nlevels ? nlevels - 1 : lvl;
}

// Frame::UnprojectStereo (src/Frame.cc:713-727) / KeyFrame::UnprojectStereo (KeyFrame.cc:629-645)
// for z > 0: x = (u - cx) * z * invfx, y likewise, x3D = Rwc * (x, y, z) + Ow; Rwc is the
// transpose of F.Rcw.
__device__ __forceinline__ void unproject(const orbx_frame_pose& F, float u, float v, float z,
                                          float* out) {
    const float invfx = fdiv(1.0f, F.fx), invfy = fdiv(1.0f, F.fy);
    const float c[3] = {fm(fm(fs(u, F.cx), z), invfx), fm(fm(fs(v, F.cy), z), invfy), z};
    gemm3t(F.Rcw, c, F.Ow, out);
}

// Frame::UpdatePoseMatrices: mOw = -mRcw.t() * mtcw, the sign applied to the float row sum;
// camera_centre_row is component r, for k_pose_opt, which writes tcw[r] and Ow[r] in turn
__device__ __forceinline__ float camera_centre_row(const float* R, const float* t, int r) {
    return -row3t(R, r, t);
}
__device__ __forceinline__ void camera_centre(const float* R, const float* t, float* Ow) {
#pragma unroll
    for (int r = 0; r < 3; ++r) Ow[r] = camera_centre_row(R, t, r);
}

}  // namespace orbx
