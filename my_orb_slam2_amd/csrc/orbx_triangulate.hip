// orbx_triangulate.hip — the per-match loop behind SearchForTriangulation:
// LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:356-507 (include/orbx_match.h,
// orbx_triangulate_matches*).
//
// k_triangulate_points runs the loop body with one lane per (job, KF1 feature slot): no LDS, no
// communication between lanes but the ballot that counts a job's new points.  Work per lane is
// bounded: the Jacobi SVD runs at most SVD_MAX_SWEEPS sweeps of six column pairs.
//
// The float / double steps follow the reference's types; the library is built with
// -ffp-contract=off, so every operation is rounded on its own as on x86-64.  Forms evaluated
// inside OpenCV 3.2 are restated ([unverified-OpenCV]): the rows of A
// (cv::addWeighted), cv::SVD::compute (JacobiSVDImpl_<float>) and x3D.rowRange(0,3)/w
// (Mat::convertTo).  hypot() is glibc 2.35's (sysdeps/ieee754/dbl-64/e_hypot.c, the form without
// a fused multiply-add, which is the one x86-64 runs), restated bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbx_frame.h"
#include "../../include/orbx_match.h"
#include "orbx_cv.h"
#include "orbx_host.h"
#include "orbx_hypot.h"
#include "orbx_match_kernels.h"

using namespace orbx;

namespace {

constexpr int SVD_MAX_SWEEPS = 30;   // max(m, 30) with m = 4 (lapack.cpp, JacobiSVDImpl_)

// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a 4x4 CV_32F A, reduced to vt.row(3)
// [unverified-OpenCV]: _SVDcompute transposes A into At (row i = column i of A) and runs
// JacobiSVDImpl_<float>(At, W, Vt, m = 4, n = 4, eps = 2 * FLT_EPSILON): one-sided Jacobi on the
// rows of At, pair moments in double, rotations in float, at most 30 sweeps; then W[i] =
// sqrt(|At row i|^2) and a selection sort, descending, that moves the Vt rows with W.  The
// normalisation and completion of u do not touch vt.  A is row-major; v receives vt.row(3).
__device__ __forceinline__ void svd4_vt_row3(const float* A, float* v) {
    float At[4][4], Vt[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = A[4 * k + i];
            At[i][k] = t;
            sd = da(sd, dm((double)t, (double)t));
            Vt[i][k] = i == k ? 1.0f : 0.0f;
        }
        W[i] = sd;
    }
    const float eps = 2.0f * 1.1920928955078125e-07f;
    for (int iter = 0; iter < SVD_MAX_SWEEPS; ++iter) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i + 1; j < 4; ++j) {
                double a = W[i], p = 0.0, b = W[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) p = da(p, dm((double)At[i][k], (double)At[j][k]));
                if (fabs(p) <= dm((double)eps, __dsqrt_rn(dm(a, b)))) continue;
                p = dm(p, 2.0);
                const double beta = ds(a, b), gamma = glibc_hypot(p, beta);
                float c, s;
                if (beta < 0.0) {
                    const double delta = dm(ds(gamma, beta), 0.5);
                    s = (float)__dsqrt_rn(dv(delta, gamma));
                    c = (float)dv(p, dm(dm(gamma, (double)s), 2.0));
                } else {
                    c = (float)__dsqrt_rn(dv(da(gamma, beta), dm(gamma, 2.0)));
                    s = (float)dv(p, dm(dm(gamma, (double)c), 2.0));
                }
                a = b = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float t0 = fa(fm(c, At[i][k]), fm(s, At[j][k]));
                    const float t1 = fa(fm(-s, At[i][k]), fm(c, At[j][k]));
                    At[i][k] = t0;
                    At[j][k] = t1;
                    a = da(a, dm((double)t0, (double)t0));
                    b = da(b, dm((double)t1, (double)t1));
                }
                W[i] = a;
                W[j] = b;
                changed = true;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float t0 = fa(fm(c, Vt[i][k]), fm(s, Vt[j][k]));
                    const float t1 = fa(fm(-s, Vt[i][k]), fm(c, Vt[j][k]));
                    Vt[i][k] = t0;
                    Vt[j][k] = t1;
                }
            }
        }
        if (!changed) break;
    }
    int id[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) sd = da(sd, dm((double)At[i][k], (double)At[i][k]));
        W[i] = __dsqrt_rn(sd);
        id[i] = i;
    }
    // for i: j = argmax of W[i..] (first on ties: W[j] < W[k]); swap i and j
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k)
            if (wj < W[k]) {
                j = k;
                wj = W[k];
            }
#pragma unroll
        for (int k = i + 1; k < 4; ++k)
            if (j == k) {
                const double tw = W[i];
                W[i] = W[k];
                W[k] = tw;
                const int ti = id[i];
                id[i] = id[k];
                id[k] = ti;
            }
    }
    const int r = id[3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        v[k] = r == 0 ? Vt[0][k] : r == 1 ? Vt[1][k] : r == 2 ? Vt[2][k] : Vt[3][k];
}

// Rcw.row(r).dot(x3Dt) + tcw(r): Mat::dot in double, + the float in double, stored in a float
__device__ __forceinline__ float row_dot(const orbx_frame_pose& F, int r, const float* X) {
    return (float)da(dot3(F.Rcw + 3 * r, X), (double)F.tcw[r]);
}

// One feature of a keyframe as the loop reads it.
struct TriFeat {
    float x, y;        // mvKeysUn[idx].pt
    float rx, ry;      // mvKeys[idx].pt (UnprojectStereo)
    int octave;
    float ur;          // mvuRight[idx]
    float depth;       // mvDepth[idx]
    float cos_stereo;  // cos(2*atan2(mb/2, mvDepth[idx])), orbx_parallax_stereo_cos
};

// The reprojection test of one keyframe (:439-463 / :466-489).  mbf is the current keyframe's in
// both (:456, :482).
__device__ __forceinline__ bool reproj_ok(const orbx_frame_pose& F, const TriFeat& f, bool stereo,
                                          float mbf, float z, const float* X) {
    const float sigma2 = fm(F.scale[f.octave], F.scale[f.octave]);
    const float x = row_dot(F, 0, X), y = row_dot(F, 1, X);
    const float invz = (float)dv(1.0, (double)z);
    const float u = pinhole_frame(F.fx, F.cx, x, invz);
    const float v = pinhole_frame(F.fy, F.cy, y, invz);
    const float ex = fs(u, f.x), ey = fs(v, f.y);
    if (!stereo)
        return !((double)fa(fm(ex, ex), fm(ey, ey)) > dm(5.991, (double)sigma2));
    const float u_r = fs(u, fm(mbf, invz));
    const float er = fs(u_r, f.ur);
    return !((double)fa(fa(fm(ex, ex), fm(ey, ey)), fm(er, er)) > dm(7.8, (double)sigma2));
}

// The loop body :361-507 for one match; X receives x3D on the three OK codes.
__device__ __forceinline__ int triangulate_one(const orbx_frame_pose& F1,
                                               const orbx_frame_pose& F2, const TriFeat& f1,
                                               const TriFeat& f2, float ratio_factor, float* X) {
    const bool st1 = f1.ur >= 0.0f, st2 = f2.ur >= 0.0f;
    const float xn1[3] = {fm(fs(f1.x, F1.cx), __fdiv_rn(1.0f, F1.fx)),
                          fm(fs(f1.y, F1.cy), __fdiv_rn(1.0f, F1.fy)), 1.0f};
    const float xn2[3] = {fm(fs(f2.x, F2.cx), __fdiv_rn(1.0f, F2.fx)),
                          fm(fs(f2.y, F2.cy), __fdiv_rn(1.0f, F2.fy)), 1.0f};
    // ray = Rwc * xn; cosParallaxRays = ray1.dot(ray2) / (cv::norm(ray1) * cv::norm(ray2)).  The
    // three sums are those of orbx_cv.h's dot3 and norm3 written out, a step of each in turn:
    // through calls the kernel's instructions come out in another order.
    float ray1[3], ray2[3];
    gemm3t(F1.Rcw, xn1, ray1);
    gemm3t(F2.Rcw, xn2, ray2);
    double dot = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        dot = da(dot, dm((double)ray1[k], (double)ray2[k]));
        s1 = da(s1, dm((double)ray1[k], (double)ray1[k]));
        s2 = da(s2, dm((double)ray2[k], (double)ray2[k]));
    }
    const float cos_rays = (float)dv(dot, dm(sq(s1), sq(s2)));
    const float cps0 = fa(cos_rays, 1.0f);
    float cps1 = cps0, cps2 = cps0;
    if (st1) cps1 = f1.cos_stereo;          // :386-389: `else if`, so never both
    else if (st2) cps2 = f2.cos_stereo;
    const float cps = cps2 < cps1 ? cps2 : cps1;   // std::min(cps1, cps2)

    int code;
    if (cos_rays < cps && cos_rays > 0.0f && (st1 || st2 || (double)cos_rays < 0.9998)) {
        // A.row = xn * Tcw.row(2) - Tcw.row(r): MatOp_AddEx -> cv::addWeighted(a, xn, b, -1, 0),
        // for CV_32F evaluated in double: (float)(a*alpha + b*beta + gamma)  [unverified-OpenCV]
        float A[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t10 = k < 3 ? F1.Rcw[k] : F1.tcw[0], t11 = k < 3 ? F1.Rcw[3 + k] : F1.tcw[1],
                        t12 = k < 3 ? F1.Rcw[6 + k] : F1.tcw[2];
            const float t20 = k < 3 ? F2.Rcw[k] : F2.tcw[0], t21 = k < 3 ? F2.Rcw[3 + k] : F2.tcw[1],
                        t22 = k < 3 ? F2.Rcw[6 + k] : F2.tcw[2];
            A[k] = (float)da(da(dm((double)t12, (double)xn1[0]), dm((double)t10, -1.0)), 0.0);
            A[4 + k] = (float)da(da(dm((double)t12, (double)xn1[1]), dm((double)t11, -1.0)), 0.0);
            A[8 + k] = (float)da(da(dm((double)t22, (double)xn2[0]), dm((double)t20, -1.0)), 0.0);
            A[12 + k] = (float)da(da(dm((double)t22, (double)xn2[1]), dm((double)t21, -1.0)), 0.0);
        }
        float v[4];
        svd4_vt_row3(A, v);
        if (v[3] == 0.0f) return ORBX_TRI_W_ZERO;
        // x3D.rowRange(0,3) / w: convertTo(alpha = 1.0 / w)
        const double alpha = dv(1.0, (double)v[3]);
        // (orbx_cv.h's cvt_scale written out: through the call the kernel comes out four
        // instructions shorter and in another order)
        if (fabs(ds(alpha, 1.0)) < 2.220446049250313e-16) {
            X[0] = v[0], X[1] = v[1], X[2] = v[2];
        } else {
            const float sc = (float)alpha;
#pragma unroll
            for (int k = 0; k < 3; ++k) X[k] = fa(fm(v[k], sc), 0.0f);
        }
        code = ORBX_TRI_OK_TRIANGULATED;
    } else if (st1 && cps1 < cps2) {
        if (!(f1.depth > 0.0f)) return ORBX_TRI_LOW_PARALLAX;   // UnprojectStereo returns no point
        unproject(F1, f1.rx, f1.ry, f1.depth, X);
        code = ORBX_TRI_OK_STEREO1;
    } else if (st2 && cps2 < cps1) {
        if (!(f2.depth > 0.0f)) return ORBX_TRI_LOW_PARALLAX;
        unproject(F2, f2.rx, f2.ry, f2.depth, X);
        code = ORBX_TRI_OK_STEREO2;
    } else {
        return ORBX_TRI_LOW_PARALLAX;
    }

    const float z1 = row_dot(F1, 2, X);
    if (z1 <= 0.0f) return ORBX_TRI_BEHIND_1;
    const float z2 = row_dot(F2, 2, X);
    if (z2 <= 0.0f) return ORBX_TRI_BEHIND_2;
    if (!reproj_ok(F1, f1, st1, F1.mbf, z1, X)) return ORBX_TRI_REPROJ_1;
    if (!reproj_ok(F2, f2, st2, F1.mbf, z2, X)) return ORBX_TRI_REPROJ_2;   // :482: KF1's mbf
    // dist = (float)cv::norm(x3D - Ow)
    const float n1[3] = {fs(X[0], F1.Ow[0]), fs(X[1], F1.Ow[1]), fs(X[2], F1.Ow[2])};
    const float dist1 = norm3(n1);
    const float n2[3] = {fs(X[0], F2.Ow[0]), fs(X[1], F2.Ow[1]), fs(X[2], F2.Ow[2])};
    const float dist2 = norm3(n2);
    if (dist1 == 0.0f || dist2 == 0.0f) return ORBX_TRI_DIST_ZERO;
    const float ratio_dist = __fdiv_rn(dist2, dist1);
    const float ratio_octave = __fdiv_rn(F1.scale[f1.octave], F2.scale[f2.octave]);
    if (fm(ratio_dist, ratio_factor) < ratio_octave || ratio_dist > fm(ratio_octave, ratio_factor))
        return ORBX_TRI_SCALE;
    return code;
}

// One lane per (job, KF1 feature slot), grid (ceil(max_feat / 256), njobs); a job with more slots
// than the grid's lanes (a keyframe above max_feat) is covered by further rounds of the same
// blocks, so every slot receives a code.  The two pose records are indexed by the block, so their
// loads are uniform.
__global__ __launch_bounds__(256) void k_triangulate_points(TriPointsLaunch g) {
    const int j = blockIdx.y;
    const int a = g.kf1[j], b = g.kf2[j];
    const int s0 = g.job_off[j], span = g.job_off[j + 1] - s0;
    const bool job_ok = a >= 0 && a < g.nkf && b >= 0 && b < g.nkf;
    int n1 = 0, n2 = 0, b1 = 0, b2 = 0;
    bool levels_ok = false;
    if (job_ok) {
        b1 = g.feat_off[a];
        b2 = g.feat_off[b];
        n1 = g.feat_off[a + 1] - b1;
        n2 = g.feat_off[b + 1] - b2;
        const int l1 = g.poses[a].nlevels, l2 = g.poses[b].nlevels;
        levels_ok = l1 >= 1 && l1 <= MATCH_MAX_LEVELS && l2 >= 1 && l2 <= MATCH_MAX_LEVELS;
    }
    int nok = 0;
    for (int base = blockIdx.x * 256; base < span; base += gridDim.x * 256) {
        const int i = base + threadIdx.x;
        bool ok = false;
        if (i < span) {
            const int slot = s0 + i;
            int code = ORBX_TRI_NO_MATCH;
            bool refuse = !job_ok || !levels_ok;
            if (!refuse && i < n1) {
                const int i2 = g.match12[slot];
                if (i2 >= 0 && i2 < n2) {
                    const orbx_frame_pose& F1 = g.poses[a];
                    const orbx_frame_pose& F2 = g.poses[b];
                    const orbx_keypoint k1 = g.keys[b1 + i], k2 = g.keys[b2 + i2];
                    if (k1.octave < 0 || k1.octave >= F1.nlevels || k2.octave < 0 ||
                        k2.octave >= F2.nlevels) {
                        refuse = true;
                    } else {
                        TriFeat f1, f2;
                        f1.x = k1.x, f1.y = k1.y, f1.octave = k1.octave;
                        f2.x = k2.x, f2.y = k2.y, f2.octave = k2.octave;
                        f1.rx = k1.x, f1.ry = k1.y, f2.rx = k2.x, f2.ry = k2.y;
                        if (g.keys_raw) {
                            f1.rx = g.keys_raw[b1 + i].x, f1.ry = g.keys_raw[b1 + i].y;
                            f2.rx = g.keys_raw[b2 + i2].x, f2.ry = g.keys_raw[b2 + i2].y;
                        }
                        f1.ur = g.u_right ? g.u_right[b1 + i] : -1.0f;
                        f2.ur = g.u_right ? g.u_right[b2 + i2] : -1.0f;
                        f1.depth = g.depth[b1 + i], f2.depth = g.depth[b2 + i2];
                        f1.cos_stereo = g.cos_stereo[b1 + i];
                        f2.cos_stereo = g.cos_stereo[b2 + i2];
                        float X[3];
                        code = triangulate_one(F1, F2, f1, f2, g.ratio_factor, X);
                        ok = code <= ORBX_TRI_OK_STEREO2;
                        if (ok) {
                            g.x3d[3 * (size_t)slot] = X[0];
                            g.x3d[3 * (size_t)slot + 1] = X[1];
                            g.x3d[3 * (size_t)slot + 2] = X[2];
                        }
                    }
                } else if (i2 != -1) {
                    refuse = true;
                }
            }
            g.status[slot] = code;
            if (refuse) atomicOr(g.err, 1);
        }
        nok += (int)__popcll(__ballot(ok));
    }
    if ((threadIdx.x & 63) == 0 && nok) atomicAdd(&g.nnew[j], nok);
}

}  // namespace

namespace orbx {

hipError_t launch_triangulate_points(const TriPointsLaunch& a, int max_feat, int njobs,
                                     hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.nnew, 0, 4 * (size_t)njobs, st);
    if (e != hipSuccess || max_feat == 0) return e;
    hipLaunchKernelGGL(k_triangulate_points, dim3((max_feat + 255) / 256, njobs), dim3(256), 0, st,
                       a);
    return hipGetLastError();
}

}  // namespace orbx

extern "C" {

// LocalMapping.cc:387 / :389 with libm's double cos and atan2 (mb / 2 is a float division); see
// include/orbx_match.h on the float overloads.
orbx_status orbx_parallax_stereo_cos(float mb, const float* depth, int32_t n, float* out) {
    if (n < 0 || (n > 0 && (!depth || !out))) return ORBX_ERR_INVALID;
    const double half = (double)(mb / 2);
    for (int32_t i = 0; i < n; ++i) out[i] = (float)::cos(2 * ::atan2(half, (double)depth[i]));
    return ORBX_OK;
}

orbx_status orbx_triangulate_matches(
    const orbx_frame_pose* pose1, const orbx_frame_pose* pose2, const orbx_keypoint* keys1,
    const orbx_keypoint* keys_raw1, const float* u_right1, const float* depth1,
    const float* cos_stereo1, int32_t n1, const orbx_keypoint* keys2,
    const orbx_keypoint* keys_raw2, const float* u_right2, const float* depth2,
    const float* cos_stereo2, int32_t n2, float mb, float ratio_factor, const int32_t* pairs,
    int32_t npairs, int32_t* status, float* x3d, int32_t* nnew, int device) {
    if (!pose1 || !pose2 || n1 < 0 || n2 < 0 || npairs < 0 || !(mb >= 0.0f) ||
        (n1 > 0 && !keys1) || (n2 > 0 && !keys2) || (npairs > 0 && (!pairs || !status || !x3d)) ||
        (u_right1 && !depth1 && n1 > 0) || (u_right2 && !depth2 && n2 > 0))
        return ORBX_ERR_INVALID;
    if (pose1->nlevels < 1 || pose2->nlevels < 1) return ORBX_ERR_INVALID;
    if (pose1->nlevels > MATCH_MAX_LEVELS || pose2->nlevels > MATCH_MAX_LEVELS || n1 > 32768 ||
        n2 > 32768)
        return ORBX_ERR_UNSUPPORTED;
    std::vector<int32_t> match12((size_t)n1, -1);
    for (int32_t p = 0; p < npairs; ++p) {
        const int32_t i1 = pairs[2 * p], i2 = pairs[2 * p + 1];
        if (i1 < 0 || i1 >= n1 || i2 < 0 || i2 >= n2 || match12[(size_t)i1] != -1)
            return ORBX_ERR_INVALID;
        if (keys1[i1].octave < 0 || keys1[i1].octave >= pose1->nlevels || keys2[i2].octave < 0 ||
            keys2[i2].octave >= pose2->nlevels)
            return ORBX_ERR_INVALID;
        match12[(size_t)i1] = i2;
    }
    if (nnew) *nnew = 0;
    if (npairs == 0) return ORBX_OK;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const size_t n = (size_t)n1 + (size_t)n2;
    const bool raw = keys_raw1 || keys_raw2, stereo = u_right1 || u_right2;
    const orbx_frame_pose poses[2] = {*pose1, *pose2};
    const int32_t idx[7] = {0, n1, n1 + n2, 0, 1, 0, n1};   // feat_off[3], kf1, kf2, job_off[2]
    // a part over both frames' features: a's n1 elements, then b's n2 (zeros where null)
    auto both = [&](bool present, const void* a, const void* b, size_t elem) {
        if (!present) return StagePlan::NONE;
        const size_t o = p.in(nullptr, elem * n);
        if (a && n1) std::memcpy(p.host<uint8_t>(o), a, elem * (size_t)n1);
        if (b && n2) std::memcpy(p.host<uint8_t>(o) + elem * (size_t)n1, b, elem * (size_t)n2);
        return o;
    };
    const size_t p_pose = p.in(poses, sizeof(poses)), p_idx = p.in(idx, sizeof(idx)),
                 p_keys = both(true, keys1, keys2, sizeof(orbx_keypoint));
    const size_t p_raw = both(raw, keys_raw1 ? keys_raw1 : keys1, keys_raw2 ? keys_raw2 : keys2,
                              sizeof(orbx_keypoint));
    const size_t p_ur = stereo ? p.in(nullptr, 4 * n) : StagePlan::NONE;
    if (stereo) {
        float* ur = p.host<float>(p_ur);
        for (size_t k = 0; k < n; ++k) ur[k] = -1.0f;
        if (u_right1 && n1) std::memcpy(ur, u_right1, 4 * (size_t)n1);
        if (u_right2 && n2) std::memcpy(ur + n1, u_right2, 4 * (size_t)n2);
    }
    const size_t p_depth = both(true, depth1, depth2, 4);
    const size_t p_cos = both(true, cos_stereo1, cos_stereo2, 4);
    float* cs = p.host<float>(p_cos);
    if (!cos_stereo1 && depth1) orbx_parallax_stereo_cos(mb, depth1, n1, cs);
    if (!cos_stereo2 && depth2) orbx_parallax_stereo_cos(mb, depth2, n2, cs + n1);
    // cnt: nnew, err (zeroed with the block; the host checks came first)
    const size_t p_match = p.in(match12.data(), 4 * (size_t)n1), p_cnt = p.out(nullptr, 8, true),
                 p_status = p.out(nullptr, 4 * (size_t)n1), p_x3d = p.out(nullptr, 12 * (size_t)n1);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    TriPointsLaunch L{};
    L.nkf = 2;
    L.feat_off = c.dev<int32_t>(p_idx);
    L.keys = c.dev<orbx_keypoint>(p_keys);
    L.keys_raw = c.dev<orbx_keypoint>(p_raw);
    L.u_right = c.dev<float>(p_ur);
    L.depth = c.dev<float>(p_depth);
    L.cos_stereo = c.dev<float>(p_cos);
    L.poses = c.dev<orbx_frame_pose>(p_pose);
    L.kf1 = L.feat_off + 3;
    L.kf2 = L.feat_off + 4;
    L.job_off = L.feat_off + 5;
    L.match12 = c.dev<int32_t>(p_match);
    L.ratio_factor = ratio_factor;
    L.status = c.dev<int32_t>(p_status);
    L.x3d = c.dev<float>(p_x3d);
    L.nnew = c.dev<int32_t>(p_cnt);
    L.err = c.dev<int>(p_cnt) + 1;
    const orbx_status s =
        c.finish(HIPOK(launch_triangulate_points(L, n1, 1, c.st())) ? ORBX_OK : ORBX_ERR_DEVICE);
    if (s != ORBX_OK) return s;
    const int32_t* hs = p.host<int32_t>(p_status);
    const float* hx = p.host<float>(p_x3d);
    for (int32_t q = 0; q < npairs; ++q) {
        const int32_t i1 = pairs[2 * q];
        status[q] = hs[i1];
        if (hs[i1] <= ORBX_TRI_OK_STEREO2)
            for (int k = 0; k < 3; ++k) x3d[3 * (size_t)q + k] = hx[3 * (size_t)i1 + k];
    }
    if (nnew) *nnew = *p.host<int32_t>(p_cnt);
    return ORBX_OK;
}

}  // extern "C"
