// orbx_sim3.hip — Sim3Solver::iterate (src/Sim3Solver.cc:140-207) on the device: Horn's closed
// form from three correspondences (ComputeSim3, :226-337) inside the reference's RANSAC loop, with
// CheckInliers (:340-364) over every correspondence (include/orbx_match.h, orbx_sim3_*).
//
//   k_sim3_prepare     one lane per correspondence: the constructor's per-correspondence work
//                      (:81-109), i.e. both camera-frame points, both image points, both bounds
//   k_sim3_hypotheses  one wave per iteration of the call: the model, computed by every lane alike
//                      in registers, then the lanes stride over the correspondences and count the
//                      inliers with ballots (integers: the order cannot change them)
//   k_sim3_select      one wave per job: the iterations' counts walked in order against the running
//                      best (:183-199), the returned model re-scored for the inlier bytes, the state
//
// What is RANSAC and not Horn (the sampling, the iteration count, the window of a call, the cursor
// scratch_of() is written with) is orbx_ransac.h's, shared with orbx_pnp.hip.  Both entry points
// are here: orbx_sim3_iterate, and orbx_sim3_iterate_batch_device on a handle (orbx_matcher.h).
//
// The library is built with -ffp-contract=off: every operation below is rounded on its own as on
// x86-64.  The forms evaluated inside OpenCV 3.2 (cv::reduce, Mat::convertTo, cv::gemm's two paths,
// cv::eigen's JacobiImpl_<float>, cv::norm, cv::Rodrigues, Mat::dot, cv::pow) are restated and
// PARITY UNPINNED.  atan2, sin and cos of doubles are orbx_math.h's, shared with the
// restatements the kernels are tested against.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/orbx_frame.h"
#include "../../include/orbx_match.h"
#include "orbx_cv.h"
#include "orbx_host.h"
#include "orbx_match_kernels.h"
#include "orbx_matcher.h"
#include "orbx_math.h"
#include "orbx_ransac.h"

using namespace orbx;

namespace {

// What k_sim3_prepare leaves per correspondence (64 bytes).
struct Sim3Prep {
    float X1[3], X2[3];   // mvX3Dc1, mvX3Dc2
    float p1[2], p2[2];   // mvP1im1, mvP2im2
    float m1, m2;         // (float)mvnMaxError1, (float)mvnMaxError2
    int32_t i1;
    int32_t pad[3];
};
// What k_sim3_hypotheses leaves per iteration (144 bytes).
struct Sim3Hyp {
    float R[9], t[3], s;      // mR12i, mt12i, ms12i
    float sR[9];              // mT12i's rotation block (its translation is t)
    float sRinv[9], tinv[3];  // mT21i
    int32_t count;            // mnInliersi
};

// lapack.cpp's hypot<float>
__device__ __forceinline__ float cv_hypotf(float a, float b) {
    a = fabsf(a);
    b = fabsf(b);
    if (a > b) {
        b = fdiv(b, a);
        return a * fsqrt(1.0f + b * b);
    }
    if (b > 0.0f) {
        a = fdiv(a, b);
        return b * fsqrt(1.0f + a * a);
    }
    return 0.0f;
}

// JacobiImpl_<float> on a symmetric 4x4 (cv::eigen): every index below is a compile-time constant
// after unrolling, so the matrix, the vectors and the two index tables stay in registers.
struct Jac {
    float A[4][4], V[4][4], W[4];
    int indR[4], indC[4];
};

template <int IDX> __device__ __forceinline__ void jac_update_ind(Jac& J) {
    if constexpr (IDX < 3) {
        int m = IDX + 1;
        float mv = fabsf(J.A[IDX][IDX + 1]);
#pragma unroll
        for (int i = IDX + 2; i < 4; ++i) {
            const float val = fabsf(J.A[IDX][i]);
            if (mv < val) mv = val, m = i;
        }
        J.indR[IDX] = m;
    }
    if constexpr (IDX > 0) {
        int m = 0;
        float mv = fabsf(J.A[0][IDX]);
#pragma unroll
        for (int i = 1; i < IDX; ++i) {
            const float val = fabsf(J.A[i][IDX]);
            if (mv < val) mv = val, m = i;
        }
        J.indC[IDX] = m;
    }
}

__device__ __forceinline__ void jac_rotate(float& v0, float& v1, float c, float s) {
    const float a0 = v0, b0 = v1;
    v0 = a0 * c - b0 * s;
    v1 = a0 * s + b0 * c;
}

// One iteration with the pivot (K, L), K < L; false: |p| <= eps, the loop ends.
template <int K, int L> __device__ __forceinline__ bool jac_step(Jac& J) {
    const float p = J.A[K][L];
    if (fabsf(p) <= 1.1920928955078125e-07f) return false;
    const float y = (float)((double)(J.W[L] - J.W[K]) * 0.5);
    float t = fabsf(y) + cv_hypotf(p, y);
    float s = cv_hypotf(p, t);
    const float c = fdiv(t, s);
    s = fdiv(p, s);
    t = fdiv(p, t) * p;
    if (y < 0.0f) s = -s, t = -t;
    J.A[K][L] = 0.0f;
    J.W[K] -= t;
    J.W[L] += t;
#pragma unroll
    for (int i = 0; i < K; ++i) jac_rotate(J.A[i][K], J.A[i][L], c, s);
#pragma unroll
    for (int i = K + 1; i < L; ++i) jac_rotate(J.A[K][i], J.A[i][L], c, s);
#pragma unroll
    for (int i = L + 1; i < 4; ++i) jac_rotate(J.A[K][i], J.A[L][i], c, s);
#pragma unroll
    for (int i = 0; i < 4; ++i) jac_rotate(J.V[K][i], J.V[L][i], c, s);
    jac_update_ind<K>(J);
    jac_update_ind<L>(J);
    return true;
}

__device__ __forceinline__ float pick4(const float* r, int j) {
    return j == 0 ? r[0] : j == 1 ? r[1] : j == 2 ? r[2] : r[3];
}

// cv::eigen(N, eval, evec) reduced to evec.row(0): eigenvalues sorted descending, the eigenvector
// rows moved with them.  N is row-major and symmetric; only its upper triangle is read.
__device__ __forceinline__ void eigen4_top(const float* N, float* q) {
    Jac J;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            J.A[i][j] = N[4 * i + j];
            J.V[i][j] = i == j ? 1.0f : 0.0f;
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        J.W[k] = J.A[k][k];
        J.indR[k] = 0;
        J.indC[k] = 0;
    }
    jac_update_ind<0>(J);
    jac_update_ind<1>(J);
    jac_update_ind<2>(J);
    jac_update_ind<3>(J);
    for (int iters = 0; iters < 4 * 4 * 30; ++iters) {
        int k = 0;
        float mv = fabsf(pick4(J.A[0], J.indR[0]));
#pragma unroll
        for (int i = 1; i < 3; ++i) {
            const float val = fabsf(pick4(J.A[i], J.indR[i]));
            if (mv < val) mv = val, k = i;
        }
        int l = k == 0 ? J.indR[0] : k == 1 ? J.indR[1] : J.indR[2];
#pragma unroll
        for (int i = 1; i < 4; ++i) {
            const int r = J.indC[i];
            const float val = fabsf(r == 0 ? J.A[0][i] : r == 1 ? J.A[1][i] : J.A[2][i]);
            if (mv < val) mv = val, k = r, l = i;
        }
        bool more;
        switch (4 * k + l) {
            case 1: more = jac_step<0, 1>(J); break;
            case 2: more = jac_step<0, 2>(J); break;
            case 3: more = jac_step<0, 3>(J); break;
            case 6: more = jac_step<1, 2>(J); break;
            case 7: more = jac_step<1, 3>(J); break;
            default: more = jac_step<2, 3>(J); break;
        }
        if (!more) break;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int m = k;
        float wm = J.W[k];
#pragma unroll
        for (int i = k + 1; i < 4; ++i)
            if (wm < J.W[i]) wm = J.W[i], m = i;
#pragma unroll
        for (int i = k + 1; i < 4; ++i)
            if (m == i) {
                const float tw = J.W[i];
                J.W[i] = J.W[k];
                J.W[k] = tw;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float tv = J.V[i][c];
                    J.V[i][c] = J.V[k][c];
                    J.V[k][c] = tv;
                }
            }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = J.V[0][c];
}

// ComputeCentroid (:215-224): cv::reduce's row sum in reduceC_'s order, C / P.cols as convertTo
// with alpha = 1.0 / 3, then the float differences.  P[r][i] is component r of point i.
__device__ __forceinline__ void centroid(const float (*P)[3], float (*Pr)[3], float* C) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float sum = (P[r][0] + P[r][2]) + P[r][1];
        C[r] = cvt_scale(sum, 1.0 / 3);
#pragma unroll
        for (int i = 0; i < 3; ++i) Pr[r][i] = P[r][i] - C[r];
    }
}

// ComputeSim3 (:226-337)
__device__ __forceinline__ void compute_sim3(const float (*P1)[3], const float (*P2)[3],
                                             bool fix_scale, Sim3Hyp& H) {
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
    // M = Pr2 * Pr1.t(): GEMM_2_T takes the general path, double sums of double products
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s = s + (double)Pr2[i][k] * (double)Pr1[j][k];
            M[i][j] = (float)(s * 1.0);
        }
    const float N11 = (M[0][0] + M[1][1]) + M[2][2], N12 = M[1][2] - M[2][1],
                N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0],
                N22 = (M[0][0] - M[1][1]) - M[2][2], N23 = M[0][1] + M[1][0],
                N24 = M[2][0] + M[0][2], N33 = (-M[0][0] + M[1][1]) - M[2][2],
                N34 = M[1][2] + M[2][1], N44 = (-M[0][0] - M[1][1]) + M[2][2];
    const float N[16] = {N11, N12, N13, N14, N12, N22, N23, N24,
                         N13, N23, N33, N34, N14, N24, N34, N44};
    float q[4];
    eigen4_top(N, q);
    // norm(vec) in double; ang = atan2(norm, evec(0,0)); vec = 2*ang*vec/norm(vec) as one scaling
    double ss = 0.0;
#pragma unroll
    for (int k = 1; k < 4; ++k) ss = ss + (double)q[k] * (double)q[k];
    const double nrm = sq(ss);
    const double ang = orbx_atan2_f64(nrm, (double)q[0]);
    const double alpha = (2 * ang) * dv(1.0, nrm);
    float vec[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vec[k] = cvt_scale(q[k + 1], alpha);
    // cv::Rodrigues of the 1x3 float vector
    double rx = vec[0], ry = vec[1], rz = vec[2];
    const double theta = sq((rx * rx + ry * ry) + rz * rz);
    if (theta < 2.220446049250313e-16) {
#pragma unroll
        for (int k = 0; k < 9; ++k) H.R[k] = (k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f;
    } else {
        double c, s;
        if (!orbx_sincos_f64(theta, &s, &c)) s = c = (double)NAN;   // theta is NaN (<= 2*pi else)
        const double c1 = 1. - c, itheta = dv(1., theta);
        rx *= itheta, ry *= itheta, rz *= itheta;
        const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry,
                               ry * rz, rx * rz, ry * rz, rz * rz};
        const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double I = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
            H.R[k] = (float)((c * I + c1 * rrt[k]) + s * r_x[k]);
        }
    }
    // P3 = mR12i * Pr2: the small-matrix path
    float P3[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float t = H.R[3 * r] * Pr2[0][i];
            t = t + H.R[3 * r + 1] * Pr2[1][i];
            P3[r][i] = t + H.R[3 * r + 2] * Pr2[2][i];
        }
    if (!fix_scale) {
        // Pr1.dot(P3): dotProd_<float, double>, four products per step, then the tail
        const float* a = &Pr1[0][0];
        const float* b = &P3[0][0];
        double nom = 0.0;
#pragma unroll
        for (int i = 0; i < 8; i += 4)
            nom = nom + ((((double)a[i] * b[i] + (double)a[i + 1] * b[i + 1]) +
                          (double)a[i + 2] * b[i + 2]) + (double)a[i + 3] * b[i + 3]);
        nom = nom + (double)a[8] * b[8];
        double den = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) den = den + (double)(b[i] * b[i]);   // cv::pow(P3, 2) in float
        H.s = (float)dv(nom, den);
    } else {
        H.s = 1.0f;
    }
    // mt12i = O1 - ms12i*mR12i*O2: one gemm, alpha = -ms12i, C = O1, beta = 1
    const double ds12 = (double)H.s;
#pragma unroll
    for (int r = 0; r < 3; ++r)
        H.t[r] = (float)((double)row3(H.R, r, O2) * -ds12 + (double)O1[r] * 1.0);
    // sR = ms12i*mR12i, sRinv = (1.0/ms12i)*mR12i.t(): convertTo scalings
    const double inv_s = dv(1.0, ds12);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            H.sR[3 * r + c] = cvt_scale(H.R[3 * r + c], ds12);
            H.sRinv[3 * r + c] = cvt_scale(H.R[3 * c + r], inv_s);
        }
    // tinv = -sRinv*mt12i: gemm with alpha = -1
#pragma unroll
    for (int r = 0; r < 3; ++r) H.tinv[r] = (float)((double)row3(H.sRinv, r, H.t) * -1.0);
}

// Project (:382-403): Rcw*X + tcw in the small-matrix path with C = tcw, then the pinhole
__device__ __forceinline__ void project(const float* R, const float* t, const float* X, float fx,
                                        float fy, float cx, float cy, float* uv) {
    float P[3];
    gemm3(R, X, t, P);
    const float invz = fdiv(1.0f, P[2]);
    uv[0] = pinhole_kf(fx, cx, P[0], invz);
    uv[1] = pinhole_kf(fy, cy, P[1], invz);
}

// CheckInliers' body (:350-356) for one correspondence
__device__ __forceinline__ bool is_inlier(const Sim3Prep& q, const Sim3Hyp& H,
                                          const orbx_frame_pose& K1, const orbx_frame_pose& K2) {
    float a[2], b[2];
    project(H.sR, H.t, q.X2, K1.fx, K1.fy, K1.cx, K1.cy, a);        // vP2im1
    project(H.sRinv, H.tinv, q.X1, K2.fx, K2.fy, K2.cx, K2.cy, b);  // vP1im2
    const float d10 = q.p1[0] - a[0], d11 = q.p1[1] - a[1];
    const float d20 = b[0] - q.p2[0], d21 = b[1] - q.p2[1];
    const float err1 = (float)((0.0 + (double)d10 * d10) + (double)d11 * d11);
    const float err2 = (float)((0.0 + (double)d20 * d20) + (double)d21 * d21);
    return err1 < q.m1 && err2 < q.m2;
}

// (float)(size_t)(9.210 * sigma2): the double product truncated (:87-88), compared as a float
// (:356).  A product that is negative or NaN has no size_t: the bound is 0, nothing is an inlier.
__device__ __forceinline__ float max_error(float sigma2) {
    const double v = 9.210 * (double)sigma2;
    if (!(v >= 0.0)) return 0.0f;
    if (v >= 18446744073709551615.0) return 18446744073709551615.0f;
    return (float)(unsigned long long)v;
}

struct Sim3Scratch {
    uint32_t* info;      // per job: what the kernels refused; first: launch_sim3 zeroes it
    Sim3Prep* prep;      // [njobs][max_n]
    Sim3Hyp* hyp;        // [njobs][max_call]
    size_t end;          // the bytes of the whole
};
__host__ __device__ inline Sim3Scratch scratch_of(void* base, int njobs, int max_n, int max_call) {
    ScratchCursor c{(uint8_t*)base};
    Sim3Scratch s;
    s.info = c.take<uint32_t>(njobs);
    s.prep = c.take<Sim3Prep>(njobs, max_n);
    s.hyp = c.take<Sim3Hyp>(njobs, max_call);
    s.end = c.end;
    return s;
}

// The iterations of this call: [S.iterations, S.iterations + sim3_window(J, S))
__device__ __forceinline__ int sim3_window(const orbx_sim3_job& J, const orbx_sim3_state& S) {
    return ransac_window_and(J.max_its, S.iterations, J.n_iterations);
}

// What the job record alone shows; the same in all three kernels.
__device__ __forceinline__ uint32_t job_refusal(const Sim3Launch& g, const orbx_sim3_job& J,
                                                const orbx_sim3_state& S) {
    uint32_t r = 0;
    if (J.nlevels1 < 1 || J.nlevels1 > 16 || J.nlevels2 < 1 || J.nlevels2 > 16)
        r |= ORBX_SIM3_REFUSED_OCTAVE;
    if (J.N < 0 || J.N > g.max_n || J.mN1 < 0 || J.max_its < 1 || J.max_its > SIM3_MAX_ITS ||
        J.n_iterations < 0 || S.iterations < 0)
        r |= ORBX_SIM3_REFUSED_LIMIT;
    else if (sim3_window(J, S) > g.max_call)
        r |= ORBX_SIM3_REFUSED_LIMIT;
    if (J.kf1 < 0 || J.kf1 >= g.nposes || J.kf2 < 0 || J.kf2 >= g.nposes || J.corr_off < 0 ||
        (long long)J.corr_off + J.N > g.ncorr || J.inlier_off < 0 ||
        (long long)J.inlier_off + J.mN1 > g.ninliers || J.triple_off < 0 ||
        (long long)J.triple_off + J.max_its > g.ntriples)
        r |= ORBX_SIM3_REFUSED_RANGE;
    return r;
}

// Grid (ceil(max_n / 256), njobs).
__global__ __launch_bounds__(256) void k_sim3_prepare(const Sim3Launch g) {
    const int j = blockIdx.y;
    const orbx_sim3_job& J = g.jobs[j];
    if (job_refusal(g, J, g.state[j])) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= J.N) return;
    const Sim3Scratch sc = scratch_of(g.scratch, g.njobs, g.max_n, g.max_call);
    const orbx_sim3_corr c = g.corr[(size_t)J.corr_off + i];
    uint32_t bad = 0;
    if (c.octave1 < 0 || c.octave1 >= J.nlevels1 || c.octave2 < 0 || c.octave2 >= J.nlevels2)
        bad |= ORBX_SIM3_REFUSED_OCTAVE;
    if (c.i1 < 0 || c.i1 >= J.mN1) bad |= ORBX_SIM3_REFUSED_I1;
    if (bad) {
        atomicOr(&sc.info[j], bad);
        return;
    }
    const orbx_frame_pose& F1 = g.poses[J.kf1];
    const orbx_frame_pose& F2 = g.poses[J.kf2];
    Sim3Prep q;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        q.X1[r] = gemm3_row(F1.Rcw, r, c.X1w, F1.tcw);
        q.X2[r] = gemm3_row(F2.Rcw, r, c.X2w, F2.tcw);
    }
    // FromCameraToImage (:405-423)
    const float iz1 = fdiv(1.0f, q.X1[2]), iz2 = fdiv(1.0f, q.X2[2]);
    q.p1[0] = pinhole_kf(F1.fx, F1.cx, q.X1[0], iz1);
    q.p1[1] = pinhole_kf(F1.fy, F1.cy, q.X1[1], iz1);
    q.p2[0] = pinhole_kf(F2.fx, F2.cx, q.X2[0], iz2);
    q.p2[1] = pinhole_kf(F2.fy, F2.cy, q.X2[1], iz2);
    q.m1 = max_error(J.sigma2_1[c.octave1]);
    q.m2 = max_error(J.sigma2_2[c.octave2]);
    q.i1 = c.i1;
    q.pad[0] = q.pad[1] = q.pad[2] = 0;
    sc.prep[(size_t)j * g.max_n + i] = q;
}

// Grid (max_call, njobs), one wave each.
__global__ __launch_bounds__(64) void k_sim3_hypotheses(const Sim3Launch g) {
    const int j = blockIdx.y, h = blockIdx.x;
    const orbx_sim3_job& J = g.jobs[j];
    const orbx_sim3_state S = g.state[j];
    if (job_refusal(g, J, S) || J.N < J.min_inliers || h >= sim3_window(J, S)) return;
    const Sim3Scratch sc = scratch_of(g.scratch, g.njobs, g.max_n, g.max_call);
    const int N = J.N;
    const int32_t* tr = g.triples + 3 * ((size_t)J.triple_off + (size_t)(S.iterations + h));
    const int ia = tr[0], ib = tr[1], ic = tr[2];
    if (ia < 0 || ia >= N || ib < 0 || ib >= N || ic < 0 || ic >= N || ia == ib || ia == ic ||
        ib == ic) {
        if (threadIdx.x == 0) atomicOr(&sc.info[j], ORBX_SIM3_REFUSED_TRIPLE);
        return;
    }
    const Sim3Prep* prep = sc.prep + (size_t)j * g.max_n;
    float P1[3][3], P2[3][3];
    {
        const Sim3Prep &a = prep[ia], &b = prep[ib], &c = prep[ic];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            P1[r][0] = a.X1[r], P1[r][1] = b.X1[r], P1[r][2] = c.X1[r];
            P2[r][0] = a.X2[r], P2[r][1] = b.X2[r], P2[r][2] = c.X2[r];
        }
    }
    Sim3Hyp H;
    compute_sim3(P1, P2, J.fix_scale != 0, H);
    const orbx_frame_pose& K1 = g.poses[J.kf1];
    const orbx_frame_pose& K2 = g.poses[J.kf2];
    int count = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + (int)threadIdx.x;
        bool in = false;
        if (i < N) in = is_inlier(prep[i], H, K1, K2);
        count += (int)__popcll(__ballot(in));
    }
    H.count = count;
    if (threadIdx.x == 0) sc.hyp[(size_t)j * g.max_call + h] = H;
}

// Grid (njobs), one wave each.
__global__ __launch_bounds__(64) void k_sim3_select(const Sim3Launch g) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const orbx_sim3_job& J = g.jobs[j];
    const orbx_sim3_state S = g.state[j];
    const Sim3Scratch sc = scratch_of(g.scratch, g.njobs, g.max_n, g.max_call);
    orbx_sim3_result& res = g.res[j];
    const uint32_t refused = job_refusal(g, J, S) | sc.info[j];
    if (refused) {
        if (lane == 0) {
            res.found = 0;
            res.info = refused;
        }
        return;
    }
    uint8_t* inl = g.inliers + J.inlier_off;
    for (int i = lane; i < J.mN1; i += 64) inl[i] = 0;   // :143
    if (J.N < J.min_inliers) {                           // :146-150
        if (lane == 0) {
            res.found = 0, res.iteration = 0, res.n_inliers = 0, res.no_more = 1;
            res.info = 0, res.best_updated = 0;
        }
        return;
    }
    const int n = sim3_window(J, S);
    const Sim3Hyp* hyp = sc.hyp + (size_t)j * g.max_call;
    int best = S.best_inliers, found_h = -1, weak_h = -1;
    for (int base = 0; base < n && found_h < 0; base += 64) {
        const int h = base + lane;
        const bool valid = h < n;
        const int cnt = valid ? hyp[h].count : INT_MIN;
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d && o > incl) incl = o;
        }
        int excl = __shfl_up(incl, 1, 64);
        excl = (lane == 0 || excl < best) ? best : excl;
        const bool weak = valid && cnt >= excl;              // :183
        const bool fnd = weak && cnt > J.min_inliers;        // :192
        const unsigned long long fb = __ballot(fnd);
        unsigned long long wb = __ballot(weak);
        if (fb) {
            const int f = __ffsll((long long)fb) - 1;
            found_h = base + f;
            if (f < 63) wb &= (2ull << f) - 1;
        }
        if (wb) {
            const int w = 63 - __clzll((long long)wb);
            weak_h = base + w;
            best = __shfl(cnt, w, 64);
        }
    }
    const int its = found_h >= 0 ? S.iterations + found_h + 1 : S.iterations + n;
    if (lane == 0) {
        res.found = found_h >= 0;
        res.iteration = found_h >= 0 ? its : 0;
        res.n_inliers = found_h >= 0 ? best : 0;
        res.no_more = found_h < 0 && its >= J.max_its;       // :203-204
        res.info = 0;
        res.best_updated = weak_h >= 0;
        if (weak_h >= 0) {
            const Sim3Hyp& H = hyp[weak_h];
            res.best_inliers = best;
#pragma unroll
            for (int k = 0; k < 9; ++k) res.R12[k] = H.R[k];
#pragma unroll
            for (int r = 0; r < 3; ++r) res.t12[r] = H.t[r];
            rt_to_4x4(H.sR, H.t, res.T12);
            res.s12 = H.s;
        }
        g.state[j].iterations = its;
        g.state[j].best_inliers = best;
    }
    if (found_h < 0) return;
    // the zeroes above are in memory before the ones below, whichever lanes wrote them
    __threadfence_block();
    __syncthreads();
    const Sim3Hyp H = hyp[found_h];
    const orbx_frame_pose& K1 = g.poses[J.kf1];
    const orbx_frame_pose& K2 = g.poses[J.kf2];
    const Sim3Prep* prep = sc.prep + (size_t)j * g.max_n;
    for (int i = lane; i < J.N; i += 64)
        if (is_inlier(prep[i], H, K1, K2)) inl[prep[i].i1] = 1;   // :195-197
}

size_t sim3_scratch_bytes(int njobs, int max_n, int max_call) {
    return scratch_of(nullptr, njobs, max_n, max_call).end;
}

hipError_t launch_sim3(const Sim3Launch& a, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.scratch, 0, 4 * (size_t)a.njobs, st);
    if (e != hipSuccess) return e;
    if (a.max_n > 0)
        hipLaunchKernelGGL(k_sim3_prepare, dim3((a.max_n + 255) / 256, a.njobs), dim3(256), 0, st, a);
    if (a.max_call > 0)
        hipLaunchKernelGGL(k_sim3_hypotheses, dim3(a.max_call, a.njobs), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_sim3_select, dim3(a.njobs), dim3(64), 0, st, a);
    return hipGetLastError();
}

// What a launch may ask for, for the host-array and the batch entry alike.  its: the most
// iterations of a job (its max_its) or of the call.
bool sim3_within_limits(int njobs, int max_n, int its) {
    return njobs <= SIM3_MAX_JOBS && max_n <= SIM3_MAX_N && its <= SIM3_MAX_ITS &&
           sim3_scratch_bytes(njobs, max_n, its) <= SIM3_MAX_SCRATCH;
}

}  // namespace

extern "C" {

int32_t orbx_sim3_ransac_iterations(double prob, int32_t min_inliers, int32_t max_its, int32_t N) {
    const float epsilon = (float)min_inliers / N;
    return ransac_iterations(prob, epsilon, min_inliers == N, max_its);
}

orbx_status orbx_sim3_sample_triples(int32_t N, int32_t n_its, const int32_t* rand_values,
                                     int32_t* triples) {
    return sample_minimal_sets<3>(N, n_its, rand_values, triples);
}

orbx_status orbx_sim3_limits(int32_t* max_n, int32_t* max_its, int32_t* max_jobs,
                             int64_t* max_scratch_bytes) {
    if (max_n) *max_n = SIM3_MAX_N;
    if (max_its) *max_its = SIM3_MAX_ITS;
    if (max_jobs) *max_jobs = SIM3_MAX_JOBS;
    if (max_scratch_bytes) *max_scratch_bytes = (int64_t)SIM3_MAX_SCRATCH;
    return ORBX_OK;
}

orbx_status orbx_sim3_iterate(const orbx_frame_pose* pose1, const orbx_frame_pose* pose2,
                              const orbx_sim3_job* job, const orbx_sim3_corr* corr,
                              const int32_t* triples, orbx_sim3_state* state,
                              orbx_sim3_result* res, uint8_t* inliers, int device) {
    if (!pose1 || !pose2 || !job || !triples || !state || !res) return ORBX_ERR_INVALID;
    if (job->N < 0 || job->mN1 < 0 || job->n_iterations < 0 || job->max_its < 1 ||
        (job->N > 0 && !corr) || (job->mN1 > 0 && !inliers))
        return ORBX_ERR_INVALID;
    if (!sim3_within_limits(1, job->N, job->max_its)) return ORBX_ERR_UNSUPPORTED;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const int N = job->N, mN1 = job->mN1, max_its = job->max_its;
    // a fresh solver's window: no later call of the same solver runs more
    const int max_call = ransac_window_and(max_its, 0, job->n_iterations);
    const orbx_frame_pose poses[2] = {*pose1, *pose2};
    orbx_sim3_job hj = *job;
    hj.kf1 = 0, hj.kf2 = 1, hj.corr_off = 0, hj.inlier_off = 0, hj.triple_off = 0;
    // res / inliers go up too: what the kernels leave untouched comes back as the caller passed it
    const size_t p_pose = p.in(poses, sizeof(poses)), p_job = p.in(&hj, sizeof(hj)),
                 p_corr = p.in(corr, sizeof(orbx_sim3_corr) * (size_t)N),
                 p_tri = p.in(triples, 12 * (size_t)max_its),
                 p_state = p.inout(state, sizeof(*state)), p_res = p.inout(res, sizeof(*res)),
                 p_inl = p.inout(inliers, (size_t)mN1),
                 p_scratch = p.scratch(sim3_scratch_bytes(1, N, max_call));
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    Sim3Launch L{};
    L.jobs = c.dev<orbx_sim3_job>(p_job);
    L.njobs = 1, L.max_n = N, L.max_call = max_call;
    L.poses = c.dev<orbx_frame_pose>(p_pose);
    L.nposes = 2;
    L.corr = c.dev<orbx_sim3_corr>(p_corr);
    L.ncorr = N;
    L.triples = c.dev<int32_t>(p_tri);
    L.ntriples = max_its;
    L.state = c.dev<orbx_sim3_state>(p_state);
    L.res = c.dev<orbx_sim3_result>(p_res);
    L.inliers = c.dev<uint8_t>(p_inl);
    L.ninliers = mN1;
    L.scratch = c.dev<uint8_t>(p_scratch);
    return c.finish(HIPOK(launch_sim3(L, c.st())) ? ORBX_OK : ORBX_ERR_DEVICE);
}

orbx_status orbx_sim3_iterate_batch_device(
    orbx_matcher* m, const orbx_sim3_job* d_jobs, int32_t njobs, int32_t max_n,
    int32_t max_call_its, const orbx_frame_pose* d_poses, int32_t nposes,
    const orbx_sim3_corr* d_corr, int64_t ncorr, const int32_t* d_triples, int64_t ntriples,
    orbx_sim3_state* d_state, orbx_sim3_result* d_results, uint8_t* d_inliers,
    int64_t ninlier_bytes, void* stream) {
    if (!m || njobs < 0 || max_n < 0 || max_call_its < 0 || nposes < 0 || ncorr < 0 ||
        ntriples < 0 || ninlier_bytes < 0)
        return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_jobs || !d_poses || !d_triples || !d_state || !d_results || (ncorr > 0 && !d_corr) ||
        (ninlier_bytes > 0 && !d_inliers))
        return ORBX_ERR_INVALID;
    if (!sim3_within_limits(njobs, max_n, max_call_its)) return ORBX_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    if (!m->d_sim3.ensure(sim3_scratch_bytes(njobs, max_n, max_call_its))) return ORBX_ERR_DEVICE;
    Sim3Launch L{};
    L.jobs = d_jobs;
    L.njobs = njobs, L.max_n = max_n, L.max_call = max_call_its;
    L.poses = d_poses;
    L.nposes = nposes;
    L.corr = d_corr;
    L.ncorr = ncorr;
    L.triples = d_triples;
    L.ntriples = ntriples;
    L.state = d_state;
    L.res = d_results;
    L.inliers = d_inliers;
    L.ninliers = ninlier_bytes;
    L.scratch = m->d_sim3.p;
    return HIPOK(launch_sim3(L, (hipStream_t)stream)) ? ORBX_OK : ORBX_ERR_DEVICE;
}

}  // extern "C"
