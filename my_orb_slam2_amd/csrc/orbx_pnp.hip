// orbx_pnp.hip — PnPsolver::iterate (src/PnPsolver.cc:165-258) on the device: EPnP (compute_pose,
// :477-525) on four sampled correspondences inside the reference's RANSAC loop, CheckInliers
// (:308-339) over every correspondence, Refine (:260-305) over the best inlier set
// (include/orbx_match.h, orbx_pnp_*), and the two small kernels that tie the solver to the
// searches around it (include/orbx_frame.h).
//
//   k_pnp_hypotheses      one wave per iteration of the call: the pose of the minimal set, then the
//                         lanes stride over the correspondences and leave the count and a bit mask
//   k_pnp_select          one wave per job: the iterations walked in order against the carried
//                         best, Refine where the reference runs it, the result, the inlier bytes,
//                         the state and the best bytes
//   k_pnp_correspondences one workgroup per job: the ordered compaction of a SearchByBoW row
//   k_pnp_apply           one workgroup per job: Tracking.cc:1546-1562
//
// How a wave runs EPnP.  Every scalar of the algorithm (rotation angles, thresholds, betas, R, t)
// is computed by all 64 lanes alike, so control flow stays uniform and barriers are legal
// everywhere.  Matrices live in LDS; in the Jacobi sweeps lane k owns column k of At and of Vt.
// Every floating-point sum of the reference is evaluated in the reference's order: either one
// lane owns the whole sum (the centroid, PW0tPW0, the 78 upper entries of MtM, pc0, pw0, ABt), or
// the lanes compute the terms and every lane adds them in index order from lane reads (`ssum`,
// the row products of the Jacobi sweeps, sum2 of reprojection_error).  Nothing is tree-reduced.
//
// What is RANSAC and not EPnP (the sampling, the iteration count, the window of a call, the cursor
// scratch_of() is written with) is orbx_ransac.h's, shared with orbx_sim3.hip.  Every entry point
// is here: orbx_pnp_iterate, and the three *_batch_device forms on a handle (orbx_matcher.h).
//
// The library is built with -ffp-contract=off: every operation below is rounded on its own as on
// x86-64.  The forms evaluated inside OpenCV 3.2 (cvMulTransposed, cvSVD / cvInvert / cvSolve over
// JacobiSVDImpl_<double> and SVBkSb, Mat::convertTo) are restated and PARITY UNPINNED.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/orbx_frame.h"
#include "../../include/orbx_match.h"
#include "orbx_cv.h"
#include "orbx_host.h"
#include "orbx_hypot.h"
#include "orbx_match_kernels.h"
#include "orbx_matcher.h"
#include "orbx_ransac.h"

using namespace orbx;

namespace {

constexpr double DBL_EPS = 2.220446049250313e-16;
constexpr double DBL_MINV = 2.2250738585072014e-308;
constexpr int SVD_SWEEPS = 30;        // max(m, 30) with m <= 12 (lapack.cpp, JacobiSVDImpl_)
constexpr int SVD_COMPLETION_TRIES = 100;

// What k_pnp_hypotheses leaves per iteration (104 bytes).
struct PnpHyp {
    double R[9], t[3];   // mRi, mti
    int32_t count;       // mnInliersi
    uint32_t flags;      // ORBX_PNP_QR_SINGULAR | ORBX_PNP_SVD_COMPLETED of this compute_pose
};

// One wave's LDS.
struct PnpLds {
    double At12[144];            // MtM^T going in, the rows of U^T coming out
    double W12[12];
    double sAt[30], sVt[25], sW[5];   // the 3x3 and the thin 6xn decompositions
    double L[60];                // l_6x10
    double ccs[12], m6[6];       // ccs; pc0 | pw0
    double q_alphas[16], q_pcs[12];   // alphas / pcs of a minimal set
    int32_t q_idx[4];
    uint32_t bad;
};

// The sum of lanes 0 .. M-1 of v in lane order from +0.0, in every lane.
template <int M> __device__ __forceinline__ double ssum(double v) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < M; ++k) s = s + __shfl(v, k, 64);
    return s;
}

// cv::RNG(0x12345678)
struct CvRng {
    uint64_t state;
    __device__ __forceinline__ uint32_t next() {
        state = (uint64_t)(uint32_t)state * 4164903690u + (uint32_t)(state >> 32);
        return (uint32_t)state;
    }
};

// JacobiSVDImpl_<double>(At, W, Vt, m = M, n = N <= M, n1 = N, DBL_MIN, 10 * DBL_EPSILON) on the N rows
// of M doubles in At (LDS; the transpose of the matrix cvSVD is given): one-sided Jacobi on the
// rows, the pair moments summed in index order, at most 30 sweeps; W[i] = sqrt(row norm^2); a
// selection sort, descending, that carries the rows of At and Vt; each row times 1 / W[i]; a row
// with W[i] <= DBL_MIN completed from cv::RNG.  At holds the rows of U^T afterwards.  VT = false:
// Vt is not formed (it feeds back into nothing).  Called by the whole wave with At in place; ends
// with a barrier.
template <int M, bool VT>
__device__ __forceinline__ void jacobi_svd(double* At, double* Vt, double* W, const int N, int lane,
                                           uint32_t& flags) {
    const bool ka = lane < M, kv = lane < N;
    const double eps = DBL_EPS * 10;
    for (int i = 0; i < N; ++i) {
        const double t = ka ? At[i * M + lane] : 0.0;
        W[i] = ssum<M>(t * t);
        if (VT && kv) Vt[i * N + lane] = i == lane ? 1.0 : 0.0;
    }
    for (int iter = 0; iter < SVD_SWEEPS; ++iter) {
        bool changed = false;
        for (int i = 0; i < N - 1; ++i)
            for (int j = i + 1; j < N; ++j) {
                const double ai = ka ? At[i * M + lane] : 0.0, aj = ka ? At[j * M + lane] : 0.0;
                double a = W[i], b = W[j];
                double p = ssum<M>(ai * aj);
                if (fabs(p) <= eps * sq(a * b)) continue;
                p = p * 2.0;
                const double beta = a - b, gamma = glibc_hypot(p, beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sq(dv(delta, gamma));
                    c = dv(p, gamma * s * 2.0);
                } else {
                    c = sq(dv(gamma + beta, gamma * 2.0));
                    s = dv(p, gamma * c * 2.0);
                }
                const double t0 = c * ai + s * aj, t1 = -s * ai + c * aj;
                if (ka) At[i * M + lane] = t0, At[j * M + lane] = t1;
                a = ssum<M>(t0 * t0);
                b = ssum<M>(t1 * t1);
                W[i] = a;
                W[j] = b;
                changed = true;
                if (VT && kv) {
                    const double vi = Vt[i * N + lane], vj = Vt[j * N + lane];
                    Vt[i * N + lane] = c * vi + s * vj;
                    Vt[j * N + lane] = -s * vi + c * vj;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < N; ++i) {
        const double t = ka ? At[i * M + lane] : 0.0;
        W[i] = sq(ssum<M>(t * t));
    }
    for (int i = 0; i < N - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < N; ++k)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            const double wi = W[i], wj = W[j];
            W[i] = wj, W[j] = wi;
            if (ka) {
                const double x = At[i * M + lane];
                At[i * M + lane] = At[j * M + lane];
                At[j * M + lane] = x;
            }
            if (VT && kv) {
                const double x = Vt[i * N + lane];
                Vt[i * N + lane] = Vt[j * N + lane];
                Vt[j * N + lane] = x;
            }
        }
    }
    CvRng rng{0x12345678u};
    for (int i = 0; i < N; ++i) {
        double sd = W[i];
        double mine = ka ? At[i * M + lane] : 0.0;   // this lane's entry of row i
        for (int ii = 0; ii < SVD_COMPLETION_TRIES && sd <= DBL_MINV; ++ii) {
            flags |= ORBX_PNP_SVD_COMPLETED;
            const double val0 = dv(1.0, (double)M);
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const double val = (rng.next() & 256) != 0 ? val0 : -val0;
                if (k == lane) mine = val;
            }
            for (int round = 0; round < 2; ++round)
                for (int j = 0; j < i; ++j) {
                    const double other = ka ? At[j * M + lane] : 0.0;
                    sd = ssum<M>(mine * other);
                    mine = mine - sd * other;
                    double asum = 0.0;
#pragma unroll
                    for (int k = 0; k < M; ++k) asum = asum + fabs(__shfl(mine, k, 64));
                    asum = asum > eps * 100 ? dv(1.0, asum) : 0.0;
                    mine = mine * asum;
                }
            sd = sq(ssum<M>(mine * mine));
        }
        const double s = sd > DBL_MINV ? dv(1.0, sd) : 0.0;
        if (ka) At[i * M + lane] = mine * s;
    }
    __syncthreads();
}

__device__ __forceinline__ double dot3(const double* a, const double* b) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// cvSolve(L_6xNC, Rho, B, CV_SVD) (:681, :712, :746): the thin Jacobi SVD of the columns `cols` of
// l_6x10, then SVBkSb with one right-hand side: threshold = 2 * DBL_EPSILON * sum(w); terms with
// |w| <= threshold skipped, the others accumulated in index order as ((u_i . b) * (1 / w_i)) * v_i.
__device__ __forceinline__ void solve_6xn(PnpLds& s, const int NC, uint32_t cols, const double* rho,
                                          int lane, double* x, uint32_t& flags) {
    if (lane < NC * 6) {
        const int i = lane / 6, k = lane % 6;
        s.sAt[lane] = s.L[k * 10 + (int)((cols >> (4 * i)) & 0xf)];   // a nibble per column
    }
    __syncthreads();
    jacobi_svd<6, true>(s.sAt, s.sVt, s.sW, NC, lane, flags);
    const double rl = lane == 0 ? rho[0] : lane == 1 ? rho[1] : lane == 2 ? rho[2]
                    : lane == 3 ? rho[3] : lane == 4 ? rho[4] : rho[5];
    double thr = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        x[i] = 0.0;
        if (i < NC) thr = thr + s.sW[i];
    }
    thr = thr * (DBL_EPS * 2);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        if (i >= NC) continue;
        double wi = s.sW[i];
        const double u = lane < 6 ? s.sAt[i * 6 + lane] : 0.0;
        double sum = ssum<6>(u * rl);
        if (fabs(wi) <= thr) continue;
        wi = dv(1.0, wi);
        sum = sum * wi;
#pragma unroll
        for (int j = 0; j < 5; ++j)
            if (j < NC) x[j] = x[j] + sum * s.sVt[i * NC + j];
    }
    __syncthreads();
}

// qr_solve (:860-950) on the 6x4 system in registers; false: the singular exit, x untouched.
__device__ __forceinline__ bool qr_solve_6x4(double (*A)[4], double* b, double* x) {
    double A1[4], A2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the scan reads its pointer before it advances (:880-885): rows k, k, k + 1 .. 4
        double eta = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double elt = fabs(A[i - 1][k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) return false;
        const double inv_eta = dv(1.0, eta);
        double sum = 0.0;
#pragma unroll
        for (int i = k; i < 6; ++i) {
            A[i][k] = A[i][k] * inv_eta;
            sum = sum + A[i][k] * A[i][k];
        }
        double sigma = sq(sum);
        if (A[k][k] < 0) sigma = -sigma;
        A[k][k] = A[k][k] + sigma;
        A1[k] = sigma * A[k][k];
        A2[k] = -eta * sigma;
#pragma unroll
        for (int j = k + 1; j < 4; ++j) {
            double sj = 0.0;
#pragma unroll
            for (int i = k; i < 6; ++i) sj = sj + A[i][k] * A[i][j];
            const double tau = dv(sj, A1[k]);
#pragma unroll
            for (int i = k; i < 6; ++i) A[i][j] = A[i][j] - tau * A[i][k];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double tau = 0.0;
#pragma unroll
        for (int i = j; i < 6; ++i) tau = tau + A[i][j] * b[i];
        tau = dv(tau, A1[j]);
#pragma unroll
        for (int i = j; i < 6; ++i) b[i] = b[i] - tau * A[i][j];
    }
    x[3] = dv(b[3], A2[3]);
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        double sum = 0.0;
#pragma unroll
        for (int j = i + 1; j < 4; ++j) sum = sum + A[i][j] * x[j];
        x[i] = dv(b[i] - sum, A2[i]);
    }
    return true;
}

// gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838); l_6x10 is read from LDS.
// The reference's X is an uninitialised stack array: here it starts as zero and keeps its value
// through a singular exit (conventions).
__device__ __forceinline__ void gauss_newton(const PnpLds& s, const double* rho, double* betas, uint32_t& flags) {
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    for (int step = 0; step < 5; ++step) {
        double A[6][4], b[6];
        const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double* l = s.L + 10 * i;
            A[i][0] = 2 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3;
            A[i][1] = l[1] * b0 + 2 * l[2] * b1 + l[4] * b2 + l[7] * b3;
            A[i][2] = l[3] * b0 + l[4] * b1 + 2 * l[5] * b2 + l[8] * b3;
            A[i][3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2 * l[9] * b3;
            b[i] = rho[i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 +
                             l[4] * b1 * b2 + l[5] * b2 * b2 + l[6] * b0 * b3 + l[7] * b1 * b3 +
                             l[8] * b2 * b3 + l[9] * b3 * b3);
        }
        if (!qr_solve_6x4(A, b, x)) flags |= ORBX_PNP_QR_SINGULAR;
#pragma unroll
        for (int i = 0; i < 4; ++i) betas[i] = betas[i] + x[i];
    }
}

// The correspondences one compute_pose runs over: corr[idx[0 .. n)], widened to double as
// add_correspondence does (:363-373).
struct PnpPoints {
    const orbx_pnp_corr* corr;
    const int32_t* idx;
    int n;
    __device__ __forceinline__ double X(int i, int j) const { return (double)corr[idx[i]].X[j]; }
    __device__ __forceinline__ double u(int i) const { return (double)corr[idx[i]].u; }
    __device__ __forceinline__ double v(int i) const { return (double)corr[idx[i]].v; }
};

struct PnpCam { double fu, fv, uc, vc; };

// compute_R_and_t (:651-662): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t and
// reprojection_error for one set of betas -> the mean reprojection error, R and t in every lane.
__device__ __forceinline__ double pose_of_betas(const PnpPoints& P, const PnpCam& K, const double* alphas,
                                double* pcs, PnpLds& s, int lane, const double* betas, double* R,
                                double* t, uint32_t& flags) {
    const int n = P.n;
    const double fn = (double)n;
    if (lane < 12) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = acc + betas[i] * s.At12[(11 - i) * 12 + lane];
        s.ccs[lane] = acc;   // ccs[j][k] at 3 * j + k
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const double* a = alphas + 4 * (size_t)i;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            pcs[3 * (size_t)i + j] =
                a[0] * s.ccs[j] + a[1] * s.ccs[3 + j] + a[2] * s.ccs[6 + j] + a[3] * s.ccs[9 + j];
    }
    __syncthreads();
    if (pcs[2] < 0.0) {   // the first point's z (:638); ccs is not read again
        __syncthreads();
        for (int i = lane; i < 3 * n; i += 64) pcs[i] = -pcs[i];
    }
    __syncthreads();
    if (lane < 6) {
        double acc = 0.0;
        if (lane < 3)
            for (int i = 0; i < n; ++i) acc = acc + pcs[3 * (size_t)i + lane];
        else
            for (int i = 0; i < n; ++i) acc = acc + P.X(i, lane - 3);
        s.m6[lane] = dv(acc, fn);
    }
    __syncthreads();
    const double pc0[3] = {s.m6[0], s.m6[1], s.m6[2]}, pw0[3] = {s.m6[3], s.m6[4], s.m6[5]};
    if (lane < 9) {
        const int j = lane / 3, c = lane % 3;
        const double pcj = j == 0 ? pc0[0] : j == 1 ? pc0[1] : pc0[2];
        const double pwc = c == 0 ? pw0[0] : c == 1 ? pw0[1] : pw0[2];
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc = acc + (pcs[3 * (size_t)i + j] - pcj) * (P.X(i, c) - pwc);
        s.sAt[c * 3 + j] = acc;   // At = ABt^T
    }
    __syncthreads();
    jacobi_svd<3, true>(s.sAt, s.sVt, s.sW, 3, lane, flags);
    // R[i][j] = dot(abt_u + 3 * i, abt_v + 3 * j) with abt_u[3 * i + k] = At[k][i], abt_v[3 * j + k]
    // = Vt[k][j]
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = s.sAt[i] * s.sVt[j] + s.sAt[3 + i] * s.sVt[3 + j] + s.sAt[6 + i] * s.sVt[6 + j];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] -
                       R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) R[6] = -R[6], R[7] = -R[7], R[8] = -R[8];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = pc0[i] - dot3(R + 3 * i, pw0);
    // reprojection_error (:550-567): the lanes compute the terms, every lane adds them in order
    double sum2 = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        double term = 0.0;
        if (i < n) {
            const double pw[3] = {P.X(i, 0), P.X(i, 1), P.X(i, 2)};
            const double Xc = dot3(R, pw) + t[0], Yc = dot3(R + 3, pw) + t[1];
            const double inv_Zc = dv(1.0, dot3(R + 6, pw) + t[2]);
            const double ue = K.uc + K.fu * Xc * inv_Zc, ve = K.vc + K.fv * Yc * inv_Zc;
            const double u = P.u(i), v = P.v(i);
            term = sq((u - ue) * (u - ue) + (v - ve) * (v - ve));
        }
        const int m = n - base < 64 ? n - base : 64;
        for (int k = 0; k < m; ++k) sum2 = sum2 + __shfl(term, k, 64);
    }
    __syncthreads();
    return dv(sum2, fn);
}

// Column i of M's row pair for one correspondence (fill_M, :436-451): comp = i % 3 of control
// point i / 3; par = 0 the u row, 1 the v row.  The zero entries take part in the products.
__device__ __forceinline__ double m_entry(double a, int comp, int par, const PnpCam& K, double ud,
                                          double vd) {
    if (comp == 0) return par == 0 ? a * K.fu : 0.0;
    if (comp == 1) return par == 1 ? a * K.fv : 0.0;
    return a * (par == 0 ? ud : vd);
}

// compute_pose (:477-525) over P by the whole wave: R (row-major) and t in every lane.  alphas
// (4 * n doubles) and pcs (3 * n doubles) are the caller's work arrays, in LDS or global memory.
__device__ __forceinline__ void epnp_pose(const PnpPoints& P, const PnpCam& K, double* alphas, double* pcs,
                          PnpLds& s, int lane, double* R, double* t, uint32_t& flags) {
    const int n = P.n;
    const double fn = (double)n;
    __syncthreads();
    // choose_control_points (:375-409)
    if (lane < 3) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc = acc + P.X(i, lane);
        s.m6[lane] = dv(acc, fn);
    }
    __syncthreads();
    double cw[12];   // cws, row-major
    cw[0] = s.m6[0], cw[1] = s.m6[1], cw[2] = s.m6[2];
    __syncthreads();
    if (lane < 6) {
        // cvMulTransposed(PW0, PW0tPW0, 1): the upper entries (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        const int a = lane < 3 ? 0 : lane < 5 ? 1 : 2, b = lane < 3 ? lane : lane < 5 ? lane - 2 : 2;
        const double ca = a == 0 ? cw[0] : a == 1 ? cw[1] : cw[2];
        const double cb = b == 0 ? cw[0] : b == 1 ? cw[1] : cw[2];
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc = acc + (P.X(k, a) - ca) * (P.X(k, b) - cb);
        s.sAt[a * 3 + b] = acc;
        s.sAt[b * 3 + a] = acc;
    }
    __syncthreads();
    jacobi_svd<3, false>(s.sAt, s.sVt, s.sW, 3, lane, flags);   // dc = sW, uct = sAt
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const double k = sq(dv(s.sW[i - 1], fn));
#pragma unroll
        for (int j = 0; j < 3; ++j) cw[3 * i + j] = cw[j] + k * s.sAt[3 * (i - 1) + j];
    }
    // compute_rho (:802-810)
    double rho[6];
    {
        auto dist2 = [&](int a, int b) {
            const double* p1 = cw + 3 * a;
            const double* p2 = cw + 3 * b;
            return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) +
                   (p1[2] - p2[2]) * (p1[2] - p2[2]);
        };
        rho[0] = dist2(0, 1), rho[1] = dist2(0, 2), rho[2] = dist2(0, 3);
        rho[3] = dist2(1, 2), rho[4] = dist2(1, 3), rho[5] = dist2(2, 3);
    }
    __syncthreads();
    // compute_barycentric_coordinates (:411-434): cvInvert(CC, CC_inv, CV_SVD) is SVD::compute,
    // then SVBkSb with no right-hand side: X(r, j) += Vt(i, r) * (U(j, i) * (1 / w_i))
    if (lane < 9) {
        const int i = lane / 3, k = lane % 3;   // At[i][k] = cc[3 * k + i] = cws[i + 1][k] - cws[0][k]
        double hi = 0.0, lo = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e)
            if (e == lane) hi = cw[3 + e], lo = cw[e % 3];
        s.sAt[i * 3 + k] = hi - lo;
    }
    __syncthreads();
    jacobi_svd<3, true>(s.sAt, s.sVt, s.sW, 3, lane, flags);
    double ci[9];
    {
#pragma unroll
        for (int e = 0; e < 9; ++e) ci[e] = 0.0;
        const double thr = ((s.sW[0] + s.sW[1]) + s.sW[2]) * (DBL_EPS * 2);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double wi = s.sW[i];
            if (fabs(wi) <= thr) continue;
            wi = dv(1.0, wi);
            double buf[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) buf[j] = s.sAt[i * 3 + j] * wi;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double v = s.sVt[i * 3 + r];
#pragma unroll
                for (int j = 0; j < 3; ++j) ci[3 * r + j] = ci[3 * r + j] + v * buf[j];
            }
        }
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        const double d0 = P.X(i, 0) - cw[0], d1 = P.X(i, 1) - cw[1], d2 = P.X(i, 2) - cw[2];
        double a[4];
#pragma unroll
        for (int j = 0; j < 3; ++j) a[1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
        a[0] = 1.0 - a[1] - a[2] - a[3];
#pragma unroll
        for (int j = 0; j < 4; ++j) alphas[4 * (size_t)i + j] = a[j];
    }
    __syncthreads();
    // fill_M and cvMulTransposed(M, MtM, 1) (:484-492): entry (ci, cj), cj >= ci, is the sum over
    // the 2n rows in order; M is evaluated on the fly.  At12 = MtM^T (MtM is symmetric).
    for (int e = lane; e < 78; e += 64) {
        int ri = 0, rem = e;
        while (rem >= 12 - ri) rem -= 12 - ri, ++ri;
        const int rj = ri + rem;
        const int pi = ri / 3, compi = ri % 3, pj = rj / 3, compj = rj % 3;
        double acc = 0.0;
        for (int c = 0; c < n; ++c) {
            const double ai = alphas[4 * (size_t)c + pi], aj = alphas[4 * (size_t)c + pj];
            const double ud = K.uc - P.u(c), vd = K.vc - P.v(c);
            acc = acc + m_entry(ai, compi, 0, K, ud, vd) * m_entry(aj, compj, 0, K, ud, vd);
            acc = acc + m_entry(ai, compi, 1, K, ud, vd) * m_entry(aj, compj, 1, K, ud, vd);
        }
        s.At12[ri * 12 + rj] = acc;
        s.At12[rj * 12 + ri] = acc;
    }
    __syncthreads();
    jacobi_svd<12, false>(s.At12, nullptr, s.W12, 12, lane, flags);   // ut = At12
    // compute_L_6x10 (:760-800): row p is the control-point pair (pa, pb), column c the pair of
    // null vectors (ia, ib), doubled when they differ
    if (lane < 60) {
        const int p = lane / 10, c = lane % 10;
        const int pa = (int)((0x211000u >> (4 * p)) & 0xf), pb = (int)((0x332321u >> (4 * p)) & 0xf);
        const int ia = (int)((0x3210210100ull >> (4 * c)) & 0xf);
        const int ib = (int)((0x3333222110ull >> (4 * c)) & 0xf);
        const double* va = s.At12 + 12 * (11 - ia);
        const double* vb = s.At12 + 12 * (11 - ib);
        double da[3], db[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            da[k] = va[3 * pa + k] - va[3 * pb + k];
            db[k] = vb[3 * pa + k] - vb[3 * pb + k];
        }
        const double d = dot3(da, db);
        s.L[lane] = ia == ib ? d : 2.0 * d;
    }
    __syncthreads();

    // find_betas_approx_1 / _2 / _3 (:667-758), gauss_newton and compute_R_and_t for each, and
    // the rep_errors choice, which starts at N = 1 (:518-520)
    double best_err = 0.0;
    for (int kind = 1; kind <= 3; ++kind) {
        double b[5], betas[4], Rk[9], tk[3];
        solve_6xn(s, kind == 1 ? 4 : kind == 2 ? 3 : 5, kind == 1 ? 0x6310u : 0x43210u, rho, lane, b,
                  flags);
        if (kind == 1) {
            if (b[0] < 0) {
                betas[0] = sq(-b[0]);
                betas[1] = dv(-b[1], betas[0]);
                betas[2] = dv(-b[2], betas[0]);
                betas[3] = dv(-b[3], betas[0]);
            } else {
                betas[0] = sq(b[0]);
                betas[1] = dv(b[1], betas[0]);
                betas[2] = dv(b[2], betas[0]);
                betas[3] = dv(b[3], betas[0]);
            }
        } else {
            if (b[0] < 0) {
                betas[0] = sq(-b[0]);
                betas[1] = (b[2] < 0) ? sq(-b[2]) : 0.0;
            } else {
                betas[0] = sq(b[0]);
                betas[1] = (b[2] > 0) ? sq(b[2]) : 0.0;
            }
            if (b[1] < 0) betas[0] = -betas[0];
            betas[2] = kind == 3 ? dv(b[3], betas[0]) : 0.0;
            betas[3] = 0.0;
        }
        gauss_newton(s, rho, betas, flags);
        const double err = pose_of_betas(P, K, alphas, pcs, s, lane, betas, Rk, tk, flags);
        if (kind == 1 || err < best_err) {
            best_err = err;
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = Rk[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = tk[k];
        }
    }
}

// CheckInliers' body (:314-337) for one correspondence, in its types
__device__ __forceinline__ bool is_inlier(const orbx_pnp_corr& c, const double* R, const double* t,
                                          const PnpCam& K, float max_error) {
    const double x = (double)c.X[0], y = (double)c.X[1], z = (double)c.X[2];
    const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + t[0]);
    const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + t[1]);
    const float invZc = (float)dv(1.0, R[6] * x + R[7] * y + R[8] * z + t[2]);
    const double ue = K.uc + K.fu * (double)Xc * (double)invZc;
    const double ve = K.vc + K.fv * (double)Yc * (double)invZc;
    const float distX = (float)((double)c.u - ue);
    const float distY = (float)((double)c.v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_error;
}

// mvMaxError[i] (:154-156); an octave outside the table (the job is refused) reads nothing
__device__ __forceinline__ float max_error_of(const orbx_pnp_job& J, int octave) {
    if (octave < 0 || octave >= J.nlevels || octave >= 16) return 0.0f;
    return J.sigma2[octave] * J.th2;
}

struct PnpScratch {
    uint32_t* info;      // per job: what k_pnp_hypotheses refused; first: launch_pnp zeroes it
    PnpHyp* hyp;         // [njobs][max_call]
    uint64_t* mask;      // [njobs][max_call][words]
    int32_t* idx;        // [njobs][max_n]: Refine's vIndices
    double* work;        // [njobs][7 * max_n]: Refine's alphas, then its pcs
    int words;
    size_t end;          // the bytes of the whole
};
__host__ __device__ inline PnpScratch scratch_of(void* base, int njobs, int max_n, int max_call) {
    ScratchCursor c{(uint8_t*)base};
    PnpScratch s;
    s.words = (max_n + 63) / 64;
    s.info = c.take<uint32_t>(njobs);
    s.hyp = c.take<PnpHyp>(njobs, max_call);
    s.mask = c.take<uint64_t>(njobs, max_call, s.words);
    s.idx = c.take<int32_t>(njobs, max_n);
    s.work = c.take<double>(7, njobs, max_n);
    s.end = c.end;
    return s;
}

// The iterations of this call: [S.iterations, S.iterations + pnp_window(J, S))
__device__ __forceinline__ long long pnp_window(const orbx_pnp_job& J, const orbx_pnp_state& S) {
    return ransac_window_or(J.max_its, S.iterations, J.n_iterations);
}

// What the job record and the state show; the same in both kernels.
__device__ __forceinline__ uint32_t job_refusal(const PnpLaunch& g, const orbx_pnp_job& J,
                                                const orbx_pnp_state& S) {
    uint32_t r = 0;
    if (J.nlevels < 1 || J.nlevels > 16) r |= ORBX_PNP_REFUSED_OCTAVE;
    if (J.N < 0 || J.N > g.max_n || J.n_matches < 0 || J.max_its < 1 || J.max_its > PNP_MAX_ITS ||
        J.min_inliers < 1 || S.iterations < 0 || S.best_inliers < 0 || pnp_window(J, S) > g.max_call)
        return r | ORBX_PNP_REFUSED_LIMIT;
    if (J.corr_off < 0 || (long long)J.corr_off + J.N > g.ncorr || J.inlier_off < 0 ||
        (long long)J.inlier_off + J.n_matches > g.ninliers || J.best_off < 0 ||
        (long long)J.best_off + J.N > g.nbest || J.quad_off < 0 ||
        (J.N >= J.min_inliers &&
         (long long)J.quad_off + S.iterations + pnp_window(J, S) > g.nquads))
        r |= ORBX_PNP_REFUSED_RANGE;
    return r;
}

__device__ __forceinline__ PnpCam cam_of(const orbx_pnp_job& J) {
    return PnpCam{(double)J.fx, (double)J.fy, (double)J.cx, (double)J.cy};
}

// Grid (max_call, njobs), one wave each.
__global__ __launch_bounds__(64) void k_pnp_hypotheses(const PnpLaunch g) {
    __shared__ PnpLds s;
    const int j = blockIdx.y, h = blockIdx.x, lane = threadIdx.x;
    const orbx_pnp_job& J = g.jobs[j];
    const orbx_pnp_state S = g.state[j];
    if (job_refusal(g, J, S) || J.N < J.min_inliers || h >= pnp_window(J, S)) return;
    const PnpScratch sc = scratch_of(g.scratch, g.njobs, g.max_n, g.max_call);
    const int N = J.N;
    const int32_t* q = g.quads + 4 * ((size_t)J.quad_off + (size_t)S.iterations + (size_t)h);
    const int q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    if (q0 < 0 || q0 >= N || q1 < 0 || q1 >= N || q2 < 0 || q2 >= N || q3 < 0 || q3 >= N ||
        q0 == q1 || q0 == q2 || q0 == q3 || q1 == q2 || q1 == q3 || q2 == q3) {
        if (lane == 0) atomicOr(&sc.info[j], ORBX_PNP_REFUSED_QUAD);
        return;
    }
    if (lane == 0) s.q_idx[0] = q0, s.q_idx[1] = q1, s.q_idx[2] = q2, s.q_idx[3] = q3;
    __syncthreads();
    const orbx_pnp_corr* corr = g.corr + J.corr_off;
    const PnpPoints P{corr, s.q_idx, 4};
    const PnpCam K = cam_of(J);
    double R[9], t[3];
    uint32_t flags = 0;
    epnp_pose(P, K, s.q_alphas, s.q_pcs, s, lane, R, t, flags);
    uint64_t* mask = sc.mask + ((size_t)j * g.max_call + h) * sc.words;
    int count = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < N) {
            const orbx_pnp_corr c = corr[i];
            in = is_inlier(c, R, t, K, max_error_of(J, c.octave));
        }
        const unsigned long long b = __ballot(in);
        count += (int)__popcll(b);
        if (lane == 0) mask[base >> 6] = b;
    }
    if (lane == 0) {
        PnpHyp& H = sc.hyp[(size_t)j * g.max_call + h];
#pragma unroll
        for (int k = 0; k < 9; ++k) H.R[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) H.t[k] = t[k];
        H.count = count;
        H.flags = flags;
    }
}

// Grid (njobs), one wave each.
__global__ __launch_bounds__(64) void k_pnp_select(const PnpLaunch g) {
    __shared__ PnpLds s;
    const int j = blockIdx.x, lane = threadIdx.x;
    const orbx_pnp_job& J = g.jobs[j];
    const orbx_pnp_state S = g.state[j];
    const PnpScratch sc = scratch_of(g.scratch, g.njobs, g.max_n, g.max_call);
    orbx_pnp_result& res = g.res[j];
    uint32_t refused = job_refusal(g, J, S) | sc.info[j];
    if (lane == 0) s.bad = 0;
    __syncthreads();
    const int N = J.N;
    if (!(refused & (ORBX_PNP_REFUSED_LIMIT | ORBX_PNP_REFUSED_RANGE))) {
        // what only the arrays show: the octaves, the slots, the carried best set
        const orbx_pnp_corr* corr = g.corr + J.corr_off;
        const uint8_t* best = g.best + J.best_off;
        uint32_t bad = 0;
        int nbest = 0;
        for (int base = 0; base < N; base += 64) {
            const int i = base + lane;
            bool set = false;
            if (i < N) {
                const orbx_pnp_corr c = corr[i];
                if (c.octave < 0 || c.octave >= J.nlevels) bad |= ORBX_PNP_REFUSED_OCTAVE;
                if (c.i < 0 || c.i >= J.n_matches || (i > 0 && corr[i - 1].i >= c.i))
                    bad |= ORBX_PNP_REFUSED_I;
                set = best[i] != 0;
            }
            nbest += (int)__popcll(__ballot(set));
        }
        if (S.best_inliers > 0 && nbest != S.best_inliers) bad |= ORBX_PNP_REFUSED_LIMIT;
        if (bad) atomicOr(&s.bad, bad);
        __syncthreads();
        refused |= s.bad;
    }
    if (refused) {
        if (lane == 0) {
            res.found = 0;
            res.info = refused;
        }
        return;
    }
    const orbx_pnp_corr* corr = g.corr + J.corr_off;
    uint8_t* best = g.best + J.best_off;
    uint8_t* inl = g.inliers + J.inlier_off;
    const PnpCam K = cam_of(J);
    const int min_in = J.min_inliers;
    int found = 0, source = 0, n_run = 0, n_inliers = 0, no_more = 0;
    int its = S.iterations, nbest = S.best_inliers, refines = 0;
    uint32_t flags = 0;
    float bestT[16], outT[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) bestT[k] = S.best_Tcw[k], outT[k] = 0.0f;
    bool best_written = false;
    double R2[9], t2[3];
    if (N < min_in) {   // :173-177
        no_more = 1;
    } else {
        const int window = (int)pnp_window(J, S);
        const PnpHyp* hyp = sc.hyp + (size_t)j * g.max_call;
        int32_t* idx = sc.idx + (size_t)j * g.max_n;
        double* alphas = sc.work + 7 * (size_t)j * g.max_n;
        double* pcs = alphas + 4 * (size_t)g.max_n;
        // the best set is the one Refine last ran on in this call, without success: the same
        // inputs give the same outcome, so it is counted and not run again
        bool refined_in_vain = false;
        for (int h = 0; h < window && !found; ++h) {
            ++its;
            n_run = h + 1;
            const int cnt = hyp[h].count;
            flags |= hyp[h].flags;
            if (cnt < min_in) continue;   // :209
            if (cnt > nbest) {            // :212-224
                const uint64_t* mask = sc.mask + ((size_t)j * g.max_call + h) * sc.words;
                for (int i = lane; i < N; i += 64) best[i] = (uint8_t)((mask[i >> 6] >> (i & 63)) & 1);
                nbest = cnt;
                rt_to_4x4(hyp[h].R, hyp[h].t, bestT);   // mRi / mti into mBestTcw (:217-223)
                best_written = true;
                refined_in_vain = false;
                __syncthreads();
            }
            ++refines;                    // Refine (:260-305)
            if (refined_in_vain) continue;
            int n = 0;
            for (int base = 0; base < N; base += 64) {
                const int i = base + lane;
                const bool set = i < N && best[i] != 0;
                const unsigned long long b = __ballot(set);
                if (set) idx[n + (int)__popcll(b & ((1ull << lane) - 1))] = i;
                n += (int)__popcll(b);
            }
            __syncthreads();
            const PnpPoints P{corr, idx, n};
            epnp_pose(P, K, alphas, pcs, s, lane, R2, t2, flags);
            int cnt2 = 0;
            for (int base = 0; base < N; base += 64) {
                const int i = base + lane;
                bool in = false;
                if (i < N) {
                    const orbx_pnp_corr c = corr[i];
                    in = is_inlier(c, R2, t2, K, max_error_of(J, c.octave));
                }
                cnt2 += (int)__popcll(__ballot(in));
            }
            if (cnt2 > min_in) {          // :292
                found = 1, source = 1, n_inliers = cnt2;
                rt_to_4x4(R2, t2, outT);   // mRefinedTcw (:294-300)
            } else {
                refined_in_vain = true;
            }
        }
        if (!found && its >= J.max_its) {   // :241-255
            no_more = 1;
            if (nbest >= min_in) {
                found = 1, source = 2, n_inliers = nbest;
#pragma unroll
                for (int k = 0; k < 16; ++k) outT[k] = bestT[k];
            }
        }
    }
    if (lane == 0) {
        res.found = found, res.source = source, res.iteration = found ? its : 0;
        res.n_run = n_run, res.n_inliers = n_inliers, res.no_more = no_more;
        res.info = (uint32_t)refines | flags;
        res.best_inliers = nbest;
#pragma unroll
        for (int k = 0; k < 16; ++k) res.Tcw[k] = outT[k];
        orbx_pnp_state& So = g.state[j];
        So.iterations = its;
        So.best_inliers = nbest;
        if (best_written) {
#pragma unroll
            for (int k = 0; k < 16; ++k) So.best_Tcw[k] = bestT[k];
        }
    }
    if (!found) return;
    // vbInliers (:229-234, :247-252): all n_matches bytes, the zeroes before the ones
    for (int i = lane; i < J.n_matches; i += 64) inl[i] = 0;
    __syncthreads();
    for (int i = lane; i < N; i += 64) {
        const orbx_pnp_corr c = corr[i];
        const bool in = source == 1 ? is_inlier(c, R2, t2, K, max_error_of(J, c.octave))
                                    : best[i] != 0;
        if (in) inl[c.i] = 1;
    }
}

// Grid (njobs), 256 threads: the ordered compaction of one SearchByBoW row.
__global__ __launch_bounds__(256) void k_pnp_correspondences(
    const int32_t* __restrict__ match, long long match_stride, const orbx_keypoint* __restrict__ kp,
    int n_feat, const orbx_map_point* __restrict__ mps, const int32_t* __restrict__ mp_off,
    orbx_pnp_corr* __restrict__ corr, long long corr_stride, int32_t* __restrict__ outN,
    int32_t* __restrict__ out_flags) {
    __shared__ int wave_count[4];
    __shared__ int base_s;
    __shared__ int dropped_s;
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* row = match + (size_t)j * match_stride;
    orbx_pnp_corr* out = corr + (size_t)j * corr_stride;
    const int lo = mp_off[j], nmp = mp_off[j + 1] - lo;
    if (tid == 0) base_s = 0, dropped_s = 0;
    __syncthreads();
    for (int start = 0; start < n_feat; start += 256) {
        const int i = start + tid;
        const int m = i < n_feat ? row[i] : -1;
        const bool keep = m >= 0 && m < nmp;
        if (m >= nmp) dropped_s = 1;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wave_count[wave] = (int)__popcll(b);
        __syncthreads();
        int pos = base_s + (int)__popcll(b & ((1ull << lane) - 1));
        for (int w = 0; w < wave; ++w) pos += wave_count[w];
        if (keep) {
            orbx_pnp_corr c;
            const orbx_map_point& mp = mps[(size_t)lo + m];
            c.i = i;
            c.X[0] = mp.pos[0], c.X[1] = mp.pos[1], c.X[2] = mp.pos[2];
            c.u = kp[i].x, c.v = kp[i].y;
            c.octave = kp[i].octave;
            out[pos] = c;
        }
        __syncthreads();
        if (tid == 0) base_s += wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
        __syncthreads();
    }
    if (tid == 0) {
        outN[j] = base_s;
        if (out_flags) out_flags[j] = dropped_s;
    }
}

// Grid (njobs), 256 threads: Tracking.cc:1546-1562.
__global__ __launch_bounds__(256) void k_pnp_apply(
    const orbx_pnp_job* __restrict__ jobs, const orbx_pnp_result* __restrict__ results,
    const uint8_t* __restrict__ inliers, long long ninliers, const int32_t* __restrict__ match,
    long long match_stride, int n_feat, const orbx_frame_pose* __restrict__ tmpl,
    orbx_frame_pose* __restrict__ poses, int32_t* __restrict__ mp_of_feat, long long feat_stride) {
    const int j = blockIdx.x, tid = threadIdx.x;
    const orbx_pnp_job& J = jobs[j];
    const orbx_pnp_result& r = results[j];
    const bool found = r.found != 0 && !(r.info & ORBX_PNP_REFUSED_ANY) && J.n_matches == n_feat &&
                       J.inlier_off >= 0 && (long long)J.inlier_off + J.n_matches <= ninliers;
    const uint8_t* inl = inliers + (found ? J.inlier_off : 0);
    for (int i = tid; i < n_feat; i += 256)
        mp_of_feat[(size_t)j * feat_stride + i] =
            found && inl[i] ? match[(size_t)j * match_stride + i] : -1;
    if (tid == 0) {
        orbx_frame_pose P = *tmpl;
        if (found) {
            // Tcw.copyTo(mCurrentFrame.mTcw) and Frame::UpdatePoseMatrices: mOw = -mRcw.t() * mtcw
            float R[9], t[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) R[3 * a + b] = r.Tcw[4 * a + b];
                t[a] = r.Tcw[4 * a + 3];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) P.Rcw[k] = R[k];
#pragma unroll
            for (int a = 0; a < 3; ++a) P.tcw[a] = t[a];
            camera_centre(R, t, P.Ow);
        }
        poses[j] = P;
    }
}

size_t pnp_scratch_bytes(int njobs, int max_n, int max_call) {
    return scratch_of(nullptr, njobs, max_n, max_call).end;
}

hipError_t launch_pnp(const PnpLaunch& a, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.scratch, 0, 4 * (size_t)a.njobs, st);
    if (e != hipSuccess) return e;
    if (a.max_call > 0)
        hipLaunchKernelGGL(k_pnp_hypotheses, dim3(a.max_call, a.njobs), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_pnp_select, dim3(a.njobs), dim3(64), 0, st, a);
    return hipGetLastError();
}

// What a launch may ask for, for the host-array and the batch entry alike.  its: the most
// iterations of a job (its max_its) or of the call.
bool pnp_within_limits(int njobs, int max_n, long long its) {
    return njobs <= PNP_MAX_JOBS && max_n <= PNP_MAX_N && its <= PNP_MAX_ITS &&
           pnp_scratch_bytes(njobs, max_n, (int)its) <= PNP_MAX_SCRATCH;
}

}  // namespace

extern "C" {

orbx_status orbx_pnp_ransac_parameters(double prob, int32_t min_inliers, int32_t max_its,
                                       int32_t min_set, float epsilon, int32_t N,
                                       int32_t* min_inliers_out, int32_t* max_its_out) {
    if (N < 0 || !min_inliers_out || !max_its_out) return ORBX_ERR_INVALID;
    if (min_set != 4) return ORBX_ERR_UNSUPPORTED;
    float mRansacEpsilon = epsilon;
    int nMinInliers = x86_trunc((double)((float)N * mRansacEpsilon));
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    const float ratio = (float)nMinInliers / (float)N;
    if (mRansacEpsilon < ratio) mRansacEpsilon = ratio;
    *min_inliers_out = nMinInliers;
    *max_its_out = ransac_iterations(prob, mRansacEpsilon, nMinInliers == N, max_its);
    return ORBX_OK;
}

orbx_status orbx_pnp_sample_quads(int32_t N, int32_t n_its, const int32_t* rand_values,
                                  int32_t* quads) {
    return sample_minimal_sets<4>(N, n_its, rand_values, quads);
}

orbx_status orbx_pnp_limits(int32_t* max_n, int32_t* max_its, int32_t* max_jobs,
                            int64_t* max_scratch_bytes) {
    if (max_n) *max_n = PNP_MAX_N;
    if (max_its) *max_its = PNP_MAX_ITS;
    if (max_jobs) *max_jobs = PNP_MAX_JOBS;
    if (max_scratch_bytes) *max_scratch_bytes = (int64_t)PNP_MAX_SCRATCH;
    return ORBX_OK;
}

orbx_status orbx_pnp_iterate(const orbx_pnp_job* job, const orbx_pnp_corr* corr,
                             const int32_t* quads, orbx_pnp_state* state, uint8_t* best,
                             orbx_pnp_result* res, uint8_t* inliers, int device) {
    if (!job || !state || !res) return ORBX_ERR_INVALID;
    if (job->N < 0 || job->n_matches < 0 || job->max_its < 1 || state->iterations < 0 ||
        (job->N > 0 && (!corr || !best)) || (job->n_matches > 0 && !inliers))
        return ORBX_ERR_INVALID;
    const long long window = ransac_window_or(job->max_its, state->iterations, job->n_iterations);
    const long long nq = (long long)state->iterations + window;
    if (nq > 0 && !quads) return ORBX_ERR_INVALID;
    if (!pnp_within_limits(1, job->N, window < job->max_its ? job->max_its : window) ||
        nq > INT_MAX / 4)
        return ORBX_ERR_UNSUPPORTED;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const int N = job->N, nm = job->n_matches, max_call = (int)window;
    orbx_pnp_job hj = *job;
    hj.corr_off = 0, hj.inlier_off = 0, hj.quad_off = 0, hj.best_off = 0;
    // res / inliers go up too: what the kernels leave untouched comes back as the caller passed it
    const size_t p_job = p.in(&hj, sizeof(hj)), p_corr = p.in(corr, sizeof(orbx_pnp_corr) * (size_t)N),
                 p_quad = p.in(quads, 16 * (size_t)nq), p_state = p.inout(state, sizeof(*state)),
                 p_best = p.inout(best, (size_t)N), p_res = p.inout(res, sizeof(*res)),
                 p_inl = p.inout(inliers, (size_t)nm),
                 p_scratch = p.scratch(pnp_scratch_bytes(1, N, max_call));
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    PnpLaunch L{};
    L.jobs = c.dev<orbx_pnp_job>(p_job);
    L.njobs = 1, L.max_n = N, L.max_call = max_call;
    L.corr = c.dev<orbx_pnp_corr>(p_corr);
    L.ncorr = N;
    L.quads = c.dev<int32_t>(p_quad);
    L.nquads = nq;
    L.state = c.dev<orbx_pnp_state>(p_state);
    L.best = c.dev<uint8_t>(p_best);
    L.nbest = N;
    L.res = c.dev<orbx_pnp_result>(p_res);
    L.inliers = c.dev<uint8_t>(p_inl);
    L.ninliers = nm;
    L.scratch = c.dev<uint8_t>(p_scratch);
    return c.finish(HIPOK(launch_pnp(L, c.st())) ? ORBX_OK : ORBX_ERR_DEVICE);
}

orbx_status orbx_pnp_iterate_batch_device(
    orbx_matcher* m, const orbx_pnp_job* d_jobs, int32_t njobs, int32_t max_n,
    int32_t max_call_its, const orbx_pnp_corr* d_corr, int64_t ncorr, const int32_t* d_quads,
    int64_t nquads, orbx_pnp_state* d_state, uint8_t* d_best, int64_t nbest_bytes,
    orbx_pnp_result* d_results, uint8_t* d_inliers, int64_t ninlier_bytes, void* stream) {
    if (!m || njobs < 0 || max_n < 0 || max_call_its < 0 || ncorr < 0 || nquads < 0 ||
        nbest_bytes < 0 || ninlier_bytes < 0)
        return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_jobs || !d_state || !d_results || (ncorr > 0 && !d_corr) || (nquads > 0 && !d_quads) ||
        (nbest_bytes > 0 && !d_best) || (ninlier_bytes > 0 && !d_inliers))
        return ORBX_ERR_INVALID;
    if (!pnp_within_limits(njobs, max_n, max_call_its)) return ORBX_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    if (!m->d_pnp.ensure(pnp_scratch_bytes(njobs, max_n, max_call_its))) return ORBX_ERR_DEVICE;
    PnpLaunch L{};
    L.jobs = d_jobs;
    L.njobs = njobs, L.max_n = max_n, L.max_call = max_call_its;
    L.corr = d_corr;
    L.ncorr = ncorr;
    L.quads = d_quads;
    L.nquads = nquads;
    L.state = d_state;
    L.best = d_best;
    L.nbest = nbest_bytes;
    L.res = d_results;
    L.inliers = d_inliers;
    L.ninliers = ninlier_bytes;
    L.scratch = m->d_pnp.p;
    return HIPOK(launch_pnp(L, (hipStream_t)stream)) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_pnp_correspondences_batch_device(
    orbx_matcher* m, int32_t njobs, const int32_t* d_match, int64_t match_stride,
    const orbx_keypoint* d_kp, int32_t n_feat, const orbx_map_point* d_mps,
    const int32_t* d_mp_off, orbx_pnp_corr* d_corr, int64_t corr_stride, int32_t* d_N,
    int32_t* d_N_flags, void* stream) {
    if (!m || njobs < 0 || n_feat < 0 || match_stride < 0 || corr_stride < 0 ||
        n_feat > match_stride || n_feat > corr_stride)
        return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_mp_off || !d_N || (n_feat > 0 && (!d_match || !d_kp || !d_mps || !d_corr)))
        return ORBX_ERR_INVALID;
    if (njobs > PNP_MAX_JOBS) return ORBX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_pnp_correspondences, dim3(njobs), dim3(256), 0, (hipStream_t)stream,
                       d_match, match_stride, d_kp, n_feat, d_mps, d_mp_off, d_corr, corr_stride,
                       d_N, d_N_flags);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_pnp_apply_batch_device(
    orbx_matcher* m, int32_t njobs, const orbx_pnp_job* d_jobs, const orbx_pnp_result* d_results,
    const uint8_t* d_inliers, int64_t ninlier_bytes, const int32_t* d_match, int64_t match_stride,
    int32_t n_feat, const orbx_frame_pose* d_template, orbx_frame_pose* d_poses,
    int32_t* d_mp_of_feat, int64_t feat_stride, void* stream) {
    if (!m || njobs < 0 || n_feat < 0 || ninlier_bytes < 0 || match_stride < 0 || feat_stride < 0 ||
        n_feat > match_stride || n_feat > feat_stride)
        return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_jobs || !d_results || !d_template || !d_poses ||
        (n_feat > 0 && (!d_match || !d_mp_of_feat)) || (ninlier_bytes > 0 && !d_inliers))
        return ORBX_ERR_INVALID;
    if (njobs > PNP_MAX_JOBS) return ORBX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_pnp_apply, dim3(njobs), dim3(256), 0, (hipStream_t)stream, d_jobs,
                       d_results, d_inliers, ninlier_bytes, d_match, match_stride, n_feat,
                       d_template, d_poses, d_mp_of_feat, feat_stride);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

}  // extern "C"
