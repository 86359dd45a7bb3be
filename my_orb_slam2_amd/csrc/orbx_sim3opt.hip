// orbx_sim3opt.hip — Optimizer::OptimizeSim3 (src/Optimizer.cc:1070-1265) on the device
// (include/orbx_match.h, orbx_sim3_optimize*): the refinement of the Sim3 between two keyframes
// that LoopClosing::ComputeSim3 runs between SearchBySim3 and SearchByProjection(KF, Scw).
//
// k_sim3_opt: one wave per job, SO_WAVES jobs per workgroup; the waves of a workgroup never meet
// (no workgroup barrier).  The g2o graph of the call is one VertexSim3Expmap with fixed points, so
// the whole of OptimizationAlgorithmLevenberg::solve is restated here as in k_pose_opt
// (orbx_poseopt.hip).  Neither edge type has an analytic Jacobian: g2o differentiates numerically
// (base_binary_edge.hpp:131-200), and the 14 perturbed estimates Sim3(+-1e-9 e_d) * estimate are
// the same for every edge of one linearisation, so lanes 0-13 compute one each, with its inverse,
// into LDS.  Every evaluation walks the correspondences in chunks of 64, one lane per pair; a
// lane evaluates its two edges at the estimate and at the perturbed estimates, the active pairs of
// a chunk put their per-edge terms (28 lower-triangle entries of H, 7 of b, the robust chi2) into
// LDS compacted in edge order (e12_i, e21_i, e12_i+1, ...; 32 pairs at a time), and 36 lanes then
// add one term each, edge by edge: the sums round exactly as g2o's loop over _activeEdges does.
// The 7x7 system, the estimate and the Levenberg state are wave-uniform: the pivoted LDLT runs on
// lane 0 over an LDS copy, the rest is computed by every lane alike.  An edge's _error is never
// stored: it is a function of the estimate it was last evaluated at, and that estimate is kept
// instead (g2o does not recompute errors after a rejected trial).
//
// The forms evaluated inside Eigen, the robust kernel and the LDLT are orbx_lm.h's, shared with
// k_pose_opt; the edge model (s3_*, the perturbed estimates, the numeric Jacobian) is here.  The
// Levenberg loop (optimize) is written out: over orbx_lm.h's lm_optimize<7> the kernel measured
// 4 % slower (profiles/lm_share_ab.txt).  sin / cos / exp are orbx_math.h's.  Built with
// -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstddef>
#include <cmath>
#include <cstdint>

#include "../../include/orbx_frame.h"
#include "../../include/orbx_match.h"
#include "orbx_host.h"
#include "orbx_lm.h"
#include "orbx_match_kernels.h"
#include "orbx_matcher.h"
#include "orbx_math.h"

using namespace orbx;

namespace {

constexpr int SO_WAVES = 2;                  // jobs per workgroup
constexpr int SO_TERMS = 36;                 // 28 of H (i >= j), 7 of b, robust chi2
constexpr int SO_HALF = 32;                  // pairs whose terms are in LDS at once (64 edges)
constexpr int SO_T = 2 * SO_HALF * SO_TERMS; // doubles: the terms
constexpr int SO_P = 14 * 16;                // the perturbed estimates and their inverses
constexpr int SO_A = 49 + 7 + 7;             // the solver's copy, temp, y
constexpr int SO_LDS_PER_WAVE = SO_T + SO_P + SO_TERMS + SO_A + 7 + 4 + 2;
// the LDS of a workgroup against the 160 KB of a gfx950 CU (three workgroups fit)
static_assert(SO_WAVES * SO_LDS_PER_WAVE * 8 <= 64 * 1024, "k_sim3_opt's LDS per workgroup");
static_assert(SIM3OPT_MAX_N <= 64 * 64, "one dropped bit per chunk in a 64-bit word per lane");

struct S3 { double qx, qy, qz, qw, tx, ty, tz, s; };
struct Cam2 { double fx, fy, cx, cy; };

// Sim3::map (sim3.h:144-146)
__device__ __forceinline__ void s3_map(const S3& S, double px, double py, double pz, double& x,
                                       double& y, double& z) {
    double rx, ry, rz;
    quat_rotate(S.qx, S.qy, S.qz, S.qw, px, py, pz, rx, ry, rz);
    x = S.s * rx + S.tx, y = S.s * ry + S.ty, z = S.s * rz + S.tz;
}

// Sim3::inverse (sim3.h:233-236)
__device__ __forceinline__ S3 s3_inverse(const S3& S) {
    S3 I;
    I.qx = -S.qx, I.qy = -S.qy, I.qz = -S.qz, I.qw = S.qw;
    const double m = dv(-1.0, S.s);
    quat_rotate(I.qx, I.qy, I.qz, I.qw, m * S.tx, m * S.ty, m * S.tz, I.tx, I.ty, I.tz);
    I.s = dv(1.0, S.s);
    return I;
}

// Sim3::operator* (sim3.h:266-272): the quaternion product is not normalised
__device__ __forceinline__ S3 s3_mul(const S3& A, const S3& B) {
    S3 N;
    quat_mul(A.qx, A.qy, A.qz, A.qw, B.qx, B.qy, B.qz, B.qw, N.qx, N.qy, N.qz, N.qw);
    double rx, ry, rz;
    quat_rotate(A.qx, A.qy, A.qz, A.qw, B.tx, B.ty, B.tz, rx, ry, rz);
    N.tx = A.s * rx + A.tx, N.ty = A.s * ry + A.ty, N.tz = A.s * rz + A.tz;
    N.s = A.s * B.s;
    return N;
}

// Sim3(const Vector7d&) (sim3.h:70-142); 0: done, otherwise the info flag of the routine that
// refused its argument (E is then not to be used)
__device__ __forceinline__ uint32_t s3_exp(const double (&u)[7], S3& E) {
    const double sigma = u[6];
    const double theta = sq((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const double O[3][3] = {{0.0, -u[2], u[1]}, {u[2], 0.0, -u[0]}, {-u[1], u[0], 0.0}};
    double s;
    if (!orbx_exp_f64(sigma, &s)) return ORBX_SIM3OPT_EXP_LIMIT;
    const double eps = 0.00001;
    const bool ssmall = fabs(sigma) < eps, tsmall = theta < eps;
    double sn = 0.0, cs = 1.0;
    if (!tsmall && !orbx_sincos_f64(theta, &sn, &cs)) return ORBX_SIM3OPT_THETA_LIMIT;
    double A, B, C;
    double ra = 1.0, rb = 1.0;      // R = I + ra * Omega + rb * Omega2
    if (!tsmall) {
        ra = dv(sn, theta);
        rb = dv(1.0 - cs, theta * theta);
    }
    if (ssmall) {
        C = 1.0;
        if (tsmall) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = dv(1.0 - cs, theta2);
            B = dv(theta - sn, theta2 * theta);
        }
    } else {
        C = dv(s - 1.0, sigma);
        if (tsmall) {
            const double sigma2 = sigma * sigma;
            A = dv((sigma - 1.0) * s + 1.0, sigma2);
            B = dv(((0.5 * sigma2 - sigma) + 1.0) * s, sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = dv(a * sigma + (1.0 - b) * theta, theta * c);
            B = dv((C - dv((b - 1.0) * sigma + a * theta, c)) * 1., theta2);
        }
    }
    double R[3][3], W[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double o2 = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];
            const double e = i == j ? 1.0 : 0.0;
            R[i][j] = tsmall ? (e + O[i][j]) + o2 : (e + ra * O[i][j]) + rb * o2;
            W[i][j] = (A * O[i][j] + B * o2) + C * e;
        }
    quat_from_matrix(R, E.qx, E.qy, E.qz, E.qw);
    E.tx = (W[0][0] * u[3] + W[0][1] * u[4]) + W[0][2] * u[5];
    E.ty = (W[1][0] * u[3] + W[1][1] * u[4]) + W[1][2] * u[5];
    E.tz = (W[2][0] * u[3] + W[2][1] * u[4]) + W[2][2] * u[5];
    E.s = s;
    return 0;
}

// computeError of either edge (types_seven_dof_expmap.h:138-145, :160-167): S maps the fixed
// point into the camera whose calibration K is; err = obs - cam_map(project(.))
__device__ __forceinline__ void edge_error(const S3& S, const double (&X)[3], const double (&obs)[2],
                                           const Cam2& K, double (&err)[2]) {
    double x, y, z;
    s3_map(S, X[0], X[1], X[2], x, y, z);
    err[0] = obs[0] - (dv(x, z) * K.fx + K.cx);
    err[1] = obs[1] - (dv(y, z) * K.fy + K.cy);
}
// chi2 (base_edge.h:60) with information = info * I
__device__ __forceinline__ double edge_chi2(const double (&err)[2], double info) {
    return err[0] * (info * err[0]) + err[1] * (info * err[1]);
}

// One correspondence's two edges as the lane holds them
struct PairIn {
    double X1[3], X2[3];      // the fixed points: P3D1c, P3D2c
    double o1[2], o2[2];      // the observations in KF1 and KF2
    double info1, info2;
};

// The job as one wave sees it
struct JobCtx {
    const orbx_sim3opt_corr* corr;
    const orbx_frame_pose* F1;
    const orbx_frame_pose* F2;
    const float* sigma2_1;
    const float* sigma2_2;
    int n, lane;
    bool fix_scale;
    Cam2 K1, K2;
    double delta;
    double* T;     // LDS: the terms
    double* P;     // LDS: 14 x (perturbed estimate, its inverse)
    double* S;     // LDS: sums[36], then the solver's block
};

// Correspondence i's pair: R1w*P3D1w + t1w and R2w*P3D2w + t2w in float as cv::Mat evaluates them
// (Optimizer.cc:1142, :1150), widened; the keypoints widened; 1.0f / sigma2[octave] widened
__device__ __forceinline__ void load_pair(const JobCtx& c, int i, PairIn& p) {
    const orbx_sim3opt_corr q = c.corr[i];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        p.X1[r] = (double)gemm3_row(c.F1->Rcw, r, q.X1w, c.F1->tcw);
        p.X2[r] = (double)gemm3_row(c.F2->Rcw, r, q.X2w, c.F2->tcw);
    }
    p.o1[0] = (double)q.kp1[0], p.o1[1] = (double)q.kp1[1];
    p.o2[0] = (double)q.kp2[0], p.o2[1] = (double)q.kp2[1];
    p.info1 = (double)__fdiv_rn(1.0f, c.sigma2_1[q.octave1]);
    p.info2 = (double)__fdiv_rn(1.0f, c.sigma2_2[q.octave2]);
}

__device__ __forceinline__ void s3_store(double* p, const S3& S) {
    p[0] = S.qx, p[1] = S.qy, p[2] = S.qz, p[3] = S.qw, p[4] = S.tx, p[5] = S.ty, p[6] = S.tz, p[7] = S.s;
}
__device__ __forceinline__ S3 s3_load(const double* p) {
    return S3{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]};
}

// One edge's 36 terms (constructQuadraticForm with a robust kernel, base_binary_edge.hpp:91-113)
__device__ __forceinline__ void put_terms(double* t, const double (&J)[2][7], const double (&err)[2],
                                          double info, double rho0, double rho1) {
    const double w = rho1 * info;
    const double r0 = ((-info) * err[0]) * rho1, r1 = ((-info) * err[1]) * rho1;
    int o = 0;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
#pragma unroll
        for (int q = 0; q <= r; ++q) t[o++] = (J[0][r] * w) * J[0][q] + (J[1][r] * w) * J[1][q];
    }
#pragma unroll
    for (int r = 0; r < 7; ++r) t[28 + r] = J[0][r] * r0 + J[1][r] * r1;
    t[35] = rho0;
}

// computeActiveErrors + activeRobustChi2 at E, and with BUILD also buildSystem at E (the numeric
// linearizeOplus + constructQuadraticForm of every active edge).  Leaves sums[35] = chi2 and,
// with BUILD, sums[0..27] = H (i >= j, row by row) and sums[28..34] = b in c.S.  dropped: bit k
// is set when this lane's pair of chunk k left the graph after the first stage.
template <bool BUILD>
__device__ __forceinline__ void evaluate(const JobCtx& c, const S3& E, unsigned long long dropped) {
    const int lane = c.lane;
    if (BUILD) {
        // the 14 estimates of the numeric differentiation: lane 2d is +delta e_d, lane 2d+1 -delta e_d
        if (lane < 14) {
            const int d = lane >> 1;
            const double v = (lane & 1) ? -1e-9 : 1e-9;
            double u[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) u[k] = k == d ? v : 0.0;
            if (c.fix_scale) u[6] = 0.0;
            S3 X;
            s3_exp(u, X);           // |u| = 1e-9: nothing to refuse
            const S3 Pd = s3_mul(X, E);
            s3_store(c.P + 16 * lane, Pd);
            s3_store(c.P + 16 * lane + 8, s3_inverse(Pd));
        }
        wave_sync();
    }
    const S3 Einv = s3_inverse(E);
    double acc = 0.0;
    int chunk = 0;
    for (int base = 0; base < c.n; base += 64, ++chunk) {
        const int i = base + lane;
        const bool active = i < c.n && !((dropped >> chunk) & 1ull);
        const unsigned long long mask = __ballot(active);
        if (mask == 0) continue;
        const int cnt = __popcll(mask);
        const int slot = __popcll(mask & ((1ull << lane) - 1ull));
        double e12[2] = {0.0, 0.0}, e21[2] = {0.0, 0.0}, J12[2][7], J21[2][7];
        double rho12 = 0.0, rho21 = 0.0, w12 = 1.0, w21 = 1.0;
        PairIn p;
        p.info1 = p.info2 = 0.0;
        if (active) {
            load_pair(c, i, p);
            edge_error(E, p.X2, p.o1, c.K1, e12);
            edge_error(Einv, p.X1, p.o2, c.K2, e21);
            huber(edge_chi2(e12, p.info1), c.delta, rho12, w12);
            huber(edge_chi2(e21, p.info2), c.delta, rho21, w21);
            if (BUILD) {
                const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll
                for (int d = 0; d < 7; ++d) {
                    const double* pp = c.P + 32 * d;
                    double a[2], b[2];
                    edge_error(s3_load(pp), p.X2, p.o1, c.K1, a);
                    edge_error(s3_load(pp + 16), p.X2, p.o1, c.K1, b);
                    J12[0][d] = scalar * (a[0] - b[0]);
                    J12[1][d] = scalar * (a[1] - b[1]);
                    edge_error(s3_load(pp + 8), p.X1, p.o2, c.K2, a);
                    edge_error(s3_load(pp + 24), p.X1, p.o2, c.K2, b);
                    J21[0][d] = scalar * (a[0] - b[0]);
                    J21[1][d] = scalar * (a[1] - b[1]);
                }
            }
        }
        if (BUILD) {
            // 32 pairs (64 edges) of the chunk at a time
            for (int half = 0; half * SO_HALF < cnt; ++half) {
                if (active && (slot >> 5) == half) {
                    double* t = c.T + (2 * (slot & 31)) * SO_TERMS;
                    put_terms(t, J12, e12, p.info1, rho12, w12);
                    put_terms(t + SO_TERMS, J21, e21, p.info2, rho21, w21);
                }
                wave_sync();
                const int left = cnt - half * SO_HALF;
                const int ne = 2 * (left < SO_HALF ? left : SO_HALF);
                if (lane < SO_TERMS)
                    for (int k = 0; k < ne; ++k) acc = acc + c.T[k * SO_TERMS + lane];
                wave_sync();
            }
        } else {
            if (active) {
                c.T[2 * slot] = rho12;
                c.T[2 * slot + 1] = rho21;
            }
            wave_sync();
            if (lane == 35)
                for (int k = 0; k < 2 * cnt; ++k) acc = acc + c.T[k];
            wave_sync();
        }
    }
    if (BUILD ? lane < SO_TERMS : lane == 35) c.S[lane] = acc;
    wave_sync();
}

struct LmCount { uint32_t iters, trials, flags; };

// SparseOptimizer::optimize(max_iter) with OptimizationAlgorithmLevenberg::solve from est, every
// call with a fresh Levenberg state (orbx_lm.h's lm_optimize at N = 7, with s3_exp's refusals and
// fix_scale in the step); err_est: the estimate the edges' errors belong to afterwards
__device__ __forceinline__ void optimize(const JobCtx& c, int max_iter, unsigned long long dropped,
                                         S3& est, S3& err_est, LmCount& n) {
    double* sums = c.S;                    // [36]
    double* Am = c.S + SO_TERMS;           // [49] + temp[7] + y[7]: the solver's copy
    double* xs = Am + SO_A;                // [7] the solution (persists over the trials) + 8 ints
    const int lane = c.lane;
    if (lane < 7) xs[lane] = 0.0;
    wave_sync();
    double lambda = 0.0, ni = 2.0;
    int nbad_lm = 0;
    for (int iter = 0; iter < max_iter; ++iter) {
        ++n.iters;
        evaluate<true>(c, est, dropped);
        err_est = est;
        double current = sums[35], temp = current;
        const double ini = current;
        double b[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) b[j] = sums[28 + j];
        if (iter == 0) {
            double m = 0.0;
            const int dg[7] = {0, 2, 5, 9, 14, 20, 27};
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const double a = fabs(sums[dg[j]]);
                m = a < m ? m : a;
            }
            lambda = 1e-5 * m;
            ni = 2.0;
            nbad_lm = 0;
        }
        double rho = 0.0;
        int qmax = 0;
        bool again;
        do {
            const S3 backup = est;
            // setLambda(lambda, true) + solve + restoreDiagonal: the sums stay untouched
            if (lane == 0) {
                int o = 0;
                for (int r = 0; r < 7; ++r)
                    for (int q = 0; q < 7; ++q)
                        Am[7 * r + q] = q < r ? sums[o++] : q == r ? sums[o++] + lambda : 0.0;
                const bool ok = ldlt_solve_lds<7>(Am, sums + 28, xs);
                ((int*)(xs + 7))[7] = ok ? 1 : 0;
            }
            wave_sync();
            bool ok2 = ((const int*)(xs + 7))[7] != 0;
            if (!ok2) n.flags |= ORBX_SIM3OPT_NONPOSITIVE_SOLVE;
            ++n.trials;
            double x[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) x[j] = xs[j];
            wave_sync();
            // oplusImpl zeroes the solver's own x[6] (types_seven_dof_expmap.h:60-69)
            if (c.fix_scale) x[6] = 0.0;
            S3 X;
            const uint32_t why = (uint32_t)__builtin_amdgcn_readfirstlane((int)s3_exp(x, X));
            if (why == 0) {
                est = s3_mul(X, est);
                evaluate<false>(c, est, dropped);
                err_est = est;
                temp = sums[35];
            } else {
                n.flags |= why;
                ok2 = false;
            }
            if (!ok2) temp = DBL_MAX;
            rho = current - temp;
            double scale = 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) scale = scale + x[j] * (lambda * x[j] + b[j]);
            scale = scale + 1e-3;
            rho = dv(rho, scale);
            if (uniform(rho > 0.0 && isfinite(temp))) {
                const double t = 2.0 * rho - 1.0;
                double alpha = 1.0 - (t * t) * t;
                const double up = 2.0 / 3.0, lo = 1.0 / 3.0;
                alpha = up < alpha ? up : alpha;
                lambda = lambda * (lo < alpha ? alpha : lo);
                ni = 2.0;
                current = temp;
            } else {
                lambda = lambda * ni;
                ni = ni * 2.0;
                est = backup;
            }
            ++qmax;
            again = uniform(rho < 0.0 && qmax < 10);
        } while (again);
        if (uniform(qmax == 10 || rho == 0.0)) break;
        if ((ini - current) * 1e3 < ini) ++nbad_lm;
        else nbad_lm = 0;
        if (uniform(nbad_lm >= 3)) break;
    }
}

// e12->chi2() > th2 || e21->chi2() > th2 (Optimizer.cc:1217, :1251) for every pair still in the
// graph, on the stored errors: those of err_est.  Sets the lanes' dropped bits and the keep bytes
// of the failing pairs; returns their count.
__device__ __forceinline__ int classify(const JobCtx& c, const S3& err_est, double th2,
                                        uint8_t* keep, unsigned long long& dropped) {
    const S3 Einv = s3_inverse(err_est);
    int nfail = 0, chunk = 0;
    for (int base = 0; base < c.n; base += 64, ++chunk) {
        const int i = base + c.lane;
        bool fail = false;
        if (i < c.n && !((dropped >> chunk) & 1ull)) {
            PairIn p;
            load_pair(c, i, p);
            double e12[2], e21[2];
            edge_error(err_est, p.X2, p.o1, c.K1, e12);
            edge_error(Einv, p.X1, p.o2, c.K2, e21);
            fail = edge_chi2(e12, p.info1) > th2 || edge_chi2(e21, p.info2) > th2;
            if (fail) {
                keep[c.corr[i].i1] = 0;
                dropped |= 1ull << chunk;
            }
        }
        nfail += (int)__popcll(__ballot(fail));
    }
    return nfail;
}

__global__ __launch_bounds__(64 * SO_WAVES) void k_sim3_opt(const Sim3OptLaunch g) {
    __shared__ double lds[SO_WAVES * SO_LDS_PER_WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x * SO_WAVES + wave;
    if (j >= g.njobs) return;
    const orbx_sim3opt_job& J = g.jobs[j];
    orbx_sim3opt_result& res = g.res[j];
    const orbx_sim3opt_in& in = *(const orbx_sim3opt_in*)(g.sim3_in + (size_t)j * g.in_stride);

    // g2o::Sim3(toMatrix3d(R12), toVector3d(t12), s12)
    S3 start;
    {
        double R[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) R[r][q] = (double)in.R12[3 * r + q];
        quat_from_matrix(R, start.qx, start.qy, start.qz, start.qw);
        start.tx = (double)in.t12[0], start.ty = (double)in.t12[1], start.tz = (double)in.t12[2];
        start.s = (double)in.s12;
    }
    // the result record: counts, info, g2oS12 and Converter::toCvMat(g2oS12) (Converter.cc:
    // s * toRotationMatrix(), t, each rounded to float)
    auto finish = [&](const S3& S, int n_in, int n_corr, int n_bad, uint32_t info) {
        if (lane != 0) return;
        res.n_inliers = n_in, res.n_correspondences = n_corr, res.n_bad = n_bad, res.info = info;
        res.q[0] = S.qx, res.q[1] = S.qy, res.q[2] = S.qz, res.q[3] = S.qw;
        res.t[0] = S.tx, res.t[1] = S.ty, res.t[2] = S.tz, res.s = S.s;
        const double tx = 2.0 * S.qx, ty = 2.0 * S.qy, tz = 2.0 * S.qz;
        const double twx = tx * S.qw, twy = ty * S.qw, twz = tz * S.qw;
        const double txx = tx * S.qx, txy = ty * S.qx, txz = tz * S.qx;
        const double tyy = ty * S.qy, tyz = tz * S.qy, tzz = tz * S.qz;
        const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz),
                             tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)};
        const double t[3] = {S.tx, S.ty, S.tz};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int q = 0; q < 3; ++q) res.T12[4 * r + q] = (float)(S.s * R[3 * r + q]);
            res.T12[4 * r + 3] = (float)t[r];
            res.T12[12 + r] = 0.0f;
        }
        res.T12[15] = 1.0f;
    };

    // refusals: nothing of a refused job is read further
    uint32_t refuse = 0;
    const int N = J.N;
    if (J.nlevels1 < 1 || J.nlevels1 > 16 || J.nlevels2 < 1 || J.nlevels2 > 16)
        refuse |= ORBX_SIM3OPT_REFUSED_OCTAVE;
    if (N < 0 || N > g.max_n || J.mN1 < 0) refuse |= ORBX_SIM3OPT_REFUSED_LIMIT;
    if (J.kf1 < 0 || J.kf1 >= g.nposes || J.kf2 < 0 || J.kf2 >= g.nposes || J.corr_off < 0 ||
        (long long)J.corr_off + N > g.ncorr || J.flag_off < 0 ||
        (long long)J.flag_off + J.mN1 > g.nkeep)
        refuse |= ORBX_SIM3OPT_REFUSED_RANGE;
    const orbx_sim3opt_corr* corr = g.corr + J.corr_off;
    if (!refuse) {
        bool bad_oct = false, bad_i1 = false;
        for (int base = 0; base < N; base += 64) {
            const int i = base + lane;
            if (i < N) {
                const orbx_sim3opt_corr& q = corr[i];
                if (q.octave1 < 0 || q.octave1 >= J.nlevels1 || q.octave2 < 0 ||
                    q.octave2 >= J.nlevels2)
                    bad_oct = true;
                if (q.i1 < 0 || q.i1 >= J.mN1 || (i > 0 && corr[i - 1].i1 >= q.i1)) bad_i1 = true;
            }
        }
        if (__ballot(bad_oct)) refuse |= ORBX_SIM3OPT_REFUSED_OCTAVE;
        if (__ballot(bad_i1)) refuse |= ORBX_SIM3OPT_REFUSED_I1;
    }
    if (refuse) {
        finish(start, 0, 0, 0, refuse);
        return;
    }

    JobCtx c;
    c.corr = corr;
    c.F1 = g.poses + J.kf1;
    c.F2 = g.poses + J.kf2;
    c.sigma2_1 = J.sigma2_1;
    c.sigma2_2 = J.sigma2_2;
    c.n = N;
    c.lane = lane;
    c.fix_scale = J.fix_scale != 0;
    c.K1 = {(double)c.F1->fx, (double)c.F1->fy, (double)c.F1->cx, (double)c.F1->cy};
    c.K2 = {(double)c.F2->fx, (double)c.F2->fy, (double)c.F2->cx, (double)c.F2->cy};
    // const float deltaHuber = sqrt(th2): the float square root, correctly rounded through double
    c.delta = (double)(float)sq((double)J.th2);
    c.T = lds + wave * SO_LDS_PER_WAVE;
    c.P = c.T + SO_T;
    c.S = c.P + SO_P;
    uint8_t* keep = g.keep + J.flag_off;
    const double th2 = (double)J.th2;

    S3 est = start, err_est = start;
    LmCount cnt = {0, 0, 0};
    unsigned long long dropped = 0;
    int rounds = 0;
    // ---- optimize(5); without an edge the optimizer has nothing to initialise and returns
    if (N > 0) {
        optimize(c, 5, dropped, est, err_est, cnt);
        ++rounds;
    }
    const int nbad = classify(c, err_est, th2, keep, dropped);
    if (nbad > 0) cnt.flags |= ORBX_SIM3OPT_DROPPED;
    auto word = [&]() {
        return (uint32_t)rounds | (cnt.iters << ORBX_SIM3OPT_ITERS_SHIFT) |
               (cnt.trials << ORBX_SIM3OPT_TRIALS_SHIFT) | cnt.flags;
    };
    if (N - nbad < 10) {       // return 0: g2oS12 stays as it came in, the dropped pairs stay dropped
        cnt.flags |= ORBX_SIM3OPT_FEW_INLIERS;
        finish(start, 0, N, nbad, word());
        return;
    }
    // ---- optimize(nMoreIterations) on the pairs that are left, from the estimate as it stands
    optimize(c, nbad > 0 ? 10 : 5, dropped, est, err_est, cnt);
    ++rounds;
    const int nfail = classify(c, err_est, th2, keep, dropped);
    finish(est, N - nbad - nfail, N, nbad, word());
}

hipError_t launch_sim3_opt(const Sim3OptLaunch& a, hipStream_t st) {
    hipLaunchKernelGGL(k_sim3_opt, dim3((a.njobs + SO_WAVES - 1) / SO_WAVES), dim3(64 * SO_WAVES),
                       0, st, a);
    return hipGetLastError();
}

}  // namespace

extern "C" {

orbx_status orbx_sim3opt_limits(int32_t* max_n, int32_t* max_jobs) {
    if (max_n) *max_n = SIM3OPT_MAX_N;
    if (max_jobs) *max_jobs = SIM3OPT_MAX_JOBS;
    return ORBX_OK;
}

orbx_status orbx_sim3_optimize(const orbx_frame_pose* pose1, const orbx_frame_pose* pose2,
                               const orbx_sim3opt_job* job, const orbx_sim3opt_corr* corr,
                               const orbx_sim3opt_in* sim3_in, orbx_sim3opt_result* res,
                               uint8_t* keep, int device) {
    if (!pose1 || !pose2 || !job || !sim3_in || !res) return ORBX_ERR_INVALID;
    if (job->N < 0 || job->mN1 < 0 || (job->N > 0 && !corr) || (job->mN1 > 0 && !keep))
        return ORBX_ERR_INVALID;
    if (job->N > SIM3OPT_MAX_N) return ORBX_ERR_UNSUPPORTED;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const int N = job->N, mN1 = job->mN1;
    const orbx_frame_pose poses[2] = {*pose1, *pose2};
    orbx_sim3opt_job hj = *job;
    hj.kf1 = 0, hj.kf2 = 1, hj.corr_off = 0, hj.flag_off = 0;
    const size_t p_pose = p.in(poses, sizeof(poses)), p_job = p.in(&hj, sizeof(hj)),
                 p_in = p.in(sim3_in, sizeof(*sim3_in)),
                 p_corr = p.in(corr, sizeof(orbx_sim3opt_corr) * (size_t)N),
                 p_keep = p.inout(keep, (size_t)mN1), p_res = p.out(res, sizeof(*res), true);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    Sim3OptLaunch L{};
    L.jobs = c.dev<orbx_sim3opt_job>(p_job);
    L.njobs = 1, L.max_n = N;
    L.poses = c.dev<orbx_frame_pose>(p_pose);
    L.nposes = 2;
    L.corr = c.dev<orbx_sim3opt_corr>(p_corr);
    L.ncorr = N;
    L.sim3_in = c.dev<uint8_t>(p_in);
    L.in_stride = sizeof(orbx_sim3opt_in);
    L.res = c.dev<orbx_sim3opt_result>(p_res);
    L.keep = c.dev<uint8_t>(p_keep);
    L.nkeep = mN1;
    return c.finish(HIPOK(launch_sim3_opt(L, c.st())) ? ORBX_OK : ORBX_ERR_DEVICE);
}

orbx_status orbx_sim3_optimize_batch_device(
    orbx_matcher* m, const orbx_sim3opt_job* d_jobs, int32_t njobs, int32_t max_n,
    const orbx_frame_pose* d_poses, int32_t nposes, const orbx_sim3opt_corr* d_corr, int64_t ncorr,
    const void* d_sim3_in, int64_t sim3_in_stride, orbx_sim3opt_result* d_results,
    uint8_t* d_keep, int64_t nkeep_bytes, void* stream) {
    if (!m || njobs < 0 || max_n < 0 || nposes < 0 || ncorr < 0 || nkeep_bytes < 0)
        return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_jobs || !d_poses || !d_sim3_in || !d_results || (ncorr > 0 && !d_corr) ||
        (nkeep_bytes > 0 && !d_keep) || sim3_in_stride < (int64_t)sizeof(orbx_sim3opt_in) ||
        (sim3_in_stride & 3) || ((uintptr_t)d_sim3_in & 3))
        return ORBX_ERR_INVALID;
    if (njobs > SIM3OPT_MAX_JOBS || max_n > SIM3OPT_MAX_N) return ORBX_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    Sim3OptLaunch L{};
    L.jobs = d_jobs;
    L.njobs = njobs, L.max_n = max_n;
    L.poses = d_poses;
    L.nposes = nposes;
    L.corr = d_corr;
    L.ncorr = ncorr;
    L.sim3_in = (const uint8_t*)d_sim3_in;
    L.in_stride = sim3_in_stride;
    L.res = d_results;
    L.keep = d_keep;
    L.nkeep = nkeep_bytes;
    return HIPOK(launch_sim3_opt(L, (hipStream_t)stream)) ? ORBX_OK : ORBX_ERR_DEVICE;
}

}  // extern "C"
