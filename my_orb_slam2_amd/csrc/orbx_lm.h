// orbx_lm.h — the device code that k_pose_opt (orbx_poseopt.hip) and k_sim3_opt (orbx_sim3opt.hip)
// share: both restate a g2o graph of one vertex with fixed points, so both need the same wave
// helpers, the same Eigen forms (quaternion from a matrix, rotation of a vector, quaternion
// product, pivoted LDLT) [unverified-Eigen], RobustKernelHuber, and the whole of
// OptimizationAlgorithmLevenberg::solve.  The edge models (error, Jacobian, update of the
// estimate) stay with the kernels and reach the loop as callables; k_pose_opt runs lm_optimize,
// k_sim3_opt keeps the same loop written out (it measured slower through the template).  The
// exactly rounded dv and sq are orbx_cv.h's, as are the OpenCV forms both kernels call.
// Built with -ffp-contract=off like the rest of the library: every operation is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "orbx_cv.h"

namespace orbx {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ bool uniform(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }

// Eigen's Quaternion(Matrix3) for one position of the largest diagonal entry
template <int I>
__device__ __forceinline__ void quat_branch(const double (&R)[3][3], double (&c)[3], double& w) {
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double t = sq(((R[I][I] - R[J][J]) - R[K][K]) + 1.0);
    c[I] = 0.5 * t;
    t = dv(0.5, t);
    w = (R[K][J] - R[J][K]) * t;
    c[J] = (R[J][I] + R[I][J]) * t;
    c[K] = (R[K][I] + R[I][K]) * t;
}

// Quaterniond(Matrix3d), not normalised afterwards: as g2o::Sim3 keeps it (sim3.h:64-66, :136);
// SE3Quat normalises it with a call of its own (orbx_poseopt.hip, se3_quat)
__device__ __forceinline__ void quat_from_matrix(const double (&R)[3][3], double& x, double& y,
                                                 double& z, double& w) {
    double t = (R[0][0] + R[1][1]) + R[2][2];
    if (t > 0.0) {
        t = sq(t + 1.0);
        w = 0.5 * t;
        t = dv(0.5, t);
        x = (R[2][1] - R[1][2]) * t;
        y = (R[0][2] - R[2][0]) * t;
        z = (R[1][0] - R[0][1]) * t;
    } else {
        double c[3];
        const bool one = R[1][1] > R[0][0];
        const bool two = R[2][2] > (one ? R[1][1] : R[0][0]);
        if (two) quat_branch<2>(R, c, w);
        else if (one) quat_branch<1>(R, c, w);
        else quat_branch<0>(R, c, w);
        x = c[0], y = c[1], z = c[2];
    }
}

// Eigen's Quaternion * Vector3: v + w*(2 q x v) + q x (2 q x v)
__device__ __forceinline__ void quat_rotate(double qx, double qy, double qz, double qw, double px,
                                            double py, double pz, double& ox, double& oy,
                                            double& oz) {
    double ux = qy * pz - qz * py, uy = qz * px - qx * pz, uz = qx * py - qy * px;
    ux = ux + ux, uy = uy + uy, uz = uz + uz;
    const double cx = qy * uz - qz * uy, cy = qz * ux - qx * uz, cz = qx * uy - qy * ux;
    ox = (px + qw * ux) + cx;
    oy = (py + qw * uy) + cy;
    oz = (pz + qw * uz) + cz;
}

// Eigen's Quaternion * Quaternion (the Hamilton product a * b), not normalised; the result is
// written as it is computed, so it is an object of its own
__device__ __forceinline__ void quat_mul(const double& ax, const double& ay, const double& az,
                                         const double& aw, const double& bx, const double& by,
                                         const double& bz, const double& bw, double& x, double& y,
                                         double& z, double& w) {
    w = ((aw * bw - ax * bx) - ay * by) - az * bz;
    x = ((aw * bx + ax * bw) + ay * bz) - az * by;
    y = ((aw * by + ay * bw) + az * bx) - ax * bz;
    z = ((aw * bz + az * bw) + ax * by) - ay * bx;
}

// RobustKernelHuber::robustify: rho and rho'
__device__ __forceinline__ void huber(double e2, double delta, double& rho0, double& rho1) {
    const double dsqr = delta * delta;
    if (e2 <= dsqr) {
        rho0 = e2;
        rho1 = 1.0;
    } else {
        const double se = sq(e2);
        rho0 = (2.0 * se) * delta - dsqr;
        rho1 = dv(delta, se);
    }
}

// Eigen::LDLT<MatrixXd>::compute + solve on the lower triangle of the NxN at A (row-major, LDS:
// A[N*N], then temp[N] and y[N]), b -> x [unverified-Eigen]; false: not positive (x is left as it
// is).  Runs on one lane.
template <int N>
__device__ __forceinline__ bool ldlt_solve_lds(double* A, const double* b, double* x) {
    int* trl = (int*)(x + N);             // N ints behind x: the transpositions, indexed freely
    int sign = 0;                         // 0 zero, 1 positive, -1 negative, 2 indefinite
    for (int k = 0; k < N; ++k) {
        int idx = k;
        double best = fabs(A[(N + 1) * k]);
        for (int i = k + 1; i < N; ++i) {
            const double v = fabs(A[(N + 1) * i]);
            if (v > best) best = v, idx = i;
        }
        trl[k] = idx;
        if (idx != k) {
            for (int j = 0; j < k; ++j) {
                const double t = A[N * k + j];
                A[N * k + j] = A[N * idx + j];
                A[N * idx + j] = t;
            }
            for (int i = idx + 1; i < N; ++i) {
                const double t = A[N * i + k];
                A[N * i + k] = A[N * i + idx];
                A[N * i + idx] = t;
            }
            {
                const double t = A[(N + 1) * k];
                A[(N + 1) * k] = A[(N + 1) * idx];
                A[(N + 1) * idx] = t;
            }
            for (int i = k + 1; i < idx; ++i) {
                const double t = A[N * i + k];
                A[N * i + k] = A[N * idx + i];
                A[N * idx + i] = t;
            }
        }
        if (k > 0) {
            double* temp = A + N * N;   // D * A10^T
            for (int j = 0; j < k; ++j) temp[j] = A[(N + 1) * j] * A[N * k + j];
            double s = A[N * k] * temp[0];
            for (int j = 1; j < k; ++j) s = s + A[N * k + j] * temp[j];
            A[(N + 1) * k] = A[(N + 1) * k] - s;
            for (int i = k + 1; i < N; ++i) {
                double si = A[N * i] * temp[0];
                for (int j = 1; j < k; ++j) si = si + A[N * i + j] * temp[j];
                A[N * i + k] = A[N * i + k] - si;
            }
        }
        const double akk = A[(N + 1) * k];
        const bool valid = fabs(akk) > 0.0;
        if (k == 0 && !valid) {
            for (int j = 0; j < N; ++j) trl[j] = j;
            break;
        }
        if (valid)
            for (int i = k + 1; i < N; ++i) A[N * i + k] = dv(A[N * i + k], akk);
        if (sign == 1) {
            if (akk < 0.0) sign = 2;
        } else if (sign == -1) {
            if (akk > 0.0) sign = 2;
        } else if (sign == 0) {
            if (akk > 0.0) sign = 1;
            else if (akk < 0.0) sign = -1;
        }
    }
    if (!(sign == 1 || sign == 0)) return false;
    double* y = A + N * N + N;
    for (int i = 0; i < N; ++i) y[i] = b[i];
    for (int k = 0; k < N; ++k) {
        const int o = trl[k];
        const double t = y[k];
        y[k] = y[o];
        y[o] = t;
    }
    for (int j = 0; j < N; ++j)
        for (int i = j + 1; i < N; ++i) y[i] = y[i] - A[N * i + j] * y[j];
    for (int i = 0; i < N; ++i) y[i] = fabs(A[(N + 1) * i]) > DBL_MIN ? dv(y[i], A[(N + 1) * i]) : 0.0;
    for (int i = N - 2; i >= 0; --i) {
        double s = A[N * (i + 1) + i] * y[i + 1];
        for (int j = i + 2; j < N; ++j) s = s + A[N * j + i] * y[j];
        y[i] = y[i] - s;
    }
    for (int k = N - 1; k >= 0; --k) {
        const int o = trl[k];
        const double t = y[k];
        y[k] = y[o];
        y[o] = t;
    }
    for (int i = 0; i < N; ++i) x[i] = y[i];
    return true;
}

// SparseOptimizer::optimize(max_iter) (sparse_optimizer.cpp:354-419) with
// OptimizationAlgorithmLevenberg::solve for one vertex of dimension N, from est, with a fresh
// Levenberg state.  Every lane runs it alike; the estimate and the state are wave-uniform.
//   sums   LDS: H (N(N+1)/2 entries, i >= j, row by row), then b[N], then the robust chi2
//   Am     LDS: the solver's copy, A[N*N] + temp[N] + y[N] (ldlt_solve_lds)
//   xs     LDS: the solution x[N] (it persists over the trials), then N + 1 ints
//   eval_build(est)   computeActiveErrors + activeRobustChi2 + buildSystem at est, into sums
//   eval_chi2(est)    computeActiveErrors + activeRobustChi2 at est, into sums' last entry
//   step(x, est)      oplus: est updated by x (which it may edit, as an oplusImpl that zeroes a
//                     component does); 0, or wave-uniform the flag of a refusal (est is then as
//                     it was and the trial counts as failed)
// nonpositive: the caller's flag for a system the LDLT found not positive.
template <int N, class Est, class EvalBuild, class EvalChi2, class Step>
__device__ __forceinline__ void lm_optimize(double* sums, double* Am, double* xs, int lane,
                                            int max_iter, uint32_t& iters, uint32_t& trials,
                                            uint32_t& flags, uint32_t nonpositive, Est& est,
                                            EvalBuild eval_build, EvalChi2 eval_chi2, Step step) {
    constexpr int B = N * (N + 1) / 2, CHI = B + N;
    if (lane < N) xs[lane] = 0.0;
    wave_sync();
    double lambda = 0.0, ni = 2.0;
    int nbad_lm = 0;
    for (int iter = 0; iter < max_iter; ++iter) {
        ++iters;
        eval_build(est);
        double current = sums[CHI], temp = current;
        const double ini = current;
        double b[N];
#pragma unroll
        for (int j = 0; j < N; ++j) b[j] = sums[B + j];
        if (iter == 0) {
            double m = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double a = fabs(sums[j * (j + 3) / 2]);   // H(j, j)
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
            const Est backup = est;
            // setLambda(lambda, true) + solve + restoreDiagonal: the sums stay untouched
            if (lane == 0) {
                int o = 0;
                for (int r = 0; r < N; ++r)
                    for (int q = 0; q < N; ++q)
                        Am[N * r + q] = q < r ? sums[o++] : q == r ? sums[o++] + lambda : 0.0;
                const bool ok = ldlt_solve_lds<N>(Am, sums + B, xs);
                ((int*)(xs + N))[N] = ok ? 1 : 0;
            }
            wave_sync();
            bool ok2 = ((const int*)(xs + N))[N] != 0;
            if (!ok2) flags |= nonpositive;
            ++trials;
            double x[N];
#pragma unroll
            for (int j = 0; j < N; ++j) x[j] = xs[j];
            wave_sync();
            const uint32_t why = step(x, est);
            if (why == 0) {
                eval_chi2(est);
                temp = sums[CHI];
            } else {
                flags |= why;
                ok2 = false;
            }
            if (!ok2) temp = DBL_MAX;
            rho = current - temp;
            double scale = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) scale = scale + x[j] * (lambda * x[j] + b[j]);
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

}  // namespace orbx
