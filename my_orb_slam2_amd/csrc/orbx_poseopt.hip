// orbx_poseopt.hip — Optimizer::PoseOptimization (src/Optimizer.cc:245-457) on the device
// (include/orbx_frame.h, orbx_pose_optimization*), and the inversion of a projection search's
// output into mvpMapPoints that feeds it (orbx_matches_to_features_batch_device).
//
// k_pose_opt: one wave per frame, PO_WAVES frames per workgroup; the waves of a workgroup never
// meet (no workgroup barrier).  The g2o graph of the call is one SE3 vertex with unary edges, so
// the whole of OptimizationAlgorithmLevenberg::solve is restated (orbx_lm.h): every evaluation walks
// the frame's features in chunks of 64, one lane per feature; the active edges of a chunk put their
// per-edge terms (21 lower-triangle entries of H, 6 of b, the robust chi2) into LDS, compacted in
// edge order, and 28 lanes then add one term each, edge by edge: the sums round exactly as g2o's
// loop over _activeEdges does.  The 6x6 system, the pose and the Levenberg state are wave-uniform:
// the pivoted LDLT runs on lane 0 over an LDS copy, the rest is computed by every lane alike.
// An edge's _error is never stored: it is a function of the pose it was last evaluated at, and
// that pose is kept instead (g2o does not recompute errors after a rejected trial).
//
// The Levenberg loop, the forms evaluated inside Eigen, the robust kernel and the LDLT are
// orbx_lm.h's (all but the loop shared with k_sim3_opt); the edge model (pose_map, pose_update,
// edge_error, the analytic Jacobian) is here.  sin / cos are orbx_sincos_f64 (orbx_math.h).  Built
// with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/orbx_frame.h"
#include "orbx_host.h"
#include "orbx_lm.h"
#include "orbx_math.h"

using namespace orbx;

namespace {

constexpr int PO_WAVES = 4;                 // frames per workgroup
constexpr int PO_TERMS = 28;                // 21 of H (i >= j), 6 of b, robust chi2
constexpr int PO_LDS_PER_WAVE = 64 * PO_TERMS + 96;   // doubles: the chunk's terms, then the system
constexpr uint32_t PO_MAX_FEAT = 32768;

struct PoseOptLaunch {
    const orbx_frame_pose* poses;
    int nframes;
    const orbx_keypoint* keys;
    const float* u_right;
    const int32_t* feat_off;
    int max_feat;
    const int32_t* mp_of_feat;
    const orbx_map_point* mps;
    const int32_t* mp_off;
    orbx_frame_pose* poses_out;
    uint8_t* outlier;
    int32_t* ngood;
    uint32_t* info;
};

struct Pose7 { double qx, qy, qz, qw, tx, ty, tz; };
struct Cam { double fx, fy, cx, cy, bf; };

// normalizeRotation (se3quat.h:280-285)
__device__ __forceinline__ void quat_normalize(double& x, double& y, double& z, double& w) {
    if (w < 0.0) x = -x, y = -y, z = -z, w = -w;
    const double n = sq(((x * x + y * y) + z * z) + w * w);
    x = dv(x, n), y = dv(y, n), z = dv(z, n), w = dv(w, n);
}

// SE3Quat(R, t)'s rotation (se3quat.h:67-71): Quaterniond(R), then normalizeRotation
__device__ __forceinline__ void se3_quat(const double (&R)[3][3], double& x, double& y, double& z,
                                         double& w) {
    quat_from_matrix(R, x, y, z, w);
    quat_normalize(x, y, z, w);
}

// SE3Quat::map
__device__ __forceinline__ void pose_map(const Pose7& T, const float* Xw, double& x, double& y,
                                         double& z) {
    double rx, ry, rz;
    quat_rotate(T.qx, T.qy, T.qz, T.qw, (double)Xw[0], (double)Xw[1], (double)Xw[2], rx, ry, rz);
    x = rx + T.tx, y = ry + T.ty, z = rz + T.tz;
}

// VertexSE3Expmap::oplusImpl: SE3Quat::exp(u) * T (se3quat.h:104-110, 223-257); false: theta is
// outside orbx_sincos_f64's range and T is left as it is
__device__ __forceinline__ bool pose_update(const double (&u)[6], Pose7& T) {
    const double theta = sq((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const double O[3][3] = {{0.0, -u[2], u[1]}, {u[2], 0.0, -u[0]}, {-u[1], u[0], 0.0}};
    double R[3][3], V[3][3];
    double a = 1.0, b = 1.0, d = 1.0;
    const bool small = theta < 0.00001;
    if (!small) {
        double s, c;
        if (!orbx_sincos_f64(theta, &s, &c)) return false;
        a = dv(s, theta);
        b = dv(1.0 - c, theta * theta);
        d = dv(theta - s, (theta * theta) * theta);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double o2 = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];
            const double e = i == j ? 1.0 : 0.0;
            if (small) {
                R[i][j] = (e + O[i][j]) + o2;
                V[i][j] = R[i][j];
            } else {
                R[i][j] = (e + a * O[i][j]) + b * o2;
                V[i][j] = (e + b * O[i][j]) + d * o2;
            }
        }
    double ex, ey, ez, ew;
    se3_quat(R, ex, ey, ez, ew);
    const double t0 = (V[0][0] * u[3] + V[0][1] * u[4]) + V[0][2] * u[5];
    const double t1 = (V[1][0] * u[3] + V[1][1] * u[4]) + V[1][2] * u[5];
    const double t2 = (V[2][0] * u[3] + V[2][1] * u[4]) + V[2][2] * u[5];
    double rx, ry, rz;
    quat_rotate(ex, ey, ez, ew, T.tx, T.ty, T.tz, rx, ry, rz);
    Pose7 N;
    N.tx = t0 + rx, N.ty = t1 + ry, N.tz = t2 + rz;
    quat_mul(ex, ey, ez, ew, T.qx, T.qy, T.qz, T.qw, N.qx, N.qy, N.qz, N.qw);
    quat_normalize(N.qx, N.qy, N.qz, N.qw);
    T = N;
    return true;
}

// One feature's edge as the lane holds it
struct EdgeIn {
    double ox, oy, our, info;
    float Xw[3];
    bool stereo;
};

// computeError (types_six_dof_expmap.h:153-157, 184-188) and chi2 (base_edge.h:60); x, y, z:
// the MapPoint in the camera frame, which linearizeOplus maps again to the same bits
__device__ __forceinline__ double edge_error(const EdgeIn& e, const Pose7& T, const Cam& K,
                                             double (&err)[3], double& x, double& y, double& z) {
    pose_map(T, e.Xw, x, y, z);
    double chi;
    if (e.stereo) {
        const double invz = (double)(float)dv(1.0, z);
        const double u = (x * invz) * K.fx + K.cx;
        const double v = (y * invz) * K.fy + K.cy;
        err[0] = e.ox - u;
        err[1] = e.oy - v;
        err[2] = e.our - (u - K.bf * invz);
        chi = (err[0] * (e.info * err[0]) + err[1] * (e.info * err[1])) + err[2] * (e.info * err[2]);
    } else {
        err[0] = e.ox - (dv(x, z) * K.fx + K.cx);
        err[1] = e.oy - (dv(y, z) * K.fy + K.cy);
        err[2] = 0.0;
        chi = err[0] * (e.info * err[0]) + err[1] * (e.info * err[1]);
    }
    return chi;
}

// The frame as one wave sees it
struct FrameCtx {
    const orbx_keypoint* keys;
    const float* ur;            // NULL: mono
    const int32_t* mp_of_feat;
    const orbx_map_point* mps;
    uint8_t* outlier;
    const float* scale;         // the pose record's scale table
    int n, lane;
    Cam K;
    double delta_mono, delta_stereo;
    double* T;                  // LDS: 64 x PO_TERMS terms of the chunk
    double* S;                  // LDS: sums[28], A[36] + temp[6] + y[6] ... (see k_pose_opt)
};

// Feature i's edge; ACTIVE_ONLY: none for an edge at level 1 (its flag is set), decided before
// anything else of the edge is read
template <bool ACTIVE_ONLY>
__device__ __forceinline__ bool load_edge(const FrameCtx& c, int i, EdgeIn& e) {
    if (i >= c.n) return false;
    const int32_t m = c.mp_of_feat[i];
    if (m < 0) return false;
    if (ACTIVE_ONLY && c.outlier[i] != 0) return false;
    const orbx_keypoint kp = c.keys[i];
    const float urf = c.ur ? c.ur[i] : -1.0f;
    e.stereo = !(urf < 0.0f);
    e.ox = (double)kp.x;
    e.oy = (double)kp.y;
    e.our = (double)urf;
    const float s = c.scale[kp.octave];
    e.info = (double)__fdiv_rn(1.0f, s * s);
    const orbx_map_point mp = c.mps[m];
    e.Xw[0] = mp.pos[0], e.Xw[1] = mp.pos[1], e.Xw[2] = mp.pos[2];
    return true;
}

// computeActiveErrors + activeRobustChi2 at T, and with BUILD also buildSystem at T
// (linearizeOplus + constructQuadraticForm of every active edge).  Leaves sums[27] = chi2 and,
// with BUILD, sums[0..20] = H (i >= j, row by row) and sums[21..26] = b in c.S.
template <bool BUILD>
__device__ __forceinline__ void evaluate(const FrameCtx& c, const Pose7& T, bool kernel) {
    double acc = 0.0;
    const int lane = c.lane;
    for (int base = 0; base < c.n; base += 64) {
        const int i = base + lane;
        EdgeIn e;
        const bool active = load_edge<true>(c, i, e);
        const unsigned long long mask = __ballot(active);
        if (mask == 0) continue;
        const int cnt = __popcll(mask);
        if (active) {
            const int slot = __popcll(mask & ((1ull << lane) - 1ull));
            double* t = c.T + slot * PO_TERMS;
            double err[3], x, y, z;
            const double chi = edge_error(e, T, c.K, err, x, y, z);
            double rho0 = chi, rho1 = 1.0;
            if (kernel) huber(chi, e.stereo ? c.delta_stereo : c.delta_mono, rho0, rho1);
            t[27] = rho0;
            if (BUILD) {
                const double invz = dv(1.0, z), invz_2 = invz * invz;
                const double fx = c.K.fx, fy = c.K.fy, bf = c.K.bf;
                double A[3][6];
                A[0][0] = ((x * y) * invz_2) * fx;
                A[0][1] = (-(1.0 + ((x * x) * invz_2))) * fx;
                A[0][2] = (y * invz) * fx;
                A[0][3] = (-invz) * fx;
                A[0][4] = 0.0;
                A[0][5] = (x * invz_2) * fx;
                A[1][0] = (1.0 + (y * y) * invz_2) * fy;
                A[1][1] = (((-x) * y) * invz_2) * fy;
                A[1][2] = ((-x) * invz) * fy;
                A[1][3] = 0.0;
                A[1][4] = (-invz) * fy;
                A[1][5] = (y * invz_2) * fy;
                A[2][0] = A[0][0] - (bf * y) * invz_2;
                A[2][1] = A[0][1] + (bf * x) * invz_2;
                A[2][2] = A[0][2];
                A[2][3] = A[0][3];
                A[2][4] = 0.0;
                A[2][5] = A[0][5] - bf * invz_2;
                const double w = kernel ? rho1 * e.info : e.info;
                int o = 0;
#pragma unroll
                for (int r = 0; r < 6; ++r) {
#pragma unroll
                    for (int q = 0; q <= r; ++q) {
                        double h = (A[0][r] * w) * A[0][q] + (A[1][r] * w) * A[1][q];
                        if (e.stereo) h = h + (A[2][r] * w) * A[2][q];
                        t[o++] = h;
                    }
                }
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    double g;
                    if (kernel) {
                        g = ((rho1 * A[0][r]) * e.info) * err[0] + ((rho1 * A[1][r]) * e.info) * err[1];
                        if (e.stereo) g = g + ((rho1 * A[2][r]) * e.info) * err[2];
                    } else {
                        g = (A[0][r] * e.info) * err[0] + (A[1][r] * e.info) * err[1];
                        if (e.stereo) g = g + (A[2][r] * e.info) * err[2];
                    }
                    t[21 + r] = g;
                }
            }
        }
        wave_sync();
        if (BUILD) {
            if (lane < 21 || lane == 27) {
                for (int k = 0; k < cnt; ++k) acc = acc + c.T[k * PO_TERMS + lane];
            } else if (lane < 27) {
                for (int k = 0; k < cnt; ++k) acc = acc - c.T[k * PO_TERMS + lane];
            }
        } else if (lane == 27) {
            for (int k = 0; k < cnt; ++k) acc = acc + c.T[k * PO_TERMS + 27];
        }
        wave_sync();
    }
    if (BUILD ? lane < PO_TERMS : lane == 27) c.S[lane] = acc;
    wave_sync();
}

__global__ __launch_bounds__(64 * PO_WAVES) void k_pose_opt(const PoseOptLaunch g) {
    __shared__ double lds[PO_WAVES * PO_LDS_PER_WAVE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x * PO_WAVES + wave;
    if (f >= g.nframes) return;

    const orbx_frame_pose* P = g.poses + f;
    orbx_frame_pose* Po = g.poses_out + f;
    const int nlevels = P->nlevels;
    const int f0 = g.feat_off[f], n = g.feat_off[f + 1] - f0;
    const int m0 = g.mp_off[f], nmp = g.mp_off[f + 1] - m0;

    FrameCtx c;
    c.keys = g.keys + f0;
    c.ur = g.u_right ? g.u_right + f0 : nullptr;
    c.mp_of_feat = g.mp_of_feat + f0;
    c.mps = g.mps + m0;
    c.outlier = g.outlier + f0;
    c.scale = P->scale;
    c.n = n;
    c.lane = lane;
    c.T = lds + wave * PO_LDS_PER_WAVE;
    c.S = c.T + 64 * PO_TERMS;

    // Every word of the output record is written once.  The camera half (words 15-41: fx ...
    // scale) travels now, lane k moving word k; the pose half (Rcw, tcw, Ow: words 0-14) is
    // either copied by copy_pose() on the paths that leave the pose as it is, or written by lane 0
    // at the end.  With d_poses_out == d_poses nothing is copied.
    static_assert(sizeof(orbx_frame_pose) == 42 * 4 && offsetof(orbx_frame_pose, fx) == 15 * 4,
                  "orbx_frame_pose layout");
    if (Po != P && lane >= 15 && lane < 42) ((uint32_t*)Po)[lane] = ((const uint32_t*)P)[lane];
    auto copy_pose = [&]() {
        if (Po != P && lane < 15) ((uint32_t*)Po)[lane] = ((const uint32_t*)P)[lane];
    };

    // refusals: nothing of a refused frame is read further
    uint32_t refuse = 0;
    if (nlevels < 1 || nlevels > 16) refuse |= ORBX_POSEOPT_REFUSED_NLEVELS;
    if (n < 0 || n > g.max_feat || nmp < 0) refuse |= ORBX_POSEOPT_REFUSED_COUNT;
    int nedges = 0;
    if (!refuse) {
        bool bad_mp = false, bad_oct = false;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            bool has = false;
            if (i < n) {
                const int32_t m = c.mp_of_feat[i];
                if (m != -1) {
                    if (m < -1 || m >= nmp) {
                        bad_mp = true;
                    } else {
                        const int32_t o = c.keys[i].octave;
                        if (o < 0 || o >= nlevels) bad_oct = true;
                        else has = true;
                    }
                }
            }
            nedges += (int)__popcll(__ballot(has));
        }
        if (__ballot(bad_mp)) refuse |= ORBX_POSEOPT_REFUSED_MP_INDEX;
        if (__ballot(bad_oct)) refuse |= ORBX_POSEOPT_REFUSED_OCTAVE;
    }
    if (refuse) {
        copy_pose();
        if (lane == 0) {
            g.ngood[f] = 0;
            g.info[f] = refuse;
        }
        return;
    }
    // mvbOutlier[i] = false for every feature with a MapPoint (Optimizer.cc:295, :329)
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        if (i < n && c.mp_of_feat[i] >= 0) c.outlier[i] = 0;
    }
    if (nedges < 3) {
        copy_pose();
        if (lane == 0) {
            g.ngood[f] = 0;
            g.info[f] = ORBX_POSEOPT_FEW_EDGES;
        }
        return;
    }

    c.K = {(double)P->fx, (double)P->fy, (double)P->cx, (double)P->cy, (double)P->mbf};
    c.delta_mono = (double)(float)sq(5.991);
    c.delta_stereo = (double)(float)sq(7.815);

    // Converter::toSE3Quat(mTcw)
    Pose7 start;
    {
        double R[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i][j] = (double)P->Rcw[3 * i + j];
        se3_quat(R, start.qx, start.qy, start.qz, start.qw);
        start.tx = (double)P->tcw[0], start.ty = (double)P->tcw[1], start.tz = (double)P->tcw[2];
    }

    // behind the sums[28] at c.S:
    double* Am = c.S + 28;         // [36] + temp[6] + y[6]: the solver's copy
    double* xs = c.S + 28 + 48;    // [6] the solution (persists over the trials of an optimize) + 6 ints

    Pose7 est = start, err_pose = start;
    uint32_t iters = 0, trials = 0, flags = 0;
    int rounds = 0, nbad = 0;
    bool kernel = true;
    int nactive = nedges;
    for (int it = 0; it < 4; ++it) {
        est = start;
        // ---- optimize(10): nothing at level 0 -> returns at once
        if (nactive > 0)
            lm_optimize<6>(
                c.S, Am, xs, lane, 10, iters, trials, flags, ORBX_POSEOPT_NONPOSITIVE_SOLVE, est,
                [&](const Pose7& T) {
                    evaluate<true>(c, T, kernel);
                    err_pose = T;
                },
                [&](const Pose7& T) {
                    evaluate<false>(c, T, kernel);
                    err_pose = T;
                },
                [&](const double (&x)[6], Pose7& T) -> uint32_t {
                    return uniform(pose_update(x, T)) ? 0u : (uint32_t)ORBX_POSEOPT_THETA_LIMIT;
                });
        ++rounds;
        // ---- classification (Optimizer.cc:387-444): outliers are re-evaluated at the estimate,
        // the others keep the error of the last evaluated trial
        nbad = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            EdgeIn e;
            const bool has = load_edge<false>(c, i, e);
            bool bad = false;
            if (has) {
                double err[3], x, y, z;
                const float chi2 =
                    (float)edge_error(e, c.outlier[i] ? est : err_pose, c.K, err, x, y, z);
                bad = chi2 > (e.stereo ? 7.815f : 5.991f);
                c.outlier[i] = bad ? 1 : 0;
            }
            nbad += (int)__popcll(__ballot(bad));
        }
        nactive = nedges - nbad;
        if (it == 2) kernel = false;
        if (nedges < 10) break;
    }

    // Converter::toCvMat(SE3Quat) + Frame::SetPose: the quaternion's matrix, rounded to float,
    // then mOw = -mRcw.t() * mtcw
    if (lane == 0) {
        const double tx = 2.0 * est.qx, ty = 2.0 * est.qy, tz = 2.0 * est.qz;
        const double twx = tx * est.qw, twy = ty * est.qw, twz = tz * est.qw;
        const double txx = tx * est.qx, txy = ty * est.qx, txz = tz * est.qx;
        const double tyy = ty * est.qy, tyz = tz * est.qy, tzz = tz * est.qz;
        float R[9];
        R[0] = (float)(1.0 - (tyy + tzz)), R[1] = (float)(txy - twz), R[2] = (float)(txz + twy);
        R[3] = (float)(txy + twz), R[4] = (float)(1.0 - (txx + tzz)), R[5] = (float)(tyz - twx);
        R[6] = (float)(txz - twy), R[7] = (float)(tyz + twx), R[8] = (float)(1.0 - (txx + tyy));
        const float t[3] = {(float)est.tx, (float)est.ty, (float)est.tz};
#pragma unroll
        for (int k = 0; k < 9; ++k) Po->Rcw[k] = R[k];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            Po->tcw[r] = t[r];
            Po->Ow[r] = camera_centre_row(R, t, r);
        }
        g.ngood[f] = nedges - nbad;
        g.info[f] = (uint32_t)rounds | (iters << ORBX_POSEOPT_ITERS_SHIFT) |
                    (trials << ORBX_POSEOPT_TRIALS_SHIFT) | flags;
    }
}

// ---- the search's d_match[q] (feature of each MapPoint) as mvpMapPoints (MapPoint of each
// feature): ORBmatcher.cc:91, :1472 assign in query order, so the highest query index wins ----
// PRIOR = false: every feature of every job to -1, ahead of the scatter.  PRIOR = true, after
// it: a feature the scatter left at -1 takes the earlier search's MapPoint, so a new match
// overwrites an earlier one as an assignment after a copy would.
template <bool PRIOR>
__global__ __launch_bounds__(256) void k_match_fill(const int32_t* __restrict__ feat_off,
                                                    const int32_t* __restrict__ prior,
                                                    int32_t* __restrict__ mp_of_feat) {
    const int j = blockIdx.y;
    const int f0 = feat_off[j], n = feat_off[j + 1] - f0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (!PRIOR) mp_of_feat[f0 + i] = -1;
        else if (mp_of_feat[f0 + i] == -1) mp_of_feat[f0 + i] = prior[f0 + i];
    }
}

__global__ __launch_bounds__(256) void k_match_scatter(const int32_t* __restrict__ match,
                                                       const int32_t* __restrict__ q_off,
                                                       const int32_t* __restrict__ feat_off,
                                                       int32_t* __restrict__ mp_of_feat,
                                                       uint32_t* __restrict__ flagged) {
    const int j = blockIdx.y;
    const int q0 = q_off[j], nq = q_off[j + 1] - q0;
    const int f0 = feat_off[j], n = feat_off[j + 1] - f0;
    bool bad = false;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
        const int32_t i = match[q0 + q];
        if (i == -1) continue;
        if (i < 0 || i >= n) bad = true;
        else atomicMax(&mp_of_feat[f0 + i], q);
    }
    if (bad) atomicOr(flagged, 1u);
}

hipError_t launch_pose_opt(const PoseOptLaunch& a, hipStream_t st) {
    hipLaunchKernelGGL(k_pose_opt, dim3((a.nframes + PO_WAVES - 1) / PO_WAVES), dim3(64 * PO_WAVES),
                       0, st, a);
    return hipGetLastError();
}

}  // namespace

extern "C" {

orbx_status orbx_pose_optimization_batch_device(
    const orbx_frame_pose* d_poses, int32_t nframes, const orbx_keypoint* d_keys_un,
    const float* d_u_right, const int32_t* d_feat_off, int32_t max_feat,
    const int32_t* d_mp_of_feat, const orbx_map_point* d_mps, const int32_t* d_mp_off,
    orbx_frame_pose* d_poses_out, uint8_t* d_outlier, int32_t* d_ngood, uint32_t* d_info,
    void* stream) {
    if (nframes < 0 || nframes > 65535 || max_feat < 0 || max_feat > (int32_t)PO_MAX_FEAT)
        return ORBX_ERR_INVALID;
    if (nframes == 0) return ORBX_OK;
    if (!d_poses || !d_keys_un || !d_feat_off || !d_mp_of_feat || !d_mps || !d_mp_off ||
        !d_poses_out || !d_outlier || !d_ngood || !d_info)
        return ORBX_ERR_INVALID;
    int ndev = 0;
    if (!HIPOK(hipGetDeviceCount(&ndev)) || ndev < 1) return ORBX_ERR_DEVICE;
    PoseOptLaunch L{d_poses, nframes, d_keys_un, d_u_right, d_feat_off, max_feat, d_mp_of_feat,
                    d_mps, d_mp_off, d_poses_out, d_outlier, d_ngood, d_info};
    return HIPOK(launch_pose_opt(L, (hipStream_t)stream)) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_pose_optimization(const orbx_frame_pose* pose, const orbx_keypoint* keys_un,
                                   const float* u_right, int32_t n, const int32_t* mp_of_feat,
                                   const orbx_map_point* mps, int32_t nmp,
                                   orbx_frame_pose* pose_out, uint8_t* outlier, int32_t* ngood,
                                   uint32_t* info, int device) {
    if (!pose || !pose_out || !ngood || n < 0 || n > (int32_t)PO_MAX_FEAT || nmp < 0 ||
        (n > 0 && (!keys_un || !mp_of_feat || !outlier)) || (nmp > 0 && !mps))
        return ORBX_ERR_INVALID;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const int32_t idx[4] = {0, n, 0, nmp};   // feat_off[2], mp_off[2]
    const size_t mpb = sizeof(orbx_map_point) * (size_t)nmp;
    const size_t p_pose = p.in(pose, sizeof(*pose)), p_idx = p.in(idx, sizeof(idx)),
                 p_keys = p.in(keys_un, sizeof(orbx_keypoint) * (size_t)n),
                 p_ur = p.in_opt(u_right, 4 * (size_t)n), p_mpf = p.in(mp_of_feat, 4 * (size_t)n),
                 p_mps = p.in(nullptr, mpb + 256), p_out = p.inout(outlier, (size_t)n),
                 p_res = p.out(pose_out, sizeof(*pose_out), true), p_ngood = p.out(ngood, 4, true),
                 p_info = p.out(info, 4, true);   // the outputs start at zero on the device, as ever
    if (nmp) std::memcpy(p.host<uint8_t>(p_mps), mps, mpb);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    return c.finish(orbx_pose_optimization_batch_device(
        c.dev<orbx_frame_pose>(p_pose), 1, c.dev<orbx_keypoint>(p_keys), c.dev<float>(p_ur),
        c.dev<int32_t>(p_idx), n, c.dev<int32_t>(p_mpf), c.dev<orbx_map_point>(p_mps),
        c.dev<int32_t>(p_idx) + 2, c.dev<orbx_frame_pose>(p_res), c.dev<uint8_t>(p_out),
        c.dev<int32_t>(p_ngood), c.dev<uint32_t>(p_info), c.st()));
}

orbx_status orbx_matches_to_features_batch_device(const int32_t* d_match, const int32_t* d_q_off,
                                                  const int32_t* d_feat_off, int32_t njobs,
                                                  int32_t max_q, int32_t max_feat,
                                                  const int32_t* d_prior, int32_t* d_mp_of_feat,
                                                  uint32_t* d_flagged, void* stream) {
    if (njobs < 0 || njobs > 65535 || max_q < 0 || max_feat < 0 || max_feat > (int32_t)PO_MAX_FEAT)
        return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_match || !d_q_off || !d_feat_off || !d_mp_of_feat || !d_flagged) return ORBX_ERR_INVALID;
    int ndev = 0;
    if (!HIPOK(hipGetDeviceCount(&ndev)) || ndev < 1) return ORBX_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (!HIPOK(hipMemsetAsync(d_flagged, 0, 4, st))) return ORBX_ERR_DEVICE;
    if (max_feat == 0) return ORBX_OK;
    const dim3 fgrid((max_feat + 255) / 256, njobs);
    hipLaunchKernelGGL(k_match_fill<false>, fgrid, dim3(256), 0, st, d_feat_off, nullptr,
                       d_mp_of_feat);
    if (max_q > 0)
        hipLaunchKernelGGL(k_match_scatter, dim3((max_q + 255) / 256, njobs), dim3(256), 0, st,
                           d_match, d_q_off, d_feat_off, d_mp_of_feat, d_flagged);
    if (d_prior)
        hipLaunchKernelGGL(k_match_fill<true>, fgrid, dim3(256), 0, st, d_feat_off, d_prior,
                           d_mp_of_feat);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

}  // extern "C"
