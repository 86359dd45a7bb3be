// poseopt_ref.cpp — Optimizer::PoseOptimization (src/Optimizer.cc:245-457) restated in plain C++
// doubles: the CPU reference of orbx_pose_optimization*.  No liborbx and no GPU; its own
// quaternion, SE3 and LDLT; only orbx_sincos_f64 (orbx_math.h) is shared with the kernel.  Built
// with -ffp-contract=off: every operation is rounded on its own.
//
// The g2o pieces restated: one SE3 vertex, unary mono / stereo edges in feature order, Huber
// kernels, OptimizationAlgorithmLevenberg::solve with the dense 6x6 solver.  Forms evaluated
// inside Eigen (quaternion from a matrix, rotation of a vector, small products, the pivoted LDLT)
// are written from the published algorithms [unverified-Eigen].
//
//   poseopt_ref cases.bin results.bin     run every case of the file (layout: read_case below)
//   poseopt_ref --sincos in.bin out.bin   doubles in, (sin, cos) pairs out, through orbx_sincos_f64
//   poseopt_ref --time cases.bin          one thread, microseconds per frame on stdout
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx_frame.h"
#include "orbx_math.h"

namespace {

struct Quat { double x, y, z, w; };
struct Vec3 { double v[3]; };
struct Se3 { Quat r; Vec3 t; };

Quat quat_from_matrix(const double R[3][3]) {
    Quat q;
    double t = (R[0][0] + R[1][1]) + R[2][2];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (R[2][1] - R[1][2]) * t;
        q.y = (R[0][2] - R[2][0]) * t;
        q.z = (R[1][0] - R[0][1]) * t;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0);
        double c[3];
        c[i] = 0.5 * t;
        t = 0.5 / t;
        q.w = (R[k][j] - R[j][k]) * t;
        c[j] = (R[j][i] + R[i][j]) * t;
        c[k] = (R[k][i] + R[i][k]) * t;
        q.x = c[0], q.y = c[1], q.z = c[2];
    }
    return q;
}

Quat normalized(Quat q) {
    if (q.w < 0.0) q.x = -q.x, q.y = -q.y, q.z = -q.z, q.w = -q.w;
    const double n = std::sqrt(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
    return {q.x / n, q.y / n, q.z / n, q.w / n};
}

Vec3 rotate(const Quat& q, const Vec3& p) {
    double ux = q.y * p.v[2] - q.z * p.v[1];
    double uy = q.z * p.v[0] - q.x * p.v[2];
    double uz = q.x * p.v[1] - q.y * p.v[0];
    ux = ux + ux, uy = uy + uy, uz = uz + uz;
    const double cx = q.y * uz - q.z * uy;
    const double cy = q.z * ux - q.x * uz;
    const double cz = q.x * uy - q.y * ux;
    return {{(p.v[0] + q.w * ux) + cx, (p.v[1] + q.w * uy) + cy, (p.v[2] + q.w * uz) + cz}};
}

Quat mul(const Quat& a, const Quat& b) {
    Quat r;
    r.w = ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z;
    r.x = ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y;
    r.y = ((a.w * b.y + a.y * b.w) + a.z * b.x) - a.x * b.z;
    r.z = ((a.w * b.z + a.z * b.w) + a.x * b.y) - a.y * b.x;
    return r;
}

void rotation_matrix(const Quat& q, double R[3][3]) {
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0][0] = 1.0 - (tyy + tzz), R[0][1] = txy - twz, R[0][2] = txz + twy;
    R[1][0] = txy + twz, R[1][1] = 1.0 - (txx + tzz), R[1][2] = tyz - twx;
    R[2][0] = txz - twy, R[2][1] = tyz + twx, R[2][2] = 1.0 - (txx + tyy);
}

Vec3 se3_map(const Se3& T, const Vec3& p) {
    const Vec3 r = rotate(T.r, p);
    return {{r.v[0] + T.t.v[0], r.v[1] + T.t.v[1], r.v[2] + T.t.v[2]}};
}

void matmul3(const double A[3][3], const double B[3][3], double C[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j];
}

// SE3Quat::exp(update) * estimate with normalizeRotation; false: theta outside the sincos limit
bool se3_update(const double u[6], const Se3& est, Se3* out) {
    const double theta = std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    const double O[3][3] = {{0.0, -u[2], u[1]}, {u[2], 0.0, -u[0]}, {-u[1], u[0], 0.0}};
    double O2[3][3], R[3][3], V[3][3];
    matmul3(O, O, O2);
    if (theta < 0.00001) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
                V[i][j] = R[i][j];
            }
    } else {
        double s, c;
        if (!orbx::orbx_sincos_f64(theta, &s, &c)) return false;
        const double a = s / theta, b = (1.0 - c) / (theta * theta);
        const double d = (theta - s) / ((theta * theta) * theta);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double e = i == j ? 1.0 : 0.0;
                R[i][j] = (e + a * O[i][j]) + b * O2[i][j];
                V[i][j] = (e + b * O[i][j]) + d * O2[i][j];
            }
    }
    const Quat qe = normalized(quat_from_matrix(R));
    Vec3 te;
    for (int i = 0; i < 3; ++i) te.v[i] = (V[i][0] * u[3] + V[i][1] * u[4]) + V[i][2] * u[5];
    const Vec3 rt = rotate(qe, est.t);
    out->t = {{te.v[0] + rt.v[0], te.v[1] + rt.v[1], te.v[2] + rt.v[2]}};
    out->r = normalized(mul(qe, est.r));
    return true;
}

// Eigen::LDLT<MatrixXd> on the lower triangle, solve included [unverified-Eigen]
bool ldlt_solve(double A[6][6], const double b[6], double x[6]) {
    const int n = 6;
    int tr[6];
    int sign = 0;   // 0 zero, 1 positive semi-definite, -1 negative semi-definite, 2 indefinite
    for (int k = 0; k < n; ++k) {
        int idx = k;
        double best = std::fabs(A[k][k]);
        for (int i = k + 1; i < n; ++i)
            if (std::fabs(A[i][i]) > best) best = std::fabs(A[i][i]), idx = i;
        tr[k] = idx;
        if (idx != k) {
            for (int j = 0; j < k; ++j) std::swap(A[k][j], A[idx][j]);
            for (int i = idx + 1; i < n; ++i) std::swap(A[i][k], A[i][idx]);
            std::swap(A[k][k], A[idx][idx]);
            for (int i = k + 1; i < idx; ++i) std::swap(A[i][k], A[idx][i]);
        }
        if (k > 0) {
            double temp[6];
            for (int j = 0; j < k; ++j) temp[j] = A[j][j] * A[k][j];
            double s = A[k][0] * temp[0];
            for (int j = 1; j < k; ++j) s = s + A[k][j] * temp[j];
            A[k][k] = A[k][k] - s;
            for (int i = k + 1; i < n; ++i) {
                double si = A[i][0] * temp[0];
                for (int j = 1; j < k; ++j) si = si + A[i][j] * temp[j];
                A[i][k] = A[i][k] - si;
            }
        }
        const double akk = A[k][k];
        const bool valid = std::fabs(akk) > 0.0;
        if (k == 0 && !valid) {
            for (int j = 0; j < n; ++j) tr[j] = j;
            break;
        }
        if (valid)
            for (int i = k + 1; i < n; ++i) A[i][k] = A[i][k] / akk;
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
    double y[6];
    for (int i = 0; i < n; ++i) y[i] = b[i];
    for (int k = 0; k < n; ++k) std::swap(y[k], y[tr[k]]);
    for (int j = 0; j < n; ++j)
        for (int i = j + 1; i < n; ++i) y[i] = y[i] - A[i][j] * y[j];
    for (int i = 0; i < n; ++i) y[i] = std::fabs(A[i][i]) > DBL_MIN ? y[i] / A[i][i] : 0.0;
    for (int i = n - 2; i >= 0; --i) {
        double s = A[i + 1][i] * y[i + 1];
        for (int j = i + 2; j < n; ++j) s = s + A[j][i] * y[j];
        y[i] = y[i] - s;
    }
    for (int k = n - 1; k >= 0; --k) std::swap(y[k], y[tr[k]]);
    for (int i = 0; i < n; ++i) x[i] = y[i];
    return true;
}

struct Edge {
    int feat;
    bool stereo;
    double obs[3], info, xw[3];
    double err[3];
    int level;
    bool kernel;
};

struct Camera { double fx, fy, cx, cy, bf; };

void compute_error(Edge& e, const Se3& T, const Camera& K) {
    const Vec3 pc = se3_map(T, {{e.xw[0], e.xw[1], e.xw[2]}});
    if (e.stereo) {
        const float invz = (float)(1.0 / pc.v[2]);
        const double u = (pc.v[0] * invz) * K.fx + K.cx;
        const double v = (pc.v[1] * invz) * K.fy + K.cy;
        e.err[0] = e.obs[0] - u;
        e.err[1] = e.obs[1] - v;
        e.err[2] = e.obs[2] - (u - K.bf * invz);
    } else {
        e.err[0] = e.obs[0] - ((pc.v[0] / pc.v[2]) * K.fx + K.cx);
        e.err[1] = e.obs[1] - ((pc.v[1] / pc.v[2]) * K.fy + K.cy);
    }
}

double chi2_of(const Edge& e) {
    double c = e.err[0] * (e.info * e.err[0]) + e.err[1] * (e.info * e.err[1]);
    if (e.stereo) c = c + e.err[2] * (e.info * e.err[2]);
    return c;
}

void huber(double e2, double delta, double* rho0, double* rho1) {
    const double dsqr = delta * delta;
    if (e2 <= dsqr) {
        *rho0 = e2, *rho1 = 1.0;
    } else {
        const double sq = std::sqrt(e2);
        *rho0 = (2 * sq) * delta - dsqr;
        *rho1 = delta / sq;
    }
}

struct Optimizer {
    std::vector<Edge> edges;
    Camera K;
    Se3 est;
    double delta_mono, delta_stereo;
    double H[6][6], b[6], x[6], lambda, ni;
    int nbad_lm;
    uint32_t iters = 0, trials = 0, flags = 0;

    double active_chi2() {
        double chi = 0.0;
        for (Edge& e : edges) {
            if (e.level) continue;
            const double c = chi2_of(e);
            if (e.kernel) {
                double r0, r1;
                huber(c, e.stereo ? delta_stereo : delta_mono, &r0, &r1);
                chi = chi + r0;
            } else {
                chi = chi + c;
            }
        }
        return chi;
    }
    void active_errors() {
        for (Edge& e : edges)
            if (!e.level) compute_error(e, est, K);
    }
    void build() {
        for (int i = 0; i < 6; ++i) {
            b[i] = 0.0;
            for (int j = 0; j < 6; ++j) H[i][j] = 0.0;
        }
        for (Edge& e : edges) {
            if (e.level) continue;
            const Vec3 pc = se3_map(est, {{e.xw[0], e.xw[1], e.xw[2]}});
            const double X = pc.v[0], Y = pc.v[1], invz = 1.0 / pc.v[2], invz_2 = invz * invz;
            double A[3][6];
            A[0][0] = X * Y * invz_2 * K.fx;
            A[0][1] = -(1 + (X * X * invz_2)) * K.fx;
            A[0][2] = Y * invz * K.fx;
            A[0][3] = -invz * K.fx;
            A[0][4] = 0;
            A[0][5] = X * invz_2 * K.fx;
            A[1][0] = (1 + Y * Y * invz_2) * K.fy;
            A[1][1] = -X * Y * invz_2 * K.fy;
            A[1][2] = -X * invz * K.fy;
            A[1][3] = 0;
            A[1][4] = -invz * K.fy;
            A[1][5] = Y * invz_2 * K.fy;
            const int D = e.stereo ? 3 : 2;
            if (e.stereo) {
                A[2][0] = A[0][0] - K.bf * Y * invz_2;
                A[2][1] = A[0][1] + K.bf * X * invz_2;
                A[2][2] = A[0][2];
                A[2][3] = A[0][3];
                A[2][4] = 0;
                A[2][5] = A[0][5] - K.bf * invz_2;
            }
            double r0 = 0, r1 = 1.0;
            if (e.kernel) huber(chi2_of(e), e.stereo ? delta_stereo : delta_mono, &r0, &r1);
            const double w = e.kernel ? r1 * e.info : e.info;
            for (int i = 0; i < 6; ++i) {
                double tb = 0;
                for (int k = 0; k < D; ++k) {
                    const double p = e.kernel ? ((r1 * A[k][i]) * e.info) * e.err[k]
                                              : (A[k][i] * e.info) * e.err[k];
                    tb = k ? tb + p : p;
                }
                b[i] = b[i] - tb;
                for (int j = 0; j <= i; ++j) {
                    double th = 0;
                    for (int k = 0; k < D; ++k) {
                        const double p = (A[k][i] * w) * A[k][j];
                        th = k ? th + p : p;
                    }
                    H[i][j] = H[i][j] + th;
                }
            }
        }
    }
    // OptimizationAlgorithmLevenberg::solve; true: OK, false: Terminate
    bool solve(int iteration) {
        active_errors();
        double current = active_chi2(), temp = current;
        const double ini = current;
        build();
        if (iteration == 0) {
            double m = 0.0;
            for (int j = 0; j < 6; ++j) {
                const double a = std::fabs(H[j][j]);
                m = a < m ? m : a;
            }
            lambda = 1e-5 * m;
            ni = 2;
            nbad_lm = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const Se3 backup = est;
            double A[6][6];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) A[i][j] = j <= i ? H[i][j] : 0.0;
            for (int j = 0; j < 6; ++j) A[j][j] = H[j][j] + lambda;
            bool ok2 = ldlt_solve(A, b, x);
            if (!ok2) flags |= 1u << 29;
            ++trials;
            Se3 next;
            bool theta_ok = se3_update(x, est, &next);
            if (theta_ok) {
                est = next;
                active_errors();
                temp = active_chi2();
            } else {
                flags |= 1u << 28;
                ok2 = false;
            }
            if (!ok2) temp = DBL_MAX;
            rho = current - temp;
            double scale = 0.0;
            for (int j = 0; j < 6; ++j) scale = scale + x[j] * (lambda * x[j] + b[j]);
            scale = scale + 1e-3;
            rho = rho / scale;
            if (rho > 0 && std::isfinite(temp)) {
                const double t = 2 * rho - 1;
                double alpha = 1. - (t * t) * t;
                const double up = 2. / 3., lo = 1. / 3.;
                alpha = up < alpha ? up : alpha;
                const double f = lo < alpha ? alpha : lo;
                lambda = lambda * f;
                ni = 2;
                current = temp;
            } else {
                lambda = lambda * ni;
                ni = ni * 2;
                est = backup;
            }
            ++qmax;
        } while (rho < 0 && qmax < 10);
        if (qmax == 10 || rho == 0) return false;
        if ((ini - current) * 1e3 < ini) ++nbad_lm;
        else nbad_lm = 0;
        return nbad_lm < 3;
    }
    void optimize(int iterations) {
        bool any = false;
        for (const Edge& e : edges) any = any || !e.level;
        if (!any) return;
        for (int j = 0; j < 6; ++j) x[j] = 0.0;
        for (int i = 0; i < iterations; ++i) {
            ++iters;
            if (!solve(i)) break;
        }
    }
};

enum : uint32_t {
    F_MP_RANGE = 1u << 24, F_OCTAVE = 1u << 25, F_NLEVELS = 1u << 26, F_COUNT = 1u << 27,
    F_FEW = 1u << 30
};

struct Case {
    orbx_frame_pose pose;
    int32_t n, nmp, has_ur, max_feat;
    std::vector<orbx_keypoint> keys;
    std::vector<float> ur;
    std::vector<int32_t> mp_of_feat;
    std::vector<orbx_map_point> mps;
    std::vector<uint8_t> outlier;
};

void run_case(Case& c, orbx_frame_pose* out, int32_t* ngood, uint32_t* info) {
    *out = c.pose;
    *ngood = 0;
    *info = 0;
    uint32_t refuse = 0;
    if (c.pose.nlevels < 1 || c.pose.nlevels > 16) refuse |= F_NLEVELS;
    if (c.n > c.max_feat) refuse |= F_COUNT;
    if (!refuse)
        for (int i = 0; i < c.n; ++i) {
            const int32_t m = c.mp_of_feat[i];
            if (m == -1) continue;
            if (m < -1 || m >= c.nmp) refuse |= F_MP_RANGE;
            else if (c.keys[i].octave < 0 || c.keys[i].octave >= c.pose.nlevels) refuse |= F_OCTAVE;
        }
    if (refuse) {
        *info = refuse;
        return;
    }
    Optimizer o;
    o.K = {c.pose.fx, c.pose.fy, c.pose.cx, c.pose.cy, c.pose.mbf};
    o.delta_mono = (float)std::sqrt(5.991);
    o.delta_stereo = (float)std::sqrt(7.815);
    for (int i = 0; i < c.n; ++i) {
        const int32_t m = c.mp_of_feat[i];
        if (m < 0) continue;
        c.outlier[i] = 0;
        Edge e{};
        e.feat = i;
        e.stereo = c.has_ur && !(c.ur[i] < 0);
        e.obs[0] = c.keys[i].x, e.obs[1] = c.keys[i].y, e.obs[2] = e.stereo ? c.ur[i] : 0.0;
        const float s = c.pose.scale[c.keys[i].octave];
        const float inv_sigma2 = 1.0f / (s * s);
        e.info = inv_sigma2;
        for (int k = 0; k < 3; ++k) e.xw[k] = c.mps[m].pos[k];
        e.level = 0;
        e.kernel = true;
        o.edges.push_back(e);
    }
    const int nedges = (int)o.edges.size();
    if (nedges < 3) {
        *info = F_FEW;
        return;
    }
    double R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = c.pose.Rcw[3 * i + j];
    Se3 start;
    start.r = normalized(quat_from_matrix(R));
    start.t = {{c.pose.tcw[0], c.pose.tcw[1], c.pose.tcw[2]}};
    o.est = start;
    int nbad = 0, rounds = 0;
    for (int it = 0; it < 4; ++it) {
        o.est = start;
        o.optimize(10);
        ++rounds;
        nbad = 0;
        for (Edge& e : o.edges) {
            if (c.outlier[e.feat]) compute_error(e, o.est, o.K);
            const float chi2 = (float)chi2_of(e);
            if (chi2 > (e.stereo ? 7.815f : 5.991f)) {
                c.outlier[e.feat] = 1;
                e.level = 1;
                ++nbad;
            } else {
                c.outlier[e.feat] = 0;
                e.level = 0;
            }
            if (it == 2) e.kernel = false;
        }
        if (nedges < 10) break;
    }
    double Ro[3][3];
    rotation_matrix(o.est.r, Ro);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out->Rcw[3 * i + j] = (float)Ro[i][j];
        out->tcw[i] = (float)o.est.t.v[i];
    }
    for (int r = 0; r < 3; ++r) {
        float s = out->Rcw[r] * out->tcw[0];
        s = s + out->Rcw[3 + r] * out->tcw[1];
        s = s + out->Rcw[6 + r] * out->tcw[2];
        out->Ow[r] = -s;
    }
    *ngood = nedges - nbad;
    *info = (uint32_t)rounds | (o.iters << 3) | (o.trials << 10) | o.flags;
}

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

// file: int32 ncases, then per case: orbx_frame_pose, int32 n, nmp, has_ur, max_feat,
// orbx_keypoint[n], float u_right[n] (if has_ur), int32 mp_of_feat[n], orbx_map_point[nmp],
// uint8 outlier[n] (the flags before the call)
bool read_case(FILE* f, Case* c) {
    int32_t h[4];
    if (!read_exact(f, &c->pose, sizeof(c->pose)) || !read_exact(f, h, sizeof(h))) return false;
    c->n = h[0], c->nmp = h[1], c->has_ur = h[2], c->max_feat = h[3];
    if (c->n < 0 || c->nmp < 0) return false;
    c->keys.resize(c->n);
    c->ur.resize(c->has_ur ? c->n : 0);
    c->mp_of_feat.resize(c->n);
    c->mps.resize(c->nmp);
    c->outlier.resize(c->n);
    return read_exact(f, c->keys.data(), sizeof(orbx_keypoint) * c->n) &&
           read_exact(f, c->ur.data(), 4 * c->ur.size()) &&
           read_exact(f, c->mp_of_feat.data(), 4 * (size_t)c->n) &&
           read_exact(f, c->mps.data(), sizeof(orbx_map_point) * c->nmp) &&
           read_exact(f, c->outlier.data(), c->n);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "--sincos")) {
        FILE* in = std::fopen(argv[2], "rb");
        FILE* out = std::fopen(argv[3], "wb");
        if (!in || !out) return 2;
        double v;
        while (std::fread(&v, 8, 1, in) == 1) {
            double sc[2] = {NAN, NAN};
            orbx::orbx_sincos_f64(v, &sc[0], &sc[1]);
            std::fwrite(sc, 8, 2, out);
        }
        std::fclose(in);
        return std::fclose(out) ? 2 : 0;
    }
    const bool timing = argc == 3 && !std::strcmp(argv[1], "--time");
    if (!timing && argc != 3) {
        std::fprintf(stderr, "usage: poseopt_ref cases.bin results.bin | --sincos in out | --time cases.bin\n");
        return 2;
    }
    FILE* in = std::fopen(argv[timing ? 2 : 1], "rb");
    if (!in) return 2;
    int32_t ncases = 0;
    if (!read_exact(in, &ncases, 4) || ncases < 0) return 2;
    std::vector<Case> cases((size_t)ncases);
    for (Case& c : cases)
        if (!read_case(in, &c)) return 2;
    std::fclose(in);
    FILE* out = timing ? nullptr : std::fopen(argv[2], "wb");
    if (!timing && !out) return 2;
    const auto t0 = std::chrono::steady_clock::now();
    for (Case& c : cases) {
        orbx_frame_pose po;
        int32_t ngood;
        uint32_t info;
        run_case(c, &po, &ngood, &info);
        if (out) {
            std::fwrite(&po, sizeof(po), 1, out);
            std::fwrite(&ngood, 4, 1, out);
            std::fwrite(&info, 4, 1, out);
            std::fwrite(c.outlier.data(), 1, c.outlier.size(), out);
        }
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (timing) std::printf("%.3f\n", ncases ? us / ncases : 0.0);
    return out && std::fclose(out) ? 2 : 0;
}
