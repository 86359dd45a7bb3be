// sim3opt_ref.cpp — Optimizer::OptimizeSim3 (src/Optimizer.cc:1070-1265) restated in plain C++
// the way g2o runs it: a vertex with an estimate and a backup stack, edge objects that keep their
// _error, a numeric linearizeOplus that perturbs the vertex through oplus / push / pop edge by
// edge (base_binary_edge.hpp:131-200), constructQuadraticForm into the vertex's H and b, and
// OptimizationAlgorithmLevenberg::solve over a dense LDLT.  It is the second, independent CPU
// restatement that tests/sim3opt_cases.py is compared with bit for bit; it shares only
// orbx_sincos_f64 / orbx_exp_f64 (csrc/orbx_math.h) and the record layouts of include/ with the
// kernel.  No liborbx, no GPU.  Forms evaluated inside Eigen are restated from the published
// algorithms [unverified-Eigen].  Built with -ffp-contract=off.
//
//   sim3opt_ref cases.bin results.bin     every case of the file (tests/sim3opt_cases.write_cases)
//   sim3opt_ref --exp in.bin out.bin      orbx_exp_f64 of every double of in.bin (NaN: refused)
//   sim3opt_ref --time cases.bin          microseconds per case, one thread
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx_frame.h"
#include "orbx_match.h"
#include "orbx_math.h"

namespace {

struct V3 { double v[3]; };
struct Quat { double x, y, z, w; };

Quat quat_of(const double R[3][3]) {
    Quat q;
    double t = (R[0][0] + R[1][1]) + R[2][2];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (R[2][1] - R[1][2]) * t;
        q.y = (R[0][2] - R[2][0]) * t;
        q.z = (R[1][0] - R[0][1]) * t;
        return q;
    }
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
    return q;
}

V3 rot(const Quat& q, const V3& p) {
    double ux = q.y * p.v[2] - q.z * p.v[1], uy = q.z * p.v[0] - q.x * p.v[2],
           uz = q.x * p.v[1] - q.y * p.v[0];
    ux = ux + ux, uy = uy + uy, uz = uz + uz;
    const double cx = q.y * uz - q.z * uy, cy = q.z * ux - q.x * uz, cz = q.x * uy - q.y * ux;
    return V3{{(p.v[0] + q.w * ux) + cx, (p.v[1] + q.w * uy) + cy, (p.v[2] + q.w * uz) + cz}};
}

Quat qmul(const Quat& a, const Quat& b) {
    Quat r;
    r.w = ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z;
    r.x = ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y;
    r.y = ((a.w * b.y + a.y * b.w) + a.z * b.x) - a.x * b.z;
    r.z = ((a.w * b.z + a.z * b.w) + a.x * b.y) - a.y * b.x;
    return r;
}

// g2o::Sim3
struct Sim3 {
    Quat r{0, 0, 0, 1};
    V3 t{{0, 0, 0}};
    double s = 1.0;

    V3 map(const V3& p) const {
        const V3 q = rot(r, p);
        return V3{{s * q.v[0] + t.v[0], s * q.v[1] + t.v[1], s * q.v[2] + t.v[2]}};
    }
    Sim3 inverse() const {
        Sim3 i;
        i.r = Quat{-r.x, -r.y, -r.z, r.w};
        const double m = -1. / s;
        i.t = rot(i.r, V3{{m * t.v[0], m * t.v[1], m * t.v[2]}});
        i.s = 1. / s;
        return i;
    }
    Sim3 operator*(const Sim3& o) const {
        Sim3 n;
        n.r = qmul(r, o.r);
        const V3 q = rot(r, o.t);
        n.t = V3{{s * q.v[0] + t.v[0], s * q.v[1] + t.v[1], s * q.v[2] + t.v[2]}};
        n.s = s * o.s;
        return n;
    }
};

constexpr uint32_t F_THETA = ORBX_SIM3OPT_THETA_LIMIT, F_EXP = ORBX_SIM3OPT_EXP_LIMIT;

// Sim3(const Vector7d& update); 0 or the flag of the routine that refused
uint32_t sim3_exp(const double* u, Sim3* out) {
    const double omega[3] = {u[0], u[1], u[2]}, upsilon[3] = {u[3], u[4], u[5]};
    const double sigma = u[6];
    const double theta = std::sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2]);
    const double Om[3][3] = {{0.0, -omega[2], omega[1]}, {omega[2], 0.0, -omega[0]},
                             {-omega[1], omega[0], 0.0}};
    double Om2[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Om2[i][j] = (Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j]) + Om[i][2] * Om[2][j];
    double s;
    if (!orbx::orbx_exp_f64(sigma, &s)) return F_EXP;
    const double eps = 0.00001;
    double A, B, C, R[3][3];
    double sn = 0, cs = 1;
    const bool small_theta = theta < eps;
    if (!small_theta && !orbx::orbx_sincos_f64(theta, &sn, &cs)) return F_THETA;
    auto rodrigues = [&]() {
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                R[i][j] = ((i == j ? 1.0 : 0.0) + a * Om[i][j]) + b * Om2[i][j];
    };
    auto first_order = [&]() {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] = ((i == j ? 1.0 : 0.0) + Om[i][j]) + Om2[i][j];
    };
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (small_theta) {
            A = 1. / 2.;
            B = 1. / 6.;
            first_order();
        } else {
            const double theta2 = theta * theta;
            A = (1 - cs) / (theta2);
            B = (theta - sn) / (theta2 * theta);
            rodrigues();
        }
    } else {
        C = (s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
            first_order();
        } else {
            rodrigues();
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    out->r = quat_of(R);
    for (int i = 0; i < 3; ++i) {
        double W[3];
        for (int j = 0; j < 3; ++j) W[j] = (A * Om[i][j] + B * Om2[i][j]) + C * (i == j ? 1.0 : 0.0);
        out->t.v[i] = (W[0] * upsilon[0] + W[1] * upsilon[1]) + W[2] * upsilon[2];
    }
    out->s = s;
    return 0;
}

// VertexSim3Expmap
struct Vertex {
    Sim3 estimate;
    std::vector<Sim3> backup;
    bool fix_scale = false;
    double fl1[2], pp1[2], fl2[2], pp2[2];
    double H[7][7], b[7];

    void push() { backup.push_back(estimate); }
    void pop() {
        estimate = backup.back();
        backup.pop_back();
    }
    void discard_top() { backup.pop_back(); }
    // oplusImpl writes into the caller's update
    uint32_t oplus(double* update) {
        if (fix_scale) update[6] = 0;
        Sim3 s;
        const uint32_t why = sim3_exp(update, &s);
        if (why) return why;
        estimate = s * estimate;
        return 0;
    }
    void clear_quadratic_form() {
        for (int i = 0; i < 7; ++i) {
            b[i] = 0.0;
            for (int j = 0; j < 7; ++j) H[i][j] = 0.0;
        }
    }
};

// EdgeSim3ProjectXYZ (inverse = false) / EdgeInverseSim3ProjectXYZ (inverse = true)
struct Edge {
    bool inverse;
    V3 point;           // the fixed VertexSBAPointXYZ
    double obs[2];
    double info;        // information = info * I
    double delta;       // the Huber kernel's
    double error[2];
    double J[2][7];
    int pair;

    void compute_error(const Vertex& v) {
        const V3 p = inverse ? v.estimate.inverse().map(point) : v.estimate.map(point);
        const double* fl = inverse ? v.fl2 : v.fl1;
        const double* pp = inverse ? v.pp2 : v.pp1;
        const double px = p.v[0] / p.v[2], py = p.v[1] / p.v[2];
        error[0] = obs[0] - (px * fl[0] + pp[0]);
        error[1] = obs[1] - (py * fl[1] + pp[1]);
    }
    double chi2() const { return error[0] * (info * error[0]) + error[1] * (info * error[1]); }
    void robustify(double e2, double* rho) const {
        const double dsqr = delta * delta;
        if (e2 <= dsqr) {
            rho[0] = e2;
            rho[1] = 1.;
        } else {
            const double sqrte = std::sqrt(e2);
            rho[0] = 2 * sqrte * delta - dsqr;
            rho[1] = delta / sqrte;
        }
    }
    void linearize_oplus(Vertex& v) {
        const double delta_ = 1e-9;
        const double scalar = 1.0 / (2 * delta_);
        const double before[2] = {error[0], error[1]};
        double add[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int d = 0; d < 7; ++d) {
            v.push();
            add[d] = delta_;
            v.oplus(add);
            compute_error(v);
            double bak[2] = {error[0], error[1]};
            v.pop();
            v.push();
            add[d] = -delta_;
            v.oplus(add);
            compute_error(v);
            bak[0] -= error[0];
            bak[1] -= error[1];
            v.pop();
            add[d] = 0.0;
            J[0][d] = scalar * bak[0];
            J[1][d] = scalar * bak[1];
        }
        error[0] = before[0], error[1] = before[1];
    }
    void construct_quadratic_form(Vertex& v) const {
        double omega_r[2] = {(-info) * error[0], (-info) * error[1]};
        double rho[2];
        robustify(chi2(), rho);
        const double w = rho[1] * info;
        omega_r[0] *= rho[1];
        omega_r[1] *= rho[1];
        for (int i = 0; i < 7; ++i) {
            v.b[i] += J[0][i] * omega_r[0] + J[1][i] * omega_r[1];
            for (int j = 0; j <= i; ++j) v.H[i][j] += (J[0][i] * w) * J[0][j] + (J[1][i] * w) * J[1][j];
        }
    }
};

// Eigen::LDLT<MatrixXd> in place on the lower triangle, with its transpositions and sign
struct Ldlt {
    static constexpr int N = 7;
    double m[N][N];
    int tr[N];
    bool positive = true;

    void compute() {
        int sign = 0;   // ZeroSign
        for (int k = 0; k < N; ++k) {
            int piv = k;
            double big = std::fabs(m[k][k]);
            for (int i = k + 1; i < N; ++i)
                if (std::fabs(m[i][i]) > big) big = std::fabs(m[i][i]), piv = i;
            tr[k] = piv;
            if (piv != k) {
                for (int j = 0; j < k; ++j) std::swap(m[k][j], m[piv][j]);
                for (int i = piv + 1; i < N; ++i) std::swap(m[i][k], m[i][piv]);
                std::swap(m[k][k], m[piv][piv]);
                for (int i = k + 1; i < piv; ++i) std::swap(m[i][k], m[piv][i]);
            }
            if (k > 0) {
                double temp[N];
                for (int j = 0; j < k; ++j) temp[j] = m[j][j] * m[k][j];
                double s = m[k][0] * temp[0];
                for (int j = 1; j < k; ++j) s = s + m[k][j] * temp[j];
                m[k][k] = m[k][k] - s;
                for (int i = k + 1; i < N; ++i) {
                    double si = m[i][0] * temp[0];
                    for (int j = 1; j < k; ++j) si = si + m[i][j] * temp[j];
                    m[i][k] = m[i][k] - si;
                }
            }
            const double d = m[k][k];
            const bool usable = std::fabs(d) > 0.0;
            if (k == 0 && !usable) {
                for (int j = 0; j < N; ++j) tr[j] = j;
                break;
            }
            if (usable)
                for (int i = k + 1; i < N; ++i) m[i][k] = m[i][k] / d;
            if (sign == 1 && d < 0.0) sign = 2;
            else if (sign == -1 && d > 0.0) sign = 2;
            else if (sign == 0) sign = d > 0.0 ? 1 : d < 0.0 ? -1 : 0;
        }
        positive = sign == 1 || sign == 0;
    }
    void solve(const double* b, double* x) const {
        double y[N];
        for (int i = 0; i < N; ++i) y[i] = b[i];
        for (int k = 0; k < N; ++k) std::swap(y[k], y[tr[k]]);
        for (int j = 0; j < N; ++j)
            for (int i = j + 1; i < N; ++i) y[i] = y[i] - m[i][j] * y[j];
        for (int i = 0; i < N; ++i) y[i] = std::fabs(m[i][i]) > DBL_MIN ? y[i] / m[i][i] : 0.0;
        for (int i = N - 2; i >= 0; --i) {
            double s = m[i + 1][i] * y[i + 1];
            for (int j = i + 2; j < N; ++j) s = s + m[j][i] * y[j];
            y[i] = y[i] - s;
        }
        for (int k = N - 1; k >= 0; --k) std::swap(y[k], y[tr[k]]);
        for (int i = 0; i < N; ++i) x[i] = y[i];
    }
};

struct Optimizer {
    Vertex v;
    std::vector<Edge> edges;          // e12_0, e21_0, e12_1, e21_1, ...
    std::vector<char> removed;        // per edge
    std::vector<Edge*> active;
    uint32_t iters = 0, trials = 0, flags = 0;
    double x[7];

    void initialize() {
        active.clear();
        for (size_t k = 0; k < edges.size(); ++k)
            if (!removed[k]) active.push_back(&edges[k]);
    }
    void compute_active_errors() {
        for (Edge* e : active) e->compute_error(v);
    }
    double active_robust_chi2() const {
        double chi = 0.0;
        for (const Edge* e : active) {
            double rho[2];
            e->robustify(e->chi2(), rho);
            chi += rho[0];
        }
        return chi;
    }
    void build_system() {
        v.clear_quadratic_form();
        for (Edge* e : active) e->linearize_oplus(v);
        for (Edge* e : active) e->construct_quadratic_form(v);
    }
    // SparseOptimizer::optimize(n) with OptimizationAlgorithmLevenberg::solve
    void optimize(int n) {
        if (active.empty()) return;
        for (double& d : x) d = 0.0;
        double lambda = 0, ni = 2;
        int n_bad = 0;
        for (int iteration = 0; iteration < n; ++iteration) {
            ++iters;
            compute_active_errors();
            double current = active_robust_chi2(), temp = current;
            const double ini = current;
            build_system();
            if (iteration == 0) {
                double max_diag = 0;
                for (int j = 0; j < 7; ++j) max_diag = std::max(std::fabs(v.H[j][j]), max_diag);
                lambda = 1e-5 * max_diag;
                ni = 2;
                n_bad = 0;
            }
            double rho = 0;
            int qmax = 0;
            do {
                v.push();
                Ldlt l;
                for (int i = 0; i < 7; ++i)
                    for (int j = 0; j < 7; ++j)
                        l.m[i][j] = j < i ? v.H[i][j] : j == i ? v.H[i][i] + lambda : 0.0;
                l.compute();
                bool ok2 = l.positive;
                if (ok2) l.solve(v.b, x);
                else flags |= ORBX_SIM3OPT_NONPOSITIVE_SOLVE;
                ++trials;
                const uint32_t why = v.oplus(x);
                if (!why) {
                    compute_active_errors();
                    temp = active_robust_chi2();
                } else {
                    flags |= why;
                    ok2 = false;
                }
                if (!ok2) temp = DBL_MAX;
                rho = current - temp;
                double scale = 0;
                for (int j = 0; j < 7; ++j) scale += x[j] * (lambda * x[j] + v.b[j]);
                scale += 1e-3;
                rho /= scale;
                if (rho > 0 && std::isfinite(temp)) {
                    const double tr = 2 * rho - 1;
                    double alpha = 1. - (tr * tr) * tr;   // pow(2 * rho - 1, 3) as the kernel forms it
                    alpha = std::min(alpha, 2. / 3.);
                    const double factor = std::max(alpha, 1. / 3.);
                    lambda *= factor;
                    ni = 2;
                    current = temp;
                    v.discard_top();
                } else {
                    lambda *= ni;
                    ni *= 2;
                    v.pop();
                }
                ++qmax;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0) return;
            if ((ini - current) * 1e3 < ini) ++n_bad;
            else n_bad = 0;
            if (n_bad >= 3) return;
        }
    }
};

struct Case {
    orbx_frame_pose pose1, pose2;
    orbx_sim3opt_job job;
    orbx_sim3opt_in in;
    int32_t max_n, out_of_range;
    std::vector<orbx_sim3opt_corr> corr;
    std::vector<uint8_t> keep;
};

float row3f(const float* R, int r, const float* X) {
    float t = R[3 * r] * X[0];
    t = t + R[3 * r + 1] * X[1];
    return t + R[3 * r + 2] * X[2];
}

void write_result(const Sim3& S, int n_in, int n_corr, int n_bad, uint32_t info,
                  orbx_sim3opt_result* r) {
    std::memset(r, 0, sizeof(*r));
    r->n_inliers = n_in, r->n_correspondences = n_corr, r->n_bad = n_bad, r->info = info;
    r->q[0] = S.r.x, r->q[1] = S.r.y, r->q[2] = S.r.z, r->q[3] = S.r.w;
    for (int k = 0; k < 3; ++k) r->t[k] = S.t.v[k];
    r->s = S.s;
    // Converter::toCvMat(g2o::Sim3): s * toRotationMatrix(), t
    const Quat& q = S.r;
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    const double R[3][3] = {{1 - (tyy + tzz), txy - twz, txz + twy},
                            {txy + twz, 1 - (txx + tzz), tyz - twx},
                            {txz - twy, tyz + twx, 1 - (txx + tyy)}};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) r->T12[4 * i + j] = (float)(S.s * R[i][j]);
        r->T12[4 * i + 3] = (float)S.t.v[i];
    }
    r->T12[15] = 1.0f;
}

void run_case(Case& c, orbx_sim3opt_result* res) {
    const orbx_sim3opt_job& J = c.job;
    const int N = J.N;
    // g2o::Sim3(toMatrix3d(R12), toVector3d(t12), s12)
    Sim3 start;
    {
        double R[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i][j] = c.in.R12[3 * i + j];
        start.r = quat_of(R);
        start.t = V3{{c.in.t12[0], c.in.t12[1], c.in.t12[2]}};
        start.s = c.in.s12;
    }
    uint32_t refuse = 0;
    if (J.nlevels1 < 1 || J.nlevels1 > 16 || J.nlevels2 < 1 || J.nlevels2 > 16)
        refuse |= ORBX_SIM3OPT_REFUSED_OCTAVE;
    if (N > c.max_n) refuse |= ORBX_SIM3OPT_REFUSED_LIMIT;
    if (c.out_of_range) refuse |= ORBX_SIM3OPT_REFUSED_RANGE;
    if (!refuse) {
        for (int i = 0; i < N; ++i) {
            const orbx_sim3opt_corr& q = c.corr[i];
            if (q.octave1 < 0 || q.octave1 >= J.nlevels1 || q.octave2 < 0 || q.octave2 >= J.nlevels2)
                refuse |= ORBX_SIM3OPT_REFUSED_OCTAVE;
            if (q.i1 < 0 || q.i1 >= J.mN1 || (i > 0 && c.corr[i - 1].i1 >= q.i1))
                refuse |= ORBX_SIM3OPT_REFUSED_I1;
        }
    }
    if (refuse) {
        write_result(start, 0, 0, 0, refuse, res);
        return;
    }
    Optimizer o;
    o.v.fix_scale = J.fix_scale != 0;
    o.v.estimate = start;
    o.v.fl1[0] = c.pose1.fx, o.v.fl1[1] = c.pose1.fy, o.v.pp1[0] = c.pose1.cx, o.v.pp1[1] = c.pose1.cy;
    o.v.fl2[0] = c.pose2.fx, o.v.fl2[1] = c.pose2.fy, o.v.pp2[0] = c.pose2.cx, o.v.pp2[1] = c.pose2.cy;
    const float th2 = J.th2;
    const float deltaHuber = std::sqrt(th2);
    for (int i = 0; i < N; ++i) {
        const orbx_sim3opt_corr& q = c.corr[i];
        float P1[3], P2[3];
        for (int r = 0; r < 3; ++r) {
            P1[r] = (float)((double)row3f(c.pose1.Rcw, r, q.X1w) + (double)c.pose1.tcw[r]);
            P2[r] = (float)((double)row3f(c.pose2.Rcw, r, q.X2w) + (double)c.pose2.tcw[r]);
        }
        Edge e12{}, e21{};
        e12.inverse = false;
        e12.point = V3{{P2[0], P2[1], P2[2]}};
        e12.obs[0] = q.kp1[0], e12.obs[1] = q.kp1[1];
        const float inv1 = 1.0f / J.sigma2_1[q.octave1];
        e12.info = inv1;
        e21.inverse = true;
        e21.point = V3{{P1[0], P1[1], P1[2]}};
        e21.obs[0] = q.kp2[0], e21.obs[1] = q.kp2[1];
        const float inv2 = 1.0f / J.sigma2_2[q.octave2];
        e21.info = inv2;
        e12.delta = e21.delta = deltaHuber;
        e12.pair = e21.pair = i;
        o.edges.push_back(e12);
        o.edges.push_back(e21);
    }
    o.removed.assign(o.edges.size(), 0);
    int rounds = 0;
    o.initialize();
    if (N > 0) {
        o.optimize(5);
        ++rounds;
    }
    int nBad = 0;
    for (int i = 0; i < N; ++i) {
        const Edge &e12 = o.edges[2 * i], &e21 = o.edges[2 * i + 1];
        if (e12.chi2() > th2 || e21.chi2() > th2) {
            c.keep[c.corr[i].i1] = 0;
            o.removed[2 * i] = o.removed[2 * i + 1] = 1;
            ++nBad;
        }
    }
    if (nBad > 0) o.flags |= ORBX_SIM3OPT_DROPPED;
    const int nMoreIterations = nBad > 0 ? 10 : 5;
    if (N - nBad < 10) {
        o.flags |= ORBX_SIM3OPT_FEW_INLIERS;
        write_result(start, 0, N, nBad, (uint32_t)rounds | (o.iters << 3) | (o.trials << 10) | o.flags,
                     res);
        return;
    }
    o.initialize();
    o.optimize(nMoreIterations);
    ++rounds;
    int nIn = 0;
    for (int i = 0; i < N; ++i) {
        if (o.removed[2 * i]) continue;
        if (o.edges[2 * i].chi2() > th2 || o.edges[2 * i + 1].chi2() > th2) c.keep[c.corr[i].i1] = 0;
        else ++nIn;
    }
    write_result(o.v.estimate, nIn, N, nBad,
                 (uint32_t)rounds | (o.iters << 3) | (o.trials << 10) | o.flags, res);
}

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

// file: int32 ncases, then per case: orbx_frame_pose x 2, orbx_sim3opt_job, orbx_sim3opt_in,
// int32 max_n, out_of_range, orbx_sim3opt_corr[N], uint8 keep[mN1] (the bytes before the call)
bool read_case(FILE* f, Case* c) {
    int32_t h[2];
    if (!read_exact(f, &c->pose1, sizeof(c->pose1)) || !read_exact(f, &c->pose2, sizeof(c->pose2)) ||
        !read_exact(f, &c->job, sizeof(c->job)) || !read_exact(f, &c->in, sizeof(c->in)) ||
        !read_exact(f, h, sizeof(h)))
        return false;
    c->max_n = h[0], c->out_of_range = h[1];
    if (c->job.N < 0 || c->job.N > (1 << 20) || c->job.mN1 < 0 || c->job.mN1 > (1 << 24)) return false;
    c->corr.resize(c->job.N);
    c->keep.resize(c->job.mN1);
    return read_exact(f, c->corr.data(), sizeof(orbx_sim3opt_corr) * c->corr.size()) &&
           read_exact(f, c->keep.data(), c->keep.size());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "--exp")) {
        FILE* in = std::fopen(argv[2], "rb");
        FILE* out = std::fopen(argv[3], "wb");
        if (!in || !out) return 2;
        double v;
        while (std::fread(&v, 8, 1, in) == 1) {
            double e = NAN;
            orbx::orbx_exp_f64(v, &e);
            std::fwrite(&e, 8, 1, out);
        }
        std::fclose(in);
        return std::fclose(out) ? 2 : 0;
    }
    const bool timing = argc == 3 && !std::strcmp(argv[1], "--time");
    if (!timing && argc != 3) {
        std::fprintf(stderr, "usage: sim3opt_ref cases.bin results.bin | --exp in out | --time cases.bin\n");
        return 2;
    }
    FILE* in = std::fopen(argv[timing ? 2 : 1], "rb");
    if (!in) return 2;
    int32_t ncases = 0;
    if (!read_exact(in, &ncases, 4) || ncases < 0 || ncases > (1 << 20)) return 2;
    std::vector<Case> cases((size_t)ncases);
    for (Case& c : cases)
        if (!read_case(in, &c)) return 2;
    std::fclose(in);
    FILE* out = timing ? nullptr : std::fopen(argv[2], "wb");
    if (!timing && !out) return 2;
    const auto t0 = std::chrono::steady_clock::now();
    for (Case& c : cases) {
        orbx_sim3opt_result res;
        run_case(c, &res);
        if (out) {
            std::fwrite(&res, sizeof(res), 1, out);
            std::fwrite(c.keep.data(), 1, c.keep.size(), out);
        }
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (timing) std::printf("%.3f\n", ncases ? us / ncases : 0.0);
    return out && std::fclose(out) ? 2 : 0;
}
