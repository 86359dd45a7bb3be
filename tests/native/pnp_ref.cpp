// pnp_ref.cpp — PnPsolver (src/PnPsolver.cc) restated in plain C++: an EPnP object over flat
// double arrays with an explicit M matrix, a RANSAC object with the reference's three inlier sets,
// and small stand-ins for the OpenCV 3.2 calls the reference makes (MulTransposed, JacobiSVD with
// the completion path, SVBkSb, invert and solve with DECOMP_SVD) [unverified-OpenCV].  It is the
// second, independent CPU restatement that tests/pnp_cases.py is compared with bit for bit; it
// shares only the record layouts of include/ with the kernels.  No liborbx, no GPU.  Built with
// -ffp-contract=off; hypot is the C library's.
//
//   pnp_ref cases.bin results.bin     every call of every case of the file (pnp_cases.write_cases)
//   pnp_ref --time cases.bin          microseconds per case, one thread
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx_match.h"

namespace {

unsigned g_flags;   // ORBX_PNP_QR_SINGULAR | ORBX_PNP_SVD_COMPLETED of the call in progress

// ---- OpenCV stand-ins -----------------------------------------------------------------------------

// MulTransposedR<double, double> with no delta and scale 1: dst = src^T * src, upper triangle by
// serial sums, then completeSymm
void MulTransposed(const double* src, int rows, int cols, double* dst) {
    for (int i = 0; i < cols; ++i)
        for (int j = i; j < cols; ++j) {
            double s = 0;
            for (int k = 0; k < rows; ++k) s += src[k * cols + i] * src[k * cols + j];
            dst[i * cols + j] = s * 1.0;
        }
    for (int i = 0; i < cols; ++i)
        for (int j = 0; j < i; ++j) dst[i * cols + j] = dst[j * cols + i];
}

struct RNG {
    uint64_t state = 0x12345678;
    unsigned next() {
        state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
        return (unsigned)state;
    }
};

// lapack.cpp JacobiSVDImpl_<double>; the sort carries the rows of At with W, and those of Vt
// where Vt is not null
void JacobiSVD(double* At, size_t astep, double* _W, double* Vt, size_t vstep, int m, int n,
               int n1) {
    const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
    std::vector<double> W(n);
    int i, j, k, iter, max_iter = std::max(m, 30);
    double c, s, sd;
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            double t = At[i * astep + k];
            sd += t * t;
        }
        W[i] = sd;
        if (Vt) {
            for (k = 0; k < n; k++) Vt[i * vstep + k] = 0;
            Vt[i * vstep + i] = 1;
        }
    }
    for (iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (i = 0; i < n - 1; i++)
            for (j = i + 1; j < n; j++) {
                double *Ai = At + i * astep, *Aj = At + j * astep;
                double a = W[i], p = 0, b = W[j];
                for (k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (std::abs(p) <= eps * std::sqrt(a * b)) continue;
                p *= 2;
                double beta = a - b, gamma = hypot(p, beta);
                if (beta < 0) {
                    double delta = (gamma - beta) * 0.5;
                    s = std::sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = std::sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (k = 0; k < m; k++) {
                    double t0 = c * Ai[k] + s * Aj[k];
                    double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += t0 * t0;
                    b += t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                if (Vt) {
                    double *Vi = Vt + i * vstep, *Vj = Vt + j * vstep;
                    for (k = 0; k < n; k++) {
                        double t0 = c * Vi[k] + s * Vj[k];
                        double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0;
                        Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            double t = At[i * astep + k];
            sd += t * t;
        }
        W[i] = std::sqrt(sd);
    }
    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            for (k = 0; k < m; k++) std::swap(At[i * astep + k], At[j * astep + k]);
            if (Vt)
                for (k = 0; k < n; k++) std::swap(Vt[i * vstep + k], Vt[j * vstep + k]);
        }
    }
    for (i = 0; i < n; i++) _W[i] = W[i];
    RNG rng;
    for (i = 0; i < n1; i++) {
        sd = i < n ? W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            g_flags |= ORBX_PNP_SVD_COMPLETED;
            const double val0 = 1. / m;
            for (k = 0; k < m; k++) At[i * astep + k] = (rng.next() & 256) != 0 ? val0 : -val0;
            for (iter = 0; iter < 2; iter++)
                for (j = 0; j < i; j++) {
                    sd = 0;
                    for (k = 0; k < m; k++) sd += At[i * astep + k] * At[j * astep + k];
                    double asum = 0;
                    for (k = 0; k < m; k++) {
                        double t = At[i * astep + k] - sd * At[j * astep + k];
                        At[i * astep + k] = t;
                        asum += std::abs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (k = 0; k < m; k++) At[i * astep + k] *= asum;
                }
            sd = 0;
            for (k = 0; k < m; k++) {
                double t = At[i * astep + k];
                sd += t * t;
            }
            sd = std::sqrt(sd);
        }
        s = sd > minval ? 1 / sd : 0.;
        for (k = 0; k < m; k++) At[i * astep + k] *= s;
    }
}

// cvSVD(A, W, U, V, flags) for a square n x n A: Ut receives U^T (CV_SVD_U_T), V (when not null)
// receives V itself
void cvSVD_square(const double* A, int n, double* W, double* Ut, double* V) {
    std::vector<double> vt(n * n);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < n; ++k) Ut[i * n + k] = A[k * n + i];
    JacobiSVD(Ut, n, W, vt.data(), n, n, n, n);
    if (V)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) V[i * n + j] = vt[j * n + i];
}

// SVBkSbImpl_<double> with uT and vT both set (u: nm rows of m, v: nm rows of n), b m x nb or
// null (then the identity, nb = m), x n x nb
void SVBkSb(int m, int n, const double* w, const double* u, const double* v, const double* b,
            int nb, double* x) {
    double threshold = 0;
    const int nm = std::min(m, n);
    if (!b) nb = m;
    for (int i = 0; i < n * nb; ++i) x[i] = 0;
    for (int i = 0; i < nm; ++i) threshold += w[i];
    threshold *= DBL_EPSILON * 2;
    std::vector<double> buffer(nb);
    for (int i = 0; i < nm; ++i, u += m, v += n) {
        double wi = w[i];
        if (std::abs(wi) <= threshold) continue;
        wi = 1 / wi;
        if (nb == 1) {
            double s = 0;
            if (b)
                for (int j = 0; j < m; ++j) s += u[j] * b[j];
            else
                s = u[0];
            s *= wi;
            for (int j = 0; j < n; ++j) x[j] = x[j] + s * v[j];
        } else {
            if (b) {
                for (int j = 0; j < nb; ++j) buffer[j] = 0;
                for (int r = 0; r < m; ++r)
                    for (int j = 0; j < nb; ++j) buffer[j] = buffer[j] + u[r] * b[r * nb + j];
                for (int j = 0; j < nb; ++j) buffer[j] *= wi;
            } else {
                for (int j = 0; j < nb; ++j) buffer[j] = u[j] * wi;
            }
            for (int r = 0; r < n; ++r)
                for (int j = 0; j < nb; ++j) x[r * nb + j] = x[r * nb + j] + v[r] * buffer[j];
        }
    }
}

// cvInvert(A, X, CV_SVD), 3x3
void cvInvert3(const double* A, double* X) {
    double ut[9], w[3], vt[9];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) ut[i * 3 + k] = A[k * 3 + i];
    JacobiSVD(ut, 3, w, vt, 3, 3, 3, 3);
    SVBkSb(3, 3, w, ut, vt, nullptr, 3, X);
}

// cvSolve(A, b, x, CV_SVD), A m x n with m >= n
void cvSolve(const double* A, int m, int n, const double* b, double* x) {
    std::vector<double> at(n * m), w(n), vt(n * n);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < m; ++k) at[i * m + k] = A[k * n + i];
    JacobiSVD(at.data(), m, w.data(), vt.data(), n, m, n, n);
    SVBkSb(m, n, w.data(), at.data(), vt.data(), b, 1, x);
}

// ---- EPnP over n correspondences (compute_pose, :477-525) ----------------------------------------

inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline double sqdist(const double* p, const double* q) {
    return (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) +
           (p[2] - q[2]) * (p[2] - q[2]);
}

struct Camera { double fu, fv, uc, vc; };

struct Epnp {
    Camera cam;
    int n = 0;
    std::vector<double> X, uv;        // 3 and 2 doubles per correspondence
    std::vector<double> alpha, Xc;    // 4 and 3 doubles per correspondence
    double ctrl_w[4][3], ctrl_c[4][3];

    void clear() { n = 0, X.clear(), uv.clear(); }
    void add(const float* P, float u, float v) {
        for (int r = 0; r < 3; ++r) X.push_back((double)P[r]);
        uv.push_back((double)u), uv.push_back((double)v);
        ++n;
    }

    // :375-409: the centroid and the three principal directions scaled by sqrt(dc / n)
    void control_points() {
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int i = 0; i < n; ++i) s += X[3 * i + j];
            ctrl_w[0][j] = s / n;
        }
        std::vector<double> centred(3 * (size_t)n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < 3; ++j) centred[3 * i + j] = X[3 * i + j] - ctrl_w[0][j];
        double cov[9], dc[3], ut[9];
        MulTransposed(centred.data(), n, 3, cov);
        cvSVD_square(cov, 3, dc, ut, nullptr);
        for (int c = 1; c < 4; ++c) {
            const double k = std::sqrt(dc[c - 1] / n);
            for (int j = 0; j < 3; ++j) ctrl_w[c][j] = ctrl_w[0][j] + k * ut[3 * (c - 1) + j];
        }
    }

    // :411-434
    void barycentric() {
        double cc[9], ci[9];
        for (int i = 0; i < 3; ++i)
            for (int c = 1; c < 4; ++c) cc[3 * i + c - 1] = ctrl_w[c][i] - ctrl_w[0][i];
        cvInvert3(cc, ci);
        alpha.assign(4 * (size_t)n, 0.0);
        for (int i = 0; i < n; ++i) {
            const double d0 = X[3 * i] - ctrl_w[0][0], d1 = X[3 * i + 1] - ctrl_w[0][1],
                         d2 = X[3 * i + 2] - ctrl_w[0][2];
            double* a = &alpha[4 * i];
            for (int j = 0; j < 3; ++j) a[1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
            a[0] = ((1.0 - a[1]) - a[2]) - a[3];
        }
    }

    // :436-451, all 2n rows
    void fill_M(std::vector<double>& M) const {
        M.assign(24 * (size_t)n, 0.0);
        for (int i = 0; i < n; ++i) {
            double* r0 = &M[24 * (size_t)i];
            double* r1 = r0 + 12;
            const double du = cam.uc - uv[2 * i], dv = cam.vc - uv[2 * i + 1];
            for (int c = 0; c < 4; ++c) {
                const double a = alpha[4 * i + c];
                r0[3 * c] = a * cam.fu, r0[3 * c + 1] = 0.0, r0[3 * c + 2] = a * du;
                r1[3 * c] = 0.0, r1[3 * c + 1] = a * cam.fv, r1[3 * c + 2] = a * dv;
            }
        }
    }

    // :760-800: the six control-point pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) of the four last rows
    static void build_L(const double* ut, double L[6][10]) {
        static const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        double d[4][6][3];
        for (int v = 0; v < 4; ++v) {
            const double* row = ut + 12 * (11 - v);
            for (int p = 0; p < 6; ++p)
                for (int k = 0; k < 3; ++k) d[v][p][k] = row[3 * pa[p] + k] - row[3 * pb[p] + k];
        }
        // column c of L pairs null vectors (ia[c], ib[c]); the mixed ones are doubled
        static const int ia[10] = {0, 0, 1, 0, 1, 2, 0, 1, 2, 3}, ib[10] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 3};
        for (int p = 0; p < 6; ++p)
            for (int c = 0; c < 10; ++c) {
                const double v = dot3(d[ia[c]][p], d[ib[c]][p]);
                L[p][c] = ia[c] == ib[c] ? v : 2.0 * v;
            }
    }

    // :860-950, a 6x4 Householder solve by index; false: the singular exit, x untouched
    static bool householder_solve(double A[6][4], double b[6], double x[4]) {
        double diag1[4], diag2[4];
        for (int k = 0; k < 4; ++k) {
            // the reference's scan reads before it steps: rows k, k, k + 1 .. 4
            double eta = std::fabs(A[k][k]);
            for (int i = k + 1; i < 6; ++i) {
                const double e = std::fabs(A[i - 1][k]);
                if (eta < e) eta = e;
            }
            if (eta == 0) return false;
            const double inv_eta = 1. / eta;
            double sum = 0.0;
            for (int i = k; i < 6; ++i) {
                A[i][k] *= inv_eta;
                sum += A[i][k] * A[i][k];
            }
            double sigma = std::sqrt(sum);
            if (A[k][k] < 0) sigma = -sigma;
            A[k][k] += sigma;
            diag1[k] = sigma * A[k][k];
            diag2[k] = -eta * sigma;
            for (int j = k + 1; j < 4; ++j) {
                double s = 0;
                for (int i = k; i < 6; ++i) s += A[i][k] * A[i][j];
                const double tau = s / diag1[k];
                for (int i = k; i < 6; ++i) A[i][j] -= tau * A[i][k];
            }
        }
        for (int j = 0; j < 4; ++j) {
            double tau = 0;
            for (int i = j; i < 6; ++i) tau += A[i][j] * b[i];
            tau /= diag1[j];
            for (int i = j; i < 6; ++i) b[i] -= tau * A[i][j];
        }
        x[3] = b[3] / diag2[3];
        for (int i = 2; i >= 0; --i) {
            double s = 0;
            for (int j = i + 1; j < 4; ++j) s += A[i][j] * x[j];
            x[i] = (b[i] - s) / diag2[i];
        }
        return true;
    }

    // :812-858
    static void refine_betas(const double L[6][10], const double rho[6], double beta[4]) {
        double x[4] = {0, 0, 0, 0};   // zero where the reference has no value
        for (int step = 0; step < 5; ++step) {
            double A[6][4], r[6];
            const double b0 = beta[0], b1 = beta[1], b2 = beta[2], b3 = beta[3];
            for (int i = 0; i < 6; ++i) {
                const double* l = L[i];
                A[i][0] = ((2 * l[0] * b0 + l[1] * b1) + l[3] * b2) + l[6] * b3;
                A[i][1] = ((l[1] * b0 + 2 * l[2] * b1) + l[4] * b2) + l[7] * b3;
                A[i][2] = ((l[3] * b0 + l[4] * b1) + 2 * l[5] * b2) + l[8] * b3;
                A[i][3] = ((l[6] * b0 + l[7] * b1) + l[8] * b2) + 2 * l[9] * b3;
                double q = l[0] * b0 * b0;
                q += l[1] * b0 * b1;
                q += l[2] * b1 * b1;
                q += l[3] * b0 * b2;
                q += l[4] * b1 * b2;
                q += l[5] * b2 * b2;
                q += l[6] * b0 * b3;
                q += l[7] * b1 * b3;
                q += l[8] * b2 * b3;
                q += l[9] * b3 * b3;
                r[i] = rho[i] - q;
            }
            if (!householder_solve(A, r, x)) g_flags |= ORBX_PNP_QR_SINGULAR;
            for (int i = 0; i < 4; ++i) beta[i] += x[i];
        }
    }

    // the least-squares start over the columns `cols` of L (:667-758); kind 1, 2, 3
    static void initial_betas(int kind, const double L[6][10], const double rho[6], double beta[4]) {
        static const int c1[4] = {0, 1, 3, 6}, c23[5] = {0, 1, 2, 3, 4};
        const int nc = kind == 1 ? 4 : kind == 2 ? 3 : 5;
        const int* cols = kind == 1 ? c1 : c23;
        double sub[30], b[5];
        for (int i = 0; i < 6; ++i)
            for (int c = 0; c < nc; ++c) sub[i * nc + c] = L[i][cols[c]];
        cvSolve(sub, 6, nc, rho, b);
        if (kind == 1) {
            const double sgn_b0 = b[0] < 0 ? -b[0] : b[0];
            beta[0] = std::sqrt(sgn_b0);
            for (int k = 1; k < 4; ++k) beta[k] = (b[0] < 0 ? -b[k] : b[k]) / beta[0];
            return;
        }
        if (b[0] < 0) {
            beta[0] = std::sqrt(-b[0]);
            beta[1] = b[2] < 0 ? std::sqrt(-b[2]) : 0.0;
        } else {
            beta[0] = std::sqrt(b[0]);
            beta[1] = b[2] > 0 ? std::sqrt(b[2]) : 0.0;
        }
        if (b[1] < 0) beta[0] = -beta[0];
        beta[2] = kind == 3 ? b[3] / beta[0] : 0.0;
        beta[3] = 0.0;
    }

    // :651-662 with what it calls (:453-475, :636-649, :569-627, :550-567) -> the mean reprojection error
    double pose_of(const double* ut, const double beta[4], double R[3][3], double t[3]) {
        for (int c = 0; c < 4; ++c)
            for (int k = 0; k < 3; ++k) ctrl_c[c][k] = 0.0;
        for (int v = 0; v < 4; ++v) {
            const double* row = ut + 12 * (11 - v);
            for (int c = 0; c < 4; ++c)
                for (int k = 0; k < 3; ++k) ctrl_c[c][k] += beta[v] * row[3 * c + k];
        }
        Xc.assign(3 * (size_t)n, 0.0);
        for (int i = 0; i < n; ++i) {
            const double* a = &alpha[4 * i];
            for (int k = 0; k < 3; ++k)
                Xc[3 * i + k] = ((a[0] * ctrl_c[0][k] + a[1] * ctrl_c[1][k]) + a[2] * ctrl_c[2][k]) +
                                a[3] * ctrl_c[3][k];
        }
        if (Xc[2] < 0.0)   // the first point's depth decides for all
            for (double& v : Xc) v = -v;
        double mc[3], mw[3];
        for (int k = 0; k < 3; ++k) {
            double sc = 0, sw = 0;
            for (int i = 0; i < n; ++i) sc += Xc[3 * i + k], sw += X[3 * i + k];
            mc[k] = sc / n, mw[k] = sw / n;
        }
        double H[9], Hd[3], Hut[9], Hv[9];
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 3; ++c) {
                double s = 0;
                for (int i = 0; i < n; ++i) s += (Xc[3 * i + j] - mc[j]) * (X[3 * i + c] - mw[c]);
                H[3 * j + c] = s;
            }
        cvSVD_square(H, 3, Hd, Hut, Hv);
        // R = U V^T: U(i, k) = Hut[3 * k + i]
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                R[i][j] = (Hut[i] * Hv[3 * j] + Hut[3 + i] * Hv[3 * j + 1]) + Hut[6 + i] * Hv[3 * j + 2];
        double det = R[0][0] * R[1][1] * R[2][2];
        det += R[0][1] * R[1][2] * R[2][0];
        det += R[0][2] * R[1][0] * R[2][1];
        det -= R[0][2] * R[1][1] * R[2][0];
        det -= R[0][1] * R[1][0] * R[2][2];
        det -= R[0][0] * R[1][2] * R[2][1];
        if (det < 0)
            for (int j = 0; j < 3; ++j) R[2][j] = -R[2][j];
        for (int i = 0; i < 3; ++i) t[i] = mc[i] - dot3(R[i], mw);
        double total = 0.0;
        for (int i = 0; i < n; ++i) {
            const double* P = &X[3 * i];
            const double x = dot3(R[0], P) + t[0], y = dot3(R[1], P) + t[1];
            const double iz = 1.0 / (dot3(R[2], P) + t[2]);
            const double eu = uv[2 * i] - (cam.uc + cam.fu * x * iz);
            const double ev = uv[2 * i + 1] - (cam.vc + cam.fv * y * iz);
            total += std::sqrt(eu * eu + ev * ev);
        }
        return total / n;
    }

    void compute_pose(double R[3][3], double t[3]) {
        control_points();
        barycentric();
        std::vector<double> M;
        fill_M(M);
        double mtm[144], d[12], ut[144];
        MulTransposed(M.data(), 2 * n, 12, mtm);
        cvSVD_square(mtm, 12, d, ut, nullptr);
        double L[6][10], rho[6];
        build_L(ut, L);
        static const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        for (int p = 0; p < 6; ++p) rho[p] = sqdist(ctrl_w[pa[p]], ctrl_w[pb[p]]);
        double err[4], Rs[4][3][3], ts[4][3];
        for (int kind = 1; kind <= 3; ++kind) {
            double beta[4];
            initial_betas(kind, L, rho, beta);
            refine_betas(L, rho, beta);
            err[kind] = pose_of(ut, beta, Rs[kind], ts[kind]);
        }
        int pick = 1;
        if (err[2] < err[1]) pick = 2;
        if (err[3] < err[pick]) pick = 3;
        std::memcpy(R, Rs[pick], sizeof(Rs[pick]));
        std::memcpy(t, ts[pick], sizeof(ts[pick]));
    }
};

// ---- the RANSAC object (:165-339) -----------------------------------------------------------------

struct Ransac {
    Epnp e;
    const orbx_pnp_corr* corr = nullptr;
    int N = 0, n_matches = 0, min_inliers = 0, max_its = 0;
    std::vector<float> bound;                    // mvMaxError
    std::vector<uint8_t> cur, best, refined;     // mvbInliersi, mvbBestInliers, mvbRefinedInliers
    int n_cur = 0, n_best = 0, n_refined = 0, iterations = 0, refines = 0;
    double R[3][3], t[3];
    float best_T[16], refined_T[16];
    const int32_t* quads = nullptr;

    // :308-339 in its types
    void check_inliers() {
        n_cur = 0;
        for (int i = 0; i < N; ++i) {
            const float* P = corr[i].X;
            const float x = R[0][0] * P[0] + R[0][1] * P[1] + R[0][2] * P[2] + t[0];
            const float y = R[1][0] * P[0] + R[1][1] * P[1] + R[1][2] * P[2] + t[1];
            const float iz = 1 / (R[2][0] * P[0] + R[2][1] * P[1] + R[2][2] * P[2] + t[2]);
            const double ue = e.cam.uc + e.cam.fu * x * iz;
            const double ve = e.cam.vc + e.cam.fv * y * iz;
            const float dx = corr[i].u - ue, dy = corr[i].v - ve;
            const float err2 = dx * dx + dy * dy;
            cur[i] = err2 < bound[i];
            n_cur += cur[i];
        }
    }

    void pose_to(float* T) const {
        for (int i = 0; i < 16; ++i) T[i] = i == 15 ? 1.0f : 0.0f;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[i][j];
            T[4 * i + 3] = (float)t[i];
        }
    }

    void fit(const std::vector<int>& idx) {
        e.clear();
        for (int k : idx) e.add(corr[k].X, corr[k].u, corr[k].v);
        e.compute_pose(R, t);
        check_inliers();
    }

    // :260-305
    bool refine() {
        ++refines;
        std::vector<int> idx;
        for (int i = 0; i < N; ++i)
            if (best[i]) idx.push_back(i);
        fit(idx);
        n_refined = n_cur;
        refined = cur;
        if (n_cur > min_inliers) {
            pose_to(refined_T);
            return true;
        }
        return false;
    }

    void give(orbx_pnp_result& res, uint8_t* out, int source, int count, const float* T,
              const std::vector<uint8_t>& mask) const {
        res.found = 1, res.source = source, res.iteration = iterations, res.n_inliers = count;
        std::memset(out, 0, (size_t)n_matches);
        for (int i = 0; i < N; ++i)
            if (mask[i]) out[corr[i].i] = 1;
        std::memcpy(res.Tcw, T, sizeof(res.Tcw));
    }

    // :165-258: res and, when found, all n_matches inlier bytes
    void iterate(int n_iterations, orbx_pnp_result& res, uint8_t* out) {
        std::memset(&res, 0, sizeof(res));
        refines = 0;
        g_flags = 0;
        if (N < min_inliers) {
            res.no_more = 1;
            res.best_inliers = n_best;
            return;
        }
        int done = 0;
        bool returned = false;
        while (!returned && (iterations < max_its || done < n_iterations)) {
            ++done, ++iterations;
            const int32_t* q = quads + 4 * (size_t)(iterations - 1);
            fit({q[0], q[1], q[2], q[3]});
            if (n_cur < min_inliers) continue;
            if (n_cur > n_best) {
                best = cur;
                n_best = n_cur;
                pose_to(best_T);
            }
            if (refine()) {
                give(res, out, 1, n_refined, refined_T, refined);
                returned = true;
            }
        }
        res.n_run = done;
        if (!returned && iterations >= max_its) {
            res.no_more = 1;
            if (n_best >= min_inliers) give(res, out, 2, n_best, best_T, best);
        }
        res.info = (unsigned)refines | g_flags;
        res.best_inliers = n_best;
    }
};

struct Case {
    int N, n_matches, ncalls, nquads;
    orbx_pnp_job job;
    std::vector<int32_t> calls, quads;
    orbx_pnp_state state;
    std::vector<uint8_t> best;
    std::vector<orbx_pnp_corr> corr;
};

bool read_cases(const char* path, std::vector<Case>& cases) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t n = 0;
    bool ok = std::fread(&n, 4, 1, f) == 1 && n >= 0;
    for (int c = 0; ok && c < n; ++c) {
        Case k;
        int32_t h[4];
        ok = std::fread(h, 4, 4, f) == 4 && h[0] >= 0 && h[1] >= 0 && h[2] >= 0 && h[3] >= 0;
        if (!ok) break;
        k.N = h[0], k.n_matches = h[1], k.ncalls = h[2], k.nquads = h[3];
        k.calls.resize(k.ncalls), k.quads.resize(4 * (size_t)k.nquads);
        k.best.resize(k.N), k.corr.resize(k.N);
        ok = std::fread(&k.job, sizeof(k.job), 1, f) == 1 &&
             std::fread(k.calls.data(), 4, k.calls.size(), f) == k.calls.size() &&
             std::fread(&k.state, sizeof(k.state), 1, f) == 1 &&
             std::fread(k.best.data(), 1, k.best.size(), f) == k.best.size() &&
             std::fread(k.corr.data(), sizeof(orbx_pnp_corr), k.corr.size(), f) == k.corr.size() &&
             std::fread(k.quads.data(), 4, k.quads.size(), f) == k.quads.size();
        ok = ok && k.job.N == k.N && k.job.nlevels >= 1 && k.job.nlevels <= 16;
        for (int i = 0; ok && i < k.N; ++i)
            ok = k.corr[i].octave >= 0 && k.corr[i].octave < k.job.nlevels && k.corr[i].i >= 0 &&
                 k.corr[i].i < k.n_matches;
        if (ok) cases.push_back(std::move(k));
    }
    std::fclose(f);
    return ok;
}

// every call of one case; out (when not null) receives result, inlier bytes, state, best per call
bool run_case(const Case& k, FILE* out) {
    Ransac s;
    s.e.cam = Camera{k.job.fx, k.job.fy, k.job.cx, k.job.cy};
    s.corr = k.corr.data();
    s.N = k.N, s.n_matches = k.n_matches;
    for (const orbx_pnp_corr& c : k.corr) s.bound.push_back(k.job.sigma2[c.octave] * k.job.th2);
    s.cur.assign(k.N, 0);
    s.best = k.best;
    s.iterations = k.state.iterations, s.n_best = k.state.best_inliers;
    std::memcpy(s.best_T, k.state.best_Tcw, sizeof(s.best_T));
    s.min_inliers = k.job.min_inliers, s.max_its = k.job.max_its;
    s.quads = k.quads.data();
    for (int c = 0; c < k.ncalls; ++c) {
        // the minimal sets the call may read lie inside the file's
        const long long left = (long long)s.max_its - s.iterations;
        const long long w = std::max<long long>(std::max<long long>(left, k.calls[c]), 0);
        if (k.N >= s.min_inliers) {
            if (s.iterations < 0 || s.iterations + w > k.nquads) return false;
            for (long long q = 4LL * s.iterations; q < 4 * (s.iterations + w); ++q)
                if (k.quads[q] < 0 || k.quads[q] >= k.N) return false;
        }
        orbx_pnp_result res;
        std::vector<uint8_t> inl(k.n_matches, 0xCC);
        s.iterate(k.calls[c], res, inl.data());
        orbx_pnp_state st;
        st.iterations = s.iterations, st.best_inliers = s.n_best;
        std::memcpy(st.best_Tcw, s.best_T, sizeof(st.best_Tcw));
        if (out) {
            std::fwrite(&res, sizeof(res), 1, out);
            std::fwrite(inl.data(), 1, inl.size(), out);
            std::fwrite(&st, sizeof(st), 1, out);
            std::fwrite(s.best.data(), 1, s.best.size(), out);
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const bool timing = argc == 3 && std::strcmp(argv[1], "--time") == 0;
    if (argc != 3) {
        std::fprintf(stderr, "usage: pnp_ref cases.bin results.bin | pnp_ref --time cases.bin\n");
        return 2;
    }
    std::vector<Case> cases;
    if (!read_cases(timing ? argv[2] : argv[1], cases)) {
        std::fprintf(stderr, "pnp_ref: cannot read the cases\n");
        return 1;
    }
    if (timing) {
        for (size_t c = 0; c < cases.size(); ++c) {
            const auto t0 = std::chrono::steady_clock::now();
            int reps = 0;
            do {
                if (!run_case(cases[c], nullptr)) return 1;
                ++reps;
            } while (std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(50));
            const double us = std::chrono::duration<double, std::micro>(
                                  std::chrono::steady_clock::now() - t0).count() / reps;
            std::printf("%zu %d %.2f\n", c, cases[c].N, us);
        }
        return 0;
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 1;
    for (const Case& k : cases)
        if (!run_case(k, out)) {
            std::fprintf(stderr, "pnp_ref: a case points outside its arrays\n");
            std::fclose(out);
            return 1;
        }
    return std::fclose(out) == 0 ? 0 : 1;
}
