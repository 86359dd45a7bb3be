"""Optimizer::OptimizeSim3 (src/Optimizer.cc:1070-1265) restated literally in numpy, and the cases
orbx_sim3_optimize* is checked on (tests/test_sim3opt_cases.py on the CPU against
tests/native/sim3opt_ref.cpp, tests/test_gpu_sim3opt.py on the GPU).

The restatement follows g2o as the call runs it: one VertexSim3Expmap, an EdgeSim3ProjectXYZ and an
EdgeInverseSim3ProjectXYZ per correspondence (fixed points, Huber kernels, Jacobians by
BaseBinaryEdge's central differences), OptimizationAlgorithmLevenberg::solve over the dense 7x7
solver, optimize(5), the classification, optimize(10 or 5).  Scalars are Python floats (IEEE
doubles, one rounding per operation); the per-edge quantities are float64 arrays (elementwise
operations round like scalars); H, b and chi2 are summed edge by edge in the order e12_0, e21_0,
e12_1, ... with np.add.accumulate from 0.0, never np.sum.  Forms evaluated inside Eigen are restated
from the published algorithms [unverified-Eigen]; sin / cos / exp are the transliterations of
orbx_sincos_f64 / orbx_exp_f64 (csrc/orbx_math.h).

`optimize_sim3_np(case, variant)` takes one of VARIANTS to change a single decision; each variant
changes the output of at least one committed case."""
import functools
import math
import struct

import numpy as np

from poseopt_cases import (DBL_MAX, DBL_MIN, _div, _sqrt, pairwise_add, quat_from_matrix, quat_mul,
                           rodrigues, rotate, rotation_matrix, scale_factors, seq_add, sincos_f64)
from my_orb_slam2_amd.features import FRAME_POSE_DTYPE, frame_pose
from my_orb_slam2_amd.sim3 import (SIM3OPT_CORR_DTYPE, SIM3OPT_IN_DTYPE, SIM3OPT_JOB_DTYPE,
                                   SIM3OPT_RESULT_DTYPE)

f32, f64 = np.float32, np.float64
EXP_LIMIT = 700.0

# orbx_match.h: the info word
ITERS_SHIFT, ITERS_MASK, TRIALS_SHIFT, TRIALS_MASK = 3, 0x7f, 10, 0x1ff
REFUSED_OCTAVE, REFUSED_I1, REFUSED_LIMIT, REFUSED_RANGE = 1 << 23, 1 << 24, 1 << 25, 1 << 26
REFUSED_ANY = 0xf << 23
THETA_LIMIT, EXP_LIMIT_FLAG, NONPOSITIVE_SOLVE, FEW_INLIERS, DROPPED = (1 << 27, 1 << 28, 1 << 29,
                                                                        1 << 30, 1 << 31)
FLAG_NAMES = {REFUSED_OCTAVE: "REFUSED_OCTAVE", REFUSED_I1: "REFUSED_I1",
              REFUSED_LIMIT: "REFUSED_LIMIT", REFUSED_RANGE: "REFUSED_RANGE",
              THETA_LIMIT: "THETA_LIMIT", EXP_LIMIT_FLAG: "EXP_LIMIT",
              NONPOSITIVE_SOLVE: "NONPOSITIVE_SOLVE", FEW_INLIERS: "FEW_INLIERS",
              DROPPED: "DROPPED"}

VARIANTS = ("one_sided_jacobian", "recompute_after_pop", "float_compare", "normalized_quat",
            "pair_major_order", "lm_state_carried", "th2_as_delta", "perturb_the_inverse",
            "pairwise_sums")

NLEVELS = 8
UNTOUCHED = 0xCC            # the keep byte of a slot that names no correspondence, before and after
TH2 = f32(10.0)


def info_fields(info):
    info = int(info)
    return dict(rounds=info & 7, iters=(info >> ITERS_SHIFT) & ITERS_MASK,
                trials=(info >> TRIALS_SHIFT) & TRIALS_MASK,
                flags={n for b, n in FLAG_NAMES.items() if info & b})


# ---- orbx_exp_f64 --------------------------------------------------------------------------------

def _hi_word(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0] >> 32


def exp_f64(x):
    """orbx_exp_f64 (csrc/orbx_math.h), operation for operation; None outside the limit."""
    if not abs(x) <= EXP_LIMIT:
        return None
    ln2HI, ln2LO, invln2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, \
        1.44269504088896338700e+00
    P1, P2, P3 = 1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05
    P4, P5 = -1.65339022054652515390e-06, 4.13813679705723846039e-08
    hx = _hi_word(x) & 0x7fffffff
    neg = math.copysign(1.0, x) < 0
    hi = lo = 0.0
    k = 0
    if hx > 0x3fd62e42:
        if hx < 0x3ff0a2b2:
            hi = x + ln2HI if neg else x - ln2HI
            lo = -ln2LO if neg else ln2LO
            k = -1 if neg else 1
        else:
            k = int(invln2 * x + (-0.5 if neg else 0.5))
            t = float(k)
            hi = x - t * ln2HI
            lo = t * ln2LO
        x = hi - lo
    elif hx < 0x3e300000:
        return 1.0 + x
    t = x * x
    c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
    if k == 0:
        return 1.0 - (_div(x * c, c - 2.0) - x)
    y = 1.0 - ((lo - _div(x * c, 2.0 - c)) - hi)
    return math.ldexp(y, k)


# ---- g2o::Sim3 (sim3.h): (q = (x, y, z, w), t, s) -------------------------------------------------

def normalize_q(q):
    x, y, z, w = q
    n = _sqrt(((x * x + y * y) + z * z) + w * w)
    return (_div(x, n), _div(y, n), _div(z, n), _div(w, n))


def sim3_map(S, p):
    """Sim3::map on scalars or arrays."""
    q, t, s = S
    rx, ry, rz = rotate(q, p)
    return (s * rx + t[0], s * ry + t[1], s * rz + t[2])


def sim3_inverse(S):
    q, t, s = S
    c = (-q[0], -q[1], -q[2], q[3])
    m = _div(-1.0, s)
    return (c, rotate(c, (m * t[0], m * t[1], m * t[2])), _div(1.0, s))


def sim3_mul(A, B, variant=None):
    qa, ta, sa = A
    qb, tb, sb = B
    r = rotate(qa, tb)
    q = quat_mul(qa, qb)
    if variant == "normalized_quat":
        q = normalize_q(q)
    return (q, (sa * r[0] + ta[0], sa * r[1] + ta[1], sa * r[2] + ta[2]), sa * sb)


def sim3_exp(u, trace=None, variant=None):
    """Sim3(const Vector7d&) -> (Sim3, 0) or (None, the flag of the routine that refused)."""
    sigma = u[6]
    theta = _sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    O = [[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]]
    s = exp_f64(sigma)
    if s is None:
        if trace is not None:
            trace.append(("exp_limit", sigma))
        return None, EXP_LIMIT_FLAG
    eps = 0.00001
    ssmall, tsmall = abs(sigma) < eps, theta < eps
    sn, cs = 0.0, 1.0
    if not tsmall:
        sc = sincos_f64(theta)
        if sc is None:
            if trace is not None:
                trace.append(("theta_limit", theta))
            return None, THETA_LIMIT
        sn, cs = sc
    if trace is not None:
        trace.append(("exp_branch", bool(ssmall), bool(tsmall)))
    ra = rb = 1.0
    if not tsmall:
        ra = _div(sn, theta)
        rb = _div(1.0 - cs, theta * theta)
    if ssmall:
        C = 1.0
        if tsmall:
            A, B = 1. / 2., 1. / 6.
        else:
            theta2 = theta * theta
            A = _div(1.0 - cs, theta2)
            B = _div(theta - sn, theta2 * theta)
    else:
        C = _div(s - 1.0, sigma)
        if tsmall:
            sigma2 = sigma * sigma
            A = _div((sigma - 1.0) * s + 1.0, sigma2)
            B = _div(((0.5 * sigma2 - sigma) + 1.0) * s, sigma2 * sigma)
        else:
            a, b = s * sn, s * cs
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = _div(a * sigma + (1.0 - b) * theta, theta * c)
            B = _div((C - _div((b - 1.0) * sigma + a * theta, c)) * 1., theta2)
    R = [[0.0] * 3 for _ in range(3)]
    W = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            o2 = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j]
            e = 1.0 if i == j else 0.0
            R[i][j] = (e + O[i][j]) + o2 if tsmall else (e + ra * O[i][j]) + rb * o2
            W[i][j] = (A * O[i][j] + B * o2) + C * e
    q = quat_from_matrix(R)
    if variant == "normalized_quat":
        q = normalize_q(q)
    t = tuple((W[i][0] * u[3] + W[i][1] * u[4]) + W[i][2] * u[5] for i in range(3))
    return (q, t, s), 0


def sim3_from_in(rec):
    """g2o::Sim3(toMatrix3d(R12), toVector3d(t12), s12)."""
    R = [[float(rec["R12"][3 * i + j]) for j in range(3)] for i in range(3)]
    return (quat_from_matrix(R), tuple(float(v) for v in rec["t12"]), float(rec["s12"]))


# ---- Eigen::LDLT<MatrixXd> on the lower triangle [unverified-Eigen] ------------------------------

def ldlt_solve(H, lam, b):
    """x or None (not positive); any size."""
    n = len(b)
    with np.errstate(all="ignore"):
        A = [[f64(H[i][j]) if j <= i else f64(0.0) for j in range(n)] for i in range(n)]
        for j in range(n):
            A[j][j] = f64(H[j][j]) + f64(lam)
        tr = list(range(n))
        sign = 0
        for k in range(n):
            idx, best = k, abs(A[k][k])
            for i in range(k + 1, n):
                if abs(A[i][i]) > best:
                    best, idx = abs(A[i][i]), i
            tr[k] = idx
            if idx != k:
                for j in range(k):
                    A[k][j], A[idx][j] = A[idx][j], A[k][j]
                for i in range(idx + 1, n):
                    A[i][k], A[i][idx] = A[i][idx], A[i][k]
                A[k][k], A[idx][idx] = A[idx][idx], A[k][k]
                for i in range(k + 1, idx):
                    A[i][k], A[idx][i] = A[idx][i], A[i][k]
            if k > 0:
                temp = [A[j][j] * A[k][j] for j in range(k)]
                s = A[k][0] * temp[0]
                for j in range(1, k):
                    s = s + A[k][j] * temp[j]
                A[k][k] = A[k][k] - s
                for i in range(k + 1, n):
                    si = A[i][0] * temp[0]
                    for j in range(1, k):
                        si = si + A[i][j] * temp[j]
                    A[i][k] = A[i][k] - si
            akk = A[k][k]
            valid = abs(akk) > 0.0
            if k == 0 and not valid:
                tr = list(range(n))
                break
            if valid:
                for i in range(k + 1, n):
                    A[i][k] = A[i][k] / akk
            if sign == 1:
                if akk < 0.0:
                    sign = 2
            elif sign == -1:
                if akk > 0.0:
                    sign = 2
            elif sign == 0:
                if akk > 0.0:
                    sign = 1
                elif akk < 0.0:
                    sign = -1
        if sign not in (0, 1):
            return None
        y = [f64(v) for v in b]
        for k in range(n):
            y[k], y[tr[k]] = y[tr[k]], y[k]
        for j in range(n):
            for i in range(j + 1, n):
                y[i] = y[i] - A[i][j] * y[j]
        for i in range(n):
            y[i] = y[i] / A[i][i] if abs(A[i][i]) > DBL_MIN else f64(0.0)
        for i in range(n - 2, -1, -1):
            s = A[i + 1][i] * y[i + 1]
            for j in range(i + 2, n):
                s = s + A[j][i] * y[j]
            y[i] = y[i] - s
        for k in range(n - 1, -1, -1):
            y[k], y[tr[k]] = y[tr[k]], y[k]
        return [float(v) for v in y]


# ---- the optimisation --------------------------------------------------------------------------

def _row3(R, X, r):
    """cv::gemm's small-matrix path, float products and sums, on arrays of points."""
    t = R[3 * r] * X[:, 0]
    t = t + R[3 * r + 1] * X[:, 1]
    return t + R[3 * r + 2] * X[:, 2]


def camera_points(pose, Xw):
    """R*P3Dw + t as cv::Mat evaluates it in float (k_sim3_prepare's form), widened."""
    Xw = np.asarray(Xw, f32).reshape(-1, 3)
    R, t = pose["Rcw"].astype(f32), pose["tcw"].astype(f32)
    with np.errstate(all="ignore"):
        return np.stack([(_row3(R, Xw, r).astype(f64) + f64(t[r])).astype(f32) for r in range(3)],
                        1).astype(f64)


class _Graph:
    """The edges of one call as arrays in correspondence order, and the vertex."""

    def __init__(self, case, variant):
        self.variant = variant
        corr = case["corr"]
        p1, p2 = case["pose1"], case["pose2"]
        self.X1 = camera_points(p1, corr["X1w"])
        self.X2 = camera_points(p2, corr["X2w"])
        self.o1 = corr["kp1"].astype(f64).reshape(-1, 2)
        self.o2 = corr["kp2"].astype(f64).reshape(-1, 2)
        with np.errstate(all="ignore"):
            self.info1 = (f32(1.0) / case["sigma2_1"].astype(f32)[corr["octave1"]]).astype(f64)
            self.info2 = (f32(1.0) / case["sigma2_2"].astype(f32)[corr["octave2"]]).astype(f64)
        self.K1 = tuple(float(p1[k]) for k in ("fx", "fy", "cx", "cy"))
        self.K2 = tuple(float(p2[k]) for k in ("fx", "fy", "cx", "cy"))
        th2 = f32(case["th2"])
        self.th2 = float(th2)
        self.delta = float(th2) if variant == "th2_as_delta" else float(np.sqrt(th2, dtype=f32))
        self.fix_scale = bool(case["fix_scale"])
        n = len(corr)
        self.e12 = np.zeros((n, 2))
        self.e21 = np.zeros((n, 2))
        self.alive = np.ones(n, bool)
        self.est = None

    @staticmethod
    def _err(S, X, obs, K):
        fx, fy, cx, cy = K
        with np.errstate(all="ignore"):
            x, y, z = sim3_map(S, (X[:, 0], X[:, 1], X[:, 2]))
            return np.stack([obs[:, 0] - ((x / z) * fx + cx), obs[:, 1] - ((y / z) * fy + cy)], 1)

    def errors_at(self, S, sel, Sinv=None):
        if Sinv is None:
            Sinv = sim3_inverse(S)
        return (self._err(S, self.X2[sel], self.o1[sel], self.K1),
                self._err(Sinv, self.X1[sel], self.o2[sel], self.K2))

    def compute_error(self, sel):
        """computeError of the selected pairs' edges at the estimate."""
        self.e12[sel], self.e21[sel] = self.errors_at(self.est, sel)

    @staticmethod
    def _chi2(e, w):
        with np.errstate(all="ignore"):
            return e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])

    def chi2(self, sel):
        return self._chi2(self.e12[sel], self.info1[sel]), self._chi2(self.e21[sel], self.info2[sel])

    def robustify(self, e2):
        """(rho, rho') of RobustKernelHuber."""
        dsqr = self.delta * self.delta
        with np.errstate(all="ignore"):
            sq = np.sqrt(e2)
            inl = e2 <= dsqr
            return (np.where(inl, e2, (2 * sq) * self.delta - dsqr),
                    np.where(inl, 1.0, self.delta / sq))

    def active(self):
        return np.flatnonzero(self.alive)

    def order(self, t12, t21):
        """The two edge types' terms in the order of _activeEdges."""
        if self.variant == "pair_major_order":
            return np.concatenate([t12, t21])
        out = np.empty(2 * len(t12))
        out[0::2], out[1::2] = t12, t21
        return out

    def add(self, t12, t21):
        t = self.order(t12, t21)
        return pairwise_add(t) if self.variant == "pairwise_sums" else seq_add(t)

    def active_chi2(self):
        a = self.active()
        c12, c21 = self.chi2(a)
        return self.add(self.robustify(c12)[0], self.robustify(c21)[0])

    def perturbed(self, d, v):
        u = [0.0] * 7
        u[d] = v
        if self.fix_scale:
            u[6] = 0.0
        X, _ = sim3_exp(u, None, self.variant)
        return X

    def jacobians(self, a):
        """linearizeOplus of BaseBinaryEdge: central differences with delta = 1e-9."""
        delta = 1e-9
        scalar = 1.0 / (2 * delta)
        J12 = np.zeros((len(a), 2, 7))
        J21 = np.zeros((len(a), 2, 7))
        with np.errstate(all="ignore"):
            for d in range(7):
                P = sim3_mul(self.perturbed(d, delta), self.est, self.variant)
                Pi = None
                if self.variant == "perturb_the_inverse":
                    Pi = sim3_mul(sim3_inverse(self.est), sim3_inverse(self.perturbed(d, delta)),
                                  self.variant)
                ap, bp = self.errors_at(P, a, Pi)
                if self.variant == "one_sided_jacobian":
                    J12[:, :, d] = (1.0 / delta) * (ap - self.e12[a])
                    J21[:, :, d] = (1.0 / delta) * (bp - self.e21[a])
                    continue
                M = sim3_mul(self.perturbed(d, -delta), self.est, self.variant)
                Mi = None
                if self.variant == "perturb_the_inverse":
                    Mi = sim3_mul(sim3_inverse(self.est), sim3_inverse(self.perturbed(d, -delta)),
                                  self.variant)
                am, bm = self.errors_at(M, a, Mi)
                J12[:, :, d] = scalar * (ap - am)
                J21[:, :, d] = scalar * (bp - bm)
        return J12, J21

    def build(self):
        """buildSystem: H (lower triangle) and b."""
        a = self.active()
        J12, J21 = self.jacobians(a)
        c12, c21 = self.chi2(a)
        with np.errstate(all="ignore"):
            parts = []
            for J, e, om, c in ((J12, self.e12[a], self.info1[a], c12),
                                (J21, self.e21[a], self.info2[a], c21)):
                rho1 = self.robustify(c)[1]
                w = rho1 * om
                r0, r1 = ((-om) * e[:, 0]) * rho1, ((-om) * e[:, 1]) * rho1
                parts.append((J, w, r0, r1))
            H = [[0.0] * 7 for _ in range(7)]
            b = [0.0] * 7
            for i in range(7):
                g = [J[:, 0, i] * r0 + J[:, 1, i] * r1 for J, w, r0, r1 in parts]
                b[i] = self.add(*g)
                for j in range(i + 1):
                    h = [(J[:, 0, i] * w) * J[:, 0, j] + (J[:, 1, i] * w) * J[:, 1, j]
                         for J, w, r0, r1 in parts]
                    H[i][j] = self.add(*h)
        return H, b


def _optimize(g, st, rnd, max_iter):
    """SparseOptimizer::optimize(max_iter) with OptimizationAlgorithmLevenberg::solve."""
    trace = st["trace"]
    x = [0.0] * 7
    carried = g.variant == "lm_state_carried" and "lm" in st
    lam, ni = st["lm"] if carried else (0.0, 0.0)
    nbad = 0
    for it in range(max_iter):
        st["iters"] += 1
        g.compute_error(g.active())
        current = g.active_chi2()
        temp = current
        ini = current
        H, b = g.build()
        if it == 0 and not carried:
            m = 0.0
            for j in range(7):
                a = abs(H[j][j])
                m = m if a < m else a
            lam = 1e-5 * m
            ni = 2.0
            nbad = 0
        rho = 0.0
        qmax = 0
        while True:
            backup = g.est
            sol = ldlt_solve(H, lam, b)
            ok2 = sol is not None
            if ok2:
                x = sol
            else:
                st["flags"] |= NONPOSITIVE_SOLVE
            st["trials"] += 1
            if g.fix_scale:
                x = x[:6] + [0.0]
            X, why = sim3_exp(x, trace, g.variant)
            if X is not None:
                g.est = sim3_mul(X, g.est, g.variant)
                g.compute_error(g.active())
                temp = g.active_chi2()
            else:
                st["flags"] |= why
                ok2 = False
            if not ok2:
                temp = DBL_MAX
            rho = current - temp
            scale = 0.0
            for j in range(7):
                scale = scale + x[j] * (lam * x[j] + b[j])
            scale = scale + 1e-3
            rho = _div(rho, scale)
            good = rho > 0 and math.isfinite(temp)
            if good:
                tt = 2 * rho - 1
                alpha = 1.0 - (tt * tt) * tt
                up, lo = 2.0 / 3.0, 1.0 / 3.0
                alpha = up if up < alpha else alpha
                lam = lam * (alpha if lo < alpha else lo)
                ni = 2.0
                current = temp
            else:
                lam = lam * ni
                ni = ni * 2
                g.est = backup
                if g.variant == "recompute_after_pop":
                    g.compute_error(g.active())
            qmax += 1
            trace.append((rnd, it, qmax, "accept" if good else "reject", ni))
            if not (rho < 0 and qmax < 10):
                break
        st["lm"] = (lam, ni)
        if qmax == 10 or rho == 0:
            trace.append((rnd, it, "terminate", "qmax" if qmax == 10 else "rho0"))
            return
        if (ini - current) * 1e3 < ini:
            nbad += 1
        else:
            nbad = 0
        if nbad >= 3:
            trace.append((rnd, it, "terminate", "three_in_a_row"))
            return
    trace.append((rnd, max_iter - 1, "ran_out"))


def refusal(case):
    corr = case["corr"]
    n, r = len(corr), 0
    nl1, nl2 = len(case["sigma2_1"]), len(case["sigma2_2"])
    nl1, nl2 = case.get("nlevels1", nl1), case.get("nlevels2", nl2)
    if nl1 < 1 or nl1 > 16 or nl2 < 1 or nl2 > 16:
        r |= REFUSED_OCTAVE
    if n > case["max_n"]:
        r |= REFUSED_LIMIT
    if case.get("out_of_range"):
        r |= REFUSED_RANGE
    if r:
        return r
    o1, o2, i1 = corr["octave1"], corr["octave2"], corr["i1"]
    if ((o1 < 0) | (o1 >= nl1) | (o2 < 0) | (o2 >= nl2)).any():
        r |= REFUSED_OCTAVE
    if ((i1 < 0) | (i1 >= case["mN1"])).any() or (np.diff(i1.astype(np.int64)) <= 0).any():
        r |= REFUSED_I1
    return r


def result_record(S, n_in, n_corr, n_bad, info):
    """orbx_sim3opt_result: the counts, g2oS12 and Converter::toCvMat(g2oS12)."""
    r = np.zeros((), SIM3OPT_RESULT_DTYPE)
    q, t, s = S
    r["n_inliers"], r["n_correspondences"], r["n_bad"], r["info"] = n_in, n_corr, n_bad, info
    r["q"], r["t"], r["s"] = q, t, s
    with np.errstate(all="ignore"):
        R = np.array(rotation_matrix(q), f64)
        T = np.zeros((4, 4), f32)
        T[:3, :3] = (f64(s) * R).astype(f32)
        T[:3, 3] = np.array(t, f64).astype(f32)
        T[3, 3] = 1
    r["T12"] = T.reshape(16)
    return r


def optimize_sim3_np(case, variant=None):
    """-> dict(res (SIM3OPT_RESULT_DTYPE), keep, trace, history [(bad per pair, chi2 12, chi2 21)])."""
    assert variant is None or variant in VARIANTS
    out = dict(keep=case["keep_in"].copy(), trace=[], history=[])
    start = sim3_from_in(case["sim3_in"])
    if variant == "normalized_quat":
        start = (normalize_q(start[0]), start[1], start[2])
    refuse = refusal(case)
    if refuse:
        out["res"] = result_record(start, 0, 0, 0, refuse)
        return out
    g = _Graph(case, variant)
    n = len(case["corr"])
    g.est = start
    st = dict(iters=0, trials=0, flags=0, trace=out["trace"])
    rounds = 0
    th = g.th2

    def classify():
        a = g.active()
        c12, c21 = g.chi2(a)
        with np.errstate(all="ignore"):
            if variant == "float_compare":
                bad = (c12.astype(f32) > f32(th)) | (c21.astype(f32) > f32(th))
            else:
                bad = (c12 > th) | (c21 > th)
        full = np.zeros(n, bool)
        full[a] = bad
        f12, f21 = np.full(n, np.nan), np.full(n, np.nan)
        f12[a], f21[a] = c12, c21
        out["history"].append((full, f12, f21))
        out["keep"][case["corr"]["i1"][full]] = 0
        g.alive &= ~full
        return int(bad.sum())

    if n > 0:
        _optimize(g, st, 0, 5)
        rounds += 1
    nbad = classify()
    if nbad > 0:
        st["flags"] |= DROPPED
    word = lambda: rounds | (st["iters"] << ITERS_SHIFT) | (st["trials"] << TRIALS_SHIFT) | st["flags"]
    if n - nbad < 10:
        st["flags"] |= FEW_INLIERS
        out["res"] = result_record(start, 0, n, nbad, word())
        return out
    _optimize(g, st, 1, 10 if nbad > 0 else 5)
    rounds += 1
    nfail = classify()
    out["res"] = result_record(g.est, n - nbad - nfail, n, nbad, word())
    return out


@functools.lru_cache(maxsize=None)
def _reference_cached(name):
    return optimize_sim3_np(case_named(name))


def reference(case):
    """The restatement's result on a committed case, computed once and shared (do not modify)."""
    return _reference_cached(case["name"])


# ---- the cases ----------------------------------------------------------------------------------

K4 = np.array([458.654, 457.296, 367.215, 248.375], f32)          # EuRoC cam0
K4B = np.array([457.587, 456.134, 379.999, 255.238], f32)         # EuRoC cam1
BOUNDS = (0.0, 752.0, 0.0, 480.0)
EXACT_K = np.array([458.75, 457.25, 367.25, 248.5], f32)


def sigma2_table(nlevels=NLEVELS, factor=1.2):
    s = scale_factors(nlevels, factor)
    return (s * s).astype(f32)


def sim3_in_record(R, t, s):
    r = np.zeros((), SIM3OPT_IN_DTYPE)
    r["R12"], r["t12"], r["s12"] = np.asarray(R, f64).reshape(9), t, s
    return r


def make_case(name, seed, n, mN1=None, noise=0.3, start_rot=0.01, start_t=0.02, start_s=0.02,
              outlier_share=0.0, outlier_px=40.0, outlier_side="both", fix_scale=False, exact=False,
              octaves=None, nlevels=NLEVELS, gt=((0.04, -0.06, 0.03), (0.15, -0.1, 0.05), 1.1),
              th2=TH2, sparse=3):
    """Two keyframes that see the same n points through maps that differ by the similarity S12
    (x1c = s R x2c + t): the points in KF1's camera frame in front of it, their images under S12^-1
    in KF2's, world positions through either keyframe's pose, observations projected with noise,
    float32 inputs.  The start is S12 off by start_rot / start_t / start_s.  exact: identity poses
    and S12, points at multiples of z / 4 at power-of-two depths and EXACT_K's short mantissas, so
    every error is 0.  The correspondences take every `sparse`-th slot of vpMatches1 or so."""
    rng = np.random.default_rng(seed)
    s2 = sigma2_table(nlevels)
    sc = scale_factors(nlevels)
    if exact:
        R12, t12, s12 = np.eye(3), np.zeros(3), 1.0
        p1 = frame_pose(np.eye(3), np.zeros(3), EXACT_K, BOUNDS, sc)
        p2 = frame_pose(np.eye(3), np.zeros(3), EXACT_K, BOUNDS, sc)
    else:
        R12, t12, s12 = rodrigues(gt[0]), np.asarray(gt[1], f64), float(gt[2])
        p1 = frame_pose(rodrigues((0.1, 0.2, -0.05)), np.array([0.3, -0.2, 0.1]), K4, BOUNDS, sc)
        p2 = frame_pose(rodrigues((-0.15, 0.1, 0.08)), np.array([-0.4, 0.1, 0.3]), K4B, BOUNDS, sc)
    mN1 = (sparse * n + 5) if mN1 is None else mN1
    corr = np.zeros(n, SIM3OPT_CORR_DTYPE)
    corr["i1"] = np.sort(rng.choice(mN1, n, replace=False)) if n else []
    corr["octave1"] = rng.integers(0, nlevels, n) if octaves is None else np.resize(octaves[0], n)
    corr["octave2"] = rng.integers(0, nlevels, n) if octaves is None else np.resize(octaves[1], n)
    planted = np.zeros(n, bool)
    planted[rng.permutation(n)[:int(round(outlier_share * n))]] = True
    R1, t1 = p1["Rcw"].reshape(3, 3).astype(f64), p1["tcw"].astype(f64)
    R2, t2 = p2["Rcw"].reshape(3, 3).astype(f64), p2["tcw"].astype(f64)
    K1, K2 = (EXACT_K, EXACT_K) if exact else (K4, K4B)
    for i in range(n):
        if exact:
            z = float(2.0 ** rng.integers(1, 4))
            P1 = np.array([rng.integers(-3, 4) * 0.25 * z, rng.integers(-2, 3) * 0.25 * z, z])
        else:
            z = rng.uniform(2.0, 10.0)
            P1 = np.array([rng.uniform(-0.5, 0.5) * z, rng.uniform(-0.35, 0.35) * z, z])
        P2 = R12.T @ (P1 - t12) / s12
        corr["X1w"][i] = (R1.T @ (P1 - t1)).astype(f32)
        corr["X2w"][i] = (R2.T @ (P2 - t2)).astype(f32)
        for kp, P, K, o, side in (("kp1", P1, K1, corr["octave1"][i], "e12"),
                                  ("kp2", P2, K2, corr["octave2"][i], "e21")):
            u, v = P[0] / P[2] * float(K[0]) + float(K[2]), P[1] / P[2] * float(K[1]) + float(K[3])
            if not exact:
                s = float(sc[o])
                du, dv = rng.normal(0, noise * s, 2)
                if planted[i] and outlier_side in ("both", side):
                    a = rng.uniform(0, 2 * math.pi)
                    du, dv = outlier_px * s * math.cos(a), outlier_px * s * math.sin(a)
                u, v = u + du, v + dv
            corr[kp][i] = (u, v)
    Rs = rodrigues(rng.normal(0, 1, 3) * start_rot) @ R12
    ts = t12 + rng.normal(0, 1, 3) * start_t
    ss = s12 * (1.0 if fix_scale and start_s == 0 else math.exp(rng.normal() * start_s))
    keep = np.full(mN1, UNTOUCHED, np.uint8)
    keep[corr["i1"]] = 1
    return dict(name=name, pose1=p1, pose2=p2, corr=corr, sigma2_1=s2, sigma2_2=s2.copy(), mN1=mN1,
                th2=f32(th2), fix_scale=bool(fix_scale), sim3_in=sim3_in_record(Rs, ts, ss),
                keep_in=keep, max_n=max(n, 1), planted=planted, gt=(R12, t12, s12), exact=exact)


def job_record(case, kf1=0, kf2=1, corr_off=0, flag_off=0):
    j = np.zeros((), SIM3OPT_JOB_DTYPE)
    s1, s2 = case["sigma2_1"], case["sigma2_2"]
    j["kf1"], j["kf2"] = kf1, kf2
    j["sigma2_1"][:min(len(s1), 16)] = s1[:16]
    j["sigma2_2"][:min(len(s2), 16)] = s2[:16]
    j["nlevels1"], j["nlevels2"] = case.get("nlevels1", len(s1)), case.get("nlevels2", len(s2))
    j["mN1"], j["N"], j["corr_off"], j["flag_off"] = case["mN1"], len(case["corr"]), corr_off, flag_off
    j["th2"], j["fix_scale"] = case["th2"], int(case["fix_scale"])
    return j


def _edit(case, name, **kw):
    c = dict(case, name=name)
    for k, v in kw.items():
        c[k] = v
    return c


def chi2_at_start(case, i):
    """(chi2 of e12, chi2 of e21) of pair i at the input Sim3."""
    g = _Graph(case, None)
    g.est = sim3_from_in(case["sim3_in"])
    sel = np.array([i])
    g.compute_error(sel)
    a, b = g.chi2(sel)
    return float(a[0]), float(b[0])


def one_place_case(name, n, P, t, fix_scale):
    """Every point of both keyframes at the one place P, a fraction of a millimetre in front of
    the identity cameras, every observation its exact projection, the start Sim3 (I, t, 1).  H is
    rank deficient; from the far start the residuals are thousands of pixels and the Huber
    weights small, so lambda = 1e-5 * max|H(j,j)| of iteration 0 is small too, and as the steps
    bring the point back towards the camera plane H grows by many orders within the one
    optimize(): lambda falls below the rounding of the factorisation, a pivot of the rank
    deficient part comes out negative and LDLT::isPositive() is false."""
    c = make_case(name, 1, n, exact=True, start_rot=0, start_t=0, start_s=0, fix_scale=fix_scale)
    c["corr"] = c["corr"].copy()
    P = np.asarray(P, f32)
    c["corr"]["X1w"][:] = P
    c["corr"]["X2w"][:] = P
    K, X = EXACT_K.astype(f64), P.astype(f64)
    uv = (X[0] / X[2] * K[0] + K[2], X[1] / X[2] * K[1] + K[3])
    c["corr"]["kp1"][:] = uv
    c["corr"]["kp2"][:] = uv
    c["sim3_in"] = sim3_in_record(np.eye(3), np.asarray(t, f32), 1.0)
    return c


def threshold_case(name, side, ulps):
    """Both cameras with focal lengths of 0 and the principal point at the origin: every projection
    is (0, 0) whatever the estimate, so the numeric Jacobians, H and b are 0, the step is 0 and
    rho == 0 ends both stages at the input Sim3, and an edge's error is its observation itself.
    Every observation is (0, 0) but pair 4's in KF1 (side "e12") or KF2 ("e21"): (e0, e1) with
    information w = 1.0f / 1.6f = 0.625, so chi2 = e0 * (w * e0) + e1 * (w * e1): e0 = 4 gives
    exactly 10 (ulps = 0), a tiny e1 beside it the double above (+1), and a search over the float
    grids of sigma2, e0 and e1 the double below (-1)."""
    c = make_case(name, 500, 14, exact=True, start_rot=0, start_t=0, start_s=0)
    corr = c["corr"].copy()
    c["corr"] = corr
    for p in ("pose1", "pose2"):
        c[p] = c[p].copy()
        for k in ("fx", "fy", "cx", "cy"):
            c[p][k] = 0
    kp, oc, sg = ("kp1", "octave1", "sigma2_1") if side == "e12" else ("kp2", "octave2", "sigma2_2")
    corr["kp1"], corr["kp2"], corr["octave1"], corr["octave2"] = 0, 0, 0, 0
    corr[oc][4] = 5
    t = c[sg].copy()
    t[5] = f32(1.6)
    c[sg] = t
    w = float(f32(1.0) / f32(1.6))
    assert w == 0.625
    chi = lambda e0, e1: float(e0) * (w * float(e0)) + float(e1) * (w * float(e1))
    want = {-1: float(np.nextafter(10.0, 0)), 0: 10.0, 1: float(np.nextafter(10.0, 20))}[ulps]
    found = None
    if ulps == 0:
        found = (f32(4), f32(0))
    elif ulps == 1:
        found = (f32(4), f32(5e-8))
    else:
        # a slightly larger information (sigma2 a few float steps below 1.6) and the e0 just below
        # sqrt(want / w) leave a gap that a small e1, on a fine part of the float grid, fills
        s2 = f32(1.6)
        for _ in range(20000):
            s2 = np.nextafter(s2, f32(0))
            w = float(f32(1.0) / s2)
            e0 = f32(math.sqrt(want / w))
            while float(e0) * float(e0) > want / w:
                e0 = np.nextafter(e0, f32(0))
            rem = want / w - float(e0) * float(e0)
            if rem > 1e-8:
                continue
            e1 = f32(math.sqrt(rem))
            lo = e1
            for _ in range(16):
                lo = np.nextafter(lo, f32(0))
            for _ in range(33):
                if chi(e0, lo) == want:
                    found = (e0, lo)
                    break
                lo = np.nextafter(lo, f32(1))
            if found:
                t[5] = s2
                break
    assert found is not None and chi(*found) == want, name
    corr[kp][4] = found
    pick = 0 if side == "e12" else 1
    assert chi2_at_start(c, 4)[pick] == want and chi2_at_start(c, 4)[1 - pick] == 0.0
    c["threshold_pair"] = 4
    return c


@functools.lru_cache(maxsize=None)
def all_cases_tuple():
    cases = []
    add = cases.append
    # correspondence counts, with the scale free and fixed
    for n in (0, 1, 9, 10, 11, 63, 64, 65, 129):
        for fs in (False, True):
            add(make_case(f"count_{n}_{'fixed' if fs else 'free'}", 100 + 7 * n + fs, n,
                          fix_scale=fs, start_s=0.0 if fs else 0.02))
    # exact observations: every chi2 is 0, the step is 0, rho == 0 terminates
    for fs in (False, True):
        add(make_case(f"exact_{'fixed' if fs else 'free'}", 300 + fs, 24, exact=True, start_rot=0,
                      start_t=0, start_s=0, fix_scale=fs))
    # the start at the optimum of noisy observations; only the scale off by a little (the
    # |sigma| >= 1e-5, theta < 1e-5 branch)
    add(make_case("start_at_optimum", 310, 60, noise=0.01, start_rot=0, start_t=0, start_s=0))
    add(make_case("scale_only", 311, 40, noise=0.0, start_rot=0, start_t=0, start_s=1e-4))
    # far starts: rejected trials, ni doubling, ten rejections, stale errors
    for k, (rot, tr, ss) in enumerate(((0.1, 0.2, 0.1), (0.3, 0.5, 0.2), (0.6, 1.0, 0.4),
                                       (1.0, 2.0, 0.6), (1.5, 3.0, 1.0), (2.5, 4.0, 1.5))):
        for fs in (False, True):
            add(make_case(f"far_{k}_{'fixed' if fs else 'free'}", 320 + k, 50, start_rot=rot,
                          start_t=tr, start_s=0.0 if fs else ss, fix_scale=fs))
    # slow progress: the three-in-a-row counter
    for k in range(4):
        add(make_case(f"slow_{k}", 340 + k, 30, noise=2.0, start_rot=0.002, start_t=0.002,
                      start_s=0.001, outlier_share=0.2, outlier_px=6.0))
    # 30 % gross outliers
    for fs in (False, True):
        add(make_case(f"outliers_{'fixed' if fs else 'free'}", 350 + fs, 100, outlier_share=0.3,
                      fix_scale=fs, start_s=0.0 if fs else 0.02))
    # a pair whose e12 passes while its e21 fails, and the reverse
    add(make_case("outliers_e21_only", 352, 40, outlier_share=0.2, outlier_side="e21"))
    add(make_case("outliers_e12_only", 353, 40, outlier_share=0.2, outlier_side="e12"))
    # exactly 10 and exactly 9 pairs left after the first stage
    add(make_case("ten_left", 354, 15, outlier_share=1 / 3))
    add(make_case("nine_left", 355, 14, outlier_share=5 / 14))
    # borderline pairs
    for k in range(4):
        add(make_case(f"borderline_{k}", 360 + k, 40, noise=1.0, start_rot=0.05, start_t=0.1,
                      start_s=0.05, outlier_share=0.25, outlier_px=4.0, fix_scale=bool(k & 1)))
    # octaves 0 and nlevels - 1, nlevels 1 and 16
    add(make_case("octave_0", 371, 25, octaves=([0], [0])))
    add(make_case("octave_top", 372, 25, octaves=([NLEVELS - 1], [NLEVELS - 1])))
    add(make_case("nlevels_16_top", 373, 25, octaves=([15, 0], [0, 15]), nlevels=16))
    add(make_case("nlevels_1", 374, 25, octaves=([0], [0]), nlevels=1))
    # every slot of vpMatches1 a correspondence, and very sparse ones
    add(make_case("dense_i1", 375, 30, mN1=30))
    add(make_case("sparse_i1", 376, 30, mN1=5000))
    # bad geometry through the same IEEE operations: a point at camera z = 0, one behind the camera
    for name, fs in (("z_zero", False), ("z_zero_fixed", True)):
        c = make_case(name, 377, 20, exact=True, start_rot=0, start_t=0, start_s=0, fix_scale=fs)
        c["corr"] = c["corr"].copy()
        c["corr"]["X1w"][3] = (0.5, -0.25, 0.0)       # identity poses: P3D1c itself
        add(c)
    c = make_case("behind", 378, 20)
    c["corr"] = c["corr"].copy()
    R2, t2 = c["pose2"]["Rcw"].reshape(3, 3).astype(f64), c["pose2"]["tcw"].astype(f64)
    P2 = R2 @ c["corr"]["X2w"][5].astype(f64) + t2
    c["corr"]["X2w"][5] = (R2.T @ (-P2 - t2)).astype(f32)
    add(c)
    c = make_case("nan_point", 379, 20)
    c["corr"] = c["corr"].copy()
    c["corr"]["X2w"][2] = np.nan
    add(c)
    # all points at one place: a rank-deficient H that lambda rescues
    c = make_case("degenerate_points", 380, 12)
    c["corr"] = c["corr"].copy()
    c["corr"]["X1w"][:] = c["corr"]["X1w"][0]
    c["corr"]["X2w"][:] = c["corr"]["X2w"][0]
    add(c)
    # updates outside the sincos / exp limits, finite: an ordinary scene seen through focal lengths
    # of 1e-6 pixels (the scale fixed) asks for rotations of 4e6 rad, through 1e-4 pixels (the
    # scale free) for sigma = 5e5
    for name, fs, foc in (("theta_limit", True, 1e-6), ("exp_limit", False, 1e-4)):
        c = make_case(name, 381, 12, fix_scale=fs, start_s=0.0 if fs else 0.3)
        for p in ("pose1", "pose2"):
            c[p] = c[p].copy()
            c[p]["fx"] = c[p]["fy"] = foc
        add(c)
    # a non-positive solve (one_place_case): one stage and two, the scale fixed and free
    add(one_place_case("nonpositive_11_fixed", 11,
                       (-0.027112402021884918, -0.013794595375657082, 0.0005939259426668286),
                       (-0.039681337773799896, 0.005319410469383001, 1.1367361545562744), True))
    add(one_place_case("nonpositive_14_fixed", 14,
                       (-0.0318603590130806, -0.01814308948814869, 0.0001743373868521303),
                       (-0.07980742305517197, 0.06427488476037979, 0.9731593728065491), True))
    add(one_place_case("nonpositive_9_free", 9,
                       (-0.041729141026735306, 0.035085856914520264, 0.0002625417255330831),
                       (0.21323521435260773, 0.27062177658081055, 0.684175968170166), False))
    add(one_place_case("nonpositive_4_fixed", 4,
                       (0.020702000707387924, 0.018674705177545547, 0.00016117047925945371),
                       (-0.09687571227550507, 0.1499362289905548, 1.3662188053131104), True))
    # a rejected trial that decides the flags: one observation at 1e20 pixels dominates the robust
    # chi2, so the first step leaves the sum as it was: rho == 0, the step is popped and optimize
    # terminates, and the classification reads the errors of that popped trial
    for name, n in (("rho0_stale_few", 8), ("rho0_stale", 14)):
        c = make_case(name, 391, n, start_rot=0.05, start_t=0.2, start_s=0.05)
        c["corr"] = c["corr"].copy()
        c["corr"]["kp1"][2][0] = 1e20
        add(c)
    # chi2 one double ulp on either side of th2 = 10, and on it, in either edge
    for side in ("e12", "e21"):
        for tag, u in (("below", -1), ("at", 0), ("above", 1)):
            add(threshold_case(f"chi2_{tag}_th2_{side}", side, u))
    # refusals
    base = make_case("refuse_base", 400, 12)
    for tag, o in (("neg", -1), ("high", NLEVELS), ("huge", 1 << 20)):
        for f in ("octave1", "octave2"):
            k = base["corr"].copy()
            k[f][1] = o
            add(_edit(base, f"refuse_{f}_{tag}", corr=k))
    for tag, nl in (("0", 0), ("17", 17), ("neg", -3)):
        add(_edit(base, f"refuse_nlevels1_{tag}", nlevels1=nl))
        add(_edit(base, f"refuse_nlevels2_{tag}", nlevels2=nl))
    k = base["corr"].copy()
    k["i1"][0] = -1
    add(_edit(base, "refuse_i1_negative", corr=k))
    k = base["corr"].copy()
    k["i1"][-1] = base["mN1"]
    add(_edit(base, "refuse_i1_high", corr=k))
    k = base["corr"].copy()
    k["i1"][5] = k["i1"][4]
    add(_edit(base, "refuse_i1_repeated", corr=k))
    k = base["corr"].copy()
    k["i1"][[5, 6]] = k["i1"][[6, 5]]
    add(_edit(base, "refuse_i1_decreasing", corr=k))
    add(_edit(base, "refuse_count", max_n=len(base["corr"]) - 1))
    add(_edit(base, "refuse_range", out_of_range=True))
    # random candidates
    rng = np.random.default_rng(2025)
    for k in range(24):
        n = int(rng.integers(1, 160))
        fs = bool(k % 3 == 0)
        add(make_case(f"random_{k}", 1000 + k, n, noise=float(rng.uniform(0.1, 1.0)),
                      start_rot=float(rng.uniform(0, 0.2)), start_t=float(rng.uniform(0, 0.3)),
                      start_s=0.0 if fs else float(rng.uniform(0, 0.2)), fix_scale=fs,
                      outlier_share=float(rng.choice([0, 0.1, 0.3])),
                      outlier_px=float(rng.uniform(5, 50))))
    return tuple(cases)


def all_cases():
    return list(all_cases_tuple())


def case_named(name):
    for c in all_cases_tuple():
        if c["name"] == name:
            return c
    raise KeyError(name)


def write_cases(path, cases):
    """The file tests/native/sim3opt_ref.cpp reads."""
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            f.write(np.asarray(c["pose1"], FRAME_POSE_DTYPE).tobytes())
            f.write(np.asarray(c["pose2"], FRAME_POSE_DTYPE).tobytes())
            f.write(job_record(c).tobytes())
            f.write(np.asarray(c["sim3_in"], SIM3OPT_IN_DTYPE).tobytes())
            f.write(np.array([c["max_n"], bool(c.get("out_of_range"))], np.int32).tobytes())
            f.write(np.ascontiguousarray(c["corr"]).tobytes())
            f.write(np.ascontiguousarray(c["keep_in"], np.uint8).tobytes())


def read_results(path, cases):
    """-> [(result record, keep bytes)] as sim3opt_ref wrote them."""
    raw = open(path, "rb").read()
    out, o = [], 0
    rs = SIM3OPT_RESULT_DTYPE.itemsize
    for c in cases:
        res = np.frombuffer(raw, SIM3OPT_RESULT_DTYPE, 1, o)[0]
        out.append((res, np.frombuffer(raw, np.uint8, c["mN1"], o + rs)))
        o += rs + c["mN1"]
    assert o == len(raw)
    return out
