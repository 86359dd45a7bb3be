"""Optimizer::PoseOptimization (src/Optimizer.cc:245-457) restated literally in numpy, and the cases
orbx_pose_optimization* is checked on (tests/test_poseopt_cases.py on the CPU against
tests/native/poseopt_ref.cpp, tests/test_gpu_poseopt.py on the GPU).

The restatement follows g2o as the call runs it: one VertexSE3Expmap, unary mono / stereo edges in
feature order with Huber kernels, OptimizationAlgorithmLevenberg::solve over the dense 6x6
solver.  Scalars are Python floats (IEEE doubles, one rounding per operation); the per-edge
quantities are float64 arrays (elementwise operations round like scalars); H, b and chi2 are
summed edge by edge with np.add.accumulate / np.subtract.accumulate from 0.0, never np.sum.  Forms
evaluated inside Eigen are restated from the published algorithms [unverified-Eigen]; sin / cos
are sincos_f64, the transliteration of orbx_sincos_f64 (csrc/orbx_math.h).

`pose_optimization_np(case, variant)` takes one of VARIANTS to change a single decision; each
variant changes the output of at least one committed case."""
import functools
import math
import struct

import numpy as np

from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import FRAME_POSE_DTYPE, MAP_POINT_DTYPE, frame_pose

f32, f64 = np.float32, np.float64
DBL_MAX = float(np.finfo(f64).max)
DBL_MIN = float(np.finfo(f64).tiny)
SINCOS_LIMIT = 1048576.0

# orbx_frame.h: the info word
ITERS_SHIFT, ITERS_MASK, TRIALS_SHIFT, TRIALS_MASK = 3, 0x7f, 10, 0x1ff
REFUSED_MP_INDEX, REFUSED_OCTAVE, REFUSED_NLEVELS, REFUSED_COUNT = (1 << 24, 1 << 25, 1 << 26,
                                                                    1 << 27)
THETA_LIMIT, NONPOSITIVE_SOLVE, FEW_EDGES = 1 << 28, 1 << 29, 1 << 30
FLAG_NAMES = {REFUSED_MP_INDEX: "REFUSED_MP_INDEX", REFUSED_OCTAVE: "REFUSED_OCTAVE",
              REFUSED_NLEVELS: "REFUSED_NLEVELS", REFUSED_COUNT: "REFUSED_COUNT",
              THETA_LIMIT: "THETA_LIMIT", NONPOSITIVE_SOLVE: "NONPOSITIVE_SOLVE",
              FEW_EDGES: "FEW_EDGES"}

VARIANTS = ("ge", "double_compare", "double_invz", "recompute_after_pop", "active_count_break",
            "pairwise_sums", "rho_ge_0", "kernel_kept", "estimate_from_previous_round")

NLEVELS = 8
UNTOUCHED = 0xCC            # the outlier flag of a feature without a MapPoint, before and after


def info_fields(info):
    info = int(info)
    return dict(rounds=info & 7, iters=(info >> ITERS_SHIFT) & ITERS_MASK,
                trials=(info >> TRIALS_SHIFT) & TRIALS_MASK,
                flags={n for b, n in FLAG_NAMES.items() if info & b})


# ---- orbx_sincos_f64 ---------------------------------------------------------------------------

def _exponent(v):
    return (struct.unpack("<Q", struct.pack("<d", v))[0] >> 52) & 0x7ff


def sincos_f64(x):
    """orbx_sincos_f64 (csrc/orbx_math.h), operation for operation; None outside the limit."""
    if not abs(x) <= SINCOS_LIMIT:
        return None
    invpio2 = 6.36619772367581382433e-01
    pio2_1, pio2_1t = 1.57079632673412561417e+00, 6.07710050650619224932e-11
    pio2_2, pio2_2t = 6.07710050630396597660e-11, 2.02226624879595063154e-21
    pio2_3, pio2_3t = 2.02226624871116645580e-21, 8.47842766036889956997e-32
    fn = float(np.rint(x * invpio2))
    n = int(fn)
    r = x - fn * pio2_1
    w = fn * pio2_1t
    y0 = r - w
    ex = _exponent(x)
    if ex - _exponent(y0) > 16:
        t = r
        w = fn * pio2_2
        r = t - w
        w = fn * pio2_2t - ((t - r) - w)
        y0 = r - w
        if ex - _exponent(y0) > 49:
            t = r
            w = fn * pio2_3
            r = t - w
            w = fn * pio2_3t - ((t - r) - w)
            y0 = r - w
    y1 = (r - y0) - w
    S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
    S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
    C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
    C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
    z = y0 * y0
    v = z * y0
    rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    ks = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * S1)
    z2 = z * z
    rc = z * (C1 + z * (C2 + z * C3)) + (z2 * z2) * (C4 + z * (C5 + z * C6))
    hz = 0.5 * z
    wc = 1.0 - hz
    kc = wc + (((1.0 - wc) - hz) + (z * rc - y0 * y1))
    return ((ks, kc), (kc, -ks), (-ks, -kc), (-kc, ks))[n & 3]


# ---- SE3Quat (se3quat.h) -----------------------------------------------------------------------

def _sqrt(v):
    return math.sqrt(v) if v >= 0 else float("nan")


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(f64(a) / f64(b))


def quat_from_matrix(R):
    """Eigen's Quaterniond(Matrix3d) -> (x, y, z, w) [unverified-Eigen]."""
    t = (R[0][0] + R[1][1]) + R[2][2]
    if t > 0.0:
        t = _sqrt(t + 1.0)
        w = 0.5 * t
        t = _div(0.5, t)
        return ((R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t, w)
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = _sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0)
    c = [0.0, 0.0, 0.0]
    c[i] = 0.5 * t
    t = _div(0.5, t)
    w = (R[k][j] - R[j][k]) * t
    c[j] = (R[j][i] + R[i][j]) * t
    c[k] = (R[k][i] + R[i][k]) * t
    return (c[0], c[1], c[2], w)


def normalize_rotation(q):
    x, y, z, w = q
    if w < 0.0:
        x, y, z, w = -x, -y, -z, -w
    n = _sqrt(((x * x + y * y) + z * z) + w * w)
    return (_div(x, n), _div(y, n), _div(z, n), _div(w, n))


def rotate(q, p):
    """Eigen's Quaternion * Vector3 on scalars or arrays [unverified-Eigen]."""
    qx, qy, qz, qw = q
    px, py, pz = p
    ux = qy * pz - qz * py
    uy = qz * px - qx * pz
    uz = qx * py - qy * px
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx = qy * uz - qz * uy
    cy = qz * ux - qx * uz
    cz = qx * uy - qy * ux
    return ((px + qw * ux) + cx, (py + qw * uy) + cy, (pz + qw * uz) + cz)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (((aw * bx + ax * bw) + ay * bz) - az * by,
            ((aw * by + ay * bw) + az * bx) - ax * bz,
            ((aw * bz + az * bw) + ax * by) - ay * bx,
            ((aw * bw - ax * bx) - ay * by) - az * bz)


def rotation_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def se3_update(u, est, trace=None):
    """SE3Quat::exp(u) * est with normalizeRotation; None: theta outside sincos_f64's range."""
    q, t = est
    theta = _sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    O = [[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]]
    O2 = [[(O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j] for j in range(3)]
          for i in range(3)]
    eye = lambda i, j: 1.0 if i == j else 0.0
    if theta < 0.00001:
        if trace is not None:
            trace.append(("small_theta",))
        R = [[(eye(i, j) + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        sc = sincos_f64(theta)
        if sc is None:
            if trace is not None:
                trace.append(("theta_limit", theta))
            return None
        s, c = sc
        a = _div(s, theta)
        b = _div(1.0 - c, theta * theta)
        d = _div(theta - s, (theta * theta) * theta)
        R = [[(eye(i, j) + a * O[i][j]) + b * O2[i][j] for j in range(3)] for i in range(3)]
        V = [[(eye(i, j) + b * O[i][j]) + d * O2[i][j] for j in range(3)] for i in range(3)]
    qe = normalize_rotation(quat_from_matrix(R))
    te = [(V[i][0] * u[3] + V[i][1] * u[4]) + V[i][2] * u[5] for i in range(3)]
    rt = rotate(qe, t)
    return (normalize_rotation(quat_mul(qe, q)), (te[0] + rt[0], te[1] + rt[1], te[2] + rt[2]))


def to_se3quat(pose):
    """Converter::toSE3Quat(mTcw)."""
    R = [[float(pose["Rcw"][3 * i + j]) for j in range(3)] for i in range(3)]
    return (normalize_rotation(quat_from_matrix(R)), tuple(float(v) for v in pose["tcw"]))


# ---- Eigen::LDLT<MatrixXd> on the lower triangle [unverified-Eigen] ------------------------------

def ldlt_solve(H, lam, b):
    """(x or None, positive)."""
    n = 6
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


# ---- the sums ----------------------------------------------------------------------------------

def seq_add(terms):
    """0.0 + t0 + t1 + ..., one rounding per edge."""
    return float(np.add.accumulate(np.concatenate([[0.0], terms]))[-1])


def seq_sub(terms):
    """0.0 - t0 - t1 - ..., one rounding per edge."""
    return float(np.subtract.accumulate(np.concatenate([[0.0], terms]))[-1])


def pairwise_add(terms):
    t = np.concatenate([[0.0], terms])
    while len(t) > 1:
        if len(t) & 1:
            t = np.concatenate([t, [0.0]])
        t = t[0::2] + t[1::2]
    return float(t[0])


# ---- the optimisation --------------------------------------------------------------------------

class _Graph:
    """The edges of one call as arrays in edge order, and the vertex."""

    def __init__(self, case, variant):
        self.variant = variant
        pose = case["pose"]
        mp = case["mp_of_feat"]
        self.feat = np.flatnonzero(mp >= 0)
        keys = case["keys"][self.feat]
        n = len(self.feat)
        ur = np.full(len(mp), -1, f32) if case["ur"] is None else case["ur"]
        self.stereo = ~(ur[self.feat] < 0)
        self.obs = np.stack([keys["x"].astype(f64), keys["y"].astype(f64),
                             np.where(self.stereo, ur[self.feat].astype(f64), 0.0)], 1)
        s = pose["scale"][keys["octave"]].astype(f32)
        self.info = (f32(1.0) / (s * s)).astype(f64)
        self.Xw = case["mps"]["pos"][mp[self.feat]].astype(f64)
        self.K = tuple(float(pose[k]) for k in ("fx", "fy", "cx", "cy", "mbf"))
        dm, ds = float(f32(math.sqrt(5.991))), float(f32(math.sqrt(7.815)))
        self.delta = np.where(self.stereo, ds, dm)
        self.err = np.zeros((n, 3))
        self.level = np.zeros(n, np.int32)
        self.kernel = True
        self.est = None

    def compute_error(self, sel):
        """computeError of the selected edges at the estimate."""
        fx, fy, cx, cy, bf = self.K
        q, t = self.est
        X = self.Xw[sel]
        with np.errstate(all="ignore"):
            rx, ry, rz = rotate(q, (X[:, 0], X[:, 1], X[:, 2]))
            x, y, z = rx + t[0], ry + t[1], rz + t[2]
            invz = 1.0 / z
            if self.variant != "double_invz":
                invz = invz.astype(f32).astype(f64)
            us = (x * invz) * fx + cx
            vs = (y * invz) * fy + cy
            um = (x / z) * fx + cx
            vm = (y / z) * fy + cy
            st = self.stereo[sel]
            o = self.obs[sel]
            e = np.zeros((len(X), 3))
            e[:, 0] = o[:, 0] - np.where(st, us, um)
            e[:, 1] = o[:, 1] - np.where(st, vs, vm)
            e[:, 2] = np.where(st, o[:, 2] - (us - bf * invz), 0.0)
        self.err[sel] = e

    def chi2(self, sel):
        e, w, st = self.err[sel], self.info[sel], self.stereo[sel]
        with np.errstate(all="ignore"):
            c = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
            return np.where(st, c + e[:, 2] * (w * e[:, 2]), c)

    def robustify(self, sel):
        """(rho, rho') of RobustKernelHuber on the selected edges' chi2."""
        e2, delta = self.chi2(sel), self.delta[sel]
        dsqr = delta * delta
        with np.errstate(all="ignore"):
            sq = np.sqrt(e2)
            inl = e2 <= dsqr
            return (np.where(inl, e2, (2 * sq) * delta - dsqr), np.where(inl, 1.0, delta / sq))

    def active(self):
        return np.flatnonzero(self.level == 0)

    def active_chi2(self):
        a = self.active()
        terms = self.robustify(a)[0] if self.kernel else self.chi2(a)
        return pairwise_add(terms) if self.variant == "pairwise_sums" else seq_add(terms)

    def build(self):
        """buildSystem: H (lower triangle) and b."""
        a = self.active()
        fx, fy, cx, cy, bf = self.K
        q, t = self.est
        X = self.Xw[a]
        st = self.stereo[a]
        with np.errstate(all="ignore"):
            rx, ry, rz = rotate(q, (X[:, 0], X[:, 1], X[:, 2]))
            x, y, z = rx + t[0], ry + t[1], rz + t[2]
            invz = 1.0 / z
            invz_2 = invz * invz
            zero = np.zeros(len(a))
            A = [[((x * y) * invz_2) * fx, (-(1.0 + ((x * x) * invz_2))) * fx, (y * invz) * fx,
                  (-invz) * fx, zero, (x * invz_2) * fx],
                 [(1.0 + (y * y) * invz_2) * fy, (((-x) * y) * invz_2) * fy, ((-x) * invz) * fy,
                  zero, (-invz) * fy, (y * invz_2) * fy]]
            A.append([A[0][0] - (bf * y) * invz_2, A[0][1] + (bf * x) * invz_2, A[0][2], A[0][3],
                      zero, A[0][5] - bf * invz_2])
            om, e = self.info[a], self.err[a]
            if self.kernel:
                rho1 = self.robustify(a)[1]
                w = rho1 * om
            else:
                w = om
            add = pairwise_add if self.variant == "pairwise_sums" else seq_add
            sub = (lambda v: -pairwise_add(v)) if self.variant == "pairwise_sums" else seq_sub
            H = [[0.0] * 6 for _ in range(6)]
            b = [0.0] * 6
            for i in range(6):
                if self.kernel:
                    g = (((rho1 * A[0][i]) * om) * e[:, 0] + ((rho1 * A[1][i]) * om) * e[:, 1])
                    g = np.where(st, g + ((rho1 * A[2][i]) * om) * e[:, 2], g)
                else:
                    g = (A[0][i] * om) * e[:, 0] + (A[1][i] * om) * e[:, 1]
                    g = np.where(st, g + (A[2][i] * om) * e[:, 2], g)
                b[i] = sub(g)
                for j in range(i + 1):
                    h = (A[0][i] * w) * A[0][j] + (A[1][i] * w) * A[1][j]
                    h = np.where(st, h + (A[2][i] * w) * A[2][j], h)
                    H[i][j] = add(h)
        return H, b


def _optimize(g, st, rnd):
    """SparseOptimizer::optimize(10) with OptimizationAlgorithmLevenberg::solve."""
    trace = st["trace"]
    if len(g.active()) == 0:
        trace.append((rnd, "empty_optimize"))
        return
    x = [0.0] * 6
    lam = ni = 0.0
    nbad = 0
    for it in range(10):
        st["iters"] += 1
        g.compute_error(g.active())
        current = g.active_chi2()
        temp = current
        ini = current
        H, b = g.build()
        if it == 0:
            m = 0.0
            for j in range(6):
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
            nxt = se3_update(x, g.est, trace)
            if nxt is not None:
                g.est = nxt
                g.compute_error(g.active())
                temp = g.active_chi2()
            else:
                st["flags"] |= THETA_LIMIT
                ok2 = False
            if not ok2:
                temp = DBL_MAX
            rho = current - temp
            scale = 0.0
            for j in range(6):
                scale = scale + x[j] * (lam * x[j] + b[j])
            scale = scale + 1e-3
            rho = _div(rho, scale)
            good = (rho >= 0 if g.variant == "rho_ge_0" else rho > 0) and math.isfinite(temp)
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
    trace.append((rnd, 9, "ran_out"))


def pose_optimization_np(case, variant=None):
    """-> dict(pose, outlier, ngood, info, trace, chi2 (per edge, as classified last), edges)."""
    assert variant is None or variant in VARIANTS
    pose = np.asarray(case["pose"], FRAME_POSE_DTYPE).reshape(())
    out = dict(pose=pose.copy(), outlier=case["outlier_in"].copy(), ngood=0, info=0, trace=[],
               chi2=None, edges=0, history=[])
    mp, keys = case["mp_of_feat"], case["keys"]
    n, nmp, nl = len(mp), len(case["mps"]), int(pose["nlevels"])
    refuse = 0
    if nl < 1 or nl > 16:
        refuse |= REFUSED_NLEVELS
    if n > case["max_feat"]:
        refuse |= REFUSED_COUNT
    if not refuse:
        has = mp != -1
        bad = has & ((mp < -1) | (mp >= nmp))
        if bad.any():
            refuse |= REFUSED_MP_INDEX
        if (has & ~bad & ((keys["octave"] < 0) | (keys["octave"] >= nl))).any():
            refuse |= REFUSED_OCTAVE
    if refuse:
        out["info"] = refuse
        return out
    g = _Graph(dict(case, pose=pose), variant)
    flag = out["outlier"]
    flag[g.feat] = 0
    nedges = len(g.feat)
    out["edges"] = nedges
    if nedges < 3:
        out["info"] = FEW_EDGES
        return out
    start = to_se3quat(pose)
    g.est = start
    st = dict(iters=0, trials=0, flags=0, trace=out["trace"])
    thr = np.where(g.stereo, f32(7.815), f32(5.991)).astype(f32)
    rounds = nbad = 0
    for it in range(4):
        if not (variant == "estimate_from_previous_round" and it > 0):
            g.est = start
        _optimize(g, st, it)
        rounds += 1
        g.compute_error(np.flatnonzero(flag[g.feat] != 0))
        chi2 = g.chi2(np.arange(nedges))
        with np.errstate(all="ignore"):
            if variant == "double_compare":
                bad = chi2 > thr.astype(f64)
            elif variant == "ge":
                bad = chi2.astype(f32) >= thr
            else:
                bad = chi2.astype(f32) > thr
        flag[g.feat] = bad
        g.level = bad.astype(np.int32)
        nbad = int(bad.sum())
        out["history"].append((bad.copy(), chi2.copy()))
        out["chi2"] = chi2
        if it == 2 and variant != "kernel_kept":
            g.kernel = False
        if (int((~bad).sum()) if variant == "active_count_break" else nedges) < 10:
            break
    R = rotation_matrix(g.est[0])
    r32 = np.array(R, f64).astype(f32)
    t32 = np.array(g.est[1], f64).astype(f32)
    out["pose"]["Rcw"] = r32.reshape(9)
    out["pose"]["tcw"] = t32
    with np.errstate(all="ignore"):
        for r in range(3):
            s = r32[0][r] * t32[0]
            s = s + r32[1][r] * t32[1]
            s = s + r32[2][r] * t32[2]
            out["pose"]["Ow"][r] = -s
    out["ngood"] = nedges - nbad
    out["info"] = rounds | (st["iters"] << ITERS_SHIFT) | (st["trials"] << TRIALS_SHIFT) | st["flags"]
    return out


@functools.lru_cache(maxsize=None)
def _reference_cached(name):
    return pose_optimization_np(case_named(name))


def reference(case):
    """The restatement's result on a committed case, computed once and shared (do not modify)."""
    return _reference_cached(case["name"])


# ---- the cases ----------------------------------------------------------------------------------

K4 = np.array([458.654, 457.296, 367.215, 248.375], f32)          # EuRoC cam0
BOUNDS = (0.0, 752.0, 0.0, 480.0)
MBF = 47.90639384423901                                           # EuRoC fx * baseline
EXACT_CAM = ((458.75, 457.25, 367.25, 248.5), 48.0)               # products stay exact in double


def scale_factors(nlevels=NLEVELS, factor=1.2):
    s = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        s[i] = s[i - 1] * f32(factor)
    return s


def rodrigues(w):
    w = np.asarray(w, f64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def make_case(name, seed, nfeat, nedges, stereo="mono", noise=0.3, start_rot=0.01, start_t=0.02,
              outlier_share=0.0, outlier_px=40.0, exact=False, octaves=None, depth=(2.0, 12.0),
              gt_rot=(0.05, -0.1, 0.02), gt_t=(0.1, -0.05, 0.2), nlevels=NLEVELS, extra_mps=3,
              start_at_gt=False, cam=None):
    """A synthetic camera, MapPoints in front of it, observations projected from a ground-truth
    pose, float32 inputs.  stereo: "mono", "stereo" or "mixed" (interleaved by feature).  The
    first `nedges` of a random permutation of the features get a MapPoint.  exact: the float32
    inputs reproject without any rounding (identity pose, MapPoints at multiples of z / 4 at
    power-of-two depths, EXACT_CAM's short mantissas), so every chi2 is 0.  cam: (K4, mbf)."""
    rng = np.random.default_rng(seed)
    sc = scale_factors(nlevels)
    K4_, mbf_ = cam if cam is not None else (EXACT_CAM if exact else (K4, MBF))
    K4_ = np.asarray(K4_, f32)
    if exact:
        Rgt, tgt = np.eye(3), np.zeros(3)
    else:
        Rgt, tgt = rodrigues(gt_rot), np.asarray(gt_t, f64)
    Rgt32, tgt32 = Rgt.astype(f32), tgt.astype(f32)
    keys = np.zeros(nfeat, KEYPOINT_DTYPE)
    keys["class_id"] = -1
    keys["x"] = rng.uniform(20, 730, nfeat).astype(f32)
    keys["y"] = rng.uniform(20, 460, nfeat).astype(f32)
    keys["octave"] = rng.integers(0, nlevels, nfeat) if octaves is None else \
        np.resize(np.asarray(octaves), nfeat)
    keys["size"] = 31 * sc[keys["octave"]]
    order = rng.permutation(nfeat)[:nedges]
    mp_of_feat = np.full(nfeat, -1, np.int32)
    nmp = nedges + extra_mps
    slots = rng.permutation(nmp)[:nedges]
    mp_of_feat[order] = slots
    mps = np.zeros(nmp, MAP_POINT_DTYPE)
    mps["pos"] = rng.uniform(-1, 1, (nmp, 3)).astype(f32) + np.array([0, 0, 5], f32)
    mps["min_dist"], mps["max_dist"] = 0.5, 50.0
    fx, fy, cx, cy = (float(v) for v in K4_)
    ur = None if stereo == "mono" else np.full(nfeat, -1, f32)
    is_st = np.zeros(nfeat, bool)
    if stereo == "stereo":
        is_st[:] = True
    elif stereo == "mixed":
        is_st[:] = rng.random(nfeat) < 0.5
        is_st[np.sort(order)] = np.arange(nedges) % 2 == 0        # interleaved in edge order
    planted = np.zeros(nfeat, bool)
    planted[order[:int(round(outlier_share * nedges))]] = True
    for i, m in zip(order, slots):
        if exact:
            z = float(2.0 ** rng.integers(1, 4))
            Xc = np.array([rng.integers(-3, 4) * 0.25 * z, rng.integers(-2, 3) * 0.25 * z, z])
            mps["pos"][m] = Xc.astype(f32)
            u, v = Xc[0] / Xc[2] * fx + cx, Xc[1] / Xc[2] * fy + cy
        else:
            z = rng.uniform(*depth)
            u0, v0 = float(keys["x"][i]), float(keys["y"][i])
            Xc = np.array([(u0 - cx) * z / fx, (v0 - cy) * z / fy, z])
            mps["pos"][m] = (Rgt.T @ (Xc - tgt)).astype(f32)
            Xc = Rgt @ mps["pos"][m].astype(f64) + tgt
            u, v = Xc[0] / Xc[2] * fx + cx, Xc[1] / Xc[2] * fy + cy
            s = float(sc[keys["octave"][i]])
            du, dv = rng.normal(0, noise * s, 2)
            if planted[i]:
                a = rng.uniform(0, 2 * math.pi)
                du, dv = outlier_px * s * math.cos(a), outlier_px * s * math.sin(a)
            u, v = u + du, v + dv
        keys["x"][i], keys["y"][i] = u, v
        if is_st[i]:
            ur[i] = f32(u - mbf_ / Xc[2] + (0 if exact else rng.normal(0, noise)))
    if start_at_gt or exact and start_rot == 0 and start_t == 0:
        Rs, ts = Rgt, tgt
    else:
        Rs = rodrigues(rng.normal(0, 1, 3) * start_rot) @ Rgt
        ts = tgt + rng.normal(0, 1, 3) * start_t
    pose = frame_pose(Rs, ts, K4_, BOUNDS, sc, mbf=mbf_)
    return dict(name=name, pose=pose, keys=keys, ur=ur, mp_of_feat=mp_of_feat, mps=mps,
                outlier_in=np.full(nfeat, UNTOUCHED, np.uint8), max_feat=max(nfeat, 1),
                planted=planted, gt=(Rgt32, tgt32), exact=exact)


def chi2_at_start(case, feat):
    """The double chi2 of feature `feat`'s edge evaluated at the input pose."""
    g = _Graph(case, None)
    g.est = to_se3quat(case["pose"])
    e = np.flatnonzero(g.feat == feat)
    g.compute_error(e)
    return float(g.chi2(e)[0])


def threshold_case(name, ulps_above):
    """Twelve mono edges with garbage observations (all outliers after round 0, so rounds 1-3 run
    the empty optimize and classify at the input pose) and one edge T whose chi2 at the input
    pose, rounded to float, is 5.991f (ulps_above = 0; its double lies above (double)5.991f) or
    the next float (1).  T's observation (float32 steps of 6e-5 px) sets chi2 coarsely; the scale
    table's entry for T's own octave (steps of 1.2e-7 relative) sets it finely."""
    c = make_case(name, 390, 16, 12, "mono", outlier_share=1.0, outlier_px=300.0, octaves=[1])
    T = int(np.flatnonzero(c["mp_of_feat"] >= 0)[4])
    c["keys"]["octave"][T] = 3
    want = f32(5.991) if ulps_above == 0 else np.nextafter(f32(5.991), f32(10))
    g = _Graph(c, None)
    g.est = to_se3quat(c["pose"])
    e = np.flatnonzero(g.feat == T)
    g.compute_error(e)
    # the observation 2.45 scaled pixels off the projection along u
    proj_u = float(c["keys"]["x"][T]) - float(g.err[e[0], 0])
    proj_v = float(c["keys"]["y"][T]) - float(g.err[e[0], 1])
    c["keys"]["y"][T] = f32(proj_v)
    s3 = float(c["pose"]["scale"][3])
    x0 = f32(proj_u + math.sqrt(5.991) * s3)
    base = c["pose"]["scale"][3]
    pose = c["pose"].copy()
    c["pose"] = pose

    def chi(s):
        pose["scale"][3] = s
        return chi2_at_start(c, T)

    # chi2 falls as the scale grows: bisection on the float grid for the largest scale entry with
    # float(chi2) >= want, then a scan of its neighbours; 1 / (s * s) in float moves chi2 by about
    # one float ulp per step and can skip the wanted value, so the observation is stepped too
    for dx in range(64):
        c["keys"]["x"][T] = x0
        for _ in range(dx):
            c["keys"]["x"][T] = np.nextafter(c["keys"]["x"][T], f32(1e9))
        a, b = f32(base * f32(0.99)), f32(base * f32(1.01))
        assert f32(chi(a)) > want > f32(chi(b))
        while np.nextafter(a, b) < b:
            m = f32((f64(a) + f64(b)) / 2)
            if f32(chi(m)) >= want:
                a = m
            else:
                b = m
        for s in (a, np.nextafter(a, f32(0)), np.nextafter(a, f32(9))):
            v = chi(s)
            if f32(v) == want and (ulps_above or v > float(want)):
                c["threshold_feat"] = T
                return c
    raise AssertionError("no input puts chi2 on the wanted float")


def one_place_case(name, seed, nedges, stereo, P, t):
    """Every MapPoint at the one place P, a fraction of a millimetre in front of the identity
    camera, every observation its exact projection through that camera, the start pose (I, t).
    H has rank 2 (3 with stereo edges); from the far start the residuals are thousands of pixels
    and the Huber weights small, so lambda = 1e-5 * max|H(j,j)| of iteration 0 is small too, and
    as the steps bring the point back towards the camera plane H grows by many orders within the
    one optimize(): lambda falls below the rounding of the factorisation, a pivot of the rank
    deficient part comes out negative and LDLT::isPositive() is false."""
    c = make_case(name, seed, nedges + 2, nedges, stereo, gt_rot=(0, 0, 0), gt_t=(0, 0, 0))
    c["mps"]["pos"][:] = np.asarray(P, f32)
    fx, fy, cx, cy = (float(v) for v in K4)
    X = np.asarray(P, f32).astype(f64)
    u, v = X[0] / X[2] * fx + cx, X[1] / X[2] * fy + cy
    has = c["mp_of_feat"] >= 0
    c["keys"]["x"][has], c["keys"]["y"][has] = u, v
    if c["ur"] is not None:
        c["ur"][has & (c["ur"] >= 0)] = f32(u - MBF / X[2])
    c["pose"] = frame_pose(np.eye(3), np.asarray(t), K4, BOUNDS, scale_factors(), mbf=MBF)
    return c


def _edit(case, name, **kw):
    c = dict(case, name=name)
    for k, v in kw.items():
        c[k] = v
    return c


@functools.lru_cache(maxsize=None)
def all_cases_tuple():
    cases = []
    add = cases.append
    # edge counts in mono-only, stereo-only and interleaved forms
    for ne in (0, 2, 3, 9, 10, 63, 64, 65, 129):
        for k, st in enumerate(("mono", "stereo", "mixed")):
            add(make_case(f"count_{ne}_{st}", 100 + 7 * ne + k, ne + 5 + (ne % 3), ne, st))
    # exact observations: chi2 = 0, the step is 0, rho == 0 terminates
    for k, st in enumerate(("mono", "stereo", "mixed")):
        add(make_case(f"exact_{st}", 300 + k, 40, 24, st, exact=True, start_rot=0, start_t=0))
    # the start pose at the optimum of noisy observations: the theta < 1e-5 branch
    add(make_case("start_at_optimum", 310, 80, 60, "mixed", noise=0.01, start_at_gt=True))
    # far starts: rejected trials, ni doubling, ten rejections, stale errors
    for k, (rot, tr) in enumerate(((0.3, 0.5), (0.6, 1.0), (1.0, 2.0), (1.5, 3.0), (2.5, 4.0))):
        for st in ("mono", "mixed"):
            add(make_case(f"far_{k}_{st}", 320 + k, 70, 50, st, start_rot=rot, start_t=tr))
    # slow progress: the three-in-a-row counter
    for k in range(4):
        add(make_case(f"slow_{k}", 340 + k, 50, 30, "mono", noise=2.0, start_rot=0.002,
                      start_t=0.002, outlier_share=0.2, outlier_px=6.0))
    # 30 % gross outliers
    for k, st in enumerate(("mono", "stereo", "mixed")):
        add(make_case(f"outliers_{st}", 350 + k, 150, 120, st, outlier_share=0.3))
    # borderline edges: outlier after round 0, inlier at the end; the kernel's effect after round 2
    for k in range(6):
        add(make_case(f"borderline_{k}", 360 + k, 60, 40, ("mono", "mixed")[k & 1], noise=1.0,
                      start_rot=0.05, start_t=0.1, outlier_share=0.25, outlier_px=4.0))
    # every edge an outlier after round 0: the empty optimize
    add(make_case("all_outliers", 370, 30, 20, "mixed", outlier_share=1.0, outlier_px=60.0))
    # octaves 0 and nlevels - 1
    add(make_case("octave_0", 371, 30, 25, "mixed", octaves=[0]))
    add(make_case("octave_top", 372, 30, 25, "mixed", octaves=[NLEVELS - 1]))
    add(make_case("nlevels_16_top", 373, 30, 25, "mono", octaves=[15, 0], nlevels=16))
    add(make_case("nlevels_1", 374, 30, 25, "stereo", octaves=[0], nlevels=1))
    # bad geometry: a MapPoint at camera z = 0 and one behind the camera, through the same IEEE
    # operations
    c = make_case("z_zero", 375, 30, 20, "mixed", start_rot=0, start_t=0, start_at_gt=True,
                  gt_rot=(0, 0, 0), gt_t=(0, 0, 0))
    m = c["mp_of_feat"][np.flatnonzero(c["mp_of_feat"] >= 0)[3]]
    c["mps"]["pos"][m] = (0.5, -0.25, 0.0)
    add(c)
    c = make_case("behind", 376, 30, 20, "mixed")
    m = c["mp_of_feat"][np.flatnonzero(c["mp_of_feat"] >= 0)[5]]
    c["mps"]["pos"][m] *= f32(-1)
    add(c)
    # a non-positive solve (one_place_case): one round and four rounds, mono, stereo, interleaved
    add(one_place_case("nonpositive_mono_5", 1, 5, "mono", (-0.0011825, -0.04128332, 0.00012894),
                       (-0.3268276, -0.28996107, 1.6760145)))
    add(one_place_case("nonpositive_mono_3", 200450, 3, "mono",
                       (-0.012357315979897976, 0.05318878963589668, 0.0001837816380430013),
                       (-0.0811382457613945, -0.0847383514046669, 0.7778266072273254)))
    add(one_place_case("nonpositive_stereo_14", 200829, 14, "stereo",
                       (0.01608249731361866, -0.023763634264469147, 0.0001285526086576283),
                       (0.1763898879289627, -0.13936221599578857, 0.6800364255905151)))
    add(one_place_case("nonpositive_stereo_4_qmax", 200256, 4, "stereo",
                       (0.034097637981176376, -0.010158763267099857, 0.0003683490795083344),
                       (0.02362137846648693, -0.047266699373722076, 0.6046757698059082)))
    add(one_place_case("nonpositive_mixed_11", 201013, 11, "mixed",
                       (-0.02016465924680233, 0.010351262055337429, 0.00032339090830646455),
                       (-0.28314584493637085, 0.1537044495344162, 1.1758302450180054)))
    # all MapPoints at one ordinary place (rank-deficient H that lambda rescues), and NaN geometry
    c = make_case("degenerate_points", 377, 20, 12, "mono")
    c["mps"]["pos"][:] = c["mps"]["pos"][0]
    add(c)
    c = make_case("nan_point", 378, 20, 12, "mixed")
    c["mps"]["pos"][c["mp_of_feat"][np.flatnonzero(c["mp_of_feat"] >= 0)[2]]] = np.nan
    add(c)
    # theta above the limit, finite: an ordinary scene seen through focal lengths of 1e-6 pixels;
    # every projection collapses onto (cx, cy) and the residuals of hundreds of pixels ask for
    # rotations of 1e8 rad
    c = make_case("theta_limit", 379, 20, 12, "mono")
    c["pose"] = c["pose"].copy()
    c["pose"]["fx"] = c["pose"]["fy"] = 1e-6
    add(c)
    # a rejected trial that decides the flags: one observation at 1e20 pixels dominates the robust
    # chi2 (about 5e20, one ulp is 65536), so the first, large step leaves the sum as it was:
    # rho == 0, the step is popped and optimize terminates, and the classification reads the
    # errors of that popped trial (all but the garbage edge are inliers there, outliers at the
    # far start pose)
    for name, ne in (("rho0_stale_one_round", 8), ("rho0_stale", 14)):
        c = make_case(name, 391, ne + 4, ne, "mono", start_rot=0.05, start_t=0.2)
        c["keys"]["x"][np.flatnonzero(c["mp_of_feat"] >= 0)[2]] = 1e20
        add(c)
    # rho == 0 at convergence with a step that still moves the last bits of the pose
    add(make_case("rho0_converged", 70530, 7, 5, "mono", noise=1.0, start_rot=0.3, start_t=0.0))
    # chi2 within one float ulp of 5.991f, on both sides
    add(threshold_case("chi2_at_threshold", 0))
    add(threshold_case("chi2_above_threshold", 1))
    # refusals
    base = make_case("refuse_base", 380, 20, 12, "mixed")
    mp = base["mp_of_feat"].copy()
    mp[np.flatnonzero(mp >= 0)[0]] = len(base["mps"])
    add(_edit(base, "refuse_mp_high", mp_of_feat=mp))
    mp = base["mp_of_feat"].copy()
    mp[np.flatnonzero(mp < 0)[0]] = -2
    add(_edit(base, "refuse_mp_negative", mp_of_feat=mp))
    for tag, o in (("neg", -1), ("high", NLEVELS), ("huge", 1 << 20)):
        k = base["keys"].copy()
        k["octave"][np.flatnonzero(base["mp_of_feat"] >= 0)[1]] = o
        add(_edit(base, f"refuse_octave_{tag}", keys=k))
    k = base["keys"].copy()
    k["octave"][np.flatnonzero(base["mp_of_feat"] < 0)[0]] = 99     # no MapPoint: not read
    add(_edit(base, "octave_unread", keys=k))
    for tag, nl in (("0", 0), ("17", 17), ("neg", -3)):
        p = base["pose"].copy()
        p["nlevels"] = nl
        add(_edit(base, f"refuse_nlevels_{tag}", pose=p))
    add(_edit(base, "refuse_count", max_feat=len(base["keys"]) - 1))
    # random frames
    rng = np.random.default_rng(2024)
    for k in range(36):
        ne = int(rng.integers(3, 200))
        add(make_case(f"random_{k}", 1000 + k, ne + int(rng.integers(0, 60)), ne,
                      ("mono", "stereo", "mixed")[k % 3], noise=float(rng.uniform(0.1, 1.0)),
                      start_rot=float(rng.uniform(0, 0.2)), start_t=float(rng.uniform(0, 0.3)),
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
    """The file tests/native/poseopt_ref.cpp reads."""
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            n = len(c["keys"])
            f.write(np.asarray(c["pose"], FRAME_POSE_DTYPE).tobytes())
            f.write(np.array([n, len(c["mps"]), c["ur"] is not None, c["max_feat"]],
                             np.int32).tobytes())
            f.write(np.ascontiguousarray(c["keys"]).tobytes())
            if c["ur"] is not None:
                f.write(np.ascontiguousarray(c["ur"], f32).tobytes())
            f.write(np.ascontiguousarray(c["mp_of_feat"], np.int32).tobytes())
            f.write(np.ascontiguousarray(c["mps"]).tobytes())
            f.write(np.ascontiguousarray(c["outlier_in"], np.uint8).tobytes())


def read_results(path, cases):
    """-> [(pose record, ngood, info, outlier)] as poseopt_ref wrote them."""
    raw = open(path, "rb").read()
    out, o = [], 0
    ps = FRAME_POSE_DTYPE.itemsize
    for c in cases:
        n = len(c["keys"])
        pose = np.frombuffer(raw, FRAME_POSE_DTYPE, 1, o)[0]
        ngood = int(np.frombuffer(raw, np.int32, 1, o + ps)[0])
        info = int(np.frombuffer(raw, np.uint32, 1, o + ps + 4)[0])
        out.append((pose, ngood, info, np.frombuffer(raw, np.uint8, n, o + ps + 8)))
        o += ps + 8 + n
    assert o == len(raw)
    return out
