"""PnPsolver (src/PnPsolver.cc) restated literally in Python, and the cases orbx_pnp_* is checked
on (tests/test_pnp_cases.py on the CPU against tests/native/pnp_ref.cpp, tests/test_gpu_pnp.py on
the GPU).

Doubles are Python floats (IEEE binary64, one rounding per operation; division and sqrt through
`dv` / `sq`, which give what IEEE gives where Python raises) and floats np.float32 scalars.  The
forms evaluated inside OpenCV 3.2 are restated as DESIGN.md §2 lists them (PARITY UNPINNED):
`mul_transposed`, `jacobi_svd` (JacobiSVDImpl_<double> with its completion path), `sv_bksb`
(cvSolve), `invert3` (cvInvert).  hypot is the C library's, as lapack.cpp calls it.

`solve(case, variant)` runs the case's sequence of iterate() calls and returns, per call, what
orbx_pnp_iterate leaves, with a decision trace per iteration.  `variant` flips one decision
(VARIANTS); each flip changes the result of at least one committed case."""
import ctypes
import ctypes.util
import functools
import math
import struct

import numpy as np

from my_orb_slam2_amd.pnp import (PNP_CORR_DTYPE, PNP_QR_SINGULAR,
                                  PNP_REFUSED_I, PNP_REFUSED_LIMIT, PNP_REFUSED_OCTAVE,
                                  PNP_REFUSED_QUAD, PNP_RESULT_DTYPE, PNP_STATE_DTYPE,
                                  PNP_SVD_COMPLETED, RAND_MAX, pnp_job, pnp_window)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.hypot.restype = ctypes.c_double
_libm.hypot.argtypes = [ctypes.c_double, ctypes.c_double]

f32 = np.float32
DBL_EPS = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
NAN, INF = float("nan"), float("inf")
SENTINEL = 0xCC
INT_MIN = -2147483648

VARIANTS = ("and_for_or", "ge_best", "ge_refine", "gt_entry", "gt_end", "refine_current",
            "v_for_u", "unsorted_w", "tree_mtm")


def dv(a, b):
    """a / b as IEEE gives it."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def sq(a):
    """sqrt(a) as IEEE gives it."""
    return math.sqrt(a) if a >= 0.0 else (a if a != a else NAN)


# ---- the forms evaluated inside OpenCV 3.2 [unverified-OpenCV] ---------------------------------

def mul_transposed(row, nrows, ncols, tree=False):
    """cvMulTransposed(A, dst, 1) on CV_64F below the gemm switch-over: dst(i, j), j >= i, is the
    sum over k ascending from +0.0 of A(k, i) * A(k, j); the lower triangle is copied from the
    upper.  row(k) gives row k of A."""
    A = [row(k) for k in range(nrows)]
    D = [[0.0] * ncols for _ in range(ncols)]
    for i in range(ncols):
        for j in range(i, ncols):
            if tree:
                t = [A[k][i] * A[k][j] for k in range(nrows)]
                while len(t) > 1:
                    t = [t[a] + t[a + 1] if a + 1 < len(t) else t[a] for a in range(0, len(t), 2)]
                s = t[0] if t else 0.0
            else:
                s = 0.0
                for k in range(nrows):
                    s = s + A[k][i] * A[k][j]
            D[i][j] = s
    for i in range(ncols):
        for j in range(i):
            D[i][j] = D[j][i]
    return D


_UNSORTED = [False]      # the `unsorted_w` variant: no jacobi_svd call sorts
_KEEP = [None]           # a list that receives the matrices of every compute_pose (svd_records)


class _Rng:
    """cv::RNG(0x12345678)"""

    def __init__(self):
        self.state = 0x12345678

    def next(self):
        self.state = ((self.state & 0xffffffff) * 4164903690 + (self.state >> 32)) & ((1 << 64) - 1)
        return self.state & 0xffffffff


def jacobi_svd(At, m, n, want_vt, ev, sort=True):
    """JacobiSVDImpl_<double>(At, W, Vt, m, n, n1 = n, DBL_MIN, 10 * DBL_EPSILON): At holds n rows
    of m doubles (the transpose of the matrix cvSVD is given) and is left as the rows of U^T; ->
    (W, Vt or None).  One-sided Jacobi on the rows, at most max(m, 30) = 30 sweeps; W[i] =
    sqrt(row norm^2); a selection sort, descending, that carries the rows of At and Vt; each row
    times 1 / W[i], a row with W[i] <= DBL_MIN completed from cv::RNG."""
    eps = DBL_EPS * 10
    W = [0.0] * n
    Vt = [[1.0 if i == k else 0.0 for k in range(n)] for i in range(n)] if want_vt else None
    for i in range(n):
        sd = 0.0
        for k in range(m):
            sd = sd + At[i][k] * At[i][k]
        W[i] = sd
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a, p, b = W[i], 0.0, W[j]
                for k in range(m):
                    p = p + Ai[k] * Aj[k]
                if abs(p) <= eps * sq(a * b):
                    continue
                p = p * 2.0
                beta = a - b
                gamma = _libm.hypot(p, beta)
                if beta < 0:
                    ev.add("beta_neg")
                    delta = (gamma - beta) * 0.5
                    s = sq(dv(delta, gamma))
                    c = dv(p, gamma * s * 2.0)
                else:
                    ev.add("beta_nonneg")
                    c = sq(dv(gamma + beta, gamma * 2.0))
                    s = dv(p, gamma * c * 2.0)
                a = b = 0.0
                for k in range(m):
                    t0 = c * Ai[k] + s * Aj[k]
                    t1 = -s * Ai[k] + c * Aj[k]
                    Ai[k], Aj[k] = t0, t1
                    a = a + t0 * t0
                    b = b + t1 * t1
                W[i], W[j] = a, b
                changed = True
                if want_vt:
                    Vi, Vj = Vt[i], Vt[j]
                    for k in range(n):
                        t0 = c * Vi[k] + s * Vj[k]
                        t1 = -s * Vi[k] + c * Vj[k]
                        Vi[k], Vj[k] = t0, t1
        if not changed:
            break
    for i in range(n):
        sd = 0.0
        for k in range(m):
            sd = sd + At[i][k] * At[i][k]
        W[i] = sq(sd)
    if sort and not _UNSORTED[0]:
        for i in range(n - 1):
            j = i
            for k in range(i + 1, n):
                if W[j] < W[k]:
                    j = k
            if i != j:
                ev.add("sort_swapped")
                W[i], W[j] = W[j], W[i]
                At[i], At[j] = At[j], At[i]
                if want_vt:
                    Vt[i], Vt[j] = Vt[j], Vt[i]
    rng = _Rng()
    for i in range(n):
        sd = W[i]
        ii = 0
        while ii < 100 and sd <= DBL_MIN:
            ev.add("svd_completed")
            val0 = dv(1.0, float(m))
            for k in range(m):
                At[i][k] = val0 if (rng.next() & 256) != 0 else -val0
            for _ in range(2):
                for j in range(i):
                    sd = 0.0
                    for k in range(m):
                        sd = sd + At[i][k] * At[j][k]
                    asum = 0.0
                    for k in range(m):
                        t = At[i][k] - sd * At[j][k]
                        At[i][k] = t
                        asum = asum + abs(t)
                    asum = dv(1.0, asum) if asum > eps * 100 else 0.0
                    for k in range(m):
                        At[i][k] = At[i][k] * asum
            sd = 0.0
            for k in range(m):
                sd = sd + At[i][k] * At[i][k]
            sd = sq(sd)
            ii += 1
        s = dv(1.0, sd) if sd > DBL_MIN else 0.0
        for k in range(m):
            At[i][k] = At[i][k] * s
    return W, Vt


def sv_bksb(L, b, ev):
    """cvSolve(L, b, x, CV_SVD) for a 6 x n L and one right-hand side: the thin Jacobi SVD of L,
    then SVBkSb: threshold = 2 * DBL_EPSILON * sum(w); terms with |w| <= threshold skipped; the
    others accumulated in index order, x[j] += ((u_i . b) * (1 / w_i)) * v_i[j]."""
    m, n = len(L), len(L[0])
    At = [[L[k][i] for k in range(m)] for i in range(n)]
    W, Vt = jacobi_svd(At, m, n, True, ev)
    x = [0.0] * n
    thr = 0.0
    for i in range(n):
        thr = thr + W[i]
    thr = thr * (DBL_EPS * 2)
    for i in range(n):
        wi = W[i]
        if abs(wi) <= thr:
            ev.add("bksb_skipped")
            continue
        wi = dv(1.0, wi)
        s = 0.0
        for j in range(m):
            s = s + At[i][j] * b[j]
        s = s * wi
        for j in range(n):
            x[j] = x[j] + s * Vt[i][j]
    return x


def invert3(A, ev):
    """cvInvert(A, X, CV_SVD) on 3x3: SVD::compute then SVD::backSubst with no right-hand side:
    X(r, j) += Vt(i, r) * (U(j, i) * (1 / w_i)) for the kept i in index order."""
    At = [[A[k][i] for k in range(3)] for i in range(3)]
    W, Vt = jacobi_svd(At, 3, 3, True, ev)
    X = [[0.0] * 3 for _ in range(3)]
    thr = ((W[0] + W[1]) + W[2]) * (DBL_EPS * 2)
    for i in range(3):
        wi = W[i]
        if abs(wi) <= thr:
            ev.add("bksb_skipped")
            continue
        wi = dv(1.0, wi)
        buf = [At[i][j] * wi for j in range(3)]
        for r in range(3):
            s = Vt[i][r]
            for j in range(3):
                X[r][j] = X[r][j] + s * buf[j]
    return X


# ---- EPnP (:375-950) -------------------------------------------------------------------------------

def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def dist2(p, q):
    return ((p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) +
            (p[2] - q[2]) * (p[2] - q[2]))


def qr_solve(A, b, x, ev):
    """:860-950 for the 6x4 system; A (flat, 24) and b are overwritten.  The singular exit leaves
    x as it was."""
    nr, nc = 6, 4
    A1, A2 = [0.0] * nc, [0.0] * nc
    for k in range(nc):
        kk = k * nc + k
        # the scan reads the pointer before it advances: rows k, k .. nr - 2 (:880-885)
        eta = abs(A[kk])
        p = kk
        for i in range(k + 1, nr):
            elt = abs(A[p])
            if eta < elt:
                eta = elt
            p += nc
        if eta == 0:
            ev.add("qr_singular")
            return
        inv_eta = dv(1.0, eta)
        s = 0.0
        for i in range(k, nr):
            A[i * nc + k] = A[i * nc + k] * inv_eta
            s = s + A[i * nc + k] * A[i * nc + k]
        sigma = sq(s)
        if A[kk] < 0:
            sigma = -sigma
        A[kk] = A[kk] + sigma
        A1[k] = sigma * A[kk]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s = s + A[i * nc + k] * A[i * nc + j]
            tau = dv(s, A1[k])
            for i in range(k, nr):
                A[i * nc + j] = A[i * nc + j] - tau * A[i * nc + k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau = tau + A[i * nc + j] * b[i]
        tau = dv(tau, A1[j])
        for i in range(j, nr):
            b[i] = b[i] - tau * A[i * nc + j]
    x[nc - 1] = dv(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s = s + A[i * nc + j] * x[j]
        x[i] = dv(b[i] - s, A2[i])


def gauss_newton(L, rho, betas, ev):
    x = [0.0] * 4        # the reference's X is an uninitialised stack array
    for _ in range(5):
        A, b = [0.0] * 24, [0.0] * 6
        b0, b1, b2, b3 = betas
        for i in range(6):
            r = L[i]
            A[4 * i] = 2 * r[0] * b0 + r[1] * b1 + r[3] * b2 + r[6] * b3
            A[4 * i + 1] = r[1] * b0 + 2 * r[2] * b1 + r[4] * b2 + r[7] * b3
            A[4 * i + 2] = r[3] * b0 + r[4] * b1 + 2 * r[5] * b2 + r[8] * b3
            A[4 * i + 3] = r[6] * b0 + r[7] * b1 + r[8] * b2 + 2 * r[9] * b3
            b[i] = rho[i] - (r[0] * b0 * b0 + r[1] * b0 * b1 + r[2] * b1 * b1 + r[3] * b0 * b2 +
                             r[4] * b1 * b2 + r[5] * b2 * b2 + r[6] * b0 * b3 + r[7] * b1 * b3 +
                             r[8] * b2 * b3 + r[9] * b3 * b3)
        qr_solve(A, b, x, ev)
        for i in range(4):
            betas[i] = betas[i] + x[i]


def compute_pose(pws, us, K, ev, variant=None):
    """compute_pose (:477-525) over the n correspondences pws[i] (3 doubles), us[i] (2 doubles);
    K = (fu, fv, uc, vc) as doubles.  -> (R, t)."""
    fu, fv, uc, vc = K
    n = len(pws)
    fn = float(n)
    # choose_control_points (:375-409)
    cws = [[0.0] * 3 for _ in range(4)]
    for i in range(n):
        for j in range(3):
            cws[0][j] = cws[0][j] + pws[i][j]
    for j in range(3):
        cws[0][j] = dv(cws[0][j], fn)
    PW0 = [[pws[i][j] - cws[0][j] for j in range(3)] for i in range(n)]
    pw0tpw0 = mul_transposed(lambda k: PW0[k], n, 3)
    uct = [[pw0tpw0[k][i] for k in range(3)] for i in range(3)]
    dc, _ = jacobi_svd(uct, 3, 3, True, ev)
    for i in range(1, 4):
        k = sq(dv(dc[i - 1], fn))
        for j in range(3):
            cws[i][j] = cws[0][j] + k * uct[i - 1][j]
    # compute_barycentric_coordinates (:411-434)
    cc = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
    ci = invert3(cc, ev)
    alphas = []
    for i in range(n):
        pi = pws[i]
        a = [0.0] * 4
        for j in range(3):
            a[1 + j] = (ci[j][0] * (pi[0] - cws[0][0]) + ci[j][1] * (pi[1] - cws[0][1]) +
                        ci[j][2] * (pi[2] - cws[0][2]))
        a[0] = 1.0 - a[1] - a[2] - a[3]
        alphas.append(a)

    # fill_M (:436-451), cvMulTransposed, cvSVD (:482-494)
    def m_row(r):
        a = alphas[r >> 1]
        u, v = us[r >> 1]
        out = [0.0] * 12
        for i in range(4):
            if r & 1:
                out[3 * i], out[3 * i + 1], out[3 * i + 2] = 0.0, a[i] * fv, a[i] * (vc - v)
            else:
                out[3 * i], out[3 * i + 1], out[3 * i + 2] = a[i] * fu, 0.0, a[i] * (uc - u)
        return out
    mtm = mul_transposed(m_row, 2 * n, 12, tree=variant == "tree_mtm")
    ut = [[mtm[k][i] for k in range(12)] for i in range(12)]
    d, vt12 = jacobi_svd(ut, 12, 12, variant == "v_for_u", ev)
    if _KEEP[0] is not None:
        _KEEP[0].append(dict(n=n, pw0tpw0=pw0tpw0, dc=list(dc), mtm=mtm, d=list(d),
                             ut=[list(r) for r in ut]))
    if variant == "v_for_u":
        ut = vt12
    # compute_L_6x10 (:760-800), compute_rho (:802-810)
    v = [ut[11], ut[10], ut[9], ut[8]]
    dvv = [[None] * 6 for _ in range(4)]
    for i in range(4):
        a, b = 0, 1
        for j in range(6):
            dvv[i][j] = [v[i][3 * a] - v[i][3 * b], v[i][3 * a + 1] - v[i][3 * b + 1],
                         v[i][3 * a + 2] - v[i][3 * b + 2]]
            b += 1
            if b > 3:
                a += 1
                b = a + 1
    L = []
    for i in range(6):
        L.append([dot3(dvv[0][i], dvv[0][i]), 2.0 * dot3(dvv[0][i], dvv[1][i]),
                  dot3(dvv[1][i], dvv[1][i]), 2.0 * dot3(dvv[0][i], dvv[2][i]),
                  2.0 * dot3(dvv[1][i], dvv[2][i]), dot3(dvv[2][i], dvv[2][i]),
                  2.0 * dot3(dvv[0][i], dvv[3][i]), 2.0 * dot3(dvv[1][i], dvv[3][i]),
                  2.0 * dot3(dvv[2][i], dvv[3][i]), dot3(dvv[3][i], dvv[3][i])])
    rho = [dist2(cws[0], cws[1]), dist2(cws[0], cws[2]), dist2(cws[0], cws[3]),
           dist2(cws[1], cws[2]), dist2(cws[1], cws[3]), dist2(cws[2], cws[3])]

    def r_and_t(betas):
        # compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
        ccs = [[0.0] * 3 for _ in range(4)]
        for i in range(4):
            vv = ut[11 - i]
            for j in range(4):
                for k in range(3):
                    ccs[j][k] = ccs[j][k] + betas[i] * vv[3 * j + k]
        pcs = [[a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j]
                for j in range(3)] for a in alphas]
        if pcs[0][2] < 0.0:
            ev.add("sign_flipped")
            pcs = [[-c for c in p] for p in pcs]
        else:
            ev.add("sign_kept")
        pc0, pw0 = [0.0] * 3, [0.0] * 3
        for i in range(n):
            for j in range(3):
                pc0[j] = pc0[j] + pcs[i][j]
                pw0[j] = pw0[j] + pws[i][j]
        for j in range(3):
            pc0[j] = dv(pc0[j], fn)
            pw0[j] = dv(pw0[j], fn)
        abt = [[0.0] * 3 for _ in range(3)]
        for i in range(n):
            for j in range(3):
                for c in range(3):
                    abt[j][c] = abt[j][c] + (pcs[i][j] - pc0[j]) * (pws[i][c] - pw0[c])
        At = [[abt[k][i] for k in range(3)] for i in range(3)]
        _, Vt = jacobi_svd(At, 3, 3, True, ev)
        # abt_u[3 * i + k] = At[k][i], abt_v[3 * j + k] = Vt[k][j]
        R = [[At[0][i] * Vt[0][j] + At[1][i] * Vt[1][j] + At[2][i] * Vt[2][j] for j in range(3)]
             for i in range(3)]
        det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] +
               R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] -
               R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
        if det < 0:
            ev.add("det_negative")
            R[2] = [-R[2][0], -R[2][1], -R[2][2]]
        t = [pc0[i] - dot3(R[i], pw0) for i in range(3)]
        sum2 = 0.0
        for i in range(n):
            pw = pws[i]
            Xc = dot3(R[0], pw) + t[0]
            Yc = dot3(R[1], pw) + t[1]
            inv_Zc = dv(1.0, dot3(R[2], pw) + t[2])
            ue = uc + fu * Xc * inv_Zc
            ve = vc + fv * Yc * inv_Zc
            u, vv = us[i]
            sum2 = sum2 + sq((u - ue) * (u - ue) + (vv - ve) * (vv - ve))
        return dv(sum2, fn), R, t

    def col(idx):
        return [[L[i][c] for c in idx] for i in range(6)]
    # find_betas_approx_1 (:667-694)
    b4 = sv_bksb(col((0, 1, 3, 6)), rho, ev)
    B1 = [0.0] * 4
    if b4[0] < 0:
        B1[0] = sq(-b4[0])
        B1[1], B1[2], B1[3] = dv(-b4[1], B1[0]), dv(-b4[2], B1[0]), dv(-b4[3], B1[0])
    else:
        B1[0] = sq(b4[0])
        B1[1], B1[2], B1[3] = dv(b4[1], B1[0]), dv(b4[2], B1[0]), dv(b4[3], B1[0])
    gauss_newton(L, rho, B1, ev)
    rep = [None, r_and_t(B1)]
    # find_betas_approx_2 (:699-726)
    b3 = sv_bksb(col((0, 1, 2)), rho, ev)
    B2 = [0.0] * 4
    if b3[0] < 0:
        B2[0] = sq(-b3[0])
        B2[1] = sq(-b3[2]) if b3[2] < 0 else 0.0
    else:
        B2[0] = sq(b3[0])
        B2[1] = sq(b3[2]) if b3[2] > 0 else 0.0
    if b3[1] < 0:
        B2[0] = -B2[0]
    gauss_newton(L, rho, B2, ev)
    rep.append(r_and_t(B2))
    # find_betas_approx_3 (:731-758)
    b5 = sv_bksb(col((0, 1, 2, 3, 4)), rho, ev)
    B3 = [0.0] * 4
    if b5[0] < 0:
        B3[0] = sq(-b5[0])
        B3[1] = sq(-b5[2]) if b5[2] < 0 else 0.0
    else:
        B3[0] = sq(b5[0])
        B3[1] = sq(b5[2]) if b5[2] > 0 else 0.0
    if b5[1] < 0:
        B3[0] = -B3[0]
    B3[2] = dv(b5[3], B3[0])
    gauss_newton(L, rho, B3, ev)
    rep.append(r_and_t(B3))
    N = 1
    if rep[2][0] < rep[1][0]:
        N = 2
    if rep[3][0] < rep[N][0]:
        N = 3
    ev.add(f"approx_{N}")
    return rep[N][1], rep[N][2]


def check_inliers(R, t, corr, K, max_err, ev):
    """CheckInliers (:308-339) in its types -> N bools"""
    fu, fv, uc, vc = K
    out = np.zeros(len(corr), np.uint8)
    with np.errstate(all="ignore"):
        for i in range(len(corr)):
            x, y, z = (float(c) for c in corr["X"][i])
            Xc = f32(R[0][0] * x + R[0][1] * y + R[0][2] * z + t[0])
            Yc = f32(R[1][0] * x + R[1][1] * y + R[1][2] * z + t[1])
            invZc = f32(dv(1.0, R[2][0] * x + R[2][1] * y + R[2][2] * z + t[2]))
            if math.isinf(float(invZc)):
                ev.add("inf_invz")
            ue = uc + fu * float(Xc) * float(invZc)
            ve = vc + fv * float(Yc) * float(invZc)
            distX = f32(float(corr["u"][i]) - ue)
            distY = f32(float(corr["v"][i]) - ve)
            error2 = f32(f32(distX * distX) + f32(distY * distY))
            out[i] = 1 if error2 < max_err[i] else 0
    return out


def tcw_of(R, t):
    T = np.zeros((4, 4), f32)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                T[i, j] = f32(R[i][j])
            T[i, 3] = f32(t[i])
    T[3, 3] = 1
    return T.reshape(16)


# ---- the host helpers --------------------------------------------------------------------------------

def _cvtt(v):
    """cvttss2si / cvttsd2si: NaN and everything outside int's range give INT_MIN."""
    v = float(v)
    return int(v) if -2147483649.0 < v < 2147483648.0 else INT_MIN


def _pow3(e):
    try:
        return math.pow(e, 3.0)
    except OverflowError:
        return math.copysign(INF, e)


def _log(x):
    if x != x or x < 0:
        return NAN
    return -INF if x == 0 else math.log(x)


def ransac_parameters(prob, min_inliers, max_its, min_set, epsilon, N):
    """SetRansacParameters (:121-152) -> (mRansacMinInliers, mRansacMaxIts)"""
    with np.errstate(all="ignore"):
        eps = f32(epsilon)
        n_min = max(_cvtt(f32(N) * eps), min_inliers, min_set)
        ratio = f32(n_min) / f32(N)
        if eps < ratio:
            eps = ratio
        if n_min == N:
            n_it = 1
        else:
            q = dv(_log(1 - prob), _log(1 - _pow3(float(eps))))
            n_it = _cvtt(math.ceil(q) if math.isfinite(q) else q)
    return n_min, max(1, min(n_it, max_its))


def sample_quads(N, rand_values):
    """:188-201 -> (n_its, 4) int32"""
    r = np.asarray(rand_values, np.int64).reshape(-1, 4)
    out = np.zeros((len(r), 4), np.int32)
    for it in range(len(r)):
        avail = list(range(N))
        for i in range(4):
            randi = int((float(r[it, i]) / (float(RAND_MAX) + 1.0)) * len(avail))
            out[it, i] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


# ---- iterate (:165-258) and Refine (:260-305) ----------------------------------------------------

def refusal(case_job, corr, quads, state, best, max_n=None, max_call=None):
    """What orbx_pnp_iterate refuses of one job with its own arrays (offsets 0)."""
    J = case_job
    N, nm = int(J["N"]), int(J["n_matches"])
    r = 0
    if not 1 <= int(J["nlevels"]) <= 16:
        r |= PNP_REFUSED_OCTAVE
    w = pnp_window(J["max_its"], state["iterations"], J["n_iterations"])
    if (N < 0 or nm < 0 or J["max_its"] < 1 or J["min_inliers"] < 1 or state["iterations"] < 0 or
            state["best_inliers"] < 0 or (max_n is not None and N > max_n) or
            (max_call is not None and w > max_call)):
        return r | PNP_REFUSED_LIMIT
    if r:
        return r
    if (corr["octave"] < 0).any() or (corr["octave"] >= J["nlevels"]).any():
        r |= PNP_REFUSED_OCTAVE
    i = corr["i"].astype(np.int64)
    if (i < 0).any() or (i >= nm).any() or (np.diff(i) <= 0).any():
        r |= PNP_REFUSED_I
    if state["best_inliers"] > 0 and int(np.count_nonzero(best)) != int(state["best_inliers"]):
        r |= PNP_REFUSED_LIMIT
    if N >= J["min_inliers"]:
        q = quads[int(state["iterations"]):int(state["iterations"]) + w]
        if (q < 0).any() or (q >= N).any() or any(len(set(row)) != 4 for row in q.tolist()):
            r |= PNP_REFUSED_QUAD
    return r


def iterate(J, corr, quads, state, best, variant=None):
    """One iterate(J.n_iterations) call.  state = dict(iterations, best_inliers, best_Tcw) and
    best (N bytes) are updated in place.  -> dict(found, source, iteration, n_run, n_inliers,
    no_more, info, best_inliers, Tcw, inliers (n_matches bytes or None), trace)."""
    N, nm = int(J["N"]), int(J["n_matches"])
    K = (float(J["fx"]), float(J["fy"]), float(J["cx"]), float(J["cy"]))
    min_in, max_its, n_it = int(J["min_inliers"]), int(J["max_its"]), int(J["n_iterations"])
    with np.errstate(all="ignore"):
        max_err = [f32(J["sigma2"][o]) * f32(J["th2"]) for o in corr["octave"]]
    pws = [[float(c) for c in corr["X"][i]] for i in range(N)]
    us = [[float(corr["u"][i]), float(corr["v"][i])] for i in range(N)]
    out = dict(found=0, source=0, iteration=0, n_run=0, n_inliers=0, no_more=0, info=0,
               best_inliers=state["best_inliers"], Tcw=np.zeros(16, f32), inliers=None, trace=[])
    if N < min_in:                                         # :173-177
        out["no_more"] = 1
        out["trace"].append(dict(exit="small_n"))
        return out
    refines = 0
    flags = set()
    cur = 0
    from_call = False        # mvbBestInliers was written in this call

    def cont():
        a, b = state["iterations"] < max_its, cur < n_it
        return (a and b) if variant == "and_for_or" else (a or b)

    def vb(mask):
        v = np.zeros(nm, np.uint8)
        v[corr["i"][np.flatnonzero(mask)]] = 1
        return v

    def info():
        return (refines | (PNP_QR_SINGULAR if "qr_singular" in flags else 0) |
                (PNP_SVD_COMPLETED if "svd_completed" in flags else 0))
    while cont():
        cur += 1
        state["iterations"] += 1
        ev = set()
        q = quads[state["iterations"] - 1]
        R, t = compute_pose([pws[k] for k in q], [us[k] for k in q], K, ev, variant)
        mask = check_inliers(R, t, corr, K, max_err, ev)
        cnt = int(mask.sum())
        tr = dict(exit="continue", count=cnt, hyp=set(ev))
        out["trace"].append(tr)
        flags |= ev
        out["n_run"] = cur
        if cnt > min_in if variant == "gt_entry" else cnt >= min_in:
            improved = cnt >= state["best_inliers"] if variant == "ge_best" else \
                cnt > state["best_inliers"]
            if improved:
                best[:] = mask
                state["best_inliers"] = cnt
                state["best_Tcw"] = tcw_of(R, t)
            tr["improved"] = improved
            # Refine (:260-305) on mvbBestInliers
            sel = np.flatnonzero(mask if variant == "refine_current" else best)
            ev2 = set()
            R2, t2 = compute_pose([pws[k] for k in sel], [us[k] for k in sel], K, ev2, variant)
            mask2 = check_inliers(R2, t2, corr, K, max_err, ev2)
            cnt2 = int(mask2.sum())
            refines += 1
            flags |= ev2
            tr.update(refine=set(ev2), refine_n=len(sel), refine_count=cnt2,
                      carried=not improved and not from_call)
            from_call = from_call or improved
            if cnt2 >= min_in if variant == "ge_refine" else cnt2 > min_in:
                tr["exit"] = "refined"
                out.update(found=1, source=1, iteration=state["iterations"], n_inliers=cnt2,
                           Tcw=tcw_of(R2, t2), inliers=vb(mask2), info=info(),
                           best_inliers=state["best_inliers"])
                return out
    out["best_inliers"] = state["best_inliers"]
    out["info"] = info()
    if state["iterations"] >= max_its:                     # :241-255
        out["no_more"] = 1
        if state["best_inliers"] > min_in if variant == "gt_end" else \
                state["best_inliers"] >= min_in:
            out.update(found=1, source=2, iteration=state["iterations"],
                       n_inliers=state["best_inliers"], Tcw=np.array(state["best_Tcw"], f32),
                       inliers=vb(best))
            out["trace"].append(dict(exit="best_at_end"))
            return out
    out["trace"].append(dict(exit="none"))
    return out


def solve(case, variant=None):
    """Every call of the case -> dict(min_inliers, max_its, quads, calls=[...])."""
    corr = case["corr"]
    N = len(corr)
    min_in, max_its = ransac_parameters(case["prob"], case["min_inliers"], case["max_iterations"],
                                        4, case["epsilon"], N)
    quads = sample_quads(N, case["rand"]) if N >= 4 else np.zeros((len(case["rand"]) // 4, 4),
                                                                  np.int32)
    for q, v in case.get("quad_edits", {}).items():
        quads[q] = v
    state = dict(iterations=case["state0"][0], best_inliers=case["state0"][1],
                 best_Tcw=np.array(case["best_Tcw0"], f32))
    best = np.array(case["best0"], np.uint8)
    calls = []
    for n_it in case["calls"]:
        J = job_of(case, min_in, max_its, n_it)
        assert refusal(J, corr, quads, state, best) == 0, case["name"]
        _UNSORTED[0] = variant == "unsorted_w"
        try:
            c = iterate(J, corr, quads, state, best, variant)
        finally:
            _UNSORTED[0] = False
        c["state"] = (state["iterations"], state["best_inliers"],
                      np.array(state["best_Tcw"], f32).copy())
        c["best"] = best.copy()
        calls.append(c)
    return dict(min_inliers=min_in, max_its=max_its, quads=quads, calls=calls)


def svd_records(case):
    """The matrices of every compute_pose of the case (hypotheses and Refines): dicts of n,
    pw0tpw0, dc, mtm, d, ut."""
    _KEEP[0] = []
    try:
        solve(case)
        return _KEEP[0]
    finally:
        _KEEP[0] = None


def find(case):
    """find() (:159-163) of a fresh solver on the case's correspondences -> the call's dict."""
    one = dict(case, calls=[None], state0=(0, 0), best0=np.zeros(len(case["corr"]), np.uint8),
               best_Tcw0=np.zeros(16, f32))
    _, max_its = ransac_parameters(case["prob"], case["min_inliers"], case["max_iterations"], 4,
                                   case["epsilon"], len(case["corr"]))
    one["calls"] = [max_its]
    return solve(one)["calls"][0]


def job_of(case, min_in, max_its, n_it, **off):
    return pnp_job(case["K4"], case["sigma2"], case["th2"], case["n_matches"], len(case["corr"]),
                   min_in, max_its, n_it, **off)


def result_record(call):
    r = np.zeros(1, PNP_RESULT_DTYPE)
    for k in ("found", "source", "iteration", "n_run", "n_inliers", "no_more", "info",
              "best_inliers"):
        r[k] = call[k]
    r["Tcw"] = call["Tcw"]
    return r


def state_record(call):
    s = np.zeros(1, PNP_STATE_DTYPE)
    s["iterations"], s["best_inliers"], s["best_Tcw"] = call["state"]
    return s


def canon(record_bytes):
    """A result or state record's bytes with every NaN float of its trailing 16 floats replaced by
    one NaN: NaN equals NaN."""
    w = np.frombuffer(bytes(record_bytes), np.uint32).copy()
    fl = w[-16:]
    fl[(fl & 0x7fffffff) > 0x7f800000] = 0x7fc00000
    return w.tobytes()


def key(result):
    """Everything observable of a solve(), as bytes."""
    out = b""
    for c in result["calls"]:
        out += canon(result_record(c).tobytes()) + canon(state_record(c).tobytes())
        out += c["best"].tobytes() + (c["inliers"].tobytes() if c["inliers"] is not None else b"-")
    return out


def expected_inliers(case, call):
    """The n_matches inlier bytes after the call when they held SENTINEL before."""
    if call["inliers"] is None:
        return np.full(case["n_matches"], SENTINEL, np.uint8)
    return call["inliers"]


@functools.lru_cache(maxsize=None)
def _reference_cached(name):
    return solve(case_named(name))


def reference(case):
    return _reference_cached(case["name"])


# ---- the cases ------------------------------------------------------------------------------------------

K4 = (520.0, 515.0, 325.5, 250.25)
SIGMA2 = np.array([1.2 ** (2 * k) for k in range(8)], f32)


def _pose(rng):
    """A camera pose with the scene in front of it: a rotation of up to ~25 degrees, a shift."""
    w = rng.normal(size=3)
    w = w / np.linalg.norm(w) * rng.uniform(0.05, 0.45)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx
    return R, rng.uniform(-0.5, 0.5, size=3)


def scene(seed, N, outliers=0, noise=0.0, n_matches=None, depth=(2.0, 8.0)):
    """N correspondences of a non-coplanar scene 2-8 m in front of a camera: -> (corr, R, t,
    n_matches).  The first `outliers` image points are moved by 30-60 px."""
    rng = np.random.default_rng(seed)
    R, t = _pose(rng)
    fx, fy, cx, cy = K4
    z = rng.uniform(depth[0], depth[1], size=N)
    u = rng.uniform(40, 600, size=N)
    v = rng.uniform(40, 440, size=N)
    Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    Pw = (Pc - t) @ R                         # R^T (Pc - t)
    n_matches = n_matches or N + 7
    corr = np.zeros(N, PNP_CORR_DTYPE)
    corr["i"] = np.sort(rng.choice(n_matches, size=N, replace=False))
    corr["X"] = Pw.astype(f32)
    # the image points of the rounded world points, so that "exact" data is exact to float
    Pc2 = corr["X"].astype(np.float64) @ R.T + t
    uv = np.stack([fx * Pc2[:, 0] / Pc2[:, 2] + cx, fy * Pc2[:, 1] / Pc2[:, 2] + cy], axis=1)
    uv += rng.normal(size=uv.shape) * noise
    sgn = rng.choice([-1.0, 1.0], size=(N, 2))
    uv[:outliers] += sgn[:outliers] * rng.uniform(30, 60, size=(outliers, 2))
    corr["u"], corr["v"] = uv[:, 0].astype(f32), uv[:, 1].astype(f32)
    corr["octave"] = rng.integers(0, len(SIGMA2), size=N)
    return corr, R, t, n_matches


def _case(name, corr, n_matches, calls, seed=1, min_inliers=8, max_iterations=35, epsilon=0.5,
          prob=0.99, th2=5.991, state0=(0, 0), best0=None, best_Tcw0=None, n_rand=None, R=None,
          t=None, quad_edits=None, rand=None, exact=False):
    rng = np.random.default_rng(1000 + seed)
    n_rand = n_rand or 4 * (max_iterations + sum(calls) + 8)
    return dict(name=name, corr=corr, n_matches=n_matches, calls=list(calls), K4=K4, sigma2=SIGMA2,
                th2=th2, prob=prob, min_inliers=min_inliers, max_iterations=max_iterations,
                epsilon=epsilon, state0=state0,
                best0=np.zeros(len(corr), np.uint8) if best0 is None else best0,
                best_Tcw0=np.zeros(16, f32) if best_Tcw0 is None else best_Tcw0,
                rand=rng.integers(0, RAND_MAX, size=n_rand, endpoint=True).astype(np.int32)
                if rand is None else rand, R=R, t=t, quad_edits=quad_edits or {}, exact=exact)


def _scene_case(name, seed, N, calls, outliers=0, noise=0.0, **kw):
    corr, R, t, nm = scene(seed, N, outliers, noise)
    return _case(name, corr, nm, calls, seed=seed, R=R, t=t, **kw)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = []
    # exact scenes of the GPU test's sizes; find() must give the generating pose
    for N, seed in ((10, 11), (15, 12), (40, 13), (64, 14), (65, 15), (130, 16)):
        cases.append(_scene_case(f"exact_{N}", seed, N, [5, 5], exact=True))
    # outliers and noise: later returns, failed Refines, several calls
    cases.append(_scene_case("outliers_40", 21, 40, [5, 5, 5], outliers=14, noise=0.3))
    cases.append(_scene_case("outliers_65", 22, 65, [4, 40], outliers=30, noise=0.5))
    cases.append(_scene_case("outliers_130", 23, 130, [5, 5], outliers=60, noise=0.4))
    # all noise: no model at all, through the loop end
    c, R, t, nm = scene(24, 15, outliers=15)
    c["u"] = np.random.default_rng(5).uniform(0, 640, 15).astype(f32)
    c["v"] = np.random.default_rng(6).uniform(0, 480, 15).astype(f32)
    cases.append(_case("no_model", c, nm, [5, 5], seed=24))
    # N == min_inliers with exact data: one iteration, Refine's count equals min_inliers, so it
    # fails, and the loop end returns mBestTcw
    corr, R, t, nm = scene(31, 8)
    cases.append(_case("n_equals_min", corr, nm, [5], seed=31, R=R, t=t))
    # the minimal set: N == 4 == min_inliers
    corr, R, t, nm = scene(32, 4)
    cases.append(_case("n_is_4", corr, nm, [1], seed=32, min_inliers=4, R=R, t=t))
    # N < min_inliers
    corr, R, t, nm = scene(33, 7)
    cases.append(_case("n_below_min", corr, nm, [5, 5], seed=33))
    # a second call after an early success: window max(max_its - iterations, n), Refine on the
    # carried best set
    cases.append(_scene_case("returned_then_again", 41, 40, [3, 2, 0], outliers=10, noise=0.2))
    # a state carried in from an earlier run whose best set is as large as the inlier set but
    # holds four outliers: an equal count does not replace it, and Refine runs on the carried set
    corr, R, t, nm = scene(42, 20, outliers=8, noise=0.1)
    best0 = np.zeros(20, np.uint8)
    best0[4:16] = 1
    T0 = np.eye(4, dtype=f32)
    T0[:3, :3], T0[:3, 3] = R.astype(f32), t.astype(f32)
    cases.append(_case("carried_best", corr, nm, [3, 3], seed=42, state0=(30, 12), best0=best0,
                       best_Tcw0=T0.reshape(16)))
    # four points with equal z in the minimal set: the SVD completion path
    corr, R, t, nm = scene(51, 15)
    corr["X"][:4, 2] = f32(1.5)
    cases.append(_case("equal_z_quad", corr, nm, [2], seed=51,
                       quad_edits={0: [0, 1, 2, 3], 1: [3, 2, 1, 0]}))
    # equal x instead: the zero row is the first, and the sort has to move it
    corr, R, t, nm = scene(57, 15)
    corr["X"][:4, 0] = f32(-0.75)
    cases.append(_case("equal_x_quad", corr, nm, [2], seed=57, quad_edits={0: [0, 1, 2, 3]}))
    # the same with a bound so wide that the degenerate hypothesis counts every point: it becomes
    # the best model, and mBestTcw shows what the sort did
    corr, R, t, nm = scene(57, 15)
    corr["X"][:4, 0] = f32(-0.75)
    cases.append(_case("equal_x_wide", corr, nm, [2], seed=57, th2=1e30,
                       quad_edits={0: [0, 1, 2, 3]}))
    # four identical points: every matrix is zero, qr_solve's singular exit, NaN through the pose
    corr, R, t, nm = scene(52, 15)
    corr["X"][:4] = corr["X"][0]
    corr["u"][:4], corr["v"][:4] = corr["u"][0], corr["v"][0]
    cases.append(_case("identical_quad", corr, nm, [2], seed=52, quad_edits={0: [0, 1, 2, 3]}))
    # a scene of 1e-40 m: every depth is below 1 / FLT_MAX, an infinite invZc
    corr, R, t, nm = scene(53, 15)
    corr["X"] = (corr["X"].astype(np.float64) * 1e-40).astype(f32)
    cases.append(_case("tiny_scene", corr, nm, [3], seed=53))
    # collinear world points in the minimal set: a skipped SVBkSb term
    corr, R, t, nm = scene(54, 15)
    for k in range(1, 4):
        corr["X"][k] = corr["X"][0] + f32(k) * np.array([0.25, 0.5, -0.125], f32)
    cases.append(_case("collinear_quad", corr, nm, [2], seed=54, quad_edits={0: [0, 1, 2, 3]}))
    # a mirrored scene: det < 0
    corr, R, t, nm = scene(55, 15)
    corr["u"] = f32(2 * K4[2]) - corr["u"]
    cases.append(_case("mirrored", corr, nm, [5], seed=55))
    # points behind the camera: solve_for_sign flips
    corr, R, t, nm = scene(56, 15, depth=(-8.0, -2.0))
    cases.append(_case("behind", corr, nm, [5], seed=56))
    return tuple(cases)


def case_named(name):
    for c in all_cases():
        if c["name"] == name:
            return c
    raise KeyError(name)


def solver_of(case, parameters=True):
    """A PnPsolver over a frame whose matched slots are the case's correspondences, with the case's
    RANSAC parameters or the class defaults."""
    from my_orb_slam2_amd import KEYPOINT_DTYPE, PnPsolver
    c = case
    nm = c["n_matches"]
    keys = np.zeros(nm, KEYPOINT_DTYPE)
    pts, valid = np.zeros((nm, 3), f32), np.zeros(nm, bool)
    i = c["corr"]["i"]
    valid[i], pts[i] = True, c["corr"]["X"]
    keys["x"][i], keys["y"][i], keys["octave"][i] = c["corr"]["u"], c["corr"]["v"], c["corr"]["octave"]
    s = PnPsolver(c["K4"], keys, c["sigma2"], pts, valid, c["rand"])
    assert np.array_equal(s.corr, c["corr"])
    if parameters:
        s.SetRansacParameters(c["prob"], c["min_inliers"], c["max_iterations"], 4, c["epsilon"],
                              c["th2"])
    return s


# ---- a small synthetic map for the relocalisation chain ---------------------------------------------

def small_map(seed, n_frame=220, shared=(48, 60, 72, 6), n_kf=150):
    """One frame with a pose, and keyframes whose first features copy descriptors and angles of
    frame features and carry the MapPoints those frame features see."""
    from my_orb_slam2_amd import synth
    from my_orb_slam2_amd.features import MAP_POINT_DTYPE, feature_vector
    from my_orb_slam2_amd.synth import _node_of
    rng = np.random.default_rng(seed)
    frame = synth.feature_pair(seed, n1=n_frame, n2=10)[0]
    corr, R, t, _ = scene(seed + 1, n_frame)
    frame.keys["x"], frame.keys["y"] = corr["u"], corr["v"]
    frame.keys["octave"] = corr["octave"]
    frame.fvec = feature_vector(_node_of(frame.desc, 40))
    kfs, valids, mps = [], [], []
    for k, m in enumerate(shared):
        kf = synth.feature_pair(seed + 10 + k, n1=10, n2=n_kf)[1]
        src = rng.choice(n_frame, m, replace=False)
        kf.desc[:m] = frame.desc[src]
        kf.keys["angle"][:m] = frame.keys["angle"][src]
        kf.fvec = feature_vector(_node_of(kf.desc, 40))
        mp = np.zeros(kf.n, MAP_POINT_DTYPE)
        mp["pos"] = rng.normal(size=(kf.n, 3)).astype(f32) * 3
        mp["pos"][:m] = corr["X"][src]
        mp["min_dist"], mp["max_dist"] = 0.1, 100.0
        kfs.append(kf), valids.append(np.ones(kf.n, bool)), mps.append(mp)
    return frame, R, t, kfs, valids, mps


# ---- the exchange with tests/native/pnp_ref.cpp -------------------------------------------------------

def write_cases(path, cases):
    """int32 ncases; per case: int32 N, n_matches, ncalls, nquads; the job record (n_iterations of
    call 0); int32 n_iterations[ncalls]; the state record; N best bytes; N corr records; 4 *
    nquads int32."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            r = reference(c)
            q = r["quads"]
            f.write(struct.pack("<iiii", len(c["corr"]), c["n_matches"], len(c["calls"]), len(q)))
            f.write(job_of(c, r["min_inliers"], r["max_its"], c["calls"][0]).tobytes())
            f.write(np.asarray(c["calls"], np.int32).tobytes())
            s = np.zeros(1, PNP_STATE_DTYPE)
            s["iterations"], s["best_inliers"], s["best_Tcw"] = c["state0"] + (c["best_Tcw0"],)
            f.write(s.tobytes())
            f.write(c["best0"].tobytes())
            f.write(c["corr"].tobytes())
            f.write(np.ascontiguousarray(q, np.int32).tobytes())


def read_results(path, cases):
    """Per case, per call: (result bytes, inlier bytes (SENTINEL where untouched), state bytes,
    best bytes)."""
    data = open(path, "rb").read()
    o = 0
    out = []
    for c in cases:
        per = []
        for _ in c["calls"]:
            parts = []
            for n in (PNP_RESULT_DTYPE.itemsize, c["n_matches"], PNP_STATE_DTYPE.itemsize,
                      len(c["corr"])):
                parts.append(data[o:o + n])
                o += n
            per.append(tuple(parts))
        out.append(per)
    assert o == len(data)
    return out
