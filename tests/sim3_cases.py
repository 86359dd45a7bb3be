"""Sim3Solver (src/Sim3Solver.cc) restated literally in numpy, and the cases orbx_sim3_* is checked
on (tests/test_sim3_cases.py on the CPU against tests/native/sim3_ref.cpp, tests/test_gpu_sim3.py
on the GPU).

Floats are np.float32 scalars and doubles np.float64 scalars, one rounding per operation; no
Python float takes part in an operation.  The forms evaluated inside OpenCV 3.2 are restated as
DESIGN.md §2 lists them (PARITY UNPINNED); cv::eigen's Jacobi is `jacobi_eigen`, a restatement of
its own.  atan2 / sin / cos are transliterations of orbx_atan2_f64 / orbx_sincos_f64
(csrc/orbx_math.h).

`solve(case, variant)` runs the case's sequence of iterate() calls and returns, per call, what
orbx_sim3_iterate leaves, with a decision trace per iteration.  `variant` flips one decision
(VARIANTS); each flip changes the result of at least one committed case."""
import functools
import struct

import numpy as np

from my_orb_slam2_amd.features import FRAME_POSE_DTYPE, frame_pose
from my_orb_slam2_amd.sim3 import (RAND_MAX, SIM3_CORR_DTYPE, SIM3_RESULT_DTYPE, SIM3_STATE_DTYPE,
                                   sim3_job)
from poseopt_cases import sincos_f64

f32, f64 = np.float32, np.float64
DBL_EPS = f64(2.220446049250313e-16)
FLT_EPS = f32(1.1920928955078125e-07)
SENTINEL = 0xCC
INT_MIN = -2147483648

VARIANTS = ("float_bounds", "ge_min", "gt_best", "double_epsilon", "reduce_012", "small_gemm_M",
            "unsorted", "float_norm", "s12_double", "redraw", "no_small_n_exit",
            "inliers_by_corr")


# ---- orbx_atan2_f64 ---------------------------------------------------------------------------

def _words(v):
    u = struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    hi, lo = u >> 32, u & 0xffffffff
    return (hi - (1 << 32) if hi & 0x80000000 else hi), lo


def atan_f64(x):
    """orbx_atan_f64, operation for operation."""
    x = f64(x)
    hi = (f64(4.63647609000806093515e-01), f64(7.85398163397448278999e-01),
          f64(9.82793723247329054082e-01), f64(1.57079632679489655800e+00))
    lo = (f64(2.26987774529616870924e-17), f64(3.06161699786838301793e-17),
          f64(1.39033110312309984516e-17), f64(6.12323399573676603587e-17))
    aT = [f64(v) for v in (
        3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01,
        -1.11111104054623557880e-01, 9.09088713343650656196e-02, -7.69187620504482999495e-02,
        6.66107313738753120669e-02, -5.83357013379057348645e-02, 4.97687799461593236017e-02,
        -3.65315727442169155270e-02, 1.62858201153657823623e-02)]
    hx, lx = _words(x)
    ix = hx & 0x7fffffff
    one, two = f64(1.0), f64(2.0)
    if ix >= 0x44100000:
        if ix > 0x7ff00000 or (ix == 0x7ff00000 and lx != 0):
            return x + x
        return hi[3] + lo[3] if hx > 0 else -hi[3] - lo[3]
    if ix < 0x3fdc0000:
        if ix < 0x3e200000:
            return x
        idn = -1
    else:
        x = abs(x)
        if ix < 0x3ff30000:
            if ix < 0x3fe60000:
                idn, x = 0, (two * x - one) / (two + x)
            else:
                idn, x = 1, (x - one) / (x + one)
        else:
            if ix < 0x40038000:
                idn, x = 2, (x - f64(1.5)) / (one + f64(1.5) * x)
            else:
                idn, x = 3, f64(-1.0) / x
    z = x * x
    w = z * z
    s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))))
    s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))))
    if idn < 0:
        return x - x * (s1 + s2)
    r = hi[idn] - ((x * (s1 + s2) - lo[idn]) - x)
    return -r if hx < 0 else r


def atan2_f64(y, x):
    """orbx_atan2_f64, operation for operation."""
    y, x = f64(y), f64(x)
    tiny, pi_o_4, pi_o_2 = f64(1.0e-300), f64(7.8539816339744827900E-01), f64(1.5707963267948965580E+00)
    pi, pi_lo = f64(3.1415926535897931160E+00), f64(1.2246467991473531772E-16)
    hx, lx = _words(x)
    hy, ly = _words(y)
    ix, iy = hx & 0x7fffffff, hy & 0x7fffffff
    if ix + (lx != 0) > 0x7ff00000 or iy + (ly != 0) > 0x7ff00000:
        return x + y
    if hx == 0x3ff00000 and lx == 0:
        return atan_f64(y)
    m = ((hy >> 31) & 1) | ((hx >> 30) & 2)
    if (iy | ly) == 0:
        if m < 2:
            return y
        return pi + tiny if m == 2 else -pi - tiny
    if (ix | lx) == 0:
        return -pi_o_2 - tiny if hy < 0 else pi_o_2 + tiny
    if ix == 0x7ff00000:
        if iy == 0x7ff00000:
            return (pi_o_4 + tiny, -pi_o_4 - tiny, f64(3.0) * pi_o_4 + tiny,
                    f64(-3.0) * pi_o_4 - tiny)[m]
        return (f64(0.0), f64(-0.0), pi + tiny, -pi - tiny)[m]
    if iy == 0x7ff00000:
        return -pi_o_2 - tiny if hy < 0 else pi_o_2 + tiny
    k = (iy - ix) >> 20
    if k > 60:
        z = pi_o_2 + f64(0.5) * pi_lo
    elif hx < 0 and k < -60:
        z = f64(0.0)
    else:
        z = atan_f64(abs(y / x))
    if m == 0:
        return z
    if m == 1:
        return -z
    if m == 2:
        return pi - (z - pi_lo)
    return (z - pi_lo) - pi


# ---- the two host helpers ---------------------------------------------------------------------

def ransac_iterations_np(prob, min_inliers, max_its, N, variant=None):
    """SetRansacParameters (:114-138) -> mRansacMaxIts."""
    with np.errstate(all="ignore"):
        if variant == "double_epsilon":
            eps = f64(min_inliers) / f64(N)
        else:
            eps = f64(f32(min_inliers) / f32(N))
        if min_inliers == N:
            n = 1
        else:
            v = np.ceil(np.log(f64(1) - f64(prob)) / np.log(f64(1) - np.power(eps, f64(3))))
            n = int(v) if (v > -2147483649.0 and v < 2147483648.0) else INT_MIN
    return max(1, min(n, max_its))


def sample_triples_np(N, rand_values, variant=None):
    """:163-177 over raw rand() values, with the list written out."""
    r = np.asarray(rand_values, np.int64).reshape(-1, 3)
    out = np.zeros((len(r), 3), np.int32)
    for it in range(len(r)):
        avail = list(range(N))
        for i in range(3):
            if variant == "redraw":      # a draw over all N; a repeat moves on to the next index
                idx = int(f64(r[it, i]) / (f64(RAND_MAX) + f64(1.0)) * f64(N))
                while idx in out[it, :i]:
                    idx = (idx + 1) % N
                out[it, i] = idx
                continue
            randi = int(f64(r[it, i]) / (f64(RAND_MAX) + f64(1.0)) * f64(len(avail)))
            out[it, i] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


# ---- cv::eigen: JacobiImpl_<float> --------------------------------------------------------------

def cv_hypot(a, b):
    a, b = abs(f32(a)), abs(f32(b))
    if a > b:
        b = b / a
        return a * np.sqrt(f32(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(f32(1) + a * a)
    return f32(0)


def jacobi_eigen(N, sort=True):
    """cv::eigen of a symmetric n x n float matrix -> (eigenvalues, eigenvector rows, rotations)."""
    A = np.array(N, f32)
    n = A.shape[0]
    V = np.eye(n, dtype=f32)
    W = np.array([A[k, k] for k in range(n)], f32)
    indR, indC = [0] * n, [0] * n

    def row_max(k):
        m, mv = k + 1, abs(A[k, k + 1])
        for i in range(k + 2, n):
            if mv < abs(A[k, i]):
                mv, m = abs(A[k, i]), i
        return m

    def col_max(k):
        m, mv = 0, abs(A[0, k])
        for i in range(1, k):
            if mv < abs(A[i, k]):
                mv, m = abs(A[i, k]), i
        return m

    for k in range(n):
        if k < n - 1:
            indR[k] = row_max(k)
        if k > 0:
            indC[k] = col_max(k)
    rotations = 0
    for _ in range(n * n * 30):
        k, mv = 0, abs(A[0, indR[0]])
        for i in range(1, n - 1):
            val = abs(A[i, indR[i]])
            if mv < val:
                mv, k = val, i
        l = indR[k]
        for i in range(1, n):
            val = abs(A[indC[i], i])
            if mv < val:
                mv, k, l = val, indC[i], i
        p = A[k, l]
        if abs(p) <= FLT_EPS:
            break
        rotations += 1
        y = f32(f64(W[l] - W[k]) * f64(0.5))
        t = abs(y) + cv_hypot(p, y)
        s = cv_hypot(p, t)
        c = t / s
        s = p / s
        t = (p / t) * p
        if y < 0:
            s, t = -s, -t
        A[k, l] = 0
        W[k] = W[k] - t
        W[l] = W[l] + t

        def rot(i0, j0, i1, j1):
            a0, b0 = A[i0, j0], A[i1, j1]
            A[i0, j0] = a0 * c - b0 * s
            A[i1, j1] = a0 * s + b0 * c
        for i in range(k):
            rot(i, k, i, l)
        for i in range(k + 1, l):
            rot(k, i, i, l)
        for i in range(l + 1, n):
            rot(k, i, l, i)
        for i in range(n):
            a0, b0 = V[k, i], V[l, i]
            V[k, i] = a0 * c - b0 * s
            V[l, i] = a0 * s + b0 * c
        for idx in (k, l):
            if idx < n - 1:
                indR[idx] = row_max(idx)
            if idx > 0:
                indC[idx] = col_max(idx)
    swaps = 0
    if sort:
        for k in range(n - 1):
            m = k
            for i in range(k + 1, n):
                if W[m] < W[i]:
                    m = i
            if k != m:
                swaps += 1
                W[[m, k]] = W[[k, m]]
                V[[m, k]] = V[[k, m]]
    return W, V, rotations, swaps


# ---- ComputeSim3 (:226-337) ---------------------------------------------------------------------

def cvt_scale(x, alpha):
    """Mat::convertTo(alpha) on one CV_32F value."""
    if abs(f64(alpha) - f64(1)) < DBL_EPS:
        return f32(x)
    return f32(x) * f32(alpha) + f32(0)


def row3(A, r, b):
    t = A[r, 0] * b[0]
    t = t + A[r, 1] * b[1]
    return t + A[r, 2] * b[2]


def centroid(P, variant):
    C, Pr = np.zeros(3, f32), np.zeros((3, 3), f32)
    for r in range(3):
        if variant == "reduce_012":
            s = (P[r, 0] + P[r, 1]) + P[r, 2]
        else:
            s = (P[r, 0] + P[r, 2]) + P[r, 1]
        C[r] = cvt_scale(s, f64(1.0) / f64(3))
        for i in range(3):
            Pr[r, i] = P[r, i] - C[r]
    return Pr, C


def compute_sim3(P1, P2, fix_scale, variant=None, ev=None):
    """P1 / P2: 3x3 float32, column i = point i.  -> dict(R, t, s, sR, sRinv, tinv)."""
    ev = {} if ev is None else ev
    Pr1, O1 = centroid(P1, variant)
    Pr2, O2 = centroid(P2, variant)
    M = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            if variant == "small_gemm_M":
                t = Pr2[i, 0] * Pr1[j, 0]
                t = t + Pr2[i, 1] * Pr1[j, 1]
                M[i, j] = t + Pr2[i, 2] * Pr1[j, 2]
            else:
                s = f64(0)
                for k in range(3):
                    s = s + f64(Pr2[i, k]) * f64(Pr1[j, k])
                M[i, j] = f32(s * f64(1))
    N11 = (M[0, 0] + M[1, 1]) + M[2, 2]
    N12 = M[1, 2] - M[2, 1]
    N13 = M[2, 0] - M[0, 2]
    N14 = M[0, 1] - M[1, 0]
    N22 = (M[0, 0] - M[1, 1]) - M[2, 2]
    N23 = M[0, 1] + M[1, 0]
    N24 = M[2, 0] + M[0, 2]
    N33 = (-M[0, 0] + M[1, 1]) - M[2, 2]
    N34 = M[1, 2] + M[2, 1]
    N44 = (-M[0, 0] - M[1, 1]) + M[2, 2]
    N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34],
                  [N14, N24, N34, N44]], f32)
    W, V, rotations, swaps = jacobi_eigen(N, sort=variant != "unsorted")
    q = V[0]
    ev["zero_M"] = not M.any()
    ev["rotations"], ev["sort_swaps"] = rotations, swaps
    ev["q0_negative"], ev["q0_zero"] = bool(q[0] < 0), bool(q[0] == 0)
    ev["top_pair_equal"] = bool(W[0] == W[1])
    if variant == "float_norm":
        ss = f32(0)
        for k in (1, 2, 3):
            ss = ss + q[k] * q[k]
        nrm = f64(np.sqrt(ss))
    else:
        ss = f64(0)
        for k in (1, 2, 3):
            ss = ss + f64(q[k]) * f64(q[k])
        nrm = np.sqrt(ss)
    ang = atan2_f64(nrm, f64(q[0]))
    ev["norm_w"] = (float(nrm), float(q[0]))
    alpha = (f64(2) * ang) * (f64(1.0) / nrm)
    vec = [cvt_scale(q[k + 1], alpha) for k in range(3)]
    rx, ry, rz = f64(vec[0]), f64(vec[1]), f64(vec[2])
    theta = np.sqrt((rx * rx + ry * ry) + rz * rz)
    R = np.zeros((3, 3), f32)
    ev["rodrigues_identity"] = bool(theta < DBL_EPS)
    if theta < DBL_EPS:
        R = np.eye(3, dtype=f32)
    else:
        sc = sincos_f64(float(theta))
        s, c = (f64(np.nan), f64(np.nan)) if sc is None else (f64(sc[0]), f64(sc[1]))
        c1, itheta = f64(1) - c, f64(1) / theta
        rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
        rrt = (rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz)
        r_x = (f64(0), -rz, ry, rz, f64(0), -rx, -ry, rx, f64(0))
        for k in range(9):
            I = f64(1) if k in (0, 4, 8) else f64(0)
            R[k // 3, k % 3] = f32((c * I + c1 * rrt[k]) + s * r_x[k])
    ev["nan_rotation"] = bool(np.isnan(R).all())
    P3 = np.zeros((3, 3), f32)
    for r in range(3):
        for i in range(3):
            t = R[r, 0] * Pr2[0, i]
            t = t + R[r, 1] * Pr2[1, i]
            P3[r, i] = t + R[r, 2] * Pr2[2, i]
    if not fix_scale:
        a, b = Pr1.reshape(9), P3.reshape(9)
        nom = f64(0)
        for i in (0, 4):
            nom = nom + (((f64(a[i]) * f64(b[i]) + f64(a[i + 1]) * f64(b[i + 1])) +
                          f64(a[i + 2]) * f64(b[i + 2])) + f64(a[i + 3]) * f64(b[i + 3]))
        nom = nom + f64(a[8]) * f64(b[8])
        den = f64(0)
        for i in range(9):
            den = den + f64(b[i] * b[i])
        s_d = nom / den
        s12 = f32(s_d)
    else:
        s12 = f32(1.0)
        s_d = f64(1.0)
    ds12 = s_d if variant == "s12_double" else f64(s12)
    t12 = np.zeros(3, f32)
    for r in range(3):
        t12[r] = f32(f64(row3(R, r, O2)) * -ds12 + f64(O1[r]) * f64(1))
    ds12 = f64(s12)
    inv_s = f64(1.0) / ds12
    sR, sRinv = np.zeros((3, 3), f32), np.zeros((3, 3), f32)
    for r in range(3):
        for c_ in range(3):
            sR[r, c_] = cvt_scale(R[r, c_], ds12)
            sRinv[r, c_] = cvt_scale(R[c_, r], inv_s)
    tinv = np.zeros(3, f32)
    for r in range(3):
        tinv[r] = f32(f64(row3(sRinv, r, t12)) * f64(-1.0))
    return dict(R=R, t=t12, s=s12, sR=sR, sRinv=sRinv, tinv=tinv)


# ---- the constructor, Project, CheckInliers --------------------------------------------------------

def gemm3(R, X, t):
    """cv::gemm(R, X, 1, t, 1), small-matrix path"""
    return np.array([f32(f64(row3(R, r, X)) + f64(t[r])) for r in range(3)], f32)


def to_image(P, K):
    fx, fy, cx, cy = K
    invz = f32(1) / P[2]
    x, y = P[0] * invz, P[1] * invz
    return fx * x + cx, fy * y + cy


def max_error(sigma2, variant=None):
    v = f64(9.210) * f64(sigma2)
    if variant == "float_bounds":
        return f32(v)
    if not v >= 0:
        return f32(0)
    if v >= 18446744073709551615.0:
        return f32(18446744073709551615.0)
    return f32(int(v))


def prepare(case, variant=None):
    out = []
    p1, p2 = case["pose1"], case["pose2"]
    K1 = tuple(f32(p1[k]) for k in ("fx", "fy", "cx", "cy"))
    K2 = tuple(f32(p2[k]) for k in ("fx", "fy", "cx", "cy"))
    R1, R2 = p1["Rcw"].reshape(3, 3), p2["Rcw"].reshape(3, 3)
    for c in case["corr"]:
        X1 = gemm3(R1, c["X1w"], p1["tcw"])
        X2 = gemm3(R2, c["X2w"], p2["tcw"])
        out.append(dict(X1=X1, X2=X2, p1=to_image(X1, K1), p2=to_image(X2, K2),
                        m1=max_error(case["sigma2_1"][c["octave1"]], variant),
                        m2=max_error(case["sigma2_2"][c["octave2"]], variant),
                        m1_exact=f64(9.210) * f64(case["sigma2_1"][c["octave1"]]),
                        m2_exact=f64(9.210) * f64(case["sigma2_2"][c["octave2"]]),
                        i1=int(c["i1"])))
    return out, K1, K2


def check_inliers(prep, K1, K2, H, ev=None):
    ev = {} if ev is None else ev
    flags = []
    for q in prep:
        a = to_image(gemm3(H["sR"], q["X2"], H["t"]), K1)
        b = to_image(gemm3(H["sRinv"], q["X1"], H["tinv"]), K2)
        d10, d11 = q["p1"][0] - a[0], q["p1"][1] - a[1]
        d20, d21 = b[0] - q["p2"][0], b[1] - q["p2"][1]
        err1 = f32((f64(0) + f64(d10) * f64(d10)) + f64(d11) * f64(d11))
        err2 = f32((f64(0) + f64(d20) * f64(d20)) + f64(d21) * f64(d21))
        if (q["m1"] < err1 < q["m1_exact"]) or (q["m2"] < err2 < q["m2_exact"]):
            ev["between_bounds"] = True
        if err1 == q["m1"] or err2 == q["m2"]:
            ev["at_bound"] = True
        if not (np.isfinite(err1) and np.isfinite(err2)) and not np.isnan(H["R"]).all():
            ev["nonfinite_error"] = True
        flags.append(bool(err1 < q["m1"] and err2 < q["m2"]))
    return flags


# ---- iterate() (:140-207) ---------------------------------------------------------------------------

def solve(case, variant=None):
    """-> dict(calls=[per iterate() call: the result fields, `inliers`, `state`], trace=[...],
    max_its, triples)."""
    with np.errstate(all="ignore"):
        return _solve(case, variant)


def _solve(case, variant):
    N, mN1, min_inl = len(case["corr"]), case["mN1"], case["min_inliers"]
    max_its = ransac_iterations_np(case["prob"], min_inl, case["max_iterations"], N, variant)
    triples = sample_triples_np(N, case["rand"][:3 * max_its], variant) if N >= 3 else \
        np.zeros((max_its, 3), np.int32)
    prep, K1, K2 = prepare(case, variant)
    its, best = case["state0"]
    calls, trace = [], []
    for n_iterations in case["calls"]:
        res = dict(found=0, iteration=0, n_inliers=0, no_more=0, info=0, best_updated=0,
                   best_inliers=None, model=None, inliers=np.zeros(mN1, np.uint8))
        if N < min_inl and variant != "no_small_n_exit":
            res["no_more"] = 1
            trace.append(dict(exit="small_n"))
        else:
            cur, best_at_start = 0, best
            while its < max_its and cur < n_iterations:
                cur += 1
                its += 1
                ev = dict(it=its, triple=tuple(int(v) for v in triples[its - 1]))
                if N < 3:
                    # only reachable under no_small_n_exit: no minimal set exists
                    ev["exit"] = "no_triple"
                    trace.append(ev)
                    continue
                P1 = np.stack([prep[i]["X1"] for i in ev["triple"]], axis=1)
                P2 = np.stack([prep[i]["X2"] for i in ev["triple"]], axis=1)
                H = compute_sim3(P1, P2, case["fix_scale"], variant, ev)
                flags = check_inliers(prep, K1, K2, H, ev)
                cnt = sum(flags)
                ev["count"] = cnt
                weak = cnt > best if variant == "gt_best" else cnt >= best
                ev["weak"], ev["tie"] = weak, weak and cnt == best and its > 1
                if weak:
                    best = cnt
                    res["best_updated"], res["best_inliers"], res["model"] = 1, cnt, H
                    if cnt >= min_inl if variant == "ge_min" else cnt > min_inl:
                        ev["exit"] = "returned"
                        ev["carried_best"] = best_at_start > min_inl
                        res["found"], res["iteration"], res["n_inliers"] = 1, its, cnt
                        for i, f in enumerate(flags):
                            if f:
                                res["inliers"][i if variant == "inliers_by_corr" else prep[i]["i1"]] = 1
                        trace.append(ev)
                        break
                ev.setdefault("exit", "continue")
                trace.append(ev)
            if not res["found"] and its >= max_its:
                res["no_more"] = 1
                trace.append(dict(exit="max_its", on_last=cur == n_iterations))
        res["state"] = (its, best)
        calls.append(res)
    return dict(calls=calls, trace=trace, max_its=max_its, triples=triples)


def result_record(call):
    """The orbx_sim3_result a call leaves in a record prefilled with SENTINEL bytes."""
    r = np.frombuffer(bytes([SENTINEL]) * SIM3_RESULT_DTYPE.itemsize, SIM3_RESULT_DTYPE).copy()[0:1]
    rec = r[0]
    for k in ("found", "iteration", "n_inliers", "no_more", "info", "best_updated"):
        rec[k] = call[k]
    if call["best_updated"]:
        H = call["model"]
        rec["best_inliers"] = call["best_inliers"]
        rec["R12"], rec["t12"], rec["s12"] = H["R"].reshape(9), H["t"], H["s"]
        T = np.zeros((4, 4), f32)
        T[:3, :3], T[:3, 3], T[3, 3] = H["sR"], H["t"], 1
        rec["T12"] = T.reshape(16)
    return r


def canon(record_bytes):
    """A result record's bytes with every NaN float replaced by one NaN: NaN equals NaN."""
    w = np.frombuffer(bytes(record_bytes), np.uint32).copy()
    first = SIM3_RESULT_DTYPE.fields["R12"][1] // 4
    fl = w[first:]
    fl[(fl & 0x7fffffff) > 0x7f800000] = 0x7fc00000
    return w.tobytes()


def key(result):
    """Everything observable of a solve(), as bytes."""
    out = b""
    for c in result["calls"]:
        out += canon(result_record(c).tobytes()) + c["inliers"].tobytes() + struct.pack("<ii", *c["state"])
    return out


@functools.lru_cache(maxsize=None)
def _reference_cached(name):
    return solve(case_named(name))


def reference(case):
    return _reference_cached(case["name"]) if case["name"] in _names() else solve(case)


# ---- the cases ------------------------------------------------------------------------------------

K_EUROC = (458.654, 457.296, 367.215, 248.375)
BOUNDS = (0.0, 752.0, 0.0, 480.0)
SIGMA2_12 = np.array([f32(1.2) ** (2 * l) for l in range(8)], f32)      # 1.44 at level 1
# 9.210 * sigma2 a hair (2^-10) above an integer: truncation moves the bound by 0.001 at most
SIGMA2_INT = np.array([(k + 2.0 ** -10) / 9.210 for k in (10, 20, 40, 80)], f64).astype(f32)


def rodrigues64(w):
    w = np.asarray(w, f64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def make_case(name, seed, N, n_outliers=0, noise=0.0, rot=(0.1, -0.2, 0.15), trans=(0.3, -0.1, 0.2),
              scale=1.1, fix_scale=False, min_inliers=6, max_iterations=300, prob=0.99,
              calls=(300,), state0=(0, 0), identity_poses=False, sigma2=SIGMA2_12, mN1=None,
              sparse_i1=False, octaves=None):
    rng = np.random.default_rng(seed)
    X2c = np.stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(2.5, 8, N)], 1)
    R12 = rodrigues64(rot)
    X1c = scale * (X2c @ R12.T) + np.asarray(trans, f64)
    X1c += rng.normal(0, noise, X1c.shape) * X1c[:, 2:3] / 458.0
    out = rng.choice(N, n_outliers, replace=False) if n_outliers else []
    for i in out:
        X1c[i] += rng.uniform(-1, 1, 3) * 0.8
    if identity_poses:
        Rc1 = Rc2 = np.eye(3)
        t1 = t2 = np.zeros(3)
    else:
        Rc1, Rc2 = rodrigues64(rng.normal(0, 0.3, 3)), rodrigues64(rng.normal(0, 0.3, 3))
        t1, t2 = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
    sc = [1.2 ** l for l in range(len(sigma2))]
    pose1 = frame_pose(Rc1, t1, K_EUROC, BOUNDS, sc)
    pose2 = frame_pose(Rc2, t2, K_EUROC, BOUNDS, sc)
    corr = np.zeros(N, SIM3_CORR_DTYPE)
    corr["X1w"] = ((X1c - t1) @ Rc1).astype(f32)
    corr["X2w"] = ((X2c - t2) @ Rc2).astype(f32)
    mN1 = (3 * N + 7 if sparse_i1 else N) if mN1 is None else mN1
    corr["i1"] = rng.permutation(mN1)[:N] if sparse_i1 else np.arange(N)
    oc = rng.integers(0, len(sigma2), (N, 2)) if octaves is None else np.asarray(octaves)
    corr["octave1"], corr["octave2"] = oc[:, 0], oc[:, 1]
    rand = rng.integers(0, RAND_MAX + 1, 3 * max_iterations).astype(np.int32)
    return dict(name=name, pose1=pose1, pose2=pose2, sigma2_1=np.asarray(sigma2, f32),
                sigma2_2=np.asarray(sigma2, f32), corr=corr, mN1=int(mN1),
                fix_scale=bool(fix_scale), min_inliers=min_inliers, max_iterations=max_iterations,
                prob=prob, rand=rand, calls=tuple(calls), state0=tuple(state0))


def _edit(case, name, **kw):
    c = dict(case)
    c["corr"] = case["corr"].copy()
    c["rand"] = case["rand"].copy()
    c.update(kw)
    c["name"] = name
    return c


def rand_for(position, size):
    """A rand() value whose RandomInt(0, size - 1) is `position`."""
    v = int(np.ceil(position * (RAND_MAX + 1.0) / size))
    assert int(f64(v) / (f64(RAND_MAX) + f64(1.0)) * f64(size)) == position
    return v


def rand_for_triple(N, triple):
    """rand() values that make :163-177 draw exactly `triple` (by literal simulation)."""
    avail, out = list(range(N)), []
    for idx in triple:
        pos = avail.index(idx)
        out.append(rand_for(pos, len(avail)))
        avail[pos] = avail[-1]
        avail.pop()
    return out


def exact_points_case(name, X1, X2, triple=(0, 1, 2), **kw):
    """Identity poses and points given in the camera frames (exact in float32)."""
    X1, X2 = np.asarray(X1, f32), np.asarray(X2, f32)
    kw.setdefault("max_iterations", 1)
    c = make_case(name, 1, len(X1), identity_poses=True, **kw)
    c["corr"]["X1w"], c["corr"]["X2w"] = X1, X2
    c["rand"][:3] = rand_for_triple(len(X1), triple)
    return c


def _shift_to_error(case, idx, d, exact):
    """Moves correspondence idx's X1w (identity pose 1) so that, under the model of the case's
    first triple, mvP1im1 - vP2im1 of :350 is `d` (exact=True: equal as floats, reached by stepping
    through neighbouring floats; exact=False: to within 1e-3 pixels)."""
    r = solve(dict(case, calls=(1,)))
    H = r["calls"][0]["model"]
    prep, K1, _ = prepare(case)
    q = prep[idx]
    a = to_image(gemm3(H["sR"], q["X2"], H["t"]), K1)
    want = (a[0] + f32(d[0]), a[1] + f32(d[1]))
    X = case["corr"]["X1w"][idx].copy()
    for k in (0, 1):
        X[k] = f32((want[k] - K1[2 + k]) / K1[k] * X[2])
        for _ in range(4000 if exact else 0):
            got = to_image(X, K1)[k]
            if got == want[k]:
                break
            X[k] = np.nextafter(X[k], f32(np.inf) if got < want[k] else f32(-np.inf))
    got = to_image(X, K1)
    if exact:
        assert got[0] - a[0] == f32(d[0]) and got[1] - a[1] == f32(d[1]), (got, a, d)
    else:
        assert abs(got[0] - a[0] - d[0]) < 1e-3 and abs(got[1] - a[1] - d[1]) < 1e-3
    case["corr"]["X1w"][idx] = X
    return case


def bound_case(name, d, exact, sigma2, octave):
    """Eight clean correspondences and one (index 8, never drawn) whose image error in keyframe 1
    is placed at d[0]^2 + d[1]^2; one iteration over the triple (0, 1, 2)."""
    c = make_case(name, 7, 9, identity_poses=True, max_iterations=1, min_inliers=3,
                  sigma2=sigma2, octaves=np.full((9, 2), (octave, len(sigma2) - 1)))
    c["rand"][:3] = rand_for_triple(9, (0, 1, 2))
    return _shift_to_error(c, 8, d, exact)


def all_cases_tuple():
    cases = []
    # the bounds (:87-88, :356)
    cases.append(bound_case("between_bounds", (3.0, 2.03), False, SIGMA2_12, 1))
    cases.append(bound_case("at_bound", (3.0, 2.0), True, SIGMA2_12, 1))
    cases.append(bound_case("integer_sigma_table", (3.0, 1.2), False, SIGMA2_INT, 0))
    # the count against min_inliers and the best count (:183, :192)
    base = make_case("count_above_min", 11, 12, n_outliers=5, min_inliers=6, max_iterations=40)
    cases.append(base)
    cases.append(_edit(base, "count_equal_min", min_inliers=7))
    # the same three points in another order: the same count, another model in the last bits; the
    # two triples after it hold displaced points and count less, so iteration 2 is the record
    tie = make_case("later_tie", 12, 10, min_inliers=9, max_iterations=4, noise=0.2, calls=(4,))
    tie["corr"]["X1w"][6:] += f32(0.5)
    tie["rand"][:12] = (rand_for_triple(10, (0, 1, 2)) + rand_for_triple(10, (2, 0, 1)) +
                        rand_for_triple(10, (6, 7, 8)) + rand_for_triple(10, (7, 8, 9)))
    cases.append(tie)
    # a large angle: norm(vec) accumulated in float gives another (float)alpha
    cases.append(make_case("norm_in_double", 201, 8, noise=0.3, min_inliers=7, max_iterations=3,
                           calls=(3,), rot=(1.2, -0.9, 0.8)))
    cases.append(_edit(base, "carried_best_equal", state0=(0, 7), calls=(5, 5, 5, 5)))
    cases.append(_edit(base, "carried_best_lower", state0=(0, 8), calls=(5, 5, 5, 5)))
    cases.append(_edit(base, "returned_then_again", calls=(5,) * 8))
    # N against min_inliers (:130, :146)
    cases.append(make_case("n_equals_min", 13, 6, min_inliers=6, calls=(5, 5)))
    cases.append(make_case("n_below_min", 14, 5, min_inliers=6, calls=(5,)))
    # max_its reached on a call's last iteration (:203)
    cases.append(make_case("max_its_on_last", 15, 20, n_outliers=20, min_inliers=19,
                           max_iterations=10, calls=(1, 2, 5)))   # mRansacMaxIts = 3
    # the NaN conventions and the angle's corners
    sq = [[0, 0, 4], [1, 0, 4], [0, 1, 4], [1, 1, 5], [-1, 0.5, 6], [0.5, -1, 3], [2, 1, 7]]
    cases.append(exact_points_case("identity_rotation_nan", np.asarray(sq) + [0.5, 0.25, 1.0], sq,
                                   min_inliers=3))
    zero = [[1, 1, 4]] * 3 + sq[3:]
    cases.append(exact_points_case("zero_M_nan", zero, zero, min_inliers=3))
    flip = np.asarray(sq, f64) * [-1, -1, 1]          # 180 degrees about z
    cases.append(exact_points_case("rotation_180", flip + [0, 0, 0.5], sq, min_inliers=3))
    cases.append(make_case("negative_q0", 16, 12, rot=(0, 0, 3.9), min_inliers=6,
                           max_iterations=20))
    line = [[0, 0, 4], [1, 0, 4], [2, 0, 4], [1, 1, 5], [-1, 0.5, 6], [0.5, -1, 3], [2, 1, 7]]
    cases.append(exact_points_case("collinear_triple", np.asarray(line) * 2.0, line, min_inliers=3))
    cases.append(make_case("fix_scale_on", 17, 14, n_outliers=3, scale=1.0, fix_scale=True,
                           max_iterations=20))
    cases.append(make_case("fix_scale_off", 17, 14, n_outliers=3, scale=1.0, fix_scale=False,
                           max_iterations=20))
    z0 = make_case("z_zero", 18, 12, identity_poses=True, min_inliers=6, max_iterations=20)
    z0["corr"]["X1w"][5, 2] = 0.0
    cases.append(z0)
    # the draws (:168-176)
    d = make_case("draw_last_and_zero", 19, 10, min_inliers=9, max_iterations=4, prob=0.99,
                  calls=(4,))
    d["rand"][:12] = [rand_for(9, 10), rand_for(8, 9), rand_for(0, 8),
                      rand_for(0, 10), rand_for(0, 9), rand_for(7, 8),
                      0, 0, 0, RAND_MAX, RAND_MAX, RAND_MAX]
    cases.append(d)
    cases.append(make_case("sparse_i1", 20, 15, n_outliers=4, sparse_i1=True, max_iterations=30))
    cases.append(make_case("epsilon_float_vs_double", 21, EPS_N, n_outliers=EPS_N,
                           min_inliers=EPS_MIN, prob=EPS_PROB, max_iterations=300,
                           calls=(300,), sigma2=SIGMA2_INT))
    # seeded random cases in the GPU test's size regimes
    for k, N in enumerate((3, 4, 19, 20, 21, 63, 64, 65, 129, 300)):
        cases.append(make_case(f"random_{N}", 100 + k, N, n_outliers=N // 3, noise=0.5,
                               min_inliers=min(6, N), max_iterations=(1, 5, 300)[k % 3],
                               sparse_i1=bool(k & 1), calls=(5,) * 3 if k % 3 == 2 else (300,)))
    return tuple(cases)


# (min_inliers, N, prob) at which the float epsilon of :125 and a double one give different
# iteration counts: 1 - prob = exp(100 * L) with L halfway between log(1 - eps^3) of the two, so
# the quotient falls on the two sides of 100 (tests/test_sim3_cases.py asserts 100 and 101)
EPS_MIN, EPS_N = 6, 20


def _eps_prob():
    ef, ed = f64(f32(EPS_MIN) / f32(EPS_N)), f64(EPS_MIN) / f64(EPS_N)
    L = (np.log(f64(1) - ef ** 3) + np.log(f64(1) - ed ** 3)) / 2
    return float(f64(1) - np.exp(100 * L))


EPS_PROB = _eps_prob()


@functools.lru_cache(maxsize=None)
def _all_cases_cached():
    return all_cases_tuple()


def all_cases():
    return list(_all_cases_cached())


@functools.lru_cache(maxsize=None)
def _names():
    return frozenset(c["name"] for c in all_cases())


def case_named(name):
    for c in all_cases():
        if c["name"] == name:
            return c
    raise KeyError(name)


def job_of(case, max_its, n_iterations, **kw):
    return sim3_job(case["sigma2_1"], case["sigma2_2"], case["mN1"], len(case["corr"]),
                    case["fix_scale"], case["min_inliers"], max_its, n_iterations, **kw)


# ---- the file tests/native/sim3_ref reads and writes --------------------------------------------

def write_cases(path, cases):
    """Per case: N, mN1, fix_scale, min_inliers, max_its, ncalls, state0[2], nlevels1, nlevels2;
    the two pose records; sigma2_1[16], sigma2_2[16]; the correspondences; the triples; the calls'
    n_iterations."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            r = reference(c)
            job = job_of(c, r["max_its"], 0)
            f.write(struct.pack("<10i", len(c["corr"]), c["mN1"], int(c["fix_scale"]),
                                c["min_inliers"], r["max_its"], len(c["calls"]), *c["state0"],
                                len(c["sigma2_1"]), len(c["sigma2_2"])))
            f.write(np.asarray(c["pose1"], FRAME_POSE_DTYPE).tobytes())
            f.write(np.asarray(c["pose2"], FRAME_POSE_DTYPE).tobytes())
            f.write(job["sigma2_1"].tobytes() + job["sigma2_2"].tobytes())
            f.write(c["corr"].tobytes())
            f.write(np.ascontiguousarray(r["triples"], np.int32).tobytes())
            f.write(np.asarray(c["calls"], np.int32).tobytes())


def read_results(path, cases):
    """-> per case, per call: (result record bytes, inlier bytes, (iterations, best_inliers))"""
    data = open(path, "rb").read()
    off, out = 0, []
    for c in cases:
        per = []
        for _ in c["calls"]:
            rec = data[off:off + SIM3_RESULT_DTYPE.itemsize]
            off += SIM3_RESULT_DTYPE.itemsize
            inl = data[off:off + c["mN1"]]
            off += c["mN1"]
            st = struct.unpack_from("<ii", data, off)
            off += 8
            per.append((rec, inl, st))
        out.append(per)
    assert off == len(data)
    return out
