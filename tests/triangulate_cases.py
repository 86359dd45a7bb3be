"""The per-match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:356-507) that
orbx_triangulate_matches* (k_triangulate_points) runs, restated literally in numpy float32 / Python
double, and the cases for it (numpy only; shared by tests/test_triangulate_cases.py on the CPU and
tests/test_gpu_triangulate.py on the GPU).

``triangulate_np`` follows the reference statement by statement and returns, per pair, the outcome
code (orbx_tri_code) and x3D.  ``svd_np`` is a separate literal restatement of OpenCV 3.2's
JacobiSVDImpl_<float> as cv::SVD::compute reaches it for a 4x4 CV_32F matrix.  The three forms
evaluated inside OpenCV ([unverified-OpenCV]) are ``a_rows`` (cv::addWeighted),
``svd_np`` and ``div_w`` (Mat::convertTo).

``variant=`` switches one decision to a plausible wrong form: ``invert:<test>`` / ``remove:<test>``
for every test of the loop (``TESTS``), and the named quirks.  tests/test_triangulate_cases.py
requires every variant to change at least one case.

A case is a dict: name, pose1 / pose2 (FRAME_POSE_DTYPE records of mpCurrentKeyFrame / pKF2),
keys1 / keys2 (mvKeysUn), raw1 / raw2 (mvKeys or None), ur1 / ur2 (mvuRight or None), depth1 /
depth2 (mvDepth or None), cos1 / cos2 (an explicit cosParallaxStereo table, or None: from mb and
the depths), mb, ratio_factor, pairs (int32 [m, 2]).  Invariant of the builder: the octaves of
paired features lie in [0, nlevels) -- the reference indexes its tables unchecked.
"""
import ctypes

import numpy as np

from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import FRAME_POSE_DTYPE, frame_pose

_libm = ctypes.CDLL("libm.so.6")
_libm.hypot.restype = ctypes.c_double
_libm.hypot.argtypes = [ctypes.c_double, ctypes.c_double]
f32 = np.float32
f64 = np.float64
FLT_EPSILON = f32(1.1920928955078125e-07)
DBL_EPSILON = 2.220446049250313e-16

CODES = ("OK_TRIANGULATED", "OK_STEREO1", "OK_STEREO2", "NO_MATCH", "LOW_PARALLAX", "W_ZERO",
         "BEHIND_1", "BEHIND_2", "REPROJ_1", "REPROJ_2", "DIST_ZERO", "SCALE")
(OK_TRIANGULATED, OK_STEREO1, OK_STEREO2, NO_MATCH, LOW_PARALLAX, W_ZERO, BEHIND_1, BEHIND_2,
 REPROJ_1, REPROJ_2, DIST_ZERO, SCALE) = range(12)
LOOP_CODES = tuple(c for c in range(12) if c != NO_MATCH)    # what a pair can get

# the tests of the loop, in source order; each can be inverted or removed
TESTS = ("cos_lt_stereo", "cos_gt_0", "parallax_gate", "stereo1_select", "stereo2_select",
         "w_zero", "behind_1", "behind_2", "reproj_1", "reproj_2", "dist_zero", "scale_low",
         "scale_high")
QUIRKS = ("if_388",            # `if` for the `else if` of :388
          "mbf2_482",          # pKF2->mbf at :482
          "cos_gt_0_nonstrict", "cos_lt_stereo_nonstrict", "behind_1_strict", "behind_2_strict",
          "xn_third_0",        # a 0.0 third entry of xn
          "svd_first_row",     # vt.row(0) for vt.row(3)
          "sort_ascending")    # singular values sorted ascending
VARIANTS = tuple(f"{k}:{t}" for t in TESTS for k in ("invert", "remove")) + QUIRKS
# Variants that cannot change a bit, so no case pretends to pin them:
#  * cosParallaxRays < 0.9998 compared in float: (float)0.9998 is above 0.9998 and no float lies
#    between them, so `<` against either selects the same floats.
#  * invz = 1.0f / z for (float)(1.0 / z): double rounding is innocuous for a quotient of floats.
#  * the sign of vt.row(3): it cancels in the division by its fourth entry.


# ---- OpenCV forms -----------------------------------------------------------------------------

def a_rows(xn1, xn2, T1, T2):
    """A.row(0) = xn1(0)*Tcw1.row(2) - Tcw1.row(0) ... (:399-402): MatOp_AddEx::assign calls
    cv::addWeighted(a, alpha, b, -1, 0), which for CV_32F computes in double
    (float)(a*alpha + b*beta + gamma)  [unverified-OpenCV]."""
    A = np.zeros((4, 4), f32)
    for r, (s, Tm, row) in enumerate(((xn1[0], T1, 0), (xn1[1], T1, 1), (xn2[0], T2, 0),
                                      (xn2[1], T2, 1))):
        for k in range(4):
            A[r, k] = f32(float(Tm[2][k]) * float(s) + float(Tm[row][k]) * -1.0 + 0.0)
    return A


def svd_np(A, sort_ascending=False):
    """cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) for a 4x4 CV_32F A -> (w, vt)
    [unverified-OpenCV]: At = A^T; JacobiSVDImpl_<float>(At, W, Vt, 4, 4, eps = 2*FLT_EPSILON):
    W in double, rotations in float, at most max(m, 30) sweeps, then W = row norms, sorted
    descending by a selection sort that carries the rows of Vt along."""
    m = n = 4
    At = np.array(A, f32).T.copy()
    Vt = np.eye(n, dtype=f32)
    W = [0.0] * n
    for i in range(n):
        sd = 0.0
        for k in range(m):
            t = At[i, k]
            sd += float(t) * float(t)
        W[i] = sd
    eps = f32(FLT_EPSILON * f32(2))
    max_iter = max(m, 30)
    with np.errstate(all="ignore"):
        for _ in range(max_iter):
            changed = False
            for i in range(n - 1):
                for j in range(i + 1, n):
                    a, p, b = W[i], 0.0, W[j]
                    for k in range(m):
                        p += float(At[i, k]) * float(At[j, k])
                    if abs(p) <= float(eps) * float(np.sqrt(f64(a) * f64(b))):
                        continue
                    p *= 2.0
                    beta = a - b
                    gamma = _libm.hypot(p, beta)
                    if beta < 0:
                        delta = (gamma - beta) * 0.5
                        s = f32(np.sqrt(f64(delta) / f64(gamma)))
                        c = f32(f64(p) / f64(gamma * float(s) * 2))
                    else:
                        c = f32(np.sqrt(f64(gamma + beta) / f64(gamma * 2)))
                        s = f32(f64(p) / f64(gamma * float(c) * 2))
                    a = b = 0.0
                    for k in range(m):
                        t0 = f32(f32(c * At[i, k]) + f32(s * At[j, k]))
                        t1 = f32(f32(-s * At[i, k]) + f32(c * At[j, k]))
                        At[i, k], At[j, k] = t0, t1
                        a += float(t0) * float(t0)
                        b += float(t1) * float(t1)
                    W[i], W[j] = a, b
                    changed = True
                    for k in range(n):
                        t0 = f32(f32(c * Vt[i, k]) + f32(s * Vt[j, k]))
                        t1 = f32(f32(-s * Vt[i, k]) + f32(c * Vt[j, k]))
                        Vt[i, k], Vt[j, k] = t0, t1
            if not changed:
                break
        for i in range(n):
            sd = 0.0
            for k in range(m):
                sd += float(At[i, k]) * float(At[i, k])
            W[i] = float(np.sqrt(f64(sd)))
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if (W[j] > W[k]) if sort_ascending else (W[j] < W[k]):
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            Vt[[i, j]] = Vt[[j, i]]
    return np.array(W, f64).astype(f32), Vt


def div_w(v):
    """x3D.rowRange(0,3) / x3D.at<float>(3): convertTo with alpha = 1.0 / w, i.e.
    x * (float)alpha + 0.0f, or a plain copy when |alpha - 1| < DBL_EPSILON  [unverified-OpenCV]."""
    with np.errstate(all="ignore"):
        alpha = f64(1.0) / f64(v[3])
        if abs(alpha - 1.0) < DBL_EPSILON:
            return [f32(v[k]) for k in range(3)]
        sc = f32(alpha)
        return [f32(f32(v[k] * sc) + f32(0)) for k in range(3)]


# ---- the loop -----------------------------------------------------------------------------------

def _dot_d(a, b):
    s = 0.0
    for k in range(3):
        s += float(a[k]) * float(b[k])
    return s


def _norm_d(a):
    ss = 0.0
    for k in range(3):
        ss += float(a[k]) * float(a[k])
    return float(np.sqrt(f64(ss)))


def _tcw(F):
    R = F["Rcw"].reshape(3, 3)
    return [[R[r, 0], R[r, 1], R[r, 2], F["tcw"][r]] for r in range(3)]


def _row(F, r, X):
    """Rcw.row(r).dot(x3Dt) + tcw.at<float>(r), stored in a float."""
    R = F["Rcw"]
    return f32(_dot_d(R[3 * r:3 * r + 3], X) + float(F["tcw"][r]))


def unproject_np(F, u, v, z):
    """KeyFrame::UnprojectStereo for z > 0 (KeyFrame.cc:629-645)."""
    invfx, invfy = f32(f32(1) / F["fx"]), f32(f32(1) / F["fy"])
    c = [f32(f32(f32(u - F["cx"]) * z) * invfx), f32(f32(f32(v - F["cy"]) * z) * invfy), f32(z)]
    R = F["Rcw"]
    out = []
    for r in range(3):
        t = f32(f32(R[r] * c[0]) + f32(R[3 + r] * c[1]))
        t = f32(t + f32(R[6 + r] * c[2]))
        out.append(f32(float(t) + float(F["Ow"][r])))
    return out


def stereo_cos_np(mb, depth):
    """(float)cos(2*atan2(mb/2, depth)) in numpy float64 (:387, :389)."""
    with np.errstate(all="ignore"):
        half = f64(f32(f32(mb) / f32(2)))
        return np.cos(2 * np.arctan2(half, np.asarray(depth, f32).astype(f64))).astype(f32)


def cos_tables(case):
    out = []
    for k in ("1", "2"):
        n = len(case["keys" + k])
        if case.get("cos" + k) is not None:
            out.append(np.asarray(case["cos" + k], f32))
        elif case.get("depth" + k) is not None:
            out.append(stereo_cos_np(case["mb"], case["depth" + k]))
        else:
            out.append(np.zeros(n, f32))
    return out


def tri_one(F1, F2, kp1, kp2, raw1, raw2, ur1, ur2, z1d, z2d, cs1, cs2, ratio_factor, variant=None,
            info=None):
    """The loop body :361-507 for one pair -> (code, x3D or None)."""
    info = {} if info is None else info

    def T(name, cond, removed):
        if variant == "invert:" + name:
            return not cond
        if variant == "remove:" + name:
            return removed
        return bool(cond)

    with np.errstate(all="ignore"):
        st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
        third = f32(0.0 if variant == "xn_third_0" else 1.0)
        xn1 = [f32(f32(kp1["x"] - F1["cx"]) * f32(f32(1) / F1["fx"])),
               f32(f32(kp1["y"] - F1["cy"]) * f32(f32(1) / F1["fy"])), third]
        xn2 = [f32(f32(kp2["x"] - F2["cx"]) * f32(f32(1) / F2["fx"])),
               f32(f32(kp2["y"] - F2["cy"]) * f32(f32(1) / F2["fy"])), third]
        R1, R2 = F1["Rcw"], F2["Rcw"]
        ray1 = [f32(f32(f32(R1[r] * xn1[0]) + f32(R1[3 + r] * xn1[1])) + f32(R1[6 + r] * xn1[2]))
                for r in range(3)]
        ray2 = [f32(f32(f32(R2[r] * xn2[0]) + f32(R2[3 + r] * xn2[1])) + f32(R2[6 + r] * xn2[2]))
                for r in range(3)]
        cos_rays = f32(f64(_dot_d(ray1, ray2)) / f64(_norm_d(ray1) * _norm_d(ray2)))
        cps = f32(cos_rays + f32(1))
        cps1 = cps2 = cps
        if st1:
            cps1 = f32(cs1)
            if variant == "if_388" and st2:
                cps2 = f32(cs2)
        elif st2:
            cps2 = f32(cs2)
        cps = cps2 if cps2 < cps1 else cps1          # std::min(cps1, cps2)
        info.update(cos_rays=cos_rays, cps1=cps1, cps2=cps2, A=None)

        lt_stereo = cos_rays <= cps if variant == "cos_lt_stereo_nonstrict" else cos_rays < cps
        gt0 = cos_rays >= f32(0) if variant == "cos_gt_0_nonstrict" else cos_rays > f32(0)
        if (T("cos_lt_stereo", lt_stereo, True) and T("cos_gt_0", gt0, True) and
                T("parallax_gate", st1 or st2 or float(cos_rays) < 0.9998, True)):
            A = a_rows(xn1, xn2, _tcw(F1), _tcw(F2))
            info["A"] = A
            w, vt = svd_np(A, variant == "sort_ascending")
            v = vt[0 if variant == "svd_first_row" else 3]
            info.update(w=w, v=v.copy())
            if T("w_zero", v[3] == 0, False):
                return W_ZERO, None
            X = div_w(v)
            code = OK_TRIANGULATED
        elif T("stereo1_select", st1 and cps1 < cps2, False):
            if not z1d > 0:
                return LOW_PARALLAX, None        # UnprojectStereo returns an empty Mat
            X = unproject_np(F1, raw1["x"], raw1["y"], f32(z1d))
            code = OK_STEREO1
        elif T("stereo2_select", st2 and cps2 < cps1, False):
            if not z2d > 0:
                return LOW_PARALLAX, None
            X = unproject_np(F2, raw2["x"], raw2["y"], f32(z2d))
            code = OK_STEREO2
        else:
            return LOW_PARALLAX, None

        z1 = _row(F1, 2, X)
        if T("behind_1", z1 < 0 if variant == "behind_1_strict" else z1 <= 0, False):
            return BEHIND_1, None
        z2 = _row(F2, 2, X)
        if T("behind_2", z2 < 0 if variant == "behind_2_strict" else z2 <= 0, False):
            return BEHIND_2, None
        info.update(z1=z1, z2=z2)

        def reproj_rejects(F, kp, ur, stereo, z, mbf):
            sigma2 = f32(F["scale"][int(kp["octave"])] * F["scale"][int(kp["octave"])])
            x, y = _row(F, 0, X), _row(F, 1, X)
            invz = f32(f64(1.0) / f64(z))
            u = f32(f32(f32(F["fx"] * x) * invz) + F["cx"])
            v_ = f32(f32(f32(F["fy"] * y) * invz) + F["cy"])
            ex, ey = f32(u - kp["x"]), f32(v_ - kp["y"])
            if not stereo:
                return float(f32(f32(ex * ex) + f32(ey * ey))) > 5.991 * float(sigma2)
            u_r = f32(u - f32(mbf * invz))
            er = f32(u_r - ur)
            return float(f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))) > 7.8 * float(sigma2)

        if T("reproj_1", reproj_rejects(F1, kp1, ur1, st1, z1, F1["mbf"]), False):
            return REPROJ_1, None
        mbf2 = F2["mbf"] if variant == "mbf2_482" else F1["mbf"]     # :482
        if T("reproj_2", reproj_rejects(F2, kp2, ur2, st2, z2, mbf2), False):
            return REPROJ_2, None

        dist1 = f32(_norm_d([f32(X[k] - F1["Ow"][k]) for k in range(3)]))
        dist2 = f32(_norm_d([f32(X[k] - F2["Ow"][k]) for k in range(3)]))
        if T("dist_zero", dist1 == 0 or dist2 == 0, False):
            return DIST_ZERO, None
        ratio_dist = f32(dist2 / dist1)
        ratio_octave = f32(F1["scale"][int(kp1["octave"])] / F2["scale"][int(kp2["octave"])])
        rf = f32(ratio_factor)
        if (T("scale_low", f32(ratio_dist * rf) < ratio_octave, False) or
                T("scale_high", ratio_dist > f32(ratio_octave * rf), False)):
            return SCALE, None
        return code, X


def triangulate_np(case, variant=None):
    """-> (status int32 [m], x3d float32 [m, 3] (NaN where not OK), info list)."""
    F1 = np.asarray(case["pose1"], FRAME_POSE_DTYPE).reshape(())
    F2 = np.asarray(case["pose2"], FRAME_POSE_DTYPE).reshape(())
    k1, k2 = case["keys1"], case["keys2"]
    r1 = k1 if case.get("raw1") is None else case["raw1"]
    r2 = k2 if case.get("raw2") is None else case["raw2"]
    ur1 = np.full(len(k1), -1, f32) if case.get("ur1") is None else case["ur1"]
    ur2 = np.full(len(k2), -1, f32) if case.get("ur2") is None else case["ur2"]
    d1 = np.zeros(len(k1), f32) if case.get("depth1") is None else case["depth1"]
    d2 = np.zeros(len(k2), f32) if case.get("depth2") is None else case["depth2"]
    c1, c2 = cos_tables(case)
    pairs = np.asarray(case["pairs"], np.int32).reshape(-1, 2)
    status = np.zeros(len(pairs), np.int32)
    x3d = np.full((len(pairs), 3), np.nan, f32)
    infos = []
    for p, (i1, i2) in enumerate(pairs):
        assert 0 <= k1["octave"][i1] < F1["nlevels"] and 0 <= k2["octave"][i2] < F2["nlevels"]
        info = {}
        code, X = tri_one(F1, F2, k1[i1], k2[i2], r1[i1], r2[i2], f32(ur1[i1]), f32(ur2[i2]),
                          f32(d1[i1]), f32(d2[i2]), c1[i1], c2[i2], case["ratio_factor"], variant,
                          info)
        status[p] = code
        if X is not None:
            x3d[p] = X
        infos.append(info)
    return status, x3d, infos


_REF = {}


def reference(case):
    """triangulate_np of a case, computed once per process and shared (treat as read-only)."""
    if case["name"] not in _REF:
        _REF[case["name"]] = triangulate_np(case)
    return _REF[case["name"]]


# ---- building cases -----------------------------------------------------------------------------

NLEVELS = 8
K4 = (f32(512.0), f32(512.0), f32(320.0), f32(240.0))
BOUNDS = (0.0, 640.0, 0.0, 480.0)
MBF = f32(40.0)
MB = f32(MBF / K4[0])
RATIO_FACTOR = f32(f32(1.5) * f32(1.2))


def scale_factors(nlevels=NLEVELS, factor=1.2):
    """mvScaleFactor as ORBextractor.cc:417-421 builds it."""
    sc = [f32(1)]
    for _ in range(1, nlevels):
        sc.append(f32(sc[-1] * f32(factor)))
    return np.array(sc, f32)


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def pose(R=None, centre=(0, 0, 0), K4_=K4, mbf=MBF, nlevels=NLEVELS):
    """A keyframe with rotation Rcw and camera centre `centre` (tcw = -Rcw * centre)."""
    R = np.eye(3) if R is None else np.asarray(R, f64)
    t = -R @ np.asarray(centre, f64)
    return frame_pose(R.astype(f32), t.astype(f32), K4_, BOUNDS, scale_factors(nlevels), mbf)


def project(F, X):
    """Pixel and depth of world points X [n, 3] in keyframe F (float64, then float32)."""
    R = F["Rcw"].reshape(3, 3).astype(f64)
    Pc = np.asarray(X, f64) @ R.T + F["tcw"].astype(f64)
    with np.errstate(all="ignore"):
        u = float(F["fx"]) * Pc[:, 0] / Pc[:, 2] + float(F["cx"])
        v = float(F["fy"]) * Pc[:, 1] / Pc[:, 2] + float(F["cy"])
    return u.astype(f32), v.astype(f32), Pc[:, 2].astype(f32)


def keys_of(u, v, octave=0):
    k = np.zeros(len(u), KEYPOINT_DTYPE)
    k["x"], k["y"] = u, v
    k["octave"] = octave
    k["size"], k["angle"], k["class_id"] = 31, 0, -1
    return k


def observe(F, X, octave=0, stereo=False, noise=None):
    """keys, ur, depth of world points seen by F; stereo: a bool or a bool array."""
    u, v, z = project(F, X)
    if noise is not None:
        u, v = (u + noise[:, 0]).astype(f32), (v + noise[:, 1]).astype(f32)
    st = np.broadcast_to(np.asarray(stereo, bool), u.shape)
    with np.errstate(all="ignore"):
        ur = np.where(st & (z > 0), u - F["mbf"] / z, f32(-1)).astype(f32)
    depth = np.where(st & (z > 0), z, f32(-1)).astype(f32)
    return keys_of(u, v, octave), ur, depth


def make(name, F1, F2, keys1, keys2, pairs=None, **kw):
    n = min(len(keys1), len(keys2))
    c = dict(name=name, pose1=F1, pose2=F2, keys1=keys1, keys2=keys2,
             pairs=np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32) if pairs is None
             else np.asarray(pairs, np.int32).reshape(-1, 2),
             raw1=None, raw2=None, ur1=None, ur2=None, depth1=None, depth2=None, cos1=None,
             cos2=None, mb=MB, ratio_factor=RATIO_FACTOR)
    c.update(kw)
    return c


def pair_case(name, F1, F2, X, st1=False, st2=False, oct1=0, oct2=0, **kw):
    k1, ur1, d1 = observe(F1, X, oct1, st1)
    k2, ur2, d2 = observe(F2, X, oct2, st2)
    return make(name, F1, F2, k1, k2, ur1=ur1, ur2=ur2, depth1=d1, depth2=d2, **kw)


def _with(case, **kw):
    c = dict(case)
    c.update(kw)
    return c


def _copy_pose(F, **fields):
    G = np.array(F, FRAME_POSE_DTYPE).reshape(()).copy()
    for k, v in fields.items():
        G[k] = v
    return G


def _bisect_key(case, field, lo, hi, pred):
    """Two neighbouring positive float32 x between lo and hi, pred false at the first and true at
    the second; pred(lo) must be false and pred(hi) true.  pred receives a case with keys2[0][field] = x."""
    def at(x):
        c = dict(case)
        k = case["keys2"].copy()
        k[field][0] = x
        c["keys2"] = k
        return c

    a, b = int(f32(lo).view(np.int32)), int(f32(hi).view(np.int32))
    assert a > 0 and b > 0 and not pred(at(f32(lo))) and pred(at(f32(hi)))
    while abs(b - a) > 1:
        mid = (a + b) // 2
        if pred(at(np.int32(mid).view(f32))):
            b = mid
        else:
            a = mid
    return at(np.int32(a).view(f32)), at(np.int32(b).view(f32))


def _cos_rays(case):
    return triangulate_np(case)[2][0]["cos_rays"]


def directed_cases():
    out = []
    F1 = pose()
    F2 = pose(centre=(0.5, 0, 0))
    X = np.array([[0.2, -0.1, 5.0], [-0.6, 0.3, 3.0], [1.0, 0.4, 8.0], [0.0, 0.0, 2.0]])
    far = np.array([[0.2, -0.1, 60.0], [-3.0, 2.0, 80.0]])
    Fn = pose(centre=(0.03, 0, 0))                # a baseline below the stereo baseline mb

    # every stereo combination, with enough parallax (the SVD branch) and with too little
    for s1 in (False, True):
        for s2 in (False, True):
            tag = f"st{int(s1)}{int(s2)}"
            out.append(pair_case(f"near_{tag}", F1, F2, X, s1, s2))
            out.append(pair_case(f"far_{tag}", F1, F2, far, s1, s2))
            out.append(pair_case(f"small_baseline_{tag}", F1, Fn, far, s1, s2))
    # octaves 0 and nlevels - 1 on either side: the scale test's two halves, and sigma2
    for o1, o2 in ((0, NLEVELS - 1), (NLEVELS - 1, 0), (NLEVELS - 1, NLEVELS - 1), (3, 4)):
        out.append(pair_case(f"octaves_{o1}_{o2}", F1, F2, X, oct1=o1, oct2=o2))
    # a scale ratio that the octaves explain: KF2 three times as far from the points
    F2far = pose(centre=(0.5, 0, -10.0))
    out.append(pair_case("octaves_explain_distance", F1, F2far, X, oct1=6, oct2=0))

    # :388 -- both stereo, tiny parallax: cosParallaxStereo1 (far depth, near 1) lets the SVD
    # branch run; reading cosParallaxStereo2 (a near depth) as well would select UnprojectStereo
    c = pair_case("quirk_388", F1, pose(centre=(0.05, 0, 0)), np.array([[0.1, 0.1, 20.0]]), True, True)
    c["cos1"] = np.array([f32(0.9999999)], f32)
    c["cos2"] = np.array([f32(0.99)], f32)
    out.append(c)
    # :482 -- keyframe 2 has another mbf; its right coordinate agrees with keyframe 1's mbf
    F2b = _copy_pose(F2, mbf=f32(80.0))
    c = pair_case("quirk_482", F1, F2b, X, False, True)
    with np.errstate(all="ignore"):
        c["ur2"] = (c["keys2"]["x"] - MBF / c["depth2"]).astype(f32)
    out.append(c)
    c = pair_case("quirk_482_own_mbf", F1, F2b, X, False, True)       # consistent with mbf2
    out.append(c)

    # equal poses: A has rank 3 with distinct keypoints (the null vector is the camera centre, a
    # point at a camera centre) and rank 2 with the same keypoint
    k1, _, _ = observe(F1, X)
    k2 = k1.copy()
    k2["x"] += f32(25)
    out.append(make("equal_poses_rank3", F1, F1, k1, k2))
    out.append(make("equal_poses_rank2_stereo", F1, F1, k1, k1.copy(),
                    ur1=(k1["x"] - f32(8)).astype(f32), depth1=np.full(len(k1), 5, f32),
                    cos1=np.full(len(k1), 2, f32)))
    Fc = pose(centre=(0, 0, 4.0))                 # points at KF2's camera centre
    out.append(pair_case("point_at_centre2", F1, Fc, np.array([[0.0, 0.0, 4.0], [1e-3, 0, 4.0]])))

    # W_ZERO: R = I, t1 = (4, 0, 0), t2 = (-4, 0, 0), equal x, opposite y: column 3 of A is
    # orthogonal to the others, is never rotated and does not hold the least singular value
    Fa = frame_pose(np.eye(3, dtype=f32), np.array([4, 0, 0], f32), K4, BOUNDS, scale_factors(), MBF)
    Fb = frame_pose(np.eye(3, dtype=f32), np.array([-4, 0, 0], f32), K4, BOUNDS, scale_factors(), MBF)
    out.append(make("w_zero", Fa, Fb, keys_of(f32([352.0]), f32([291.2])),
                    keys_of(f32([352.0]), f32([188.8]))))

    # BEHIND_1: the two keypoints exchanged, so the rays meet behind the cameras
    c = pair_case("behind_1", F1, F2, X)
    out.append(_with(c, keys1=c["keys2"], keys2=c["keys1"]))
    # BEHIND_2: UnprojectStereo of KF1, KF2 ahead of the point and looking the same way
    c = pair_case("behind_2", F1, pose(centre=(0, 0, 100.0)), far[:1], True, False)
    c["keys2"] = c["keys1"].copy()
    out.append(c)
    # z == 0 exactly (tcw is an input of its own): rejected by `<=`
    c = pair_case("z2_zero", F1, Fn, far[:1], True, False)
    Xs = triangulate_np(c)[1][0]
    assert triangulate_np(c)[0][0] == OK_STEREO1
    out.append(_with(c, name="z2_zero", pose2=_copy_pose(Fn, tcw=np.array([-0.03, 0, -Xs[2]], f32))))
    c = pair_case("z1_zero", F1, Fn, far[:1], False, True)
    Xs = triangulate_np(c)[1][0]
    assert triangulate_np(c)[0][0] == OK_STEREO2
    out.append(_with(c, name="z1_zero", pose1=_copy_pose(F1, tcw=np.array([0, 0, -Xs[2]], f32))))
    # DIST_ZERO: mOw of keyframe 1 (an input of its own) at the unprojected point
    out.append(_with(c, name="dist1_zero", pose1=_copy_pose(F1, Ow=Xs)))
    c = pair_case("dist2_zero", F1, Fn, far[:1], True, False)
    out.append(_with(c, pose2=_copy_pose(Fn, Ow=triangulate_np(c)[1][0])))

    # reprojection: a keypoint moved by a few pixels; mono (5.991) and stereo (7.8) forms
    for which in ("1", "2"):
        for px, octv in ((1.0, 0), (6.0, 0), (6.0, NLEVELS - 1), (40.0, NLEVELS - 1)):
            c = pair_case(f"reproj_{which}_{px:g}px_o{octv}", F1, F2, X, oct1=octv, oct2=octv)
            k = c["keys" + which].copy()
            k["y"] += f32(px)
            c["keys" + which] = k
            out.append(c)
    c = pair_case("reproj_2_mono", F1, F2, X, oct1=NLEVELS - 1, oct2=0)   # sigma2 of KF1 absorbs it
    k = c["keys2"].copy()
    k["y"] += f32(6)
    out.append(_with(c, keys2=k))
    for which, s1, s2 in (("1", True, False), ("2", False, True)):
        for px in (0.5, 2.0, 4.0):
            c = pair_case(f"reproj_stereo_{which}_{px:g}px", F1, Fn, far, s1, s2)
            c["ur" + which] = (c["ur" + which] + f32(px)).astype(f32)
            out.append(c)
    # raw keypoints differ from the undistorted ones: UnprojectStereo reads mvKeys
    c = pair_case("raw_keys", F1, Fn, far, True, True)
    r = c["keys1"].copy()
    r["x"] += f32(0.75)
    r["y"] -= f32(0.5)
    out.append(_with(c, raw1=r, raw2=c["keys2"].copy()))
    # a stereo feature without depth: UnprojectStereo returns nothing
    c = pair_case("stereo_without_depth", F1, Fn, far, True, False)
    out.append(_with(c, depth1=np.array([0.0, -1.0], f32), cos1=np.array([0.5, 0.5], f32)))

    # ---- thresholds of cosParallaxRays --------------------------------------------------------
    # cosParallaxStereo: the table entry at cosParallaxRays and one float either side
    base = pair_case("t", F1, pose(centre=(0.05, 0, 0)), np.array([[0.1, 0.1, 10.0]]), True, False)
    cr = _cos_rays(base)
    for tag, val in (("below", np.nextafter(cr, f32(-np.inf))), ("equal", cr),
                     ("above", np.nextafter(cr, f32(np.inf)))):
        out.append(_with(base, name=f"threshold_stereo1_{tag}", cos1=np.array([val], f32)))
    base2 = pair_case("t", F1, pose(centre=(0.05, 0, 0)), np.array([[0.1, 0.1, 10.0]]), False, True)
    cr = _cos_rays(base2)
    for tag, val in (("below", np.nextafter(cr, f32(-np.inf))), ("equal", cr),
                     ("above", np.nextafter(cr, f32(np.inf)))):
        out.append(_with(base2, name=f"threshold_stereo2_{tag}", cos2=np.array([val], f32)))
    # 0.9998 (a double): monocular, keypoint 2 moved until cosParallaxRays steps over it
    base = pair_case("t", F1, F2, np.array([[0.2, -0.1, 40.0]]))
    x0 = base["keys2"]["x"][0]
    lo, hi = _bisect_key(base, "x", x0, x0 - f32(20),
                         lambda c: float(_cos_rays(c)) < 0.9998)
    out.append(_with(lo, name="threshold_9998_at_or_above"))
    out.append(_with(hi, name="threshold_9998_below"))
    # 0: KF2 turned by a right angle, cx = cy = 0 and power-of-two focal lengths, so that the
    # dot product of the rays is y1 * y2 exactly
    Kz = (f32(512.0), f32(512.0), f32(0.0), f32(0.0))
    Fz1 = pose(K4_=Kz)
    Fz2 = pose(R=rot(1, 90), centre=(2.0, 0, 2.0), K4_=Kz)
    Fz2["Rcw"] = np.round(Fz2["Rcw"])             # exactly 0 / +-1
    tiny = f32(2.0 ** -66)
    for tag, y2 in (("neg", -tiny), ("zero", f32(0)), ("pos", tiny)):
        out.append(make(f"threshold_0_{tag}", Fz1, Fz2, keys_of(f32([0.0]), np.array([tiny * 2], f32)),
                        keys_of(f32([0.0]), np.array([y2], f32))))
    return out


RANDOM_SEEDS = (11, 12, 13, 14)
RANDOM_SEEDS_SHORT = (15,)        # baselines below the stereo baseline: the UnprojectStereo branches
RANDOM_PAIRS = 160


def random_case(seed, n=RANDOM_PAIRS, baseline=(0.3, 1.2)):
    """A seeded keyframe pair: baselines of 0.3-1.2 m, points 2-25 m ahead, pixel noise, a share
    of stereo features, random octaves, and a share of wrong matches."""
    rng = np.random.default_rng(seed)
    R1 = rot(0, rng.uniform(-8, 8)) @ rot(1, rng.uniform(-8, 8)) @ rot(2, rng.uniform(-5, 5))
    R2 = rot(0, rng.uniform(-8, 8)) @ rot(1, rng.uniform(-8, 8)) @ rot(2, rng.uniform(-5, 5))
    c1 = rng.uniform(-0.2, 0.2, 3)
    c2 = c1 + rng.uniform(*baseline) * np.array([1.0, rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3)])
    F1, F2 = pose(R1, c1), pose(R2, c2)
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(2, 25, n)], 1)
    X[: n // 8, 2] = rng.uniform(40, 120, n // 8)              # low parallax
    st1, st2 = rng.random(n) < 0.4, rng.random(n) < 0.4
    o1 = rng.integers(0, NLEVELS, n)
    o2 = np.clip(o1 + rng.integers(-1, 2, n), 0, NLEVELS - 1)
    o2[: n // 10] = rng.integers(0, NLEVELS, n // 10)
    sig = scale_factors()[o1][:, None]
    k1, ur1, d1 = observe(F1, X, o1, st1, (rng.normal(0, 0.6, (n, 2)) * sig).astype(f32))
    k2, ur2, d2 = observe(F2, X, o2, st2, (rng.normal(0, 0.6, (n, 2)) * sig).astype(f32))
    perm = np.arange(n)
    wrong = rng.choice(n, n // 8, replace=False)
    perm[wrong] = np.roll(wrong, 1)                            # wrong matches
    pairs = np.stack([np.arange(n), perm], 1).astype(np.int32)
    return make(f"random{seed}", F1, F2, k1, k2, pairs, ur1=ur1, ur2=ur2, depth1=d1, depth2=d2)


def random_cases():
    return ([random_case(s) for s in RANDOM_SEEDS] +
            [random_case(s, baseline=(0.01, 0.06)) for s in RANDOM_SEEDS_SHORT])


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = directed_cases() + random_cases()
        names = [c["name"] for c in _ALL]
        assert len(set(names)) == len(names), "case names are unique"
    return _ALL


def case_named(name):
    (c,) = [c for c in all_cases() if c["name"] == name]
    return c
