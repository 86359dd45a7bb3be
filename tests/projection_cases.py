"""The per-MapPoint projection loops of the six projection searches that orbx_project_map_points*
(k_project) runs, restated literally in numpy float32 / Python double, and directed cases for
them (numpy only; shared by tests/test_projection_cases.py on the CPU and
tests/test_gpu_projection.py on the GPU).

``project_np`` follows src/ORBmatcher.cc statement by statement, in the style of
tests/test_frustum.py::numpy_is_in_frustum: LAST_FRAME :1402-1458, KEYFRAME :1544-1596, KF_SCW
:321-390, FUSE :881-946, FUSE_SCW :1035-1105, SIM3 :1166-1247 (one direction; :1284-1327 is the
mirror).  Besides the queries it reports, per point, what happened to it (``OUTCOMES``), for
LAST_FRAME the search window kind, for the PredictScale modes the side of the level clamp, and
the intermediate values the census of tests/test_projection_cases.py looks at.

``variant=`` switches one decision of the restatement to a plausible wrong form; the CPU tests
require every variant to change at least one case, so each decision is pinned by a case.

A case is a dict: mode, name, job (PROJ_JOB_DTYPE record), mps (MAP_POINT_DTYPE), keys
(KEYPOINT_DTYPE or None: the source features of LAST_FRAME / KEYFRAME), skip (uint8 or None).
Invariant of the builder (asserted in ``_case``): the source octaves of every case lie in
[0, nlevels) -- the reference indexes mvScaleFactors[nLastOctave] unchecked, and what the library
does outside that range is its own definition, tested on the GPU only.
"""
import ctypes
import math

import numpy as np

from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import (MAP_POINT_DTYPE, PROJ_FUSE, PROJ_FUSE_SCW, PROJ_JOB_DTYPE,
                                       PROJ_KEYFRAME, PROJ_KF_SCW, PROJ_LAST_FRAME,
                                       PROJ_QUERY_DTYPE, PROJ_SIM3, frame_pose, proj_job)

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
_libm.ceilf.restype = ctypes.c_float
_libm.ceilf.argtypes = [ctypes.c_float]
f32 = np.float32
INT_MIN = -2 ** 31

MODES = (PROJ_KF_SCW, PROJ_LAST_FRAME, PROJ_KEYFRAME, PROJ_FUSE, PROJ_FUSE_SCW, PROJ_SIM3)
MODE_NAMES = {PROJ_KF_SCW: "KF_SCW", PROJ_LAST_FRAME: "LAST_FRAME", PROJ_KEYFRAME: "KEYFRAME",
              PROJ_FUSE: "FUSE", PROJ_FUSE_SCW: "FUSE_SCW", PROJ_SIM3: "SIM3"}
FRAME_MODES = (PROJ_LAST_FRAME, PROJ_KEYFRAME)            # Frame bounds, (fx*xc)*invz
NORMAL_MODES = (PROJ_KF_SCW, PROJ_FUSE, PROJ_FUSE_SCW)    # the viewing-angle test
FLOAT_INVZ_MODES = (PROJ_KF_SCW, PROJ_FUSE)               # 1 / z on floats
UR_MODES = (PROJ_LAST_FRAME, PROJ_FUSE)

OUTCOMES = ("skipped", "depth", "bounds_u", "bounds_v", "range_low", "range_high", "normal",
            "active")
WINDOWS = ("forward", "backward", "default")
CLAMPS = ("below", "above", "inside")


def outcomes_of(mode):
    """The outcome codes the reference's loop of `mode` can produce."""
    out = ["skipped", "bounds_u", "bounds_v", "active"]
    if mode != PROJ_KEYFRAME:
        out.append("depth")
    if mode != PROJ_LAST_FRAME:
        out += ["range_low", "range_high"]
    if mode in NORMAL_MODES:
        out.append("normal")
    return out


VARIANTS = {
    # name: the modes whose result it can change
    "frame_min_strict": FRAME_MODES,          # u <= min_x rejects
    "frame_max_strict": FRAME_MODES,          # u >= max_x rejects
    "kf_min_strict": tuple(m for m in MODES if m not in FRAME_MODES),     # u > min_x keeps
    "kf_max_inclusive": tuple(m for m in MODES if m not in FRAME_MODES),  # u <= max_x keeps
    "depth_flip": MODES,                      # the z < 0 test where there is none, none where it is
    "u_assoc": MODES,                         # (fx*xc)*invz <-> fx*(xc*invz)
    "norm_f32": tuple(m for m in MODES if m != PROJ_LAST_FRAME),
    "dot_f32": NORMAL_MODES,
    "half_d_f32": NORMAL_MODES,               # (float)dot < 0.5f*d
    "max_level_L": FRAME_MODES,               # L for L + 1 in the default window
    "windows_swapped": (PROJ_LAST_FRAME,),
    "threshold_nonstrict": (PROJ_LAST_FRAME,),   # tlc.z >= mb
}
# Variants that provably cannot change a bit, so no case pretends to pin them:
#  * 1.0f / z against (float)(1.0 / (double)z): z converts to double exactly, and rounding a
#    quotient to 53 bits and then to 24 equals rounding it to 24 bits directly whenever the wide
#    format has at least 2*24 + 2 bits (double rounding is innocuous for + - * / sqrt then); the
#    restatement still writes each mode's own form.
#  * `+ tcw` in float against (float)((double)t + (double)tcw): the same argument for the sum.
#  * `< 0.0` (double) against `< 0.0f` on a float z: the conversion is exact.
#  * 0.5 * (double)d against (double)(0.5f * d): halving is exact (d is a norm, never subnormal
#    here) -- what half_d_f32 changes is the rounding of the dot product to float.


def _gemm(R, P, t):
    """cv::gemm(R, P, 1, t, 1), small-matrix path: float products summed left to right, + t in
    double, rounded to float."""
    out = []
    for r in range(3):
        s = f32(f32(R[3 * r] * P[0]) + f32(R[3 * r + 1] * P[1]))
        s = f32(s + f32(R[3 * r + 2] * P[2]))
        out.append(f32(float(s) + float(t[r])))
    return out


def _norm(a, in_f32=False):
    if in_f32:
        ss = f32(0)
        for k in range(3):
            ss = f32(ss + f32(a[k] * a[k]))
        return f32(np.sqrt(ss))
    ss = 0.0
    for k in range(3):
        ss += float(a[k]) * float(a[k])
    return f32(math.sqrt(ss)) if ss == ss and ss >= 0 else f32(np.nan)


def trunc_x86(v) -> int:
    v = float(v)
    return int(v) if v == v and -2.0 ** 31 <= v < 2.0 ** 31 else INT_MIN


def last_frame_window(job, variant=None):
    """forward / backward / default for a LAST_FRAME job (ORBmatcher.cc:1405-1410)."""
    cam = job["cam"]
    tlc = _gemm(job["pre_R"], cam["Ow"], job["pre_t"])
    mb, mono = job["mb"], bool(job["mono"])
    if variant == "threshold_nonstrict":
        fwd, bwd = tlc[2] >= mb and not mono, -tlc[2] >= mb and not mono
    else:
        fwd, bwd = tlc[2] > mb and not mono, -tlc[2] > mb and not mono
    if variant == "windows_swapped":
        fwd, bwd = bwd, fwd
    return ("forward" if fwd else "backward" if bwd else "default"), tlc[2]


def project_np(mode, job, mps, src_keys=None, skip=None, variant=None):
    """-> (queries PROJ_QUERY_DTYPE, nactive, info).  info: per-point 'outcome' (OUTCOMES),
    'window' (WINDOWS or ''), 'clamp' (CLAMPS or ''), and the float values 'z', 'u', 'v', 'd',
    'dot' (NaN where not computed), plus 'tlc_z' for LAST_FRAME."""
    n = len(mps)
    q = np.zeros(n, PROJ_QUERY_DTYPE)
    q["radius"] = -1.0
    q["min_level"] = q["max_level"] = q["pred_level"] = -1
    info = dict(outcome=["skipped"] * n, window=[""] * n, clamp=[""] * n,
                z=np.full(n, np.nan, f32), u=np.full(n, np.nan, f32), v=np.full(n, np.nan, f32),
                d=np.full(n, np.nan, f32), dot=np.full(n, np.nan, np.float64))
    job = np.asarray(job, PROJ_JOB_DTYPE).reshape(())
    F = job["cam"]
    nlevels = int(F["nlevels"])
    frame = mode in FRAME_MODES
    th = f32(job["th"])
    window = None
    if mode == PROJ_LAST_FRAME:
        window, info["tlc_z"] = last_frame_window(job, variant)
    if not 1 <= nlevels <= 16:
        return q, 0, info              # library-defined: such a job produces nothing
    depth_test = mode != PROJ_KEYFRAME
    if variant == "depth_flip":
        depth_test = not depth_test
    nact = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            if skip is not None and skip[i]:
                continue
            m = mps[i]
            P = m["pos"]
            if mode == PROJ_SIM3:
                Pc = _gemm(F["Rcw"], _gemm(job["pre_R"], P, job["pre_t"]), F["tcw"])
            else:
                Pc = _gemm(F["Rcw"], P, F["tcw"])
            z = Pc[2]
            info["z"][i] = z
            if mode != PROJ_LAST_FRAME and depth_test and z < f32(0):
                info["outcome"][i] = "depth"
                continue
            if mode in FLOAT_INVZ_MODES:
                invz = f32(f32(1.0) / z)
            else:
                invz = f32(np.float64(1.0) / np.float64(z))
            if mode == PROJ_LAST_FRAME and depth_test and invz < f32(0):
                info["outcome"][i] = "depth"
                continue
            if frame != (variant == "u_assoc"):
                u = f32(f32(f32(F["fx"] * Pc[0]) * invz) + F["cx"])
                v = f32(f32(f32(F["fy"] * Pc[1]) * invz) + F["cy"])
            else:
                x, y = f32(Pc[0] * invz), f32(Pc[1] * invz)
                u = f32(f32(F["fx"] * x) + F["cx"])
                v = f32(f32(F["fy"] * y) + F["cy"])
            info["u"][i], info["v"][i] = u, v
            if frame:
                lo = (lambda a, b: a <= b) if variant == "frame_min_strict" else (lambda a, b: a < b)
                hi = (lambda a, b: a >= b) if variant == "frame_max_strict" else (lambda a, b: a > b)
                if lo(u, F["min_x"]) or hi(u, F["max_x"]):
                    info["outcome"][i] = "bounds_u"
                    continue
                if lo(v, F["min_y"]) or hi(v, F["max_y"]):
                    info["outcome"][i] = "bounds_v"
                    continue
            else:
                ge = (lambda a, b: a > b) if variant == "kf_min_strict" else (lambda a, b: a >= b)
                lt = (lambda a, b: a <= b) if variant == "kf_max_inclusive" else (lambda a, b: a < b)
                if not (ge(u, F["min_x"]) and lt(u, F["max_x"])):
                    info["outcome"][i] = "bounds_u"
                    continue
                if not (ge(v, F["min_y"]) and lt(v, F["max_y"])):
                    info["outcome"][i] = "bounds_v"
                    continue
            if mode == PROJ_LAST_FRAME:
                lvl = int(src_keys["octave"][i])
                assert 0 <= lvl < nlevels, "project_np: source octave outside [0, nlevels)"
            else:
                PO = None
                if mode == PROJ_SIM3:
                    d = _norm(Pc, variant == "norm_f32")
                else:
                    PO = [f32(P[k] - F["Ow"][k]) for k in range(3)]
                    d = _norm(PO, variant == "norm_f32")
                info["d"][i] = d
                maxd, mind = f32(f32(1.2) * m["max_dist"]), f32(f32(0.8) * m["min_dist"])
                if d < mind:
                    info["outcome"][i] = "range_low"
                    continue
                if d > maxd:
                    info["outcome"][i] = "range_high"
                    continue
                if mode in NORMAL_MODES:
                    if variant == "dot_f32":
                        dot = f32(0)
                        for k in range(3):
                            dot = f32(dot + f32(PO[k] * m["normal"][k]))
                        dot = float(dot)
                    else:
                        dot = 0.0
                        for k in range(3):
                            dot += float(PO[k]) * float(m["normal"][k])
                    info["dot"][i] = dot
                    if variant == "half_d_f32":
                        rej = f32(dot) < f32(f32(0.5) * d)
                    else:
                        rej = dot < 0.5 * float(d)
                    if rej:
                        info["outcome"][i] = "normal"
                        continue
                ratio = f32(m["max_dist"] / d)
                qf = _libm.ceilf(f32(f32(_libm.logf(ratio)) / F["log_scale_factor"]))
                lvl = trunc_x86(qf)
                if lvl < 0:
                    lvl, info["clamp"][i] = 0, "below"
                elif lvl >= nlevels:
                    lvl, info["clamp"][i] = nlevels - 1, "above"
                else:
                    info["clamp"][i] = "inside"
            radius = f32(th * F["scale"][lvl])
            ur = f32(u - f32(F["mbf"] * invz)) if mode in UR_MODES else f32(0)
            up = lvl if variant == "max_level_L" else lvl + 1
            if mode == PROJ_KEYFRAME:
                lv = (lvl - 1, up)
            elif mode == PROJ_LAST_FRAME:
                info["window"][i] = window
                lv = {"forward": (lvl, -1), "backward": (0, lvl), "default": (lvl - 1, up)}[window]
            else:
                lv = (-1, -1)
            ang = src_keys["angle"][i] if frame else f32(0)
            q[i] = (u, v, ur, radius, lv[0], lv[1], lvl, ang)
            info["outcome"][i] = "active"
            nact += 1
    return q, nact, info


# ---- case building ------------------------------------------------------------------------------

def _case(mode, name, job, mps, keys=None, skip=None):
    mps = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
    n = len(mps)
    assert n <= 1000
    if mode in FRAME_MODES:
        if keys is None:
            keys = _keys(n, int(job["cam"]["nlevels"]), seed=n + mode)
        keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
        assert len(keys) == n
        nl = int(job["cam"]["nlevels"])
        if 1 <= nl <= 16:   # the invariant: valid cases keep source octaves in [0, nlevels)
            assert ((keys["octave"] >= 0) & (keys["octave"] < nl)).all(), name
    else:
        keys = None
    if skip is not None:
        skip = np.ascontiguousarray(skip, np.uint8)
        assert len(skip) == n
    return dict(mode=mode, name=f"{MODE_NAMES[mode]}/{name}", job=job, mps=mps, keys=keys, skip=skip)


def _keys(n, nlevels, seed=0, octave=None):
    rng = np.random.default_rng(1000 + seed)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["octave"] = rng.integers(0, max(nlevels, 1), n) if octave is None else octave
    k["angle"] = rng.uniform(0, 360, n).astype(f32)
    k["x"], k["y"] = rng.uniform(0, 300, n), rng.uniform(0, 300, n)
    return k


NEG0 = f32(-0.0)


def exact_job(mode, th=3.0, nlevels=8, c=0.0, pre_tz=NEG0, mb=0.5, mono=False,
              scale_factor=1.2, log_scale_factor=None):
    """Identity rotations and power-of-two intrinsics: fx = fy = 256, cx = cy = c, bounds
    [64, 320] x [32, 288], so u = 256 * x / z + c is exact where z is a power of two.  tcw.z and
    (SIM3) pre_t.z are -0.0 so that a negative-zero depth survives the additions; Ow = 0.  For
    LAST_FRAME tlc.z = pre_t.z (pre_R = I, Ow = 0)."""
    scale = synth.scale_tables(nlevels, scale_factor)[0] if nlevels >= 1 else np.ones(1, f32)
    cam = frame_pose(np.eye(3), (0, 0, NEG0), (256, 256, c, c), (64, 320, 32, 288), scale[:16],
                     mbf=32.0, scale_factor=scale_factor)
    cam["Ow"] = 0
    cam["nlevels"] = nlevels
    if log_scale_factor is not None:
        cam["log_scale_factor"] = log_scale_factor
    return proj_job(cam, th, np.eye(3), (0, 0, pre_tz), mb, mono)


def mp(P, min_dist=0.0, max_dist=None, normal=None, lvl=2):
    """One MapPoint record; by default in range with PredictScale = lvl and the normal along the
    viewing ray from the origin."""
    r = np.zeros((), MAP_POINT_DTYPE)
    r["pos"] = np.asarray(P, f32)
    d = float(np.linalg.norm(np.asarray(P, np.float64)))
    d = d if np.isfinite(d) and d > 0 else 1.0
    r["min_dist"] = f32(min_dist)
    r["max_dist"] = f32(d * 1.2 ** (lvl - 0.5)) if max_dist is None else f32(max_dist)
    if normal is None:
        P64 = np.nan_to_num(np.asarray(P, np.float64), nan=0.0, posinf=1.0, neginf=-1.0)
        normal = P64 / d
    r["normal"] = np.asarray(normal, f32)
    return r


def _stack(points):
    return np.array(points, MAP_POINT_DTYPE)


def _at_pixel(u, v, z=1.0, c=0.0, **kw):
    """The point that projects exactly to (u, v) under exact_job(c=c) when z is a power of 2."""
    z = f32(z)
    return mp((f32(f32(f32(u) - f32(c)) / f32(256)) * z, f32(f32(f32(v) - f32(c)) / f32(256)) * z, z),
              **kw)


def directed_cases(mode):
    cases = []
    up, dn = (lambda a: np.nextafter(f32(a), f32(np.inf))), (lambda a: np.nextafter(f32(a), f32(-np.inf)))
    J = exact_job(mode)

    # u (v) exactly at the bounds and one float either side
    pts = [_at_pixel(u, 100.0) for u in (dn(64), 64, up(64), dn(320), 320, up(320))]
    pts += [_at_pixel(100.0, v) for v in (dn(32), 32, up(32), dn(288), 288, up(288))]
    pts += [_at_pixel(dn(64), dn(32)), _at_pixel(up(320), up(288)), _at_pixel(128, 128, 2.0)]
    cases.append(_case(mode, "bounds", J, _stack(pts)))

    # the depth values against the mode's rule.  -0.0 needs x < 0 and y < 0 (every term of the
    # gemm row a negative zero); a negative z with x, y < 0 lands in bounds.
    tiny = f32(-1e-30)
    pts = [mp((0.0, 0.0, 0.0)), mp((0.5, 0.5, 0.0)), mp((-0.5, -0.5, NEG0)), mp((0.0, 0.0, NEG0)),
           mp((-0.5, -0.5, tiny)), mp((-0.5, -0.5, -1.0), lvl=3), mp((0.5, 0.5, -1.0)),
           mp((-1.0, -0.75, -2.0), lvl=1), mp((0.5, 0.5, np.nan)), mp((0.5, 0.5, np.inf)),
           mp((0.5, 0.5, -np.inf)), mp((0.5, 0.5, 1.0)), mp((0.0, 0.0, 1.0)),
           mp((1e30, 0.5, 1e-30))]
    cases.append(_case(mode, "depth", J, _stack(pts)))

    # the same depths reached through tcw.z alone (P.z = 0)
    for name, tz in (("tz+0", 0.0), ("tz-0", NEG0), ("tz-1", -1.0), ("tz_nan", np.nan),
                     ("tz_inf", np.inf), ("tz_tiny", 1e-38)):
        Jt = exact_job(mode, c=192.0)
        Jt["cam"]["tcw"][2] = tz
        pts = [mp((0.0, 0.0, 0.0)), mp((-0.25, -0.25, NEG0)), mp((0.25, 0.25, 0.0)),
               mp((1e-38, 1e-38, 0.0))]
        cases.append(_case(mode, "depth_" + name, Jt, _stack(pts)))

    # d equal to 0.8f * min and 1.2f * max, and one float outside each (P on the optical axis,
    # cx = cy = 192: d = z exactly)
    Jc = exact_job(mode, c=192.0)
    pts = []
    for mn in (5.0, 0.3, 7.7):
        lo = f32(f32(0.8) * f32(mn))
        pts += [mp((0, 0, lo), min_dist=mn, max_dist=100.0), mp((0, 0, dn(lo)), min_dist=mn, max_dist=100.0),
                mp((0, 0, up(lo)), min_dist=mn, max_dist=100.0)]
    for mx in (5.0, 0.3, 7.7):
        hi = f32(f32(1.2) * f32(mx))
        pts += [mp((0, 0, hi), max_dist=mx), mp((0, 0, up(hi)), max_dist=mx), mp((0, 0, dn(hi)), max_dist=mx)]
    pts += [mp((0, 0, 4.0), min_dist=np.nan, max_dist=np.nan), mp((0, 0, 4.0), min_dist=np.inf, max_dist=np.inf),
            mp((0, 0, 4.0), min_dist=9.0, max_dist=1.0)]
    cases.append(_case(mode, "range", Jc, _stack(pts)))

    # dot == 0.5 * d exactly (kept) and one double ulp below (dropped): P = (2^-30, 0, 4) has
    # d = 4 (2^-60 vanishes under 16 in double), and normal (-2^-22, 0, 0.5) gives
    # dot = -2^-52 + 2 = 2 - 2^-52, the double just below 2 = 0.5 * d.  In float32 the dot product
    # rounds to 2 and the point would stay.
    e = 2.0 ** -30
    pts = [mp((e, 0, 4.0), normal=(0, 0, 0.5), max_dist=8.0), mp((e, 0, 4.0), normal=(-2.0 ** -22, 0, 0.5), max_dist=8.0),
           mp((0, 0, 4.0), normal=(0, 0, 0.5), max_dist=8.0), mp((0, 0, 4.0), normal=(0, 0, dn(0.5)), max_dist=8.0),
           mp((0, 0, 4.0), normal=(0, 0, -1.0), max_dist=8.0), mp((0, 0, 4.0), normal=(np.nan, 0, 1.0), max_dist=8.0),
           mp((e, 0, 4.0), normal=(2.0 ** -22, 0, 0.5), max_dist=8.0), mp((0.25, 0.25, 4.0), normal=(1.0, 0, 0), max_dist=8.0)]
    cases.append(_case(mode, "normal", Jc, _stack(pts)))

    # PredictScale: below 0 (needs a scale factor under 1.2: a ratio under 1 / 1.2 is out of
    # range first), at or above nlevels, exact-integer quotients, a NaN ratio; nlevels 1, 8, 16
    for nl in (1, 8, 16):
        Jp = exact_job(mode, c=192.0, nlevels=nl, scale_factor=1.05)
        lsf = Jp["cam"]["log_scale_factor"]
        pts = [mp((0, 0, 8.0), max_dist=8.0 * 0.9), mp((0, 0, 8.0), max_dist=8.0 * 0.84),
               mp((0, 0, 8.0), max_dist=8.0), mp((0, 0, 8.0), max_dist=f32(1.05) * f32(8.0)),
               mp((0, 0, 8.0), max_dist=8.0 * 1.05 ** 6.5), mp((0, 0, 8.0), max_dist=8.0 * 1.05 ** 15.5),
               mp((0, 0, 8.0), max_dist=8.0 * 1.05 ** 40), mp((0, 0, 8.0), max_dist=np.nan),
               mp((0, 0, 8.0), max_dist=np.inf), mp((0, 0, 8.0), max_dist=3e38),
               mp((0, 0, 8.0), max_dist=8.0 * 1.05 ** 0.5), mp((0, 0, 8.0), max_dist=up(8.0))]
        assert _libm.logf(f32(1.05)) == lsf
        cases.append(_case(mode, f"predict_scale_nl{nl}", Jp, _stack(pts)))
    Jp = exact_job(mode, c=192.0)          # the reference's 1.2: quotient exactly 1 and exactly 0
    pts = [mp((0, 0, 8.0), max_dist=f32(1.2) * f32(8.0)), mp((0, 0, 8.0), max_dist=8.0),
           mp((0, 0, 8.0), max_dist=8.0 * 1.2 ** 30)] + [mp((0, 0, 8.0), lvl=l) for l in range(9)]
    cases.append(_case(mode, "predict_scale_1.2", Jp, _stack(pts)))

    # th of 1, 3, 7, 10 and 15
    for th in (1, 3, 7, 10, 15):
        pts = [mp((0.01 * k, -0.02 * k, 2.0 + k), lvl=k % 8) for k in range(8)]
        cases.append(_case(mode, f"th{th}", exact_job(mode, th=th, c=192.0), _stack(pts)))

    # skip flags interleaved with active points
    pts = [mp((0.01 * k, 0.01 * k, 3.0), lvl=k % 8) for k in range(41)]
    cases.append(_case(mode, "skip", Jc, _stack(pts), skip=(np.arange(41) % 3 == 1)))

    # a job the library refuses: nlevels outside [1, 16]
    for nl in (0, 17, -3):
        Jn = exact_job(mode, c=192.0)
        Jn["cam"]["nlevels"] = nl
        cases.append(_case(mode, f"nlevels{nl}", Jn, _stack(pts[:5]), keys=_keys(5, 1)))

    if mode == PROJ_LAST_FRAME:
        # tlc.z == mb and -tlc.z == mb (neither window), one float above each, mono with a large
        # tlc.z; octaves 0 .. nlevels-1 in each (octave 0: min_level -1 in the default window)
        mb = f32(0.5)
        for name, tz, mono in (("tlc==mb", mb, False), ("tlc>mb", up(mb), False),
                               ("-tlc==mb", -mb, False), ("-tlc>mb", dn(-mb), False),
                               ("mono_fwd", 5.0, True), ("mono_bwd", -5.0, True),
                               ("tlc_nan", np.nan, False), ("tlc0", 0.0, False)):
            Jw = exact_job(mode, c=192.0, pre_tz=tz, mb=mb, mono=mono)
            pts = [mp((0.02 * k, 0.01 * k, 2.0)) for k in range(8)]
            cases.append(_case(mode, "window_" + name, Jw, _stack(pts),
                               keys=_keys(8, 8, octave=np.arange(8))))
        for nl in (1, 16):
            Jw = exact_job(mode, c=192.0, nlevels=nl)
            pts = [mp((0.02 * k, 0.01 * k, 2.0)) for k in range(nl)]
            cases.append(_case(mode, f"octaves_nl{nl}", Jw, _stack(pts),
                               keys=_keys(nl, nl, octave=np.arange(nl))))
    return cases


# ---- random scenes --------------------------------------------------------------------------------

def _scene_keys(seed, n=800, w=752, h=480):
    rng = np.random.default_rng(seed)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(20, w - 20, n), rng.uniform(20, h - 20, n)
    k["octave"] = rng.integers(0, 8, n)
    k["angle"] = rng.uniform(0, 360, n)
    return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def job_from_pose(mode, pose, seed, th=None):
    """The job of `mode` that views a scene through `pose` (a frame_pose record).  SIM3: a random
    first transform (R1w, t1w) with cam = pose composed with its inverse, so the points land where
    `pose` alone puts them; LAST_FRAME: a random last-frame pose, stereo."""
    rng = np.random.default_rng(seed)
    th = {PROJ_KF_SCW: 10, PROJ_LAST_FRAME: 7, PROJ_KEYFRAME: 10, PROJ_FUSE: 3, PROJ_FUSE_SCW: 4,
          PROJ_SIM3: 7.5}[mode] if th is None else th
    cam = pose.copy()
    pre_R = pre_t = None
    mb, mono = 0.0, True
    if mode == PROJ_SIM3:
        R1, t1 = synth._rot(rng, 30.0), rng.normal(0, 1.0, 3)
        R = pose["Rcw"].reshape(3, 3).astype(np.float64)
        Rc = R @ R1.T
        cam["Rcw"] = Rc.astype(f32).reshape(9)
        cam["tcw"] = (pose["tcw"].astype(np.float64) - Rc @ t1).astype(f32)
        pre_R, pre_t = R1, t1
    elif mode == PROJ_LAST_FRAME:
        pre_R, pre_t = synth._rot(rng, 10.0), rng.normal(0, 0.5, 3)
        mb, mono = 0.08, bool(seed % 3 == 2)
    return proj_job(cam, th, pre_R, pre_t, mb, mono)


def random_cases(mode, seeds=(3, 11), n=500):
    """synth.local_map_points scenes (behind the camera, outside in u, out of range both ways,
    oblique normals, skips) with a few points pushed outside in v as well."""
    K4, _ = synth.EUROC_CAM
    bounds = (0.0, 752.0, 0.0, 480.0)
    cases = []
    for seed in seeds:
        keys, desc = _scene_keys(seed)
        pose, mps, _, skip = synth.local_map_points(seed, keys, desc, n, K4, bounds, mbf=40.0,
                                                    outside_frac=0.3)
        rng = np.random.default_rng(seed + 77)
        R, t = pose["Rcw"].reshape(3, 3).astype(np.float64), pose["tcw"].astype(np.float64)
        for i in rng.choice(n, 25, replace=False):       # v pushed out of the image
            Pc = R @ mps["pos"][i].astype(np.float64) + t
            Pc[1] += (1 if i % 2 else -1) * 480.0 / K4[1] * Pc[2]
            mps["pos"][i] = (R.T @ (Pc - t)).astype(f32)
        job = job_from_pose(mode, pose, seed)
        src = _keys(n, 8, seed=seed) if mode in FRAME_MODES else None
        cases.append(_case(mode, f"random{seed}", job, mps, src, skip))
    return cases


_CACHE = {}


def all_cases(mode):
    if mode not in _CACHE:
        _CACHE[mode] = directed_cases(mode) + random_cases(mode)
    return _CACHE[mode]


_REF = {}


def reference(case, variant=None):
    """project_np of a case, computed once and shared (the arrays must not be modified)."""
    key = (case["name"], variant)
    if key not in _REF:
        _REF[key] = project_np(case["mode"], case["job"], case["mps"], case["keys"], case["skip"],
                               variant)
    return _REF[key]


# ---- MapPoints that observe a featureset's features (the end-to-end tests) ----------------------

def random_pose(seed, K4, bounds, mbf=40.0, nlevels=8):
    rng = np.random.default_rng(seed)
    return frame_pose(synth._rot(rng, 20.0), rng.normal(0, 1.0, 3), K4, bounds,
                      synth.scale_tables(nlevels)[0], mbf=mbf)


def mappoints_onto(seed, pose, keys, target, nlevels=8, scale_factor=1.2, jitter=0.7, depth=None):
    """One MapPoint per entry of `target`: it projects through `pose` within ~`jitter` px of
    keys[target[i]] (anywhere in the image where target[i] < 0), at a depth of 2..30 (or the
    feature's `depth` where that is positive), with the viewing ray as its normal and a
    mfMaxDistance that puts PredictScale at the feature's octave."""
    rng = np.random.default_rng(seed)
    n = len(target)
    fx, fy, cx, cy = (float(pose[k]) for k in ("fx", "fy", "cx", "cy"))
    has = np.asarray(target) >= 0
    ti = np.maximum(target, 0)
    u = np.where(has, keys["x"][ti] + rng.normal(0, jitter, n),
                 rng.uniform(float(pose["min_x"]) + 1, float(pose["max_x"]) - 1, n))
    v = np.where(has, keys["y"][ti] + rng.normal(0, jitter, n),
                 rng.uniform(float(pose["min_y"]) + 1, float(pose["max_y"]) - 1, n))
    lvl = np.where(has, keys["octave"][ti], rng.integers(0, nlevels, n))
    Z = rng.uniform(2.0, 30.0, n)
    if depth is not None:
        dz = np.asarray(depth, np.float64)[ti]
        Z = np.where(has & (dz > 0), dz, Z)
    R, t = pose["Rcw"].reshape(3, 3).astype(np.float64), pose["tcw"].astype(np.float64)
    Pc = np.stack([(u - cx) / fx * Z, (v - cy) / fy * Z, Z], 1)
    P = (Pc - t[None, :]) @ R
    PO = P + (R.T @ t)[None, :]
    dist = np.linalg.norm(PO, axis=1)
    out = np.zeros(n, MAP_POINT_DTYPE)
    out["pos"] = P.astype(f32)
    out["normal"] = (PO / dist[:, None]).astype(f32)
    out["max_dist"] = (dist * float(scale_factor) ** (lvl - 0.5)).astype(f32)
    out["min_dist"] = out["max_dist"] / f32(float(scale_factor) ** (nlevels - 1))
    return out
