"""The RGB-D front-end's three reference pieces restated literally in numpy float32 / Python
double, and directed cases for them (numpy only; shared by tests/test_rgbd_cases.py on the CPU
and tests/test_gpu_rgbd.py on the GPU).

* ``depth_rule`` / ``compute_stereo_from_rgbd``: Tracking.cc:244-245 (imDepth.convertTo(CV_32F,
  mDepthMapFactor) when fabs(mDepthMapFactor - 1.0f) > 1e-5 or the image is not CV_32F; OpenCV 3.2
  cvtScale_: one float multiply) and Frame::ComputeStereoFromRGBD (Frame.cc:689-710).
* ``unproject``: Frame::UnprojectStereo (Frame.cc:713-727), Rwc * x3Dc + Ow in cv::gemm's
  small-matrix form as tests/test_frustum.py restates it.
* ``close_points_ref``: Tracking::UpdateLastFrame's loop (Tracking.cc:862-912; CreateNewKeyFrame
  :1164-1217 is the same loop) as a Python sorted() of (z, i) tuples and the loop with its break,
  plus NeedNewKeyFrame's counts (:1080-1089).

Directed cases are deterministic in a seed and plant, per keypoint, the outcome it must have.
Depth images are 64x48 inside an allocation with a padded row stride and one spare row and
column, all filled with a valid depth, so that a broken bounds guard reads owned memory and
shows up as a wrong (valid) answer instead of a fault.
"""
import numpy as np

from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import DEPTH_F32, DEPTH_U16, frame_pose

f32 = np.float32
W, H = 64, 48
ROW_ELEMS = W + 1 + 7          # one spare column, then padding
ALLOC_ROWS = H + 1             # one spare row
INT_MIN = -2 ** 31
TUM_FACTOR = f32(1.0) / f32(5000.0)   # Tracking.cc:159-163: mDepthMapFactor = 1.0f / 5000
FACTORS = {"one": f32(1.0), "tum": TUM_FACTOR, "one+5e-6": f32(1.0 + 5e-6),
           "one+2e-5": f32(1.0 + 2e-5)}


def trunc_x86(v) -> int:
    """(int)v of a float on x86-64 (cvttss2si): truncation, INT_MIN for NaN / out of range."""
    v = float(f32(v))
    if v != v or not (-2.0 ** 31 <= v < 2.0 ** 31):
        return INT_MIN
    return int(v)


def scales(depth_type: int, factor) -> bool:
    """Tracking.cc:244: is the image converted at all?"""
    return bool(abs(f32(f32(factor) - f32(1.0))) > 1e-5) or depth_type != DEPTH_F32


def depth_rule(raw, depth_type: int, factor):
    """The float depth of one raw pixel."""
    factor = f32(factor)
    if depth_type == DEPTH_U16:
        return f32(f32(int(raw)) * factor)
    if abs(f32(factor - f32(1.0))) > 1e-5:
        return f32(f32(raw) * factor)
    return f32(raw)


def compute_stereo_from_rgbd(img, depth_type, factor, mbf, kps, kps_un):
    """Frame.cc:689-710 on the H x W view `img` of the raw depth image; a pixel outside the image
    gives -1 / -1 (the reference reads out of bounds there)."""
    h, w = img.shape
    n = len(kps)
    ur = np.full(n, -1.0, f32)
    de = np.full(n, -1.0, f32)
    with np.errstate(all="ignore"):
        for i in range(n):
            col, row = trunc_x86(kps["x"][i]), trunc_x86(kps["y"][i])
            if not (0 <= col < w and 0 <= row < h):
                continue
            d = depth_rule(img[row, col], depth_type, factor)
            if d > 0:
                de[i] = d
                ur[i] = f32(kps_un["x"][i] - f32(f32(mbf) / d))
    return ur, de


def unproject(F, u, v, z):
    """Frame::UnprojectStereo for z > 0: three float32 values."""
    with np.errstate(all="ignore"):
        invfx, invfy = f32(f32(1.0) / F["fx"]), f32(f32(1.0) / F["fy"])
        u, v, z = f32(u), f32(v), f32(z)
        c = [f32(f32(f32(u - F["cx"]) * z) * invfx), f32(f32(f32(v - F["cy"]) * z) * invfy), z]
        Rwc = F["Rcw"].reshape(3, 3).T
        out = np.zeros(3, f32)
        for r in range(3):
            s = f32(f32(Rwc[r, 0] * c[0]) + f32(Rwc[r, 1] * c[1]))
            s = f32(s + f32(Rwc[r, 2] * c[2]))
            out[r] = f32(float(s) + float(F["Ow"][r]))
    return out


def unproject_all(F, keys, depth, x3d=None):
    n = len(keys)
    out = np.zeros((n, 3), f32) if x3d is None else x3d.copy()
    valid = np.zeros(n, np.uint8)
    for i in range(n):
        if depth[i] > 0:
            out[i] = unproject(F, keys["x"][i], keys["y"][i], depth[i])
            valid[i] = 1
    return out, valid


def close_points_ref(F, keys, depth, th, has_point=None, tracked=None, min_points=100):
    """(order [M], counts {M, V, nTrackedClose, nNonTrackedClose}, create [V], x3d [V, 3])."""
    th = float(f32(th))
    v = sorted((float(z), i) for i, z in enumerate(depth) if z > 0)   # vDepthIdx after sort
    create, pts = [], []
    n_points = 0
    for z, i in v:
        b_create = has_point is None or not has_point[i]
        create.append(1 if b_create else 0)
        pts.append(unproject(F, keys["x"][i], keys["y"][i], depth[i]))
        n_points += 1                      # both branches
        if z > th and n_points > min_points:
            break
    n_tr = n_ntr = 0
    for i, z in enumerate(depth):          # Tracking.cc:1080-1089
        if z > 0 and float(z) < th:
            if tracked is not None and tracked[i]:
                n_tr += 1
            else:
                n_ntr += 1
    order = np.array([i for _, i in v], np.int32)
    counts = np.array([len(v), len(create), n_tr, n_ntr], np.int32)
    return (order, counts, np.array(create, np.uint8),
            np.array(pts, f32).reshape(-1, 3))


def visited_closed_form(M, L, min_points=100):
    """V = min(M, max(min_points, L) + 1): the break fires at the first sorted position
    j >= L (z > th) with j + 1 > min_points."""
    return min(M, max(min_points, L) + 1)


def same_floats(a, b):
    """Bit patterns equal, except that any NaN matches any NaN (inf * 0 and inf - inf arise from a
    +inf depth; the sign and payload of a generated NaN are not the reference's to define)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan))


# ---- depth cases ------------------------------------------------------------------------------

U16_SPECIALS = [0, 1, 65535, 5000, 12345]
F32_SPECIALS = [f32(0.0), f32(-0.0), f32(-1.5), f32(np.nan), f32(np.inf), f32(1e-41),
                np.nextafter(f32(0), f32(1)), f32(2.5), f32(0.75)]
# coordinate styles: (name, in the image?)
OOB = [("x==width", lambda c, r: (f32(W), f32(r))), ("y==height", lambda c, r: (f32(c), f32(H))),
       ("x<0", lambda c, r: (f32(-1.0), f32(r))), ("y<0", lambda c, r: (f32(c), f32(-3.5))),
       ("nan", lambda c, r: (f32(np.nan), f32(r))), ("3e9", lambda c, r: (f32(c), f32(3e9))),
       ("-3e9", lambda c, r: (f32(-3e9), f32(r)))]


def depth_case(seed: int, depth_type: int, factor_name: str, n: int):
    """One frame: the allocation `alloc` ((H+1) x ROW_ELEMS, all valid depth), its H x W view
    `img`, `kps`, a perturbed `kps_un`, and per keypoint the planted `pixel` (row, col; -1 = out
    of the image), `raw` value and outcome class `cls` in {"oob", "invalid", "valid"}."""
    rng = np.random.default_rng(seed * 1000 + n)
    factor = FACTORS[factor_name]
    if depth_type == DEPTH_U16:
        alloc = np.full((ALLOC_ROWS, ROW_ELEMS), 7777, np.uint16)
        specials = U16_SPECIALS
        rand = lambda: int(rng.integers(0, 65536))
    else:
        alloc = np.full((ALLOC_ROWS, ROW_ELEMS), 3.5, f32)
        specials = F32_SPECIALS
        rand = lambda: f32(rng.uniform(-1.0, 8.0))
    img = alloc[:H, :W]
    pix = 1 + rng.permutation(W * H - 1)[:n]        # distinct pixels; pixel (0, 0) is reserved
    kps = np.zeros(n, KEYPOINT_DTYPE)
    kps["octave"] = rng.integers(0, 8, n)
    pixel = np.zeros((n, 2), np.int64)
    raws, cls, style = [], [], []
    for i in range(n):
        r, c = divmod(int(pix[i]), W)
        raw = specials[i % len(specials)] if i < 3 * len(specials) else rand()
        k = i % 11
        if i == 0:                                   # (int)-0.5 == 0: the pixel (0, 0)
            r, c, x, y, st = 0, 0, f32(-0.5), f32(-0.25), "trunc-to-zero"
        elif k < 4:
            x, y, st = f32(c), f32(r), "integral"
        elif k < 8:                                  # a float below the next integer
            x, y = np.nextafter(f32(c + 1), f32(0)), np.nextafter(f32(r + 1), f32(0))
            st = "below-next"
        elif k < 10:
            x, y, st = f32(c + rng.uniform(0.05, 0.95)), f32(r + rng.uniform(0.05, 0.95)), "frac"
        else:
            name, fn = OOB[(i // 11) % len(OOB)]
            x, y = fn(c, r)
            st = name
        kps["x"][i], kps["y"][i] = x, y
        inside = st in ("trunc-to-zero", "integral", "below-next", "frac")
        if inside:
            img[r, c] = raw
            pixel[i] = (r, c)
            d = depth_rule(raw, depth_type, factor)
            cls.append("valid" if d > 0 else "invalid")
        else:
            pixel[i] = (-1, -1)
            cls.append("oob")
        raws.append(raw)
        style.append(st)
    kps_un = kps.copy()
    kps_un["x"] = (kps["x"] + f32(0.37)).astype(f32)
    kps_un["y"] = (kps["y"] - f32(0.21)).astype(f32)
    return dict(alloc=alloc, img=img, depth_type=depth_type, factor=factor, factor_name=factor_name,
                mbf=f32(40.0), kps=kps, kps_un=kps_un, pixel=pixel, raw=raws, cls=cls,
                style=style, row_stride=ROW_ELEMS * alloc.itemsize)


DEPTH_SIZES = [0, 1, 63, 64, 65, 256, 257]
DEPTH_COMBOS = [(DEPTH_U16, "tum"), (DEPTH_U16, "one"), (DEPTH_U16, "one+5e-6"),
                (DEPTH_U16, "one+2e-5"), (DEPTH_F32, "one"), (DEPTH_F32, "one+5e-6"),
                (DEPTH_F32, "one+2e-5"), (DEPTH_F32, "tum")]


def depth_cases():
    out = []
    for t, fname in DEPTH_COMBOS:
        for n in DEPTH_SIZES:
            out.append(depth_case(3 + t, t, fname, n))
    return out


# ---- poses ------------------------------------------------------------------------------------

K4 = (517.3, 516.5, 318.6, 255.3)   # TUM1


def pose(seed=None):
    """An orbx_frame_pose record: identity (seed None) or a random rotation and translation."""
    if seed is None:
        R, t = np.eye(3), np.zeros(3)
    else:
        rng = np.random.default_rng(seed)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        R, t = q * np.sign(np.linalg.det(q)), rng.uniform(-2, 2, 3)
    return frame_pose(R, t, K4, (0.0, 640.0, 0.0, 480.0), 1.2 ** np.arange(8), mbf=40.0)


# ---- close-point cases --------------------------------------------------------------------------

TH = f32(3.0)


def _close_case(name, seed, below, at, above, invalid, masks=True, th=TH, extra=()):
    """`below` values 0 < z < th, `at` values == th, `above` values > th (arrays or counts),
    `invalid` slots without depth, shuffled over the indices.  Plants M and L."""
    rng = np.random.default_rng(seed)

    def vals(spec, lo, hi):
        if not isinstance(spec, (int, np.integer)):
            return np.asarray(spec, f32)
        # u16-like depths (k / 5000): ties are common
        return (rng.integers(int(lo * 5000), int(hi * 5000), int(spec)).astype(f32) * TUM_FACTOR
                ).astype(f32)

    b = vals(below, 0.2, float(th) - 0.01) if np.isfinite(th) else vals(below, 0.2, 6.0)
    a = np.full(at, th, f32)
    ab = vals(above, float(th) + 0.01, 9.0) if np.isfinite(th) else np.zeros(0, f32)
    inv = np.resize(np.array([-1.0, 0.0, -0.0, np.nan, -2.5], f32), invalid)
    depth = np.concatenate([b, a, ab, np.asarray(extra, f32), inv]).astype(f32)
    depth = depth[rng.permutation(len(depth))]
    n = len(depth)
    keys = np.zeros(n, KEYPOINT_DTYPE)
    keys["x"] = rng.uniform(0, 640, n)
    keys["y"] = rng.uniform(0, 480, n)
    has_point = (rng.random(n) < 0.4).astype(np.uint8) if masks else None
    tracked = ((rng.random(n) < 0.7) & (has_point > 0)).astype(np.uint8) if masks else None
    pos = depth > 0
    return dict(name=name, n=n, keys=keys, depth=depth, th=f32(th), has_point=has_point,
                tracked=tracked, F=pose(seed), M=int(pos.sum()),
                L=int((pos & ~(depth > f32(th))).sum()),
                n_close=int((pos & (depth < f32(th))).sum()))


def close_cases():
    c = []
    for m in (0, 1, 99, 100, 101, 102):                       # M alone
        c.append(_close_case(f"M={m}", 10 + m, m // 3, 0, m - m // 3, 7))
    c.append(_close_case("L<100<M", 20, 50, 0, 100, 11))
    c.append(_close_case("L=100", 21, 100, 0, 50, 11))
    c.append(_close_case("L=101", 22, 101, 0, 49, 11))
    c.append(_close_case("L=M>100", 23, 130, 0, 0, 11))
    c.append(_close_case("all-far", 24, 0, 0, 150, 11))
    # z == th_depth: not close for the counts, does not trigger the break
    c.append(_close_case("at-threshold", 25, 98, 5, 30, 9))
    c.append(_close_case("at-threshold-only", 26, 0, 120, 20, 3))
    # a run of equal z across sorted position 100 (above the threshold) and across the threshold
    c.append(_close_case("tie-across-100", 27, 20, 0, np.concatenate(
        [np.linspace(3.1, 3.9, 75), np.full(12, 4.25), np.linspace(5, 6, 20)]), 5))
    c.append(_close_case("tie-across-th", 28, np.concatenate(
        [np.linspace(0.5, 2.5, 90), np.full(8, np.nextafter(TH, f32(0)))]), 6,
        np.concatenate([np.full(7, np.nextafter(TH, f32(9))), np.linspace(4, 5, 30)]), 5))
    # +inf and denormal depths are valid
    c.append(_close_case("inf-denormal", 29, 60, 0, 60, 5,
                         extra=[np.inf, 1e-41, np.nextafter(f32(0), f32(1)), np.inf]))
    c.append(_close_case("no-masks", 30, 70, 2, 60, 9, masks=False))
    # th_depth = +inf: V = M (StereoInitialization reads every z > 0 through `order`)
    c.append(_close_case("th=inf", 31, 140, 0, 0, 9, th=f32(np.inf), extra=[np.inf, 1e-41]))
    return c


CLOSE_SIZES = [1, 64, 65, 1023, 1024, 1025, 2024, 8192]


def close_size_case(n, seed=40):
    """n slots, about 7 in 8 with depth, u16-like values (ties), a third of them close."""
    m = n - n // 8
    below = m // 3
    at = min(2, m - below)
    return _close_case(f"n={n}", seed + n, below, at, m - below - at, n - m)


def random_close_frame(seed):
    """A random frame for the closed form of V: sizes and the threshold anywhere."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 400))
    depth = (rng.integers(0, 200, n).astype(f32) * f32(0.05)).astype(f32)   # zeros and ties
    depth[rng.random(n) < 0.1] = -1.0
    th = f32(rng.choice([0.0, 1.0, 2.5, 5.0, 9.95, 20.0, np.inf]))
    return depth, th, int(rng.choice([100, 0, 1, 37, 1000]))
