"""The per-frame geometry kernels of csrc/orbx_frame.hip that run before any matcher -- k_undistort /
k_undistort_batch (Frame::UndistortKeyPoints), k_grid (Frame::AssignFeaturesToGrid / PosInGrid),
k_gray (cvtColor(*2GRAY)) and k_frustum (Frame::isInFrustum + MapPoint::PredictScale) -- restated
plainly in numpy / Python, and directed cases for every regime of each (numpy only; shared by
tests/test_frame_cases.py on the CPU and tests/test_gpu_frame_directed.py on the GPU).

Nothing here calls the code under test for an expected value: the package supplies record dtypes,
``frame_pose`` (which fills a record) and ``image_bounds`` (inputs of the camera grid cases only).

``variant=`` switches one decision of a restatement to a plausible wrong form; the CPU tests
require every variant to change at least one directed case, so each decision is pinned by a case.

Records that may hold NaN are compared after ``canon_*``: every NaN of a *float* field becomes the
one quiet NaN 0x7fc00000.  x86 and the GPU differ in the sign of the default NaN (0 * inf is
0xffc00000 on x86 and 0x7fc00000 on the GPU); integer fields are never touched.
"""
import ctypes
import math

import numpy as np

from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import MAP_POINT_DTYPE, PROJ_QUERY_DTYPE, frame_pose

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
_libm.ceilf.restype = ctypes.c_float
_libm.ceilf.argtypes = [ctypes.c_float]
_libm.floorf.restype = ctypes.c_float
_libm.floorf.argtypes = [ctypes.c_float]
f32 = np.float32
INT_MIN = -2 ** 31
NEG0 = f32(-0.0)
WIDTH, HEIGHT = 752, 480

CAMS = {"euroc": synth.EUROC_CAM, "tum1": synth.TUM1_CAM,
        "rational": ((500.0, 501.0, 320.5, 240.25), (0.1, -0.05, 0.001, -0.002, 0.01, 0.02, -0.01, 0.005))}


def up(a):
    return np.nextafter(f32(a), f32(np.inf))


def dn(a):
    return np.nextafter(f32(a), f32(-np.inf))


def _ord(x) -> int:
    """The position of a float32 in the order of all float32 (monotone in x)."""
    i = int(f32(x).view(np.int32))
    return i if i >= 0 else -(i & 0x7fffffff)


def _unord(o: int):
    return np.int32(o).view(f32) if o >= 0 else np.uint32(0x80000000 | -o).view(f32)


def first_at_least(fn, target, lo, hi):
    """The smallest float32 x in [lo, hi] with fn(x) >= target, fn non-decreasing (bisection over
    the float32 order); hi when there is none."""
    a, b = _ord(lo), _ord(hi)
    while a < b:
        m = (a + b) // 2
        if fn(_unord(m)) >= target:
            b = m
        else:
            a = m + 1
    return _unord(a)


def trunc_x86(v) -> int:
    """(int) of a float as x86 cvttss2si: INT_MIN when NaN or out of range."""
    v = float(v)
    return int(v) if v == v and -2.0 ** 31 <= v < 2.0 ** 31 else INT_MIN


# ---- NaN canonisation (float fields only) -----------------------------------------------------------

def _canon_words(words, float_cols):
    for c in float_cols:
        col = words[:, c]
        col[(col & 0x7fffffff) > 0x7f800000] = 0x7fc00000
    return words


def canon_queries(q):
    """orbx_proj_query records as uint32 [n, 8], NaN canonised in u, v, ur, radius and angle; the
    three level fields are integers and stay as they are."""
    w = np.ascontiguousarray(q).view(np.uint8).reshape(-1, 32).copy().view(np.uint32)
    return _canon_words(w, (0, 1, 2, 3, 7))


def canon_keys(k):
    """orbx_keypoint records as uint32 [n, 7], NaN canonised in x, y, size, angle and response;
    octave and class_id are integers and stay as they are."""
    w = np.ascontiguousarray(k).view(np.uint8).reshape(-1, 28).copy().view(np.uint32)
    return _canon_words(w, (0, 1, 2, 3, 4))


def kp(x, y):
    """Keypoint records at (x, y), the other fields distinct per slot."""
    x = np.asarray(x, f32).reshape(-1)
    y = np.broadcast_to(np.asarray(y, f32).reshape(-1), x.shape) if np.size(y) == 1 else np.asarray(y, f32).reshape(-1)
    assert len(x) == len(y)
    n = len(x)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"], k["y"] = x, y
    k["size"] = 31.0
    k["angle"] = (np.arange(n) * 7) % 360
    k["response"] = np.arange(n) + 0.5
    k["octave"] = np.arange(n) % 8
    k["class_id"] = -1 - np.arange(n)
    return k


# ---- the grid: Frame::AssignFeaturesToGrid + PosInGrid ------------------------------------------------

GRID_VARIANTS = ("rint", "trunc", "px_le_cols", "row_major", "no_sort", "nan_zero", "min_y_for_x")


def _to_cell_pos(v, variant=None) -> int:
    """(int)std::round(v) of a float product: half away from zero, then the x86 conversion."""
    v = float(v)
    if v != v:
        return 0 if variant == "nan_zero" else INT_MIN
    if math.isinf(v):
        return INT_MIN
    if variant == "rint":
        r = round(v)                                   # half to even
    elif variant == "trunc":
        r = int(v)
    else:
        r = math.copysign(math.floor(abs(v) + 0.5), v)
    return int(r) if -2.0 ** 31 <= r < 2.0 ** 31 else INT_MIN


def axis_product(x, mn, inv):
    """(x - mnMin) * inv, each step rounded to float32."""
    with np.errstate(all="ignore"):
        return f32(f32(f32(x) - f32(mn)) * f32(inv))


def grid_np(keys, cols, rows, min_x, min_y, inv_w, inv_h, variant=None):
    """-> (off int32 [cols*rows + 1], feat int32, info).  info: the float products 'vx', 'vy', the
    converted positions 'px', 'py' and the cell (-1 = outside) of every keypoint."""
    n = len(keys)
    min_x, min_y, inv_w, inv_h = f32(min_x), f32(min_y), f32(inv_w), f32(inv_h)
    xs, ys = np.asarray(keys["x"], f32), np.asarray(keys["y"], f32)
    info = dict(vx=np.zeros(n, f32), vy=np.zeros(n, f32), px=np.zeros(n, np.int64),
                py=np.zeros(n, np.int64), cell=np.full(n, -1, np.int64))
    ncell = cols * rows
    cells = [[] for _ in range(ncell + (rows if variant == "px_le_cols" else 0))]
    for i in range(n):
        vx = axis_product(xs[i], min_y if variant == "min_y_for_x" else min_x, inv_w)
        vy = axis_product(ys[i], min_y, inv_h)
        px, py = _to_cell_pos(vx, variant), _to_cell_pos(vy, variant)
        info["vx"][i], info["vy"][i], info["px"][i], info["py"][i] = vx, vy, px, py
        x_out = px > cols if variant == "px_le_cols" else px >= cols
        if px < 0 or x_out or py < 0 or py >= rows:
            continue
        c = py * cols + px if variant == "row_major" else px * rows + py
        info["cell"][i] = c
        cells[c].append(i)
    off = np.zeros(len(cells) + 1, np.int32)
    feat = []
    for c, members in enumerate(cells):
        off[c] = len(feat)
        feat += members[::-1] if variant == "no_sort" else members
    off[len(cells)] = len(feat)
    return off[:ncell + 1].copy(), np.array(feat, np.int32), info


def grid_params(bounds, cols, rows):
    """mnMinX, mnMinY and the inverse cell sizes as Frame.cc:114-115 forms them, in float."""
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    return min_x, min_y, f32(cols) / f32(max_x - min_x), f32(rows) / f32(max_y - min_y)


def _grid_case(name, keys, bounds, cols=64, rows=48):
    min_x, min_y, inv_w, inv_h = grid_params(bounds, cols, rows)
    return dict(name=name, keys=np.ascontiguousarray(keys, KEYPOINT_DTYPE), cols=cols, rows=rows,
                bounds=tuple(float(f32(b)) for b in bounds), min_x=min_x, min_y=min_y,
                inv_w=inv_w, inv_h=inv_h)


def boundary_pair(c, mn, inv):
    """The largest float32 coordinate the restatement puts at position <= c and its successor (the
    smallest at position c + 1), found by stepping around mn + (c + 0.5) / inv."""
    pos = lambda x: _to_cell_pos(axis_product(x, mn, inv))
    x = f32(float(mn) + (c + 0.5) / float(inv))
    while pos(x) > c:
        x = dn(x)
    while pos(up(x)) <= c:
        x = up(x)
    return x, up(x)


def _boundary_keys(bounds, cols, rows, col_list=None, row_list=None):
    """Keypoints on either side of every column and row boundary (the exact half included where a
    float has one: it is then the smaller neighbour of a positive boundary, the larger of -0.5)."""
    min_x, min_y, inv_w, inv_h = grid_params(bounds, cols, rows)
    xm = f32(float(min_x) + (cols // 2 + 0.25) / float(inv_w))      # inside a cell, off any boundary
    ym = f32(float(min_y) + (rows // 2 + 0.25) / float(inv_h))
    xs, ys = [], []
    for c in (range(-1, cols) if col_list is None else col_list):
        a, b = boundary_pair(c, min_x, inv_w)
        xs += [a, b]
        ys += [ym, ym]
    for r in (range(-1, rows) if row_list is None else row_list):
        a, b = boundary_pair(r, min_y, inv_h)
        xs += [xm, xm]
        ys += [a, b]
    return kp(xs, ys)


EXACT_BOUNDS = (0.0, 512.0, 0.0, 384.0)           # 64 x 48 cells of 8 x 8: both inverses are 0.125
NONFINITE = (np.nan, np.inf, -np.inf, 3e9, -3e9, 1e30, -1e30, -0.0)
GRID_SHAPES = ((1, 1), (1, 7), (7, 1), (31, 33), (32, 32), (41, 25), (64, 48), (128, 120))
GRID_COUNTS = (0, 1, 1023, 1024, 1025, 2049)
_GRID = None


def grid_cases():
    """The directed grid cases (built once; image_bounds needs the library, not a GPU)."""
    global _GRID
    if _GRID is not None:
        return _GRID
    from my_orb_slam2_amd.features import image_bounds
    cases = []
    # every column / row boundary of the exact grid: the half itself and its two neighbours
    xs, ys = [], []
    for c in range(-1, 65):
        h = f32(8 * c + 4)
        xs += [dn(h), h, up(h)]
        ys += [f32(101.0)] * 3
    for r in range(-1, 49):
        h = f32(8 * r + 4)
        xs += [f32(101.0)] * 3
        ys += [dn(h), h, up(h)]
    cases.append(_grid_case("exact_halves", kp(xs, ys), EXACT_BOUNDS))
    cam_bounds = {}
    for cam, (K4, dist) in CAMS.items():
        b = cam_bounds[cam] = image_bounds(K4, dist, WIDTH, HEIGHT)
        cases.append(_grid_case(f"boundaries_{cam}", _boundary_keys(b, 64, 48), b))
    # the four edges of the grid: on, just inside, just outside
    for name, b in (("exact", EXACT_BOUNDS), ("euroc", cam_bounds["euroc"])):
        mnx, mxx, mny, mxy = (f32(v) for v in b)
        xm, ym = f32((float(mnx) + float(mxx)) / 2 + 1.3), f32((float(mny) + float(mxy)) / 2 + 1.3)
        ex = [mnx, up(mnx), dn(mnx), mxx, dn(mxx), up(mxx)]
        ey = [mny, up(mny), dn(mny), mxy, dn(mxy), up(mxy)]
        cases.append(_grid_case(f"edges_{name}", kp(ex + [xm] * 6 + ex, [ym] * 6 + ey + ey), b))
    # non-finite and extreme coordinates in x only, in y only and in both
    for name, b in (("exact", EXACT_BOUNDS), ("euroc", cam_bounds["euroc"])):
        xs = list(NONFINITE) + [100.0] * len(NONFINITE) + [np.nan, np.inf, -np.inf, 100.0]
        ys = [100.0] * len(NONFINITE) + list(NONFINITE) + [np.nan, -np.inf, np.nan, 100.0]
        cases.append(_grid_case(f"nonfinite_{name}", kp(xs, ys), b))
    # feature counts around the stride of the kernel's per-thread loops
    be = cam_bounds["euroc"]
    for n in GRID_COUNTS:
        rng = np.random.default_rng(100 + n)
        cases.append(_grid_case(f"count_{n}", kp(rng.uniform(be[0] - 20, be[1] + 20, n),
                                                 rng.uniform(be[2] - 20, be[3] + 20, n)), be))
    # every feature in one cell, descending in space so that no fill order is the sorted one
    t = np.linspace(3.0, -3.0, 2048)
    cases.append(_grid_case("one_cell_2048", kp(80.0 + t, 160.0 + t), EXACT_BOUNDS))
    rng = np.random.default_rng(7)
    side = rng.integers(0, 4, 300)
    ox = np.where(side == 0, -50.0, np.where(side == 1, 600.0, rng.uniform(0, 512, 300)))
    oy = np.where(side == 2, -50.0, np.where(side == 3, 450.0, rng.uniform(0, 384, 300)))
    oy = np.where(side < 2, rng.uniform(0, 384, 300), oy)
    cases.append(_grid_case("all_outside", kp(ox, oy), EXACT_BOUNDS))
    cx, cy = np.meshgrid(np.arange(64) * 8.0 + 1.0, np.arange(48) * 8.0 - 1.0, indexing="ij")
    perm = np.random.default_rng(8).permutation(3072)
    cases.append(_grid_case("every_cell_once", kp(cx.reshape(-1)[perm], cy.reshape(-1)[perm]), EXACT_BOUNDS))
    # grid shapes: fewer cells than threads, 1023 / 1024 / 1025 cells, the largest accepted
    for cols, rows in GRID_SHAPES:
        rng = np.random.default_rng(cols * 1000 + rows)
        k = kp(rng.uniform(be[0] - 10, be[1] + 10, 300), rng.uniform(be[2] - 10, be[3] + 10, 300))
        edge = _boundary_keys(be, cols, rows, sorted({-1, 0, cols // 2, cols - 2, cols - 1} & set(range(-1, cols))),
                              sorted({-1, 0, rows // 2, rows - 2, rows - 1} & set(range(-1, rows))))
        cases.append(_grid_case(f"shape_{cols}x{rows}", np.concatenate([k, edge]), be, cols, rows))
    _GRID = cases
    return cases


_GRID_REF = {}


def grid_reference(case, variant=None):
    key = (case["name"], variant)
    if key not in _GRID_REF:
        _GRID_REF[key] = grid_np(case["keys"], case["cols"], case["rows"], case["min_x"], case["min_y"],
                                 case["inv_w"], case["inv_h"], variant)
    return _GRID_REF[key]


GRID_BATCH_STRIDE = 1100


def grid_batch_case():
    """Six frames of kp_stride 1100 with counts that are full, empty, above the stride, negative
    and one; every slot, the pad slots included, lies inside the grid, so a read past a frame's
    count shows in the result."""
    s = GRID_BATCH_STRIDE
    d_n = np.array([1024, 0, s + 5, -3, 1, s], np.int32)
    rng = np.random.default_rng(55)
    keys = kp(rng.uniform(1, 507, len(d_n) * s), rng.uniform(1, 379, len(d_n) * s))
    c = _grid_case("batch", keys, EXACT_BOUNDS)
    c.update(d_n=d_n, stride=s, counts=np.clip(d_n, 0, s))
    return c


def grid_batch_reference(case):
    s = case["stride"]
    return [grid_np(case["keys"][f * s:f * s + int(n)], case["cols"], case["rows"], case["min_x"],
                    case["min_y"], case["inv_w"], case["inv_h"])[:2] for f, n in enumerate(case["counts"])]


# ---- undistortion: Frame::UndistortKeyPoints --------------------------------------------------------

UNDIST_VARIANTS = ("iters4", "copy_all_zero", "f32")


def undistort_np(xy, K4, dist, iters=5, real=np.float64):
    """cvUndistortPoints (OpenCV 3.2) in numpy, same operation order; float64 as the reference."""
    k = np.zeros(8, real)
    d = np.asarray(dist, np.float32).astype(real)
    k[:len(d)] = d
    fx, fy, cx, cy = (real(np.float32(v)) for v in K4)
    one = real(1.0)
    ifx, ify = one / fx, one / fy
    with np.errstate(all="ignore"):
        x = (xy[:, 0].astype(real) - cx) * ifx
        y = (xy[:, 1].astype(real) - cy) * ify
        x0, y0 = x.copy(), y.copy()
        for _ in range(iters):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
            dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
            x = (x0 - dx) * icdist
            y = (y0 - dy) * icdist
        xx = fx * x + 0 * y + cx
        yy = 0 * x + fy * y + cy
        ww = 1 / (0 * x + 0 * y + one)
        return np.stack([(xx * ww).astype(np.float32), (yy * ww).astype(np.float32)], 1)


def undistort_ref(keys, K4, dist, variant=None):
    """mvKeysUn from mvKeys (Frame.cc:429-459): a copy when dist[0] == 0, else x / y replaced."""
    d = np.asarray(dist, np.float32)
    copy = bool((d == 0).all()) if variant == "copy_all_zero" else bool(d[0] == 0)
    out = np.array(keys, KEYPOINT_DTYPE)
    if copy or len(out) == 0:
        return out
    xy = undistort_np(np.stack([keys["x"], keys["y"]], 1).astype(np.float32), K4, dist,
                      4 if variant == "iters4" else 5, np.float32 if variant == "f32" else np.float64)
    out["x"], out["y"] = xy[:, 0], xy[:, 1]
    return out


# The denominator 1 + ((k3*r2 + k2)*r2 + k1)*r2 of CAMS["rational"] has no root at r2 >= 0 (its
# derivative in r2 is positive throughout), so the near-zero denominator is reached with a second
# 8-coefficient camera whose denominator is 1 - 0.5*r2: the pole lies at r2 = 2.
UNDIST_CAMS = dict(CAMS)
UNDIST_CAMS["copy"] = (synth.EUROC_CAM[0], (0.0, 0.1, 0.01, 0.01))
UNDIST_CAMS["rational_pole"] = (CAMS["rational"][0], (-0.5, 0.0, 0.001, -0.002, 0.0, 0.02, -0.01, 0.005))
UNDIST_COUNTS = (0, 1, 255, 256, 257)
CORNERS = ((0.0, 0.0), (float(WIDTH), 0.0), (0.0, float(HEIGHT)), (float(WIDTH), float(HEIGHT)))


def pole_point(K4, dist):
    """The float32 x on the row y = cy at which the float64 denominator of the first iteration is
    closest to zero (searched around the root of the reference's own polynomial)."""
    fx, _, cx, cy = (float(np.float32(v)) for v in K4)
    k = np.zeros(8)
    k[:len(dist)] = np.asarray(dist, np.float32).astype(np.float64)
    ifx = 1.0 / fx

    def den(x):
        r2 = ((float(x) - cx) * ifx) ** 2
        return 1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2
    x = f32(cx + fx * math.sqrt(2.0))
    cand = [x]
    a = b = x
    for _ in range(64):
        a, b = dn(a), up(b)
        cand += [a, b]
    best = min(cand, key=lambda v: abs(den(v)))
    return best, f32(cy), den(best)


def undistort_keys(cam, n):
    """n keypoints: the image corners first, the principal point, points 10^4 pixels outside on
    both axes, the pole of the rational_pole camera, then uniformly random ones."""
    K4, dist = UNDIST_CAMS[cam]
    pts = list(CORNERS) + [(f32(K4[2]), f32(K4[3])), (WIDTH + 1e4, HEIGHT + 1e4), (-1e4, -1e4),
                           (WIDTH + 1e4, 100.0), (100.0, -1e4)]
    if cam == "rational_pole":
        px, py, _ = pole_point(K4, dist)
        pts += [(px, py), (up(px), py), (dn(px), py)]
    rng = np.random.default_rng(len(cam) + 31)
    while len(pts) < n:
        pts.append((rng.uniform(0, WIDTH), rng.uniform(0, HEIGHT)))
    pts = np.array(pts[:n], np.float32).reshape(-1, 2)
    return kp(pts[:, 0], pts[:, 1])


def undistort_cases():
    return [dict(name=f"{cam}_n{n}", cam=cam, K4=UNDIST_CAMS[cam][0], dist=UNDIST_CAMS[cam][1],
                 keys=undistort_keys(cam, n)) for cam in UNDIST_CAMS for n in UNDIST_COUNTS]


UNDIST_BATCH_STRIDE = 300


def undistort_batch_case(cam):
    """Six frames of kp_stride 300, counts full, empty, above the stride, negative and one; every
    slot holds a keypoint, so a slot past the count that is written shows."""
    s = UNDIST_BATCH_STRIDE
    d_n = np.array([257, 0, s + 5, -3, 1, s], np.int32)
    K4, dist = UNDIST_CAMS[cam]
    keys = np.concatenate([undistort_keys(cam, s) for _ in d_n])
    rng = np.random.default_rng(77)
    keys["x"][9:] += rng.uniform(-3, 3, len(keys) - 9).astype(f32)
    return dict(name=f"batch_{cam}", cam=cam, K4=K4, dist=dist, keys=keys, d_n=d_n, stride=s,
                counts=np.clip(d_n, 0, s))


def bounds_from_corners(un):
    """Frame::ComputeImageBounds from the four undistorted corners (0,0) (w,0) (0,h) (w,h)."""
    return (min(un["x"][0], un["x"][2]), max(un["x"][1], un["x"][3]),
            min(un["y"][0], un["y"][1]), max(un["y"][2], un["y"][3]))


# ---- colour conversion: cvtColor(*2GRAY) ---------------------------------------------------------------

GRAY_VARIANTS = ("swap", "no_round", "alpha_as_colour")
GRAY_WIDTHS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 1028)
GRAY_HEIGHTS = (1, 3)


def gray_np(img, rgb, variant=None):
    """RGB2Gray<uchar> of OpenCV 3.2 in integers: (c0*s0 + 9617*s1 + c2*s2 + 8192) >> 14 with
    c0 / c2 = 1868 / 4899 for BGR order and 4899 / 1868 for RGB order."""
    s = np.asarray(img, np.uint8).astype(np.int64)
    c0, c2 = (4899, 1868) if rgb else (1868, 4899)
    if variant == "swap":
        c0, c2 = c2, c0
    last = 3 if variant == "alpha_as_colour" and s.shape[2] == 4 else 2
    rnd = 0 if variant == "no_round" else 8192
    return ((c0 * s[..., 0] + 9617 * s[..., 1] + c2 * s[..., last] + rnd) >> 14).astype(np.uint8)


_EXH = None


def exhaustive_image():
    """4096 x 4096 x 3: every (s0, s1, s2) triple once."""
    global _EXH
    if _EXH is None:
        a = np.arange(1 << 24, dtype="<u4")
        _EXH = np.ascontiguousarray(a.view(np.uint8).reshape(-1, 4)[:, :3]).reshape(4096, 4096, 3)
    return _EXH


def gray_cases():
    out = []
    for w in GRAY_WIDTHS:
        for h in GRAY_HEIGHTS:
            for c in (3, 4):
                for rgb in (0, 1):
                    rng = np.random.default_rng(w * 100 + h * 10 + c + rgb)
                    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
                    img[0, 0, :3] = 255                       # the largest sum
                    img[-1, -1, :3] = 0
                    out.append(dict(name=f"w{w}_h{h}_c{c}_{'rgb' if rgb else 'bgr'}", img=img, rgb=rgb))
    return out


def with_other_alpha(img):
    out = img.copy()
    out[..., 3] = ~out[..., 3]
    return out


# ---- the frustum: Frame::isInFrustum + MapPoint::PredictScale ------------------------------------------

FRUSTUM_OUTCOMES = ("skipped", "depth", "u_low", "u_high", "v_low", "v_high", "dist_low",
                    "dist_high", "viewcos", "visible")
FRUSTUM_VARIANTS = ("u_low_le", "u_high_ge", "v_low_le", "v_high_ge", "dist_low_le", "dist_high_ge",
                    "viewcos_le", "z_le", "f998", "floor", "th_never", "th_eps", "no_clamp_above",
                    "ur_plus")
# "th multiplied unconditionally" cannot change a bit: th is applied whenever (double)th != 1.0,
# and r * 1.0f == r for every float r (2.5f and 4.0f here), so the unconditional product equals the
# conditional one for every th.  What the condition can get wrong is pinned instead: th_never (the
# product dropped) and th_eps (th treated as 1 when it is within 1e-6 of it; nextafter(1.0) pins it).


def frustum_np(F, mps, skip, cos_lim=0.5, th=1.0, variant=None):
    """Statement by statement in numpy float32 / Python double.  -> (queries, nToMatch, info);
    info: per-point 'outcome' (FRUSTUM_OUTCOMES), 'clamp' ('below' / 'above' / 'inside' / ''), and
    the reference's own intermediates 'z', 'u', 'v', 'dist', 'vc', 'quot' (the quotient before
    ceil), 'r0' (the radius before th and the scale) and 'th_applied'."""
    n = len(mps)
    q = np.zeros(n, PROJ_QUERY_DTYPE)
    q["radius"] = -1.0
    q["min_level"] = q["max_level"] = q["pred_level"] = -1
    nan = lambda: np.full(n, np.nan, f32)
    info = dict(outcome=["skipped"] * n, clamp=[""] * n, z=nan(), u=nan(), v=nan(), dist=nan(),
                vc=nan(), quot=nan(), r0=nan(), th_applied=np.zeros(n, bool))
    R, t, Ow = F["Rcw"].reshape(3, 3), F["tcw"], F["Ow"]
    lt = lambda a, b, name: a <= b if variant == name else a < b
    gt = lambda a, b, name: a >= b if variant == name else a > b
    n_vis = 0
    with np.errstate(all="ignore"):
        for i, m in enumerate(mps):
            if skip is not None and skip[i]:
                continue
            P = m["pos"]
            Pc = []
            for r in range(3):
                s = f32(f32(R[r, 0] * P[0]) + f32(R[r, 1] * P[1]))
                s = f32(s + f32(R[r, 2] * P[2]))
                Pc.append(f32(float(s) + float(t[r])))
            info["z"][i] = Pc[2]
            if lt(Pc[2], f32(0), "z_le"):
                info["outcome"][i] = "depth"
                continue
            invz = f32(f32(1.0) / Pc[2])
            u = f32(f32(f32(F["fx"] * Pc[0]) * invz) + F["cx"])
            v = f32(f32(f32(F["fy"] * Pc[1]) * invz) + F["cy"])
            info["u"][i], info["v"][i] = u, v
            if lt(u, F["min_x"], "u_low_le"):
                info["outcome"][i] = "u_low"
                continue
            if gt(u, F["max_x"], "u_high_ge"):
                info["outcome"][i] = "u_high"
                continue
            if lt(v, F["min_y"], "v_low_le"):
                info["outcome"][i] = "v_low"
                continue
            if gt(v, F["max_y"], "v_high_ge"):
                info["outcome"][i] = "v_high"
                continue
            maxd, mind = f32(f32(1.2) * m["max_dist"]), f32(f32(0.8) * m["min_dist"])
            PO = [f32(P[k] - Ow[k]) for k in range(3)]
            ss = 0.0
            for k in range(3):
                ss += float(PO[k]) * float(PO[k])
            dist = f32(math.sqrt(ss)) if ss == ss and ss >= 0 else f32(np.nan)
            info["dist"][i] = dist
            if lt(dist, mind, "dist_low_le"):
                info["outcome"][i] = "dist_low"
                continue
            if gt(dist, maxd, "dist_high_ge"):
                info["outcome"][i] = "dist_high"
                continue
            dot = 0.0
            for k in range(3):
                dot += float(PO[k]) * float(m["normal"][k])
            vc = f32(np.float64(dot) / np.float64(dist))
            info["vc"][i] = vc
            if lt(vc, f32(cos_lim), "viewcos_le"):
                info["outcome"][i] = "viewcos"
                continue
            ratio = f32(m["max_dist"] / dist)
            quot = f32(f32(_libm.logf(ratio)) / F["log_scale_factor"])
            info["quot"][i] = quot
            lvl = trunc_x86(_libm.floorf(quot) if variant == "floor" else _libm.ceilf(quot))
            nl = int(F["nlevels"])
            if lvl < 0:
                lvl, info["clamp"][i] = 0, "below"
            elif lvl >= nl:
                info["clamp"][i] = "above"
                if variant != "no_clamp_above":
                    lvl = nl - 1
            else:
                info["clamp"][i] = "inside"
            if variant == "f998":
                r = f32(2.5) if vc > f32(0.998) else f32(4.0)
            else:
                r = f32(2.5) if float(vc) > 0.998 else f32(4.0)
            info["r0"][i] = r
            apply = float(f32(th)) != 1.0
            if variant == "th_never":
                apply = False
            elif variant == "th_eps":
                apply = abs(float(f32(th)) - 1.0) > 1e-6
            if apply:
                r = f32(r * f32(th))
            info["th_applied"][i] = apply
            scale = F["scale"][lvl] if lvl < 16 else f32(0)
            bf = f32(F["mbf"] * invz)
            ur = f32(u + bf) if variant == "ur_plus" else f32(u - bf)
            q[i] = (u, v, ur, f32(r * scale), lvl - 1, lvl, lvl, 0)
            info["outcome"][i] = "visible"
            n_vis += 1
    return q, n_vis, info


def numpy_is_in_frustum(F, mps, skip, cos_lim=0.5, th=1.0):
    q, n, _ = frustum_np(F, mps, skip, cos_lim, th)
    return q, n


def exact_frame(nlevels=8, scale_factor=1.2, c=192.0):
    """Identity rotation, tcw = (0, 0, -0.0), Ow = 0, fx = fy = 256, cx = cy = c, bounds
    [64, 320] x [32, 288]: u = 256 * x / z + c is exact where z is a power of two, and a
    negative-zero depth survives the additions."""
    F = frame_pose(np.eye(3), (0, 0, NEG0), (256, 256, c, c), (64, 320, 32, 288),
                   synth.scale_tables(nlevels, scale_factor)[0], mbf=32.0, scale_factor=scale_factor)
    F["Ow"] = 0
    return F


def shifted_frame(nlevels=8, c=192.0):
    """Identity rotation and a small translation, tcw = (0.25, 0.125, 0.5), Ow = -tcw."""
    return frame_pose(np.eye(3), (0.25, 0.125, 0.5), (256, 256, c, c), (64, 320, 32, 288),
                      synth.scale_tables(nlevels, 1.2)[0], mbf=32.0)


def mp(P, Ow=(0, 0, 0), min_dist=0.0, max_dist=None, normal=None, lvl=2, sf=1.2):
    """One MapPoint record; by default in range with PredictScale = lvl and the normal along the
    viewing ray from Ow."""
    r = np.zeros((), MAP_POINT_DTYPE)
    r["pos"] = np.asarray(P, f32)
    PO = np.nan_to_num(np.asarray(r["pos"], np.float64) - np.asarray(Ow, np.float64), nan=0.0,
                       posinf=1.0, neginf=-1.0)
    d = float(np.linalg.norm(PO))
    d = d if np.isfinite(d) and d > 0 else 1.0
    r["min_dist"] = f32(min_dist)
    r["max_dist"] = f32(d * sf ** (lvl - 0.5)) if max_dist is None else f32(max_dist)
    r["normal"] = np.asarray(PO / d if normal is None else normal, f32)
    return r


def _stack(points):
    return np.array(points, MAP_POINT_DTYPE)


def _at_pixel(u, v, z=1.0, c=192.0, **kw):
    """The point that projects exactly to (u, v) through exact_frame(c=c), z a power of two."""
    z = f32(z)
    return mp((f32(f32(f32(u) - f32(c)) / f32(256)) * z, f32(f32(f32(v) - f32(c)) / f32(256)) * z, z), **kw)


def _fcase(name, F, mps, skip=None, cos_lim=0.5, th=1.0):
    mps = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
    if skip is not None:
        skip = np.ascontiguousarray(skip, np.uint8)
        assert len(skip) == len(mps)
    return dict(name=name, F=F, mps=mps, skip=skip, cos_lim=float(cos_lim), th=float(f32(th)))


def _one(F, point, key, cos_lim=0.5):
    return frustum_np(F, _stack([point]), None, cos_lim)[2][key][0]


def _search(F, make, key, target, lo, hi):
    """The input x in [lo, hi] at which the restatement's own intermediate `key` of make(x) equals
    `target` exactly (the intermediate is non-decreasing in x).  Asserts that there is one."""
    x = first_at_least(lambda a: _one(F, make(a), key), f32(target), lo, hi)
    assert _one(F, make(x), key) == f32(target), (key, float(target))
    return x


def level_boundary(L, lsf, lo=0.85, hi=1e6):
    """The largest float32 ratio whose quotient logf(ratio) / lsf is <= L (searched on the CPU)."""
    quot = lambda r: f32(f32(_libm.logf(f32(r))) / f32(lsf))
    return dn(first_at_least(lambda r: quot(r) > f32(L), True, lo, hi))


LO998 = dn(f32(0.998))      # float(0.998f) > 0.998, so the two floats that bracket 0.998 are
HI998 = f32(0.998)          # 0.998f and the one below it
FRUSTUM_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)
TH1UP = float(up(1.0))
_FRUSTUM = None


def _visible_points(n, Ow=(0, 0, 0), shift=(0, 0, 0)):
    return _stack([mp((0.01 * (k % 50) + shift[0], -0.01 * (k % 37) + shift[1], 2.0 + (k % 5) + shift[2]),
                      Ow=Ow, lvl=k % 8) for k in range(n)])


def frustum_cases():
    global _FRUSTUM
    if _FRUSTUM is not None:
        return _FRUSTUM
    cases = []
    FX, FX0, FT = exact_frame(), exact_frame(c=0.0), shifted_frame(c=0.0)   # c = 0: u = 256 * x / z
    OwT = FT["Ow"]
    tiny = f32(1.4e-45)                                   # the smallest subnormal
    # depth: -0.0 needs x < 0 and y < 0 (every term of the gemm row a negative zero)
    pts = [mp((-0.5, -0.5, NEG0)), mp((0.0, 0.0, 0.0)), mp((0.5, 0.5, 0.0)), mp((0.0, 0.0, tiny)),
           mp((-0.5, -0.5, tiny)), mp((0.0, 0.0, -tiny)), mp((-0.5, -0.5, -tiny)),
           mp((-0.5, -0.5, -1.0), lvl=3), mp((0.5, 0.5, np.nan)), mp((0.25, 0.25, 1.0))]
    cases.append(_fcase("depth", FX, _stack(pts)))
    # u, v on each of the four bounds and one float either side (exact construction)
    pts = [_at_pixel(u, 100.0, c=0.0) for u in (dn(64), 64, up(64), dn(320), 320, up(320))]
    pts += [_at_pixel(100.0, v, c=0.0) for v in (dn(32), 32, up(32), dn(288), 288, up(288))]
    pts += [_at_pixel(dn(64), dn(32), c=0.0), _at_pixel(up(320), up(288), c=0.0), _at_pixel(128, 128, 2.0, c=0.0)]
    cases.append(_fcase("bounds", FX0, _stack(pts)))
    # the same through the translated frame, each input found by searching the restatement
    pts = []
    for b in (64, 320):
        mk = lambda a: mp((a, 0.375, 0.5), Ow=OwT)
        x = _search(FT, mk, "u", b, -2.0, 2.0)
        pts += [mk(x)]
        pts += [mk(_search(FT, mk, "u", dn(b), -2.0, 2.0)), mk(_search(FT, mk, "u", up(b), -2.0, 2.0))]
    for b in (32, 288):
        mk = lambda a: mp((0.25, a, 0.5), Ow=OwT)
        pts += [mk(_search(FT, mk, "v", t, -2.0, 2.0)) for t in (b, dn(b), up(b))]
    cases.append(_fcase("bounds_shifted", FT, _stack(pts)))
    # dist on 0.8f*min and 1.2f*max and one float either side (on the optical axis dist = z)
    pts = []
    for mn in (5.0, 0.3, 7.7):
        lo = f32(f32(0.8) * f32(mn))
        pts += [mp((0, 0, d), min_dist=mn, max_dist=100.0) for d in (lo, dn(lo), up(lo))]
    for mx in (5.0, 0.3, 7.7):
        hi = f32(f32(1.2) * f32(mx))
        pts += [mp((0, 0, d), max_dist=mx) for d in (hi, up(hi), dn(hi))]
    pts += [mp((0, 0, 0), max_dist=0.0), mp((0, 0, 4.0), max_dist=0.0), mp((0, 0, 4.0), max_dist=np.inf),
            mp((0, 0, 4.0), min_dist=np.nan, max_dist=np.nan), mp((0, 0, 4.0), min_dist=9.0, max_dist=1.0),
            mp((0, 0, 0), max_dist=1.0), mp((0, 0, 0), min_dist=1.0, max_dist=1.0)]
    cases.append(_fcase("dist", FX, _stack(pts)))
    pts = []
    for mn, mx in ((5.0, None), (None, 3.0)):
        tgt = f32(f32(0.8) * f32(mn)) if mn else f32(f32(1.2) * f32(mx))
        mk = lambda a: mp((OwT[0] + 1, OwT[1] + 1, a), Ow=OwT, min_dist=mn or 0.0, max_dist=mx or 100.0,
                          normal=(0, 0, 1))
        pts += [mk(_search(FT, mk, "dist", t, 2.6, 3.4)) for t in (tgt, dn(tgt), up(tgt))]
    cases.append(_fcase("dist_shifted", FT, _stack(pts)))
    # viewCos on cos_lim and either side of it, and on the two floats that bracket 0.998
    for cl in (0.5, 0.25, 0.7):
        c = f32(cl)
        pts = [mp((0, 0, 4.0), normal=(0, 0, n), max_dist=8.0) for n in (c, dn(c), up(c), LO998, HI998, up(HI998), 1.0, -1.0)]
        pts += [mp((0, 0, 4.0), normal=(np.nan, 0, 1.0), max_dist=8.0)]
        cases.append(_fcase(f"viewcos_{cl}", FX, _stack(pts), cos_lim=cl))
    # PredictScale: quotients on an integer and one float either side, for levels 0 .. nlevels
    for nl in (1, 8, 16):
        F = exact_frame(nl)
        pts = []
        for L in range(nl + 1):
            r = level_boundary(L, F["log_scale_factor"])
            pts += [mp((0, 0, 8.0), max_dist=f32(x * f32(8.0))) for x in (dn(r), r, up(r))]
        pts += [mp((0, 0, 8.0), max_dist=8.0 * 1.2 ** 40), mp((0, 0, 8.0), max_dist=3e38),
                mp((0, 0, 8.0), max_dist=np.inf), mp((0, 0, 8.0), max_dist=np.nan)]
        pts += [mp((0, 0, 8.0), lvl=l) for l in range(nl)]
        cases.append(_fcase(f"level_nl{nl}", F, _stack(pts)))
        # below 0 needs a scale factor under 1.2: a ratio under 1 / 1.2 is out of range first
        F = exact_frame(nl, 1.05)
        pts = [mp((0, 0, 8.0), max_dist=8.0 * 0.9), mp((0, 0, 8.0), max_dist=8.0 * 0.84),
               mp((0, 0, 8.0), max_dist=8.0), mp((0, 0, 8.0), max_dist=f32(1.05) * f32(8.0)),
               mp((0, 0, 8.0), max_dist=8.0 * 1.05 ** 40)]
        cases.append(_fcase(f"level_clamp_nl{nl}", F, _stack(pts)))
    # th: 1 is not applied, 3 and the float above 1 are; both radii in each
    for th in (1.0, 3.0, TH1UP):
        pts = [mp((0.01 * k, -0.02 * k, 2.0 + k), lvl=k % 8) for k in range(8)]
        pts += [mp((0, 0, 4.0), normal=(0, 0, 0.9), max_dist=8.0)]
        cases.append(_fcase(f"th_{th!r}", FX, _stack(pts), th=th))
    # skip flags: none, all clear, all set, alternating
    pts = _visible_points(41)
    for name, sk in (("none", None), ("zeros", np.zeros(41)), ("ones", np.ones(41)), ("alt", np.arange(41) % 2)):
        cases.append(_fcase(f"skip_{name}", FX, pts, skip=sk))
    # counts: every point visible; only the last one visible (the ballot of a partial last wave,
    # waves without a visible point)
    for n in FRUSTUM_COUNTS:
        cases.append(_fcase(f"count_all_{n}", FX, _visible_points(n)))
        pts = _visible_points(n)
        pts["pos"][:n - 1, 2] = -1.0
        cases.append(_fcase(f"count_last_{n}", FX, pts))
    _FRUSTUM = cases
    return cases


_FRUSTUM_REF = {}


def frustum_reference(case, variant=None):
    key = (case["name"], variant)
    if key not in _FRUSTUM_REF:
        _FRUSTUM_REF[key] = frustum_np(case["F"], case["mps"], case["skip"], case["cos_lim"],
                                       case["th"], variant)
    return _FRUSTUM_REF[key]


def frustum_batch_case():
    """Five frames with 257, 0, 1, 0 and 64 MapPoints, each frame with its own pose and levels."""
    FT = shifted_frame()
    frames = [exact_frame(), FT, exact_frame(16), FT, exact_frame(1)]
    sizes = [257, 0, 1, 0, 64]
    mps = []
    for F, n in zip(frames, sizes):
        shifted = F is FT
        m = _visible_points(n, Ow=F["Ow"], shift=F["Ow"] if shifted else (0, 0, 0))
        m["pos"][1::5, 2] = -1.0            # some behind the camera
        mps.append(m)
    skip = [(np.arange(n) % 7 == 3).astype(np.uint8) for n in sizes]
    return dict(name="batch", frames=frames, mps=mps, skip=skip)
