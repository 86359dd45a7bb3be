"""cv::remap(8UC1, CV_32FC1 maps, INTER_LINEAR, BORDER_CONSTANT 0) and cv::initUndistortRectifyMap
restated in numpy / Python from OpenCV 3.2 (modules/imgproc/src/imgwarp.cpp, undistort.cpp), and
directed cases for them (numpy only; shared by tests/test_remap_cases.py on the CPU and
tests/test_gpu_remap.py / tests/test_remap_facade.py on the GPU).  PARITY UNPINNED against the
library: the restatements pin the GPU kernel and the host helpers to each other.

* ``remap_literal``: the per-pixel scalar fixed-point conversion, the short weight table built as
  initInterTab2D builds it (saturation of 32768 and the fix-up included), the inlier run and the
  border path, (sum + (1 << 14)) >> 15.
* ``remap_closed``: (sum of the taps times their 5-bit weight products + 512) >> 10, vectorised.
* ``init_map_np``: the double loop of initUndistortRectifyMap, vectorised over rows.

A case is a dict: src [B, sh, sw] uint8, map1 / map2 [dh, dw] float32, and a memory layout
(padded source rows, destination row stride / base offset / image stride).  ``layout`` builds the
two allocations: the source inside decoy bytes (a broken bounds guard reads owned memory and shows
as a wrong answer, not a fault), the destination pre-filled with a sentinel.
"""
import functools

import numpy as np

f32 = np.float32
INT_MIN = -2 ** 31
SENTINEL = 0xA5
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
HEIGHTS = (1, 2, 5)
SPECIALS = (np.nan, np.inf, -np.inf, 1e9, -1e9, 3e9, 2.0 ** 26, 40000.0)


# ---- the fixed-point conversion ------------------------------------------------------------------
def cv_round(v) -> int:
    """cvRound(float) on x86 (cvtss2si): half to even; NaN / outside int: INT_MIN."""
    v = f32(v)
    if not (v >= f32(-2.0 ** 31) and v < f32(2.0 ** 31)):
        return INT_MIN
    return int(np.rint(v))


def sat_short(v: int) -> int:
    return max(-32768, min(32767, v))


def fixed_point_scalar(mx, my):
    """(X, Y, a, b) of one map entry."""
    with np.errstate(all="ignore"):
        sx, sy = cv_round(f32(mx) * f32(32.0)), cv_round(f32(my) * f32(32.0))
    return sat_short(sx >> 5), sat_short(sy >> 5), sx & 31, sy & 31


def fixed_point_np(map1, map2):
    """Vectorised: X, Y, a, b int64 arrays."""
    def conv(m):
        with np.errstate(all="ignore"):
            p = np.asarray(m, f32) * f32(32.0)
            ok = (p >= f32(-2.0 ** 31)) & (p < f32(2.0 ** 31))
            s = np.where(ok, np.rint(np.where(ok, p, f32(0))), float(INT_MIN)).astype(np.int64)
        return np.clip(s >> 5, -32768, 32767), s & 31
    X, a = conv(map1)
    Y, b = conv(map2)
    return X, Y, a, b


def fixed_point_cv(map1, map2):
    """The CV_16SC2 + CV_16UC1 pair orbx_remap_fixed_point writes."""
    X, Y, a, b = fixed_point_np(map1, map2)
    return np.stack([X, Y], -1).astype(np.int16), (b * 32 + a).astype(np.uint16)


# ---- initInterTab2D(INTER_LINEAR, fixpt) ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weight_table() -> np.ndarray:
    """[1024, 4] short weights (entry b * 32 + a; taps v00 v01 v10 v11), built in table order into
    one flat zero-initialised array as the library's static table is: the fix-up's window
    (k1, k2 in {ksize/2, ksize/2 + 1}, ksize = 2) reaches past the 2x2 entry into the entries not
    yet written."""
    n, ks = 32, 2
    tab1 = np.zeros((n, ks), f32)
    scale = f32(1.0) / f32(n)
    for i in range(n):                       # interpolateLinear(i * scale)
        x = f32(i) * scale
        tab1[i] = (f32(1.0) - x, x)
    flat = np.zeros(n * n * ks * ks + 8, np.int64)
    for i in range(n):
        for j in range(n):
            base = (i * n + j) * ks * ks
            isum = 0
            for k1 in range(ks):
                vy = tab1[i, k1]
                for k2 in range(ks):
                    v = f32(vy * tab1[j, k2])
                    w = sat_short(cv_round(f32(v * f32(32768.0))))
                    flat[base + k1 * ks + k2] = w
                    isum += w
            if isum != 32768:
                diff = isum - 32768
                h = ks // 2
                Mk1 = Mk2 = mk1 = mk2 = h
                for k1 in range(h, h + 2):
                    for k2 in range(h, h + 2):
                        if flat[base + k1 * ks + k2] < flat[base + mk1 * ks + mk2]:
                            mk1, mk2 = k1, k2
                        elif flat[base + k1 * ks + k2] > flat[base + Mk1 * ks + Mk2]:
                            Mk1, Mk2 = k1, k2
                if diff < 0:
                    flat[base + Mk1 * ks + Mk2] -= diff
                else:
                    flat[base + mk1 * ks + mk2] -= diff
    return flat[:n * n * ks * ks].reshape(n * n, ks * ks).copy()


# ---- the two restatements of remap ---------------------------------------------------------------
def remap_literal(src, map1, map2, stats=None):
    """src [B, sh, sw] uint8 -> [B, dh, dw] uint8, pixel by pixel (vectorised over the batch
    only).  stats (a dict) counts the pixels of each code path."""
    src = np.asarray(src, np.uint8)
    B, sh, sw = src.shape
    dh, dw = map1.shape
    S = src.astype(np.int64)
    tab = weight_table()
    out = np.zeros((B, dh, dw), np.uint8)
    stats = stats if stats is not None else {}
    for y in range(dh):
        for x in range(dw):
            X, Y, a, b = fixed_point_scalar(map1[y, x], map2[y, x])
            w = tab[b * 32 + a]
            if 0 <= X < sw - 1 and 0 <= Y < sh - 1:      # (unsigned)X < width1 && ...
                stats["inlier"] = stats.get("inlier", 0) + 1
                s = (S[:, Y, X] * w[0] + S[:, Y, X + 1] * w[1] + S[:, Y + 1, X] * w[2] +
                     S[:, Y + 1, X + 1] * w[3])
            else:
                stats["border"] = stats.get("border", 0) + 1
                if X >= sw or X + 1 < 0 or Y >= sh or Y + 1 < 0:   # BORDER_CONSTANT, all outside
                    continue
                s = np.zeros(B, np.int64)
                for k, (ty, tx) in enumerate(((Y, X), (Y, X + 1), (Y + 1, X), (Y + 1, X + 1))):
                    if 0 <= tx < sw and 0 <= ty < sh:    # borderInterpolate(...) >= 0
                        s = s + S[:, ty, tx] * w[k]
            out[:, y, x] = np.clip((s + (1 << 14)) >> 15, 0, 255)
    return out


def taps(src, X, Y):
    """The four taps [4, B, dh, dw] int64 (0 outside the source)."""
    B, sh, sw = src.shape
    S = src.astype(np.int64)
    res = []
    for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1)):
        ty, tx = Y + oy, X + ox
        ok = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
        v = S[:, np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)]
        res.append(np.where(ok[None], v, 0))
    return np.stack(res)


def closed_sum(src, map1, map2):
    X, Y, a, b = fixed_point_np(map1, map2)
    t = taps(np.asarray(src, np.uint8), X, Y)
    return ((32 - a) * (32 - b) * t[0] + a * (32 - b) * t[1] + (32 - a) * b * t[2] + a * b * t[3])


def remap_closed(src, map1, map2):
    return ((closed_sum(src, map1, map2) + 512) >> 10).astype(np.uint8)


# ---- cv::initUndistortRectifyMap -----------------------------------------------------------------
def init_map_np(K, dist, R, P, width, height):
    K = np.asarray(K, np.float64).reshape(3, 3)
    P = np.asarray(P, np.float64).reshape(3, -1)[:, :3]
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    d = np.zeros(8)
    d[:len(dist)] = np.asarray(dist, np.float64).reshape(-1)
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    M = [[P[i, 0] * R[0, j] + P[i, 1] * R[1, j] + P[i, 2] * R[2, j] for j in range(3)]
         for i in range(3)]
    det = (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) -
           M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))
    s = 1.0 / det
    iR = [[(M[1][1] * M[2][2] - M[1][2] * M[2][1]) * s, (M[0][2] * M[2][1] - M[0][1] * M[2][2]) * s,
           (M[0][1] * M[1][2] - M[0][2] * M[1][1]) * s],
          [(M[1][2] * M[2][0] - M[1][0] * M[2][2]) * s, (M[0][0] * M[2][2] - M[0][2] * M[2][0]) * s,
           (M[0][2] * M[1][0] - M[0][0] * M[1][2]) * s],
          [(M[1][0] * M[2][1] - M[1][1] * M[2][0]) * s, (M[0][1] * M[2][0] - M[0][0] * M[2][1]) * s,
           (M[0][0] * M[1][1] - M[0][1] * M[1][0]) * s]]
    i = np.arange(height, dtype=np.float64)
    _x, _y, _w = i * iR[0][1] + iR[0][2], i * iR[1][1] + iR[1][2], i * iR[2][1] + iR[2][2]
    m1 = np.empty((height, width), f32)
    m2 = np.empty((height, width), f32)
    for j in range(width):
        w = 1.0 / _w
        x, y = _x * w, _y * w
        x2, y2 = x * x, y * y
        r2, _2xy = x2 + y2, 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
        m1[:, j] = (fx * xd + cx).astype(f32)
        m2[:, j] = (fy * yd + cy).astype(f32)
        _x, _y, _w = _x + iR[0][0], _y + iR[1][0], _w + iR[2][0]
    return m1, m2


# ---- directed cases ------------------------------------------------------------------------------
def _case(name, src, map1, map2, src_pad=0, dst_pad=0, dst_off=0, src_gap=0, dst_gap=0):
    src = np.ascontiguousarray(src, np.uint8)
    if src.ndim == 2:
        src = src[None]
    return dict(name=name, src=src, map1=np.ascontiguousarray(map1, f32),
                map2=np.ascontiguousarray(map2, f32), src_pad=src_pad, dst_pad=dst_pad,
                dst_off=dst_off, src_gap=src_gap, dst_gap=dst_gap)


def _grid(xs, ys):
    m1, m2 = np.meshgrid(np.asarray(xs, f32), np.asarray(ys, f32))
    return m1, m2


def _rand_src(rng, b, h, w):
    return rng.integers(1, 256, (b, h, w), dtype=np.uint8)      # never 0: a 0 output is a border


def _border_coords(n):
    """Coordinates putting X at -2, -1, 0, n-2, n-1, n with and without a fraction."""
    return [-2.5, -1.5, -1.0, -0.5, -1 / 32, 0.0, 0.25, n - 1.5, n - 1.0, n - 0.75, float(n), n + 0.5]


def build_cases(chunk: int):
    """Every directed case; `chunk` is the kernel's images-per-chunk (my_orb_slam2_amd.rectify.
    images_per_chunk(): batches of 1, 2, 3 and chunk + 1 are used)."""
    rng = np.random.default_rng(20240607)
    cases = []
    # identity and integer shifts
    yy, xx = np.mgrid[0:5, 0:8].astype(f32)
    s = _rand_src(rng, 2, 5, 8)
    cases.append(_case("identity", s, xx, yy))
    cases.append(_case("shift+1-2", s, xx + 1, yy - 2))
    cases.append(_case("shift-3+1", s, xx - 3, yy + 1))
    # all 1024 (a, b) pairs on 2x2 blocks of {0, 255} patterns plus random bytes
    a, b = np.meshgrid(np.arange(32, dtype=f32) / f32(32), np.arange(32, dtype=f32) / f32(32))
    pat = np.array([[(p >> 0) & 1, (p >> 1) & 1, (p >> 2) & 1, (p >> 3) & 1] for p in range(16)],
                   np.uint8).reshape(16, 2, 2) * 255
    blocks = np.concatenate([pat, rng.integers(0, 256, (8, 2, 2), dtype=np.uint8),
                             np.array([[[255, 254], [253, 255]], [[1, 0], [0, 2]]], np.uint8)])
    cases.append(_case("ab_grid", blocks, a, b))
    # cvRound ties k + (2m+1)/64 and negative coordinates through the arithmetic shift
    ties = [1 / 64, 3 / 64, -1 / 64, -3 / 64, 2 + 1 / 64, 2 + 3 / 64, 1 + 5 / 64, -1 / 32,
            -1 - 1 / 64, 3 + 31 / 64, 3 + 33 / 64, -33 / 32]
    cases.append(_case("ties", _rand_src(rng, 2, 6, 6), *_grid(ties, ties)))
    # borders, corners, all-outside
    for (sh, sw) in ((4, 5), (1, 1), (2, 2), (1, 4), (3, 1)):
        cases.append(_case(f"border_{sw}x{sh}", _rand_src(rng, 2, sh, sw),
                           *_grid(_border_coords(sw), _border_coords(sh)), src_pad=3, dst_pad=1))
    # a source size different from the destination size
    m1 = rng.uniform(-1.5, 13.5, (11, 9)).astype(f32)
    m2 = rng.uniform(-1.5, 7.5, (11, 9)).astype(f32)
    cases.append(_case("src13x7_dst9x11", _rand_src(rng, 3, 7, 13), m1, m2, src_pad=5, dst_pad=2,
                       dst_off=1, src_gap=9, dst_gap=7))
    # NaN, +-inf, huge values: every one must give 0
    sp = np.asarray(SPECIALS, f32)
    ok = np.full(len(sp), 1.5, f32)
    m1 = np.stack([sp, ok, sp])
    m2 = np.stack([ok, sp, sp[::-1]])
    cases.append(_case("specials", _rand_src(rng, 2, 4, 4), m1, m2, dst_pad=3, dst_off=3))
    # smooth maps (scales, slopes and offsets around the kernel's per-group footprint limits: 8
    # source columns x 3 rows), running off every side of the source; sources of 7, 8 and 9 columns
    k = 0
    for (sw, sh) in ((7, 6), (8, 6), (9, 5), (40, 12), (23, 1), (16, 2)):
        for (sx, slope_y, sy, slope_x) in ((1.0, 0.0, 1.0, 0.0), (1.0, 0.3, 1.0, 0.05),
                                           (1.5, 0.7, 0.9, 0.2), (2.0, 0.26, 1.1, 0.0),
                                           (2.25, 0.5, 1.0, 0.1), (0.5, 1.2, 0.5, 0.4),
                                           (7 / 3, 2 / 3, 1.0, 0.0), (8 / 3, 1.0, 1.0, 0.0)):
            dw, dh = (37, 5) if k % 2 else (44, 4)
            yy, xx = np.mgrid[0:dh, 0:dw].astype(np.float64)
            ox, oy = (-2.3, -1.6) if k % 3 else (sw - 9.5, sh - 2.5)
            m1 = (xx * sx + yy * slope_x + ox + (k % 5) / 32).astype(f32)
            m2 = (yy * sy + xx * slope_y / 4 + oy + (k % 7) / 32).astype(f32)
            cases.append(_case(f"smooth{k}_src{sw}x{sh}", _rand_src(rng, 2 + k % 2, sh, sw), m1, m2,
                               src_pad=k % 4, dst_pad=k % 3, dst_off=k % 2))
            k += 1
    # destination widths x heights, batches and layouts
    batches = (1, 2, 3, chunk + 1)
    layouts = (dict(), dict(src_pad=7), dict(dst_pad=5, dst_off=1), dict(dst_pad=2, dst_off=3),
               dict(src_pad=1, dst_pad=3, src_gap=11, dst_gap=13, dst_off=2),
               dict(dst_pad=4, dst_gap=64))
    k = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            bsz = batches[k % len(batches)]
            lay = layouts[(k // 2) % len(layouts)]
            sw, sh = min(w, 40) + 3, h + 2
            m1 = rng.uniform(-1.5, sw + 0.5, (h, w)).astype(f32)
            m2 = rng.uniform(-1.5, sh + 0.5, (h, w)).astype(f32)
            cases.append(_case(f"w{w}_h{h}_b{bsz}", _rand_src(rng, bsz, sh, sw), m1, m2, **lay))
            k += 1
    return cases


def build_stereo_cases(chunk: int):
    """(left, right) case pairs of one geometry and layout, with different maps and sources."""
    rng = np.random.default_rng(77)
    out = []
    for (w, h, bsz, lay) in ((65, 5, chunk + 1, dict(src_pad=3, dst_pad=5, dst_off=1, src_gap=5,
                                                      dst_gap=9)),
                             (4, 1, 1, dict()), (257, 2, 3, dict(dst_pad=1)),
                             (7, 3, 2 * chunk, dict(dst_off=2, dst_pad=2))):
        sw, sh = min(w, 40) + 3, h + 2
        pair = []
        for side in "LR":
            m1 = rng.uniform(-1.5, sw + 0.5, (h, w)).astype(f32)
            m2 = rng.uniform(-1.5, sh + 0.5, (h, w)).astype(f32)
            pair.append(_case(f"stereo{side}_w{w}_h{h}_b{bsz}", _rand_src(rng, bsz, sh, sw), m1, m2,
                              **lay))
        out.append(tuple(pair))
    return out


def layout(c):
    """The source and destination allocations of a case: dict(src, src_off, src_rs, src_is, dst,
    dst_off, dst_rs, dst_is), 1-D uint8 arrays and byte offsets / strides."""
    B, sh, sw = c["src"].shape
    dh, dw = c["map1"].shape
    rng = np.random.default_rng(sw * 131 + sh * 17 + dw)
    src_rs = sw + c["src_pad"]
    src_is = src_rs * sh + c["src_gap"]
    src_off = 5
    src = rng.integers(1, 256, src_off + src_is * B + src_rs + 8, dtype=np.uint8)   # decoys
    v = np.lib.stride_tricks.as_strided(src[src_off:], (B, sh, sw), (src_is, src_rs, 1))
    v[...] = c["src"]
    dst_rs = dw + c["dst_pad"]
    dst_is = dst_rs * dh + c["dst_gap"]
    dst = np.full(c["dst_off"] + dst_is * B + 16, SENTINEL, np.uint8)
    return dict(src=src, src_off=src_off, src_rs=src_rs, src_is=src_is, dst=dst,
                dst_off=c["dst_off"], dst_rs=dst_rs, dst_is=dst_is)


def expected_dst(c, lay, out=None):
    """The destination allocation after the remap: sentinels everywhere but the images."""
    out = remap_closed(c["src"], c["map1"], c["map2"]) if out is None else out
    B, dh, dw = out.shape
    e = np.full_like(lay["dst"], SENTINEL)
    v = np.lib.stride_tricks.as_strided(e[lay["dst_off"]:], (B, dh, dw),
                                        (lay["dst_is"], lay["dst_rs"], 1))
    v[...] = out
    return e


# ---- census --------------------------------------------------------------------------------------
def census(cases):
    """Which of the directed constructs occur over `cases`: {name: count}."""
    cn = {}

    def add(k, n):
        cn[k] = cn.get(k, 0) + int(n)
    for c in cases:
        B, sh, sw = c["src"].shape
        X, Y, a, b = fixed_point_np(c["map1"], c["map2"])
        inx, iny = (X >= 0) & (X < sw - 1), (Y >= 0) & (Y < sh - 1)
        add("inlier", (inx & iny).sum())
        add("border_path", (~(inx & iny)).sum())
        for nm, m in (("X=-1", X == -1), ("X=sw-1", X == sw - 1), ("Y=-1", Y == -1),
                      ("Y=sh-1", Y == sh - 1), ("X=-2", X == -2), ("X=sw", X == sw),
                      ("Y=sh", Y == sh)):
            add(nm, m.sum())
        add("corner_tl", ((X == -1) & (Y == -1)).sum())
        add("corner_tr", ((X == sw - 1) & (Y == -1)).sum())
        add("corner_bl", ((X == -1) & (Y == sh - 1)).sum())
        add("corner_br", ((X == sw - 1) & (Y == sh - 1)).sum())
        outside = (X >= sw) | (X + 1 < 0) | (Y >= sh) | (Y + 1 < 0)
        add("all_outside", outside.sum())
        add("partial", (~outside & ~(inx & iny)).sum())
        add("neg_shift_a31", ((X == -1) & (a == 31) & (c["map1"] == f32(-1 / 32))).sum())
        for t, sx in ((1 / 64, 0), (3 / 64, 2), (-1 / 64, 0), (-3 / 64, -2)):
            hit = c["map1"] == f32(t)
            add(f"tie{t:+.6f}", (hit & (X * 32 + a == sx)).sum())
        for m in (c["map1"], c["map2"]):
            add("nan", np.isnan(m).sum())
            add("+inf", (m == np.inf).sum())
            add("-inf", (m == -np.inf).sum())
            for v in (1e9, -1e9, 3e9, 2.0 ** 26, 40000.0):
                add(f"{v:g}", (m == f32(v)).sum())
        s = closed_sum(c["src"], c["map1"], c["map2"])
        for r in (0, 1023, 512, 511):
            add(f"sum%1024=={r}", ((s % 1024 == r) & (s > 0)).sum())
        add(f"batch{B if B <= 3 else 'chunk+'}", 1)
        dh, dw = c["map1"].shape
        add(f"w{dw}", 1)
        add(f"h{dh}", 1)
        add("src!=dst", (sh, sw) != (dh, dw))
        add("src_pad", c["src_pad"] > 0)
        add("dst_stride%4", (dw + c["dst_pad"]) % 4 != 0 and c["dst_pad"] > 0)
        add("dst_odd_base", c["dst_off"] % 2 == 1)
        add("image_gap", c["src_gap"] > 0 and c["dst_gap"] > 0 and B > 1)
        add("src1x1", (sh, sw) == (1, 1))
        add("src2x2", (sh, sw) == (2, 2))
    return cn


def group_forms(c):
    """The kernel's choice per group of 4 destination pixels, restated: {name: count} of groups
    that fit the 8-column x 3-row window (and how tightly) and of groups that do not."""
    B, sh, sw = c["src"].shape
    X, Y, _, _ = fixed_point_np(c["map1"], c["map2"])
    dh, dw = X.shape
    cl = lambda v, n: np.clip(v, 0, n - 1)                      # noqa: E731
    pad = (-dw) % 4
    def grp(a):
        return np.concatenate([a, np.repeat(a[:, -1:], pad, 1)], 1).reshape(dh, -1, 4)
    x0, x1, y0, y1 = grp(cl(X, sw)), grp(cl(X + 1, sw)), grp(cl(Y, sh)), grp(cl(Y + 1, sh))
    xmin, xmax, ymin, ymax = x0.min(2), x1.max(2), y0.min(2), y1.max(2)
    xl = np.minimum(xmin, max(sw - 8, 0))
    xs, ys = xmax - xl, ymax - ymin
    win = (sw >= 8) & (xs <= 7) & (ys <= 2)
    return {"window": int(win.sum()), "gather": int((~win).sum()),
            "window_xspan7": int((win & (xs == 7)).sum()),
            "window_yspan2": int((win & (ys == 2)).sum()),
            "window_clamped_start": int((win & (xl < xmin)).sum()),
            "window_last_row": int((win & (ymin + 2 > sh - 1)).sum()),
            "gather_xspan8": int(((sw >= 8) & (xs == 8) & (ys <= 2)).sum()),
            "gather_yspan3": int(((sw >= 8) & (xs <= 7) & (ys == 3)).sum()),
            "gather_narrow_source": int(((sw < 8) & (xs <= 7) & (ys <= 2)).sum()),
            "window_partial_group": int(win[:, -1].sum()) if pad else 0}


# ---- EuRoC ---------------------------------------------------------------------------------------
EUROC_W, EUROC_H = 752, 480


@functools.lru_cache(maxsize=None)
def euroc_maps(settings_path):
    """((map1, map2) left, (map1, map2) right, settings) of the reference's EuRoC stereo settings,
    by init_map_np."""
    from my_orb_slam2_amd.rectify import load_stereo_settings
    s = load_stereo_settings(settings_path)
    res = []
    for side in ("left", "right"):
        c = s[side]
        res.append(init_map_np(c["K"], c["D"], c["R"], c["P"], c["width"], c["height"]))
    return res[0], res[1], s
