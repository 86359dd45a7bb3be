"""Directed image-content cases for the extractor kernels (k_fast, k_octree, k_orient_desc).

numpy only, deterministic.  Three parts:

1. ``StampImage``: images made of stamps on a flat background whose level-0 FAST output is
   known in closed form.
   * dot: one pixel of value bg + a (bg - a on a bright background).  All 16 pixels of its
     Bresenham circle are background, so it is a FAST corner at threshold t iff a > t, with
     response a - 1.  A background pixel sees at most two stamp pixels on its circle and is
     never a corner.
   * pair: two adjacent pixels (horizontal, vertical or diagonal) of amplitudes a, a'.  A
     circle of radius 3 does not contain the 8-neighbourhood, so both are corners (a - 1,
     a' - 1) and the 3x3 non-maximum suppression decides between them.
   * ballast: a pixel of amplitude <= minThFAST is never a corner and makes none (every
     difference that involves only background and ballast is <= minThFAST).  On bg = 0 the
     ballast inside a keypoint's patch is all of m10 and m01.
   Pixels of different dots / pairs stay >= 4 apart (Chebyshev), so no stamp lies on another's
   circle (radius 3) or in its 3x3 neighbourhood; ballast keeps the same distance from them.
   The constructor of every case asserts these invariants.
2. Restatements with a ``variant=`` switch that flips exactly one decision: the cell grid /
   two-pass / NMS logic of ComputeKeyPointsOctTree (src/ORBextractor.cc:785-842) over the
   stamps (``predict_fast``), DistributeOctTree on Python lists (``octree_reference``, which
   also reports the events it took), and the IC_Angle moments (``moments``).
3. ``cases()``: the table of named cases, each with the constructs it plants.

Coordinates: stamps are placed in image coordinates; FAST candidates and octree keys are in
the reference's border-relative frame (image - 16).
"""
import math

import numpy as np

MIN_BORDER = 16          # EDGE_THRESHOLD - 3
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
PAIR_DIRS = {"h": (1, 0), "v": (0, 1), "d": (1, 1), "a": (-1, 1)}


# ------------------------------------------------------------------------------------------
# the FAST cell grid (src/ORBextractor.cc:785-818)
# ------------------------------------------------------------------------------------------
def cell_grid(w, h):
    """Cells of a w x h level: dict(ncols, nrows, wcell, hcell, cells=[(i, j, c0, r0, c1, r1)])
    with the ROI [c0, c1) x [r0, r1) in image coordinates.  cv::FAST detects (and suppresses)
    on the ROI less a 3-pixel frame."""
    maxbx, maxby = w - MIN_BORDER, h - MIN_BORDER
    width, height = float(maxbx - MIN_BORDER), float(maxby - MIN_BORDER)
    ncols, nrows = int(width / 30.0), int(height / 30.0)
    out = dict(ncols=ncols, nrows=nrows, wcell=0, hcell=0, cells=[])
    if ncols < 1 or nrows < 1:
        return out
    wcell, hcell = int(math.ceil(width / ncols)), int(math.ceil(height / nrows))
    out.update(wcell=wcell, hcell=hcell)
    for i in range(nrows):
        r0 = MIN_BORDER + i * hcell
        if r0 >= maxby - 3:
            continue
        r1 = min(r0 + hcell + 6, maxby)
        for j in range(ncols):
            c0 = MIN_BORDER + j * wcell
            if c0 >= maxbx - 6:
                continue
            c1 = min(c0 + wcell + 6, maxbx)
            out["cells"].append((i, j, c0, r0, c1, r1))
    return out


# ------------------------------------------------------------------------------------------
# stamp images
# ------------------------------------------------------------------------------------------
class StampImage:
    def __init__(self, w, h, bg=0, t_ini=20, t_min=7):
        assert 0 <= bg <= 255
        self.w, self.h, self.bg, self.t_ini, self.t_min = w, h, bg, t_ini, t_min
        self.pol = 1 if bg <= 127 else -1
        self.img = np.full((h, w), bg, np.uint8)
        self.corners = {}      # (x, y) -> amplitude, pixels of dots and pairs
        self.ballast_px = {}   # (x, y) -> amplitude
        self._owner = {}       # (x, y) -> stamp id
        self._next = 0

    def _put(self, x, y, a, sid):
        assert 0 <= x < self.w and 0 <= y < self.h, f"stamp pixel ({x}, {y}) outside the image"
        v = self.bg + self.pol * a
        assert 0 < a and 0 <= v <= 255, (a, v)
        assert (x, y) not in self._owner, f"two stamps on pixel ({x}, {y})"
        self.img[y, x] = v
        self._owner[(x, y)] = sid

    def dot(self, x, y, a):
        self._next += 1
        self._put(x, y, a, self._next)
        self.corners[(x, y)] = a
        return self

    def pair(self, x, y, a, a2, d="h"):
        """Pixels (x, y) of amplitude a and (x, y) + PAIR_DIRS[d] of amplitude a2."""
        dx, dy = PAIR_DIRS[d]
        self._next += 1
        self._put(x, y, a, self._next)
        self._put(x + dx, y + dy, a2, self._next)
        self.corners[(x, y)] = a
        self.corners[(x + dx, y + dy)] = a2
        return self

    def ballast(self, x, y, b):
        assert b <= self.t_min, f"ballast {b} above minThFAST {self.t_min}"
        self._put(x, y, b, 0)
        self.ballast_px[(x, y)] = b
        return self

    def check(self):
        """The invariants the closed-form prediction rests on."""
        for (x, y), sid in self._owner.items():
            if sid == 0:
                continue
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    o = self._owner.get((x + dx, y + dy))
                    assert o is None or o == sid, \
                        f"stamps closer than 4 pixels at ({x}, {y}) / ({x + dx}, {y + dy})"
        assert all(b <= self.t_min for b in self.ballast_px.values())
        return self


# ------------------------------------------------------------------------------------------
# level-0 FAST output of a stamp image (src/ORBextractor.cc:785-842, cv::FAST with NMS)
# ------------------------------------------------------------------------------------------
FAST_VARIANTS = ("nms_gt", "nms_global", "no_second_pass", "second_pass_always",
                 "fallback_before_nms", "raster_order", "region_short", "corner_ge")


def predict_fast(corners, w, h, t_ini, t_min, variant=None):
    """(candidates, cells): candidates [(x, y, response, cell, pass)] in the order
    ComputeKeyPointsOctTree collects them (cell-major, raster inside a cell; x, y relative to
    the border), cells [dict(corners=(n at iniTh, n at minTh or None), emitted_pass, n)].

    A cell is detected at iniThFAST; only if nothing survives NMS there, again at minThFAST.
    cv::FAST keeps a corner iff its score is above all 8 neighbours' (scores of pixels that
    are no corner at this threshold, or outside the ROI's detection frame, are 0): ties remove
    both, and a score of 0 never survives.

    variant flips one decision: nms_gt (a neighbour suppresses only when strictly larger),
    nms_global (NMS sees across cell borders), no_second_pass, second_pass_always (every cell
    reports its minThFAST result), fallback_before_nms (second pass only for cells without a
    corner before NMS), raster_order (candidates in raster order of the level), region_short
    (the detection frame loses its last column and row), corner_ge (corner iff a >= t)."""
    assert variant is None or variant in FAST_VARIANTS, variant
    grid = cell_grid(w, h)
    per_cell = [[] for _ in grid["cells"]]
    short = 1 if variant == "region_short" else 0
    for (x, y), a in corners.items():
        for n, (_, _, c0, r0, c1, r1) in enumerate(grid["cells"]):
            if c0 + 3 <= x <= c1 - 4 - short and r0 + 3 <= y <= r1 - 4 - short:
                per_cell[n].append((y, x, a))
                break

    def is_corner(a, t):
        return a >= t if variant == "corner_ge" else a > t

    def detect(pts, t):
        score = {(x, y): a - 1 for y, x, a in pts if is_corner(a, t)}
        look = score
        if variant == "nms_global":
            look = {p: a - 1 for p, a in corners.items() if is_corner(a, t)}
        kept = []
        for y, x, a in sorted(pts):
            if (x, y) not in score:
                continue
            s = score[(x, y)]
            nb = [look.get((x + i, y + j), 0) for j in (-1, 0, 1) for i in (-1, 0, 1) if i or j]
            ok = all(s >= q for q in nb) and s > 0 if variant == "nms_gt" else \
                all(s > q for q in nb)
            if ok:
                kept.append((x - MIN_BORDER, y - MIN_BORDER, float(s)))
        return kept, len(score)

    cands, cells = [], []
    for n, pts in enumerate(per_cell):
        kept, n_ini = detect(pts, t_ini)
        n_min, p = None, 0
        fallback = not kept if variant != "fallback_before_nms" else n_ini == 0
        if variant == "second_pass_always":
            fallback = True
        if fallback and variant != "no_second_pass":
            kept, n_min = detect(pts, t_min)
            p = 1
        cells.append(dict(corners=(n_ini, n_min), emitted_pass=p, n=len(kept)))
        cands += [(x, y, s, n, p) for x, y, s in kept]
    if variant == "raster_order":
        cands.sort(key=lambda c: (c[1], c[0]))
    return cands, cells


# ------------------------------------------------------------------------------------------
# DistributeOctTree (src/ORBextractor.cc:539-765) on Python lists
# ------------------------------------------------------------------------------------------
OCTREE_VARIANTS = ("x_le_sx", "y_le_sy", "floor_split", "last_max", "tie_seq_reversed",
                   "switch_ge", "end_gt", "no_phase2", "no_prev_stop", "root_round")
OCTREE_EVENTS = ("rounds1", "rounds2", "switch_round", "seq_ties", "seq_ties_at_cut", "big_nodes",
                 "big_equal", "big_distinct", "cuts", "end", "roots", "roots_dropped",
                 "on_split_x", "on_split_y", "odd_splits", "even_splits", "best_ties",
                 "single_key_nodes", "max_list", "max_expandable", "one_quadrant_rounds", "phase1",
                 "switch_margin", "on_split_odd")


def octree_reference(cands, minX, maxX, minY, maxY, N, variant=None, events=None):
    """DistributeOctTree on Python lists; node identity = allocation sequence number (the
    documented tie-break of equal sizes in phase 2).  cands: (x, y, response, ...) tuples,
    returned as they came.  `events`, if a dict, receives what the run went through
    (OCTREE_EVENTS).  `variant` flips one decision:
      x_le_sx / y_le_sy   a key on the split line goes to the left / upper child
      floor_split         the split line is floor (not ceil) of half the size
      last_max            the last (not the first) maximal response of a node is kept
      tie_seq_reversed    equal sizes in phase 2 are ordered by falling sequence number
      switch_ge           phase 2 starts at S + 3 nToExpand >= N (not > N)
      end_gt              the loop ends at S > N (not >= N)
      no_phase2           phase 1 runs to the end
      no_prev_stop        (guarded) the loop ignores S == prevS, ending only when nothing is
                          expandable
      root_round          the root of a candidate is round(x / hX), not its truncation"""
    assert variant is None or variant in OCTREE_VARIANTS, variant
    ev = events if events is not None else {}
    ev.update(rounds1=0, rounds2=0, switch_round=None, seq_ties=0, seq_ties_at_cut=0,
              big_nodes=0, big_equal=0, big_distinct=0, cuts=[], end=None, roots=0,
              roots_dropped=0, on_split_x=0, on_split_y=0, odd_splits=0, even_splits=0,
              best_ties=0, single_key_nodes=0, max_list=0, max_expandable=0,
              one_quadrant_rounds=0, phase1=[], switch_margin=None, on_split_odd=0)
    if not cands:
        return []
    seq = [0]
    nIni = int(np.round(np.float32(maxX - minX) / np.float32(maxY - minY)))
    if nIni < 1:
        return []
    hX = np.float32(maxX - minX) / np.float32(nIni)

    def node(x0, y0, x1, y1, keys):
        seq[0] += 1
        return {"r": (x0, y0, x1, y1), "k": keys, "more": len(keys) != 1, "seq": seq[0]}

    roots = [node(int(hX * np.float32(i)), 0, int(hX * np.float32(i + 1)), maxY - minY, [])
             for i in range(nIni)]
    for c in cands:
        q = np.float32(c[0]) / hX
        r = int(np.round(q)) if variant == "root_round" else int(q)
        roots[min(r, nIni - 1)]["k"].append(c)
    for r in roots:
        r["more"] = len(r["k"]) != 1
    lst = [r for r in roots if r["k"]]
    ev["roots"], ev["roots_dropped"] = nIni, nIni - len(lst)

    def divide(n):
        x0, y0, x1, y1 = n["r"]
        half = math.floor if variant == "floor_split" else math.ceil
        hx = int(half(np.float32(x1 - x0) / np.float32(2)))
        hy = int(half(np.float32(y1 - y0) / np.float32(2)))
        sx, sy = x0 + hx, y0 + hy
        for d in (x1 - x0, y1 - y0):
            ev["odd_splits" if d & 1 else "even_splits"] += 1
        rects = [(x0, y0, sx, sy), (sx, y0, x1, sy), (x0, sy, sx, y1), (sx, sy, x1, y1)]
        parts = [[], [], [], []]
        for c in n["k"]:
            ev["on_split_x"] += c[0] == sx
            ev["on_split_y"] += c[1] == sy
            ev["on_split_odd"] += (c[0] == sx and (x1 - x0) & 1) + (c[1] == sy and (y1 - y0) & 1)
            left = c[0] <= sx if variant == "x_le_sx" else c[0] < sx
            up = c[1] <= sy if variant == "y_le_sy" else c[1] < sy
            parts[(0 if up else 2) if left else (1 if up else 3)].append(c)
        if sum(1 for p in parts if p) == 1:
            ev["one_quadrant_rounds"] += 1
        return [(rects[q], parts[q]) for q in range(4)]

    def done(size, prev):
        if variant == "end_gt":
            return size > N or size == prev
        if variant == "no_prev_stop":
            return size >= N
        return size >= N or size == prev

    finish = False
    rounds = 0
    while not finish:
        rounds += 1
        ev["rounds1"] += 1
        prev = len(lst)
        new_front, rest, vsize = [], [], []
        for n in lst:
            if not n["more"]:
                rest.append(n)
                continue
            for rect, keys in divide(n):
                if keys:
                    ch = node(*rect, keys)
                    new_front.insert(0, ch)
                    if len(keys) > 1:
                        vsize.append(ch)
        lst = new_front + rest
        ev["max_list"] = max(ev["max_list"], len(lst))
        ev["max_expandable"] = max(ev["max_expandable"], len(vsize))
        ev["phase1"].append((len(lst), len(vsize)))
        if done(len(lst), prev) or (variant == "no_prev_stop" and not vsize):
            finish = True
            ev["end"] = ("S==N" if len(lst) == N else "S>N") if len(lst) >= N else "S==prevS"
        elif variant != "no_phase2" and (len(lst) + 3 * len(vsize) >= N if variant == "switch_ge"
                                         else len(lst) + 3 * len(vsize) > N):
            ev["switch_round"] = rounds
            ev["switch_margin"] = len(lst) + 3 * len(vsize) - N
            while not finish:
                ev["rounds2"] += 1
                prev = len(lst)
                sign = -1 if variant == "tie_seq_reversed" else 1
                order = sorted(vsize, key=lambda n: (len(n["k"]), sign * n["seq"]))
                big = [len(n["k"]) for n in order if len(n["k"]) >= 63]
                ev["big_nodes"] += len(big)
                ev["big_equal"] += len(big) - len(set(big))
                ev["big_distinct"] += max(len(set(big)) - 1, 0)
                ev["max_expandable"] = max(ev["max_expandable"], len(order))
                vsize = []
                processed = 0
                for n in reversed(order):
                    kids = []
                    for rect, keys in divide(n):
                        if keys:
                            ch = node(*rect, keys)
                            kids.insert(0, ch)
                            if len(keys) > 1:
                                vsize.append(ch)
                    lst = kids + [m for m in lst if m is not n]
                    processed += 1
                    if len(lst) >= N:
                        break
                sizes = [len(n["k"]) for n in reversed(order)]
                for i in range(1, len(sizes)):
                    if sizes[i] == sizes[i - 1]:
                        if i < processed:
                            ev["seq_ties"] += 1
                        elif i == processed:
                            ev["seq_ties_at_cut"] += 1
                ev["cuts"].append((processed, len(order)))
                ev["max_list"] = max(ev["max_list"], len(lst))
                if done(len(lst), prev) or (variant == "no_prev_stop" and not vsize):
                    finish = True
                    ev["end"] = ("S==N" if len(lst) == N else "S>N") if len(lst) >= N \
                        else "S==prevS"
    out = []
    for n in lst:
        best = n["k"][0]
        ev["single_key_nodes"] += len(n["k"]) == 1
        top = max(c[2] for c in n["k"])
        ev["best_ties"] += sum(1 for c in n["k"] if c[2] == top) > 1
        for c in n["k"][1:]:
            if c[2] >= best[2] if variant == "last_max" else c[2] > best[2]:
                best = c
        out.append(best)
    return out


# ------------------------------------------------------------------------------------------
# IC_Angle moments (src/ORBextractor.cc:77-104) in integers
# ------------------------------------------------------------------------------------------
def moments(img, x, y, umax=UMAX):
    """(m10, m01) of the circular patch around image pixel (x, y)."""
    I = img.astype(np.int64)
    m10 = m01 = 0
    for v in range(-15, 16):
        d = umax[abs(v)]
        row = I[y + v, x - d:x + d + 1]
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


# ------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------
class Case:
    """name; img; params = (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST); st: the
    StampImage (None for a textured image); constructs: names of what the case plants;
    expect: [(construct, kind, data)] checked against the closed-form prediction
    (tests/test_extract_cases.py).  The oracle's keypoint count of each case is in FLOORS."""

    def __init__(self, name, st, params, constructs, expect=(), img=None):
        self.name, self.st, self.params = name, st, tuple(params)
        self.img = st.img if st is not None else img
        self.constructs, self.expect = tuple(constructs), list(expect)
        if st is not None:
            st.check()
            # (cv::FAST clamps its threshold to [0, 255]; the stamps are built for the clamped)
            assert (st.t_ini, st.t_min) == tuple(min(max(t, 0), 255) for t in params[3:5])
        h, w = self.img.shape
        assert 96 <= w <= 320 and 80 <= h <= 240, (w, h)

    @property
    def single_level(self):
        return self.params[2] == 1 and self.st is not None

    def prediction(self, variant=None):
        h, w = self.img.shape
        return predict_fast(self.st.corners, w, h, self.st.t_ini, self.st.t_min, variant)

    def octree(self, cands, variant=None, events=None):
        h, w = self.img.shape
        return octree_reference(cands, MIN_BORDER, w - MIN_BORDER, MIN_BORDER, h - MIN_BORDER,
                                self.params[0], variant, events)


def _rel(x, y):
    return (x - MIN_BORDER, y - MIN_BORDER)


def _threshold_case(name, bg, t_ini, t_min, passed=None):
    """164 x 96: 4 x 2 cells of 33 x 32 (ROIs of 38 rows, prefetched; dw = 33 > 32; ini_x & 3 in
    all four residues).  Cell (0, j): only sub-ini dots (t_min, t_min + 1, t_ini): falls back and
    returns those above t_min.  Cell (1, j): one dot of t_ini + 1 among the same: returns only
    that one."""
    st = StampImage(164, 96, bg, t_ini, t_min)
    g = cell_grid(164, 96)
    assert (g["ncols"], g["nrows"], g["wcell"], g["hcell"]) == (4, 2, 33, 32)
    exp = []
    hi = min(t_ini + 1, 255)
    for i, j, c0, r0, c1, r1 in g["cells"]:
        x, y = c0 + 5 + j, r0 + 6
        amps = [a for a in (t_min, t_min + 1, t_ini) if 0 < a <= 255]
        pts = [(x + 6 * k, y + 5 * k) for k in range(len(amps))]
        for (px, py), a in zip(pts, amps):
            st.dot(px, py, a)
        if i == 1 and hi > t_ini:
            st.dot(x + 3, y + 17, hi)
            if hi > 1:
                exp.append(("ini_among_sub_ini", "fast", [_rel(x + 3, y + 17) + (hi - 1, 0)]))
            else:               # a corner of score 0 never survives cv::FAST's NMS
                exp.append(("score_0_never_survives", "nofast", [_rel(x + 3, y + 17)]))
            if hi + 1 <= 255:   # (with thresholds 0 / 0 the first dot that can survive: score 1)
                st.dot(x + 12, y + 21, hi + 1)
                exp.append(("ini_among_sub_ini", "fast", [_rel(x + 12, y + 21) + (hi, 0)]))
            exp.append(("ini_among_sub_ini", "nofast", [_rel(*p) for p, a in zip(pts, amps)
                                                        if not a > t_ini]))
        elif t_ini == t_min:    # t_min + 1 is above iniThFAST too: no fallback to speak of
            exp.append(("ini_equals_min", "fast", [_rel(*p) + (a - 1, 0)
                                                   for p, a in zip(pts, amps) if a > t_ini > 0]))
            exp.append(("ini_equals_min", "nofast", [_rel(*p) for p, a in zip(pts, amps)
                                                     if not a > t_ini > 0]))
        else:
            keep = [(_rel(*p) + (a - 1, 1)) for p, a in zip(pts, amps) if a > t_min and a > 1]
            drop = [_rel(*p) for p, a in zip(pts, amps) if not (a > t_min and a > 1)]
            exp.append(("fallback_cell", "fast", keep))
            exp.append(("fallback_cell", "nofast", drop))
    exp = [e for e in exp if e[2]]
    cons = sorted({e[0] for e in exp})
    if (t_ini, t_min) == (20, 7):
        cons += ["threshold_edges", "ini_x_residues", "dw_gt_32", "rows_le_40",
                 "polarity_dark" if bg > 127 else "polarity_bright"]
    if passed:      # thresholds outside [0, 255] as passed; t_ini, t_min are their clamped values
        cons.append("thresholds_out_of_range")
    return Case(name, st, (500, 1.2, 1) + (passed or (t_ini, t_min)), cons, exp)


def _pairs_case():
    """164 x 96, thresholds 20 / 7.  Per cell one construct:
    cell 0: only tied pairs above ini (all four directions) + one sub-ini dot: NMS empties the
            cell at ini, the fallback returns the dot alone (the ties stay removed);
    cell 1: pairs (a, a + 1) and (a + 1, a) in all four directions: the larger survives;
    cell 2: a pair with one pixel above ini and the other between min and ini: the first;
    cell 3: a sub-ini tied pair and a sub-ini (a, a + 1) pair: fallback keeps one pixel."""
    st = StampImage(164, 96, 0, 20, 7)
    g = cell_grid(164, 96)
    C = g["cells"]
    exp = []
    # cell 0
    _, _, c0, r0, _, _ = C[0]
    tied = []
    for k, d in enumerate("hvda"):
        x, y = c0 + 6 + 7 * k, r0 + 5
        st.pair(x, y, 40 + k, 40 + k, d)
        dx, dy = PAIR_DIRS[d]
        tied += [_rel(x, y), _rel(x + dx, y + dy)]
    st.dot(c0 + 8, r0 + 20, 12)
    exp.append(("tied_pairs_empty_ini", "nofast", tied))
    exp.append(("tied_pairs_empty_ini", "fast", [_rel(c0 + 8, r0 + 20) + (11, 1)]))
    # cell 1
    _, _, c0, r0, _, _ = C[1]
    win, lose = [], []
    for k, d in enumerate("hvda"):
        dx, dy = PAIR_DIRS[d]
        x, y = c0 + 6 + 7 * k, r0 + 5
        st.pair(x, y, 50, 51, d)
        win.append(_rel(x + dx, y + dy) + (50, 0))
        lose.append(_rel(x, y))
        y += 12
        st.pair(x, y, 51, 50, d)
        win.append(_rel(x, y) + (50, 0))
        lose.append(_rel(x + dx, y + dy))
    exp.append(("pair_larger_wins", "fast", win))
    exp.append(("pair_larger_wins", "nofast", lose))
    # cell 2
    _, _, c0, r0, _, _ = C[2]
    st.pair(c0 + 8, r0 + 8, 30, 15, "h")
    st.pair(c0 + 20, r0 + 8, 15, 30, "v")
    exp.append(("pair_ini_and_sub_ini", "fast", [_rel(c0 + 8, r0 + 8) + (29, 0),
                                                 _rel(c0 + 20, r0 + 9) + (29, 0)]))
    exp.append(("pair_ini_and_sub_ini", "nofast", [_rel(c0 + 9, r0 + 8), _rel(c0 + 20, r0 + 8)]))
    # cell 3
    _, _, c0, r0, _, _ = C[3]
    st.pair(c0 + 8, r0 + 8, 15, 15, "d")
    st.pair(c0 + 20, r0 + 8, 15, 16, "a")
    exp.append(("sub_ini_pairs", "fast", [_rel(c0 + 19, r0 + 9) + (15, 1)]))
    exp.append(("sub_ini_pairs", "nofast", [_rel(c0 + 8, r0 + 8), _rel(c0 + 9, r0 + 9),
                                            _rel(c0 + 20, r0 + 8)]))
    cons = ["tied_pairs_empty_ini", "pair_larger_wins", "pair_ini_and_sub_ini", "sub_ini_pairs"]
    return Case("pairs", st, (500, 1.2, 1, 20, 7), cons, exp)


def _pairs_across_cells_case():
    """164 x 96: pairs straddling the cell borders in x, in y and at the cell corners (both
    diagonals), tied and unequal: NMS is cell-local, so both pixels are keypoints.  The
    detection regions of cells (i, 0) | (i, 1) meet between x = c1 - 4 and c1 - 3, those of
    (0, j) / (1, j) between y = r1 - 4 and r1 - 3."""
    st = StampImage(164, 96, 0, 20, 7)
    C = cell_grid(164, 96)["cells"]
    exp = []
    _, _, c0, r0, c1, r1 = C[0]
    xb, yb = c1 - 4, r1 - 4
    both = []
    st.pair(xb, yb + 12, 60, 60, "h")          # tied, straddles x
    both += [_rel(xb, yb + 12) + (59, 0), _rel(xb + 1, yb + 12) + (59, 0)]
    st.pair(xb, yb + 20, 60, 70, "h")          # unequal, straddles x
    both += [_rel(xb, yb + 20) + (59, 0), _rel(xb + 1, yb + 20) + (69, 0)]
    st.pair(xb + 12, yb, 60, 60, "v")          # tied, straddles y (cells (0,1) / (1,1))
    both += [_rel(xb + 12, yb) + (59, 0), _rel(xb + 12, yb + 1) + (59, 0)]
    st.pair(xb + 20, yb, 70, 60, "v")
    both += [_rel(xb + 20, yb) + (69, 0), _rel(xb + 20, yb + 1) + (59, 0)]
    st.pair(xb, yb, 60, 60, "d")               # the cell corner: cells (0,0) and (1,1)
    both += [_rel(xb, yb) + (59, 0), _rel(xb + 1, yb + 1) + (59, 0)]
    _, _, _, _, c1b, _ = C[2]
    xc = c1b - 4
    st.pair(xc + 1, yb, 60, 61, "a")           # anti-diagonal: cells (0,3) and (1,2)
    both += [_rel(xc + 1, yb) + (59, 0), _rel(xc, yb + 1) + (60, 0)]
    exp.append(("pair_across_cells", "fast", both))
    # dots in every quadrant of both octree roots: without them the first round leaves the
    # list as long as it was and DistributeOctTree stops with one keypoint per root
    for k, (x, y) in enumerate(((10, 10), (50, 10), (10, 55), (60, 58), (76, 10), (120, 10),
                                (76, 55), (120, 55))):
        st.dot(16 + x, 16 + y, 25 + k)
    return Case("pairs_across_cells", st, (500, 1.2, 1, 20, 7), ["pair_across_cells"], exp)


def _extremes_case(bg):
    """bg 0 with dots of 255 / bg 255 with dots of 0 (score 254), at the first and last
    detectable column and row of the level and of the inner cell borders.  96 x 80: 2 x 1 cells
    of 32 x 48 (ROIs of 48 rows: the unprefetched path; dw = 32)."""
    w, h = 96, 80
    st = StampImage(w, h, bg, 20, 7)
    g = cell_grid(w, h)
    assert (g["ncols"], g["nrows"], g["wcell"]) == (2, 1, 32)
    assert g["cells"][0][5] - g["cells"][0][3] == 48
    pts = [(19, 19), (w - 20, 19), (19, h - 20), (w - 20, h - 20)]
    c1 = g["cells"][0][4]
    pts += [(c1 - 4, 30), (c1 - 3, 36), (30, 19), (30, h - 20), (60, 40)]
    for p in pts:
        st.dot(*p, 255)
    # one pixel outside the detectable frame: never a keypoint
    out = [(18, 50), (w - 19, 50), (40, 18), (44, h - 19)]
    for p in out:
        st.dot(*p, 255)
    exp = [("extreme_score_254", "fast", [_rel(*p) + (254, 0) for p in pts]),
           ("position_edges", "nofast", [_rel(*p) for p in out])]
    cons = ["extreme_score_254", "position_edges", "rows_gt_40", "dw_le_32",
            "polarity_dark" if bg else "polarity_bright"]
    return Case(f"extremes_bg{bg}", st, (500, 1.2, 1, 20, 7), cons, exp)


def _crowded_case():
    """More than 64 corners in a cell (120 x 96: 2 x 2 cells of 44 x 32, dw = 44 > 32).
    cell 0: 41 tied horizontal pairs (82 corners, none survives) and one dot of 30 placed last in
            raster order: the only ini keypoint is corner 83;
    cell 1: exactly 64 corners: 31 tied pairs + one (50, 51) pair, the survivor is corner 64;
    cell 2: exactly 65 corners: 32 tied pairs + one dot, the survivor is corner 65;
    cell 3: 35 tied pairs above ini (70 corners) and two sub-ini dots: the fallback returns the
            two dots although the first pass saw more than 64 corners."""
    w, h = 120, 96
    st = StampImage(w, h, 0, 20, 7)
    g = cell_grid(w, h)
    assert (g["ncols"], g["nrows"], g["wcell"], g["hcell"]) == (2, 2, 44, 32)
    exp = []

    def fill(cell, npairs):
        _, _, c0, r0, c1, r1 = g["cells"][cell]
        xs = list(range(c0 + 3, c1 - 9, 5))
        ys = list(range(r0 + 3, r1 - 3, 4))
        slots = [(x, y) for y in ys for x in xs]
        assert npairs < len(slots), (npairs, len(slots))
        tied = []
        for x, y in slots[:npairs]:
            st.pair(x, y, 40, 40, "h")
            tied += [_rel(x, y), _rel(x + 1, y)]
        return slots[npairs:], tied

    free, tied = fill(0, 41)
    st.dot(*free[-1], 30)
    exp.append(("ini_keypoint_is_corner_65_plus", "fast", [_rel(*free[-1]) + (29, 0)]))
    exp.append(("ini_keypoint_is_corner_65_plus", "nofast", tied))
    exp.append(("ini_keypoint_is_corner_65_plus", "cell_corners", (0, 83)))
    free, tied = fill(1, 31)
    x, y = free[0]
    st.pair(x, y, 50, 51, "h")
    exp.append(("cell_of_64_corners", "fast", [_rel(x + 1, y) + (50, 0)]))
    exp.append(("cell_of_64_corners", "cell_corners", (1, 64)))
    free, tied = fill(2, 32)
    st.dot(*free[0], 30)
    exp.append(("cell_of_65_corners", "fast", [_rel(*free[0]) + (29, 0)]))
    exp.append(("cell_of_65_corners", "cell_corners", (2, 65)))
    free, tied = fill(3, 35)
    st.dot(*free[0], 15)
    st.dot(*free[-1], 9)
    exp.append(("fallback_after_65_corners", "fast", [_rel(*free[0]) + (14, 1),
                                                      _rel(*free[-1]) + (8, 1)]))
    exp.append(("fallback_after_65_corners", "nofast", tied))
    exp.append(("fallback_after_65_corners", "cell_corners", (3, 70)))
    cons = ["ini_keypoint_is_corner_65_plus", "cell_of_64_corners", "cell_of_65_corners",
            "fallback_after_65_corners", "dw_gt_32"]
    return Case("crowded_cells", st, (500, 1.2, 1, 20, 7), cons, exp)


def dot_field(w, h, pitch, seed, nfeatures, lo=21, hi=119, keep=1.0, t=(20, 7), levels=1,
              jitter=0, region=None):
    """Dots of random amplitude in [lo, hi] on a square grid of `pitch` (>= 4; jitter moves a dot
    by up to `jitter` pixels, pitch - 2 jitter >= 4), each kept with probability `keep`, inside
    `region` = (x0, y0, x1, y1) in image coordinates (default: the detectable frame)."""
    assert pitch - 2 * jitter >= 4
    rng = np.random.default_rng(seed)
    st = StampImage(w, h, 0, *t)
    x0, y0, x1, y1 = region or (19, 19, w - 20, h - 20)
    for y in range(y0 + jitter, y1 - jitter + 1, pitch):
        for x in range(x0 + jitter, x1 - jitter + 1, pitch):
            a = int(rng.integers(lo, hi + 1))
            jx, jy = (int(v) for v in rng.integers(-jitter, jitter + 1, 2)) if jitter else (0, 0)
            if rng.random() < keep:
                st.dot(x + jx, y + jy, a)
    return st


def _octree_cases():
    out = []
    P = lambda nf, t=(20, 7), nl=1: (nf, 1.2, nl, t[0], t[1])
    # --- roots ---
    # 96 x 80: one root of 64 x 48.  N = 1: the root's quadrants are the final nodes.  Equal
    # maximal responses in the upper right quadrant (x >= 32, y < 24): A in the right-hand cell
    # (x >= 35) on a higher row, B in the left-hand cell (x = 32..34) on a lower row: B comes
    # first in candidate (cell-major) order, A in raster order.  And two equal dots inside one
    # cell in the lower left quadrant, with a weaker one between them in raster order.
    st = StampImage(96, 80, 0, 20, 7)
    st.dot(16 + 36, 16 + 5, 90).dot(16 + 33, 16 + 10, 90).dot(16 + 40, 16 + 16, 50)
    st.dot(16 + 6, 16 + 30, 70).dot(16 + 12, 16 + 34, 40).dot(16 + 6, 16 + 40, 70)
    st.dot(16 + 50, 16 + 40, 33)
    # (the list order: children are pushed to the front, so n4 .. n1)
    exp = [("best_tie_cell_major", "octree", [(50, 40, 32.0), (6, 30, 69.0), (33, 10, 89.0)])]
    out.append(Case("roots1_best_ties", st, P(1), ["n_ini_1", "best_tie_cell_major",
                                                   "best_tie_in_cell", "quota_1", "end_S_gt_N"],
                    exp))
    # a single candidate: a node of one key, N larger than the candidate count
    st = StampImage(96, 80, 0, 20, 7).dot(40, 40, 100)
    out.append(Case("one_key", st, P(500), ["node_of_one_key", "N_above_candidates"],
                    [("node_of_one_key", "octree", [(24, 24, 99.0)])]))
    # 240 x 96: three roots, hX = 208 / 3 = 69.33: x = 69 is the last column of root 0, x = 70
    # the first of root 1 (both rounded ends), root 1 empty otherwise in "roots3_gap"
    st = StampImage(240, 96, 0, 20, 7)
    for x, y, a in ((69, 10, 60), (69, 30, 61), (138, 12, 62), (139, 40, 63), (150, 20, 64),
                    (10, 10, 65), (200, 50, 66)):
        st.dot(16 + x, 16 + y, a)
    out.append(Case("roots3_edges", st, P(500),
                    ["n_ini_3", "root_last_first_column", "end_S_eq_prevS"],
                    [("root_last_first_column", "octree_roots", None)]))
    st = StampImage(240, 96, 0, 20, 7)
    for x, y, a in ((5, 5, 60), (60, 40, 61), (69, 20, 62), (139, 12, 63), (190, 40, 64),
                    (160, 50, 65)):
        st.dot(16 + x, 16 + y, a)
    out.append(Case("roots3_gap", st, P(500), ["empty_root_between"],
                    [("empty_root_between", "octree_roots_dropped", 1)]))
    # 164 x 96: two roots of 66 x 64
    out.append(Case("roots2_field", dot_field(164, 96, 7, 3, 40), P(40),
                    ["n_ini_2", "phase2_switch", "small_list", "seq_ties", "rank_sort_ncap_lt_nt"]))
    # --- splits and termination ---
    # all keys in one quadrant for several rounds (a tight cluster in the lower right corner),
    # keys exactly on split lines of even and odd rectangles: 96 x 80 root 64 x 48 splits at
    # (32, 24), then 16 / 12 wide, then 8 / 6, 4 / 3 (odd), ...
    st = StampImage(96, 80, 0, 20, 7)
    for x, y, a in ((32, 24, 50), (32, 4, 51), (4, 24, 52), (48, 36, 53), (56, 42, 54),
                    (60, 38, 55), (52, 44, 56), (59, 30, 57), (48, 12, 58), (16, 36, 59),
                    (40, 30, 60), (36, 40, 61)):
        st.dot(16 + x, 16 + y, a)
    out.append(Case("split_lines", st, P(500), ["keys_on_split_x", "keys_on_split_y"]))
    # the same on rectangles of odd size: 129 x 97, a root of 97 x 65 splits at (49, 33), its
    # right half (48 x 33) at y = 17, its lower left quarter (49 x 32) at x = 25
    st = StampImage(129, 97, 0, 20, 7)
    for x, y, a in ((49, 10, 50), (20, 33, 51), (49, 33, 52), (70, 17, 53), (90, 8, 54),
                    (25, 50, 55), (10, 40, 56), (80, 50, 57), (60, 25, 58), (10, 10, 59),
                    (35, 20, 60)):
        st.dot(16 + x, 16 + y, a)
    out.append(Case("split_lines_odd", st, P(500), ["keys_on_odd_split"]))
    st = StampImage(96, 80, 0, 20, 7)
    for k, (x, y) in enumerate(((52, 36), (56, 36), (52, 40), (56, 40), (60, 44))):
        st.dot(16 + x, 16 + y, 50 + k)
    # one node, all keys in one quadrant: the list is as long as before (1), so the loop stops
    # although the node could be split further: one keypoint for five candidates
    out.append(Case("stall", st, P(500), ["stop_while_expandable"]))
    # the same while other nodes keep the list growing: (49, 43) and (53, 43) share a quadrant
    # of the root's (32, 24, 64, 48) and of its (48, 36, 64, 48), and part in (48, 42, 56, 48)
    st = StampImage(96, 80, 0, 20, 7)
    for k, (x, y) in enumerate(((49, 43), (53, 43), (4, 4), (12, 4), (4, 12), (12, 12))):
        st.dot(16 + x, 16 + y, 50 + k)
    out.append(Case("one_quadrant", st, P(500), ["one_quadrant_rounds"]))
    # quota 0: nfeatures = 0 (the reference still runs one round of splits)
    out.append(Case("quota_0", dot_field(96, 80, 9, 5, 0), P(0), ["quota_0"]))
    return out


def _search_cases():
    """Dot fields whose octree runs were picked by scanning seeds and quotas with
    octree_reference's events (tools are the functions above); the census in
    tests/test_extract_cases.py asserts the events each one is listed for."""
    P = lambda nf, t=(20, 7), nl=1: (nf, 1.2, nl, t[0], t[1])
    out = []
    for name, kw, nf, cons in SEARCHED:
        out.append(Case(name, dot_field(nfeatures=nf, **kw), P(nf), cons))
    return out


# (name, dot_field arguments, nfeatures, constructs).  Found with scan_octree below; every
# listed construct is asserted from the run's events by the census.  The 320 x 240 fields at
# pitch 4 hold about 3000 candidates (the global-scratch path of large batches) and more than
# 256 expandable nodes when phase 2 begins; their quotas put the cut of the sorted list at
# the end of a chunk of 128 / 256 threads' worth of nodes, or one past it.
_F1 = dict(w=320, h=240, pitch=4, seed=1, keep=0.9)
_F2 = dict(w=320, h=240, pitch=4, seed=2, keep=0.85)
_F3 = dict(w=164, h=96, pitch=4, seed=3, keep=0.7)
_F4 = dict(w=200, h=150, pitch=4, seed=0, keep=1.0)
SEARCHED = [
    ("cut_128_end_eq_n", _F2, 1373, ["cut_at_128", "end_S_eq_N", "expandable_above_nt",
                                     "bucket_sort", "seq_tie_at_cut"]),
    ("cut_129", _F2, 1374, ["cut_past_128"]),
    ("cut_256", _F1, 1756, ["cut_at_256", "expandable_above_nt", "bucket_sort"]),
    ("cut_257", _F1, 1759, ["cut_past_256"]),
    ("margin_0", _F3, 128, ["switch_margin_0", "rank_sort_ncap_lt_nt"]),
    ("margin_1", _F3, 127, ["switch_margin_1"]),
    ("end_eq_n_phase1", _F3, 32, ["end_S_eq_N_phase1"]),
    ("big_nodes", _F4, 20, ["big_nodes_distinct", "big_nodes_equal"]),
    ("cross_512", _F4, 1700, ["list_crosses_512_phase1", "N_above_candidates"]),
]


def _orientation_cases():
    out = []
    t = (100, 60)
    P = (500, 1.2, 1, 100, 60)
    # exact moments around isolated dots (bg 0, ballast <= 60): 320 x 240, dots 40 apart
    st = StampImage(320, 240, 0, *t)
    plan = {
        "zero": [],
        "axis_0": [(5, 0, 10)], "axis_90": [(0, 5, 10)], "axis_180": [(-5, 0, 10)],
        "axis_270": [(0, -5, 10)],
        "diag_45": [(6, 6, 9)], "diag_135": [(-6, 6, 9)], "diag_225": [(-6, -6, 9)],
        "diag_315": [(6, -6, 9)],
        "cancel": [(7, 3, 20), (-7, -3, 20)],                       # m10 = m01 = 0 with ballast
        "huge_tiny": [(15, 0, 60), (14, 1, 60), (14, -1, 60), (13, 0, 60), (0, 4, 1)],
        "tiny_huge": [(0, 15, 60), (1, 14, 60), (-1, 14, 60), (0, 13, 60), (-4, 0, 1)],
    }
    spots = [(30 + 40 * i, 30 + 37 * j) for j in range(6) for i in range(7)]
    moms = {}
    for (name, bl), (x, y) in zip(plan.items(), spots):
        st.dot(x, y, 200)
        for u, v, b in bl:
            st.ballast(x + u, y + v, b)
        moms[name] = (_rel(x, y), (sum(u * b for u, v, b in bl), sum(v * b for u, v, b in bl)))
    out.append(Case("moments_exact", st, P, ["m10_m01_zero", "axis_angles", "diagonal_angles",
                                             "huge_beside_tiny"],
                    [("planted_moments", "moments", moms)]))
    # the umax circle: for every |v| a keypoint with ballast at u = s * umax[|v|] (inside) and
    # its twin with one more ballast pixel one further out, which must not change the angle;
    # a fixed off-axis ballast pixel makes the angle generic.  s = +1 / v > 0 in one image,
    # s = -1 / v < 0 in the other.  Dots 33 apart: x mod 16 and y mod 4 take every value.
    for s in (1, -1):
        st = StampImage(320, 240, 0, *t)
        spots = [(20 + 33 * i, 21 + 33 * j) for j in range(6) for i in range(8)]
        assert len({x % 16 for x, _ in spots}) == 8 and len({y % 4 for _, y in spots}) == 4
        twins = []
        k = 0
        for v in range(16):
            d = UMAX[v]
            for twin in (0, 1):
                x, y = spots[k]
                k += 1
                st.dot(x, y, 200)
                st.ballast(x - 4 * s, y - 6 * s, 31)
                st.ballast(x + s * d, y + s * v, 50)
                if twin and d + 1 <= 16:
                    st.ballast(x + s * (d + 1), y + s * v, 60)
                twins.append(_rel(x, y))
        out.append(Case(f"umax_circle_{'pos' if s > 0 else 'neg'}", st, P,
                        ["umax_edge", "x_mod_16_y_mod_4"],
                        [("umax_edge", "twins", twins)]))
    # every x mod 16 and y mod 4, and the extreme coordinates of the level (129 x 97)
    st = StampImage(129, 97, 0, *t)
    w, h = 129, 97
    pts = [(19, 19), (w - 20, 19), (19, h - 20), (w - 20, h - 20)]
    pts += [(32 + i + 16 * (i % 4), 24 + 3 * i) for i in range(16)]
    for n, (x, y) in enumerate(pts):
        st.dot(x, y, 150 + n)
    for n, (x, y) in enumerate(pts[:4]):
        for u, v, b in ((15, 0, 40), (-15, 1, 30), (3, 15, 50), (-2, -15, 45)):
            if (x + u, y + v) not in st._owner and 0 <= x + u < w and 0 <= y + v < h:
                st.ballast(x + u, y + v, b)
    assert {x % 16 for x, _ in pts} == set(range(16)) and {y % 4 for _, y in pts} == set(range(4))
    out.append(Case("coords_extreme", st, (500, 1.2, 1, 100, 60),
                    ["x_mod_16_all", "extreme_coordinates"]))
    # level counts 1, 2, 7, 8, 9, 31, 32, 33: that many isolated dots (all survive the octree)
    for n in (1, 2, 7, 8, 9, 31, 32, 33):
        st = StampImage(160, 96, 0, *t)
        rng = np.random.default_rng(100 + n)
        spots = [(20 + 11 * i, 20 + 9 * j) for j in range(7) for i in range(11)]
        for q in rng.permutation(len(spots))[:n]:
            x, y = spots[q]
            st.dot(x, y, int(rng.integers(101, 256)))
            st.ballast(x + 4 + int(rng.integers(0, 3)), y - 4, int(rng.integers(1, 61)))
        out.append(Case(f"count_{n}", st, (500, 1.2, 1, 100, 60), [f"level_count_{n}"],
                        [(f"level_count_{n}", "count", n)]))
    return out


def textured(seed, w, h):
    """Blocks and noise: the multi-level cases' one image without a closed-form prediction."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 110.0)
    for _ in range(w * h // 50):
        x, y = rng.integers(0, w), rng.integers(0, h)
        img[y:y + rng.integers(2, 9), x:x + rng.integers(2, 9)] = rng.uniform(0, 255)
    img += rng.normal(0, 3.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# The oracle's keypoint count of every case, measured on the CPU (tests/test_extract_cases.py
# keeps it equal; the GPU tests assert it before they compare, so an empty result cannot pass;
# thresholds_255_255 has no corner by construction: nothing is brighter than v + 255).
FLOORS = {
    "thresholds_20_7_bright": 16, "thresholds_20_7_dark": 16, "thresholds_20_20": 16,
    "thresholds_1_0": 8, "thresholds_0_0": 4, "thresholds_254_253": 12, "thresholds_255_255": 0,
    "pairs": 12, "pairs_across_cells": 14, "split_lines_odd": 11, "stall": 1,
    "extremes_bg0": 9, "extremes_bg255": 9, "crowded_cells": 5,
    "roots1_best_ties": 3, "one_key": 1, "roots3_edges": 7, "roots3_gap": 6, "roots2_field": 41,
    "split_lines": 12, "one_quadrant": 6, "quota_0": 4, "cut_128_end_eq_n": 1373,
    "cut_129": 1376, "cut_256": 1758, "cut_257": 1761, "margin_0": 128, "margin_1": 128,
    "end_eq_n_phase1": 32, "big_nodes": 22, "cross_512": 1148,
    "moments_exact": 12, "umax_circle_pos": 32, "umax_circle_neg": 32, "coords_extreme": 20,
    "count_1": 1, "count_2": 2, "count_7": 7, "count_8": 8, "count_9": 9, "count_31": 31,
    "count_32": 32, "count_33": 33, "pairs_L3": 19, "pairs_L8": 19, "crowded_cells_L3": 25,
    "crowded_cells_L8": 25, "moments_exact_L3": 28, "moments_exact_L8": 28, "textured_L3": 303,
    "textured_L8": 308, "quota_0_last_level": 12, "thresholds_300_m5": 8,
}

_CASES = None


def cases():
    """The table, built once (the images are read-only)."""
    global _CASES
    if _CASES is None:
        cs = []
        # threshold pairs: (20, 7), (20, 20), (1, 0), (0, 0), (254, 253), (255, 255)
        cs.append(_threshold_case("thresholds_20_7_bright", 0, 20, 7))
        cs.append(_threshold_case("thresholds_20_7_dark", 255, 20, 7))
        cs.append(_threshold_case("thresholds_20_20", 0, 20, 20))
        cs.append(_threshold_case("thresholds_1_0", 255, 1, 0))
        cs.append(_threshold_case("thresholds_0_0", 0, 0, 0))
        cs.append(_threshold_case("thresholds_254_253", 0, 254, 253))
        cs.append(_threshold_case("thresholds_255_255", 255, 255, 255))
        # outside [0, 255]: orbx_extractor_create accepts them and both sides clamp like cv::FAST
        cs.append(_threshold_case("thresholds_300_m5", 0, 255, 0, passed=(300, -5)))
        cs.append(_pairs_case())
        cs.append(_pairs_across_cells_case())
        cs.append(_extremes_case(0))
        cs.append(_extremes_case(255))
        cs.append(_crowded_case())
        cs += _octree_cases()
        cs += _search_cases()
        cs += _orientation_cases()
        # multi-level: the stamp images again with 3 and 8 levels, and one textured image
        base = {c.name: c for c in cs}
        for name in ("pairs", "crowded_cells", "moments_exact"):
            b = base[name]
            for nl in (3, 8):
                cs.append(Case(f"{name}_L{nl}", b.st, (b.params[0], 1.2, nl) + b.params[3:],
                               [f"nlevels_{nl}"]))
        for nl in (3, 8):
            cs.append(Case(f"textured_L{nl}", None, (300, 1.2, nl, 20, 7),
                           [f"nlevels_{nl}", "textured"], img=textured(11, 320, 240)))
        # nfeatures = 2 on 3 levels gives the quotas 1, 1, 0 (the last level takes what the
        # rounded others leave): the last level still keeps the nodes of its first round
        cs.append(Case("quota_0_last_level", None, (2, 1.2, 3, 20, 7), ["quota_0_level"],
                       img=textured(11, 320, 240)))
        for c in cs:
            c.img.setflags(write=False)
        assert len({c.name for c in cs}) == len(cs)
        _CASES = cs
    return _CASES


def scan_octree(w, h, pitches=(4, 5, 7, 9), seeds=range(4), quotas=(20, 60, 130, 300, 700, 1500),
                keep=(1.0, 0.6)):
    """How SEARCHED was found: yields (arguments, nfeatures, events) over a grid of dot fields,
    to pick runs that take an event (a cut at a multiple of the thread count, a switch margin
    of exactly 1, two nodes of equal size >= 63, ...)."""
    for p in pitches:
        for s in seeds:
            for kp in keep:
                for nf in quotas:
                    st = dot_field(w, h, p, s, nf, keep=kp)
                    cands, _ = predict_fast(st.corners, w, h, 20, 7)
                    ev = {}
                    octree_reference(cands, 16, w - 16, 16, h - 16, nf, events=ev)
                    yield (w, h, p, s, kp), nf, len(cands), ev
