"""CPU checks of the ORBmatcher restatement (oracle/orb_matcher_oracle.cpp).

The reference ships no matcher fixtures and cannot be built here, so the C++ restatement is
cross-checked against a second, independent reading of src/ORBmatcher.cc written below in
plain Python (small sizes), plus known answers for ComputeThreeMaxima and the grid.  Also
checks the product's host-side grid / FeatureVector builders against the oracle.
"""
from __future__ import annotations

import numpy as np
import pytest

from my_orb_slam2_amd import synth
from my_orb_slam2_amd.features import (PROJ_FRAME_MAPPOINTS, PROJ_FUSE, PROJ_FUSE_SCW,
                                       PROJ_KEYFRAME, PROJ_KF_SCW, PROJ_LAST_FRAME, PROJ_SIM3,
                                       assign_features_to_grid, feature_vector)
from oracle import matcher as om

f32 = np.float32


def hd(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def rot_bin(a1, a2):
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    v = float(f32(rot * f32(f32(1.0) / f32(30))))
    b = int(np.floor(v + 0.5))   # round half away (v >= 0)
    return 0 if b == 30 else b


def three_maxima_py(counts):
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(counts):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            i3, i2, i1 = i2, i1, i
        elif s > max2:
            max3, max2 = max2, s
            i3, i2 = i2, i
        elif s > max3:
            max3, i3 = s, i
    if max2 < f32(0.1) * f32(max1):
        i2 = i3 = -1
    elif max3 < f32(0.1) * f32(max1):
        i3 = -1
    return i1, i2, i3


@pytest.mark.parametrize("counts,expect", [
    ([0] * 30, (-1, -1, -1)),
    ([5] + [0] * 29, (0, -1, -1)),
    ([1, 2, 3] + [0] * 27, (2, 1, 0)),
    ([100, 9, 10] + [0] * 27, (0, 2, -1)),     # 9 < 0.1*100 drops the third
    ([100, 5, 3] + [0] * 27, (0, -1, -1)),     # second below 10%: both dropped
    ([4, 4, 4, 4] + [0] * 26, (0, 1, 2)),      # ties keep the first bins (strict >)
])
def test_three_maxima_kat(counts, expect):
    assert om.three_maxima(counts) == expect
    assert three_maxima_py(counts) == expect


def test_three_maxima_random():
    rng = np.random.default_rng(3)
    for _ in range(300):
        c = rng.integers(0, 20, 30) * (rng.random(30) < 0.3)
        assert om.three_maxima(c) == three_maxima_py(list(c))


def test_grid_matches_oracle():
    for seed in range(4):
        f1, _, _ = synth.feature_pair(seed, n1=600, n2=10)
        g = f1.grid
        off, feat = om.assign_grid(f1.keys, g.min_x, g.min_y, g.inv_w, g.inv_h)
        np.testing.assert_array_equal(off, g.off)
        np.testing.assert_array_equal(feat, g.feat)


def test_grid_rounding_edges():
    # PosInGrid uses std::round (half away from zero): x exactly on a half cell
    from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
    k = np.zeros(6, KEYPOINT_DTYPE)
    k["x"] = [0.0, 5.875, 5.874, 751.99, -0.1, -5.875]
    k["y"] = [0.0, 5.0, 5.0, 479.9, 3.0, 3.0]
    g = assign_features_to_grid(k, 0.0, 752.0, 0.0, 480.0)
    off, feat = om.assign_grid(k, g.min_x, g.min_y, g.inv_w, g.inv_h)
    np.testing.assert_array_equal(off, g.off)
    np.testing.assert_array_equal(feat, g.feat)


def test_feature_vector_layout():
    fv = feature_vector(np.array([7, 3, 7, -1, 3, 11]))
    np.testing.assert_array_equal(fv.node_id, [3, 7, 11])
    np.testing.assert_array_equal(fv.off, [0, 2, 4, 5])
    np.testing.assert_array_equal(fv.feat, [1, 4, 0, 2, 5])


# ---- independent restatements (plain Python) ----------------------------------------------

def nodes(fs):
    return {int(fs.fvec.node_id[j]): [int(i) for i in fs.fvec.feat[fs.fvec.off[j]:fs.fvec.off[j + 1]]]
            for j in range(len(fs.fvec.node_id))}


def bow_py(a, va, b, vb, kf_kf, ratio, check_ori):
    """SearchByBoW, both flavours (:182-319, :563-696) -> (nmatches, matches, codes): matches
    per B feature (KF-F) or per A feature (KF-KF); codes: the outcome of every A feature
    (tests/matcher_cases.py lists them; "+rescan": its static best or second was claimed)."""
    match = [-1] * (a.n if kf_kf else b.n)
    taken = [False] * b.n
    codes = ["skipped"] * a.n
    hist = [[] for _ in range(30)]
    n = 0
    bn = nodes(b)
    for nid, la in sorted(nodes(a).items()):
        if nid not in bn:
            continue
        for ia in la:
            if not va[ia]:
                continue
            b1, b2, bi = 256, 256, -1
            static = []
            for jb in bn[nid]:
                if kf_kf and not vb[jb]:
                    continue
                d = hd(a.desc[ia], b.desc[jb])
                static.append((d, jb))
                if taken[jb]:
                    continue
                if d < b1:
                    b2, b1, bi = b1, d, jb
                elif d < b2:
                    b2 = d
            static.sort(key=lambda t: t[0])   # stable: the lower position first among equals
            sfx = "+rescan" if any(taken[j] for _, j in static[:2]) else ""
            if bi < 0:
                codes[ia] = "no_candidate" + sfx
            elif not (b1 < 50 if kf_kf else b1 <= 50):
                codes[ia] = "over_threshold" + sfx
            elif not f32(b1) < f32(ratio) * f32(b2):
                codes[ia] = "ratio_rejected" + sfx
            else:
                codes[ia] = "accepted" + sfx
                taken[bi] = True
                match[ia if kf_kf else bi] = bi if kf_kf else ia
                if check_ori:
                    hist[rot_bin(a.keys["angle"][ia], b.keys["angle"][bi])].append(
                        (ia if kf_kf else bi, ia))
                n += 1
    if check_ori:
        t = three_maxima_py([len(h) for h in hist])
        for k in range(30):
            if k not in t:
                for j, ia in hist[k]:
                    match[j] = -1
                    codes[ia] = "rotation_removed"
                    n -= 1
    return n, np.array(match, np.int32), codes


def bow_kf_frame_py(kf, valid, f, ratio, check_ori):
    return bow_py(kf, valid, f, None, False, ratio, check_ori)[:2]


def epi_ok(kp1, kp2, F, sigma2):
    a = f32(f32(f32(kp1["x"]) * F[0]) + f32(f32(kp1["y"]) * F[3])) + F[6]
    b = f32(f32(f32(kp1["x"]) * F[1]) + f32(f32(kp1["y"]) * F[4])) + F[7]
    c = f32(f32(f32(kp1["x"]) * F[2]) + f32(f32(kp1["y"]) * F[5])) + F[8]
    a, b, c = f32(a), f32(b), f32(c)
    num = f32(f32(f32(a * f32(kp2["x"])) + f32(b * f32(kp2["y"]))) + c)
    den = f32(f32(a * a) + f32(b * b))
    if den == 0:
        return False
    dsqr = f32(f32(num * num) / den)
    return float(dsqr) < 3.84 * float(sigma2[kp2["octave"]])


def triangulation_py(k1, h1, k2, h2, F, ex, ey, sigma2, scale, only_stereo, check_ori=False,
                     codes=None):
    """`codes` (a list of k1.n entries, filled in place): the outcome of every KF1 feature."""
    F = np.asarray(F, f32).reshape(9)
    out = {}
    if codes is None:
        codes = [None] * k1.n
    codes[:] = ["skipped"] * k1.n
    n2 = nodes(k2)
    for nid, l1 in sorted(nodes(k1).items()):
        if nid not in n2:
            continue
        for i1 in l1:
            if h1[i1]:
                continue
            s1 = k1.u_right[i1] >= 0
            if only_stereo and not s1:
                continue
            best, bi = 50, -1
            for i2 in n2[nid]:
                if h2[i2]:
                    continue
                s2 = k2.u_right[i2] >= 0
                if only_stereo and not s2:
                    continue
                d = hd(k1.desc[i1], k2.desc[i2])
                if d > 50 or d > best:
                    continue
                kp2 = k2.keys[i2]
                if not s1 and not s2:
                    dx, dy = f32(f32(ex) - kp2["x"]), f32(f32(ey) - kp2["y"])
                    if f32(f32(dx * dx) + f32(dy * dy)) < f32(f32(100) * scale[kp2["octave"]]):
                        continue
                if epi_ok(k1.keys[i1], kp2, F, sigma2):
                    best, bi = d, i2
            codes[i1] = "accepted" if bi >= 0 else "no_candidate"
            if bi >= 0:
                out[i1] = bi
    if check_ori:
        hist = [[] for _ in range(30)]
        for i1, bi in out.items():
            hist[rot_bin(k1.keys["angle"][i1], k2.keys["angle"][bi])].append(i1)
        t = three_maxima_py([len(h) for h in hist])
        for k in range(30):
            if k not in t:
                for i1 in hist[k]:
                    del out[i1]
                    codes[i1] = "rotation_removed"
    pairs = np.array(sorted(out.items()), np.int32).reshape(-1, 2)
    return len(pairs), pairs


def area_py(fs, x, y, r, minl, maxl):
    with np.errstate(all="ignore"):   # non-finite queries are part of the directed cases
        return _area_py(fs, x, y, r, minl, maxl)


def _area_py(fs, x, y, r, minl, maxl):
    g = fs.grid
    x, y, r = f32(x), f32(y), f32(r)
    # (int)floor(v) / (int)ceil(v) as x86-64 converts: INT_MIN for NaN and out-of-range values
    x86 = lambda v: int(v) if np.isfinite(v) and -2.0**31 <= v < 2.0**31 else -2**31
    fl = lambda v: x86(np.floor(v))
    ce = lambda v: x86(np.ceil(v))
    cx0 = max(0, fl(f32(f32(f32(x - f32(g.min_x)) - r) * f32(g.inv_w))))
    if cx0 >= g.cols:
        return []
    cx1 = min(g.cols - 1, ce(f32(f32(f32(x - f32(g.min_x)) + r) * f32(g.inv_w))))
    if cx1 < 0:
        return []
    cy0 = max(0, fl(f32(f32(f32(y - f32(g.min_y)) - r) * f32(g.inv_h))))
    if cy0 >= g.rows:
        return []
    cy1 = min(g.rows - 1, ce(f32(f32(f32(y - f32(g.min_y)) + r) * f32(g.inv_h))))
    if cy1 < 0:
        return []
    check = minl > 0 or maxl >= 0
    out = []
    for ix in range(cx0, cx1 + 1):
        for iy in range(cy0, cy1 + 1):
            c = ix * g.rows + iy
            for i in g.feat[g.off[c]:g.off[c + 1]]:
                kp = fs.keys[i]
                if check:
                    if kp["octave"] < minl:
                        continue
                    if maxl >= 0 and kp["octave"] > maxl:
                        continue
                if abs(f32(kp["x"] - x)) < r and abs(f32(kp["y"] - y)) < r:
                    out.append(int(i))
    return out


CLAIM_MODES = (PROJ_FRAME_MAPPOINTS, PROJ_KF_SCW, PROJ_LAST_FRAME, PROJ_KEYFRAME)
PROJ_TH = {PROJ_FRAME_MAPPOINTS: 100, PROJ_KF_SCW: 50, PROJ_LAST_FRAME: 100, PROJ_FUSE: 50,
           PROJ_FUSE_SCW: 50, PROJ_SIM3: 100}


def projection_py(mode, T, q, qdesc, claimed, ratio, check_ori, orb_dist=100, inv_sigma2=None,
                  qflags=None, prefilter=False, info=None):
    """The seven projection searches.  `info` (a dict, filled in place): "codes" = the outcome
    of every query ("+rescan": its static best was claimed by an earlier query of this call);
    "exhausted" = the claim-mode queries whose list of the 8 best static candidates was
    truncated and had fewer than two unclaimed entries left at their turn (the replay kernel
    then re-scans the window); "overwritten" = no-claim queries whose feature a later query
    took."""
    pre = [bool(c) for c in claimed] if claimed is not None and mode in CLAIM_MODES else [False] * T.n
    cl = list(pre)
    out = [-1] * len(q)
    codes = ["skipped"] * len(q)
    exhausted, overwritten, holder = [], [], {}
    qbin = {}
    hist = [[] for _ in range(30)]
    n = 0
    init256 = mode not in (PROJ_FUSE_SCW, PROJ_SIM3)
    for iq, qq in enumerate(q):
        if not qq["radius"] >= 0:
            continue
        if mode in (PROJ_FRAME_MAPPOINTS, PROJ_LAST_FRAME, PROJ_KEYFRAME):
            cand = area_py(T, qq["u"], qq["v"], qq["radius"], qq["min_level"], qq["max_level"])
        else:
            cand = area_py(T, qq["u"], qq["v"], qq["radius"], -1, -1)
        bd, bl, bd2, bl2, bi = (256 if init256 else 2**31 - 1), -1, 256, -1, -1
        static = []
        for i in cand:
            kp = T.keys[i]
            if mode in (PROJ_KF_SCW, PROJ_FUSE, PROJ_FUSE_SCW, PROJ_SIM3):
                if kp["octave"] < qq["pred_level"] - 1 or kp["octave"] > qq["pred_level"]:
                    continue
            if mode in (PROJ_FRAME_MAPPOINTS, PROJ_LAST_FRAME) and T.u_right[i] > 0:
                if abs(f32(qq["ur"] - T.u_right[i])) > qq["radius"]:
                    continue
            if mode == PROJ_FUSE:
                ex, ey = f32(qq["u"] - kp["x"]), f32(qq["v"] - kp["y"])
                if T.u_right[i] >= 0:
                    er = f32(qq["ur"] - T.u_right[i])
                    e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                    if float(f32(e2 * inv_sigma2[kp["octave"]])) > 7.8:
                        continue
                else:
                    e2 = f32(f32(ex * ex) + f32(ey * ey))
                    if float(f32(e2 * inv_sigma2[kp["octave"]])) > 5.99:
                        continue
            d = hd(qdesc[iq], T.desc[i])
            if not pre[i] and (d < 256 or not init256):
                static.append((d, i))
            if cl[i]:
                continue
            if d < bd:
                bd2, bl2, bd, bl, bi = bd, bl, d, int(kp["octave"]), i
            elif d < bd2:
                bd2, bl2 = d, int(kp["octave"])
        static.sort(key=lambda t: t[0])   # stable: visiting order among equal distances
        sfx = "+rescan" if static and cl[static[0][1]] else ""
        if mode in CLAIM_MODES and len(static) > 8 and sum(not cl[i] for _, i in static[:8]) < 2:
            exhausted.append(iq)
        th = orb_dist if mode == PROJ_KEYFRAME else PROJ_TH[mode]
        if bi < 0:
            codes[iq] = "no_candidate" + sfx
        elif bd > th:
            codes[iq] = "over_threshold" + sfx
        elif mode == PROJ_FRAME_MAPPOINTS and bl == bl2 and f32(bd) > f32(ratio) * f32(bd2):
            codes[iq] = "ratio_rejected" + sfx
        else:
            codes[iq] = "accepted" + sfx
            no_claim = qflags is not None and mode in (PROJ_FRAME_MAPPOINTS, PROJ_LAST_FRAME) \
                and qflags[iq] & 1
            if bi in holder:
                overwritten.append(holder.pop(bi))
            if mode in CLAIM_MODES and not no_claim:
                cl[bi] = True
            elif no_claim:
                holder[bi] = iq
            out[iq] = bi
            n += 1
            if check_ori and mode in (PROJ_LAST_FRAME, PROJ_KEYFRAME):
                qbin[iq] = rot_bin(qq["angle"], T.keys["angle"][bi])
                hist[qbin[iq]].append(bi)
    if check_ori and not prefilter and mode in (PROJ_LAST_FRAME, PROJ_KEYFRAME):
        t = three_maxima_py([len(h) for h in hist])
        for iq, b in qbin.items():
            if b not in t:
                out[iq] = -1
                codes[iq] = "rotation_removed"
                n -= 1
    if info is not None:
        info.update(codes=codes, exhausted=exhausted, overwritten=overwritten)
    return n, np.array(out, np.int32)


def sim3_py(k1, k2, qdesc1, q12, qdesc2, q21):
    """SearchBySim3 (:1158-1382): the two projection loops and the agreement check."""
    _, m1 = projection_py(PROJ_SIM3, k2, q12, qdesc1, None, 0.0, False)
    _, m2 = projection_py(PROJ_SIM3, k1, q21, qdesc2, None, 0.0, False)
    out = np.full(len(q12), -1, np.int32)
    for i1, i2 in enumerate(m1):
        if i2 >= 0 and i2 < len(m2) and m2[i2] == i1:
            out[i1] = i2
    return int((out >= 0).sum()), out


def initialization_py(f1, f2, prev, window, ratio, check_ori):
    """SearchForInitialization (:446-561) -> (nmatches, vnMatches12, codes); `prev` [n1, 2] is
    updated in place for the matched features."""
    INF = 2**31 - 1
    m12, m21, mdist = [-1] * f1.n, [-1] * f2.n, [INF] * f2.n
    codes = ["skipped"] * f1.n
    hist = [[] for _ in range(30)]
    n = 0
    for i1 in range(f1.n):
        lvl = int(f1.keys["octave"][i1])
        if lvl > 0:
            continue
        cand = area_py(f2, prev[i1][0], prev[i1][1], f32(window), lvl, lvl)
        bd, bd2, bi = INF, INF, -1
        static = (INF, -1)
        for i2 in cand:
            d = hd(f1.desc[i1], f2.desc[i2])
            if d < static[0]:
                static = (d, i2)
            if mdist[i2] <= d:
                continue
            if d < bd:
                bd2, bd, bi = bd, d, i2
            elif d < bd2:
                bd2 = d
        sfx = "+rescan" if static[1] >= 0 and mdist[static[1]] <= static[0] else ""
        if bi < 0:
            codes[i1] = "no_candidate" + sfx
        elif bd > 50:
            codes[i1] = "over_threshold" + sfx
        elif not f32(bd) < f32(f32(bd2) * f32(ratio)):
            codes[i1] = "ratio_rejected" + sfx
        else:
            codes[i1] = "accepted" + sfx
            if m21[bi] >= 0:
                m12[m21[bi]] = -1
                codes[m21[bi]] = "taken_over"
                n -= 1
            m12[i1], m21[bi], mdist[bi] = bi, i1, bd
            n += 1
            if check_ori:
                hist[rot_bin(f1.keys["angle"][i1], f2.keys["angle"][bi])].append(i1)
    if check_ori:
        t = three_maxima_py([len(h) for h in hist])
        for k in range(30):
            if k not in t:
                for i1 in hist[k]:
                    if m12[i1] >= 0:
                        m12[i1] = -1
                        codes[i1] = "rotation_removed"
                        n -= 1
    for i1 in range(f1.n):
        if m12[i1] >= 0:
            prev[i1][0] = f2.keys["x"][m12[i1]]
            prev[i1][1] = f2.keys["y"][m12[i1]]
    return n, np.array(m12, np.int32), codes


# ---- cross-checks ----------------------------------------------------------------------

@pytest.mark.parametrize("seed,check_ori,ratio,single", [(0, True, 0.75, False),
                                                         (1, False, 0.6, False),
                                                         (2, True, 0.7, True)])
def test_bow_kf_frame_crosscheck(seed, check_ori, ratio, single):
    f1, f2, _ = synth.feature_pair(seed, n1=160, n2=150, nodes=6, single_node=single)
    valid = np.random.default_rng(seed).random(f1.n) < 0.8
    n_o, m_o = om.search_by_bow_kf_frame(f1, valid, f2, ratio, check_ori)
    n_p, m_p = bow_kf_frame_py(f1, valid, f2, ratio, check_ori)
    assert n_o == n_p and n_o > 0
    np.testing.assert_array_equal(m_o, m_p)


@pytest.mark.parametrize("seed,only_stereo", [(0, False), (1, True), (2, False)])
def test_triangulation_crosscheck(seed, only_stereo):
    k1, k2, F, epi, _ = synth.keyframe_pair(seed, n1=220, n2=220, nodes=5, stereo_frac=0.4)
    rng = np.random.default_rng(seed + 10)
    h1, h2 = rng.random(k1.n) < 0.3, rng.random(k2.n) < 0.3
    s, s2, _ = synth.scale_tables()
    n_o, p_o = om.search_for_triangulation(k1, h1, k2, h2, F, epi, s2, s, only_stereo,
                                           check_ori=False)
    n_p, p_p = triangulation_py(k1, h1, k2, h2, F, epi[0], epi[1], s2, s, only_stereo)
    assert n_o == n_p and n_o > 0
    np.testing.assert_array_equal(p_o, p_p)


@pytest.mark.parametrize("mode", [PROJ_FRAME_MAPPOINTS, PROJ_KF_SCW, PROJ_LAST_FRAME,
                                  PROJ_KEYFRAME, PROJ_FUSE])
def test_projection_crosscheck(mode):
    f1, f2, t = synth.feature_pair(11 + mode, n1=150, n2=160, dup_frac=0.15)
    q, d = synth.projection_queries(5 + mode, f1, f2, t, th=6.0,
                                    mode_levels="frame" if mode in (0, 2, 3) else "kf")
    claimed = np.random.default_rng(mode).random(f2.n) < 0.1
    _, _, isg = synth.scale_tables()
    n_o, m_o = om.search_by_projection(mode, f2, q, d, claimed, isg, orb_dist=64, nnratio=0.8)
    n_p, m_p = projection_py(mode, f2, q, d, claimed, 0.8, True, orb_dist=64, inv_sigma2=isg)
    assert n_o == n_p and n_o > 0
    np.testing.assert_array_equal(m_o, m_p)


@pytest.mark.parametrize("mode,prefilter", [(PROJ_FRAME_MAPPOINTS, False),
                                            (PROJ_LAST_FRAME, True), (PROJ_KEYFRAME, True)])
def test_projection_ex_crosscheck(mode, prefilter):
    """orbx_search_by_projection_ex's per-query no-claim flag and the prefilter call flag."""
    f1, f2, t = synth.feature_pair(31 + mode, n1=150, n2=160, dup_frac=0.15)
    q, d = synth.projection_queries(9 + mode, f1, f2, t, th=12.0,
                                    mode_levels="frame" if mode in (0, 2, 3) else "kf")
    rng = np.random.default_rng(mode + 3)
    claimed = rng.random(f2.n) < 0.1
    qflags = (rng.random(len(q)) < 0.4).astype(np.uint8)
    q, d = np.concatenate([q[:40], q]), np.concatenate([d[:40], d])   # see test_gpu_match
    qflags = np.concatenate([np.ones(40, np.uint8), qflags])
    n_o, m_o = om.search_by_projection_ex(mode, f2, q, d, qflags, claimed, orb_dist=64,
                                          nnratio=0.8, prefilter=prefilter)
    n_p, m_p = projection_py(mode, f2, q, d, claimed, 0.8, True, orb_dist=64, qflags=qflags,
                             prefilter=prefilter)
    assert n_o == n_p and n_o > 0
    np.testing.assert_array_equal(m_o, m_p)
    if mode != PROJ_KEYFRAME:
        hit = m_o[m_o >= 0]
        assert len(np.unique(hit)) < len(hit)


def test_projection_ex_last_frame_no_claim_needs_prefilter():
    """LAST_FRAME + rotation check + a no-claim query without the prefilter: the oracle refuses
    (-1), as the C ABI does (ORBX_ERR_INVALID): the reference clears per feature
    (ORBmatcher.cc:1516-1535), which a per-query filter cannot reproduce."""
    f1, f2, t = synth.feature_pair(34, n1=150, n2=160, dup_frac=0.15)
    q, d = synth.projection_queries(12, f1, f2, t, th=12.0, mode_levels="frame")
    qflags = np.zeros(len(q), np.uint8)
    qflags[0] = 1
    n_o, _ = om.search_by_projection_ex(PROJ_LAST_FRAME, f2, q, d, qflags, orb_dist=64,
                                        nnratio=0.8, prefilter=False)
    assert n_o == -1
    n_o, _ = om.search_by_projection_ex(PROJ_LAST_FRAME, f2, q, d, qflags, orb_dist=64,
                                        nnratio=0.8, prefilter=False, check_ori=False)
    assert n_o >= 0


def _distinctive_case(seed, npts=60, maxn=40):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, maxn + 1, npts)
    sizes[:3] = [0, 1, 2]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    base = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    desc = np.repeat(base, sizes, axis=0)
    flips = rng.random(desc.shape) < 0.05   # observations of one point are similar
    desc = desc ^ (flips * rng.integers(1, 256, desc.shape)).astype(np.uint8)
    dup = rng.random(len(desc)) < 0.1       # repeated observations: median ties
    desc[1:][dup[1:]] = desc[:-1][dup[1:]]
    return desc, off


def distinctive_py(desc, off):
    out = []
    for p in range(len(off) - 1):
        rows = desc[off[p]:off[p + 1]]
        n = len(rows)
        if n == 0:
            out.append(-1)
            continue
        bits = np.unpackbits(rows, axis=1).astype(np.int32)
        D = (bits[:, None, :] != bits[None, :, :]).sum(2).tolist()
        best, bi = None, 0
        for i in range(n):
            med = sorted(D[i])[int(0.5 * (n - 1))]
            if best is None or med < best:
                best, bi = med, i
        out.append(bi)
    return np.array(out, np.int32)


def test_distinctive_descriptors_crosscheck():
    desc, off = _distinctive_case(1, npts=40, maxn=12)
    np.testing.assert_array_equal(om.distinctive_descriptors(desc, off), distinctive_py(desc, off))
